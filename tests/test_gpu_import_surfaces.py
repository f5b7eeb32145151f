"""efx_import_surfaces / efx_detect_crop_surfaces (k_import_surf*, k_crop_sums_surf*): NV12, P010 and pitched planar
4:2:0 pictures read where a decoder left them, bit for bit against the NumPy model of include/efx.h's definition
(tests/surface_model.py: the canonical I420 image, then the unmodified models of the packed formats)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import import_model as M
import surface_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def dec(efx):
    d = efx.Decoder(max_streams=16, max_pictures=4, ring_depth=5)
    yield d
    d.close()


def c_surface(efx, s):
    return efx._Surface(s.layout, s.shift, s.swap_uv, s.width, s.height, (C.c_size_t * 3)(*s.offset), (C.c_size_t * 3)(*s.pitch), s.bytes)


def upload_padded(dec, src, stride, gap=None):
    """Image i at i * stride; gap: the bytes between the images (and behind the last one), zeros when None."""
    n, size = src.shape
    host = np.zeros((n, stride), dtype=np.uint8)
    if gap is not None:
        host[:] = gap
    host[:, :size] = src
    buf = dec.alloc(n * stride)
    buf.upload(host)
    return buf


def run_import(efx, dec, src, s, crop=None, rect=None, stride=None, gap=None):
    n = len(src)
    stride = stride or (s.bytes + 15) // 16 * 16
    sbuf, dbuf = upload_padded(dec, src, stride, gap), dec.alloc(n * M.FRAME_BYTES)
    try:
        dec.import_to(sbuf, dbuf, n_images=n, fmt="i420", width=s.width, height=s.height, crop=crop, dst_rect=rect,
                      src_stride=stride, surface=c_surface(efx, s))
        dec.sync()
        return dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES)
    finally:
        sbuf.free()
        dbuf.free()


def run_detect(efx, dec, src, s, per, limit=24, rnd=16, stride=None, gap=None, surface=True):
    """(sums, records) from the device; surface=False: src holds packed I420 images for efx_detect_crop."""
    n, size = src.shape
    stride = stride or (size + 15) // 16 * 16
    w, h = s.width, s.height
    sums_stride = (h + w + 3) // 4 * 4
    sbuf, rbuf, ubuf = upload_padded(dec, src, stride, gap), dec.alloc(32 * (n // per)), dec.alloc(4 * n * sums_stride)
    try:
        dec.detect_crop_to(sbuf, rbuf, n_streams=n // per, images_per_stream=per, fmt="i420", width=w, height=h, limit=limit,
                           round=rnd, src_stride=stride, sums=ubuf, surface=c_surface(efx, s) if surface else None)
        dec.sync()
        sums = ubuf.download(np.uint32, n * sums_stride).reshape(n, sums_stride)[:, :h + w]
        return sums, rbuf.download(np.int32, 8 * (n // per)).reshape(n // per, 8)
    finally:
        for b in (sbuf, rbuf, ubuf):
            b.free()


def assert_same(got, want, what):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first (image, byte) = {bad[0].tolist()}"


@pytest.mark.parametrize("kind,w,h,pitch,rows,n,crop,rect", S.GEOMETRIES)
def test_geometry_matrix(efx, dec, kind, w, h, pitch, rows, n, crop, rect):
    s = S.layout(kind, w, h, pitch, rows)
    src = S.sources(n, s, w * 31 + h)
    got = run_import(efx, dec, src, s, crop, rect)
    assert_same(got, S.import_images(src, s, crop, rect), f"{kind} {w}x{h}")
    assert len({g.tobytes() for g in got}) == n
    sums, recs = run_detect(efx, dec, src, s, n)
    want_sums, want_recs = S.detect(src, s)
    assert np.array_equal(sums, want_sums) and np.array_equal(recs, want_recs)


EQUIVALENT = [g for g in S.GEOMETRIES if g[:3] in (("nv12", 34, 18), ("p010", 34, 18), ("i010", 354, 194))]


@pytest.mark.parametrize("kind,w,h,pitch,rows,n,crop,rect", EQUIVALENT)
def test_equivalence_on_the_device(efx, dec, kind, w, h, pitch, rows, n, crop, rect):
    """efx_import_surfaces against efx_import_frames fed the host-made canonical I420 images, and
    efx_detect_crop_surfaces against efx_detect_crop (records and sums) on letterboxed and pillarboxed content with a
    black level of 16 (64 << 6 as P010 keeps it)."""
    s = S.layout(kind, w, h, pitch, rows)
    src = S.sources(n, s, 77 + w)
    canon = S.canonicals(src, s)
    got = run_import(efx, dec, src, s, crop, rect)
    stride = (canon.shape[1] + 15) // 16 * 16
    sbuf, dbuf = upload_padded(dec, canon, stride), dec.alloc(n * M.FRAME_BYTES)
    dec.import_to(sbuf, dbuf, n_images=n, fmt="i420", width=w, height=h, crop=crop, dst_rect=rect, src_stride=stride)
    dec.sync()
    want = dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES)
    sbuf.free()
    dbuf.free()
    assert_same(got, want, f"{kind} against efx_import_frames")

    bx, by = 2 * (w // 8) + 1, 2 * (h // 8) + 1   # (odd borders: the rounding takes part)
    boxes = [(0, by, w, h - 2 * by), (bx, 0, w - 2 * bx, h)]
    src = np.concatenate([S.boxed(2, s, box, 5 + i) for i, box in enumerate(boxes)])
    sums, recs = run_detect(efx, dec, src, s, 2, rnd=2)
    csums, crecs = run_detect(efx, dec, S.canonicals(src, s), s, 2, rnd=2, surface=False)
    assert np.array_equal(sums, csums) and np.array_equal(recs, crecs)
    assert [tuple(r[4:]) for r in recs] == [(0, by, w - 1, h - by - 1), (bx, 0, w - bx - 1, h - 1)]
    assert np.array_equal(recs, S.detect(src, s, 2, 24, 2)[1])


@pytest.mark.parametrize("kind,pitch", [("nv12", 50), ("p010", 74), ("i010", 80), ("yv12", 38)])
def test_padding_is_never_used(efx, dec, kind, pitch):
    """The same call with two different random patterns in the pitch padding, the rows between height and plane_rows and
    the gap between images: identical outputs, the model's; and nothing outside the output images is written."""
    w, h, n, crop, rect = 34, 18, 3, (2, 2, 30, 14), (16, 8, 320, 160)
    s = S.layout(kind, w, h, pitch, 22)
    src = S.sources(n, s, 9)
    stride, dst_stride = (s.bytes + 15) // 16 * 16 + 48, M.FRAME_BYTES + 48
    want = S.import_images(src, s, crop, rect)
    want_sums, want_recs = S.detect(src, s)
    rng = np.random.default_rng(3)
    dbuf = dec.alloc((n + 1) * dst_stride)
    outs = []
    for seed in (1, 2):
        filled = S.refill_padding(src, s, seed)
        assert not np.array_equal(filled, src) and np.array_equal(S.canonicals(filled, s), S.canonicals(src, s))
        gap = rng.integers(0, 256, (n, stride), dtype=np.uint8)
        sbuf = upload_padded(dec, filled, stride, gap)
        dbuf.upload(np.full(dbuf.nbytes, 0xA5, dtype=np.uint8))
        dec.import_to(sbuf, dbuf, n_images=n, fmt="i420", width=w, height=h, crop=crop, dst_rect=rect, src_stride=stride,
                      dst_stride=dst_stride, surface=c_surface(efx, s))
        dec.sync()
        sbuf.free()
        raw = dbuf.download(np.uint8, dbuf.nbytes)
        for i in range(n):
            assert_same(raw[None, i * dst_stride:i * dst_stride + M.FRAME_BYTES], want[i][None], f"{kind} image {i}")
            assert (raw[i * dst_stride + M.FRAME_BYTES:(i + 1) * dst_stride] == 0xA5).all()
        assert (raw[n * dst_stride:] == 0xA5).all()
        outs.append(raw)
        sums, recs = run_detect(efx, dec, filled, s, n, stride=stride, gap=gap)
        assert np.array_equal(sums, want_sums) and np.array_equal(recs, want_recs)
    dbuf.free()
    assert np.array_equal(outs[0], outs[1])


def test_fields(efx, dec):
    """The bottom field of an NV12 68 x 36 surface -- every pitch doubled, the height halved, each offset one pitch on --
    is the import of the canonical image made from the odd rows."""
    s = S.layout("nv12", 68, 36, 80)
    src = S.sources(3, s, 12)
    for bottom in (1, 0):
        f = S.field_of(s, bottom)
        got = run_import(efx, dec, src, f)
        frames = S.canonicals(src, s)
        y = frames[:, :68 * 36].reshape(3, 36, 68)[:, bottom::2]
        cb = frames[:, 68 * 36:68 * 36 * 5 // 4].reshape(3, 18, 34)[:, bottom::2]
        cr = frames[:, 68 * 36 * 5 // 4:].reshape(3, 18, 34)[:, bottom::2]
        fields = np.concatenate([p.reshape(3, -1) for p in (y, cb, cr)], axis=1)
        assert_same(got, M.import_images(fields, "i420", 68, 18), f"field {bottom}")


def test_queued_calls_keep_their_geometry(efx, dec):
    """Two calls with different surfaces and rectangles queued back to back without a sync: each equals its model."""
    jobs = []
    for kind, w, h, pitch, crop, rect in (("p010", 354, 194, 720, (2, 2, 352, 192), None),
                                          ("nv21", 100, 50, 112, None, (0, 46, 352, 100))):
        s = S.layout(kind, w, h, pitch)
        src = S.sources(2, s, 40 + w)
        stride = (s.bytes + 15) // 16 * 16
        jobs.append((s, src, crop, rect, upload_padded(dec, src, stride), dec.alloc(2 * M.FRAME_BYTES)))
    for s, src, crop, rect, sbuf, dbuf in jobs:
        dec.import_to(sbuf, dbuf, n_images=2, fmt="i420", width=s.width, height=s.height, crop=crop, dst_rect=rect,
                      surface=c_surface(efx, s))
    dec.sync()
    for s, src, crop, rect, sbuf, dbuf in jobs:
        got = dbuf.download(np.uint8, 2 * M.FRAME_BYTES).reshape(2, M.FRAME_BYTES)
        assert_same(got, S.import_images(src, s, crop, rect), "queued")
        sbuf.free()
        dbuf.free()


def test_argument_errors(efx, dec):
    lib, ctx = dec._lib, dec._ctx
    good = S.layout("nv12", 34, 18, 50)
    src, dst, rects = dec.alloc(1 << 16), dec.alloc(2 * M.FRAME_BYTES), dec.alloc(64)
    I420, RGB24 = efx.PIX_I420, efx.PIX_RGB24

    def imp(s=good, fmt=I420, w=None, h=None, ss=0, sp=src.ptr):
        o = efx._ImportOpts(2, fmt, s.width if w is None else w, s.height if h is None else h, 0, 0, 0, 0, 0, 0, 0, 0, 0, ss, 0)
        return lib.efx_import_surfaces(ctx, C.byref(c_surface(efx, s)), C.byref(o), sp, dst.ptr)

    def det(s=good, fmt=I420, w=None, h=None, ss=0, sp=src.ptr):
        o = efx._CropOpts(1, 2, fmt, s.width if w is None else w, s.height if h is None else h, 0, 24, 16, ss, 0)
        return lib.efx_detect_crop_surfaces(ctx, C.byref(c_surface(efx, s)), C.byref(o), sp, rects.ptr, None)

    for call in (imp, det):
        assert call() == 0
        for what, bad in S.rejected_surfaces():
            assert call(s=bad) == ARG, (call.__name__, what, bad)
            assert lib.efx_last_error(ctx).startswith(b"efx_import_surfaces: " if call is imp else b"efx_detect_crop_surfaces: ")
        # the opts describe the canonical image
        assert call(fmt=RGB24) == ARG and call(fmt=3) == ARG and call(w=36) == ARG and call(h=20) == ARG and call(w=32) == ARG
        # src_stride: bytes between images
        size = good.bytes
        assert call(ss=size // 16 * 16) == ARG and call(ss=(size + 15) // 16 * 16 + 8) == ARG and call(ss=(size + 15) // 16 * 16 + 16) == 0
        assert call(sp=None) == ARG and call(sp=src.ptr + 8) == ARG
    assert lib.efx_import_surfaces(ctx, None, C.byref(efx._ImportOpts()), src.ptr, dst.ptr) == ARG
    assert lib.efx_detect_crop_surfaces(ctx, None, C.byref(efx._CropOpts()), src.ptr, rects.ptr, None) == ARG
    # the crop rules of the canonical I420 image
    o = efx._ImportOpts(2, I420, 34, 18, 1, 0, 16, 16, 0, 0, 0, 0, 0, 0, 0)
    assert lib.efx_import_surfaces(ctx, C.byref(c_surface(efx, good)), C.byref(o), src.ptr, dst.ptr) == ARG
    dec.sync()
    for b in (src, dst, rects):
        b.free()
    # a following valid call is correct
    data = S.sources(2, good, 1)
    assert_same(run_import(efx, dec, data, good), S.import_images(data, good), "after the errors")
    with pytest.raises(efx.EfxError) as e:
        dec.import_to(0, 0, n_images=1, fmt="i420", width=34, height=18, surface=c_surface(efx, good))
    assert e.value.status == ARG


def test_python_arrays(efx, dec):
    """import_pictures / detect_crop with kind strings on NumPy arrays: the model applied to the detected rectangle."""
    w, h, n, pitch, rows = 96, 64, 2, 224, 72
    s = S.layout("p010", w, h, pitch, rows)
    src = S.boxed(n, s, (0, 12, 96, 40), 31)
    recs = dec.detect_crop(src, fmt="p010", width=w, height=h, pitch=pitch, plane_rows=rows)
    want_recs = S.detect(src, s)[1]
    assert np.array_equal(recs, want_recs) and tuple(recs[0, :4]) == (0, 16, 96, 32)
    words = src.view(np.uint16)
    assert words.shape == (n, s.bytes // 2)
    crop = tuple(int(v) for v in want_recs[0, :4])
    want = S.import_images(src, s, crop, M.letterbox_rect(crop[2], crop[3]))
    for a in (src, words):
        got = dec.import_pictures(a, fmt="p010", width=w, height=h, pitch=pitch, plane_rows=rows, crop="auto", fit="letterbox")
        assert isinstance(got, np.ndarray)
        assert_same(got, want, "import_pictures p010")
    nv = S.layout("nv12", w, h, 128)
    src = S.boxed(n, nv, (20, 0, 56, 64), 32)
    assert np.array_equal(dec.detect_crop(src, fmt="nv12", width=w, height=h, pitch=128), S.detect(src, nv)[1])
    assert_same(dec.import_pictures(src, fmt="nv12", width=w, height=h, pitch=128, fit="cover"),
                S.import_images(src, nv, efx.cover_crop(w, h)), "import_pictures nv12 cover")
    # packed i420 stays on its old path; with a pitch it is a surface
    yuv = S.sources(n, S.layout("i420", w, h), 33)
    assert_same(dec.import_pictures(yuv, fmt="i420", width=w, height=h), M.import_images(yuv, "i420", w, h), "i420")
    pitched = S.layout("i420", w, h, 112)
    psrc = S.sources(n, pitched, 34)
    assert_same(dec.import_pictures(psrc, fmt="i420", width=w, height=h, pitch=112), S.import_images(psrc, pitched), "pitched i420")
    with pytest.raises(ValueError):
        dec.import_pictures(src, fmt="nv12", width=w, height=h)            # the shape is that of pitch 128
    with pytest.raises(ValueError):
        dec.import_pictures(src.view(np.uint16), fmt="nv12", width=w, height=h, pitch=128)
    with pytest.raises(ValueError):
        dec.import_pictures(src, fmt="nv12", pitch=128)
    with pytest.raises(ValueError):
        dec.import_pictures(src, fmt="nv12", width=w, height=h, pitch=64)


TORCH_CHILD = textwrap.dedent("""
    import os
    import sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
    import espflix_amd as efx
    import import_model as M
    import surface_model as S

    torch.cuda.set_stream(torch.cuda.Stream())
    dec = efx.Decoder(4, 2, device=torch.cuda.current_device(), hip_stream=torch.cuda.current_stream().cuda_stream)
    w, h, n, pitch, rows = 96, 64, 2, 224, 72
    s = S.layout("p010", w, h, pitch, rows)
    src = S.boxed(n, s, (0, 12, 96, 40), 31)
    crop = tuple(int(v) for v in S.detect(src, s)[1][0, :4])
    want = S.import_images(src, s, crop, M.letterbox_rect(crop[2], crop[3]))
    t = torch.from_numpy(src.view(np.uint16).copy()).cuda()       # (n, bytes / 2) uint16, queued on torch's stream
    assert t.dtype == torch.uint16 and tuple(t.shape) == (n, s.bytes // 2)
    kw = dict(fmt="p010", width=w, height=h, pitch=pitch, plane_rows=rows, crop="auto", fit="letterbox")
    got = dec.import_pictures(t, **kw)
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (n, 101376)
    assert np.array_equal(got.cpu().numpy(), want)
    out = torch.full((n * 101376,), 7, dtype=torch.uint8, device="cuda")
    got = dec.import_pictures(t.view(torch.uint8), out=out, sync=False, **kw)   # the same memory as bytes, no sync
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(dec.import_pictures(src, **kw), want)    # the array path
    assert np.array_equal(dec.detect_crop(t, fmt="p010", width=w, height=h, pitch=pitch, plane_rows=rows), S.detect(src, s)[1])
    dec.close()
    print("torch surfaces ok")
""")


def test_python_torch_tensor(efx, tmp_path):
    """In a child process (torch's HIP runtime must come up first): import_pictures(fmt="p010", crop="auto",
    fit="letterbox") on a uint16 torch tensor on the device and on a NumPy array: the model applied to the detected
    rectangle."""
    script = tmp_path / "torch_surfaces.py"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch surfaces ok" in r.stdout
