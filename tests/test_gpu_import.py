"""efx_import_frames (k_import): I420 / RGB24 / RGBP pictures of any size cropped, scaled and converted to 352 x 192 I420
on the device, bit for bit against the NumPy model of include/efx.h's formulas (tests/import_model.py)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import import_model as M

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


def sources(n, fmt, w, h, seed):
    """n pictures of distinct content: noise, two-level noise, a smooth ramp with noise in its low bits, ..."""
    rng = np.random.default_rng(seed)
    size = M.src_bytes(fmt, w, h)
    out = np.empty((n, size), dtype=np.uint8)
    for i in range(n):
        if i % 3 == 0:
            out[i] = rng.integers(0, 256, size, dtype=np.uint8)
        elif i % 3 == 1:
            out[i] = rng.integers(0, 2, size, dtype=np.uint8) * 255
        else:
            out[i] = (np.arange(size) * 7 // max(1, w) + rng.integers(0, 4, size)) & 0xFF
    return out


def upload_padded(dec, src, stride, fill=0):
    n, size = src.shape
    host = np.full((n, stride), fill, dtype=np.uint8)
    host[:, :size] = src
    buf = dec.alloc(n * stride)
    buf.upload(host)
    return buf


def run_import(dec, src, fmt, w, h, crop=None, rect=None, full=False):
    n, size = src.shape
    stride = (size + 15) // 16 * 16
    sbuf, dbuf = upload_padded(dec, src, stride), dec.alloc(n * M.FRAME_BYTES)
    try:
        dec.import_to(sbuf, dbuf, n_images=n, fmt=fmt, width=w, height=h, crop=crop, dst_rect=rect, full_range=full)
        dec.sync()
        return dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES)
    finally:
        sbuf.free()
        dbuf.free()


def assert_same(got, want, what):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first (image, byte) = {bad[0].tolist()}"


GEOMETRIES = [
    # fmt, width, height, images, crop, destination rectangle, full range
    ("rgbp", 2, 2, 3, None, None, False),
    ("i420", 16, 16, 3, None, None, False),
    ("rgb24", 333, 77, 3, None, None, False),
    ("rgb24", 333, 77, 3, None, None, True),
    ("i420", 354, 194, 3, None, None, False),
    ("rgb24", 704, 384, 3, None, None, False),
    ("rgb24", 1920, 1080, 3, None, None, False),
    ("i420", 4096, 2304, 1, None, None, False),
    ("rgb24", 30, 4094, 3, None, (160, 32, 30, 128), False),
    ("rgbp", 353, 193, 3, (1, 1, 351, 191), (2, 2, 348, 188), True),
]


@pytest.mark.parametrize("fmt,w,h,n,crop,rect,full", GEOMETRIES)
def test_geometry_matrix(dec, fmt, w, h, n, crop, rect, full):
    src = sources(n, fmt, w, h, w * 31 + h)
    got = run_import(dec, src, fmt, w, h, crop, rect, full)
    want = M.import_images(src, fmt, w, h, crop, rect, full)
    assert_same(got, want, f"{fmt} {w}x{h}")
    assert len({g.tobytes() for g in got}) == n


def test_crop_rectangle_border_and_strides(efx, dec):
    """The reference indexer's crop of a 1920 x 1080 picture into letterbox rectangles: the border is exactly black, and
    with padded strides nothing between or behind the output images is written."""
    w, h, n, crop = 1920, 1080, 2, (144, 0, 992, 546)
    src = sources(n, "rgb24", w, h, 5)
    size = src.shape[1]
    src_stride, dst_stride = size + 64, M.FRAME_BYTES + 48
    sbuf = upload_padded(dec, src, src_stride, fill=0x5A)
    dbuf = dec.alloc((n + 1) * dst_stride)
    for rect, full in ((efx.letterbox_rect(992, 546), False), ((16, 24, 320, 144), False), ((320, 160, 32, 32), True)):
        dbuf.upload(np.full(dbuf.nbytes, 0xA5, dtype=np.uint8))
        dec.import_to(sbuf, dbuf, n_images=n, fmt="rgb24", width=w, height=h, crop=crop, dst_rect=rect, full_range=full,
                      src_stride=src_stride, dst_stride=dst_stride)
        dec.sync()
        raw = dbuf.download(np.uint8, dbuf.nbytes)
        want = M.import_images(src, "rgb24", w, h, crop, rect, full)
        x, y, dw, dh = rect
        for i in range(n):
            img = raw[i * dst_stride:i * dst_stride + M.FRAME_BYTES]
            assert_same(img[None], want[i][None], f"rect {rect} image {i}")
            assert (raw[i * dst_stride + M.FRAME_BYTES:(i + 1) * dst_stride] == 0xA5).all()
            luma = img[:M.Y_BYTES].reshape(M.H, M.W).copy()
            inside = luma[y:y + dh, x:x + dw].copy()
            luma[y:y + dh, x:x + dw] = 0 if full else 16
            assert (luma == (0 if full else 16)).all() and inside.std() > 0
            for p in range(2):
                c = img[M.Y_BYTES + p * M.C_BYTES:M.Y_BYTES + (p + 1) * M.C_BYTES].reshape(M.CH, M.CW).copy()
                c[y // 2:(y + dh) // 2, x // 2:(x + dw) // 2] = 128
                assert (c == 128).all()
        assert (raw[n * dst_stride:] == 0xA5).all()
    sbuf.free()
    dbuf.free()


def test_identity_of_exported_pictures(efx):
    """Decoded pictures exported as I420 and imported at 352 x 192: the same bytes."""
    from espflix_amd import gen
    S, P = 6, 3
    d = efx.Decoder(max_streams=S, max_pictures=P, ring_depth=P + 1)
    d.upload(gen.Batch(3, S, P, 12, 0, threads=16).all_es(), efx.FORMAT_ES)
    d.decode()
    pics = d.export_host("i420", picture=P - 1)
    assert pics.shape == (S, M.FRAME_BYTES) and pics.std() > 0
    got = d.import_pictures(pics, width=352, height=192)
    assert isinstance(got, np.ndarray)
    assert_same(got, pics, "identity")
    d.close()


QUEUED = [("rgb24", 333, 77, None, None, False), ("i420", 704, 384, (64, 32, 512, 320), (16, 8, 320, 176), False),
          ("rgbp", 100, 50, None, (0, 46, 352, 100), True), ("i420", 352, 192, None, None, False)]


def test_queued_calls_keep_their_geometry(efx, dec):
    """Four imports of four geometries queued without a sync: each buffer holds its own geometry's result (one tap table
    serves them all, rewritten on the device in stream order).  Then import -> encode without a sync between: the
    encoder's reconstruction is that of the model's pictures."""
    n = 2
    jobs = []
    for k, (fmt, w, h, crop, rect, full) in enumerate(QUEUED):
        src = sources(n, fmt, w, h, 40 + k)
        stride = (src.shape[1] + 15) // 16 * 16
        jobs.append((src, upload_padded(dec, src, stride), dec.alloc(n * M.FRAME_BYTES)))
    for (fmt, w, h, crop, rect, full), (_, sbuf, dbuf) in zip(QUEUED, jobs):
        dec.import_to(sbuf, dbuf, n_images=n, fmt=fmt, width=w, height=h, crop=crop, dst_rect=rect, full_range=full)
    dec.sync()
    for (fmt, w, h, crop, rect, full), (src, sbuf, dbuf) in zip(QUEUED, jobs):
        got = dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES)
        assert_same(got, M.import_images(src, fmt, w, h, crop, rect, full), f"queued {fmt} {w}x{h}")
        sbuf.free()
        dbuf.free()

    # two streams of three pictures: a smooth moving picture, 640 x 360 RGB24
    S, P, w, h = 2, 3, 640, 360
    yy, xx = np.mgrid[0:h, 0:w]
    src = np.stack([np.stack([(xx + 9 * i) & 0xFF, (yy * 2 + 5 * i) & 0xFF, ((xx + yy) // 2 + i) & 0xFF], axis=-1).astype(np.uint8)
                    for i in range(S * P)]).reshape(S * P, -1)
    want_pics = M.import_images(src, "rgb24", w, h)
    stride = efx.encode_bound(efx.FORMAT_ES, P)
    sbuf = upload_padded(dec, src, src.shape[1])
    pics, out, rec = dec.alloc(S * P * M.FRAME_BYTES), dec.alloc(S * stride), dec.alloc(S * P * M.FRAME_BYTES)
    meta = dec.alloc(64)
    dec.import_to(sbuf, pics, n_images=S * P, fmt="rgb24", width=w, height=h)
    dec.encode_to(pics, out, meta.ptr, meta.ptr + 16, n_streams=S, n_pictures=P, qscale=6, fmt=efx.FORMAT_ES, recon=rec)
    dec.sync()
    got_rec = rec.download(np.uint8, S * P * M.FRAME_BYTES).reshape(S, P, M.FRAME_BYTES)
    lens = meta.download(np.uint32, S)
    got_streams = [bytes(out.download(np.uint8, S * stride)[i * stride:i * stride + int(lens[i])]) for i in range(S)]
    for b in (sbuf, pics, out, rec, meta):
        b.free()
    r = dec.encode(want_pics.reshape(S, P, M.FRAME_BYTES), qscale=6, fmt=efx.FORMAT_ES, recon=True)
    assert (r.status == 0).all()
    assert np.array_equal(got_rec, r.recon)
    assert got_streams == r.streams


def test_many_small_images(dec):
    n, w, h = 256, 64, 48
    src = sources(n, "rgb24", w, h, 9)
    stride = src.shape[1] + 48
    sbuf, dbuf = upload_padded(dec, src, stride, fill=0xEE), dec.alloc(n * M.FRAME_BYTES)
    dec.import_to(sbuf, dbuf, n_images=n, fmt="rgb24", width=w, height=h, src_stride=stride)
    dec.sync()
    got = dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES)
    sbuf.free()
    dbuf.free()
    assert_same(got, M.import_images(src, "rgb24", w, h), "256 images")


def test_import_pictures_letterbox(efx, dec):
    """The array path of import_pictures with every format, a crop and fit="letterbox"."""
    w, h, n = 200, 120, 2
    rgb = sources(n, "rgb24", w, h, 21).reshape(n, h, w, 3)
    got = dec.import_pictures(rgb, fit="letterbox")
    rect = M.letterbox_rect(w, h)
    assert rect == (16, 0, 320, 192)
    assert_same(got, M.import_images(rgb, "rgb24", w, h, None, rect), "letterbox rgb24")
    chw = np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))
    assert_same(dec.import_pictures(chw, fit="letterbox"), got, "letterbox rgbp")
    crop = (10, 20, 180, 40)
    got = dec.import_pictures(chw, crop=crop, fit="letterbox", full_range=True)
    assert_same(got, M.import_images(chw, "rgbp", w, h, crop, M.letterbox_rect(180, 40), True), "letterbox crop")
    yuv = sources(n, "i420", w, h, 22)
    out = dec.alloc(n * M.FRAME_BYTES)
    assert dec.import_pictures(yuv, width=w, height=h, out=out) is out
    assert_same(out.download(np.uint8, n * M.FRAME_BYTES).reshape(n, -1), M.import_images(yuv, "i420", w, h), "i420 out=")
    out.free()
    with pytest.raises(ValueError):
        dec.import_pictures(rgb, fit="fill")
    with pytest.raises(ValueError):
        dec.import_pictures(yuv)  # i420 without width / height
    with pytest.raises(ValueError):
        dec.import_pictures(np.zeros((1, 5000, 8, 3), dtype=np.uint8))


def test_argument_errors(efx, dec):
    lib, ctx = dec._lib, dec._ctx
    src, dst = dec.alloc(1 << 20), dec.alloc(4 * (M.FRAME_BYTES + 64))
    I420, RGB24, RGBP = efx.PIX_I420, efx.PIX_RGB24, efx.PIX_RGBP

    def call(s=src.ptr, d=dst.ptr, n=2, fmt=RGB24, w=64, h=48, crop=(0, 0, 0, 0), rect=(0, 0, 0, 0), full=0, ss=0, ds=0):
        o = efx._ImportOpts(n, fmt, w, h, *crop, *rect, full, ss, ds)
        return lib.efx_import_frames(ctx, C.byref(o), s, d)

    assert call() == 0
    assert call(s=None) == ARG and call(d=None) == ARG and call(s=src.ptr + 8) == ARG and call(d=dst.ptr + 4) == ARG
    assert lib.efx_import_frames(ctx, None, src.ptr, dst.ptr) == ARG
    assert call(n=0) == ARG and call(n=-3) == ARG
    assert call(fmt=3) == ARG and call(fmt=-1) == ARG
    assert call(w=1) == ARG and call(h=1) == ARG and call(w=4097) == ARG and call(h=4097) == ARG and call(w=0) == ARG
    assert call(fmt=I420, w=63) == ARG and call(fmt=I420, h=47) == ARG and call(fmt=I420) == 0 and call(w=63, h=47) == 0
    # crop: outside the source, negative, odd for I420
    assert call(crop=(0, 0, 65, 48)) == ARG and call(crop=(1, 0, 64, 48)) == ARG and call(crop=(0, 1, 64, 48)) == ARG
    assert call(crop=(-1, 0, 16, 16)) == ARG and call(crop=(0, -2, 16, 16)) == ARG and call(crop=(0, 0, 16, 0)) == ARG
    assert call(crop=(0, 0, -16, 16)) == ARG and call(crop=(0, 0, 16, 49)) == ARG
    assert call(crop=(3, 5, 61, 43)) == 0 and call(crop=(63, 47, 1, 1)) == 0
    for odd in ((1, 0, 16, 16), (0, 1, 16, 16), (0, 0, 15, 16), (0, 0, 16, 15)):
        assert call(fmt=I420, crop=odd) == ARG and call(fmt=RGBP, crop=odd) == 0
    # destination rectangle: odd, below 16, outside the frame
    for bad in ((1, 0, 16, 16), (0, 1, 16, 16), (0, 0, 17, 16), (0, 0, 16, 17), (0, 0, 14, 16), (0, 0, 16, 14),
                (-2, 0, 16, 16), (0, -2, 16, 16), (338, 0, 16, 16), (0, 178, 16, 16), (0, 0, 354, 192), (0, 0, 352, 194),
                (0, 0, -16, 16), (0, 0, 16, 0)):
        assert call(rect=bad) == ARG, bad
    assert call(rect=(336, 176, 16, 16)) == 0
    # strides
    size = 64 * 48 * 3
    assert call(ss=size - 16) == ARG and call(ss=size + 8) == ARG and call(ss=size + 16) == 0
    assert call(w=63, h=47, ss=63 * 47 * 3) == ARG and call(w=63, h=47, ss=(63 * 47 * 3 + 15) // 16 * 16) == 0
    assert call(ds=M.FRAME_BYTES - 16) == ARG and call(ds=M.FRAME_BYTES + 8) == ARG and call(ds=M.FRAME_BYTES + 64) == 0
    # the ratio limit: crop <= 32 x destination rectangle
    assert call(n=1, w=520, h=48, rect=(0, 0, 16, 16)) == ARG and call(n=1, w=512, h=48, rect=(0, 0, 16, 16)) == 0
    assert call(n=1, w=48, h=514, rect=(0, 0, 16, 16)) == ARG and call(n=1, w=48, h=512, rect=(0, 0, 16, 16)) == 0
    assert call(n=1, fmt=I420, w=514, h=48, rect=(0, 0, 16, 16)) == ARG
    assert call(n=1, w=520, h=48, crop=(4, 0, 512, 48), rect=(0, 0, 16, 16)) == 0
    dec.sync()
    assert lib.efx_import_src_bytes(RGB24, 64, 48) == size and lib.efx_import_src_bytes(I420, 64, 48) == size // 2
    assert lib.efx_import_src_bytes(RGBP, 333, 77) == 333 * 77 * 3
    for bad in ((3, 64, 48), (-1, 64, 48), (RGB24, 1, 48), (RGB24, 64, 1), (RGB24, 4097, 48), (RGB24, 64, 4097),
                (I420, 63, 48), (I420, 64, 47), (RGBP, 0, 0), (RGBP, -4, 16)):
        assert lib.efx_import_src_bytes(*bad) == 0, bad
    src.free()
    dst.free()
    with pytest.raises(ValueError):
        dec.import_to(0, 0, n_images=1, fmt="yuv444", width=16, height=16)
    with pytest.raises(efx.EfxError) as e:
        dec.import_to(0, 0, n_images=1, fmt="rgb24", width=16, height=16)
    assert e.value.status == ARG


TORCH_CHILD = textwrap.dedent("""
    import os
    import sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
    import espflix_amd as efx
    import import_model as M

    # a stream of torch's own (the default stream's handle is 0, which tells the library to make a private one)
    torch.cuda.set_stream(torch.cuda.Stream())
    dec = efx.Decoder(4, 2, device=torch.cuda.current_device(), hip_stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(11)
    checked = 0
    for n, h, w in ((3, 77, 333), (2, 360, 640)):   # (an image size that is no multiple of 16, and one that is)
        host = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        want = dec.import_pictures(host, fit="letterbox")           # the array path
        assert isinstance(want, np.ndarray) and want.shape == (n, 101376)
        assert np.array_equal(want, M.import_images(host, "rgb24", w, h, None, M.letterbox_rect(w, h)))
        t = torch.from_numpy(host).cuda()                            # (queued on torch's stream)
        out = torch.full((n * 101376,), 7, dtype=torch.uint8, device="cuda")
        got = dec.import_pictures(t, fit="letterbox", out=out, sync=False)  # ordered on torch's stream
        assert isinstance(got, torch.Tensor) and tuple(got.shape) == (n, 101376) and got.data_ptr() == out.data_ptr()
        assert np.array_equal(got.cpu().numpy(), want)
        chw = t.permute(0, 3, 1, 2).contiguous()
        got = dec.import_pictures(chw, fit="letterbox")              # allocated by import_pictures, synchronised
        assert np.array_equal(got.cpu().numpy(), want)
        checked += 1
    t = torch.zeros((2, 48, 64, 3), dtype=torch.uint8, device="cuda")
    for bad in (torch.empty(2 * 101376, dtype=torch.int16, device="cuda"), torch.empty(2 * 101376 + 1, dtype=torch.uint8, device="cuda"),
                torch.empty(2 * 101376, dtype=torch.uint8), torch.empty((2 * 101376, 2), dtype=torch.uint8, device="cuda")[:, 0]):
        try:
            dec.import_pictures(t, out=bad)
        except ValueError:
            checked += 1
    for bad in (t.cpu(), t.to(torch.int16)):
        try:
            dec.import_pictures(bad)
        except ValueError:
            checked += 1
    dec.close()
    print("torch import ok", checked)
""")


def test_torch_tensor_in_and_out(efx, tmp_path):
    """In a child process (torch's HIP runtime must come up first): a decoder on torch's current stream, a cuda tensor
    in, a tensor out without a sync, equal to the array path; out= and src checks."""
    script = tmp_path / "torch_import.py"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch import ok 8" in r.stdout
