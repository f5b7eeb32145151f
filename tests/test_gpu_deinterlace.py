"""efx_deinterlace (k_deint.hip) on the device against tests/deint_model.py, byte for byte, on padded regions whose fill
bytes must survive: every size at which the kernel takes another path, both modes and parities, NV12 / NV21, streams,
pieces against the whole, short calls, every refused argument, and the Python methods."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import textwrap
from dataclasses import replace

import numpy as np
import pytest

import deint_model as M
import import_model
import surface_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64        # bytes between images in every padded region
FILL = 0xA5
ARG = -1
TILE, BAND = 992, 16  # k_deint's column tile and row band (deint_px.h: kTileCols, kBandRows)


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def dec(efx):
    d = efx.Decoder(1, 1)
    yield d
    d.close()


def test_tile_and_band_are_the_kernels():
    text = open(os.path.join(ROOT, "espflix_amd", "csrc", "deint_px.h")).read()
    assert "kTileChunks = 62;" in text and "kChunk = 16;" in text and "kBandRows = 16;" in text and "kHalfChunks = 30;" in text


class Region:
    """n images of `image` bytes, `stride` apart (a pad behind each), filled with FILL, on the device."""

    def __init__(self, dec, n, image):
        self.n, self.image = n, image
        self.stride = (image + 15) // 16 * 16 + PAD
        self.buf = dec.alloc(n * self.stride)
        self.buf.upload(np.full(n * self.stride, FILL, dtype=np.uint8))
        self.want = np.full((n, self.stride), FILL, dtype=np.uint8)  # what the model expects there

    def expect(self, images):
        """images (k, image) from image 0 on."""
        self.want[:len(images), :self.image] = images

    def check(self, what):
        got = self.buf.download(np.uint8, self.n * self.stride).reshape(self.n, self.stride)
        bad = np.argwhere(got != self.want)
        assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at (image, byte) {bad[0].tolist()}"

    def free(self):
        self.buf.free()


def upload_padded(dec, srcs):
    """(n, bytes) source images with a pad behind each: (buffer, stride)."""
    n, size = srcs.shape
    stride = (size + 15) // 16 * 16 + PAD
    host = np.full((n, stride), 0x5A, dtype=np.uint8)
    host[:, :size] = srcs
    buf = dec.alloc(n * stride)
    buf.upload(host)
    return buf, stride


def c_surface(efx, s):
    c = efx._Surface()
    c.layout, c.shift, c.swap_uv, c.width, c.height, c.bytes = s.layout, s.shift, s.swap_uv, s.width, s.height, s.bytes
    for i in range(3):
        c.offset[i], c.pitch[i] = s.offset[i], s.pitch[i]
    return c


def run_call(efx, dec, srcs, s, n_streams=1, first_field="top", rate="field", lead=False, tail=False, src=None):
    """One call on padded regions against the model; returns the outputs (n_streams, n_out, image)."""
    what = (s.width, s.height, s.layout, first_field, rate, lead, tail)
    want = M.deinterlace(srcs, s, n_streams, M.TOP if first_field == "top" else M.BOTTOM, M.FIELD if rate == "field" else M.FRAME,
                         int(lead), int(tail))
    image = s.width * s.height * 3 // 2
    sbuf, src_stride = src or upload_padded(dec, srcs)
    dst = Region(dec, n_streams * want.shape[1], image)
    got = dec.deinterlace_to(sbuf, dst.buf, surface=c_surface(efx, s), n_streams=n_streams, n_frames=len(srcs) // n_streams,
                             first_field=first_field, rate=rate, lead=lead, tail=tail, src_stride=src_stride, dst_stride=dst.stride)
    dec.sync()
    assert got == want.shape[1] == efx.deinterlace_count(len(srcs) // n_streams, rate=rate, lead=lead, tail=tail), what
    dst.expect(want.reshape(-1, image))
    dst.check(what)
    if src is None:
        sbuf.free()
    dst.free()
    return want


def all_settings(efx, dec, s, seed, frames=3):
    srcs = S.sources(frames, s, seed)
    src = upload_padded(dec, srcs)
    for first_field in ("top", "bottom"):
        for rate in ("frame", "field"):
            run_call(efx, dec, srcs, s, first_field=first_field, rate=rate, src=src)
    src[0].free()


# the sizes of the host test; the widest and the tallest picture; a pitched SD strip; 2 below and 2 above the column tile
# (luma: 992, and 1984 + 2 for the chroma planes' tile); 4 below and 4 above the row band (luma: 16; 32 + 4 for chroma)
# 960 and 962: the widest picture whose chroma planes share a wave (480 samples a row), and the first whose do not
SIZES = [(2, 8), (18, 8), (34, 12), (70, 20), (4096, 8), (8, 4096), (TILE - 2, 8), (TILE + 2, 8), (2 * TILE + 2, 8),
         (18, BAND - 4), (18, BAND + 4), (18, 2 * BAND + 4), (960, 8), (962, 8)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes_both_modes_both_parities(efx, dec, w, h):
    all_settings(efx, dec, S.layout("i420", w, h), 1000 * w + h)


def test_pitched_planes(efx, dec):
    """720 x 32 with a pitch of 768 and padded plane rows, I420 and YV12 (swapped offsets)."""
    for kind in ("i420", "yv12"):
        s = S.layout(kind, 720, 32, 768, 40)
        assert s.pitch[0] == 768 and 768 * 40 in s.offset
        all_settings(efx, dec, s, 720)


@pytest.mark.parametrize("kind,w,h,pitch", [("nv12", 34, 12, 39), ("nv21", 34, 12, 0), ("nv12", TILE + 2, 8, 1000), ("nv21", TILE + 2, 8, 0), ("nv12", 960, 8, 0)])
def test_semi_planar(efx, dec, kind, w, h, pitch):
    """NV12 and NV21 at two sizes, one with rows on every byte phase, one across the column tile."""
    all_settings(efx, dec, S.layout(kind, w, h, pitch), w + len(kind))


def test_two_streams_do_not_see_each_other(efx, dec):
    s = S.layout("i420", 34, 12)
    srcs = S.sources(10, s, 11)
    for rate in ("frame", "field"):
        both = run_call(efx, dec, srcs, s, n_streams=2, first_field="bottom", rate=rate)
        # stream 1's first frame has no previous frame, stream 0's last has no next one
        alone = M.deinterlace(srcs[5:], s, 1, M.BOTTOM, M.FIELD if rate == "field" else M.FRAME)
        assert np.array_equal(both[1], alone[0])
        seen = M.deinterlace(srcs[4:], s, 1, M.BOTTOM, M.FIELD if rate == "field" else M.FRAME, 1, 0)
        assert not np.array_equal(both[1][:2], seen[0][:2])


def test_pieces_concatenate_to_the_whole(efx, dec):
    """7 frames as pieces with one frame of overlap: 3 with tail, 4 with lead + tail, 4 with lead; and 3 / 4 / 3 of the
    first 6 frames."""
    s = S.layout("nv12", 70, 20, 80)
    title = S.sources(7, s, 12)
    for rate in ("frame", "field"):
        whole = run_call(efx, dec, title, s, rate=rate)
        parts = [run_call(efx, dec, title[0:3], s, rate=rate, tail=True), run_call(efx, dec, title[1:5], s, rate=rate, lead=True, tail=True),
                 run_call(efx, dec, title[3:7], s, rate=rate, lead=True)]
        assert np.array_equal(np.concatenate(parts, axis=1), whole)
        six = run_call(efx, dec, title[:6], s, rate=rate)
        parts[2] = run_call(efx, dec, title[3:6], s, rate=rate, lead=True)
        assert np.array_equal(np.concatenate(parts, axis=1), six)


def test_short_calls(efx, dec):
    s = S.layout("i420", 18, 8)
    srcs = S.sources(2, s, 13)
    for first_field in ("top", "bottom"):
        one = run_call(efx, dec, srcs[:1], s, first_field=first_field)
        assert one.shape[1] == 2
        led = run_call(efx, dec, srcs, s, first_field=first_field, lead=True)
        assert led.shape[1] == 2
        assert run_call(efx, dec, srcs, s, first_field=first_field, rate="frame", lead=True).shape[1] == 1


def test_argument_errors(efx, dec):
    """Every EFX_ERR_ARG case of include/efx.h returns its status and leaves the destination alone."""
    lib = efx.load_library()
    good = S.layout("nv12", 34, 12, 50)
    srcs = S.sources(4, good, 14)
    src, src_stride = upload_padded(dec, srcs)
    image = 34 * 12 * 3 // 2
    dst = Region(dec, 8, image)
    ok = dict(n_streams=1, n_frames=4, first_field=0, mode=1, lead=0, tail=0, src_stride=src_stride, dst_stride=dst.stride)

    def status(s, sp, dp, **kw):
        f = {**ok, **kw}
        o = efx._DeintOpts(f["n_streams"], f["n_frames"], f["first_field"], f["mode"], f["lead"], f["tail"], f["src_stride"], f["dst_stride"])
        return lib.efx_deinterlace(dec._ctx, C.byref(c_surface(efx, s)) if s is not None else None, C.byref(o), sp, dp)

    P, D = src.ptr, dst.buf.ptr
    for what, s in S.rejected_surfaces():
        assert status(s, P, D) == ARG, what
        assert lib.efx_last_error(dec._ctx).startswith(b"efx_deinterlace: "), what
    words = [S.layout("p010", 34, 12, 74), S.layout("i010", 34, 12, 72)]
    heights = [replace(good, height=10), replace(good, height=6), replace(good, height=4), replace(good, height=2)]
    for s in words + heights:
        assert S.check(s) and not M.accepts(s) and status(s, P, D) == ARG, s
    cases = [dict(n_streams=0), dict(n_frames=0), dict(first_field=2), dict(first_field=-1), dict(mode=2), dict(mode=-1), dict(lead=2),
             dict(tail=-1), dict(lead=1, tail=1, n_frames=2), dict(lead=1, n_frames=1), dict(tail=1, n_frames=1),
             dict(n_streams=1 << 16, n_frames=1 << 15),            # 2^31 images in
             dict(n_streams=1 << 15, n_frames=1 << 15),            # 2^30 in, 2^31 out
             dict(src_stride=good.bytes // 16 * 16), dict(src_stride=src_stride + 8), dict(dst_stride=image // 16 * 16), dict(dst_stride=dst.stride + 8)]
    assert good.bytes % 16 and image % 16
    for kw in cases:
        assert status(good, P, D, **kw) == ARG, kw
    for sp, dp in [(None, D), (P, None), (P + 8, D), (P, D + 4)]:
        assert status(good, sp, dp) == ARG, (sp, dp)
    assert status(None, P, D) == ARG
    dec.sync()
    dst.check("after the refused calls")
    assert status(good, P, D) == 0
    dec.sync()
    dst.expect(M.deinterlace(srcs, good, 1).reshape(-1, image))
    dst.check("the accepted call")
    src.free()
    dst.free()


def test_python_methods(efx, dec):
    """import_pictures(deinterlace="tff") is deinterlace(rate="frame") followed by import_pictures(); field_rate=True
    doubles the count; deinterlace() returns the model's pictures."""
    w, h = 70, 40
    s = S.layout("nv12", w, h, 96, 48)
    srcs = S.sources(3, s, 15)
    kw = dict(fmt="nv12", width=w, height=h, pitch=96, plane_rows=48)
    prog = dec.deinterlace(srcs, first_field="top", rate="frame", **kw)
    assert isinstance(prog, np.ndarray) and np.array_equal(prog, M.deinterlace(srcs, s, 1, M.TOP, M.FRAME)[0])
    two = dec.import_pictures(prog, fmt="i420", width=w, height=h)
    one = dec.import_pictures(srcs, deinterlace="tff", **kw)
    assert one.shape == (3, 101376) and np.array_equal(one, two)
    assert np.array_equal(one, import_model.import_images(prog, "i420", w, h, None, None))
    fields = dec.import_pictures(srcs, deinterlace="bff", field_rate=True, crop=(2, 4, 60, 32), fit="letterbox", **kw)
    prog2 = dec.deinterlace(srcs, first_field="bff", rate="field", **kw)
    assert fields.shape == (6, 101376) and prog2.shape == (6, w * h * 3 // 2)
    assert np.array_equal(fields, dec.import_pictures(prog2, fmt="i420", width=w, height=h, crop=(2, 4, 60, 32), fit="letterbox"))
    # streams and pieces through the array method
    assert np.array_equal(dec.deinterlace(srcs[:2], n_streams=2, **kw), M.deinterlace(srcs[:2], s, 2).reshape(4, -1))
    assert np.array_equal(dec.deinterlace(srcs, lead=True, tail=True, **kw), M.deinterlace(srcs, s, 1, lead=1, tail=1)[0])
    # without deinterlace= nothing changes
    assert np.array_equal(dec.import_pictures(srcs, **kw), S.import_images(srcs, s))
    with pytest.raises(ValueError):
        dec.import_pictures(srcs, field_rate=True, **kw)
    with pytest.raises(ValueError):
        dec.import_pictures(srcs, deinterlace="top", **kw)
    with pytest.raises(ValueError):
        dec.deinterlace(srcs, rate="double", **kw)


TORCH_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import surface_model as S

    out = []
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device())
    for kind, w, h in (("i420", 64, 48), ("nv12", 18, 8)):   # 4608 bytes a picture: packed rows of 16; 216: padded
        s = S.layout(kind, w, h)
        t = torch.from_numpy(S.sources(3, s, 16)).cuda()
        prog = dec.deinterlace(t, fmt=kind, width=w, height=h, first_field="bottom")
        pics = dec.import_pictures(t, fmt=kind, width=w, height=h, deinterlace="bff", field_rate=True)
        assert all(isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.uint8 for o in (prog, pics))
        assert tuple(prog.shape) == (6, w * h * 3 // 2) and tuple(pics.shape) == (6, 101376)
        same = dec.import_pictures(prog, fmt="i420", width=w, height=h)
        assert torch.equal(pics, same)
        out.append(prog.cpu().numpy())
    dec.close()
    pickle.dump(out, open(sys.argv[2], "wb"))
    print("deinterlace ok")
""")


def test_tensor_in_tensor_out(efx, tmp_path):
    """A tensor in, a tensor out on the device (a process of its own: torch's HIP runtime first)."""
    script, out = tmp_path / "deint_tensor.py", tmp_path / "out.pkl"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "deinterlace ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = pickle.load(open(out, "rb"))
    for prog, (kind, w, h) in zip(got, (("i420", 64, 48), ("nv12", 18, 8))):
        s = S.layout(kind, w, h)
        assert np.array_equal(prog, M.deinterlace(S.sources(3, s, 16), s, 1, M.BOTTOM, M.FIELD)[0])
