"""efx_denoise (k_denoise.hip) on the device against tests/denoise_model.py, byte for byte, on padded regions whose fill
bytes must survive: every size at which the kernel takes another path, frame and stream counts, pitched planes, NV12 /
NV21, every threshold's extremes, a previous output that lies in the previous call's destination against one long call,
the default strides, every refused argument, the Python methods, and one chain from interlaced frames to imported
pictures."""
import ctypes as C
import os
import pickle
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import deint_model
import denoise_model as M
import import_model
import surface_model as S
import test_denoise_model as T
from test_gpu_telecine import Region, c_surface, upload_padded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
CHUNK, TILE, BAND = 16, 992, 4  # k_denoise's chunk, column tile and row band (denoise_px.h: kChunk, kTileCols, kBandRows)
MID = dict(luma_spatial=7, chroma_spatial=5, luma_temporal=9, chroma_temporal=12)


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
    """The sizes below were chosen by these constants."""
    text = open(os.path.join(ROOT, "espflix_amd", "csrc", "denoise_px.h")).read()
    value = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    assert "kChunk = dpx::kChunk;" in text and "kTileChunks = dpx::kTileChunks;" in text
    deint = open(os.path.join(ROOT, "espflix_amd", "csrc", "deint_px.h")).read()
    assert "kChunk = 16;" in deint and "kTileChunks = 62;" in deint
    assert value("kTileCols") == TILE == 62 * CHUNK and value("kBandRows") == BAND


def run_call(efx, dec, srcs, s, n_streams=1, prev=None, thr=MID, default_strides=False):
    """One call on padded regions against the model; returns the model's outputs (n_streams * n_frames, image).  prev: the
    streams' previous outputs (n_streams, image), uploaded into a padded region of their own."""
    what = (s.width, s.height, s.layout, len(srcs), n_streams, thr, prev is not None)
    want = M.denoise(srcs, s, n_streams, prev=prev, **thr)
    image = s.width * s.height * 3 // 2
    sbuf, src_stride = upload_padded(dec, srcs, 0 if default_strides else 64)
    dst = Region(dec, len(srcs), image, pad=0 if default_strides else 64)
    pbuf, prev_stride = upload_padded(dec, prev) if prev is not None else (None, 0)
    got = dec.denoise_to(sbuf, dst.buf, surface=c_surface(efx, s), n_streams=n_streams, n_frames=len(srcs) // n_streams, prev=pbuf,
                         src_stride=0 if default_strides else src_stride, dst_stride=0 if default_strides else dst.stride,
                         prev_stride=prev_stride, **thr)
    dec.sync()
    assert got == len(srcs) // n_streams
    dst.expect(want)
    dst.check(what)
    sbuf.free()
    dst.free()
    if pbuf is not None:
        pbuf.free()
    return want


def every_layout(efx, dec, w, h, frames=2, seed=0):
    for k, (name, s) in enumerate(T.surfaces(w, h)):
        run_call(efx, dec, T.directed(frames, s, 1000 * w + 10 * h + k + seed), s)


# widths: the smallest, a chunk - 2, a chunk, + 2, and the column tile - 2, the tile, + 2 (a second tile of one chunk; the
# chroma planes of these no longer share a wave)
WIDTHS = [(2, 6), (CHUNK - 2, 6), (CHUNK, 6), (CHUNK + 2, 6), (TILE - 2, 10), (TILE, 10), (TILE + 2, 10)]
# heights: the smallest (one chroma row), 6 (three), and the row band - 2, the band, + 2 and two bands + 2 (luma), four
# bands + 2 (the same for the chroma planes: 9 rows), eight bands + 2
HEIGHTS = [(18, 2), (18, 6), (18, BAND - 2), (18, BAND), (18, BAND + 2), (18, 2 * BAND + 2), (18, 4 * BAND + 2), (34, 8 * BAND + 2)]


@pytest.mark.parametrize("w,h", WIDTHS + HEIGHTS, ids=[f"{w}x{h}" for w, h in WIDTHS + HEIGHTS])
def test_sizes_in_every_layout(efx, dec, w, h):
    """I420, pitched YV12, pitched NV12 and NV21 at every size at which the kernel takes another path."""
    every_layout(efx, dec, w, h)


@pytest.mark.parametrize("frames", [1, 2, 5])
@pytest.mark.parametrize("n_streams", [1, 3])
def test_frames_and_streams(efx, dec, frames, n_streams):
    for name, s in T.surfaces(34, 10):
        srcs = np.concatenate([T.directed(frames, s, 20 + i) if i != 1 else S.sources(frames, s, 30) for i in range(n_streams)])
        want = run_call(efx, dec, srcs, s, n_streams=n_streams)
        if n_streams > 1:
            assert np.array_equal(want[frames:2 * frames], M.denoise(srcs[frames:2 * frames], s, **MID)), "the model's streams see each other"


def test_wide_pitched_picture(efx, dec):
    """720 x 16 with a pitch of 768 and padded plane rows, I420, YV12 and NV12: whole waves of chunks."""
    for kind in ("i420", "yv12", "nv12"):
        s = S.layout(kind, 720, 16, 768, 24)
        assert s.pitch[0] == 768
        run_call(efx, dec, T.directed(3, s, 40), s)


def test_last_row_ends_near_the_regions_end(efx, dec):
    """Images whose last row ends fewer than 16 bytes before the end of the source region (the default strides, no pad
    behind any image, source or destination): the 16-byte loads of that row must stay inside and still give its samples."""
    for kind, w, h, pitch in (("i420", 18, 6, 0), ("nv12", 30, 6, 31), ("i420", 34, 10, 0), ("nv21", 2, 2, 0)):
        s = S.layout(kind, w, h, pitch)
        last = max(s.offset[p] + (rows - 1) * s.pitch[p] + n for p, rows, n in s.planes())
        assert 0 <= (s.bytes + 15) // 16 * 16 - last < 16
        run_call(efx, dec, T.directed(3, s, w), s, default_strides=True)
        prev = np.random.default_rng(w).integers(0, 256, (1, w * h * 3 // 2), dtype=np.uint8)
        run_call(efx, dec, T.directed(2, s, w + 1), s, prev=prev)


@pytest.mark.parametrize("position", T.NAMES)
def test_threshold_extremes(efx, dec, position):
    """0, 1 and 64 in each of the four positions, the other three in mid-range."""
    s = S.layout("nv12", 34, 10, 40)
    srcs = T.directed(3, s, 50)
    outs = [run_call(efx, dec, srcs, s, thr={**MID, position: v}) for v in (0, 1, 64)]
    assert not np.array_equal(outs[0], outs[2])


def test_spatial_only_and_temporal_only(efx, dec):
    s = S.layout("i420", 34, 10)
    srcs = T.directed(4, s, 51)
    spatial = run_call(efx, dec, srcs, s, thr=dict(luma_spatial=12, chroma_spatial=12, luma_temporal=0, chroma_temporal=0))
    temporal = run_call(efx, dec, srcs, s, thr=dict(luma_spatial=0, chroma_spatial=0, luma_temporal=24, chroma_temporal=24))
    assert np.array_equal(temporal[0], S.canonicals(srcs, s)[0]) and not np.array_equal(spatial[0], temporal[0])
    assert np.array_equal(run_call(efx, dec, srcs, s, thr=dict.fromkeys(T.NAMES, 0)), S.canonicals(srcs, s))


def test_pieces_with_prev_in_the_previous_destination(efx, dec):
    """Two streams of 5 frames as pieces of 2 + 3: the second call's prev points at the last picture of each stream in
    the first call's destination (prev_stride = 2 x dst_stride).  The pieces equal one long call, byte for byte."""
    for s in (S.layout("nv12", 70, 20, 80), S.layout("i420", 18, 6)):
        image = s.width * s.height * 3 // 2
        a, b = T.directed(5, s, 60), T.directed(5, s, 61)
        whole = run_call(efx, dec, np.concatenate([a, b]), s, n_streams=2)
        first, second = Region(dec, 4, image), Region(dec, 6, image)
        src1, stride1 = upload_padded(dec, np.concatenate([a[:2], b[:2]]))
        src2, stride2 = upload_padded(dec, np.concatenate([a[2:], b[2:]]))
        surf = c_surface(efx, s)
        dec.denoise_to(src1, first.buf, surface=surf, n_streams=2, n_frames=2, src_stride=stride1, dst_stride=first.stride, **MID)
        dec.denoise_to(src2, second.buf, surface=surf, n_streams=2, n_frames=3, src_stride=stride2, dst_stride=second.stride,
                       prev=first.buf.ptr + first.stride, prev_stride=2 * first.stride, **MID)
        dec.sync()
        first.expect(whole[[0, 1, 5, 6]])
        first.check("the first piece")
        second.expect(whole[[2, 3, 4, 7, 8, 9]])
        second.check("the second piece")
        for b_ in (src1, src2):
            b_.free()
        first.free()
        second.free()


def test_argument_errors(efx, dec):
    """Every EFX_ERR_ARG case of include/efx.h returns its status and leaves the destination alone."""
    lib = efx.load_library()
    good = S.layout("nv12", 34, 10, 50)
    srcs = S.sources(4, good, 70)
    src, src_stride = upload_padded(dec, srcs)
    image = 34 * 10 * 3 // 2
    dst = Region(dec, 6, image)
    prev = Region(dec, 2, image)
    ok = dict(n_streams=1, n_frames=4, luma_spatial=7, chroma_spatial=5, luma_temporal=9, chroma_temporal=12, src_stride=src_stride,
              dst_stride=dst.stride, prev_stride=0)

    def status(s, sp, pp, dp, **kw):
        o = np.zeros(1, dtype=efx.DENOISE_OPTS_DTYPE)
        for k, v in {**ok, **kw}.items():
            o[0][k] = v
        return lib.efx_denoise(dec._ctx, C.byref(c_surface(efx, s)) if s is not None else None, o.ctypes.data, sp, pp, dp)

    P, D, V = src.ptr, dst.buf.ptr, prev.buf.ptr
    for what, s in S.rejected_surfaces():
        assert status(s, P, None, D) == ARG, what
        assert lib.efx_last_error(dec._ctx).startswith(b"efx_denoise: "), what
    for s in (S.layout("p010", 34, 10, 74), S.layout("i010", 34, 10, 72)):
        assert S.check(s) and not M.accepts(s) and status(s, P, None, D) == ARG, s
    cases = [dict(n_streams=0), dict(n_streams=-1), dict(n_frames=0), dict(n_frames=-1),
             dict(luma_spatial=65), dict(luma_spatial=-1), dict(chroma_spatial=65), dict(chroma_spatial=-1),
             dict(luma_temporal=65), dict(luma_temporal=-1), dict(chroma_temporal=65), dict(chroma_temporal=-1),
             dict(n_streams=1 << 16, n_frames=1 << 15),            # 2^31 images
             dict(src_stride=good.bytes // 16 * 16), dict(src_stride=src_stride + 8), dict(dst_stride=image // 16 * 16),
             dict(dst_stride=dst.stride + 8), dict(prev_stride=8), dict(prev_stride=prev.stride + 8)]
    assert good.bytes % 16 and image % 16
    for kw in cases:
        assert status(good, P, None, D, **kw) == ARG, kw
    for sp, pp, dp in [(None, None, D), (P, None, None), (P + 8, None, D), (P, None, D + 4), (P, V + 8, D)]:
        assert status(good, sp, pp, dp) == ARG, (sp, pp, dp)
    # a previous output for each of two streams needs their distance
    assert status(good, P, V, D, n_streams=2, n_frames=2, prev_stride=0) == ARG
    assert status(good, P, V, D, n_streams=2, n_frames=2, prev_stride=image // 16 * 16) == ARG
    assert status(None, P, None, D) == ARG
    dec.sync()
    dst.check("after the refused calls")
    prev.check("the previous outputs after the refused calls")
    # one stream with a prev needs no prev_stride; two streams with theirs
    before = np.random.default_rng(71).integers(0, 256, (2, image), dtype=np.uint8)
    prev.expect(before)
    prev.buf.upload(prev.want.reshape(-1))
    assert status(good, P, V, D) == 0
    dec.sync()
    dst.expect(M.denoise(srcs, good, 1, prev=before[:1], **MID))
    dst.check("the accepted call")
    assert status(good, P, V, D, n_streams=2, n_frames=2, prev_stride=prev.stride) == 0
    dec.sync()
    dst.expect(M.denoise(srcs, good, 2, prev=before, **MID))
    dst.check("the accepted call with two streams")
    prev.check("the previous outputs")
    src.free()
    dst.free()
    prev.free()


def test_python_methods(efx, dec):
    """denoise() on arrays returns the model's pictures; its result is the next piece's prev and import_pictures' source."""
    w, h = 70, 40
    s = S.layout("nv12", w, h, 96, 48)
    srcs = T.directed(6, s, 80)
    kw = dict(fmt="nv12", width=w, height=h, pitch=96, plane_rows=48)
    thr = dict(zip(T.NAMES, efx.denoise_thresholds(3)))
    want = M.denoise(srcs, s, **thr)
    out = dec.denoise(srcs, **kw, **thr)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (6, w * h * 3 // 2) and np.array_equal(out, want)
    first = dec.denoise(srcs[:4], **kw, **thr)
    second = dec.denoise(srcs[4:], prev=first[-1:], **kw, **thr)
    assert np.array_equal(np.concatenate([first, second]), want)
    two = dec.denoise(srcs, n_streams=2, prev=want[:2], **kw, **thr)
    assert np.array_equal(two, M.denoise(srcs, s, 2, prev=want[:2], **thr))
    assert np.array_equal(dec.denoise(srcs, **kw), S.canonicals(srcs, s)), "all thresholds 0 is the identity"
    assert dec.import_pictures(out, fmt="i420", width=w, height=h).shape == (6, 101376)
    with pytest.raises(ValueError):
        dec.denoise(srcs, luma_spatial=65, **kw)
    with pytest.raises(ValueError):
        dec.denoise(srcs, n_streams=4, **kw)
    with pytest.raises(ValueError):
        dec.denoise(srcs, prev=want[:2], **kw)
    with pytest.raises(efx.EfxError):
        dec.denoise_to(0, 0, surface=c_surface(efx, s), n_frames=1)


def test_interlaced_frames_to_imported_pictures(efx, dec):
    """deinterlace -> denoise -> import_pictures on the device equals the models' chain."""
    w, h = 34, 12
    s = S.layout("nv12", w, h, 40)
    srcs = T.directed(4, s, 90)
    prog = dec.deinterlace(srcs, fmt="nv12", width=w, height=h, pitch=40, first_field="top", rate="field")
    clean = dec.denoise(prog, fmt="i420", width=w, height=h, **MID)
    pics = dec.import_pictures(clean, fmt="i420", width=w, height=h)
    want_prog = deint_model.deinterlace(srcs, s, 1, deint_model.TOP, deint_model.FIELD)[0]
    want_clean = M.denoise_i420(want_prog, w, h, **MID)
    assert np.array_equal(prog, want_prog) and np.array_equal(clean, want_clean)
    assert np.array_equal(pics, import_model.import_images(want_clean, "i420", w, h, None, None))


TORCH_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import surface_model as S
    import test_denoise_model as T
    from test_gpu_telecine import c_surface

    out = []
    thr = dict(luma_spatial=7, chroma_spatial=5, luma_temporal=9, chroma_temporal=12)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device())
    for kind, w, h in (("i420", 64, 48), ("nv12", 18, 6)):   # 4608 bytes a picture: packed rows of 16; 162: padded
        s = S.layout(kind, w, h)
        t = torch.from_numpy(T.directed(5, s, 95)).cuda()
        whole = dec.denoise(t, fmt=kind, width=w, height=h, **thr)
        first = dec.denoise(t[:2], fmt=kind, width=w, height=h, **thr)
        second = dec.denoise(t[2:], fmt=kind, width=w, height=h, prev=first[1:], **thr)
        assert all(isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.uint8 for o in (whole, first, second))
        assert tuple(whole.shape) == (5, w * h * 3 // 2) and torch.equal(whole, torch.cat([first, second]))
        if kind == "i420":  # denoise_to on the tensors' own memory
            dst = torch.zeros_like(t)
            torch.cuda.synchronize()
            dec.denoise_to(t.data_ptr(), dst.data_ptr(), surface=c_surface(efx, s), n_frames=5, src_stride=s.bytes, dst_stride=s.bytes, **thr)
            dec.sync()
            assert torch.equal(dst, whole)
        pics = dec.import_pictures(whole, fmt="i420", width=w, height=h)
        assert tuple(pics.shape) == (5, 101376)
        out.append(whole.cpu().numpy())
    dec.close()
    pickle.dump(out, open(sys.argv[2], "wb"))
    print("denoise ok")
""")


def test_tensor_in_tensor_out(efx, tmp_path):
    """A tensor in, a tensor out on the device, prev a tensor too, and denoise_to on tensors' memory (a process of its own:
    torch's HIP runtime first)."""
    script, out = tmp_path / "denoise_tensor.py", tmp_path / "out.pkl"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "denoise ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = pickle.load(open(out, "rb"))
    for whole, (kind, w, h) in zip(got, (("i420", 64, 48), ("nv12", 18, 6))):
        s = S.layout(kind, w, h)
        assert np.array_equal(whole, M.denoise(T.directed(5, s, 95), s, **MID))
