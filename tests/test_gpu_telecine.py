"""efx_detelecine (k_telecine.hip) on the device against tests/telecine_model.py, byte for byte, outputs and records, on
padded regions whose fill bytes must survive: every size at which the kernels take another path, both parities, pitched
planes, NV12 / NV21, streams, pieces against the whole, short calls, a dirty record buffer, every refused argument, the
Python methods, and one cadence case."""
import ctypes as C
import os
import pickle
import re
import subprocess
import sys
import textwrap
from dataclasses import replace

import numpy as np
import pytest

import surface_model as S
import telecine_model as M
import test_telecine_model as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64        # bytes between images in every padded region
FILL = 0xA5
ARG = -1
CHUNK, TILE, BAND = 16, 1024, 32  # k_telecine's chunk, the columns of a wave's 64 strips and the row band (telecine_px.h: kChunk, kWaveStrips, kBandRows)


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
    text = open(os.path.join(ROOT, "espflix_amd", "csrc", "telecine_px.h")).read()
    value = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    assert "kChunk = dpx::kChunk;" in text
    assert "kChunk = 16;" in open(os.path.join(ROOT, "espflix_amd", "csrc", "deint_px.h")).read()
    assert value("kWaveStrips") * CHUNK == TILE and value("kBandRows") == BAND and value("kCycle") == 5


class Region:
    """n items of `image` bytes, `stride` apart (a pad behind each), filled with `fill`, on the device."""

    def __init__(self, dec, n, image, fill=FILL, pad=PAD, align=16):
        self.n, self.image = n, image
        self.stride = (image + align - 1) // align * align + pad
        self.buf = dec.alloc(n * self.stride)
        self.buf.upload(np.full(n * self.stride, fill, dtype=np.uint8))
        self.want = np.full((n, self.stride), fill, dtype=np.uint8)  # what the model expects there

    def expect(self, images):
        """images (k, image) from item 0 on."""
        self.want[:len(images), :self.image] = images

    def check(self, what):
        got = self.buf.download(np.uint8, self.n * self.stride).reshape(self.n, self.stride)
        bad = np.argwhere(got != self.want)
        assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at (item, byte) {bad[0].tolist()}"

    def free(self):
        self.buf.free()


def upload_padded(dec, srcs, pad=PAD):
    """(n, bytes) source images with a pad behind each but the last, which ends where its bytes rounded up to 16 end:
    (buffer, stride)."""
    n, size = srcs.shape
    stride = (size + 15) // 16 * 16 + pad
    host = np.full((n, stride), 0x5A, dtype=np.uint8)
    host[:, :size] = srcs
    buf = dec.alloc(n * stride - pad)
    buf.upload(host.reshape(-1)[:n * stride - pad])
    return buf, stride


def c_surface(efx, s):
    c = efx._Surface()
    c.layout, c.shift, c.swap_uv, c.width, c.height, c.bytes = s.layout, s.shift, s.swap_uv, s.width, s.height, s.bytes
    for i in range(3):
        c.offset[i], c.pitch[i] = s.offset[i], s.pitch[i]
    return c


def run_call(efx, dec, srcs, s, n_streams=1, first_field="top", lead=False, nt=10, src=None, info_fill=FILL, pad=PAD):
    """One call on padded regions against the model; returns the model's (outputs (n_streams, n_out, image), records
    (n_streams, n))."""
    what = (s.width, s.height, s.layout, first_field, lead, nt)
    want, recs = M.detelecine(srcs, s, n_streams, M.TOP if first_field == "top" else M.BOTTOM, int(lead), nt)
    image = s.width * s.height * 3 // 2
    sbuf, src_stride = src or upload_padded(dec, srcs, pad)
    dst = Region(dec, n_streams * want.shape[1], image)
    # the records lie one behind the other; one region item holds them all, the pad behind it must survive
    info = Region(dec, 1, recs.size * 32, fill=info_fill)
    got = dec.detelecine_to(sbuf, dst.buf, info.buf, surface=c_surface(efx, s), n_streams=n_streams, n_frames=len(srcs) // n_streams,
                            first_field=first_field, lead=lead, nt=nt, src_stride=src_stride, dst_stride=dst.stride)
    dec.sync()
    assert got == want.shape[1] == efx.detelecine_count(len(srcs) // n_streams, lead=lead), what
    info.expect(np.frombuffer(recs.tobytes(), dtype=np.uint8)[None, :])
    info.check((what, "records"))
    dst.expect(want.reshape(-1, image))
    dst.check(what)
    if src is None:
        sbuf.free()
    dst.free()
    info.free()
    return want, recs


def both_parities(efx, dec, s, seed, frames=11):
    """Noise and combed sources (matches of both kinds), top and bottom field first: 11 frames are two whole cycles and a
    partial one."""
    seen = set()
    for srcs in (S.sources(frames, s, seed), T.pulled(frames, s, seed + 1)):
        src = upload_padded(dec, srcs)
        for first_field in ("top", "bottom"):
            seen |= set(run_call(efx, dec, srcs, s, first_field=first_field, src=src)[1]["match"].reshape(-1).tolist())
        src[0].free()
    assert seen == {0, 1}


# the smallest picture; one chunk - 2, + 2; the columns of a wave's strips + 2 (1024: a band that no longer fits one wave;
# and 2048 + 2 for the same on the chroma planes) at height 8; the row band - 4, + 4 at a small width (luma: 32; 64 + 4 for
# the chroma planes' band), where the lanes of one wave walk different bands; two sizes of the host test
SIZES = [(2, 8), (CHUNK - 2, 8), (CHUNK + 2, 8), (TILE + 2, 8), (2 * TILE + 2, 8), (18, BAND - 4), (18, BAND + 4), (18, 2 * BAND + 4),
         (34, 12), (70, 20)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes_both_parities(efx, dec, w, h):
    both_parities(efx, dec, S.layout("i420", w, h), 1000 * w + h)


def test_pitched_planes(efx, dec):
    """720 x 32 with a pitch of 768 and padded plane rows, I420 and YV12 (swapped offsets)."""
    for kind in ("i420", "yv12"):
        s = S.layout(kind, 720, 32, 768, 40)
        assert s.pitch[0] == 768 and 768 * 40 in s.offset
        both_parities(efx, dec, s, 720, frames=6)


@pytest.mark.parametrize("kind,w,h,pitch", [("nv12", 34, 12, 39), ("nv21", 34, 12, 0), ("nv12", TILE + 2, 8, 1031), ("nv12", 960, 8, 0)])
def test_semi_planar(efx, dec, kind, w, h, pitch):
    """NV12 and NV21: rows on every byte phase, a band wider than a wave, and one wide picture."""
    both_parities(efx, dec, S.layout(kind, w, h, pitch), w + len(kind), frames=6)


def test_last_row_ends_near_the_regions_end(efx, dec):
    """Images whose last row ends 8, 13 and 12 bytes before the end of the source region (no pad behind any image): the
    16-byte loads of that row must stay inside and still give its samples."""
    for kind, w, h, pitch in (("i420", 18, 8, 0), ("nv12", 30, 8, 31), ("i420", 34, 12, 0)):
        s = S.layout(kind, w, h, pitch)
        last = max(s.offset[p] + (rows - 1) * s.pitch[p] + n for p, rows, n in s.planes())
        assert 0 < (s.bytes + 15) // 16 * 16 - last < 16
        srcs = T.pulled(6, s, w)
        for first_field in ("top", "bottom"):
            run_call(efx, dec, srcs, s, first_field=first_field, pad=0)


def test_two_streams_do_not_see_each_other(efx, dec):
    s = S.layout("i420", 34, 12)
    srcs = T.pulled(12, s, 11)
    both, recs = run_call(efx, dec, srcs, s, n_streams=2, first_field="bottom")
    alone, alone_recs = M.detelecine(srcs[6:], s, 1, M.BOTTOM)
    assert np.array_equal(both[1], alone[0]) and np.array_equal(recs[1], alone_recs[0])
    assert recs[1]["diff"][0] == M.NO_DIFF and recs[1]["match"][0] == 0


def test_pieces_concatenate_to_the_whole(efx, dec):
    """13 frames as pieces of 5 + 5 + 3 processed frames with one frame of overlap: outputs and records."""
    s = S.layout("nv12", 70, 20, 80)
    title = T.pulled(13, s, 12)
    whole = run_call(efx, dec, title, s)
    parts = [run_call(efx, dec, title[0:5], s), run_call(efx, dec, title[4:10], s, lead=True), run_call(efx, dec, title[9:13], s, lead=True)]
    assert [p[0].shape[1] for p in parts] == [4, 4, 3]
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), whole[0])
    recs, base = [], 0
    for outs, info in parts:
        info = info.copy()
        info["out"][info["out"] >= 0] += base
        base += outs.shape[1]
        recs.append(info)
    assert np.array_equal(np.concatenate(recs, axis=1), whole[1])


def test_short_calls(efx, dec):
    """1-frame and 4-frame calls drop nothing; calls that process one frame behind a lead; five behind a lead drop one."""
    s = S.layout("i420", 18, 8)
    srcs = T.pulled(6, s, 13)
    for first_field in ("top", "bottom"):
        assert run_call(efx, dec, srcs[:1], s, first_field=first_field)[1]["out"].tolist() == [[0]]
        assert run_call(efx, dec, srcs[:4], s, first_field=first_field)[1]["out"].tolist() == [[0, 1, 2, 3]]
        led = run_call(efx, dec, srcs[:2], s, first_field=first_field, lead=True)
        assert led[0].shape[1] == 1 and led[1]["diff"][0, 0] != M.NO_DIFF
        assert sorted(run_call(efx, dec, srcs, s, first_field=first_field, lead=True)[1]["out"][0].tolist()) == [-1, 0, 1, 2, 3]


def test_noise_threshold_extremes(efx, dec):
    s = S.layout("i420", 34, 12)
    srcs = S.sources(6, s, 14)
    assert np.any(run_call(efx, dec, srcs, s, nt=0)[1]["comb_c"] > 0)
    assert not np.any(run_call(efx, dec, srcs, s, nt=255)[1]["comb_c"])


def test_dirty_records_do_not_matter(efx, dec):
    """The record buffer is the kernels' scratch: 0xA5, 0x00 and 0xFF in it before the call give the same records."""
    s = S.layout("nv12", 34, 12, 40)
    srcs = T.pulled(11, s, 15)
    for fill in (0xA5, 0x00, 0xFF):
        run_call(efx, dec, srcs, s, n_streams=1, info_fill=fill)


def test_argument_errors(efx, dec):
    """Every EFX_ERR_ARG case of include/efx.h returns its status and leaves the destination and the records alone."""
    lib = efx.load_library()
    good = S.layout("nv12", 34, 12, 50)
    srcs = S.sources(6, good, 16)
    src, src_stride = upload_padded(dec, srcs)
    image = 34 * 12 * 3 // 2
    dst = Region(dec, 8, image)
    info = Region(dec, 1, 6 * 32)
    ok = dict(n_streams=1, n_frames=6, first_field=0, lead=0, nt=10, src_stride=src_stride, dst_stride=dst.stride)

    def status(s, sp, dp, ip, **kw):
        f = {**ok, **kw}
        o = efx._DetelecineOpts(f["n_streams"], f["n_frames"], f["first_field"], f["lead"], f["nt"], f["src_stride"], f["dst_stride"])
        return lib.efx_detelecine(dec._ctx, C.byref(c_surface(efx, s)) if s is not None else None, C.byref(o), sp, dp, ip)

    P, D, I = src.ptr, dst.buf.ptr, info.buf.ptr
    for what, s in S.rejected_surfaces():
        assert status(s, P, D, I) == ARG, what
        assert lib.efx_last_error(dec._ctx).startswith(b"efx_detelecine: "), what
    words = [S.layout("p010", 34, 12, 74), S.layout("i010", 34, 12, 72)]
    heights = [replace(good, height=10), replace(good, height=6), replace(good, height=4), replace(good, height=2)]
    for s in words + heights:
        assert S.check(s) and not M.accepts(s) and status(s, P, D, I) == ARG, s
    cases = [dict(n_streams=0), dict(n_frames=0), dict(first_field=2), dict(first_field=-1), dict(lead=2), dict(lead=-1),
             dict(lead=1, n_frames=1), dict(nt=-1), dict(nt=256),
             dict(n_streams=1 << 16, n_frames=1 << 15),            # 2^31 images in
             dict(src_stride=good.bytes // 16 * 16), dict(src_stride=src_stride + 8), dict(dst_stride=image // 16 * 16), dict(dst_stride=dst.stride + 8)]
    assert good.bytes % 16 and image % 16
    for kw in cases:
        assert status(good, P, D, I, **kw) == ARG, kw
    for sp, dp, ip in [(None, D, I), (P, None, I), (P, D, None), (P + 8, D, I), (P, D + 4, I), (P, D, I + 8)]:
        assert status(good, sp, dp, ip) == ARG, (sp, dp, ip)
    assert status(None, P, D, I) == ARG
    dec.sync()
    dst.check("after the refused calls")
    info.check("the records after the refused calls")
    assert status(good, P, D, I) == 0
    dec.sync()
    want, recs = M.detelecine(srcs, good, 1)
    dst.expect(want.reshape(-1, image))
    dst.check("the accepted call")
    info.expect(np.frombuffer(recs.tobytes(), dtype=np.uint8)[None, :])
    info.check("the records of the accepted call")
    src.free()
    dst.free()
    info.free()


def test_python_methods(efx, dec):
    """detelecine() on arrays returns the model's pictures and, with info=True, its records; what it returns goes into
    import_pictures() as it is."""
    w, h = 70, 40
    s = S.layout("nv12", w, h, 96, 48)
    srcs = T.pulled(11, s, 17)
    kw = dict(fmt="nv12", width=w, height=h, pitch=96, plane_rows=48)
    want, recs = M.detelecine(srcs, s, 1)
    film = dec.detelecine(srcs, **kw)
    assert isinstance(film, np.ndarray) and film.shape == (9, w * h * 3 // 2) and np.array_equal(film, want[0])
    film, info = dec.detelecine(srcs, info=True, **kw)
    assert np.array_equal(film, want[0]) and info.dtype == efx.TELECINE_INFO == M.INFO and np.array_equal(info, recs)
    assert dec.import_pictures(film, fmt="i420", width=w, height=h).shape == (9, 101376)
    # streams, a lead, the other parity and another threshold through the array method
    want, recs = M.detelecine(srcs[:10], s, 2, M.BOTTOM, 0, 3)
    film, info = dec.detelecine(srcs[:10], n_streams=2, first_field="bff", nt=3, info=True, **kw)
    assert np.array_equal(film, want.reshape(8, -1)) and np.array_equal(info, recs)
    want, recs = M.detelecine(srcs, s, 1, M.TOP, 1)
    film, info = dec.detelecine(srcs, lead=True, info=True, **kw)
    assert np.array_equal(film, want[0]) and np.array_equal(info, recs) and efx.detelecine_count(11, lead=True) == 8
    with pytest.raises(ValueError):
        dec.detelecine(srcs, first_field="first", **kw)
    with pytest.raises(ValueError):
        dec.detelecine(srcs[:1], lead=True, **kw)
    with pytest.raises(ValueError):
        dec.detelecine(srcs, n_streams=2, **kw)


def test_pulldown_comes_back_as_the_film_on_the_device(efx, dec):
    """One cadence case at 34 x 12: the device's outputs and records are the model's, and the film comes back."""
    film = T.film_frames(15, 1)
    video, early = M.telecine(film, T.W, T.H, M.BOTTOM, 1, 2)
    outs, info = dec.detelecine(video, fmt="i420", width=T.W, height=T.H, first_field="bottom", info=True)
    want, recs = M.detelecine_i420(video, T.W, T.H, M.BOTTOM)
    assert np.array_equal(outs, want) and np.array_equal(info[0], recs)
    T.recovered(film, video, early, outs, info[0], 0)


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
        t = torch.from_numpy(S.sources(6, s, 18)).cuda()
        film, info = dec.detelecine(t, fmt=kind, width=w, height=h, first_field="bottom", info=True)
        only = dec.detelecine(t, fmt=kind, width=w, height=h, first_field="bottom")
        assert all(isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.uint8 for o in (film, only))
        assert tuple(film.shape) == (5, w * h * 3 // 2) and torch.equal(film, only) and isinstance(info, np.ndarray)
        pics = dec.import_pictures(film, fmt="i420", width=w, height=h)
        assert tuple(pics.shape) == (5, 101376)
        out.append((film.cpu().numpy(), info))
    dec.close()
    pickle.dump(out, open(sys.argv[2], "wb"))
    print("detelecine ok")
""")


def test_tensor_in_tensor_out(efx, tmp_path):
    """A tensor in, a tensor out on the device (a process of its own: torch's HIP runtime first)."""
    script, out = tmp_path / "telecine_tensor.py", tmp_path / "out.pkl"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "detelecine ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = pickle.load(open(out, "rb"))
    for (film, info), (kind, w, h) in zip(got, (("i420", 64, 48), ("nv12", 18, 8))):
        s = S.layout(kind, w, h)
        want, recs = M.detelecine(S.sources(6, s, 18), s, 1, M.BOTTOM)
        assert np.array_equal(film, want[0]) and np.array_equal(info, recs)
