"""efx_detect_scan (k_scan.hip) on the device against tests/scan_model.py, byte for byte, frame records and stream records, on
padded regions whose fill bytes must survive: every size at which the kernel takes another path, with and without a
lead, pitched planes, NV12 / NV21, a last row near the region's end, streams, accumulated pieces against the whole, a
dirty frame-record buffer, every refused argument, the Python methods, the material the rule is for, and
import_pictures(deinterlace="auto")."""
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

import scan_model as M
import surface_model as S
import test_scan_model as T
from test_gpu_telecine import ARG, FILL, PAD, Region, c_surface, upload_padded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, STRIPS, BAND = T.CHUNK, T.STRIPS, T.BAND
KINDS = {M.IS_UNKNOWN: "unknown", M.IS_PROGRESSIVE: "progressive", M.IS_INTERLACED: "interlaced", M.IS_TELECINED: "telecined"}
FIELDS = {None: None, M.TOP: "top", M.BOTTOM: "bottom"}


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
    text = open(os.path.join(ROOT, "espflix_amd", "csrc", "scan_px.h")).read()
    value = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    assert "kChunk = tpx::kChunk;" in text and "kChunk = dpx::kChunk;" in open(os.path.join(ROOT, "espflix_amd", "csrc", "telecine_px.h")).read()
    assert "kChunk = 16;" in open(os.path.join(ROOT, "espflix_amd", "csrc", "deint_px.h")).read()
    assert (CHUNK, value("kWaveStrips"), value("kBandRows"), value("kCycle")) == (16, STRIPS, BAND, 5)


def run_call(efx, dec, srcs, s, n_streams=1, lead=False, first_frame=0, recs=None, src=None, frames_fill=FILL, pad=PAD, **opts):
    """One call on padded regions against the model; returns the model's (frame records (n_streams, n), records
    (n_streams,)).  recs: what the record buffer holds before the call, to be added to."""
    o = {**M.DEFAULTS, **opts}
    what = (s.width, s.height, s.layout, lead, first_frame, o)
    want_f, want_r = M.scan(srcs, s, n_streams, int(lead), first_frame, recs, **o)
    sbuf, src_stride = src or upload_padded(dec, srcs, pad)
    # the records lie one behind the other; one region item holds them all, the pad behind it must survive
    fr = Region(dec, 1, want_f.size * 48, fill=frames_fill)
    rr = Region(dec, 1, n_streams * 64)
    if recs is not None:
        before = rr.want.copy()
        before[0, :n_streams * 64] = np.frombuffer(np.asarray(recs, dtype=M.REC).tobytes(), dtype=np.uint8)
        rr.buf.upload(before.reshape(-1))
    got = dec.detect_scan_to(sbuf, fr.buf, rr.buf, surface=c_surface(efx, s), n_streams=n_streams, n_frames=len(srcs) // n_streams, lead=lead,
                             first_frame=first_frame, accumulate=recs is not None, src_stride=src_stride, **o)
    dec.sync()
    assert got == want_f.shape[1], what
    fr.expect(np.frombuffer(want_f.tobytes(), dtype=np.uint8)[None, :])
    fr.check((what, "frame records"))
    rr.expect(np.frombuffer(want_r.tobytes(), dtype=np.uint8)[None, :])
    rr.check((what, "stream records"))
    if src is None:
        sbuf.free()
    fr.free()
    rr.free()
    return want_f, want_r


def with_and_without_lead(efx, dec, s, seed, frames=6):
    """Noise and directed sources (every label but UNDETERMINED within 7 frames; noise gives that one), 2 to 6 frames."""
    for srcs in (S.sources(3, s, seed), T.directed(frames, s, seed + 1)):
        src = upload_padded(dec, srcs)
        for lead in (False, True):
            run_call(efx, dec, srcs, s, lead=lead, first_frame=3, src=src)
        src[0].free()


# the smallest picture; one chunk - 2, + 2; the columns of a wave's 64 strips + 2 (a band that no longer fits one wave) at
# height 8; the row band - 4, + 4 and twice the band + 4 at a small width, where the lanes of one wave walk different bands;
# two sizes of the host test
SIZES = [(2, 8), (CHUNK - 2, 8), (CHUNK + 2, 8), (STRIPS * CHUNK + 2, 8), (18, BAND - 4), (18, BAND + 4), (18, 2 * BAND + 4), (34, 12), (70, 20)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes(efx, dec, w, h):
    with_and_without_lead(efx, dec, S.layout("i420", w, h), 1000 * w + h)


def test_pitched_planes(efx, dec):
    """720 x 32 with a pitch of 768 and padded plane rows, I420 and YV12 (swapped offsets)."""
    for kind in ("i420", "yv12"):
        s = S.layout(kind, 720, 32, 768, 40)
        assert s.pitch[0] == 768 and 768 * 40 in s.offset
        with_and_without_lead(efx, dec, s, 720, frames=4)


@pytest.mark.parametrize("kind,w,h,pitch", [("nv12", 34, 12, 39), ("nv21", 34, 12, 0), ("nv12", STRIPS * CHUNK + 2, 8, 1031)])
def test_semi_planar(efx, dec, kind, w, h, pitch):
    """NV12 with an odd pitch (rows on every byte phase) and NV21, and a band wider than a wave."""
    with_and_without_lead(efx, dec, S.layout(kind, w, h, pitch), w + len(kind))


def test_last_row_ends_near_the_regions_end(efx, dec):
    """Images whose last row ends 8, 13 and 12 bytes before the end of the source region (no pad behind any image): the
    16-byte loads of that row must stay inside and still give its samples."""
    for kind, w, h, pitch in (("i420", 18, 8, 0), ("nv12", 30, 8, 31), ("i420", 34, 12, 0)):
        s = S.layout(kind, w, h, pitch)
        last = max(s.offset[p] + (rows - 1) * s.pitch[p] + n for p, rows, n in s.planes())
        assert 0 < (s.bytes + 15) // 16 * 16 - last < 16
        run_call(efx, dec, T.directed(6, s, w), s, pad=0)


def test_two_streams_do_not_see_each_other(efx, dec):
    s = S.layout("i420", 34, 12)
    srcs = np.concatenate([T.directed(6, s, 11), T.directed(13, s, 12)[7:]])
    frames, recs = run_call(efx, dec, srcs, s, n_streams=2, first_frame=2)
    alone = M.scan(srcs[6:], s, 1, 0, 2)
    assert np.array_equal(frames[1], alone[0][0]) and np.array_equal(recs[1:], alone[1]) and frames[1, 0]["label"] == M.NONE
    assert frames[1, 0]["comb"] == 0 and not np.array_equal(recs[:1], recs[1:])


def test_accumulated_pieces_equal_one_call(efx, dec):
    """13 frames as pieces of any length with one frame of overlap, each adding to the record of the one before, from a
    first_frame that is no multiple of 5: the frame records and the final counts, phases included, are the whole's."""
    s = S.layout("nv12", 70, 20, 80)
    title = T.directed(13, s, 12)
    whole = run_call(efx, dec, title, s, first_frame=7)
    assert whole[1][0]["rep_top"].sum() and whole[1][0]["rep_bottom"].sum()
    frames, recs = [], None
    for a, b in ((0, 4), (3, 5), (4, 11), (10, 13)):
        f, recs = run_call(efx, dec, title[a:b], s, lead=a > 0, first_frame=7 + a, recs=recs)
        frames.append(f)
    assert np.array_equal(np.concatenate(frames, axis=1), whole[0]) and np.array_equal(recs, whole[1])
    assert not np.array_equal(run_call(efx, dec, title, s, first_frame=8)[1], whole[1])   # (the phases do move with first_frame)


def test_dirty_frame_records_do_not_matter(efx, dec):
    """The frame records are the kernels' scratch: 0xA5, 0x00 and 0xFF in them before the call give the same records."""
    s = S.layout("nv12", 34, 12, 40)
    srcs = T.directed(6, s, 15)
    for fill in (0xA5, 0x00, 0xFF):
        run_call(efx, dec, srcs, s, frames_fill=fill)


def test_option_extremes(efx, dec):
    s = S.layout("i420", 34, 12)
    srcs = T.directed(6, s, 14)
    src = upload_padded(dec, srcs)
    for name, (lo, hi) in M.RANGES.items():
        for v in (lo, hi):
            run_call(efx, dec, srcs, s, src=src, **{name: v})
    src[0].free()


def test_argument_errors(efx, dec):
    """Every EFX_ERR_ARG case of include/efx.h returns its status and leaves both record buffers alone."""
    lib = efx.load_library()
    good = S.layout("nv12", 34, 12, 50)
    srcs = S.sources(6, good, 16)
    src, src_stride = upload_padded(dec, srcs)
    fr = Region(dec, 1, 6 * 48)
    rr = Region(dec, 1, 64)
    ok = dict(n_streams=1, n_frames=6, lead=0, accumulate=0, **M.DEFAULTS, reserved=0, first_frame=0, src_stride=src_stride)

    def status(s, sp, fp, rp, **kw):
        o = np.zeros(1, dtype=efx.SCAN_OPTS_DTYPE)
        for k, v in {**ok, **kw}.items():
            o[k] = v
        return lib.efx_detect_scan(dec._ctx, C.byref(c_surface(efx, s)) if s is not None else None, o.ctypes.data, sp, fp, rp)

    P, F, R = src.ptr, fr.buf.ptr, rr.buf.ptr
    for what, s in S.rejected_surfaces():
        assert status(s, P, F, R) == ARG, what
        assert lib.efx_last_error(dec._ctx).startswith(b"efx_detect_scan: "), what
    words = [S.layout("p010", 34, 12, 74), S.layout("i010", 34, 12, 72)]
    heights = [replace(good, height=10), replace(good, height=6), replace(good, height=4), replace(good, height=2)]
    for s in words + heights:
        assert S.check(s) and not M.accepts(s) and status(s, P, F, R) == ARG, s
    cases = [dict(n_streams=0), dict(n_frames=0), dict(lead=2), dict(lead=-1), dict(lead=1, n_frames=1), dict(accumulate=2), dict(accumulate=-1),
             dict(n_streams=1 << 16, n_frames=1 << 15),            # 2^31 images in
             dict(src_stride=good.bytes // 16 * 16), dict(src_stride=src_stride + 8)]
    cases += [{name: v} for name, (lo, hi) in M.RANGES.items() for v in (lo - 1, hi + 1)]
    assert good.bytes % 16 and len(cases) == 20
    for kw in cases:
        assert status(good, P, F, R, **kw) == ARG, kw
    for sp, fp, rp in [(None, F, R), (P, None, R), (P, F, None), (P + 8, F, R), (P, F + 8, R), (P, F, R + 8)]:
        assert status(good, sp, fp, rp) == ARG, (sp, fp, rp)
    assert status(None, P, F, R) == ARG and lib.efx_detect_scan(dec._ctx, C.byref(c_surface(efx, good)), None, P, F, R) == ARG
    dec.sync()
    fr.check("the frame records after the refused calls")
    rr.check("the stream records after the refused calls")
    assert status(good, P, F, R) == 0
    dec.sync()
    want_f, want_r = M.scan(srcs, good, 1)
    fr.expect(np.frombuffer(want_f.tobytes(), dtype=np.uint8)[None, :])
    fr.check("the frame records of the accepted call")
    rr.expect(np.frombuffer(want_r.tobytes(), dtype=np.uint8)[None, :])
    rr.check("the stream records of the accepted call")
    src.free()
    fr.free()
    rr.free()


@pytest.fixture(scope="module")
def cases():
    """The material of the host test at noise +-3, and its still picture at +-6: computed once."""
    return T.semantic_cases(3) + [c for c in T.semantic_cases(6) if c[0] == "still"]


def test_material_gets_its_verdict_on_the_device(efx, dec, cases):
    """Decoder.detect_scan on the definition's cases, all as streams of one call: the model's records, the required
    verdicts."""
    s = S.layout("i420", T.W, T.H)
    srcs = np.concatenate([M.with_chroma(l) for _, l, _ in cases])
    results, frames = dec.detect_scan(srcs, fmt="i420", width=T.W, height=T.H, n_streams=len(cases), frames=True, **M.DEFAULTS)
    want_f, want_r = M.scan(srcs, s, len(cases))
    assert frames.dtype == efx.SCAN_FRAME_DTYPE and np.array_equal(frames, want_f)
    for (name, _, (kind, first)), res, r in zip(cases, results, want_r):
        assert isinstance(res, efx.ScanResult) and res.rec.tobytes() == r.tobytes(), name
        assert (res.kind, res.first_field) == (KINDS[kind], FIELDS[first]), (name, res)


def test_python_methods(efx, dec):
    """Pieces through detect_scan(recs=) equal the whole; a pitched NV12 surface; refused arguments raise."""
    w, h = 70, 20
    s = S.layout("nv12", w, h, 96, 24)
    srcs = T.directed(13, s, 17)
    kw = dict(fmt="nv12", width=w, height=h, pitch=96, plane_rows=24)
    want_f, want_r = M.scan(srcs, s, 1, 0, 4)
    whole = dec.detect_scan(srcs, first_frame=4, **kw)
    assert len(whole) == 1 and whole[0].rec.tobytes() == want_r[0].tobytes() and (whole[0].kind, whole[0].first_field) == (
        KINDS[M.verdict(want_r[0])[0]], FIELDS[M.verdict(want_r[0])[1]])
    first = dec.detect_scan(srcs[:6], first_frame=4, **kw)
    rest, frames = dec.detect_scan(srcs[5:], first_frame=9, lead=True, recs=first, frames=True, **kw)
    assert rest[0].rec.tobytes() == want_r[0].tobytes() and np.array_equal(frames, want_f[:, 6:])   # (frame 5 is the lead)
    again = dec.detect_scan(srcs[5:], first_frame=9, lead=True, recs=np.array([first[0].rec]), nt=3, **kw)
    assert again[0].rec.tobytes() == M.scan(srcs[5:], s, 1, 1, 9, [first[0].rec], nt=3)[1][0].tobytes()
    with pytest.raises(ValueError):
        dec.detect_scan(srcs[:1], lead=True, **kw)
    with pytest.raises(ValueError):
        dec.detect_scan(srcs, n_streams=2, **kw)
    with pytest.raises(ValueError):
        dec.detect_scan(srcs, recs=[first[0], first[0]], **kw)
    with pytest.raises(efx.EfxError):
        dec.detect_scan(srcs, still=5000, **kw)


def test_import_pictures_deinterlace_auto(efx, dec, cases):
    """deinterlace="auto": the interlaced case is imported as deinterlace= its order, the progressive and the still one
    as None, and pulldown raises, naming detelecine()."""
    by_name = {name: M.with_chroma(l) for name, l, _ in cases}
    kw = dict(fmt="i420", width=T.W, height=T.H)
    for name, order in (("interlaced tff", "tff"), ("interlaced bff", "bff"), ("progressive", None)):
        src = by_name[name][:8]
        got = dec.import_pictures(src, deinterlace="auto", **kw)
        assert np.array_equal(got, dec.import_pictures(src, deinterlace=order, **kw)), name
        other = dec.import_pictures(src, deinterlace="bff" if order != "bff" else "tff", **kw)
        assert not np.array_equal(got, other), name
    still = [l for name, l, _ in cases if name == "still"][0]
    assert np.array_equal(dec.import_pictures(M.with_chroma(still), deinterlace="auto", **kw), dec.import_pictures(M.with_chroma(still), **kw))
    assert np.array_equal(dec.import_pictures(by_name["progressive"][:1], deinterlace="auto", **kw), dec.import_pictures(by_name["progressive"][:1], **kw))
    with pytest.raises(ValueError, match=r"detelecine\(first_field='bottom'\)"):
        dec.import_pictures(by_name["pulldown bff phase 2"], deinterlace="auto", **kw)
    with pytest.raises(ValueError):
        dec.import_pictures(by_name["progressive"], deinterlace="auto", field_rate=True, **kw)


TORCH_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import surface_model as S
    import test_scan_model as T

    out = []
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device())
    for kind, w, h in (("i420", 64, 48), ("nv12", 18, 8)):   # 4608 bytes a picture: packed rows of 16; 216: padded
        s = S.layout(kind, w, h)
        t = torch.from_numpy(T.directed(6, s, 18)).cuda()
        results, frames = dec.detect_scan(t, fmt=kind, width=w, height=h, first_frame=1, frames=True)
        assert isinstance(frames, np.ndarray) and frames.shape == (1, 6) and len(results) == 1
        out.append((frames, results[0].rec, results[0].kind, results[0].first_field))
    dec.close()
    pickle.dump(out, open(sys.argv[2], "wb"))
    print("detect_scan ok")
""")


def test_tensor_in(efx, tmp_path):
    """A tensor in, records out (a process of its own: torch's HIP runtime first)."""
    script, out = tmp_path / "scan_tensor.py", tmp_path / "out.pkl"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "detect_scan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = pickle.load(open(out, "rb"))
    for (frames, rec, kind, first), (k, w, h) in zip(got, (("i420", 64, 48), ("nv12", 18, 8))):
        s = S.layout(k, w, h)
        want_f, want_r = M.scan(T.directed(6, s, 18), s, 1, 0, 1)
        assert np.array_equal(frames, want_f) and rec.tobytes() == want_r[0].tobytes()
        assert (kind, first) == (KINDS[M.verdict(want_r[0])[0]], FIELDS[M.verdict(want_r[0])[1]])
