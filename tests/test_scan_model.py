"""The rule of efx_detect_scan: whole calls on the host through espflix_amd/csrc/scan_px.h with the kernel's own walk
(tests/scan_model_main.cpp, built here with the host compiler, once plain and once under the address and
undefined-behaviour sanitizers) against the NumPy model of include/efx.h's definition (tests/scan_model.py), every branch
of the label, the repeat and the verdict at its boundary, the record dtypes against the header, and what the rule is for:
synthetic progressive, interlaced, still and 2-3 pulldown material gets the right verdict.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import scan_model as M
import surface_model as S
import telecine_model as TM
from test_denoise_model import surfaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, STRIPS, BAND = 16, 64, 32   # scan_px.h: kChunk, kWaveStrips, kBandRows
# widths 2, chunk - 2, chunk + 2 and one of more than 64 strips at height 8; heights 8, band - 4, band + 4, 2 band + 4 at a
# small width, where the lanes of one wave walk different bands; two middling sizes
SIZES = [(2, 8), (CHUNK - 2, 8), (CHUNK + 2, 8), (STRIPS * CHUNK + 2, 8), (18, BAND - 4), (18, BAND + 4), (18, 2 * BAND + 4), (34, 12), (70, 20)]
OPTS = M.DEFAULTS


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build scan_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "scan_model_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("scan_px_san"), "drv_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("scan_px_plain"), "drv", [])


def host_call(exe, srcs, s, n_streams=1, lead=0, first_frame=0, recs=None, accumulate=None, **opts):
    """One call of the host program: (frame records (n_streams, n), records (n_streams,)), or the exit status of a refused
    call.  recs: what the record buffer holds before the call; it is added to unless accumulate=0."""
    o = {**OPTS, **opts}
    n_frames = len(srcs) // n_streams
    acc = (0 if recs is None else 1) if accumulate is None else accumulate
    before = np.full(n_streams, 0xA5A5A5A5, dtype="<u4").repeat(16).view(M.REC) if recs is None else np.asarray(recs, dtype=M.REC)
    r = subprocess.run([exe, "call", *[str(v) for v in s.args()], str(n_streams), str(n_frames), str(lead), str(acc),
                        *[str(o[k]) for k in ("nt", "still", "prog", "intl", "rep")], str(first_frame)],
                       input=np.ascontiguousarray(srcs).tobytes() + before.tobytes(), capture_output=True, timeout=300)
    if r.returncode:
        assert r.returncode == 1, r.stderr[-3000:]
        return r.returncode
    n = n_frames - lead
    assert len(r.stdout) == n_streams * (n * 48 + 64)
    return (np.frombuffer(r.stdout[:n_streams * n * 48], dtype=M.FRAME).reshape(n_streams, n),
            np.frombuffer(r.stdout[n_streams * n * 48:], dtype=M.REC))


def same(got, want):
    return not isinstance(got, int) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


# (field period of the top field, of the bottom field) of the frames of `directed`: a progressive step, two frames top field
# first, two bottom field first, a still frame, a repeated top field, a repeated bottom field, and some of it again
TIMES = [(0, 0), (2, 2), (4, 5), (6, 7), (9, 8), (11, 10), (11, 10), (11, 12), (13, 12), (14, 14), (16, 17), (18, 19), (20, 20)]


def directed(n, s, seed):
    """n <= 13 source images of one stream in which every label and every repeat occurs (at middling sizes): a texture
    (scan_model.scene's) that pans 3 pels per field period, each field taken at its time of TIMES, with noise of +-1.  Chroma and padding are
    noise."""
    srcs = S.sources(n, s, seed)
    rng = np.random.default_rng(seed + 1)
    x = np.arange(s.width, dtype=np.float64)
    for i in range(n):
        for r in range(s.height):
            k = TIMES[i][r & 1]
            xk = x + 3 * k
            v = 110 + 40 * np.sin(2 * np.pi * xk / 13 + 0.7) + 25 * np.cos(2 * np.pi * (xk + 3 * r) / 29 + 0.3) + 15 * np.sin(2 * np.pi * (r - xk / 2) / 7 + 1.9)
            at = s.offset[0] + r * s.pitch[0]
            srcs[i, at:at + s.width] = np.rint(v) + rng.integers(-1, 2, s.width)
    return srcs


def test_every_label_and_repeat_occurs():
    """The sources of the tests below exercise every branch (else part of the rule would go unchecked)."""
    s = S.layout("i420", 70, 20)
    frames = M.scan(directed(13, s, 70), s)[0][0]
    assert set(frames["label"].tolist()) == {M.NONE, M.STILL, M.PROGRESSIVE, M.TFF, M.BFF, M.UNDETERMINED}
    assert set(frames["repeat"].tolist()) == {M.REPEAT_NONE, M.REPEAT_TOP, M.REPEAT_BOTTOM}
    assert set(frames["label"][:7].tolist()) >= {M.NONE, M.STILL, M.PROGRESSIVE, M.TFF, M.BFF}   # (the first 7 serve the sizes)


@pytest.mark.parametrize("w,h", SIZES)
def test_header_matches_model(sanitized, w, h):
    """Every layout, noise and directed sources, with and without a lead: the header's walk writes what the definition
    says, bit for bit, and the sanitizers see no access outside the block."""
    for k, (name, s) in enumerate(surfaces(w, h)):
        assert s is not None and M.accepts(s), name
        for srcs in (S.sources(5, s, 100 * w + k), directed(7, s, 200 * w + k)):
            for lead in (0, 1):
                got = host_call(sanitized, srcs, s, 1, lead, first_frame=3)
                assert same(got, M.scan(srcs, s, 1, lead, 3)), (name, lead)


def test_plain_build_agrees(plain, sanitized):
    s = S.layout("nv12", 70, 20, 75)
    srcs = directed(13, s, 5)
    got = host_call(plain, srcs, s, 1, 0, 7)
    assert same(got, M.scan(srcs, s, 1, 0, 7)) and same(got, host_call(sanitized, srcs, s, 1, 0, 7))
    r = subprocess.run([plain, "tile"], capture_output=True, text=True, check=True)
    assert [int(v) for v in r.stdout.split()] == [CHUNK, STRIPS, BAND, 5]


def test_option_extremes(sanitized):
    s = S.layout("i420", 34, 12)
    srcs = directed(13, s, 9)
    for name, (lo, hi) in M.RANGES.items():
        for v in (lo, hi):
            got = host_call(sanitized, srcs, s, **{name: v})
            assert same(got, M.scan(srcs, s, **{name: v})), (name, v)
        assert host_call(sanitized, srcs, s, **{name: lo - 1}) == 1 and host_call(sanitized, srcs, s, **{name: hi + 1}) == 1
    nt255 = host_call(sanitized, srcs, s, nt=255)[0]
    assert not np.any(nt255["comb"]) and not np.any(nt255["comb_tb"]) and np.any(nt255["diff_top"])   # v - 1530 <= 0
    assert set(host_call(sanitized, srcs, s, still=0)[0]["label"][0].tolist()) & {M.STILL} == set()
    assert set(host_call(sanitized, srcs, s, still=4080)[0]["label"][0, 1:].tolist()) == {M.STILL}    # 16 x 255 w h


# (cc, ctb, cbt, dt, db) at w x h = 16 x 16 with still 64 (16 (dt + db) < 16384), prog 384, intl 266, rep 768: each test one
# count either side of its boundary
BRANCHES = [
    ((0, 0, 0, 511, 512), (M.STILL, 0)), ((0, 0, 0, 0, 1023), (M.STILL, 0)),        # a still frame has no repeat
    ((0, 0, 0, 512, 512), (M.UNDETERMINED, 0)),                                     # 16 x 1024 = 16384: not still; all combs 0
    ((2, 3, 9, 512, 512), (M.TFF, 0)),                                              # 256 x 3 = 384 x 2: not progressive
    ((2, 4, 3, 512, 512), (M.BFF, 0)),                                              # min is cbt = 3
    ((2, 4, 4, 512, 512), (M.PROGRESSIVE, 0)), ((2, 9, 4, 512, 512), (M.PROGRESSIVE, 0)),
    ((0, 1, 1, 512, 512), (M.PROGRESSIVE, 0)),
    ((1000, 128, 133, 512, 512), (M.UNDETERMINED, 0)),                              # 256 x 133 = 266 x 128
    ((1000, 128, 134, 512, 512), (M.TFF, 0)), ((1000, 133, 128, 512, 512), (M.UNDETERMINED, 0)), ((1000, 134, 128, 512, 512), (M.BFF, 0)),
    ((1000, 0, 1, 512, 512), (M.TFF, 0)), ((1000, 1, 0, 512, 512), (M.BFF, 0)),
    ((2, 4, 4, 400, 1200), (M.PROGRESSIVE, 0)), ((2, 4, 4, 400, 1201), (M.PROGRESSIVE, M.REPEAT_TOP)),   # 768 x 400 = 256 x 1200
    ((2, 4, 4, 1200, 400), (M.PROGRESSIVE, 0)), ((2, 4, 4, 1201, 400), (M.PROGRESSIVE, M.REPEAT_BOTTOM)),
    ((1000, 128, 134, 0, 1024), (M.TFF, M.REPEAT_TOP)), ((1000, 128, 133, 1024, 0), (M.UNDETERMINED, M.REPEAT_BOTTOM)),
    ((1530 << 24, 1530 << 24, 1530 << 24, 255 << 23, 255 << 23), (M.UNDETERMINED, 0)),   # the largest sums: no product overflows
]


@pytest.mark.parametrize("five,want", BRANCHES)
def test_label_and_repeat_branches(sanitized, five, want):
    w, h = (4096, 4096) if five[0] >> 30 else (16, 16)
    r = subprocess.run([sanitized, "label", *[str(v) for v in five], str(w), str(h), *[str(OPTS[k]) for k in ("still", "prog", "intl", "rep")]],
                       capture_output=True, text=True, check=True)
    assert tuple(int(v) for v in r.stdout.split()) == want == M.label(five, w, h, **OPTS)


def test_sums_are_detelecines(sanitized):
    """cc / ctb / dt are efx_detelecine's comb_c / comb_p / diff for first_field TOP, cc / cbt / db for BOTTOM."""
    s = S.layout("nv21", 34, 12)
    srcs = directed(11, s, 12)
    frames = host_call(sanitized, srcs, s)[0][0]
    for first_field, comb, diff in ((TM.TOP, "comb_tb", "diff_top"), (TM.BOTTOM, "comb_bt", "diff_bottom")):
        info = TM.detelecine(srcs, s, 1, first_field, 0, OPTS["nt"])[1][0]
        assert np.array_equal(frames["comb"][1:], info["comb_c"][1:])
        assert np.array_equal(frames[comb][1:], info["comb_p"][1:]) and np.array_equal(frames[diff][1:], info["diff"][1:])
    assert frames[0].tolist() == (0, 0, 0, 0, 0, M.NONE, 0)


def test_streams_and_pieces(sanitized):
    """Two streams do not see each other; pieces of any length with one frame of overlap, accumulated, equal the whole,
    with a first_frame that is no multiple of 5; without accumulate a dirty record is overwritten, with it added to."""
    s = S.layout("nv12", 34, 12, 40)
    srcs = np.concatenate([directed(6, s, 7), directed(13, s, 8)[7:]])
    two = host_call(sanitized, srcs, s, 2, first_frame=2)
    assert same(two, M.scan(srcs, s, 2, 0, 2))
    alone = M.scan(srcs[6:], s, 1, 0, 2)
    assert np.array_equal(two[0][1], alone[0][0]) and np.array_equal(two[1][1:], alone[1]) and two[0][1, 0]["label"] == M.NONE
    title = directed(13, s, 9)
    whole = host_call(sanitized, title, s, first_frame=7)
    assert whole[1][0]["rep_top"].sum() and whole[1][0]["rep_bottom"].sum()
    frames, recs = [], None
    for a, b in ((0, 4), (3, 5), (4, 11), (10, 13)):
        f, recs = host_call(sanitized, title[a:b], s, 1, 1 if a else 0, 7 + a, recs)
        frames.append(f)
    assert np.array_equal(np.concatenate(frames, axis=1), whole[0]) and np.array_equal(recs, whole[1])
    dirty = np.frombuffer(np.arange(16, dtype="<u4").tobytes(), dtype=M.REC)
    assert np.array_equal(host_call(sanitized, title, s, 1, 0, 7, dirty, accumulate=0)[1], whole[1])
    added = host_call(sanitized, title, s, 1, 0, 7, dirty)
    assert same(added, M.scan(title, s, 1, 0, 7, dirty)) and added[1][0]["reserved"] == 0 and added[1][0]["n_still"] == whole[1][0]["n_still"]


def test_refusals(sanitized):
    ok = S.layout("i420", 18, 8)
    srcs = S.sources(2, ok, 3)
    assert host_call(sanitized, srcs, S.layout("i420", 18, 10)) == 1   # height not a multiple of 4
    assert host_call(sanitized, srcs, S.layout("i420", 18, 4)) == 1    # below 8
    assert host_call(sanitized, srcs, S.layout("p010", 18, 8)) == 1    # a 16-bit layout
    assert host_call(sanitized, srcs, ok, lead=2) == 1 and host_call(sanitized, srcs[:1], ok, lead=1) == 1
    assert host_call(sanitized, srcs, ok, accumulate=2) == 1 and host_call(sanitized, srcs, ok, accumulate=-1) == 1
    assert not isinstance(host_call(sanitized, srcs, ok, lead=1), int)


def rec(n_still=0, n_prog=0, n_tff=0, n_bff=0, n_undet=0, top=(0, 0, 0, 0, 0), bot=(0, 0, 0, 0, 0)):
    r = np.zeros((), dtype=M.REC)
    r["n_still"], r["n_prog"], r["n_tff"], r["n_bff"], r["n_undet"] = n_still, n_prog, n_tff, n_bff, n_undet
    r["rep_top"], r["rep_bottom"] = top, bot
    return r


T, B = M.TOP, M.BOTTOM
VERDICTS = [
    (rec(), (M.IS_UNKNOWN, None)), (rec(n_still=50), (M.IS_UNKNOWN, None)), (rec(n_undet=9), (M.IS_UNKNOWN, None)),
    # telecined: m >= 4, both repeats seen, 4 m >= 3 tot, 5 m >= n_moving, the gap 2 or 3
    (rec(n_prog=20, top=(2, 0, 0, 0, 0), bot=(0, 0, 2, 0, 0)), (M.IS_TELECINED, T)),
    (rec(n_prog=20, top=(2, 0, 0, 0, 0), bot=(0, 0, 0, 2, 0)), (M.IS_TELECINED, B)),
    (rec(n_prog=20, top=(0, 0, 0, 2, 0), bot=(2, 0, 0, 0, 0)), (M.IS_TELECINED, T)),    # (0 - 3) mod 5 = 2
    (rec(n_prog=20, top=(0, 0, 0, 2, 0), bot=(0, 2, 0, 0, 0)), (M.IS_TELECINED, B)),    # (1 - 3) mod 5 = 3
    (rec(n_prog=20, top=(2, 0, 0, 0, 0), bot=(0, 2, 0, 0, 0)), (M.IS_PROGRESSIVE, None)),   # gap 1
    (rec(n_prog=20, top=(2, 0, 0, 0, 0), bot=(0, 0, 0, 0, 2)), (M.IS_PROGRESSIVE, None)),   # gap 4
    (rec(n_prog=20, top=(2, 0, 0, 0, 0), bot=(2, 0, 0, 0, 0)), (M.IS_PROGRESSIVE, None)),   # gap 0
    (rec(n_prog=20, top=(2, 0, 0, 0, 0), bot=(0, 0, 1, 0, 0)), (M.IS_PROGRESSIVE, None)),   # m = 3
    (rec(n_prog=20, top=(4, 0, 0, 0, 0), bot=(0, 0, 0, 0, 0)), (M.IS_PROGRESSIVE, None)),   # no bottom repeat
    (rec(n_prog=20, top=(0, 0, 0, 0, 0), bot=(0, 0, 4, 0, 0)), (M.IS_PROGRESSIVE, None)),   # no top repeat
    (rec(n_prog=20, top=(3, 0, 0, 0, 0), bot=(0, 0, 1, 0, 0)), (M.IS_TELECINED, T)),
    (rec(n_prog=20, top=(3, 1, 0, 0, 0), bot=(0, 0, 3, 1, 0)), (M.IS_TELECINED, T)),        # 4 x 6 = 3 x 8
    (rec(n_prog=20, top=(3, 1, 1, 0, 0), bot=(0, 0, 3, 1, 0)), (M.IS_PROGRESSIVE, None)),   # 4 x 6 < 3 x 9
    (rec(n_prog=20, top=(2, 2, 0, 0, 0), bot=(0, 0, 0, 4, 0)), (M.IS_TELECINED, B)),        # a tie takes the lowest phase: pt = 0
    (rec(n_prog=20, top=(0, 4, 0, 0, 0), bot=(2, 0, 0, 2, 0)), (M.IS_PROGRESSIVE, None)),   # pb = 0: gap 4; 4 x 6 = 3 x 8
    (rec(n_prog=12, n_tff=8, top=(2, 0, 0, 0, 0), bot=(0, 0, 2, 0, 0)), (M.IS_TELECINED, T)),      # 5 x 4 = 20
    (rec(n_prog=12, n_tff=8, n_undet=1, top=(2, 0, 0, 0, 0), bot=(0, 0, 2, 0, 0)), (M.IS_PROGRESSIVE, None)),   # 5 x 4 < 21
    (rec(n_still=100, n_prog=12, n_tff=8, top=(2, 0, 0, 0, 0), bot=(0, 0, 2, 0, 0)), (M.IS_TELECINED, T)),    # still frames do not move
    # interlaced: the ordered frames outnumber the progressive ones, and one order leads four to one
    (rec(n_tff=1), (M.IS_INTERLACED, T)), (rec(n_bff=1), (M.IS_INTERLACED, B)),
    (rec(n_prog=5, n_tff=6), (M.IS_INTERLACED, T)), (rec(n_prog=6, n_tff=6), (M.IS_PROGRESSIVE, None)),
    (rec(n_prog=7, n_tff=6), (M.IS_PROGRESSIVE, None)),
    (rec(n_tff=8, n_bff=2), (M.IS_INTERLACED, T)), (rec(n_tff=2, n_bff=8), (M.IS_INTERLACED, B)),
    (rec(n_tff=7, n_bff=2), (M.IS_UNKNOWN, None)), (rec(n_tff=2, n_bff=7), (M.IS_UNKNOWN, None)), (rec(n_tff=7, n_bff=5), (M.IS_UNKNOWN, None)),
    (rec(n_tff=3, n_bff=3), (M.IS_UNKNOWN, None)),
    (rec(n_prog=1), (M.IS_PROGRESSIVE, None)), (rec(n_prog=9, n_tff=7, n_bff=2), (M.IS_PROGRESSIVE, None)),
    (rec(n_prog=8, n_tff=7, n_bff=2), (M.IS_UNKNOWN, None)),
    (rec(n_prog=0xFFFFFFFF, n_tff=0xFFFFFFFF, n_bff=0xFFFFFFFF, n_undet=0xFFFFFFFF, top=(0xFFFFFFFF,) * 5, bot=(0xFFFFFFFF,) * 5), (M.IS_UNKNOWN, None)),
]


@pytest.mark.parametrize("k", range(len(VERDICTS)))
def test_verdict(sanitized, k):
    r, want = VERDICTS[k]
    out = subprocess.run([sanitized, "verdict", *[str(v) for v in np.frombuffer(r.tobytes(), dtype="<u4")]], capture_output=True, text=True, check=True)
    kind, first = (int(v) for v in out.stdout.split())
    assert (kind, None if first < 0 else first) == want == M.verdict(r)


def test_library_entry_point_is_the_header():
    """efx_scan_verdict of the built library (host only) against the model."""
    import espflix_amd as efx
    kinds = {M.IS_UNKNOWN: "unknown", M.IS_PROGRESSIVE: "progressive", M.IS_INTERLACED: "interlaced", M.IS_TELECINED: "telecined"}
    for r, (kind, first) in VERDICTS:
        got = efx.scan_verdict(r)
        assert (got.kind, got.first_field) == (kinds[kind], {None: None, T: "top", B: "bottom"}[first]) and got.rec.tobytes() == r.tobytes()
    assert efx.load_library().efx_scan_verdict(None, None) == -1
    assert efx.SCAN_DEFAULTS == M.DEFAULTS and (efx.SCAN_NONE, efx.SCAN_UNDETERMINED, efx.SCAN_REPEAT_BOTTOM) == (M.NONE, M.UNDETERMINED, M.REPEAT_BOTTOM)


def test_dtypes_match_the_header(tmp_path):
    """SCAN_OPTS_DTYPE, SCAN_FRAME_DTYPE and SCAN_REC_DTYPE against the host C compiler's layout of include/efx.h, and the
    model's dtypes against them."""
    from espflix_amd import _abi
    import espflix_amd as efx
    from test_abi_layout import header_fields
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a host C compiler is needed to lay out include/efx.h"
    pairs = {"efx_scan_opts": _abi.SCAN_OPTS_DTYPE, "efx_scan_frame": _abi.SCAN_FRAME_DTYPE, "efx_scan_rec": _abi.SCAN_REC_DTYPE}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "efx.h"', "int main(void) {"]
    for c, dt in pairs.items():
        assert list(dt.names) == header_fields(c), "the header names other fields, or in another order"
        lines.append(f'  printf("{c} - %zu 0\\n", sizeof({c}));')
        for f in dt.names:
            lines.append(f'  printf("{c} {f} %zu %zu\\n", offsetof({c}, {f}), sizeof((({c} *)0)->{f}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True, capture_output=True, text=True)
    seen = 0
    for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines():
        c, f, a, b = line.split()
        dt = pairs[c]
        if f == "-":
            assert dt.itemsize == int(a) == sum(dt.fields[n][0].itemsize for n in dt.names), c
        else:
            assert (dt.fields[f][1], dt.fields[f][0].itemsize) == (int(a), int(b)), (c, f)
        seen += 1
    assert seen == 3 + sum(len(dt.names) for dt in pairs.values())
    assert _abi.SCAN_FRAME_DTYPE == M.FRAME and _abi.SCAN_REC_DTYPE == M.REC
    assert efx.SCAN_OPTS_DTYPE is _abi.SCAN_OPTS_DTYPE and efx.SCAN_FRAME_DTYPE is _abi.SCAN_FRAME_DTYPE and efx.SCAN_REC_DTYPE is _abi.SCAN_REC_DTYPE


# ---- what the rule is for ---------------------------------------------------------------------------------------------------
W, H, N = 48, 32, 21


def pulldown(first_field, start):
    """21 frames of 2-3 pulldown of the scene at 5 field periods per film frame, cut in at frame `start` of the cadence:
    luma planes."""
    film = M.with_chroma(np.stack([M.scene(5 * k, W, H) for k in range(22)]))
    video = TM.telecine(film, W, H, first_field, 0, start)[0][:N]
    assert len(video) == N
    return video[:, :W * H].reshape(N, H, W)


def semantic_cases(noise):
    """(name, luma planes with noise, the required (verdict, first_field))."""
    cases = [("progressive", M.material("progressive", N), (M.IS_PROGRESSIVE, None)),
             ("interlaced tff", M.material("interlaced", N, M.TOP), (M.IS_INTERLACED, M.TOP)),
             ("interlaced bff", M.material("interlaced", N, M.BOTTOM), (M.IS_INTERLACED, M.BOTTOM)),
             ("still", M.material("still", N), (M.IS_UNKNOWN, None))]
    for p in (M.TOP, M.BOTTOM):
        cases += [(f"pulldown {'tb'[p]}ff phase {start}", pulldown(p, start), (M.IS_TELECINED, p)) for start in range(5)]
    return [(name, M.noisy(l, noise, 11 + k), want) for k, (name, l, want) in enumerate(cases)]


@pytest.mark.parametrize("noise", [0, 3, 6])
def test_material_gets_its_verdict(sanitized, noise):
    """Progressive, interlaced in both orders, a still picture with fresh noise and 2-3 pulldown in both orders at all five
    phases, clean, at the noise of +-3 of the definition's cases and at +-6, where the still picture's frames are no
    longer STILL and the verdict's order clause has to call it unknown.  Through the header and the model."""
    s = S.layout("i420", W, H)
    for name, lumas, want in semantic_cases(noise):
        srcs = M.with_chroma(lumas)
        got = host_call(sanitized, srcs, s, still=64)
        assert same(got, M.scan(srcs, s, still=64)), name
        r = got[1][0]
        assert M.verdict(r) == want, (name, r)
        if want[0] == M.IS_TELECINED:
            assert int(r["rep_top"].max()) + int(r["rep_bottom"].max()) >= 4, (name, r)
        if name == "still":
            assert (r["n_still"] == N - 1) == (noise < 6) and (noise < 6 or r["n_tff"] + r["n_bff"] > 0), r
