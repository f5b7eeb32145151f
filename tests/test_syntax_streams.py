"""The directed streams of tests/syntax_streams.py on the CPU: what they cover is ASSERTED from the oracle's parse trace
(oracle.trace_syntax), the writer's manifest is held against that trace, a NumPy restatement of the prediction computes the
motion-only pictures independently, the oracle is held against the live reference (where oracle/_ref is built) and against
tests/golden/syntax.json (what the unmodified reference decoded), and k_parse's token machine parses every stream on the
host (tests/_build/parse_harness).  The -m gpu side is tests/test_gpu_syntax.py."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import common
import oracle
import syntax_streams as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "_build", "parse_harness")
FAMILIES = ["codes", "vectors", "windows", "outside"]
DEFINED = ["codes", "vectors", "windows"]   # families the reference defines (every fetch inside the picture)


@pytest.fixture(scope="module")
def traces():
    return {s.name: oracle.trace_syntax(s.array(), 0) for s in ss.all_streams()}


@pytest.fixture(scope="module")
def frames():
    """name -> the oracle's frames of the elementary stream; shared, never written to."""
    out = {}
    for s in ss.all_streams(DEFINED):
        n, _, _, fr = oracle.decode(s.array(), 0, want_frames=True)
        assert n == len(s.pictures)
        fr.setflags(write=False)
        out[s.name] = fr
    return out


def union(traces, family, key):
    out = set()
    for s in ss.family(family):
        out |= traces[s.name][key]
    return out


def motion_mbs(picture):
    return [(m["addr"], m["mv"]) for m in picture["mbs"] if m["type"] != ss.T_SKIPPED and m["type"] & ss.T_FORWARD]


# ---- the manifest is what the oracle parsed ---------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_manifest_equals_trace(family, traces):
    """Picture type, f_code, full_pel; address, type, vector (half-pels), pattern and quantiser of every macroblock."""
    for s in ss.family(family):
        t = traces[s.name]
        assert 2 <= len(s.pictures) <= 8 and len(t["pictures"]) == len(s.pictures), s.name
        for k, (want, got) in enumerate(zip(s.pictures, t["pictures"])):
            if want is None:
                assert got["type"] == 1 and len(got["mbs"]) == ss.MBW * ss.MBH   # the generator's I picture
                continue
            assert got["type"] == want["type"], (s.name, k)
            if want["type"] == 2:
                assert (got["r_size"] + 1, got["full_pel"]) == (want["f_code"], want["full_pel"]), (s.name, k)
            assert len(got["mbs"]) == len(want["mbs"]) == ss.MBW * ss.MBH, (s.name, k)
            for a, b in zip(want["mbs"], got["mbs"]):
                assert a == b, (s.name, k, a, b)


@pytest.mark.parametrize("family", DEFINED)
def test_every_fetch_inside_the_picture(family):
    for s in ss.family(family):
        for p in s.pictures[1:]:
            for addr, mv in motion_mbs(p):
                assert ss.fetch_inside(addr, mv), (s.name, addr, mv)


# ---- coverage, from the trace ------------------------------------------------------------------------------------------------
def test_codes_cover_every_table(traces):
    bk = ss.books()
    # address increments 1 ... 33, stuffing (34), escape (35), and 1 ... 33 behind an escape
    assert union(traces, "codes", "mba") == set(range(1, 36))
    assert union(traces, "codes", "mba_esc") >= set(range(1, 34))
    # all 7 P macroblock types and both I types; the I types from the hand-written I picture
    assert union(traces, "codes", "types") == {(2, t) for t in bk["type_p"]} | {(1, t) for t in bk["type_i"]}
    main = next(s for s in ss.family("codes") if s.name == "codes_main")
    hand_i = [p for p in main.pictures[1:] if p["type"] == 1]
    assert hand_i and {m["type"] for p in hand_i for m in p["mbs"]} == set(bk["type_i"])
    assert len(bk["type_p"]) == 7 and len(bk["type_i"]) == 2
    # all 63 patterns
    assert union(traces, "codes", "cbp") == set(range(1, 64)) == set(bk["cbp"])
    # all 33 motion codes in each component at f_code 1
    t = traces["codes_main"]
    f1 = {k for k, p in enumerate(main.pictures) if p and p["type"] == 2 and p["f_code"] == 1}
    for comp in (0, 1):
        assert {c for (pic, cp, c) in t["motion"] if cp == comp and pic in f1} == set(range(-16, 17)) == set(bk["motion"])
    # all 110 run / level entries with both signs, as the first code of a block and later; "1s" and "11s"
    assert len(bk["dct"]) == 110
    want = {(r, s * l, pos) for (r, l) in bk["dct"] for s in (1, -1) for pos in (0, 1)}
    assert want - t["dct"] == set()
    assert t["dct_short"] == {(0, s, pos) for s in (1, -1) for pos in (0, 1)}
    # scan position 63 reached by a table code and by an escape
    assert t["last_pos"] == {0, 1}
    # the three escape forms (0 one byte, 1 "00 xx", 2 "80 xx") with runs 0 and 63 and levels +-1, +-127, +-128, +-255
    want = set()
    for run in (0, 63):
        for level in (1, -1, 127, -127, 128, -128, 255, -255):
            forms = ([0] if abs(level) <= 127 else []) + [1 if level > 0 else 2]
            for form in forms:
                want.add((form, run, level, 0))
                if run == 0:
                    want.add((form, run, level, 1))
    assert want - t["escapes"] == set()
    # dct_dc_size 0 ... 8 for luminance and chrominance, both signs of the differential
    assert t["dc"] == {(c, size, sign) for c in (0, 1) for size in range(1, 9) for sign in (1, -1)} | {(0, 0, 0), (1, 0, 0)}
    # quantiser_scale 1 ... 31 in a slice header and as a macroblock's own
    assert {(w, q) for w in (0, 1) for q in range(1, 32)} - t["qscale"] == set()


def test_vectors_cover_every_f_code(traces):
    """Per P picture and component: every motion code the geometry reaches (syntax_streams.reachable says which, and why),
    the residuals 0, 2^r - 1 and one other, the ends of the range where they lie inside the picture, both wraps, and each
    of the four predictor resets behind a large vector."""
    seen = set()
    for s in ss.family("vectors"):
        t = traces[s.name]
        for pic, p in enumerate(s.pictures):
            if p is None:
                continue
            f, fp = p["f_code"], p["full_pel"]
            seen.add((f, fp))
            r, scale = f - 1, 1 << (f - 1)
            for comp in (0, 1):
                kmax, wraps, lo_in, hi_in = ss.reachable(comp, f, fp)
                got = {c for (q, cp, c) in t["motion"] if q == pic and cp == comp}
                assert got >= {s_ * k for k in range(1, kmax + 1) for s_ in (1, -1)}, (s.name, pic, comp, sorted(got))
                if r:
                    res = {x for (q, cp, rs, x) in t["residual"] if q == pic and cp == comp and rs == r}
                    assert {0, scale - 1} <= res, (s.name, pic, comp)
                    assert r < 2 or res - {0, scale - 1}, (s.name, pic, comp)
                else:
                    assert not [x for x in t["residual"] if x[0] == pic]
                assert not lo_in or (pic, comp, -16 * scale) in t["ends"], (s.name, pic, comp)
                assert not hi_in or (pic, comp, 16 * scale - 1) in t["ends"], (s.name, pic, comp)
                assert not wraps or {(pic, comp, 1), (pic, comp, -1)} <= t["wraps"], (s.name, pic, comp)
            assert {k for (q, k) in t["resets"] if q == pic} == {"skipped", "intra", "pattern", "slice"}, (s.name, pic)
    assert seen == {(f, fp) for f in range(1, 8) for fp in (0, 1)}
    assert union(traces, "vectors", "r_sizes") == set(range(7)) and union(traces, "vectors", "full_pel") == {0, 1}
    ch = next(s for s in ss.family("vectors") if s.name == "vectors_changing")
    got = [(p["r_size"] + 1, p["full_pel"]) for p in traces[ch.name]["pictures"][1:]]
    assert got == [(1, 0), (7, 0), (2, 1), (4, 0)]
    # what reachable() claims for the small f_codes: everything
    for f, fp in ((1, 0), (1, 1), (4, 0), (4, 1), (5, 0)):
        assert ss.reachable(0, f, fp) == (16, True, True, True)


def test_windows_cover_every_alignment_and_edge(traces):
    mbs = [x for s in ss.family("windows") for p in traces[s.name]["pictures"][1:] for x in motion_mbs(p)]
    luma, chroma, flush = ss.alignment_sets(mbs)
    assert luma == {(a, hx, hy) for a in range(4) for hx in (0, 1) for hy in (0, 1)}
    assert chroma == {(blk, a, hx, hy, y) for blk in (4, 5) for a in range(4) for hx in (0, 1) for hy in (0, 1) for y in range(8)}
    want = set()
    for kind, sides in (("luma13", ("top", "right", "bottom")), ("luma", ("left", "top", "bottom")),
                        ("cr", ("left", "top", "right", "bottom")), ("cb", ("left", "top", "right", "bottom"))):
        for side in sides:
            for h in (0, 1):
                want.add((kind, side, h))
        for a in ("left", "right"):
            for b in ("top", "bottom"):
                if a in sides and b in sides:
                    for ha in (0, 1):
                        for hb in (0, 1):
                            want.add((kind, "corner", a + "-" + b, ha, hb))
    assert want - flush == set()


def test_outside_leaves_the_picture(traces):
    near = traces["outside_near_far"]["pictures"]
    pos = lambda p: {(32 * (m["addr"] % ss.MBW) + m["mv"][0], 32 * (m["addr"] // ss.MBW) + m["mv"][1]) for m in p["mbs"]}
    xs, ys = {x for x, _ in pos(near[1])}, {y for _, y in pos(near[1])}
    assert {-1, ss.X_MAX + 2} <= xs and {-1, ss.Y_MAX + 2} <= ys                      # one half-pel beyond each edge
    assert {(-1, -1), (-1, ss.Y_MAX + 2), (ss.X_MAX + 2, -1), (ss.X_MAX + 2, ss.Y_MAX + 2)} <= pos(near[1])
    for pic, unit in ((2, 1), (3, 2)):                                                # far beyond: f_code 7, every code
        assert (near[pic]["r_size"], near[pic]["full_pel"]) == (6, unit - 1)
        comps = {v for m in near[pic]["mbs"] for v in m["mv"]}
        assert {-1024 * unit, 1023 * unit} <= comps
        for comp in (0, 1):
            assert {c for (q, cp, c) in traces["outside_near_far"]["motion"] if q == pic and cp == comp} == set(range(-16, 17))
    assert min(min(m["mv"]) for m in near[3]["mbs"]) == -2048 and max(max(m["mv"]) for m in near[3]["mbs"]) == 2046
    corners = [(x, y) for x, y in pos(near[4]) if (x < -32 or x > ss.X_MAX + 32) and (y < -32 or y > ss.Y_MAX + 32)]
    assert len({(x < 0, y < 0) for x, y in corners}) == 4                              # beyond each corner
    all_luma = set()
    for p in traces["outside_one_in_eight"]["pictures"][1:]:                         # one in eight outside, the rest varied
        mbs = motion_mbs(p)
        out = [x for x in mbs if not ss.fetch_inside(*x)]
        assert len(out) == ss.MBW * ss.MBH // 8
        luma, chroma, _ = ss.alignment_sets([x for x in mbs if ss.fetch_inside(*x)])
        assert {a for a, hx, hy in luma} == set(range(4))
        all_luma |= luma
        for blk in (4, 5):
            assert {(a, hx, hy) for b, a, hx, hy, y in chroma if b == blk} == {(a, hx, hy) for a in range(4) for hx in (0, 1) for hy in (0, 1)}
            assert {y for b, a, hx, hy, y in chroma if b == blk} == set(range(8))
    assert len(all_luma) == 16


# ---- an independent prediction -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["vectors", "windows"])
def test_numpy_prediction_equals_oracle(family, frames):
    """Every motion-only and skipped macroblock of every P picture, computed from the oracle's previous picture with the
    manifest's vector by syntax_streams.predict_picture (mocomp()'s four cases, predict()'s halved chroma position), equals
    the oracle's picture byte for byte.  (The intra and pattern macroblocks of the reset rows are not predictions.)"""
    for s in ss.family(family):
        fr = frames[s.name]
        for k in range(1, len(s.pictures)):
            mbs = [(m["addr"], m["mv"]) for m in s.pictures[k]["mbs"] if m["type"] in (ss.T_SKIPPED, ss.T_FORWARD)]
            assert len(mbs) >= ss.MBW * ss.MBH - 4
            want, mask = ss.predict_picture(fr[k - 1], mbs)
            got = ss.planes(fr[k])
            for addr in np.nonzero(mask)[0]:
                for plane, (a, b) in enumerate(zip(ss.mb_pixels(want, addr), ss.mb_pixels(got, addr))):
                    assert np.array_equal(a, b), (s.name, k, int(addr), plane, s.pictures[k]["mbs"][addr])


def test_windows_inputs_are_sensitive(frames):
    """A condition on the inputs: for every macroblock of `windows`, the prediction with the vector moved by one half-pel in
    either axis, either way, differs from the correct one -- a fetch that is off by one cannot pass unnoticed."""
    for s in ss.family("windows"):
        fr = frames[s.name]
        for k in range(1, len(s.pictures)):
            rp = ss.planes(fr[k - 1])
            for addr, mv in motion_mbs(s.pictures[k]):
                right = ss.predict_mb(rp, addr, mv)
                for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                    moved = ss.predict_mb(rp, addr, (mv[0] + dx, mv[1] + dy))
                    assert any(not np.array_equal(a, b) for a, b in zip(right, moved)), (s.name, k, addr, mv, dx, dy)


# ---- the oracle against the reference ------------------------------------------------------------------------------------
def as_ts(s):
    return np.frombuffer(common.one_pes_per_picture(s.es), dtype=np.uint8)


@pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("family", DEFINED)
def test_oracle_equals_live_reference(family):
    for s in ss.family(family):
        ts = as_ts(s)
        rh, rpts, rframes = oracle.ref_decode(ts, flush_last=True, want_frames=True)
        n, h, pts, fr = oracle.decode(ts, 1, want_frames=True)
        assert n == len(rh) == len(s.pictures), s.name
        assert (h == rh).all() and (pts == rpts).all(), s.name
        assert np.array_equal(fr, rframes), s.name


@pytest.fixture(scope="module")
def syntax_golden():
    with open(os.path.join(ROOT, "tests", "golden", "syntax.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("family", DEFINED)
def test_oracle_equals_reference_golden(family, syntax_golden):
    """tests/golden/syntax.json: what the unmodified reference decoded (tests/golden/make_syntax_golden.py)."""
    for s in ss.family(family):
        g = syntax_golden[s.name]
        assert f"{common.fnv_bytes(s.array()):016x}" == g["es_fnv"], f"{s.name}: the stream is not the one the golden was made from"
        n, h, pts, _ = oracle.decode(as_ts(s), 1)
        assert n == len(g["hashes"]) == len(s.pictures)
        assert [f"{int(x):016x}" for x in h] == g["hashes"] and [int(x) for x in pts] == g["pts"], s.name


def test_golden_names_every_defined_stream(syntax_golden):
    assert set(syntax_golden) == {s.name for s in ss.all_streams(DEFINED)}


# ---- k_parse's token machine on the host ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(HARNESS):
        subprocess.run(["make", "-C", ROOT, "harness"], check=True, capture_output=True)
    return HARNESS


@pytest.mark.parametrize("family", FAMILIES)
def test_token_machine_parses_every_stream(family, harness, tmp_path):
    """Every macroblock record (address, flags, vector, counts) and coefficient entry equals the oracle's trace; no status
    bit on any slice."""
    for s in ss.family(family):
        f = tmp_path / (s.name + ".es")
        f.write_bytes(s.es)
        p = subprocess.run([harness, str(f)], capture_output=True, text=True, timeout=300, env=dict(os.environ, EFX_HARNESS_CLEAN="1"))
        assert p.returncode == 0, s.name + ": " + p.stdout[-1000:] + p.stderr[-1000:]
        m = re.match(r"OK slices=(\d+) macroblocks=(\d+) entries=(\d+) trips=(\d+) rejected=(\d+) unseen=(\d+) phantom=(\d+)", p.stdout)
        assert m, p.stdout
        r = dict(zip(("slices", "macroblocks", "entries", "trips", "rejected", "unseen", "phantom"), map(int, m.groups())))
        assert r["rejected"] == 0 and r["unseen"] == 0 and r["phantom"] == 0, (s.name, r)
        assert r["macroblocks"] == s.macroblocks() + ss.MBW * ss.MBH, (s.name, r)   # + the generator's I picture
