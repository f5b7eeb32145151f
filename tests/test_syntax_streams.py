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
FAMILIES = ["codes", "vectors", "windows", "outside", "coefs", "range"]
DEFINED = ["codes", "vectors", "windows", "coefs"]   # families the reference defines (every fetch inside the picture, every
                                                      # reconstructed value inside its clamp table)


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
    """Picture type, f_code, full_pel; address, type, vector (half-pels), pattern, quantiser and every block's (scan position,
    level) list of every macroblock."""
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


# ---- coefficient to pixel: families coefs and range ------------------------------------------------------------------------
def coded_blocks(t):
    """(picture, picture's trace, macroblock, block index, entries) of every coded block of the hand-written pictures."""
    for k, p in enumerate(t["pictures"][1:], 1):
        for m in p["mbs"]:
            if m["type"] == ss.T_SKIPPED:
                continue
            blks = [b for b in range(6) if m["cbp"] & (0x20 >> b)]
            assert len(blks) == len(m["blocks"])
            for b, e in zip(blks, m["blocks"]):
                yield k, p, m, b, e


def test_tables_are_the_oracles():
    zz, pm = oracle.tables()
    assert list(zz) == ss.ZIGZAG and [int(x) for x in pm] == [v for row in ss.PREMUL for v in row]
    assert [int(x) for x in oracle.default_intra()] == ss.DEFAULT_INTRA
    assert sorted(ss.recon_order(mb, blk) for mb in range(ss.MBW * ss.MBH) for blk in range(6)) == list(range(1584))


def copy_block_dc(dc):
    """copy_block_dc (player.cpp:1175-1187): the value replicated as a 32-bit word, unclamped and unmasked."""
    w = dc & 0xFFFFFFFF
    w |= (w << 8) & 0xFFFFFFFF
    w |= (w << 16) & 0xFFFFFFFF
    return np.array([[(w >> (8 * (x & 3))) & 0xFF for x in range(8)]] * 8, dtype=np.int64)


@pytest.fixture(scope="module")
def new_frames():
    out = {}
    for s in ss.all_streams(("coefs", "range")):
        n, _, _, fr = oracle.decode(s.array(), 0, want_frames=True)
        assert n == len(s.pictures)
        fr.setflags(write=False)
        out[s.name] = fr
    return out


@pytest.mark.parametrize("family", ["coefs", "range"])
def test_integer_restatement_equals_oracle(family, new_frames):
    """Every macroblock of every hand-written picture, computed in NumPy from the manifest alone -- the plain-integer
    dequantiser, the integer IDCT of syntax_streams.idct_block, the prediction of predict_mb, the "n == 1" shortcuts and a
    plain clamp to 0 ... 248 -- equals the oracle's picture.  What the tests below compute about operands and residuals
    with idct_block is therefore what the oracle's arithmetic does."""
    for s in ss.family(family):
        fr = new_frames[s.name]
        for k in range(1, len(s.pictures)):
            P = s.pictures[k]
            prev, got = ss.planes(fr[k - 1]), ss.planes(fr[k])
            jobs, blocks = [], []
            for m in P["mbs"]:
                intra = m["type"] != ss.T_SKIPPED and bool(m["type"] & ss.T_INTRA)
                pred = [np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)] if intra \
                    else ss.predict_mb(prev, m["addr"], m["mv"])
                ent = iter(m["blocks"])
                for b in range(6):
                    pb = (pred[0][8 * (b >> 1):8 * (b >> 1) + 8, 8 * (b & 1):8 * (b & 1) + 8] if b < 4 else pred[b - 3]).astype(np.int64)
                    e = next(ent) if m["cbp"] & (0x20 >> b) else None
                    if e is not None:
                        blocks.append(ss.block_values(e, m["q"], P["intra_m"] if intra else P["non_intra_m"], intra))
                    jobs.append((m["addr"], b, pb, e, intra))
            res = ss.idct_block(np.stack(blocks, axis=2))[0] if blocks else None
            j = 0
            for addr, b, pb, e, intra in jobs:
                if e is None:
                    want = pb
                else:
                    r, first = res[:, :, j], int(blocks[j][0, 0])
                    j += 1
                    if len(e) == 1 and e[0][0] == 0:
                        want = copy_block_dc(first >> 8) if intra else np.clip(pb + (first >> 8), 0, 248)
                    else:
                        want = np.clip(pb + r, 0, 248)
                px = ss.mb_pixels(got, addr)
                have = px[0][8 * (b >> 1):8 * (b >> 1) + 8, 8 * (b & 1):8 * (b & 1) + 8] if b < 4 else px[b - 3]
                assert np.array_equal(have, want), (s.name, k, addr, b, e)


def test_coefs_see_every_scan_position_alone(traces):
    """Non-intra at positions 0 ... 63, intra (beside its DC) at 1 ... 63, either sign, under the default matrices and under
    loaded ones; the loaded matrices hold 64 distinct entries each, 255 and one below 16 among them, and at the quantiser
    used no two scan positions dequantise alike -- an entry taken from another position is another coefficient."""
    seen = set()
    for name in ("coefs_positions", "coefs_matrices"):
        for k, p, m, b, e in coded_blocks(traces[name]):
            intra = bool(m["type"] & ss.T_INTRA)
            if len(e) == 1 + intra and abs(e[-1][1]) == 1:
                seen.add((intra, p["custom"], e[-1][0], e[-1][1]))
    want = {(i, c, n, sg) for i in (False, True) for c in (False, True) for n in range(int(i), 64) for sg in (1, -1)}
    assert seen == want
    mat = next(s for s in ss.family("coefs") if s.name == "coefs_matrices")
    assert [p["custom"] for p in mat.pictures[1:]] == [True, True, False, False]
    assert [p["custom"] for p in traces["coefs_matrices"]["pictures"][1:]] == [True, True, False, False]
    for key, intra in (("intra_m", True), ("non_intra_m", False)):
        m = mat.pictures[1][key]
        assert len(set(m)) == 64
        assert len({ss.dequant(1, 16, v, intra) for v in m}) == 64
        assert mat.pictures[3][key] == ss.by_scan(default=ss.DEFAULT_INTRA if intra else [16] * 64)
    assert max(mat.pictures[1]["non_intra_m"]) == 255 and min(mat.pictures[1]["intra_m"]) < 16
    # intra blocks stand beside DC differentials of zero and not
    pos = next(s for s in ss.family("coefs") if s.name == "coefs_positions")
    dcs = [[e[0][1] for e in m["blocks"]] for m in pos.pictures[2]["mbs"]]
    assert any(a[0] == a[1] for a in dcs) and any(a[0] != a[1] for a in dcs)


def test_coefs_rounding_classes(traces):
    """Every class of the dequantiser's rounding (player.cpp:1110-1121), recomputed from the oracle's trace in plain integers:
    the product p = (2 level +- 1) q m of a non-intra coefficient at scan position 0, alone in its block (the "n == 1"
    shortcut) and beside +-1 at scan position 1 (the IDCT path)."""
    s = next(x for x in ss.family("coefs") if x.name == "coefs_rounding")
    alone, beside, zero = set(), set(), set()
    for k, p, m, b, e in coded_blocks(traces[s.name]):
        intra = bool(m["type"] & ss.T_INTRA)
        if any(level == 0 for n, level in e[int(intra):]):
            assert e[-1][1] == 0 and len(e) >= 2 + intra
            zero.add(intra)
        if intra or e[0][0] != 0 or not (len(e) == 1 or (len(e) == 2 and e[1][0] == 1 and abs(e[1][1]) == 1)):
            continue
        level, mq = e[0][1], s.pictures[k]["non_intra_m"][0]
        prod = (2 * level + (1 if level > 0 else -1)) * m["q"] * mq
        t = abs(prod) // 16
        cls = {("multiple of 16", prod > 0)} if prod % 16 == 0 else {("truncated toward zero", prod > 0)}
        if t % 2 == 0 and t:
            cls.add(("even, moved toward zero", prod > 0))
        if t in (2047, 2049):
            cls.add((t, prod > 0))
        if t > 2 * 2049:
            cls.add(("far beyond", prod > 0))
        if (level, m["q"], mq) == (-256, 31, 255):
            cls.add("largest")
        assert ss.dequant(level, m["q"], mq, False) == max(-2048, min(2047, (t - (t % 2 == 0)) * (1 if prod > 0 else -1)))
        (alone if len(e) == 1 else beside).update(cls)
    want = {(c, sg) for c in ("multiple of 16", "truncated toward zero", "even, moved toward zero", 2047, 2049, "far beyond")
            for sg in (True, False)} | {"largest"}
    assert alone == want and beside == want
    assert zero == {False, True}
    assert traces[s.name]["escapes"] >= {(2, 0, -256, 0), (1, 0, 0, 1)}   # "80 00" and "00 00"


def test_coefs_dense_fills_a_wave(traces):
    """In k_recon's block order, a wave of 64 blocks that hold 64 entries each (4096: the prefix counts reach 4032), as
    non-intra and as intra blocks; and waves in which full blocks stand among empty and one-entry ones."""
    t = traces["coefs_dense"]
    for p in t["pictures"][1:]:
        count = np.zeros(1584, dtype=np.int64)
        for m in p["mbs"]:
            blks = [b for b in range(6) if m["cbp"] & (0x20 >> b)]
            for b, e in zip(blks, m["blocks"]):
                count[ss.recon_order(m["addr"], b)] = len(e)
        waves = [count[g:g + 64] for g in range(0, 1584, 64)]
        assert sum(1 for w in waves if (w == 64).all()) >= 4
        steps = {tuple(sorted(set(int(x) for x in w))) for w in waves}
        floor = 1 if p["type"] == 1 else 0   # (an intra block always holds its DC)
        assert (floor, 64) in steps and any(64 in st and floor + 1 in st for st in steps)   # full among empty / one-entry blocks
        # long flat runs of the prefix array with a jump of 64 in them
        assert any((w == 64).sum() in (1, 2) and (w == floor).sum() >= 62 for w in waves)


def range_blocks(s):
    """(picture, macroblock, block, intra, entries, pre-multiplied block) of the blocks of a range stream with 63 and more entries."""
    for k, P in enumerate(s.pictures[1:], 1):
        for m in P["mbs"]:
            intra = m["type"] != ss.T_SKIPPED and bool(m["type"] & ss.T_INTRA)
            blks = [b for b in range(6) if m["cbp"] & (0x20 >> b)]
            for b, e in zip(blks, m["blocks"]):
                if len(e) >= 63:
                    yield k, m, b, intra, e, ss.block_values(e, m["q"], P["intra_m"] if intra else P["non_intra_m"], intra)


def test_range_idct_stands_at_the_extremes(capsys):
    """The integer IDCT over the blocks of range_idct: each multiplied operand of either pass reaches 99 % of its L1 bound
    (2048 x the sum of the absolute weights; the rounding shifts of the column pass cost a fraction of a percent), every
    operand stays below 2^23 (v_mad_i32_i24 in k_recon) and |residual| + 255 below 2^15 (its packed 16-bit add)."""
    s = ss.family("range")[0]
    col_w, row_w, res_w = ss.idct_weights()
    items = list(range_blocks(s))
    assert all(abs(int(v)) in (2047, 2048) for *_, intra, e, blk in items for v in (blk // np.array(ss.PREMUL)).reshape(-1)[1:])
    res, col, row = ss.idct_block(np.stack([x[-1] for x in items], axis=2))
    with capsys.disabled():
        for tag, ops, w in (("column", col, col_w), ("row", row, row_w)):
            for op in range(4):
                bound = 2048 * float(np.abs(w[op]).sum(axis=1).max())
                got = int(np.abs(ops[op]).max())
                print(f"\nrange_idct: {tag} pass {ss.OPERANDS[op]}: reached {got} of L1 bound {bound:.0f} ({got / bound:.4f})", end="")
                assert got >= 0.99 * bound and got < 1 << 23
        ac = 2048 * float(np.abs(res_w.reshape(64, 64)[:, 1:]).sum(axis=1).max())
        nonintra = np.array([not x[3] for x in items])
        print(f"\nrange_idct: largest |residual| {int(np.abs(res[:, :, nonintra]).max())} (non-intra), AC only "
              f"{int(np.abs(res[:, :, ~nonintra] - 128).max())} (L1 bound {ac:.0f})")
    assert int(np.abs(res).max()) + 255 < 1 << 15
    assert int(np.abs(col).max()) < 1 << 23 and int(np.abs(row).max()) < 1 << 23
    # each aimed-at pixel's residual comes within a percent of its own bound, on predictions of 0 and of 248, and intra
    for name, w, (kind, y, x) in ss.range_patterns():
        if kind == "pixel":
            for sel, first in ((nonintra, 0), (~nonintra, 1)):
                bound = 2048 * float(np.abs(w[first:]).sum())
                r = res[y, x, sel] - (0 if first == 0 else 128)
                assert r.max() >= 0.99 * bound and r.min() <= -0.99 * bound, (name, first)
    preds = {(m["addr"] % ss.MBW) < ss.MBW // 2 for k, m, b, intra, e, blk in items if not intra}
    assert preds == {True, False}


def largest_ac_residual():
    """The largest |residual| the 63 AC coefficients of a block can give a pixel: per pixel 2048 x the L1 norm of its weights,
    plus the half unit each of the IDCT's seven rounding shifts on the way can add."""
    res_w = ss.idct_weights()[2].reshape(64, 64)
    return int(np.ceil(2048 * np.abs(res_w[:, 1:]).sum(axis=1).max())) + 4


def test_range_dc_walks_the_predictors(traces, capsys):
    """From the trace: each DC predictor takes each listed value in a DC-only block, beside +-1 at scan position 1 and, from
    +-18 500 outward, beside the residual-maximising AC pattern signed the same way -- the sum crosses +-2^15 from +-18 500
    on; behind the walks a predictor is back on its exact value."""
    t = traces["range_dc"]
    s = ss.family("range")[1]
    seen = {}
    w, py, px = ss.max_ac_residual()
    for k, p, m, b, e in coded_blocks(t):
        comp = 0 if b < 4 else b - 3
        kind = "dc" if len(e) == 1 else ("ac1" if len(e) == 2 and e[1][0] == 1 and abs(e[1][1]) == 1 else ("pattern" if len(e) == 64 else None))
        assert kind
        seen.setdefault((comp, e[0][1]), set()).add(kind if kind != "ac1" else ("ac1", e[1][1]))
        if kind == "pattern":
            r = int(ss.idct_block(ss.block_values(e, m["q"], s.pictures[k]["intra_m"], True))[0][py, px])
            # (the largest AC-only residual is some 14 060: from +-18 500 the sum comes within a percent of +-2^15, from
            # +-32 767 on it is far beyond)
            assert (r > 0) == (e[0][1] > 0) and abs(r) >= abs(e[0][1]) + 0.99 * (largest_ac_residual() - 4), (k, m["addr"], b, r)
            assert abs(r) >= 1 << 15 or abs(e[0][1]) == 18500, (k, m["addr"], b, r)
    for comp in range(3):
        for v in ss.DC_TARGETS:
            want = {"dc", ("ac1", 1), ("ac1", -1)} | ({"pattern"} if abs(v) >= 18500 else set())
            assert seen.get((comp, v), set()) >= want, (comp, v)
        assert "dc" in seen[(comp, 100)] and {"dc", ("ac1", 1)} <= seen[(comp, 107)]
    with capsys.disabled():
        print(f"\nrange_dc: largest AC-only residual {largest_ac_residual()}", end="")
    # the bound k_recon puts on the DC term of a block that runs the IDCT: beyond it the pixel is 0 or 248 whatever the AC
    # coefficients do, and inside it DC + AC fits the 16 bits the kernel keeps
    with open(os.path.join(ROOT, "espflix_amd", "csrc", "k_recon.hip")) as f:
        B = int(re.search(r"constexpr int kDcBound = (\d+);", f.read()).group(1))
    assert B - largest_ac_residual() > 248 and B + largest_ac_residual() < 1 << 15


SAMPLES = {   # stream -> (picture, macroblock address, block, index into the block's coefficient list, what to change)
    "coefs_positions": [(1, 0, 3, 0, "sign move"), (1, 100, 5, 0, "sign move"), (2, 5, 0, 0, "sign move"), (2, 200, 4, 0, "sign move")],
    "coefs_matrices": [(1, 30, 2, 0, "sign move"), (2, 61, 1, 0, "sign move"), (3, 30, 2, 0, "sign move"), (4, 130, 5, 0, "sign move")],
    "coefs_rounding": [(2, 29, 0, 0, "sign move"), (3, 71, 2, 0, "sign move"), (4, 111, 4, 0, "sign move"), (5, 156, 0, 0, "sign")],
    "coefs_dense": [(1, 0, 0, 5, "sign"), (1, 43, 5, 63, "sign"), (2, 3, 2, 30, "sign"), (1, 89, 0, 0, "sign move")],
    "range_idct": [(2, 0, 0, 1, "sign"), (2, 12, 4, 2, "sign"), (3, 1, 3, 0, "sign"), (3, 2, 5, 4, "sign")],
    "range_dc": [(1, 0, 2, 0, "sign move"), (1, 0, 1, 0, "sign move"), (2, 1, 5, 0, "sign move"), (4, 1, 4, 0, "sign move")],
}


@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_coefficient_inputs_are_sensitive(name, new_frames):
    """A condition on the inputs, as test_windows_inputs_are_sensitive: for a sample of blocks of every stream, the oracle's
    picture changes when one level changes its sign and when one coefficient moves by one scan position -- a sign or a
    position lost on the way to the pixel cannot pass unnoticed there."""
    s = next(x for f in ("coefs", "range") for x in ss.family(f) if x.name == name)
    for pic, addr, blk, k, kinds in SAMPLES[name]:
        for kind in kinds.split():
            changed = ss.rebuild(name, (pic, addr, blk, k, kind))
            assert changed.es != s.es and len(changed.pictures) == len(s.pictures), (name, pic, addr, blk, k, kind)
            n, _, _, fr = oracle.decode(changed.array(), 0, want_frames=True)
            assert n == len(s.pictures)
            a, b = ss.mb_pixels(ss.planes(fr[pic]), addr), ss.mb_pixels(ss.planes(new_frames[name][pic]), addr)
            assert any(not np.array_equal(x, y) for x, y in zip(a, b)), (name, pic, addr, blk, k, kind)
            assert all(np.array_equal(fr[j], new_frames[name][j]) for j in range(pic)), (name, pic, addr, blk, k, kind)


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
