"""The MPEG-1 encoder's arithmetic (espflix_amd/csrc/enc_core.h, built for the host) against yardsticks that share no code
with it (tests/encode_float.py): the forward DCT against float64 under the criteria of IEEE Std 1180-1990, the intra DC
against the pixel sum, the levels against float64 quantisation of the exact coefficients, every search and mode decision
against an exhaustive model of the documented rule, and the quality against a float64 encoder.  No GPU;
tests/test_gpu_encode.py applies the decision and quality checks to the device.

Regenerate tests/golden/encode_psnr.json (the float yardstick's PSNRs and margins) with tests/golden/make_encode_psnr.py."""
import json

import numpy as np
import pytest

import encode_float as F
import encode_model as E
import export_model as M
import oracle


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return E.build(str(tmp_path_factory.mktemp("enc_model")))


@pytest.fixture(scope="module")
def blocks_exe(tmp_path_factory):
    return E.build_blocks(str(tmp_path_factory.mktemp("enc_blocks")))


@pytest.fixture(scope="module")
def clip_i420(clips):
    out = {}
    for name in ("splash", "vmedia"):
        n, _, _, frames = oracle.decode(clips[name], 1, flush_last=True, want_frames=True)
        out[name] = M.strip_to_i420(frames[:n])
    return out


# -- forward DCT ------------------------------------------------------------------------------------------------------

def fdct_errors(exe, blocks):
    """fdct8 / 8 less the float64 2-D DCT, in standard units: (n, 8, 8)."""
    return E.fdct_blocks(exe, blocks) / 8.0 - F.dct2(blocks)


@pytest.mark.parametrize("lo,hi", [(-255, 255), (-5, 5), (-128, 127)])
@pytest.mark.parametrize("sign", [1, -1], ids=["plus", "minus"])
def test_fdct_meets_ieee_1180(blocks_exe, lo, hi, sign):
    """10 000 random blocks (and their negations) per range: the criteria of IEEE Std 1180-1990 (peak, mean square and
    mean error per coefficient and overall), applied to the forward transform against float64."""
    rng = np.random.default_rng(1180 + hi)
    blocks = sign * rng.integers(lo, hi + 1, size=(10000, 8, 8))
    e = fdct_errors(blocks_exe, blocks)
    figures = {"peak": np.abs(e).max(), "mse per coefficient": (e ** 2).mean(axis=0).max(), "mse overall": (e ** 2).mean(),
               "mean per coefficient": np.abs(e.mean(axis=0)).max(), "mean overall": abs(e.mean())}
    print(f"fdct8 [{lo}, {hi}] x {sign}:", {k: float(f"{v:.5f}") for k, v in figures.items()})
    assert figures["peak"] <= 1
    assert figures["mse per coefficient"] <= 0.06
    assert figures["mse overall"] <= 0.02
    assert figures["mean per coefficient"] <= 0.015
    assert figures["mean overall"] <= 0.0015


def edge_blocks(lo, hi):
    """Flat, the pel checkerboard, row and column stripes (both phases) between lo and hi."""
    yy, xx = np.mgrid[0:8, 0:8]
    out = [np.full((8, 8), lo), np.full((8, 8), hi)]
    for pattern in ((xx ^ yy) & 1, xx & 1, yy & 1, (xx >> 1) & 1, (yy >> 2) & 1):
        out.append(np.where(pattern == 1, hi, lo))
        out.append(np.where(pattern == 1, lo, hi))
    return np.stack(out)


def test_fdct_peak_error_on_intra_inputs_and_edges(blocks_exe):
    """Peak error <= 1 on intra inputs 0..255 (random, flat 0, flat 255, the pel checkerboard, stripes) and on the +-255
    checkerboard, flat +-255 and +-255 stripes."""
    rng = np.random.default_rng(255)
    sets = {"intra random": rng.integers(0, 256, size=(10000, 8, 8)), "intra bright": rng.integers(230, 256, size=(2000, 8, 8)),
            "intra edges": edge_blocks(0, 255), "+-255 edges": edge_blocks(-255, 255)}
    for name, blocks in sets.items():
        peak = np.abs(fdct_errors(blocks_exe, blocks)).max()
        print(f"fdct8 {name}: peak error {peak:.4f}")
        assert peak <= 1, name


# -- intra DC ---------------------------------------------------------------------------------------------------------

def test_intra_dc_is_the_rounded_mean(blocks_exe):
    """Every intra block: the DC level l and the pixel sum S satisfy |64 l - S| <= 36: 32 for ideal rounding plus 4 for
    the 12-bit DC basis entry (1448 for 1448.15) applied in two passes, which leaves the DC term short by at most
    2.2e-4 x 16320, plus the row rounding."""
    rng = np.random.default_rng(64)
    blocks = [rng.integers(0, 256, size=(4000, 8, 8)), rng.integers(240, 256, size=(2000, 8, 8)),
              np.stack([np.full((8, 8), m) for m in range(256)])]
    # means just above x.5: a flat block of m with 33 .. 40 pels one higher, m up to 254
    near = []
    for m in list(range(0, 255, 23)) + list(range(245, 255)):
        for k in range(33, 41):
            for _ in range(4):
                b = np.full(64, m)
                b[rng.choice(64, k, replace=False)] += 1
                near.append(b.reshape(8, 8))
    blocks.append(np.stack(near))
    # and just below: 24 .. 32 pels one higher
    below = []
    for m in (0, 100, 200, 250, 253, 254):
        for k in range(24, 33):
            b = np.full(64, m)
            b[rng.choice(64, k, replace=False)] += 1
            below.append(b.reshape(8, 8))
    blocks.append(np.stack(below))
    src = np.concatenate(blocks).astype(np.uint8)
    worst = 0
    for q in (1, 8, 31):
        _, lev, _ = E.code_blocks(blocks_exe, 1, q, src, np.zeros_like(src))
        dev = np.abs(64 * lev[:, 0].astype(np.int64) - src.reshape(len(src), -1).sum(axis=1, dtype=np.int64))
        worst = max(worst, int(dev.max()))
        assert (lev[:, 0] >= 0).all() and (lev[:, 0] <= 255).all()
        assert dev.max() <= 36, (q, int(dev.max()), src[np.argmax(dev)].tolist())
    print("intra DC: largest |64 l - S| =", worst)


# -- levels -----------------------------------------------------------------------------------------------------------

def zigzag():
    """Scan position -> raster index (ISO 11172-2 2.4.3.7), built from the diagonals."""
    out = []
    for s in range(15):
        diag = [(v, s - v) for v in range(8) if 0 <= s - v < 8]     # (v, u), v ascending
        out += [v * 8 + u for v, u in (diag if s & 1 else diag[::-1])]
    return np.array(out)


def level_inputs(rng, n):
    """(src, pred) blocks: noise, smooth ramps, and predictions that miss the source by a little or by a lot."""
    yy, xx = np.mgrid[0:8, 0:8]
    src, pred = [], []
    for k in range(n):
        kind = k % 5
        if kind == 0:
            s = rng.integers(0, 256, size=(8, 8))
        elif kind == 1:
            s = rng.integers(96, 160, size=(8, 8))
        else:
            a, b, c = rng.uniform(-12, 12), rng.uniform(-12, 12), rng.uniform(40, 215)
            s = c + a * (xx - 3.5) + b * (yy - 3.5) + rng.normal(0, (2, 6, 15)[kind - 2], size=(8, 8))
        s = np.clip(np.rint(s), 0, 255)
        amp = (3, 12, 40, 120)[(k // 5) % 4]
        p = np.clip(s + rng.integers(-amp, amp + 1, size=(8, 8)), 0, 255)
        src.append(s)
        pred.append(p)
    return np.stack(src).astype(np.uint8), np.stack(pred).astype(np.uint8)


@pytest.mark.parametrize("intra", [1, 0], ids=["intra", "non_intra"])
@pytest.mark.parametrize("q", [1, 2, 8, 31])
def test_levels_follow_float64_quantisation(blocks_exe, q, intra):
    """Blocks whose levels were not halved: every level equals the float64 quantisation of the exact coefficient (intra AC
    rounded to nearest, non-intra truncated, |level| <= 255) or differs from it by 1, and by 1 only where the exact
    |F| lies within 8 F-units (the forward DCT's peak bound) of a decision threshold."""
    rng = np.random.default_rng(100 * q + intra)
    src, pred = level_inputs(rng, 6000)
    _, lev, halved = E.code_blocks(blocks_exe, intra, q, src, pred)
    keep = ~halved
    assert keep.sum() >= 3000, int(keep.sum())
    res = src.astype(np.float64) - (0 if intra else pred.astype(np.float64))
    Fx = 8 * F.dct2(res)[keep]                        # exact, fdct8's units
    got = np.zeros((len(lev), 64), dtype=np.int64)
    got[:, zigzag()] = lev
    got = got.reshape(-1, 8, 8)[keep]
    d = q * F.INTRA_Q if intra else np.full((8, 8), 16.0 * q)
    x = np.abs(Fx) / d
    if intra:
        want = np.minimum(np.floor(x + 0.5), 255)
        k = np.clip(np.rint(x - 0.5), 0, 254)         # thresholds at (k + 1 / 2) d
        dist = np.abs(np.abs(Fx) - (k + 0.5) * d)
    else:
        want = np.minimum(np.floor(x), 255)
        k = np.clip(np.rint(x), 1, 255)               # thresholds at k d
        dist = np.abs(np.abs(Fx) - k * d)
    want = (want * np.sign(Fx)).astype(np.int64)
    diff = np.abs(got - want)
    if intra:
        diff[:, 0, 0] = 0                             # the DC has its own test
    print(f"q {q} intra {intra}: {int(keep.sum())} blocks, {int((diff == 1).sum())} of {diff.size} levels differ by 1, "
          f"largest threshold distance among them {dist[diff == 1].max() if (diff == 1).any() else 0:.3f} F-units")
    assert diff.max() <= 1
    assert (dist[diff == 1] <= 8).all(), float(dist[diff == 1].max())
    assert (np.abs(want) > 0).sum() > 1000            # the case quantises something


# -- search and mode decisions ------------------------------------------------------------------------------------------

def decision_sources(clip_i420):
    return {"big_motion": F.big_motion(5), "moving": E.moving(5), "checkerboard": E.checkerboard(3), "flat": E.flat(3, 90),
            "noise": E.noise(), "splash": clip_i420["splash"][14:18], "vmedia": clip_i420["vmedia"][14:18]}


@pytest.mark.parametrize("search", [0, 1, 7, 8, 15])
def test_search_decisions_are_the_models(model, clip_i420, search):
    """Every macroblock of every P picture of the host model's streams: (intra, h, v) equals the exhaustive model's, with
    the encoder's own previous reconstruction as the reference picture.  Exact."""
    total = 0
    for name, pics in decision_sources(clip_i420).items():
        stream, recon = E.encode(model, pics, gop=len(pics), qscale=5, search=search, fmt=0)
        total += E.check_decisions(stream, 0, pics, recon, len(pics), search)
    assert total == 264 * 19


def test_big_motion_reaches_the_window_edge(model):
    """The source of the device's radius matrix: at every radius the chosen vectors reach +-(2 R + 1) half pels."""
    pics = F.big_motion(5)
    for R in range(1, 16):
        stream, _ = E.encode(model, pics, gop=5, qscale=5, search=R, fmt=0)
        vec = [(h, v) for _, _, intra, _, h, v in E.p_vectors(stream, 0) if not intra]
        assert max(abs(h) for h, _ in vec) == 2 * R + 1 and max(abs(v) for _, v in vec) == 2 * R + 1, R


# -- quality ----------------------------------------------------------------------------------------------------------

def test_record_margins_are_quarter_steps():
    """tests/golden/encode_psnr.json: every margin is a quarter of the yardstick's own step to the neighbouring qscale."""
    record = json.load(open(E.PSNR_JSON))
    assert (record["gop"], record["search"]) == (E.QUALITY_GOP, E.QUALITY_SEARCH)
    assert sorted(record["cases"]) == sorted(f"{n}_q{q}" for n in ("splash", "vmedia", "moving") for q in E.QUALITY_Q)
    for name, rec in record["cases"].items():
        q = int(name.split("_q")[1])
        assert rec["neighbour"] == E.neighbour_q(q)
        for t in "IP":
            assert abs(rec[t + "_margin"] - abs(rec[t] - rec[t + "_neighbour"]) / 4) <= 1e-4, (name, t)
            assert rec[t + "_margin"] > 0


@pytest.mark.parametrize("q", E.QUALITY_Q)
def test_quality_against_the_float_yardstick(model, clip_i420, q):
    """splash and vmedia (pictures 14..25) and the moving texture, gop 4: the host model's mean luma PSNR of the I pictures
    and of the P pictures is at least the float64 yardstick's less a quarter of the yardstick's own step to the
    neighbouring qscale (a quantiser defect costs about a step, arithmetic rounding far less).  The yardstick's PSNRs are
    those recorded in tests/golden/encode_psnr.json (0.01 dB)."""
    record = json.load(open(E.PSNR_JSON))
    failures = []
    for name, pics in E.quality_sources(clip_i420).items():
        rec = record["cases"][f"{name}_q{q}"]
        yard = F.psnr_by_type(pics, F.encode(pics, E.QUALITY_GOP, q, E.QUALITY_SEARCH), E.QUALITY_GOP)
        for t, y in zip("IP", yard):
            assert abs(y - rec[t]) <= 0.01, (name, q, t, y, rec[t])
        _, recon = E.encode(model, pics, gop=E.QUALITY_GOP, qscale=q, search=E.QUALITY_SEARCH, fmt=0)
        failures += E.check_quality(record, name, q, pics, recon, "host model")
    assert not failures, failures
