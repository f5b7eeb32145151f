"""Adaptive quantisation of the MPEG-1 encoder (espflix_amd/csrc/enc_aq.h with enc_core.h and enc_rate.h, built for the
host by tests/encode_aq_model.py): the rule of include/efx.h, restated there in NumPy, against the quantisers the host
model uses, and what the model writes against what the test oracle (and the reference, where built) reads.  No GPU;
tests/test_gpu_adaptive_quant.py holds the device to the same host model byte for byte."""
import numpy as np
import pytest

import encode_aq_model as A
import encode_model as E
import encode_rate_model as R
import export_model as M
import oracle

PROFILE = dict(vbv_bits=250_000, qmin=3, qmax=31)
QS = [(q, s) for q in (2, 8, 31) for s in (64, 256)]


@pytest.fixture(scope="module")
def aq(tmp_path_factory):
    return A.build(str(tmp_path_factory.mktemp("enc_aq_model")))


@pytest.fixture(scope="module")
def directed():
    return A.directed(3)


@pytest.fixture(scope="module")
def clip(clips):
    """vmedia's first pictures."""
    n, _, _, frames = oracle.decode(clips["vmedia"], 1, flush_last=True, want_frames=True)
    return M.strip_to_i420(frames[:12])


def round_trip(stream, fmt, recon, first_pts=0):
    n, _, pts, frames = oracle.decode(np.frombuffer(stream, dtype=np.uint8), fmt, flush_last=True, want_frames=True)
    assert n == len(recon), (n, len(recon))
    assert np.array_equal(frames, M.i420_to_strip(recon)), "the oracle's pictures differ from the encoder's reconstruction"
    if fmt == 1 and oracle.have_ref():
        from espflix_amd import gen
        hashes, rpts, _ = oracle.ref_decode(np.frombuffer(stream, dtype=np.uint8), flush_last=True)
        assert [int(h) for h in hashes] == [gen.fnv1a64(s) for s in M.i420_to_strip(recon)]
        assert list(rpts) == [first_pts + 3003 * k for k in range(n)]


def rule(pics, q, s, lo=1, hi=31):
    return np.stack([A.mq_map(p, q, s, lo, hi) for p in pics])


def test_rule_on_random_pictures(aq, clip):
    """The NumPy rule equals the C model's maps: pictures of noise whose amplitude differs per macroblock, the directed
    clip and a golden clip's pictures, every strength's ends and every clamp."""
    rng = np.random.default_rng(3)
    amp = np.kron(rng.integers(0, 9, size=(4, 12, 22)) ** 2 * 4, np.ones((16, 16), dtype=np.int64))
    luma = np.clip(128 + rng.integers(-128, 128, size=(4, E.H, E.W)) * amp // 256, 0, 255).astype(np.uint8)
    pics = np.concatenate([np.stack([A._i420(l, 9) for l in luma]), A.directed(2), clip[:2]])
    for q, s in [(1, 1), (1, 256), (31, 1), (31, 256), (8, 64), (8, 128), (20, 255)]:
        got = A.encode(aq, pics, aq=s, qscale=q, gop=1, fmt=0)
        assert np.array_equal(got.maps, rule(pics, q, s)), (q, s)
        assert (got.qscales == q).all()
    a = np.stack([A.activities(p) for p in pics])
    assert a.min() >= 1 and a.max() <= 8161 and len(np.unique(a)) > 100


def test_tiled_pictures_are_untouched(aq, tmp_path_factory):
    """a == avg in every macroblock: mq == q, and the stream is the one without adaptive quantisation -- the model's at
    strength 0, and the plain host model's (tests/enc_model_main.cpp calls write_slice without the new argument)."""
    pics = A.tiled(3)
    plain = E.build(str(tmp_path_factory.mktemp("enc_model")))
    for q in (2, 8, 31):
        on, off = A.encode(aq, pics, aq=256, qscale=q), A.encode(aq, pics, aq=0, qscale=q)
        assert (on.maps == q).all() and np.array_equal(rule(pics, q, 256), on.maps)
        assert on.stream == off.stream and np.array_equal(on.recon, off.recon)
        want, want_rec = E.encode(plain, pics, qscale=q)
        assert off.stream == want and np.array_equal(off.recon, want_rec)
        assert len(on.stream) > 3 * 5000, "the P pictures code nothing"


@pytest.mark.parametrize("value", [0, 255])
def test_flat(aq, value):
    """flat0 / flat255: a = 1, avg = 1, mq == q."""
    pics = E.flat(2, value)
    assert (np.stack([A.activities(p) for p in pics]) == 1).all()
    for q in (1, 20, 31):
        r = A.encode(aq, pics, aq=256, qscale=q, fmt=0)
        assert (r.maps == q).all()
        assert r.stream == A.encode(aq, pics, aq=0, qscale=q, fmt=0).stream


@pytest.mark.parametrize("r,c", A.ODD_AT)
def test_one_odd_macroblock(aq, r, c):
    """One macroblock unlike the rest, at the columns where a lane's first set of words ends (15), its second begins (16)
    and ends (21), in the first and the last row.
    Full-range noise in a flat picture, q 20, strength 256: 263 macroblocks have a = 1, so avg = (263 + a_n + 132) / 264
    with a_n the noise macroblock's activity (thousands: avg is 10 to 30).  The noise macroblock's factor is close to 2:
    31 after the clamp.  A flat one's is (2 + avg) / (1 + 2 avg).
    Faint noise (0 .. 3 around 128): a_n < 133, so avg = 1 and the flat macroblocks keep q; the factor of the noise
    macroblock, (2 a_n + 1) / (a_n + 2), still takes 20 past 31.
    One flat macroblock in noise, q 1: the factor is above 1/2, the result rounds to 1 or is clamped to it."""
    pic = A.one_odd("noise_in_flat", r, c)
    a_n = int(A.activities(pic)[r, c])
    avg = (263 + a_n + 132) // 264
    assert a_n > 2000 and 8 <= avg <= 31
    got = A.encode(aq, pic[None], aq=256, qscale=20, gop=1, fmt=0).maps[0]
    flat_q = (20 * (512 + 256 * avg) + (256 + 512 * avg) // 2) // (256 + 512 * avg)
    want = np.full((12, 22), flat_q)
    want[r, c] = 31
    assert np.array_equal(got, want) and np.array_equal(got, A.mq_map(pic, 20, 256))

    pic = A.one_odd("faint_in_flat", r, c)
    assert 4 < int(A.activities(pic)[r, c]) < 133
    got = A.encode(aq, pic[None], aq=256, qscale=20, gop=1, fmt=0).maps[0]
    want = np.full((12, 22), 20)
    want[r, c] = 31
    assert np.array_equal(got, want) and np.array_equal(got, A.mq_map(pic, 20, 256))

    pic = A.one_odd("flat_in_noise", r, c)
    res = A.encode(aq, pic[None], aq=256, qscale=1, gop=1, fmt=0)
    assert res.maps[0, r, c] == 1 and np.array_equal(res.maps[0], A.mq_map(pic, 1, 256))
    got = A.encode(aq, pic[None], aq=256, qscale=8, gop=1, fmt=0).maps[0]
    assert got[r, c] == 4 and np.array_equal(got, A.mq_map(pic, 8, 256))   # (2 + avg) / (1 + 2 avg) just above 1/2
    round_trip(res.stream, 0, res.recon)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("q,s", QS)
def test_directed_clip(aq, directed, q, s, fmt):
    """The model's stream decodes to the model's reconstruction; every coded macroblock is decoded at the map's
    quantiser, the slice headers carry column 0, the quant flag stands exactly where the quantiser changes; at q 8 all
    four quant variants occur."""
    r = A.encode(aq, directed, aq=s, qscale=q, fmt=fmt, first_pts=129003)
    assert np.array_equal(r.maps, rule(directed, q, s))
    round_trip(r.stream, fmt, r.recon, 129003)
    seen = A.check_stream(r.stream, fmt, r.maps, f"q {q} strength {s}")
    if q == 8:
        assert seen == A.QUANT_TYPES, seen
    assert r.stream != A.encode(aq, directed, aq=0, qscale=q, fmt=fmt, first_pts=129003).stream or (r.maps == q).all()


def test_search_15(aq, directed):
    r = A.encode(aq, directed, aq=256, qscale=8, search=15, fmt=1)
    round_trip(r.stream, 1, r.recon)
    assert A.check_stream(r.stream, 1, r.maps, "search 15") == A.QUANT_TYPES


def test_slices_keep_their_bound(aq):
    """The argument beside enc_core.h's kMbMaxBits, from the code book's lengths: an inter macroblock reaches the budget
    only with all six blocks coded, where pattern 63 and an increment of at most 21 leave the 4 bits the quant variants
    cost; an intra macroblock has the motion, pattern and one coefficient per block to spare.  And the domain-edge noise
    picture at q 1, strength 256, stays inside kSliceCap."""
    L = A.lengths(aq)
    budget = 11 + 6 + 24 + 9
    assert L["mb_max_bits"] == budget + 6 * (64 * 28 + 2)
    block = 64 * 28 + 2
    for t in ("pat_q", "fwd_pat_q"):
        assert L[t] + 5 == 10
        assert L["mba21"] + L[t] + 5 + 2 * (L["mv_max"] + 1) + L["cbp63"] <= budget           # all six blocks coded
        assert L["mba21"] + L[t] + 5 + 2 * (L["mv_max"] + 1) + L["cbp_max"] <= budget + block  # fewer: a block's bits to spare
    dc = 4 * (7 + 8) + 2 * (8 + 8)   # put_dc: luminance sizes up to 7 bits, chrominance 8, differentials 8
    assert L["mba21"] + L["intra_q"] + 5 + dc + 6 * (63 * 28 + 2) <= L["mb_max_bits"]
    assert L["slice_cap"] >= 4 + (6 + 22 * L["mb_max_bits"] + 7) // 8
    pics = E.noise()
    r = A.encode(aq, pics, aq=256, qscale=1, fmt=0)
    assert r.slice_len.max() <= L["slice_cap"], r.slice_len.max()
    round_trip(r.stream, 0, r.recon)
    print(f"noise, q 1, strength 256: longest slice {r.slice_len.max()} of {L['slice_cap']} bytes")


@pytest.mark.parametrize("bitrate", [400_000, 1_500_000])
def test_rate_control(aq, directed, clip, bitrate):
    """efx_encode_rc: the maps stay in qmin .. qmax around the reported picture quantiser, the status bit is the buffer
    model's verdict on the bytes written, the stream decodes; the first picture is coded at clamp(qscale, qmin, qmax)."""
    pics = np.concatenate([clip[:9], directed])
    r = A.encode(aq, pics, aq=256, bitrate=bitrate, qscale=2, **PROFILE)
    assert r.maps.min() >= 3 and int(r.qscales[0]) == 3
    assert np.array_equal(r.maps, np.stack([A.mq_map(p, int(q), 256, 3, 31) for p, q in zip(pics, r.qscales)]))
    assert len(np.unique(r.maps[0])) > 1
    A.check_stream(r.stream, 1, r.maps, f"{bitrate} bit/s")
    under = R.vbv(R.ts_picture_bytes(r.stream), bitrate, PROFILE["vbv_bits"])[0]
    assert bool(r.status & R.ENCODE_VBV) == under and r.status & ~R.ENCODE_VBV == 0
    round_trip(r.stream, 1, r.recon)


def test_rate_control_fixed_quantiser_and_off(aq, clip, tmp_path_factory):
    """qmin == qmax: the clamp makes adaptive quantisation a no-op; strength 0 under rate control is the rate model."""
    rate = R.build(str(tmp_path_factory.mktemp("enc_rate_model")))
    pics = clip[:6]
    fixed = A.encode(aq, pics, aq=256, bitrate=400_000, vbv_bits=250_000, qmin=8, qmax=8, qscale=5)
    plain = A.encode(aq, pics, aq=0, qscale=8)
    assert fixed.stream == plain.stream and (fixed.maps == 8).all()
    off = A.encode(aq, pics, aq=0, bitrate=400_000, qscale=8, **PROFILE)
    want = R.encode(rate, pics, bitrate=400_000, qscale=8, **PROFILE)
    assert off.stream == want.stream and np.array_equal(off.qscales, want.qscales) and off.status == want.status


def test_continuation(aq, directed, clip):
    """2 + 2 pictures with a carried state equal 4 at once, fixed quantiser and rate control."""
    pics = np.concatenate([directed[:2], clip[:2]])
    for kw in (dict(qscale=8), dict(bitrate=400_000, qscale=8, **PROFILE)):
        whole = A.encode(aq, pics, aq=64, first_pts=129003, **kw)
        a = A.encode(aq, pics[:2], aq=64, first_pts=129003, **kw)
        b = A.encode(aq, pics[2:], aq=64, first_pts=129003, state=a.state, **kw)
        assert a.stream + b.stream == whole.stream
        assert np.array_equal(np.concatenate([a.maps, b.maps]), whole.maps)
        assert np.array_equal(np.concatenate([a.recon, b.recon]), whole.recon)
