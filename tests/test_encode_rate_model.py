"""Rate control of the MPEG-1 encoder (espflix_amd/csrc/enc_rate.h with enc_core.h, built for the host by
tests/encode_rate_model.py): the buffer model of include/efx.h, restated here in Python integers, against what the
controller writes.  No GPU; tests/test_gpu_encode_rate.py holds the device to the same host model byte for byte.

Figures of this build (host model, 250 000-bit buffer, qmin 3, qmax 31, GOP 12, search 7, TS): V at 400 / 800 / 1500 kbit/s
keeps at least 16 178 / 15 221 / 11 019 bytes in the buffer, X at 400 kbit/s 16 394; mean luma PSNR of V 36.26 dB at 400 k
(constant q* + 1 = 10: 35.78 dB) and 40.33 dB at 800 k (constant q* + 1 = 6: 39.29 dB)."""
import numpy as np
import pytest

import encode_model as E
import encode_rate_model as R
import export_model as M
import oracle

VBV_BITS, QMIN, QMAX, QSCALE = 250_000, 3, 31, 8
CASES = [("V", 400_000), ("V", 800_000), ("V", 1_500_000), ("X", 400_000), ("N", 400_000)]


@pytest.fixture(scope="module")
def rc(tmp_path_factory):
    return R.build(str(tmp_path_factory.mktemp("enc_rate_model")))


@pytest.fixture(scope="module")
def const(tmp_path_factory):
    return E.build(str(tmp_path_factory.mktemp("enc_model")))


@pytest.fixture(scope="module")
def src(clips):
    ci = {}
    for name in ("splash", "vmedia"):
        n, _, _, frames = oracle.decode(clips[name], 1, flush_last=True, want_frames=True)
        ci[name] = M.strip_to_i420(frames[:n])
    return R.sources(ci)


@pytest.fixture(scope="module")
def runs(rc, src):
    """Every case encoded once, on demand."""
    done = {}

    def get(name, bitrate):
        if (name, bitrate) not in done:
            done[name, bitrate] = R.encode(rc, src[name], bitrate=bitrate, vbv_bits=VBV_BITS, qmin=QMIN, qmax=QMAX, qscale=QSCALE)
        return done[name, bitrate]
    return get


@pytest.fixture(scope="module")
def const_runs(const, src):
    done = {}

    def get(q):
        if q not in done:
            stream, recon = E.encode(const, src["V"], qscale=q)
            done[q] = (R.ts_picture_bytes(stream), E.luma_psnr(src["V"], recon))
        return done[q]
    return get


def check(r, name, bitrate):
    return R.check_stream(r.stream, 1, r.qscales, r.status, bitrate=bitrate, vbv_bits=VBV_BITS, qmin=QMIN, qmax=QMAX, qscale=QSCALE,
                          what=name)


def round_trip(stream, fmt, recon, first_pts=0):
    n, _, pts, frames = oracle.decode(np.frombuffer(stream, dtype=np.uint8), fmt, flush_last=True, want_frames=True)
    assert n == len(recon), (n, len(recon))
    assert np.array_equal(frames, M.i420_to_strip(recon)), "the oracle's pictures differ from the encoder's reconstruction"
    if fmt == 1:
        assert list(pts) == [first_pts + 3003 * k for k in range(n)]
        if oracle.have_ref():
            from espflix_amd import gen
            hashes, rpts, _ = oracle.ref_decode(np.frombuffer(stream, dtype=np.uint8), flush_last=True)
            assert [int(h) for h in hashes] == [gen.fnv1a64(s) for s in M.i420_to_strip(recon)]
            assert list(rpts) == [first_pts + 3003 * k for k in range(n)]


@pytest.mark.parametrize("q", [3, 8, 31])
def test_constant_quantiser(rc, const, src, q):
    """1: qmin = qmax = q is efx_encode at qscale q, whatever the rate: bytes and reconstruction."""
    pics = src["V"][:24]
    r = R.encode(rc, pics, bitrate=400_000, vbv_bits=VBV_BITS, qmin=q, qmax=q, qscale=QSCALE)
    want, want_rec = E.encode(const, pics, qscale=q)
    assert r.stream == want and np.array_equal(r.recon, want_rec)
    assert (r.qscales == q).all()


@pytest.mark.parametrize("name,bitrate", CASES)
def test_status_bit_is_honest(runs, name, bitrate):
    """2: EFX_ENCODE_VBV exactly when the verifier sees F < 0; the quantisers in the stream are the reported ones, all in
    qmin..qmax, the first clamp(qscale, qmin, qmax)."""
    check(runs(name, bitrate), name, bitrate)


@pytest.mark.parametrize("bitrate", [400_000, 800_000, 1_500_000])
def test_v_conforms(runs, bitrate):
    """3"""
    r = runs("V", bitrate)
    under, _, low = check(r, "V", bitrate)
    assert not under and r.status == 0, low


def test_scene_cut_conforms(runs):
    """4: X cuts from easy to hard content on a P picture -- the case the activity measure exists for."""
    r = runs("X", 400_000)
    under, _, low = check(r, "X", 400_000)
    assert not under and r.status == 0, low


def test_noise_shows_debt(runs, src):
    """5: N cannot conform at 400 kbit/s: the bit is set, every picture that starts in debt is coded at qmax, and the
    stream still decodes."""
    r = runs("N", 400_000)
    under, before, _ = check(r, "N", 400_000)
    assert under and r.status == R.ENCODE_VBV
    in_debt = [p for p, f in enumerate(before) if f <= 0]
    assert in_debt and all(int(r.qscales[p]) == QMAX for p in in_debt), (in_debt, r.qscales)
    round_trip(r.stream, 1, r.recon)


@pytest.mark.parametrize("bitrate", [400_000, 800_000])
def test_not_wasteful(runs, const_runs, src, bitrate):
    """6: the yardstick is the encoder itself at constant qscale.  q* = the smallest constant qscale whose stream of V
    conforms (bisection: a coarser quantiser never costs a picture more here); the rate-controlled stream's mean luma PSNR
    is at least that of constant q* + 1."""
    conforms = lambda q: not R.vbv(const_runs(q)[0], bitrate, VBV_BITS)[0]
    lo, hi = 1, 31
    assert conforms(hi)
    while lo < hi:
        mid = (lo + hi) // 2
        if conforms(mid):
            hi = mid
        else:
            lo = mid + 1
    q_star = lo
    assert q_star < 31
    want = const_runs(q_star + 1)[1]
    r = runs("V", bitrate)
    got = E.luma_psnr(src["V"], r.recon)
    print(f"V at {bitrate} bit/s: q* {q_star}, constant {q_star + 1}: {want:.3f} dB, rate control: {got:.3f} dB, {len(r.stream)} bytes")
    assert got >= want


def test_continuation(rc, src):
    """7: V[:36] in one call equals 7 + 12 + 17 pictures with cont: bytes, reconstruction, quantisers, status."""
    kw = dict(bitrate=400_000, vbv_bits=VBV_BITS, qmin=QMIN, qmax=QMAX, qscale=QSCALE, first_pts=129003)
    pics = src["V"][:36]
    whole = R.encode(rc, pics, **kw)
    parts, state, at = [], None, 0
    for n in (7, 12, 17):
        parts.append(R.encode(rc, pics[at:at + n], state=state, **kw))
        state, at = parts[-1].state, at + n
    assert b"".join(p.stream for p in parts) == whole.stream
    assert np.array_equal(np.concatenate([p.recon for p in parts]), whole.recon)
    assert np.array_equal(np.concatenate([p.qscales for p in parts]), whole.qscales)
    assert len(set(int(q) for q in whole.qscales)) > 2
    round_trip(whole.stream, 1, whole.recon, 129003)


@pytest.mark.parametrize("name,bitrate", CASES)
def test_decodes(runs, name, bitrate):
    """8: every stream decodes with the oracle (and the reference, where built) to the reported reconstruction."""
    r = runs(name, bitrate)
    round_trip(r.stream, 1, r.recon)


def test_elementary_stream(rc, src):
    """ES: the cost of a picture is its headers plus slices; the same checks hold."""
    r = R.encode(rc, src["X"], bitrate=400_000, vbv_bits=VBV_BITS, qmin=QMIN, qmax=QMAX, qscale=QSCALE, fmt=0)
    under, _, _ = R.check_stream(r.stream, 0, r.qscales, r.status, bitrate=400_000, vbv_bits=VBV_BITS, qmin=QMIN, qmax=QMAX,
                                 qscale=QSCALE, what="X ES")
    assert not under
    round_trip(r.stream, 0, r.recon)
