"""Scene cuts of the MPEG-1 encoder (espflix_amd/csrc/enc_cut.h with enc_core.h and enc_rate.h, built for the host by
tests/encode_cut_model.py): the measure and the rule of include/efx.h ("scene cuts"), restated here in NumPy, against what
the host model decides and writes.  No GPU; tests/test_gpu_scene_cut.py holds the device to the same host model byte for
byte.

The margins asserted here are those of the source pictures alone (the measure reads no reconstruction): every cut of the two
clips scores at least 160, every other picture whose cut_p is above the floor at most 124; the default threshold of 144 lies
between."""
import numpy as np
import pytest

import encode_cut_model as C
import encode_model as E
import encode_rate_model as R
import export_model as M
import oracle

RATE = dict(bitrate=400_000, vbv_bits=250_000, qmin=3, qmax=31)
CUTS = {"vmedia": {19, 71}, "splash": {12, 92}, "X": {18}}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return C.build(str(tmp_path_factory.mktemp("enc_cut_model")))


@pytest.fixture(scope="module")
def src(clips):
    ci = {}
    for name in ("splash", "vmedia"):
        n, _, _, frames = oracle.decode(clips[name], 1, flush_last=True, want_frames=True)
        ci[name] = M.strip_to_i420(frames[:n])
    out = dict(ci)
    out["X"] = R.sources(ci)["X"]
    return out


@pytest.fixture(scope="module")
def measured(src):
    """The NumPy restatement's sums of the three sources: computed once, never changed."""
    return {name: C.measure(src[name]) for name in CUTS}


@pytest.fixture(scope="module")
def x_cut(model, src):
    """X with gop 12, min_gop 6, TS: the stream most tests look at."""
    return C.encode(model, src["X"], scene_cut=C.THRESHOLD, min_gop=6, first_pts=129003)


def i_pictures(types):
    return [k for k, t in enumerate(types) if int(t) != C.TYPE_P]


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


@pytest.mark.parametrize("name", sorted(CUTS))
def test_cuts_found(model, src, measured, name):
    """1: threshold 144, min_gop 1, gop 255: the cut pictures are exactly the known ones; every cut scores at least 160 and
    every other picture with cut_p above the floor at most 124; the host model's sums are the NumPy restatement's."""
    pics = src[name]
    r = C.encode(model, pics, scene_cut=C.THRESHOLD, min_gop=1, gop=255, search=0, qscale=31)
    ci, cp = measured[name]
    assert np.array_equal(r.cut_i, ci) and np.array_equal(r.cut_p, cp), "enc_cut.h and the NumPy restatement differ"
    assert int(cp[0]) == int(ci[0])
    s = C.scores(ci, cp)
    for k in range(1, len(pics)):
        print(f"{name} picture {k}: score {int(s[k])}, cut_p {int(cp[k])}, type {int(r.types[k])}")
    assert {k for k, t in enumerate(r.types) if int(t) == C.TYPE_CUT} == CUTS[name]
    assert i_pictures(r.types) == [0] + sorted(CUTS[name])
    assert list(r.types) == C.decide(ci, cp, gop=255, threshold=C.THRESHOLD, min_gop=1)
    for k in range(1, len(pics)):
        if k in CUTS[name]:
            assert s[k] >= 160 and cp[k] > C.FLOOR, (name, k, int(s[k]), int(cp[k]))
        elif cp[k] > C.FLOOR:
            assert s[k] <= 124, (name, k, int(s[k]), int(cp[k]))


def test_fades_stay_below_the_floor(measured):
    """The fade-in of splash (pictures 1 .. 7) and picture 93 score 256 on sums below the floor: what kCutFloor is for."""
    ci, cp = measured["splash"]
    s = C.scores(ci, cp)
    for k in list(range(1, 8)) + [93]:
        assert s[k] == 256 and 0 < cp[k] <= C.FLOOR, (k, int(s[k]), int(cp[k]))


def test_picture_types(model, src, x_cut):
    """2: gop 12, min_gop 6: X has I at 0, 12, 18 (by the cut) and 30; vmedia[:36] at 0, 12, 19 (cut) and 31; with min_gop
    8 picture 19 of vmedia stays P (7 pictures after the I at 12) and I falls at 0, 12, 24."""
    assert i_pictures(x_cut.types) == [0, 12, 18, 30] and int(x_cut.types[18]) == C.TYPE_CUT
    assert [int(x_cut.types[k]) for k in (0, 12, 30)] == [C.TYPE_I] * 3
    v = C.encode(model, src["vmedia"][:36], scene_cut=C.THRESHOLD, min_gop=6)
    assert i_pictures(v.types) == [0, 12, 19, 31] and int(v.types[19]) == C.TYPE_CUT
    v8 = C.encode(model, src["vmedia"][:36], scene_cut=C.THRESHOLD, min_gop=8)
    assert i_pictures(v8.types) == [0, 12, 24] and C.TYPE_CUT not in [int(t) for t in v8.types]
    for r, what in ((x_cut, "X"), (v, "vmedia"), (v8, "vmedia min_gop 8")):
        C.check_headers(R.ts_payload(r.stream), r.types, what)


def test_pan_is_no_cut(model):
    """A pan by (4, 0) per picture is found by the search (low scores); the unrelated texture from picture 20 on is a cut."""
    r = C.encode(model, C.pan(), scene_cut=C.THRESHOLD, min_gop=6)
    s = r.scores
    assert i_pictures(r.types) == [0, 12, 20, 32] and int(r.types[20]) == C.TYPE_CUT
    assert all(s[k] <= 124 for k in range(1, 36) if k != 20) and s[20] >= 160, [int(x) for x in s]


@pytest.mark.parametrize("fmt", [0, 1])
def test_identity_with_the_option_off(model, src, tmp_path_factory, fmt):
    """3: threshold 0 is the encoder without scene cuts, byte for byte: the existing host models on the same inputs."""
    pics = src["X"]
    const = E.build(str(tmp_path_factory.mktemp("enc_model")))
    rc = R.build(str(tmp_path_factory.mktemp("enc_rate_model")))
    want, want_rec = E.encode(const, pics, fmt=fmt, first_pts=129003)
    got = C.encode(model, pics, fmt=fmt, first_pts=129003)
    assert got.stream == want and np.array_equal(got.recon, want_rec)
    assert list(got.types) == [C.TYPE_I if k % 12 == 0 else C.TYPE_P for k in range(36)]
    assert not got.cut_i.any() and not got.cut_p.any()
    want = R.encode(rc, pics, fmt=fmt, first_pts=129003, **RATE)
    got = C.encode(model, pics, fmt=fmt, first_pts=129003, **RATE)
    assert got.stream == want.stream and np.array_equal(got.recon, want.recon)
    assert np.array_equal(got.qscales, want.qscales) and got.status == want.status


@pytest.mark.parametrize("fmt", [0, 1])
def test_decodes(model, src, x_cut, fmt):
    """4: the oracle (and the reference, where built) decodes the streams to the model's reconstruction; temporal_reference
    and the GOP headers are as specified."""
    r = x_cut if fmt == 1 else C.encode(model, src["X"], scene_cut=C.THRESHOLD, min_gop=6, fmt=0)
    round_trip(r.stream, fmt, r.recon, 129003)
    C.check_headers(r.stream if fmt == 0 else R.ts_payload(r.stream), r.types, f"X fmt {fmt}")
    # a cut I picture costs what an I picture costs, not what a P picture of 264 failed searches costs
    off = C.encode(model, src["X"], fmt=fmt, first_pts=129003)
    sizes_on, sizes_off = R.picture_sizes_and_quants(r.stream, fmt)[0], R.picture_sizes_and_quants(off.stream, fmt)[0]
    print(f"fmt {fmt}: picture 18 takes {sizes_on[18]} bytes as I, {sizes_off[18]} as P; the streams {len(r.stream)} / {len(off.stream)}")


def test_continuation(model, src, x_cut):
    """5: X in 7 + 11 + 18 pictures equals the single call: the cut is the first picture of the third call, so the decimated
    picture and g cross a call boundary."""
    parts, state, at = [], None, 0
    for n in (7, 11, 18):
        parts.append(C.encode(model, src["X"][at:at + n], scene_cut=C.THRESHOLD, min_gop=6, first_pts=129003, state=state))
        state, at = parts[-1].state, at + n
    assert b"".join(p.stream for p in parts) == x_cut.stream
    assert np.array_equal(np.concatenate([p.recon for p in parts]), x_cut.recon)
    for f in ("types", "cut_i", "cut_p"):
        assert np.array_equal(np.concatenate([getattr(p, f) for p in parts]), getattr(x_cut, f)), f
    assert int(parts[2].types[0]) == C.TYPE_CUT


def test_rate_control(model, src):
    """6: efx_encode_rc's model at 400 kbit/s with scene cuts on: the checks of the rate-control tests hold for X, the cut
    picture is an I picture, and the stream decodes."""
    r = C.encode(model, src["X"], scene_cut=C.THRESHOLD, min_gop=6, **RATE)
    assert i_pictures(r.types) == [0, 12, 18, 30]
    R.check_stream(r.stream, 1, r.qscales, r.status, qscale=8, what="X, scene cuts", **RATE)
    round_trip(r.stream, 1, r.recon)
    C.check_headers(R.ts_payload(r.stream), r.types, "X rc")
