"""The SBC encoder's arithmetic (espflix_amd/csrc/sbc_enc_core.h) on the host, no GPU: tests/sbc_enc_model_main.cpp makes the
decisions k_sbc_enc.hip makes.  Its frames are decoded by the test oracle (and by the unmodified reference decoder where
oracle/_ref is built); its decisions are checked for exactness; its quality is measured against a double-precision encoder
straight from A2DP Appendix B (tests/sbc_encode_float.py).

Regenerate tests/golden/sbc_encode_snr.json (the float yardstick's SNRs) with `python tests/test_sbc_encode_model.py`."""
import json
import os
import sys

import numpy as np
import pytest

import oracle
import sbc_encode_float as F
import sbc_encode_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNR_JSON = os.path.join(ROOT, "tests", "golden", "sbc_encode_snr.json")
HAVE_REF_SBC = os.path.exists(os.path.join(oracle.REF_DIR, "efx_ref_sbc"))
BITPOOLS = (2, 19, 28, 53, 128)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return M.build(str(tmp_path_factory.mktemp("sbc_enc_model")))


def mixed_pcm(blocks: int, channels: int, n_frames: int = 10, seed: int = 3) -> np.ndarray:
    """A chord that fades in over noise, different per channel, laid out frame-planar."""
    n = n_frames * blocks * 8
    lines = []
    for c in range(channels):
        x = (M.signal("chord", n).astype(np.float64) * np.linspace(0.05, 1.5, n) +
             M.signal("white", n, seed + c).astype(np.float64) * 0.1 * (c + 1))
        lines.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return np.stack(lines).reshape(channels, n_frames, blocks * 8).transpose(1, 0, 2).reshape(-1)


@pytest.mark.parametrize("mode", [0, 1], ids=["mono", "dual"])
@pytest.mark.parametrize("blocks", [4, 8, 12, 16])
@pytest.mark.parametrize("allocation", [0, 1], ids=["loudness", "snr"])
def test_frames_decode_and_decisions_are_exact(exe, mode, blocks, allocation):
    """Items 1 and 2: every frame decodes with return value frame_bytes and blocks x 8 x channels x 2 bytes, the header is as
    asked, the CRC is the standard's; every scale factor is the smallest that fits the integer analysis' largest |S| (or
    15), every quantised sample is at most 2^bits - 2, and the widths this file's copy of the decoder's allocation derives
    spend exactly the bitpool: the frame ends at frame_bytes."""
    ch = 2 if mode else 1
    pcm = mixed_pcm(blocks, ch)
    for bitpool in BITPOOLS:
        frames, maxabs, _, _ = M.encode(exe, pcm, blocks=blocks, mode=mode, allocation=allocation, bitpool=bitpool)
        fb = M.frame_bytes(blocks, ch, bitpool)
        assert frames.shape == (1, 10, fb)
        want_ret = [(fb, blocks * 8 * ch * 2)] * 10
        got, rets = oracle.sbc_decode(frames.reshape(-1), fb)
        assert rets == want_ret, (bitpool, rets)
        if HAVE_REF_SBC:
            ref, rrets = oracle.ref_sbc_decode(frames.reshape(-1), fb)
            assert rrets == want_ret and np.array_equal(ref, got), bitpool
        for f in range(10):
            h = M.parse_frame(frames[0, f])
            assert (h["sync"], h["frequency"], h["blocks"], h["mode"], h["allocation"], h["subbands"], h["bitpool"]) == \
                (0x9C, 3, blocks, mode, allocation, 8, bitpool)
            assert h["crc"] == h["crc_want"]
            assert h["end"] == fb
            assert (h["bits"].sum(axis=1) == bitpool).all()
            for c in range(ch):
                for sb in range(8):
                    mx, s = int(maxabs[0, f, c, sb]), int(h["scale"][c, sb])
                    assert mx < (1 << (s + 15)) or s == 15
                    assert s == 0 or mx >= (1 << (s + 14)), "a smaller scale factor fits"
                    n = int(h["bits"][c, sb])
                    if n:
                        assert 0 <= h["q"][:, c, sb].max() <= (1 << n) - 2
                    else:
                        assert (h["q"][:, c, sb] == -1).all()


# -- quality: items 3 and 4 ------------------------------------------------------------------------------------------------

def quality_cases():
    """(id, pcm [channels, samples], options, channel measured)."""
    out = []
    for alloc, aname in ((0, "loudness"), (1, "snr")):
        for name in M.SIGNALS:
            for bp in (28, 53):
                out.append((f"{name}_{aname}_{bp}", M.signal(name)[None], dict(mode=0, allocation=alloc, bitpool=bp), 0))
    pair = np.stack([M.signal("chord"), M.signal("lowpass")])
    for c, name in enumerate(("chord", "lowpass")):
        out.append((f"dual_{name}_53", pair, dict(mode=1, allocation=0, bitpool=53), c))
    return out


def decode_channel(frames, fb, channels, c):
    pcm, _ = oracle.sbc_decode(np.asarray(frames).reshape(-1), fb)
    return M.deplanar(pcm, 16, channels)[c]


def float_snr(case):
    _, pcm, opt, c = case
    ch = pcm.shape[0]
    fr = F.encode(pcm, blocks=16, **opt)
    dec = decode_channel(fr, fr.shape[1], ch, c)
    g, snr = M.fit(pcm[c], dec)
    return g, snr, M.best_delay(pcm[c], dec)


def int_snr(exe, case):
    _, pcm, opt, c = case
    ch = pcm.shape[0]
    planar = pcm.reshape(ch, -1, 128).transpose(1, 0, 2).reshape(-1)
    fr, _, _, _ = M.encode(exe, planar, blocks=16, **opt)
    dec = decode_channel(fr, fr.shape[2], ch, c)
    g, snr = M.fit(pcm[c], dec)
    return g, snr, M.best_delay(pcm[c], dec)


def test_quality_against_the_float_yardstick(exe):
    """Items 3 and 4.  Every case: the integer model's SNR through the oracle's decoder is at least the float yardstick's
    less 1.0 dB (a 32-bit integer analysis has its rounding floor tens of dB below every quantisation floor here, so a
    larger loss is an error, not arithmetic).  The yardstick's own SNRs are those recorded in tests/golden/
    sbc_encode_snr.json (0.01 dB).  Every case whose yardstick SNR is at least 40 dB: fitted gain within 1 +- 0.005, best
    alignment 73 samples; at least half of the ten mono loudness cases qualify."""
    recorded = json.load(open(SNR_JSON))
    cases = quality_cases()
    assert sorted(recorded) == sorted(c[0] for c in cases)
    qualified = 0
    failures = []
    for case in cases:
        gf, sf, _ = float_snr(case)
        gi, si, di = int_snr(exe, case)
        print(f"{case[0]:24s} float {sf:6.2f} dB gain {gf:.4f} | integer {si:6.2f} dB gain {gi:.4f} delay {di}")
        assert abs(sf - recorded[case[0]]) <= 0.01, (case[0], sf, recorded[case[0]])
        if si < sf - 1.0:
            failures.append((case[0], si, sf))
        if sf >= 40:
            if "_loudness_" in case[0]:
                qualified += 1
            if abs(gi - 1) > 0.005 or di != M.DELAY:
                failures.append((case[0], "gain", gi, "delay", di))
    assert not failures, failures
    assert qualified >= 5, qualified


@pytest.mark.parametrize("allocation", [0, 1], ids=["loudness", "snr"])
def test_silence_and_the_constant_one(exe, allocation):
    """Item 4: digital silence decodes to all zeros at bitpool 2, 28 and 128.  The constant 1 decodes to values of magnitude
    at most 1 at bitpool 2, 19 and 28.  Not at 128, and not with the float yardstick's frames either (it measures 9): there
    every subband has 16 bits at scale factor 0, and the decoder's integer reconstruction (2q + 1) / 65535 - 1 turns every
    subband sample below zero, however small, into -1.  An error of at most 1 in each of the 8 subbands, in the decoder's
    halved amplitude convention (2 in PCM), bounds the output by 16 there."""
    for bitpool in (2, 28, 128):
        fr, _, _, _ = M.encode(exe, M.signal("silence"), allocation=allocation, bitpool=bitpool)
        pcm, _ = oracle.sbc_decode(fr.reshape(-1), fr.shape[2])
        assert pcm.size == 60 * 128 and not pcm.any(), bitpool
    one = M.signal("one")
    for bitpool, bound in ((2, 1), (19, 1), (28, 1), (128, 16)):
        fr, _, _, _ = M.encode(exe, one, allocation=allocation, bitpool=bitpool)
        pcm, _ = oracle.sbc_decode(fr.reshape(-1), fr.shape[2])
        print("constant 1, bitpool", bitpool, "largest magnitude", np.abs(pcm).max())
        assert np.abs(pcm).max() <= bound, (bitpool, np.abs(pcm).max())


@pytest.mark.parametrize("mode,layout", [(0, 0), (1, 0), (1, 1)], ids=["mono", "dual_planar", "dual_interleaved"])
def test_continuation_through_the_state(exe, mode, layout):
    """Item 5: 60 frames in one call and in calls of 1 + 7 + 52 frames give the same bytes and leave the same state."""
    ch = 2 if mode else 1
    lines = np.stack([M.signal("chord"), M.signal("lowpass")][:ch])
    if layout:
        pcm = lines.T.reshape(-1)
    else:
        pcm = lines.reshape(ch, 60, 128).transpose(1, 0, 2).reshape(-1)
    whole, _, st_whole, _ = M.encode(exe, pcm, mode=mode, layout=layout)
    per = 128 * ch
    parts, state, at = [], None, 0
    for n in (1, 7, 52):
        fr, _, state, _ = M.encode(exe, pcm[at * per:(at + n) * per], mode=mode, layout=layout, state=state)
        parts.append(fr[0])
        at += n
    assert np.array_equal(np.concatenate(parts), whole[0])
    assert np.array_equal(state, st_whole)
    if layout:  # the two layouts hold the same samples: the same frames
        planar = lines.reshape(ch, 60, 128).transpose(1, 0, 2).reshape(-1)
        assert np.array_equal(M.encode(exe, planar, mode=mode, layout=0)[0], whole)


def test_worst_case_input_does_not_wrap(exe):
    """Item 5: full scale on every tap with the sign of its coefficient (and mirrored), for each of the eight folded window
    sums: the model evaluates every window sum and every subband sample in 64 bits as well and reports a difference from
    the 32-bit value.  The largest |S| stays below 2^31 and shows that the inputs do reach past 2^29."""
    w = M.worst_case()
    frames, maxabs, _, status = M.encode(exe, w, check=False)
    assert status == 0, "a 32-bit intermediate of the analysis wrapped"
    assert (1 << 29) < int(maxabs.max()) < (1 << 31)
    fb = frames.shape[2]
    for s in range(w.shape[0]):
        _, rets = oracle.sbc_decode(frames[s].reshape(-1), fb)
        assert rets == [(fb, 256)] * frames.shape[1]


def test_frame_bytes_formula():
    assert M.frame_bytes(16, 1, 28) == 64 and M.frame_bytes(16, 2, 128) == 524 and M.frame_bytes(4, 1, 2) == 9


if __name__ == "__main__":
    out = {}
    for case in quality_cases():
        g, snr, d = float_snr(case)
        out[case[0]] = round(snr, 4)
        print(f"{case[0]:24s} {snr:7.3f} dB gain {g:.4f} delay {d}")
    with open(SNR_JSON, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    sys.exit(0)
