"""The directed SBC streams of tests/sbc_streams.py on the CPU: what they cover, asserted from their manifests; the writer's
plain-Python model against the oracle's restatement; and the oracle against the reference -- the hashes of
tests/golden/sbc_directed.json everywhere, the reference itself where oracle/_ref is built.  tests/test_gpu_sbc_directed.py
decodes the same streams on the device."""
import json
import os

import numpy as np
import pytest

import oracle
import sbc_streams as S

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sbc_directed.json")) as _f:
    GOLDEN = json.load(_f)


def check_call(call):
    """The oracle's decode of a call -- held to the golden hashes and, where it is built, to the reference.  Returns
    (pcm per stream, int32 [stream, frame, 2] return values and decoded bytes, sb_sample [stream, 16, 2, 8])."""
    data = [s.data for s in call.streams]
    pcm, rets, sb = oracle.sbc_decode_call(data, call.fb)
    assert oracle.sbc_call_hashes(pcm, rets) == GOLDEN[call.name], call.name
    if oracle.have_ref_sbc():
        # (one run of the reference harness per call: all its streams back to back as ONE stream -- the same frames, the
        # filter memory carried from stream to stream on both sides; the golden hashes are the streams one by one)
        whole = np.concatenate(data)
        rpcm, rrets = oracle.ref_sbc_decode(whole, call.fb)
        opcm, orets, _ = oracle.sbc_decode_call([whole], call.fb)
        assert rrets == [tuple(r) for r in orets[0].tolist()], call.name
        assert np.array_equal(rpcm, opcm[0]), call.name
    return pcm, rets, sb


def test_golden_file_lists_every_call():
    names = [S.call_name(k) for k in S.call_names()]
    assert sorted(names) == sorted(GOLDEN) and len(names) == 4 * 129 + 16 * 4 + 3 + 4


@pytest.mark.parametrize("geometry", list(S.GEOMETRIES))
def test_alloc(geometry):
    """Every sampling frequency x allocation method at every bitpool 0..128, the 52 scale-factor shapes in each: the frame
    length the manifest's widths imply is what the oracle's lazy bit reader returns -- for every frame; a width the model and
    the oracle disagreed on would move it (the sample bits are random, the last byte fetched depends on every width)."""
    blocks, mode = S.GEOMETRIES[geometry]
    reached = set()
    for bp in S.BITPOOLS:
        call = S.alloc_call(geometry, bp)
        assert len(call.streams) == 8 and call.frames == 52 and call.fb == S.frame_bytes(blocks, 1 if mode == 0 else 2, bp)
        pcm, rets, _ = check_call(call)
        for i, s in enumerate(call.streams):
            assert s.mode == mode and (s.blocks == blocks).all() and s.ok.all()
            assert (s.scale[:, 0] == S.alloc_shapes()).all() and (s.scale[:, -1] == S.alloc_shapes()[:, ::1 if mode == 0 else -1]).all()
            assert (s.width.astype(int).sum(axis=2) == bp).all()
            assert len(set(s.freq)) == 1 and len(set(s.alloc)) == 1 and (s.bitpool == bp).all()
            reached.add((int(s.freq[0]), int(s.alloc[0]), bp))
            assert np.array_equal(rets[i, :, 0], s.implied_lengths()), s.name
            assert (rets[i, :, 1] == blocks * 8 * s.channels * 2).all()
    assert reached == {(f, a, bp) for f in range(4) for a in range(2) for bp in range(129)}


def test_alloc_shapes_reach_the_slice_counter_edges():
    """The edges of the reference's bit-slice loop that k_sbc.hip's at_least() counts in bytes, found in the directed shapes by
    the model: a subband with bitneed == bitslice + 1 in the slice that ends the loop (counted twice), one at or beyond
    bitslice + 16 (cut off), and all eight needs at -5 under a max_bitneed held at 0."""
    twice = cut = low = False
    for freq in range(4):
        for alloc in range(2):
            for shape in S.alloc_shapes().tolist():
                need = S.bitneed(freq, alloc, shape)
                for bp in (1, 17, 64, 127, 128):
                    bitcount, slicecount, bitslice = 0, 0, max(0, max(need)) + 1
                    while bitcount + slicecount < bp or bitslice == max(0, max(need)) + 1:   # the loop once more, watching
                        bitslice -= 1
                        bitcount += slicecount
                        slicecount = sum(1 if bitslice + 1 < n < bitslice + 16 else 2 if n == bitslice + 1 else 0 for n in need)
                        twice |= bitslice + 1 in need
                        cut |= any(n >= bitslice + 16 for n in need)
                        low |= max(need) == -5 and slicecount > 0
    assert twice and cut and low


@pytest.mark.parametrize("b", list(S.WIDTHS))
def test_dequant(b):
    """Every code of width b at every scale factor is in the one-frame streams' manifests, and the oracle's sb_sample after
    each of those frames is the plain-Python IQUANT of its codes -- also behind a rejected frame (the `gen` layout).  The long
    layouts hold the same frames."""
    table = S.iquant_table(b)
    assert table.tolist() == [[S.iquant(c, b, s) for c in range(1 << b)] for s in range(16)]   # Python integers, every entry
    for layout in S.DEQUANT_LAYOUTS:
        call = S.dequant_call(layout, b)
        _, rets, sb = check_call(call)
        if layout in ("one", "gen"):
            seen = np.zeros((16, 1 << b), dtype=bool)
            for i, s in enumerate(call.streams):
                f = s.frames - 1
                live = s.width[f] > 0
                assert (s.width[f][live] == b).all() and live.any() and len(set(s.scale[f].reshape(-1))) == 1
                seen[int(s.scale[f, 0, 0]), s.codes[f][:, live]] = True
                assert np.array_equal(sb[i], S.last_frame_samples(s)), s.name
                assert rets[i, f, 0] == s.implied_lengths()[f]
            assert seen.all()
            assert len(call.streams) == 16 * max(1, (1 << b) // 128) and np.array_equal(sb, S.dequant_samples(b))
        else:
            one = S.dequant_call("one", b)
            s = call.streams[0]
            assert len(call.streams) == 1 and s.frames == len(one.streams)
            assert np.array_equal(s.codes[:, :, 0], np.concatenate([o.codes[:, :, 0] for o in one.streams]))
            assert np.array_equal(s.codes[:, :, -1], s.codes[:, :, 0]) and (s.width[:, -1] == s.width[:, 0]).all()
            assert np.array_equal(rets[0, :, 0], s.implied_lengths())


def test_iquant_model_wraps_and_truncates():
    """The model's corner cases, spelled out: at scale 15 a 16-bit code of 32768 or more wraps the 32-bit dividend negative,
    and the division truncates toward zero (a floor would give one less)."""
    assert S.iquant(32767, 16, 15) == 0
    assert S.iquant(32768, 16, 15) == -((0x100000000 - (65537 << 15)) // 65535) - 32768 == -65536
    assert S.iquant(65535, 16, 15) == -32768 and S.iquant(0, 16, 15) == -32768
    assert (80001 << 15) - (1 << 32) == -1673494528 and 1673494528 // 65535 == 25535 and 1673494528 % 65535 != 0
    assert S.iquant(40000, 16, 15) == -25535 - 32768    # (floor division would give -25536)
    assert S.iquant(3, 2, 15) == (7 << 15) // 3 - 32768 == 43690


@pytest.mark.parametrize("layout", S.PHASE_LAYOUTS)
def test_phase(layout):
    """Fields of every width 1..16 start at every bit position modulo 32 of the stream (the staged layout: field_staged's 64-bit
    window over dwords) or modulo 8 (field_global's and k_sbc_gen's four bytes and a shift); odd bitpools, odd frame sizes."""
    call = S.phase_call(layout)
    mod = 32 if layout == "staged" else 8
    seen = np.zeros((17, mod), dtype=bool)
    for s in call.streams:
        w, p = s.fields()
        seen[w, p % mod] = True
        assert s.mode == 0 and (s.bitpool & 1).all() and s.fb & 1
        assert max(len(set(x) - {0}) for x in s.width[:, 0].tolist()) >= 4   # widths are mixed inside a frame
    assert seen[1:].all() and not seen[0].any()
    _, rets, _ = check_call(call)
    for i, s in enumerate(call.streams):
        assert np.array_equal(rets[i, s.ok, 0], s.implied_lengths()[s.ok]) and (rets[i, ~s.ok, 0] == -1).all()
    if layout == "staged":
        assert 19 * call.fb + 528 + 8 <= 4096         # k_sbc_par_mono: 16 + 3 frames in reach, the slack behind them
    elif layout == "global":
        assert call.frames >= 17 and 16 * call.fb + 528 > 4096 and all((s.bitpool[0::2] >= 121).all() for s in call.streams)
    else:
        for s in call.streams:
            assert not s.ok[0] and s.ok[1:].all() and call.frames == 16
            assert (s.blocks[:8] == 16).all() and (s.blocks[8:] == 12).all()


def _synthesis_int64(x):
    """Matrixing and windowing of one channel (sbc_decoder.cpp:74-139) over the oracle's tables in int64: x int [blocks, 8] ->
    (matrixing sums, windowing sums, PCM), the sums unwrapped -- each row is wrapped to 32 bits, shifted and handed on as
    the reference does."""
    syn, proto = (t.astype(np.int64) for t in oracle.sbc_tables())
    wrap = lambda a: ((a + (1 << 31)) % (1 << 32)) - (1 << 31)
    M = x.astype(np.int64) @ syn.reshape(16, 8).T
    rows = np.concatenate([np.zeros((10, 16), dtype=np.int64), wrap(M) >> 15])
    T = x.shape[0]
    P = proto.reshape(8, 10)
    W = np.zeros((T, 8), dtype=np.int64)
    for j in range(0, 10, 2):
        W += rows[10 - j:10 - j + T, :8] * P[:, j] + rows[9 - j:9 - j + T, 8:] * P[:, j + 1]
    return M, W, np.clip(wrap(W) >> 15, -0x7FFF, 0x7FFF)


@pytest.mark.parametrize("width,mode", S.RANGE_CALLS)
def test_range(width, mode):
    """Full-scale streams wrap the 32-bit sums of both filter stages and reach both clip values; the streams of levels
    around the clip's edge (width 16) leave the last unclipped values on either side."""
    call = S.range_call(width, mode)
    pcm, _, _ = check_call(call)
    m_out = w_out = False
    for i, s in enumerate(call.streams):
        assert (s.scale == 15).all() and (s.width == width).all() and s.frames * 16 >= 10
        x = S.iquant_table(width)[15][s.codes.astype(np.int64)]          # [frame, block, channel, subband]
        got = pcm[i].reshape(s.frames, s.channels, 16, 8)
        for c in range(s.channels):
            M, W, out = _synthesis_int64(x[:, :, c].reshape(-1, 8))
            assert np.array_equal(out.reshape(s.frames, 16, 8), got[:, c]), s.name
            m_out |= bool((np.abs(M) >= 1 << 31).any())
            w_out |= bool((np.abs(W) >= 1 << 31).any())
    assert m_out and w_out
    allpcm = np.concatenate(pcm)
    assert (allpcm == 0x7FFF).any() and (allpcm == -0x7FFF).any() and allpcm.min() == -0x7FFF
    if width == 16:
        assert np.isin(allpcm, (0x7FFD, 0x7FFE)).any() and np.isin(allpcm, (-0x7FFD, -0x7FFE)).any()
