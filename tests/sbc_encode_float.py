"""A double-precision SBC encoder straight from A2DP Appendix B: the yardstick the integer encoder's quality is measured
against (tests/test_sbc_encode_model.py).  Not product code.  8 subbands, mono or dual channel, the subband samples in
the amplitude convention of the reference decoder (src/sbc_decoder.cpp:257-264,330-334: a sample is reconstructed
inside (-2^scale, 2^scale)), which is the standard's analysis halved."""
import numpy as np

import sbc_encode_model as M


def encode(pcm, *, blocks=16, mode=0, allocation=0, bitpool=28, frequency=3) -> np.ndarray:
    """pcm: int16 [channels, samples] (or 1-D for mono), a fresh encoder.  Returns uint8 [n_frames, frame_bytes]."""
    pcm = np.asarray(pcm, dtype=np.float64)
    if pcm.ndim == 1:
        pcm = pcm[None]
    ch = 2 if mode else 1
    assert pcm.shape[0] == ch
    spf = blocks * 8
    n_frames = pcm.shape[1] // spf
    C = M._proto()
    cosm = np.array([[np.cos((sb + 0.5) * (i - 4) * np.pi / 8) for i in range(16)] for sb in range(8)])
    fb = M.frame_bytes(blocks, ch, bitpool)
    out = np.zeros((n_frames, fb), dtype=np.uint8)
    line = np.concatenate([np.zeros((ch, M.HIST)), pcm], axis=1)
    for f in range(n_frames):
        S = np.empty((blocks, ch, 8))
        for c in range(ch):
            for blk in range(blocks):
                newest = M.HIST + f * spf + blk * 8 + 7
                X = line[c, newest - 79:newest + 1][::-1]
                Y = (C * X).reshape(5, 16).sum(axis=0)
                S[blk, c] = 0.5 * (cosm @ Y)
        mx = np.abs(S).max(axis=0)
        scale = np.zeros((ch, 8), dtype=np.int64)
        for c in range(ch):
            for sb in range(8):
                s = 0
                while s < 15 and not mx[c, sb] < 2 ** s:
                    s += 1
                scale[c, sb] = s
        bits = [M.allocation_bits(frequency, allocation, bitpool, scale[c]) for c in range(ch)]
        fr = out[f]
        fr[0] = 0x9C
        fr[1] = frequency << 6 | (blocks // 4 - 1) << 4 | mode << 2 | allocation << 1 | 1
        fr[2] = bitpool
        for c in range(ch):
            for p in range(4):
                fr[4 + c * 4 + p] = scale[c, 2 * p] << 4 | scale[c, 2 * p + 1]
        fr[3] = M.crc8(fr[1:3].tolist() + fr[4:4 + 4 * ch].tolist())
        stream = []
        for blk in range(blocks):
            for c in range(ch):
                for sb in range(8):
                    n = bits[c][sb]
                    if n:
                        s = int(scale[c, sb])
                        q = int(np.floor((S[blk, c, sb] + 2.0 ** s) * (2 ** n - 1) / 2.0 ** (s + 1)))
                        q = min(max(q, 0), 2 ** n - 2)
                        stream.extend((q >> i) & 1 for i in range(n - 1, -1, -1))
        packed = np.packbits(np.array(stream, dtype=np.uint8))
        assert 4 + 4 * ch + packed.size == fb
        fr[4 + 4 * ch:] = packed
    return out
