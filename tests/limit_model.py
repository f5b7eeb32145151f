"""NumPy model of efx_limit_peaks / efx_pcm_limit, written from the rule in include/efx.h ("peak limiter"), not from
espflix_amd/csrc/limit_px.h: block peaks, required gains, nodes, the sliding minimum and the box average over windows of
W = 2H + 1 nodes, the line between two nodes, the application.  One stream at a time, int64 throughout, true integer
division (//) wherever the rule says floor."""
import numpy as np

import loudness_model as L

BLOCK = {16000: 16, 32000: 32, 44100: 48, 48000: 48}
MAX_HALF = 64
DEFAULT_HALF = 32
TILE = 256  # blocks of a workgroup's tile, in both kernels (the shapes of the GPU tests follow it)


def block_of(rate):
    return BLOCK.get(rate, 0)


def stream_gain(gated_mean, n_gated, T, step):
    """G: loudness_model.gain_q12 without its peak cap."""
    if n_gated == 0:
        return L.UNITY
    import math
    return max(1, min(32767, math.isqrt(min((int(T) << 24) * 4 * step // max(int(gated_mean), 1), 1 << 32))))


def peaks(x, rate):
    """p of every block of the stream x (int16 [samples]): uint16 [ceil(samples / Bk)]."""
    bk = BLOCK[rate]
    x = np.abs(np.asarray(x).astype(np.int64))
    nb = -(-len(x) // bk)
    return np.pad(x, (0, nb * bk - len(x))).reshape(nb, bk).max(axis=1).astype(np.uint16) if nb else np.zeros(0, np.uint16)


def required(p, G, C):
    p = np.asarray(p).astype(np.int64)
    return np.where(p == 0, G, np.minimum(G, 4096 * C // np.maximum(p, 1)))


def nodes(p_of, b0, b1, H, G, C):
    """a[b0 .. b1] (b1 inclusive).  p_of(lo, hi): the peaks of blocks lo .. hi - 1 as the call sees them (0 outside)."""
    W = 2 * H + 1
    r = required(p_of(b0 - 2 * H - 1, b1 + 2 * H + 1), G, C)          # blocks b0 - 2H - 1 .. b1 + 2H
    q = np.minimum(r[:-1], r[1:])                                     # nodes b0 - 2H .. b1 + 2H
    M = np.lib.stride_tricks.sliding_window_view(q, W).min(axis=1)    # nodes b0 - H .. b1 + H
    return np.lib.stride_tricks.sliding_window_view(M, W).sum(axis=1) // W


def row_view(row, peaks_first):
    """p_of over a row of entries whose entry 0 is stream block peaks_first; blocks outside it are 0."""
    row = np.asarray(row).astype(np.int64)

    def p_of(lo, hi):
        b = np.arange(lo, hi)
        e = b - peaks_first
        ok = (e >= 0) & (e < len(row))
        out = np.zeros(hi - lo, dtype=np.int64)
        out[ok] = row[e[ok]]
        return out
    return p_of


def gains(n, first_block, rate, p_of, H, G, C):
    """g of the n samples that begin at block first_block: int64 [n]."""
    bk = BLOCK[rate]
    nb = -(-n // bk)
    a = nodes(p_of, first_block, first_block + nb, H, G, C)
    t = np.arange(bk)
    g = (a[:-1, None] * (bk - t)[None, :] + a[1:, None] * t[None, :]) // bk
    return g.reshape(-1)[:n]


def limit(x, rate, G, C, H=DEFAULT_HALF, first_sample=0, row=None, peaks_first=0, want_gains=False):
    """efx_pcm_limit for one stream's piece x that begins at stream sample first_sample, with the peaks row given (None: the
    piece is the whole stream and its own peaks are the row)."""
    bk = BLOCK[rate]
    assert first_sample % bk == 0 and 1 <= H <= MAX_HALF
    if row is None:
        assert first_sample == 0
        row, peaks_first = peaks(x, rate), 0
    g = gains(len(x), first_sample // bk, rate, row_view(row, peaks_first), H, int(G), int(C))
    y = np.clip((np.asarray(x).astype(np.int64) * g + 2048) >> 12, -32768, 32767).astype(np.int16)
    return (y, g) if want_gains else y


def peaky_title(rate, seconds=12.3):
    """The issue's peaky title: noise and a 440 Hz tone at about -31 LUFS with three 2 ms full-scale bursts."""
    n = int(round(seconds * rate))
    t = np.arange(n) / rate
    x = np.random.default_rng(1).normal(0, 400, n) + 800 * np.sin(2 * np.pi * 440 * t)
    for s in (0.7, 4.7, 8.7):
        i0, i1 = int(round(s * rate)), int(round((s + 0.002) * rate))
        x[i0:i1] += 31000 * np.sin(2 * np.pi * 1000 * t[i0:i1])
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)
