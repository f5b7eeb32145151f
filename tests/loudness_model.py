"""NumPy model of efx_loudness_steps / efx_loudness_gate / efx_pcm_gain, written from the formulas in include/efx.h (not
from espflix_amd/csrc/loudness_px.h): the K-weighting recurrence with Q28 coefficients and 12 fraction bits, every step
started at rest W = step / 2 samples in front of itself, the step energies and peaks, the gates on integer block
energies, the gain and its application.  Steps are independent, so the model is vectorised over (stream, step) and loops
over the W + step time positions."""
import math

import numpy as np

RATES = (16000, 32000, 44100, 48000)
F = 12
COEF_BITS = 28
UNITY = 4096
STEP_DTYPE = np.dtype([("energy", "<u8"), ("peak", "<u4"), ("zero", "<u4")])
REC_DTYPE = np.dtype([("gated_mean", "<u8"), ("max_block", "<u8"), ("n_gated", "<u4"), ("n_blocks", "<u4"), ("n_abs", "<u4"),
                      ("peak", "<u2"), ("gain_q12", "<u2")])


def step_of(rate):
    return rate // 10


def runin_of(rate):
    return rate // 20


def hist_of(rate):
    return (step_of(rate) + runin_of(rate) + 7) & ~7


def state_bytes(rate):
    return 2 * hist_of(rate)


def step_count(rate, first_sample, n_samples):
    return (first_sample + n_samples) // step_of(rate) - first_sample // step_of(rate)


def coefs_float(rate):
    """b0 b1 b2 a1 a2 of the shelf, then of the high pass, as floats."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return shelf + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def coefs(rate):
    return [int(math.floor(c * (1 << COEF_BITS) + 0.5)) for c in coefs_float(rate)]


def steps(x, rate, k=None, watch=None):
    """x: int16 [n_streams, samples], every stream from its first sample.  Returns (energy uint64 [n, n_steps], peak uint32
    [n, n_steps]).  watch: a dict that receives the largest |y|, |z| and |sum of products| seen."""
    x = np.atleast_2d(np.asarray(x)).astype(np.int64)
    k = [int(v) for v in (k if k is not None else coefs(rate))]
    step, W = step_of(rate), runin_of(rate)
    n_steps = x.shape[1] // step
    xp = np.concatenate([np.zeros((x.shape[0], W), dtype=np.int64), x], axis=1)  # samples in front of the stream are zero
    start = np.arange(n_steps) * step  # where step s's run-in begins in xp
    shape = (x.shape[0], n_steps)
    x1, x2, y1, y2, z1, z2, E = (np.zeros(shape, dtype=np.int64) for _ in range(7))
    half = 1 << (COEF_BITS - 1)
    big = [0, 0, 0]
    for i in range(W + step):
        x0 = xp[:, start + i] << F
        a = k[0] * x0 + k[1] * x1 + k[2] * x2 - k[3] * y1 - k[4] * y2
        y = (a + half) >> COEF_BITS
        b = k[5] * y + k[6] * y1 + k[7] * y2 - k[8] * z1 - k[9] * z2
        z = (b + half) >> COEF_BITS
        if watch is not None and a.size:
            big = [max(big[0], int(np.abs(y).max())), max(big[1], int(np.abs(z).max())), max(big[2], int(np.abs(a).max()), int(np.abs(b).max()))]
        if i >= W:
            s = (z + (1 << (F - 5))) >> (F - 4)
            E += s * s
        x2, x1, y2, y1, z2, z1 = x1, x0, y1, y, z1, z
    if watch is not None:
        watch.update(y=big[0], z=big[1], sum=big[2])
    peak = np.abs(x[:, :n_steps * step].reshape(x.shape[0], n_steps, step)).max(axis=2) if n_steps else np.zeros(shape, np.int64)
    return E.astype(np.uint64), peak.astype(np.uint32)


def step_records(x, rate, k=None):
    """The records efx_loudness_steps appends: STEP_DTYPE [n_streams, n_steps]."""
    E, peak = steps(x, rate, k)
    out = np.zeros(E.shape, dtype=STEP_DTYPE)
    out["energy"], out["peak"] = E, peak
    return out


def state(x, rate):
    """The state after the samples x [n_streams, samples] of fresh streams: int16 [n_streams, H], the newest H samples."""
    x = np.atleast_2d(np.asarray(x, dtype=np.int16))
    H = hist_of(rate)
    return np.concatenate([np.zeros((x.shape[0], H), dtype=np.int16), x], axis=1)[:, -H:]


def thresholds(rate, target=-23.0, peak=-1.0):
    unit = 32768.0 ** 2 * 256.0
    return (int(math.floor(10.0 ** ((-70.0 + 0.691) / 10.0) * unit * 4.0 * step_of(rate) + 0.5)),
            int(math.floor(10.0 ** ((target + 0.691) / 10.0) * unit + 0.5)), max(1, int(math.floor(32767.0 * 10.0 ** (peak / 20.0) + 0.5))))


def lufs(block_energy, rate):
    if not block_energy:
        return -math.inf
    return -0.691 + 10.0 * math.log10(int(block_energy) / (4.0 * step_of(rate) * 32768.0 ** 2 * 256.0))


def gain_q12(gated_mean, n_gated, peak, T, C, step):
    if n_gated == 0 or peak == 0:
        return UNITY
    g = math.isqrt(min((T << 24) * 4 * step // max(gated_mean, 1), 1 << 32))
    g = min(g, 4096 * C // peak)
    return max(1, min(32767, g))


def gate(recs, rate, thr, hist=None):
    """recs: STEP_DTYPE [n_steps] of one stream; thr = (abs_thr, target_ms, ceiling); hist: the stream's state (int16 [H]) or
    None.  Returns the stream's record as a REC_DTYPE scalar array, in Python integers throughout."""
    abs_thr, T, C = thr
    E = [int(v) for v in recs["energy"]]
    B = [E[j] + E[j + 1] + E[j + 2] + E[j + 3] for j in range(len(E) - 3)]
    above = [b for b in B if b > abs_thr]
    n_abs, S_abs = len(above), sum(above)
    gated = [b for b in above if 10 * b * n_abs > S_abs]
    peak = max([int(v) for v in recs["peak"]] + [0])
    if hist is not None:
        peak = max(peak, int(np.abs(np.asarray(hist).astype(np.int64)).max()))
    out = np.zeros((), dtype=REC_DTYPE)
    out["gated_mean"] = sum(gated) // len(gated) if gated else 0
    out["max_block"] = max(B) if B else 0
    out["n_gated"], out["n_blocks"], out["n_abs"], out["peak"] = len(gated), len(B), n_abs, peak
    out["gain_q12"] = gain_q12(int(out["gated_mean"]), len(gated), peak, T, C, step_of(rate))
    return out


def apply_gain(x, g):
    return np.clip((np.asarray(x).astype(np.int64) * int(g) + 2048) >> 12, -32768, 32767).astype(np.int16)


def measure(x, rate, target=-23.0, peak=-1.0, k=None):
    """One stream x (int16 [samples]) from steps to record, with the state's samples in the peak: (record, integrated LUFS)."""
    rec = gate(step_records(x, rate, k)[0], rate, thresholds(rate, target, peak), state(x, rate)[0])
    return rec, lufs(int(rec["gated_mean"]), rate)
