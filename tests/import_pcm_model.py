"""NumPy model of efx_import_pcm (include/efx.h's formulas, written out tap by tap with plain floor divisions): downmix,
prototype table, polyphase resampling with a history that carries from call to call.  The C header
(espflix_amd/csrc/import_pcm.h) and the kernels (k_import_pcm.hip) must give these samples bit for bit."""
import math

import numpy as np

P, Q, HALF = 512, 22, 16
TABLE_LEN = HALF * P + 1
HIST = 127
STATE_BYTES = 256
OUT_RATES = (16000, 32000, 44100, 48000)
FREQUENCY = {16000: 0, 32000: 1, 44100: 2, 48000: 3}  # the SBC header's code
INTERLEAVED, PLANAR = 1, 2
LAYOUTS = {"interleaved": INTERLEAVED, "planar": PLANAR}

# the rate pairs the tests run (input, output)
RATE_PAIRS = [(44100, 48000), (8000, 48000), (96000, 48000), (192000, 48000), (22050, 16000), (11025, 32000), (47999, 48000),
              (48000, 48000)]


def rates_ok(r, o):
    return o in OUT_RATES and 8000 <= r <= 192000 and r <= 4 * o


def delay(r, o):
    return 0 if r == o else -(-16 * max(r, o) // o)


def out_samples(r, o, first_in, n_in):
    return -(-(first_in + n_in) * o // r) - -(-first_in * o // r)


def _i0(x):
    """The modified Bessel function by its power series."""
    y, term, total = x * x / 4.0, 1.0, 1.0
    for k in range(1, 64):
        term *= y / (k * k)
        total += term
    return total


_TABLE = None


def table():
    """T[i] = round(2^Q p(i / P)), i = 0 .. 16 P; p(16) = 0."""
    global _TABLE
    if _TABLE is None:
        t = np.zeros(TABLE_LEN, dtype=np.int64)
        i0b = _i0(9.0)
        for i in range(TABLE_LEN - 1):
            u = i / P
            x = math.pi * 0.97 * u
            sinc = 1.0 if i == 0 else math.sin(x) / x
            w = _i0(9.0 * math.sqrt(1.0 - (u / HALF) ** 2)) / i0b
            t[i] = math.floor(2.0 ** Q * 0.97 * sinc * w + 0.5)
        _TABLE = t
    return _TABLE


def weights(channels, mix=None):
    if mix is None or not any(mix):
        return np.full(channels, 32768 // channels, dtype=np.int64)
    w = np.asarray(mix[:channels], dtype=np.int64)
    assert np.abs(w).sum() <= 32768
    return w


def downmix(x, mix=None):
    """x: [..., frames, channels] int16 -> [..., frames] int64 in the int16 range."""
    x = np.asarray(x).astype(np.int64)
    s = (x * weights(x.shape[-1], mix)).sum(axis=-1)
    return np.clip((s + 16384) >> 15, -32768, 32767)


def frames_of(src, n_in, channels, layout):
    """The [n, n_in, channels] view of [n, n_in * channels] elements in either layout."""
    src = np.asarray(src)
    n = src.shape[0]
    if layout in (INTERLEAVED, "interleaved"):
        return src[:, :n_in * channels].reshape(n, n_in, channels)
    return src[:, :n_in * channels].reshape(n, channels, n_in).transpose(0, 2, 1)


def resample(m, r, o, first_in=0, hist=None):
    """m: [n, n_in] mixed samples of this call, hist: [n, 127] the mixed samples in front of them (None: zeros).  Returns
    (y [n, n_out] int16, the new history [n, 127] int16)."""
    m = np.asarray(m).astype(np.int64)
    n, n_in = m.shape
    if hist is None:
        hist = np.zeros((n, HIST), dtype=np.int64)
    ext = np.concatenate([np.asarray(hist).astype(np.int64), m], axis=1)  # ext[:, HIST + j - first_in] = m[j]
    new_hist = ext[:, -HIST:].astype(np.int16)
    if r == o:
        return m.astype(np.int16), new_hist
    T = table()
    M, W = max(r, o), delay(r, o)
    n0 = -(-first_in * o // r)
    nn = n0 + np.arange(out_samples(r, o, first_in, n_in), dtype=np.int64)  # below 2^40 o / r: n r < 2^57
    a = nn * r
    fl = a // o
    acc = np.zeros((n, nn.size), dtype=np.int64)
    for tap in range(2 * W):
        j = fl - 2 * W + 1 + tap
        e = np.abs(j * o - a + W * o)
        q, rho = (e * P) // M, (e * P) % M
        f = (rho * 4096) // M
        qc = np.minimum(q, HALF * P - 1)
        k = np.where(q >= HALF * P, 0, T[qc] + (((T[qc + 1] - T[qc]) * f) >> 12))
        acc += k[None, :] * ext[:, HIST + j - first_in]
    if r > o:
        acc = (acc * o) // r  # floor
    y = np.clip((acc + (1 << (Q - 1))) >> Q, -32768, 32767)
    return y.astype(np.int16), new_hist


def import_pcm(src, r, o, channels, layout=INTERLEAVED, mix=None, first_in=0, hist=None):
    """src: [n, >= n_in * channels] int16 elements with n_in = src.shape[1] // channels.  Returns (y, new history)."""
    src = np.asarray(src)
    n_in = src.shape[1] // channels
    return resample(downmix(frames_of(src, n_in, channels, layout), mix), r, o, first_in, hist)


def state_bytes(hist):
    """The device's state of a stream with this history: 127 int16 and a zero."""
    hist = np.asarray(hist, dtype=np.int16)
    out = np.zeros((hist.shape[0], STATE_BYTES // 2), dtype=np.int16)
    out[:, :HIST] = hist
    return out
