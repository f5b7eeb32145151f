"""NumPy model of the import's HDR stage (include/efx.h, "HDR sources"): the 10-bit import, the matrix and gamut
coefficients recomputed in rational arithmetic, the two tables recomputed in float64, the integer item (one chroma site and
its 2 x 2 luma samples) and one picture; and beside it a float64 yardstick of the same map -- matrix, PQ EOTF, BT.2390
EETF, BT.2020 -> BT.709, gamma 1 / 2.4 and the BT.601 matrix, nothing rounded before the end.  It shares no code with
espflix_amd/csrc/hdr_px.h."""
from fractions import Fraction as F

import numpy as np

import colour_model as K
import import_model as M

ONE = 1 << 14
GAMUT_ONE = 1 << 28
POS_ONE = 1 << 24        # the source's non-linear R', G', B': steps of 2^-24
PQ_BITS = 11
PQ_ENTRIES = (1 << PQ_BITS) + 1   # E' = i / 2^PQ_BITS
PQ_FRAC = 24 - PQ_BITS
GAM_ENTRIES = 1217       # 0 .. 63 direct, then 64 entries per octave up to 2^24
LIN_ONE = 1 << 24
E_ONE = 1 << 15
LUMA = (16763, 32910, 6391)                 # 219 x (0.299, 0.587, 0.114) in steps of 2^-8: sums to 219 x 256
CB = (-4838, -9498, 14336)                  # 224 x (-0.168736, -0.331264, 0.5) in steps of 2^-7: sums to 0
CR = (14336, -12005, -2331)                 # 224 x (0.5, -0.418688, -0.081312)
PRIMARIES = {9: ((F("0.708"), F("0.292")), (F("0.170"), F("0.797")), (F("0.131"), F("0.046"))),
             1: ((F("0.64"), F("0.33")), (F("0.30"), F("0.60")), (F("0.15"), F("0.06")))}
WHITE = (F("0.3127"), F("0.3290"))
PEAKS = (400, 1000, 4000)
SETTINGS = [(peak, full, prim) for peak in PEAKS for full in (0, 1) for prim in (9, 1)]


def rnd(v):
    return int((v + F(1, 2)).__floor__())


# ---- coefficients (Fractions) -----------------------------------------------------------------------------------------------
def matrix_exact(code, full_range):
    """(sy, rv, gu, gv, bu) as Fractions: R' = sy (Y10 - y0) + rv (Cr10 - 512) and so on, R' in [0, 1]; and y0."""
    kr, kb = (F(s) for s in K.MATRICES[code])
    kg = 1 - kr - kb
    sy, sc, y0 = (F(1, 1020), F(1, 1020), 0) if full_range else (F(1, 876), F(1, 896), 64)
    return (sy, 2 * (1 - kr) * sc, -2 * (1 - kb) * kb / kg * sc, -2 * (1 - kr) * kr / kg * sc, 2 * (1 - kb) * sc), y0


def matrix_coefs(code, full_range, height=0):
    """([qy, qrv, qgu, qgv, qbu], y0): round(2^14 x 2^24 x exact): R' comes out in steps of 2^-24."""
    m, y0 = matrix_exact(K.resolve(code, height), full_range)
    return [rnd(v * POS_ONE * ONE) for v in m], y0


def _inv3(m):
    (a, b, c), (d, e, f), (g, h, i) = m
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    return [[v / det for v in row] for row in adj]


def _mul3(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def rgb_to_xyz(prim):
    cols = [(x / y, F(1), (1 - x - y) / y) for x, y in PRIMARIES[prim]]
    m = [[cols[j][i] for j in range(3)] for i in range(3)]
    w = (WHITE[0] / WHITE[1], F(1), (1 - WHITE[0] - WHITE[1]) / WHITE[1])
    s = [sum(r[j] * w[j] for j in range(3)) for r in _inv3(m)]
    return [[m[i][j] * s[j] for j in range(3)] for i in range(3)]


def gamut_exact(primaries):
    """Linear RGB of `primaries` to linear BT.709 RGB, Fractions."""
    return _mul3(_inv3(rgb_to_xyz(1)), rgb_to_xyz(primaries))


def gamut_coefs(primaries):
    """Nine ints in steps of 2^-28, row major; what a row's rounded entries miss of 2^28 goes to its diagonal entry."""
    q = [[rnd(v * GAMUT_ONE) for v in row] for row in gamut_exact(primaries)]
    for i in range(3):
        q[i][i] += GAMUT_ONE - sum(q[i])
    return [v for row in q for v in row]


# ---- SMPTE ST 2084 and BT.2390, float64 ---------------------------------------------------------------------------------------
M1, M2 = 2610 / 16384, 2523 / 4096 * 128
C1, C2, C3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32


def pq_eotf(e):
    """PQ code 0 .. 1 -> nits."""
    p = np.power(np.asarray(e, dtype=np.float64), 1 / M2)
    return 10000 * np.power(np.maximum(p - C1, 0) / (C2 - C3 * p), 1 / M1)


def pq_inverse(nits):
    y = np.power(np.asarray(nits, dtype=np.float64) / 10000, M1)
    return np.power((C1 + C2 * y) / (1 + C3 * y), M2)


def tone_curve(e, peak):
    """PQ code of the source -> display light relative to 100 nits (BT.2390 EETF without black lift, then the EOTF)."""
    pk = float(pq_inverse(peak))
    max_lum = float(pq_inverse(100)) / pk
    ks = 1.5 * max_lum - 0.5
    e1 = np.minimum(1.0, np.asarray(e, dtype=np.float64) / pk)
    t = np.maximum(e1 - ks, 0) / (1 - ks)
    t2, t3 = t * t, t * t * t
    spline = (2 * t3 - 3 * t2 + 1) * ks + (t3 - 2 * t2 + t) * (1 - ks) + (-2 * t3 + 3 * t2) * max_lum
    e2 = np.where(e1 < ks, e1, spline)
    return pq_eotf(e2 * pk) / 100


def gam_x(idx):
    """The linear value (steps of 2^-24) of entry idx of the second table."""
    idx = np.asarray(idx, dtype=np.int64)
    s = np.maximum(idx // 64 - 1, 0)
    return (idx - 64 * s) << s


def tables(peak):
    """(pq, gam): the first table as int64 (PQ_ENTRIES), the second (GAM_ENTRIES), recomputed in float64."""
    lin = tone_curve(np.arange(PQ_ENTRIES) / (PQ_ENTRIES - 1), peak or 1000)
    pq = np.floor(np.minimum(lin, 1.0) * LIN_ONE + 0.5).astype(np.int64)
    gam = np.floor(np.power(gam_x(np.arange(GAM_ENTRIES)) / LIN_ONE, 1 / 2.4) * E_ONE + 0.5).astype(np.int64)
    return pq, gam


# ---- the integer item ----------------------------------------------------------------------------------------------------------
class Setting:
    """Everything the integer model reads: the coefficients from Fractions, the tables as given (the library's own, or
    tables(peak))."""

    def __init__(self, peak=1000, full_range=0, primaries=9, matrix=9, height=0, pq=None, gam=None):
        self.q, self.y0 = matrix_coefs(matrix, full_range, height)
        self.g = gamut_coefs(primaries)
        if pq is None:
            pq, gam = tables(peak)
        self.pq, self.gam = np.asarray(pq, dtype=np.int64), np.asarray(gam, dtype=np.int64)
        self.peak, self.full_range, self.primaries, self.matrix = peak, full_range, primaries, matrix


def sdr_rgb(s, y10, cb10, cr10):
    """Arrays of 10-bit samples -> the SDR R', G', B' in steps of 2^-15 (three int64 arrays)."""
    y = np.asarray(y10, dtype=np.int64) - s.y0
    u, v = np.asarray(cb10, dtype=np.int64) - 512, np.asarray(cr10, dtype=np.int64) - 512
    qy, qrv, qgu, qgv, qbu = s.q
    e = [np.clip((qy * y + t + 8192) >> 14, 0, POS_ONE) for t in (qrv * v, qgu * u + qgv * v, qbu * u)]
    lin = []
    for p in e:
        i, f = p >> PQ_FRAC, p & ((1 << PQ_FRAC) - 1)
        a, b = s.pq[i], s.pq[np.minimum(i + 1, PQ_ENTRIES - 1)]
        lin.append(a + (((b - a) * f + (1 << (PQ_FRAC - 1))) >> PQ_FRAC))
    out = []
    for r in range(3):
        x = np.clip((s.g[3 * r] * lin[0] + s.g[3 * r + 1] * lin[1] + s.g[3 * r + 2] * lin[2] + (GAMUT_ONE >> 1)) >> 28, 0, LIN_ONE)
        top = np.zeros_like(x)
        nz = x > 0
        top[nz] = np.floor(np.log2(x[nz].astype(np.float64))).astype(np.int64)   # (exact: x < 2^53)
        sh = np.maximum(top - 6, 0)
        idx = 64 * sh + (x >> sh)
        f = x & ((1 << sh) - 1)
        a, b = s.gam[idx], s.gam[np.minimum(idx + 1, GAM_ENTRIES - 1)]
        out.append(a + (((b - a) * f + ((1 << sh) >> 1)) >> sh))
    return out


def luma(rgb):
    return np.clip(16 + ((LUMA[0] * rgb[0] + LUMA[1] * rgb[1] + LUMA[2] * rgb[2] + (1 << 22)) >> 23), 0, 255)


def chroma(sum4):
    """(Cb', Cr') from the sums of the four pixels' R', G', B'."""
    cb = 128 + ((CB[0] * sum4[0] + CB[1] * sum4[1] + CB[2] * sum4[2] + (1 << 23)) >> 24)
    cr = 128 + ((CR[0] * sum4[0] + CR[1] * sum4[1] + CR[2] * sum4[2] + (1 << 23)) >> 24)
    return np.clip(cb, 0, 255), np.clip(cr, 0, 255)


def item(s, y4, cb10, cr10):
    """y4: (..., 4) luma samples of the items, cb10 / cr10: (...) -> (Y' (..., 4), Cb', Cr')."""
    rgb = sdr_rgb(s, y4, np.asarray(cb10)[..., None], np.asarray(cr10)[..., None])
    cb, cr = chroma([c.sum(axis=-1) for c in rgb])
    return luma(rgb), cb, cr


# ---- the float64 yardstick ------------------------------------------------------------------------------------------------------
def yard_rgb(peak, full_range, primaries, matrix, y10, cb10, cr10):
    """The SDR R', G', B' in float64, nothing rounded."""
    kr, kb = (float(F(v)) for v in K.MATRICES[matrix])
    kg = 1 - kr - kb
    if full_range:
        y, pb, pr = np.asarray(y10) / 1020.0, (np.asarray(cb10) - 512) / 1020.0, (np.asarray(cr10) - 512) / 1020.0
    else:
        y, pb, pr = (np.asarray(y10) - 64) / 876.0, (np.asarray(cb10) - 512) / 896.0, (np.asarray(cr10) - 512) / 896.0
    r = y + 2 * (1 - kr) * pr
    b = y + 2 * (1 - kb) * pb
    g = (y - kr * r - kb * b) / kg
    lin = [tone_curve(np.clip(c, 0, 1), peak) for c in (r, g, b)]
    m = [[float(v) for v in row] for row in gamut_exact(primaries)]
    return [np.power(np.clip(m[i][0] * lin[0] + m[i][1] * lin[1] + m[i][2] * lin[2], 0, 1), 1 / 2.4) for i in range(3)]


def yard_luma(rgb):
    return np.clip(np.floor(16 + 219 * (0.299 * rgb[0] + 0.587 * rgb[1] + 0.114 * rgb[2]) + 0.5), 0, 255).astype(np.int64)


def yard_chroma(mean_rgb):
    r, g, b = mean_rgb
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb, cr = 128 + 224 * (b - y) / 1.772, 128 + 224 * (r - y) / 1.402
    return tuple(np.clip(np.floor(c + 0.5), 0, 255).astype(np.int64) for c in (cb, cr))


# ---- pictures ---------------------------------------------------------------------------------------------------------------------
def resample10(plane, dw, dh):
    """import_model.resample with the last rounding at 10 bits: (sum + 2^19) >> 20, 0 .. 1020."""
    h, w = plane.shape
    kx, ky = M.tap_matrix(w, dw), M.tap_matrix(h, dh)
    hs = ((plane.astype(np.float64) @ kx.T.astype(np.float64)).astype(np.int64) + 32) >> 6   # (exact: every sum is below 2^53)
    return ((ky.astype(np.float64) @ hs.astype(np.float64)).astype(np.int64) + (1 << 19)) >> 20


def import10(src, width, height, crop=None, dst=None):
    """One packed I420 picture -> (Y10 (dh, dw), Cb10, Cr10 (dh / 2, dw / 2)) of the destination rectangle."""
    crop = crop or (0, 0, width, height)
    _, _, dw, dh = dst or (0, 0, M.W, M.H)
    y, u, v = M.source_planes(src, "i420", width, height, crop, False)
    return resample10(y, dw, dh), resample10(u, dw // 2, dh // 2), resample10(v, dw // 2, dh // 2)


def import_image(s, src, width, height, crop=None, dst=None):
    """One packed I420 picture -> the 101376 bytes of the HDR import: tonemap(import10) inside the rectangle."""
    dx, dy, dw, dh = dst or (0, 0, M.W, M.H)
    y10, cb10, cr10 = import10(src, width, height, crop, dst)
    y4 = y10.reshape(dh // 2, 2, dw // 2, 2).transpose(0, 2, 1, 3).reshape(dh // 2, dw // 2, 4)
    yy, cb, cr = item(s, y4, cb10, cr10)
    out_y = np.full((M.H, M.W), 16, dtype=np.uint8)
    out_u = np.full((M.CH, M.CW), 128, dtype=np.uint8)
    out_v = np.full((M.CH, M.CW), 128, dtype=np.uint8)
    out_y[dy:dy + dh, dx:dx + dw] = yy.reshape(dh // 2, dw // 2, 2, 2).transpose(0, 2, 1, 3).reshape(dh, dw)
    out_u[dy // 2:(dy + dh) // 2, dx // 2:(dx + dw) // 2] = cb
    out_v[dy // 2:(dy + dh) // 2, dx // 2:(dx + dw) // 2] = cr
    return np.concatenate([out_y.reshape(-1), out_u.reshape(-1), out_v.reshape(-1)])


def import_images(s, srcs, width, height, crop=None, dst=None):
    return np.stack([import_image(s, x, width, height, crop, dst) for x in srcs])


def peak_code(peak, full_range):
    """The smallest Y10 whose PQ code is at or above that of `peak` nits."""
    pk = float(pq_inverse(peak))
    return int(np.ceil(pk * 1020)) if full_range else 64 + int(np.ceil(pk * 876))


if __name__ == "__main__":
    for c in K.CODES:
        print(c, [matrix_coefs(c, fr)[0] for fr in (0, 1)])
    for p in (9, 1):
        print(p, gamut_coefs(p), [[float(v) for v in r] for r in gamut_exact(p)])
