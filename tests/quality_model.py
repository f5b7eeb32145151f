"""NumPy model of efx_compare_pictures (the definition: include/efx.h, "picture quality"): per image and plane the sum of
squared errors and the sum of the Q16 SSIM of the 8 x 8 windows on the 4-pel grid, and the luma SSE of every macroblock.
It shares no code with espflix_amd/csrc/quality_px.h: sums are made with NumPy on whole planes, and num, den and the
quotient of every window are Python integers, so nothing here can overflow or round."""
import functools
import math

import numpy as np

W, H = 352, 192
PIC = 101376
PLANES = ((0, H, W), (W * H, H // 2, W // 2), (W * H + W * H // 4, H // 2, W // 2))   # (offset, rows, columns) of Y, Cb, Cr
C1, C2 = 416, 235963
WINDOWS = (87 * 47, 43 * 23, 43 * 23)
SAMPLES = (W * H, W * H // 4, W * H // 4)


def planes(image):
    """The three planes of one 101376-byte image as int64 arrays."""
    image = np.asarray(image, dtype=np.uint8).reshape(PIC)
    return [image[o:o + r * c].reshape(r, c).astype(np.int64) for o, r, c in PLANES]


def block_sums(a, b):
    """s1, s2, ss, s12 of every 4 x 4 block of a plane pair (int64 arrays of the block grid's shape)."""
    r, c = a.shape
    tile = lambda v: v.reshape(r // 4, 4, c // 4, 4).sum(axis=(1, 3))
    return tile(a), tile(b), tile(a * a + b * b), tile(a * b)


def window_sums(a, b):
    """S1, S2, SS, S12 of every window: the sums of 2 x 2 adjacent blocks."""
    quad = lambda v: v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:]
    return tuple(quad(v) for v in block_sums(a, b))


def num_den(S1, S2, SS, S12):
    """Python integers in, Python integers out."""
    vars_ = 64 * SS - S1 * S1 - S2 * S2
    covar = 64 * S12 - S1 * S2
    return (2 * S1 * S2 + C1) * (2 * covar + C2), (S1 * S1 + S2 * S2 + C1) * (vars_ + C2)


def quotient(num: int, den: int) -> int:
    """sign(num) floor(|num| 65536 / den): Q16, truncated toward zero."""
    q = (abs(num) << 16) // den
    return -q if num < 0 else q


@functools.lru_cache(maxsize=1 << 20)
def window_q(S1: int, S2: int, SS: int, S12: int) -> int:
    return quotient(*num_den(S1, S2, SS, S12))


def plane_q(a, b):
    """The Q16 SSIM of every window of a plane pair, as a list of lists of Python integers."""
    S1, S2, SS, S12 = (v.tolist() for v in window_sums(a, b))
    return [[window_q(*t) for t in zip(*rows)] for rows in zip(S1, S2, SS, S12)]


def plane_ssim_float(a, b) -> float:
    """The mean over the windows of num / den, evaluated in float64 from the exact integers."""
    S1, S2, SS, S12 = (v.reshape(-1).tolist() for v in window_sums(a, b))
    vals = []
    for t in zip(S1, S2, SS, S12):
        n, d = num_den(*t)
        vals.append(n / d)
    return math.fsum(vals) / len(vals)


def compare(ref, test, ref_max=0):
    """One image pair: (sse[3], ssim[3], mb_sse[264]) as Python integers / a uint32 array."""
    m = ref_max or 255
    sse, ssim = [], []
    mb = None
    for p, (a, b) in enumerate(zip(planes(ref), planes(test))):
        a = np.minimum(a, m)
        d2 = (a - b) ** 2
        sse.append(int(d2.sum()))
        ssim.append(sum(sum(row) for row in plane_q(a, b)))
        if p == 0:
            mb = d2.reshape(12, 16, 22, 16).sum(axis=(1, 3)).reshape(264).astype(np.uint32)
    return sse, ssim, mb


def compare_batch(ref, test, ref_max=0):
    """(n, 101376) pairs: sse (n, 3) uint64, ssim (n, 3) int64, mb_sse (n, 264) uint32."""
    ref = np.asarray(ref, dtype=np.uint8).reshape(-1, PIC)
    test = np.asarray(test, dtype=np.uint8).reshape(-1, PIC)
    out = [compare(r, t, ref_max) for r, t in zip(ref, test)]
    return (np.array([o[0] for o in out], dtype=np.uint64).reshape(-1, 3), np.array([o[1] for o in out], dtype=np.int64).reshape(-1, 3),
            np.stack([o[2] for o in out]))


def psnr(sse: int, samples: int) -> float:
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * samples / sse)


def mean_ssim(total: int, plane: int) -> float:
    return total / (65536.0 * WINDOWS[plane])


def image_of(y, cb=None, cr=None):
    """A 101376-byte image from a luma plane (192, 352) and chroma planes (96, 176); missing chroma is 128."""
    cb = np.full((H // 2, W // 2), 128, np.uint8) if cb is None else cb
    cr = np.full((H // 2, W // 2), 128, np.uint8) if cr is None else cr
    return np.concatenate([np.asarray(v, dtype=np.uint8).reshape(-1) for v in (y, cb, cr)])
