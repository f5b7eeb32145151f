"""NumPy model of efx_import_frames (include/efx.h, "pictures in"): the RGB -> YCbCr matrix, the widened-triangle taps
of one axis as a dense coefficient matrix, the two passes with their rounding steps, the border and the letterbox
rectangle.  Everything is integer arithmetic on the source bytes; the matrix products run in float64, where every partial
sum is an integer below 2^53 and therefore exact."""
import numpy as np

W, H = 352, 192
CW, CH = W // 2, H // 2
Y_BYTES, C_BYTES = W * H, CW * CH
FRAME_BYTES = Y_BYTES + 2 * C_BYTES
ONE = 16384
MAX_RATIO = 32
MAX_TAPS = 130  # (RGB chroma: the full crop to half the rectangle, a ratio of up to 64)

STUDIO = dict(y=(66, 129, 25), y0=16, cb=(-38, -74, 112), cr=(112, -94, -18))
FULL = dict(y=(77, 150, 29), y0=0, cb=(-43, -85, 128), cr=(128, -107, -21))


def src_bytes(fmt, width, height):
    """efx_import_src_bytes: 0 for arguments efx_import_frames rejects."""
    if not (2 <= width <= 4096 and 2 <= height <= 4096):
        return 0
    if fmt == "i420":
        return 0 if (width | height) & 1 else width * height * 3 // 2
    return width * height * 3 if fmt in ("rgb24", "rgbp") else 0


def rgb_to_ycbcr(r, g, b, full_range=False):
    """Integer arrays in, (Y, Cb, Cr) int arrays out (numpy's >> on signed integers is arithmetic)."""
    m = FULL if full_range else STUDIO
    r, g, b = (np.asarray(c).astype(np.int32) for c in (r, g, b))
    y = ((m["y"][0] * r + m["y"][1] * g + m["y"][2] * b + 128) >> 8) + m["y0"]
    cb = ((m["cb"][0] * r + m["cb"][1] * g + m["cb"][2] * b + 128) >> 8) + 128
    cr = ((m["cr"][0] * r + m["cr"][1] * g + m["cr"][2] * b + 128) >> 8) + 128
    return tuple(np.clip(c, 0, 255) for c in (y, cb, cr))


def raw_weights(S, D):
    """u[d, s] = max(0, 2M - |(2s + 1) D - (2d + 1) S|), M = max(S, D)."""
    s = np.arange(S, dtype=np.int64)[None, :]
    d = np.arange(D, dtype=np.int64)[:, None]
    return np.maximum(0, 2 * max(S, D) - np.abs((2 * s + 1) * D - (2 * d + 1) * S))


def tap_matrix(S, D):
    """(D, S) int64 coefficients: row d holds the window of destination index d, zero elsewhere; every row sums to 16384."""
    u = raw_weights(S, D)
    k = u * ONE // u.sum(axis=1, keepdims=True)
    k[np.arange(D), u.argmax(axis=1)] += ONE - k.sum(axis=1)  # (argmax: the first of equal maxima)
    return k


def windows(S, D):
    """Per destination index: first source index, tap count, and the coefficients padded with zeros to MAX_TAPS."""
    k, u = tap_matrix(S, D), raw_weights(S, D)
    start = (u > 0).argmax(axis=1)
    count = (u > 0).sum(axis=1)
    coef = np.zeros((D, MAX_TAPS), dtype=np.int64)
    for d in range(D):
        coef[d, :count[d]] = k[d, start[d]:start[d] + count[d]]
    return start, count, coef


def resample(plane, dw, dh):
    """A byte plane (h, w) -> (dh, dw) int64: horizontal pass, 16-bit rounding, vertical pass."""
    h, w = plane.shape
    kx, ky = tap_matrix(w, dw), tap_matrix(h, dh)
    hs = plane.astype(np.float64) @ kx.T.astype(np.float64)
    hs = (hs.astype(np.int64) + 32) >> 6
    vs = ky.astype(np.float64) @ hs.astype(np.float64)
    return (vs.astype(np.int64) + (1 << 21)) >> 22


def letterbox_rect(w, h):
    """fit="letterbox": the largest rectangle of the aspect ratio w : h with even sides inside 352 x 192 (the long side
    fills the frame, the other is floor(...) rounded down to even, at least 16), centred on even coordinates."""
    if w * H >= h * W:
        dw, dh = W, max(16, (W * h // w) & ~1)
    else:
        dw, dh = max(16, (H * w // h) & ~1), H
    return ((W - dw) // 2) & ~1, ((H - dh) // 2) & ~1, dw, dh


def source_planes(src, fmt, width, height, crop, full_range):
    cx, cy, cw, ch = crop
    if fmt == "i420":
        flat = np.asarray(src, dtype=np.uint8).reshape(-1)
        y = flat[:width * height].reshape(height, width)
        u = flat[width * height:width * height * 5 // 4].reshape(height // 2, width // 2)
        v = flat[width * height * 5 // 4:width * height * 3 // 2].reshape(height // 2, width // 2)
        c = (slice(cy // 2, (cy + ch) // 2), slice(cx // 2, (cx + cw) // 2))
        return y[cy:cy + ch, cx:cx + cw], u[c], v[c]
    a = np.asarray(src, dtype=np.uint8)
    if fmt == "rgb24":
        a = a.reshape(height, width, 3)
        r, g, b = a[..., 0], a[..., 1], a[..., 2]
    else:
        a = a.reshape(3, height, width)
        r, g, b = a[0], a[1], a[2]
    win = (slice(cy, cy + ch), slice(cx, cx + cw))
    return rgb_to_ycbcr(r[win], g[win], b[win], full_range)


def import_image(src, fmt, width, height, crop=None, dst=None, full_range=False):
    """One source picture -> the 101376 bytes efx_import_frames writes for it."""
    crop = crop or (0, 0, width, height)
    dx, dy, dw, dh = dst or (0, 0, W, H)
    y, u, v = source_planes(src, fmt, width, height, crop, full_range)
    out_y = np.full((H, W), 0 if (full_range and fmt != "i420") else 16, dtype=np.uint8)
    out_u = np.full((CH, CW), 128, dtype=np.uint8)
    out_v = np.full((CH, CW), 128, dtype=np.uint8)
    out_y[dy:dy + dh, dx:dx + dw] = resample(y, dw, dh)
    out_u[dy // 2:(dy + dh) // 2, dx // 2:(dx + dw) // 2] = resample(u, dw // 2, dh // 2)
    out_v[dy // 2:(dy + dh) // 2, dx // 2:(dx + dw) // 2] = resample(v, dw // 2, dh // 2)
    return np.concatenate([out_y.reshape(-1), out_u.reshape(-1), out_v.reshape(-1)])


def import_images(srcs, fmt, width, height, crop=None, dst=None, full_range=False):
    return np.stack([import_image(s, fmt, width, height, crop, dst, full_range) for s in srcs])
