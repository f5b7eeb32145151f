"""NumPy model of efx_detect_crop (include/efx.h, "black borders"): the luma of a source picture, its row and column sums,
the picture / black classification, the union over a stream's contributing images, the rounding of an axis, the record,
and cover_crop.  It shares no code with espflix_amd/csrc/crop_px.h."""
import numpy as np

FRAME_W, FRAME_H = 352, 192
Y_STUDIO = (66, 129, 25, 16)
Y_FULL = (77, 150, 29, 0)


def rgb_luma(r, g, b, full_range=False):
    """Y of the BT.601 matrix of efx_import_frames, clamped to a byte."""
    kr, kg, kb, y0 = Y_FULL if full_range else Y_STUDIO
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    return np.clip(((kr * r + kg * g + kb * b + 128) >> 8) + y0, 0, 255)


def luma(src, fmt, width, height, full_range=False):
    """(height, width) int64 luma plane of one source image given as flat bytes (or any array of its size)."""
    flat = np.asarray(src, dtype=np.uint8).reshape(-1)
    if fmt == "i420":
        return flat[:width * height].reshape(height, width).astype(np.int64)
    if fmt == "rgb24":
        a = flat[:width * height * 3].reshape(height, width, 3)
        return rgb_luma(a[..., 0], a[..., 1], a[..., 2], full_range)
    if fmt == "rgbp":
        a = flat[:width * height * 3].reshape(3, height, width)
        return rgb_luma(a[0], a[1], a[2], full_range)
    raise ValueError(fmt)


def sums(src, fmt, width, height, full_range=False):
    """uint32 array R[0 .. height) followed by C[0 .. width)."""
    l = luma(src, fmt, width, height, full_range)
    return np.concatenate([l.sum(axis=1), l.sum(axis=0)]).astype(np.uint32)


def classify(s, width, height, limit):
    """(picture rows, picture columns) as boolean arrays."""
    s = np.asarray(s).astype(np.int64)
    return s[:height] > limit * width, s[height:height + width] > limit * height


def image_bounds(s, width, height, limit):
    """(left, top, right, bottom) of a contributing image, None otherwise."""
    rows, cols = classify(s, width, height, limit)
    if not rows.any() or not cols.any():
        return None
    ys, xs = np.flatnonzero(rows), np.flatnonzero(cols)
    return int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])


def round_axis(a, b, r):
    """(pos, len) of bounds a .. b inclusive, or None when the axis fails."""
    a1 = a + (a & 1)
    avail = b + 1 - a1
    if avail < 2:
        return None
    length = avail - avail % r if avail >= r else avail & ~1
    return a1 + (((avail - length) >> 1) & ~1), length


def record(all_sums, width, height, limit, rnd):
    """The eight int32 of one stream from the sums of its images."""
    x1, y1, x2, y2 = width, height, -1, -1
    for s in all_sums:
        b = image_bounds(s, width, height, limit)
        if b is not None:
            x1, y1, x2, y2 = min(x1, b[0]), min(y1, b[1]), max(x2, b[2]), max(y2, b[3])
    rect = (0, 0, width, height)
    if x2 >= 0:
        ax, ay = round_axis(x1, x2, rnd), round_axis(y1, y2, rnd)
        if ax is not None and ay is not None:
            rect = (ax[0], ay[0], ax[1], ay[1])
    return np.array([*rect, x1, y1, x2, y2], dtype=np.int32)


def detect(srcs, fmt, width, height, images_per_stream=None, limit=24, rnd=16, full_range=False):
    """srcs: (n, bytes) -> (sums (n, height + width) uint32, records (n_streams, 8) int32)."""
    n = len(srcs)
    per = n if images_per_stream is None else images_per_stream
    assert n % per == 0
    all_sums = np.stack([sums(s, fmt, width, height, full_range) for s in srcs])
    recs = np.stack([record(all_sums[i:i + per], width, height, limit, rnd) for i in range(0, n, per)])
    return all_sums, recs


def cover_crop(width, height, region=None):
    """The largest centred rectangle with even sides and the frame's 11 : 6 shape inside region (x, y, w, h)."""
    x, y, w, h = region or (0, 0, width, height)
    if w * FRAME_H >= h * FRAME_W:
        w2, h2 = (h * FRAME_W // FRAME_H) & ~1, h
    else:
        w2, h2 = w, (w * FRAME_H // FRAME_W) & ~1
    return x + (((w - w2) >> 1) & ~1), y + (((h - h2) >> 1) & ~1), w2, h2
