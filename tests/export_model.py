"""NumPy model of efx_export_frames (include/efx.h): the strip layout's planes, chroma upsampling and the BT.601 matrix.

A helper module of the export tests (not a test itself).  Everything is integer arithmetic on the frame bytes, written
straight from the formulas in efx.h -- independent of espflix_amd/csrc/export_px.h, which the tests check against it."""
import numpy as np

W, H = 352, 192
CW, CH = W // 2, H // 2
FRAME_BYTES = 101376
Y_BYTES, C_BYTES = W * H, CW * CH
RGB_BYTES = 3 * W * H

# (cy, y0, rv, gu, gv, bu)
STUDIO = (298, 16, 409, -100, -208, 516)
FULL = (256, 0, 359, -88, -183, 454)


def planes(frames):
    """Strip-layout frames (..., 101376) -> Y (..., 192, 352), U = Cb (..., 96, 176), V = Cr (..., 96, 176).
    Strip rows 0-7 hold Cb, rows 8-15 Cr (whatever the reference calls them)."""
    f = np.asarray(frames, dtype=np.uint8)
    lead = f.shape[:-1]
    s = f.reshape(lead + (12, 16, 528))
    y = s[..., :W].reshape(lead + (H, W))
    u = s[..., :8, W:].reshape(lead + (CH, CW))
    v = s[..., 8:, W:].reshape(lead + (CH, CW))
    return y, u, v


def strip_to_i420(frames):
    y, u, v = planes(frames)
    lead = y.shape[:-2]
    return np.concatenate([y.reshape(lead + (-1,)), u.reshape(lead + (-1,)), v.reshape(lead + (-1,))], axis=-1)


def i420_to_strip(i420):
    """The inverse of strip_to_i420 (vectorised over leading axes)."""
    a = np.asarray(i420, dtype=np.uint8)
    lead = a.shape[:-1]
    y = a[..., :Y_BYTES].reshape(lead + (12, 16, W))
    u = a[..., Y_BYTES:Y_BYTES + C_BYTES].reshape(lead + (12, 8, CW))
    v = a[..., Y_BYTES + C_BYTES:].reshape(lead + (12, 8, CW))
    out = np.empty(lead + (12, 16, 528), dtype=np.uint8)
    out[..., :W] = y
    out[..., :8, W:] = u
    out[..., 8:, W:] = v
    return out.reshape(lead + (FRAME_BYTES,))


def near_index(n_luma):
    """For every luma coordinate: (chroma coordinate x >> 1, its neighbour on the side x lies on, clamped)."""
    x = np.arange(n_luma)
    c0 = x >> 1
    c1 = np.clip(c0 + np.where(x & 1, 1, -1), 0, n_luma // 2 - 1)
    return c0, c1


def upsample(c, chroma):
    """Chroma plane(s) (..., 96, 176) -> luma resolution (..., 192, 352), int32."""
    c = np.asarray(c).astype(np.int32)
    cx0, cx1 = near_index(W)
    cy0, cy1 = near_index(H)
    if chroma == "nearest":
        return c[..., cy0, :][..., cx0]
    r0, r1 = c[..., cy0, :], c[..., cy1, :]
    return (9 * r0[..., cx0] + 3 * r0[..., cx1] + 3 * r1[..., cx0] + r1[..., cx1] + 8) >> 4


def bilinear4(c00, c01, c10, c11):
    return (9 * np.asarray(c00, np.int32) + 3 * np.asarray(c01, np.int32) + 3 * np.asarray(c10, np.int32)
            + np.asarray(c11, np.int32) + 8) >> 4


def ycbcr_to_rgb(y, u, v, full_range=False):
    """Integer BT.601 matrix; returns (..., 3) uint8 (R, G, B)."""
    cy, y0, rv, gu, gv, bu = FULL if full_range else STUDIO
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    t = cy * (y - y0) + 128
    u = u - 128
    v = v - 128
    r = np.clip((t + rv * v) >> 8, 0, 255)
    g = np.clip((t + gu * u + gv * v) >> 8, 0, 255)
    b = np.clip((t + bu * u) >> 8, 0, 255)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def export(frames, fmt, chroma="bilinear", full_range=False):
    """What efx_export_frames writes for strip-layout frames (..., 101376): "i420" (..., 101376), "rgb24"
    (..., 192, 352, 3), "rgbp" (..., 3, 192, 352)."""
    if fmt == "i420":
        return strip_to_i420(frames)
    y, u, v = planes(frames)
    rgb = ycbcr_to_rgb(y, upsample(u, chroma), upsample(v, chroma), full_range)
    if fmt == "rgb24":
        return rgb
    assert fmt == "rgbp"
    return np.ascontiguousarray(np.moveaxis(rgb, -1, -3))
