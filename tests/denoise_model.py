"""NumPy model of efx_denoise, written from the text of include/efx.h ("noisy sources") alone: the thresholded 3 x 3
binomial filter, the recursive temporal blend, the three planes of the canonical image of a surface, streams and pieces.
The canonical image is surface_model.py's.  It shares no code with espflix_amd/csrc/denoise_px.h."""
import numpy as np

import surface_model as S

MAX_THRESHOLD = 64
K = ((1, 2, 1), (2, 4, 2), (1, 2, 1))


def accepts(s):
    """True for a surface efx_denoise reads: a byte layout that efx_import_surfaces accepts."""
    return S.check(s) and s.layout in (S.PLANAR8, S.SEMI8)


def spatial(plane, ts):
    """The spatial step on one plane (h, w) uint8 -> int64."""
    F = np.asarray(plane).astype(np.int64)
    h, w = F.shape
    pad = np.pad(F, 1, mode="edge")  # indices clamped to the plane
    acc = np.zeros_like(F)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            v = pad[1 + i:1 + i + h, 1 + j:1 + j + w]
            acc += K[i + 1][j + 1] * np.where(np.abs(v - F) <= ts, v, F)
    return (acc + 8) >> 4


def blend_k(a, tt):
    """k of the temporal step for |d| = a (array) and Tt >= 1."""
    q = 12582912 // (tt * tt)
    return np.where(a >= tt, 256, 64 + ((a * a * q) >> 16))


def temporal(s, prev, tt):
    """The temporal step: s int64 (h, w), prev the previous output (or None: the stream's first picture)."""
    if prev is None or tt == 0:
        return s
    P = np.asarray(prev).astype(np.int64)
    d = s - P
    a = np.abs(d)
    return P + np.sign(d) * ((a * blend_k(a, tt) + 128) >> 8)


def denoise_plane(frames, ts, tt, prev=None):
    """frames (n, h, w) uint8 of one stream's plane, prev (h, w) or None -> (n, h, w) uint8."""
    out = np.empty_like(frames)
    for t in range(len(frames)):
        o = temporal(spatial(frames[t], ts), prev, tt)
        assert o.min() >= 0 and o.max() <= 255
        prev = out[t] = o.astype(np.uint8)
    return out


def planes_of(pics, w, h):
    """(n, w * h * 3 / 2) packed I420 -> [(n, h, w), (n, h/2, w/2), (n, h/2, w/2)]."""
    n = len(pics)
    y, c = w * h, (w // 2) * (h // 2)
    return [pics[:, :y].reshape(n, h, w), pics[:, y:y + c].reshape(n, h // 2, w // 2), pics[:, y + c:y + 2 * c].reshape(n, h // 2, w // 2)]


def denoise_i420(pics, w, h, n_streams=1, luma_spatial=0, chroma_spatial=0, luma_temporal=0, chroma_temporal=0, prev=None):
    """pics (n_streams * n_frames, w * h * 3 / 2) packed I420, stream by stream; prev (n_streams, w * h * 3 / 2) or None.
    Returns the outputs in the same shape."""
    pics = np.asarray(pics, dtype=np.uint8)
    total = len(pics)
    assert n_streams >= 1 and total % n_streams == 0 and total // n_streams >= 1
    for t in (luma_spatial, chroma_spatial, luma_temporal, chroma_temporal):
        assert 0 <= t <= MAX_THRESHOLD
    n = total // n_streams
    out = np.empty_like(pics)
    prevs = planes_of(np.asarray(prev, dtype=np.uint8).reshape(n_streams, -1), w, h) if prev is not None else None
    for p, plane in enumerate(planes_of(pics, w, h)):
        ts, tt = (luma_spatial, luma_temporal) if p == 0 else (chroma_spatial, chroma_temporal)
        for i in range(n_streams):
            res = denoise_plane(plane[i * n:(i + 1) * n], ts, tt, prevs[p][i] if prevs is not None else None)
            lo = 0 if p == 0 else w * h + (p - 1) * (w // 2) * (h // 2)
            out[i * n:(i + 1) * n, lo:lo + res[0].size] = res.reshape(n, -1)
    return out


def denoise(srcs, s, n_streams=1, prev=None, **thresholds):
    """What efx_denoise writes for the source images srcs (n_streams * n_frames, s.bytes) of surface s."""
    assert accepts(s)
    return denoise_i420(S.canonicals(srcs, s), s.width, s.height, n_streams, prev=prev, **thresholds)


def thresholds(sigma):
    """denoise_thresholds: (2 sigma, 2 sigma, 4 sigma, 4 sigma), rounded and clamped to 64."""
    clamp = lambda v: int(min(MAX_THRESHOLD, max(0, np.floor(v + 0.5))))
    return clamp(2 * sigma), clamp(2 * sigma), clamp(4 * sigma), clamp(4 * sigma)
