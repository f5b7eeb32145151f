"""NumPy model of efx_deinterlace, written from the text of include/efx.h ("interlaced sources") alone: the rule for a
missing sample on whole planes, the index rule, the outputs of a call and its pieces.  The canonical image of a surface is
surface_model.py's.  It shares no code with espflix_amd/csrc/deint_px.h."""
import numpy as np

import surface_model as S

TOP, BOTTOM = 0, 1
FRAME, FIELD = 0, 1


def count(n_frames, lead, tail, mode):
    """efx_deinterlace_count: outputs per stream, -1 for rejected arguments."""
    if n_frames < 1 or lead not in (0, 1) or tail not in (0, 1) or lead + tail >= n_frames or mode not in (FRAME, FIELD):
        return -1
    n = (n_frames - lead - tail) * (2 if mode == FIELD else 1)
    return n if n < (1 << 31) else -1


def accepts(s):
    """True for a surface efx_deinterlace reads."""
    return S.check(s) and s.layout in (S.PLANAR8, S.SEMI8) and s.height >= 8 and s.height % 4 == 0


def planes(img, w, h):
    """The three planes of a packed I420 picture as int64 arrays."""
    img = np.asarray(img).reshape(-1)
    y, c = w * h, (w // 2) * (h // 2)
    return [img[:y].reshape(h, w).astype(np.int64), img[y:y + c].reshape(h // 2, w // 2).astype(np.int64),
            img[y + c:y + 2 * c].reshape(h // 2, w // 2).astype(np.int64)]


def _rows(h, ys, off):
    """The index rule for rows ys + off."""
    r = ys + off
    return np.where(r < 0, r + 2, np.where(r >= h, r - 2, r))


def _cols(w, off):
    return np.clip(np.arange(w) + off, 0, w - 1)


def complete_plane(cur, prev, nxt, B, A, p):
    """One plane of an output: the lines of parity p kept, the others made by the rule."""
    h, w = cur.shape
    out = cur.copy()
    ys = np.arange(1 - p, h, 2)
    up, dn = cur[_rows(h, ys, -1)], cur[_rows(h, ys, 1)]
    c, e = up, dn
    b0, a0 = B[ys], A[ys]
    d = (b0 + a0) >> 1
    t0 = np.abs(b0 - a0) >> 1
    t1 = (np.abs(prev[_rows(h, ys, -1)] - c) + np.abs(prev[_rows(h, ys, 1)] - e)) >> 1
    t2 = (np.abs(nxt[_rows(h, ys, -1)] - c) + np.abs(nxt[_rows(h, ys, 1)] - e)) >> 1
    diff = np.maximum(np.maximum(t0, t1), t2)

    def score(j):
        return sum(np.abs(up[:, _cols(w, k + j)] - dn[:, _cols(w, k - j)]) for k in (-1, 0, 1))

    def pred(j):
        return (up[:, _cols(w, j)] + dn[:, _cols(w, -j)]) >> 1

    best, sp = score(0) - 1, pred(0)
    for s in (-1, 1):
        s1 = score(s)
        first = s1 < best
        best, sp = np.where(first, s1, best), np.where(first, pred(s), sp)
        s2 = score(2 * s)
        second = first & (s2 < best)
        best, sp = np.where(second, s2, best), np.where(second, pred(2 * s), sp)
    b = (B[_rows(h, ys, -2)] + A[_rows(h, ys, -2)]) >> 1
    f = (B[_rows(h, ys, 2)] + A[_rows(h, ys, 2)]) >> 1
    mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, f - e))
    mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, f - e))
    diff = np.maximum(np.maximum(diff, mn), -mx)
    res = np.minimum(np.maximum(sp, d - diff), d + diff)
    assert res.min() >= 0 and res.max() <= 255
    out[ys] = res
    return out


def complete(frames, t, i, first_field, w, h):
    """Output (t, i) of a stream of packed I420 frames (N, w * h * 3 / 2): a packed I420 picture."""
    N = len(frames)
    cur = planes(frames[t], w, h)
    prev = planes(frames[t - 1] if t - 1 >= 0 else frames[t], w, h)
    nxt = planes(frames[t + 1] if t + 1 < N else frames[t], w, h)
    B, A = (prev, cur) if i == 0 else (cur, nxt)
    p = i if first_field == TOP else 1 - i
    return np.concatenate([complete_plane(cur[k], prev[k], nxt[k], B[k], A[k], p).reshape(-1) for k in range(3)]).astype(np.uint8)


def deinterlace_i420(frames, w, h, first_field=TOP, mode=FIELD, lead=0, tail=0):
    """One stream of packed I420 frames (n_frames, w * h * 3 / 2) through one call: (n_out, w * h * 3 / 2) uint8."""
    n = len(frames)
    assert count(n, lead, tail, mode) >= 0
    out = [complete(frames, t, i, first_field, w, h) for t in range(lead, n - tail) for i in range(2 if mode == FIELD else 1)]
    return np.stack(out)


def deinterlace(srcs, s, n_streams, first_field=TOP, mode=FIELD, lead=0, tail=0):
    """What a call writes for source images srcs (n_streams * n_frames, bytes) of surface s: (n_streams, n_out, w h 3 / 2)."""
    assert accepts(s) and len(srcs) % n_streams == 0
    n_frames = len(srcs) // n_streams
    can = S.canonicals(srcs, s).reshape(n_streams, n_frames, -1)
    return np.stack([deinterlace_i420(can[k], s.width, s.height, first_field, mode, lead, tail) for k in range(n_streams)])
