"""NumPy model of efx_detelecine, written from the text of include/efx.h ("telecined sources") alone: the comb score, the
match, the cycles of five, the records and the woven outputs of a call and its pieces.  The canonical image of a surface
is surface_model.py's.  It shares no code with espflix_amd/csrc/telecine_px.h."""
import numpy as np

import surface_model as S

TOP, BOTTOM = 0, 1
NO_DIFF = (1 << 64) - 1
INFO = np.dtype([("comb_c", "<u8"), ("comb_p", "<u8"), ("diff", "<u8"), ("match", "<i4"), ("out", "<i4")])
assert INFO.itemsize == 32


def count(n_frames, lead):
    """efx_detelecine_count: outputs per stream, -1 for rejected arguments."""
    if n_frames < 1 or lead not in (0, 1) or lead >= n_frames:
        return -1
    n = n_frames - lead
    return n - n // 5


def accepts(s):
    """True for a surface efx_detelecine reads."""
    return S.check(s) and s.layout in (S.PLANAR8, S.SEMI8) and s.height >= 8 and s.height % 4 == 0


def planes(img, w, h):
    """The three planes of a packed I420 picture as int64 arrays."""
    img = np.asarray(img).reshape(-1)
    y, c = w * h, (w // 2) * (h // 2)
    return [img[:y].reshape(h, w).astype(np.int64), img[y:y + c].reshape(h // 2, w // 2).astype(np.int64),
            img[y + c:y + 2 * c].reshape(h // 2, w // 2).astype(np.int64)]


def score(W, nt):
    """The comb score of a woven luma plane (Python int)."""
    W = np.asarray(W).astype(np.int64)
    v = np.abs(W[:-4] + 4 * W[2:-2] + W[4:] - 3 * (W[1:-3] + W[3:-1]))
    return int(np.maximum(0, v - 6 * nt).sum())


def weave_plane(e_from, l_from, p):
    """The lines of parity p of e_from, the others of l_from."""
    out = np.array(l_from, copy=True)
    out[p::2] = e_from[p::2]
    return out


def weave(e_img, l_img, w, h, p):
    """weave(E of e_img, L of l_img) of packed I420 pictures: a packed I420 picture (uint8)."""
    return np.concatenate([weave_plane(a, b, p).reshape(-1) for a, b in zip(planes(e_img, w, h), planes(l_img, w, h))]).astype(np.uint8)


def detelecine_i420(frames, w, h, first_field=TOP, lead=0, nt=10):
    """One stream of packed I420 frames (n_frames, w * h * 3 / 2) through one call: (outputs (n_out, w * h * 3 / 2) uint8,
    records (n,) INFO)."""
    n_frames = len(frames)
    assert count(n_frames, lead) >= 0 and 0 <= nt <= 255
    p = first_field
    n = n_frames - lead
    info = np.zeros(n, dtype=INFO)
    for j in range(n):
        t = lead + j
        cur = planes(frames[t], w, h)[0]
        cc = score(cur, nt)
        if t == 0:
            cp, d = 0, NO_DIFF
        else:
            prev = planes(frames[t - 1], w, h)[0]
            cp = score(weave_plane(cur, prev, p), nt)
            d = int(np.abs(cur[p::2] - prev[p::2]).sum())
        info[j] = (cc, cp, d, 1 if t > 0 and 4 * cp < 3 * cc else 0, 0)
    keep = np.ones(n, dtype=bool)
    for c0 in range(0, n - n % 5, 5):
        ds = [int(info["diff"][c0 + k]) for k in range(5)]
        keep[c0 + ds.index(min(ds))] = False
    outs, m = [], 0
    for j in range(n):
        if not keep[j]:
            info["out"][j] = -1
            continue
        info["out"][j] = m
        m += 1
        t = lead + j
        outs.append(weave(frames[t], frames[t - int(info["match"][j])], w, h, p))
    assert m == count(n_frames, lead)
    return np.stack(outs), info


def detelecine(srcs, s, n_streams, first_field=TOP, lead=0, nt=10):
    """What a call writes for source images srcs (n_streams * n_frames, bytes) of surface s: (outputs (n_streams, n_out,
    w h 3 / 2), records (n_streams, n) INFO)."""
    assert accepts(s) and len(srcs) % n_streams == 0
    n_frames = len(srcs) // n_streams
    can = S.canonicals(srcs, s).reshape(n_streams, n_frames, -1)
    res = [detelecine_i420(can[k], s.width, s.height, first_field, lead, nt) for k in range(n_streams)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- synthetic pulldown ------------------------------------------------------------------------------------------------------
def telecine(film, w, h, p, phase, start):
    """Hard 2-3 pulldown of packed I420 film frames: film frame k fills 2 (k even) or 3 (k odd) consecutive field slots, of
    which the first `phase` are cut off; slot s of the rest belongs to video frame s // 2, the earlier slot of a frame
    being its field of parity p.  Then the first `start` video frames are cut off.  Returns (video frames, for each the
    film frame of its earlier field)."""
    slots = []
    for k in range(len(film)):
        slots += [k] * (3 if k & 1 else 2)
    slots = slots[phase:]
    video, early = [], []
    for f in range(len(slots) // 2):
        a, b = slots[2 * f], slots[2 * f + 1]
        video.append(weave(film[a], film[b], w, h, p))
        early.append(a)
    return np.stack(video[start:]), early[start:]
