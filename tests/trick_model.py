"""TEST: the NumPy model of efx_trick_pick's selection rule (include/efx.h, espflix_amd/csrc/trick_sel.h), written from the
definition: picture t of a title is picked iff t mod speed == 0 and is pick k = t // speed; a call offers the pictures
first .. first + n - 1; fwd placement is call-relative (image k - k0), rwd placement title-absolute (image K - 1 - k)."""
import numpy as np

FRAME_BYTES = 101376


def total_picks(total: int, speed: int) -> int:
    return len([t for t in range(total) if t % speed == 0])


def count(first: int, n: int, speed: int) -> int:
    return len([t for t in range(first, first + n) if t % speed == 0])


def placements(first: int, n: int, speed: int, total: int):
    """[(picture of the call, fwd image of the call, rwd image of the title)] of a call, in playing order."""
    K = total_picks(total, speed)
    k0 = len([t for t in range(first) if t % speed == 0])  # picks in front of the call
    out = []
    for j in range(n):
        t = first + j
        if t % speed == 0:
            k = t // speed
            out.append((j, k - k0, K - 1 - k))
    return out


def pick(src: np.ndarray, first: int, speed: int, total: int, fwd: np.ndarray | None, rwd: np.ndarray | None) -> int:
    """One call on arrays: src (n_streams, n, ...) pictures, fwd (n_streams, >= picks, ...), rwd (n_streams, >= K, ...);
    only the picked images are written.  Returns the call's picks."""
    pl = placements(first, src.shape[1], speed, total)
    for j, f, r in pl:
        if fwd is not None:
            fwd[:, f] = src[:, j]
        if rwd is not None:
            rwd[:, r] = src[:, j]
    return len(pl)


def splits(total: int, parts: int):
    """Every way to cut a title of `total` pictures into `parts` calls of at least one picture: lists of (first, n)."""
    if parts == 1:
        return [[(0, total)]]
    out = []
    if parts == 2:
        for a in range(1, total):
            out.append([(0, a), (a, total - a)])
    elif parts == 3:
        for a in range(1, total):
            for b in range(a + 1, total):
                out.append([(0, a), (a, b - a), (b, total - b)])
    return out
