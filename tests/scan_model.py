"""NumPy model of efx_detect_scan and efx_scan_verdict, written from the text of include/efx.h ("scan type") alone: the five
sums of a frame, its label and repeat, the counts of a stream over a call and its pieces, and the verdict of a record.
The comb score is telecine_model.py's and the canonical image of a surface is surface_model.py's.  It shares no code with
espflix_amd/csrc/scan_px.h."""
import numpy as np

import surface_model as S
from telecine_model import score

TOP, BOTTOM = 0, 1
NONE, STILL, PROGRESSIVE, TFF, BFF, UNDETERMINED = range(6)
REPEAT_NONE, REPEAT_TOP, REPEAT_BOTTOM = range(3)
IS_UNKNOWN, IS_PROGRESSIVE, IS_INTERLACED, IS_TELECINED = range(4)
FRAME = np.dtype([("comb", "<u8"), ("comb_tb", "<u8"), ("comb_bt", "<u8"), ("diff_top", "<u8"), ("diff_bottom", "<u8"),
                  ("label", "<i4"), ("repeat", "<i4")])
REC = np.dtype([("n_still", "<u4"), ("n_prog", "<u4"), ("n_tff", "<u4"), ("n_bff", "<u4"), ("n_undet", "<u4"),
                ("rep_top", "<u4", 5), ("rep_bottom", "<u4", 5), ("reserved", "<u4")])
assert FRAME.itemsize == 48 and REC.itemsize == 64
DEFAULTS = dict(nt=10, still=64, prog=384, intl=266, rep=768)
RANGES = dict(nt=(0, 255), still=(0, 4080), prog=(256, 65535), intl=(256, 65535), rep=(256, 65535))
COUNTER = {STILL: "n_still", PROGRESSIVE: "n_prog", TFF: "n_tff", BFF: "n_bff", UNDETERMINED: "n_undet"}


def accepts(s):
    """True for a surface efx_detect_scan reads (efx_detelecine's)."""
    return S.check(s) and s.layout in (S.PLANAR8, S.SEMI8) and s.height >= 8 and s.height % 4 == 0


def options_ok(o):
    return all(lo <= o[k] <= hi for k, (lo, hi) in RANGES.items())


def sums(cur, prev, nt):
    """(cc, ctb, cbt, dt, db) of luma plane cur with predecessor prev, as Python ints."""
    cur, prev = np.asarray(cur).astype(np.int64), np.asarray(prev).astype(np.int64)
    tb, bt = prev.copy(), cur.copy()
    tb[0::2] = cur[0::2]   # the even lines of F[t] and the odd lines of F[t-1]
    bt[0::2] = prev[0::2]  # the even lines of F[t-1] and the odd lines of F[t]
    return (score(cur, nt), score(tb, nt), score(bt, nt), int(np.abs(cur[0::2] - prev[0::2]).sum()), int(np.abs(cur[1::2] - prev[1::2]).sum()))


def label(five, w, h, still=64, prog=384, intl=266, rep=768, **_):
    """(label, repeat) of a frame that has a predecessor, from its five sums."""
    cc, ctb, cbt, dt, db = (int(v) for v in five)
    if 16 * (dt + db) < still * w * h:
        return STILL, REPEAT_NONE
    if 256 * min(ctb, cbt) > prog * cc:
        lab = PROGRESSIVE
    elif 256 * cbt > intl * ctb:
        lab = TFF
    elif 256 * ctb > intl * cbt:
        lab = BFF
    else:
        lab = UNDETERMINED
    if rep * dt < 256 * db:
        return lab, REPEAT_TOP
    if rep * db < 256 * dt:
        return lab, REPEAT_BOTTOM
    return lab, REPEAT_NONE


def scan_luma(lumas, lead=0, first_frame=0, rec=None, **opts):
    """One stream of luma planes (n_frames, h, w) through one call: (frame records (n,) FRAME, the stream's record REC).
    rec: the record to add to (accumulate = 1), None to overwrite."""
    o = {**DEFAULTS, **opts}
    assert options_ok(o) and lead in (0, 1) and lead < len(lumas)
    h, w = np.asarray(lumas[0]).shape
    frames = np.zeros(len(lumas) - lead, dtype=FRAME)
    out = np.zeros((), dtype=REC) if rec is None else np.array(rec, dtype=REC, copy=True)
    out["reserved"] = 0
    for j in range(len(frames)):
        t = lead + j
        if t == 0:
            continue  # EFX_SCAN_NONE, sums 0, counted nowhere
        five = sums(lumas[t], lumas[t - 1], o["nt"])
        lab, repeat = label(five, w, h, **o)
        frames[j] = (*five, lab, repeat)
        out[COUNTER[lab]] += 1
        phase = (first_frame + t) % 5
        if repeat == REPEAT_TOP:
            out["rep_top"][phase] += 1
        elif repeat == REPEAT_BOTTOM:
            out["rep_bottom"][phase] += 1
    return frames, out


def scan(srcs, s, n_streams=1, lead=0, first_frame=0, recs=None, **opts):
    """What a call writes for source images srcs (n_streams * n_frames, bytes) of surface s: (frame records (n_streams, n),
    records (n_streams,)).  recs: what recs_device held, for accumulate = 1."""
    assert accepts(s) and len(srcs) % n_streams == 0
    n_frames = len(srcs) // n_streams
    w, h = s.width, s.height
    luma = S.canonicals(srcs, s).reshape(n_streams, n_frames, -1)[:, :, :w * h].reshape(n_streams, n_frames, h, w)
    res = [scan_luma(luma[k], lead, first_frame, None if recs is None else recs[k], **opts) for k in range(n_streams)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def verdict(rec):
    """(kind, first_field) of a record: first_field TOP / BOTTOM, None where the verdict names none."""
    n_prog, n_tff, n_bff, n_undet = (int(rec[k]) for k in ("n_prog", "n_tff", "n_bff", "n_undet"))
    top, bot = [int(v) for v in rec["rep_top"]], [int(v) for v in rec["rep_bottom"]]
    n_moving = n_prog + n_tff + n_bff + n_undet
    pt, pb = top.index(max(top)), bot.index(max(bot))
    m, tot = top[pt] + bot[pb], sum(top) + sum(bot)
    if top[pt] >= 1 and bot[pb] >= 1 and m >= 4 and 4 * m >= 3 * tot and 5 * m >= n_moving and (pb - pt) % 5 in (2, 3):
        return IS_TELECINED, TOP if (pb - pt) % 5 == 2 else BOTTOM
    if n_tff + n_bff > n_prog and 4 * min(n_tff, n_bff) <= max(n_tff, n_bff):
        return IS_INTERLACED, TOP if n_tff > n_bff else BOTTOM
    if n_prog >= 1 and n_prog >= n_tff + n_bff:
        return IS_PROGRESSIVE, None
    return IS_UNKNOWN, None


# ---- synthetic material ----------------------------------------------------------------------------------------------------
def scene(k, w=48, h=32):
    """The luma plane of the scene at field period k: a textured background that pans 3 pels per field period, and a
    bright 12 x 8 block that moves down 2 lines per field period (and starts again at the top)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x = x + 3 * k
    v = 110 + 40 * np.sin(2 * np.pi * x / 13 + 0.7) + 25 * np.cos(2 * np.pi * (x + 3 * y) / 29 + 0.3) + 15 * np.sin(2 * np.pi * (y - x / 2) / 7 + 1.9)
    v = np.rint(v)
    top = (2 * k) % (h - 8)
    v[top:top + 8, 18:30] = 235
    return v.astype(np.int64)


def with_chroma(lumas):
    """Luma planes as packed I420 pictures with grey chroma."""
    lumas = np.asarray(lumas)
    n, h, w = lumas.shape
    return np.concatenate([lumas.reshape(n, -1), np.full((n, w * h // 2), 128, dtype=lumas.dtype)], axis=1).astype(np.uint8)


def noisy(lumas, noise, seed):
    """Independent uniform noise of +-noise on every sample of every frame (so on each field of it), clipped."""
    lumas = np.asarray(lumas).astype(np.int64)
    if noise:
        lumas = lumas + np.random.default_rng(seed).integers(-noise, noise + 1, lumas.shape)
    return np.clip(lumas, 0, 255)


def material(kind, n=21, first_field=TOP, w=48, h=32):
    """n luma planes: "progressive" (a frame per two field periods), "interlaced" (its two fields one field period apart,
    the one of parity first_field the earlier) or "still"."""
    out = []
    for t in range(n):
        if kind == "still":
            out.append(scene(0, w, h))
        elif kind == "progressive":
            out.append(scene(2 * t, w, h))
        else:
            f = scene(2 * t, w, h).copy()
            late = scene(2 * t + 1, w, h)
            f[1 - first_field::2] = late[1 - first_field::2]
            out.append(f)
    return np.stack(out)
