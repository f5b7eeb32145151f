"""NumPy model of efx_overlay, written from the text of include/efx.h ("subtitles and logos") alone: the validity rule,
activity, the gain of an event at a picture, sample alpha and colour, the luma blend, the premultiplied 2 x 2 chroma
blend, and the list order.  Divisions are plain integer divisions.  It shares no code with espflix_amd/csrc/overlay_px.h."""
import numpy as np

W, H, PICTURE = 352, 192, 101376
CB, CR = W * H, W * H + W * H // 4
A8, RGBA = 0, 1
BAD_EVENT = 8192
# the 64-byte record as the header's struct lists it
EVENT = np.dtype([("first", "<i8"), ("last", "<i8"), ("offset", "<u8"), ("stream", "<i4"), ("x", "<i4"), ("y", "<i4"), ("pitch", "<u4"),
                  ("colour", "<u4"), ("w", "<u2"), ("h", "<u2"), ("opacity", "<u2"), ("fade_in", "<u2"), ("fade_out", "<u2"),
                  ("kind", "u1"), ("reserved0", "u1"), ("reserved", "<u8")])
assert EVENT.itemsize == 64


def event(first=0, last=0, offset=0, stream=-1, x=0, y=0, pitch=None, colour=0xFFFFFF, w=1, h=1, opacity=256, fade_in=0, fade_out=0,
          kind=A8, reserved0=0, reserved=0):
    """One record; pitch None = the row's bytes; an RGBA event's colour defaults to 0."""
    e = np.zeros(1, dtype=EVENT)
    if kind == RGBA and colour == 0xFFFFFF:
        colour = 0
    e[0] = (first, last, offset, stream, x, y, w * (4 if kind == RGBA else 1) if pitch is None else pitch, colour, w, h, opacity, fade_in,
            fade_out, kind, reserved0, reserved)
    return e[0]


def events(records):
    out = np.zeros(len(records), dtype=EVENT)
    for i, r in enumerate(records):
        out[i] = r
    return out


def valid(e, atlas_bytes):
    kind, first, last = int(e["kind"]), int(e["first"]), int(e["last"])
    if kind not in (A8, RGBA) or not 0 <= first <= last < 1 << 40 or int(e["stream"]) < -1:
        return False
    if not (-4096 <= int(e["x"]) <= 4095 and -4096 <= int(e["y"]) <= 4095 and 1 <= int(e["w"]) <= 4096 and 1 <= int(e["h"]) <= 4096):
        return False
    if int(e["opacity"]) > 256 or int(e["fade_in"]) > 32767 or int(e["fade_out"]) > 32767:
        return False
    bpp = 4 if kind == RGBA else 1
    w, h, pitch, offset, colour = int(e["w"]), int(e["h"]), int(e["pitch"]), int(e["offset"]), int(e["colour"])
    if pitch < w * bpp:
        return False
    if kind == RGBA and (offset % 4 or pitch % 4 or colour != 0):
        return False
    if kind == A8 and colour >= 1 << 24:
        return False
    if offset + (h - 1) * pitch + w * bpp > int(atlas_bytes):
        return False
    return int(e["reserved0"]) == 0 and int(e["reserved"]) == 0


def check(evs, atlas_bytes):
    """efx_overlay_check: the first invalid event's index, or -1."""
    return next((i for i, e in enumerate(evs) if not valid(e, atlas_bytes)), -1)


def gain(e, p):
    def side(k, length):
        return 256 if length == 0 or k >= length else (256 * (k + 1)) // (length + 1)
    fi, fo = side(p - int(e["first"]), int(e["fade_in"])), side(int(e["last"]) - p, int(e["fade_out"]))
    return (int(e["opacity"]) * min(fi, fo) + 128) >> 8


def ycbcr(r, g, b):
    """The import's BT.601 studio-swing matrix on int arrays (or ints): (Y, Cb, Cr)."""
    r, g, b = (np.asarray(v, dtype=np.int64) for v in (r, g, b))
    y = np.clip(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, 0, 255)
    cb = np.clip(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128, 0, 255)
    cr = np.clip(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128, 0, 255)
    return y, cb, cr


def luma(y, c, a):
    """out = (2 t + 255) / 510 with t = Y (255 - a) + Cy a."""
    t = np.asarray(y, dtype=np.int64) * (255 - a) + np.asarray(c, dtype=np.int64) * a
    return (2 * t + 255) // 510


def chroma(C, a, c):
    """One plane's sites: C (...,) and the four alphas and colours a, c (4, ...)."""
    a, c = np.asarray(a, dtype=np.int64), np.asarray(c, dtype=np.int64)
    S, N = a.sum(axis=0), (a * c).sum(axis=0)
    return (np.asarray(C, dtype=np.int64) * (1020 - S) + N + 510) // 1020


def samples(e, atlas, g):
    """The bitmap of a valid event as (a, Cy, Ccb, Ccr), each (h, w) int64: alpha after the gain, and the colours."""
    w, h, pitch, offset = int(e["w"]), int(e["h"]), int(e["pitch"]), int(e["offset"])
    bpp = 4 if int(e["kind"]) == RGBA else 1
    at = offset + np.arange(h)[:, None] * pitch + np.arange(w * bpp)[None, :]
    raw = np.asarray(atlas, dtype=np.uint8)[at].astype(np.int64)
    if bpp == 4:
        px = raw.reshape(h, w, 4)
        A = px[:, :, 3]
        cy, ccb, ccr = ycbcr(px[:, :, 0], px[:, :, 1], px[:, :, 2])
    else:
        A = raw
        col = int(e["colour"])
        y1, cb1, cr1 = ycbcr(col >> 16 & 255, col >> 8 & 255, col & 255)
        cy, ccb, ccr = (np.full((h, w), int(v), dtype=np.int64) for v in (y1, cb1, cr1))
    return (A * g + 128) >> 8, cy, ccb, ccr


def blend(pic, e, atlas, g):
    """One active event on one picture (101376 uint8, changed in place)."""
    x, y, w, h = int(e["x"]), int(e["y"]), int(e["w"]), int(e["h"])
    x0, x1, y0, y1 = max(x, 0), min(x + w, W), max(y, 0), min(y + h, H)
    if x0 >= x1 or y0 >= y1:
        return
    a, cy, ccb, ccr = (v[y0 - y:y1 - y, x0 - x:x1 - x] for v in samples(e, atlas, g))
    Y = pic[:CB].reshape(H, W)
    Y[y0:y1, x0:x1] = luma(Y[y0:y1, x0:x1], cy, a)
    # the sites the rectangle touches, and their 2 x 2 luma samples: absent ones have a = 0
    cx0, cx1, cy0, cy1 = x0 // 2, (x1 + 1) // 2, y0 // 2, (y1 + 1) // 2
    box = np.zeros((3, 2 * (cy1 - cy0), 2 * (cx1 - cx0)), dtype=np.int64)
    sl = (slice(y0 - 2 * cy0, y1 - 2 * cy0), slice(x0 - 2 * cx0, x1 - 2 * cx0))
    box[0][sl], box[1][sl], box[2][sl] = a, ccb, ccr
    four = lambda v: np.stack([v[j::2, i::2] for j in (0, 1) for i in (0, 1)])
    for plane, first in ((1, CB), (2, CR)):
        C = pic[first:first + W * H // 4].reshape(H // 2, W // 2)
        C[cy0:cy1, cx0:cx1] = chroma(C[cy0:cy1, cx0:cx1], four(box[0]), four(box[plane]))


def overlay(pictures, evs, atlas, atlas_bytes=None, first_picture=0):
    """What efx_overlay leaves in pictures (n_streams, n_pictures, 101376): a new array.  atlas: the bytes at atlas_device
    (atlas_bytes of them count, all by default)."""
    out = np.array(pictures, dtype=np.uint8, copy=True)
    atlas_bytes = len(atlas) if atlas_bytes is None else atlas_bytes
    ok = [valid(e, atlas_bytes) for e in evs]
    for s in range(out.shape[0]):
        for j in range(out.shape[1]):
            p = first_picture + j
            for e, good in zip(evs, ok):
                if good and int(e["stream"]) in (-1, s) and int(e["first"]) <= p <= int(e["last"]):
                    blend(out[s, j], e, atlas, gain(e, p))
    return out


def status(evs, atlas_bytes):
    """The bit every status word gets."""
    return BAD_EVENT if check(evs, atlas_bytes) >= 0 else 0
