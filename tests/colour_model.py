"""NumPy model of the import's colour conversion (include/efx.h, "source colour"): the coefficients of a source matrix and
range recomputed in rational arithmetic from (Kr, Kb), the exact affine map they round, one pixel, and one picture -- the
samples inside the destination rectangle, a luma sample with the unconverted chroma of its 2 x 2 block.  It shares no code
with espflix_amd/csrc/colour_px.h."""
from fractions import Fraction as F

import numpy as np

import import_model as M

# H.273 matrix_coefficients: (Kr, Kb)
MATRICES = {1: ("0.2126", "0.0722"), 4: ("0.30", "0.11"), 5: ("0.299", "0.114"), 6: ("0.299", "0.114"),
            7: ("0.212", "0.087"), 9: ("0.2627", "0.0593")}
CODES = sorted(MATRICES)
INVALID_CODES = (0, 3, 8, 10, 11, 12, 13, 14, -1, 255)
NAMES = {"bt709": 1, "fcc": 4, "bt601": 6, "smpte240m": 7, "bt2020": 9, "auto": 2}
ONE = 1 << 14

# the 8-bit bars of the two standards (the issue's table): name, BT.709 studio, BT.601
BARS = [("red", (63, 102, 240), (81, 90, 240)), ("green", (173, 42, 26), (145, 54, 34)), ("blue", (32, 240, 118), (41, 240, 110)),
        ("yellow", (219, 16, 138), (210, 16, 146)), ("cyan", (188, 154, 16), (170, 166, 16)),
        ("magenta", (78, 214, 230), (106, 202, 222))]


def resolve(code, height=0):
    """Code 2 (unspecified): BT.709 above 576 lines, BT.601 otherwise.  None for an invalid code."""
    if code == 2:
        return 1 if height > 576 else 6
    return code if code in MATRICES else None


def exact(code, full_range):
    """The exact 3 x 3 matrix (Fractions, row major) that takes (Y - y0, Cb - 128, Cr - 128) of the source to
    (Y' - 16, Cb' - 128, Cr' - 128) of BT.601 studio swing, and y0."""
    kr, kb = (F(s) for s in MATRICES[code])
    kg = 1 - kr - kb
    # R, G, B from normalised (y, pb, pr)
    rgb = [[F(1), F(0), 2 * (1 - kr)],
           [F(1), -2 * (1 - kb) * kb / kg, -2 * (1 - kr) * kr / kg],
           [F(1), 2 * (1 - kb), F(0)]]
    # BT.601 (y', pb', pr') from R, G, B
    tr, tb = F("0.299"), F("0.114")
    tg = 1 - tr - tb
    yrow = [tr, tg, tb]
    to = [yrow,
          [(F(int(i == 2)) - yrow[i]) / (2 * (1 - tb)) for i in range(3)],
          [(F(int(i == 0)) - yrow[i]) / (2 * (1 - tr)) for i in range(3)]]
    m = [[sum(to[i][k] * rgb[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    sy, sc, y0 = (255, 255, 0) if full_range else (219, 224, 16)
    scale_in = [F(1, sy), F(1, sc), F(1, sc)]
    scale_out = [219, 224, 224]
    return [[m[i][j] * scale_out[i] * scale_in[j] for j in range(3)] for i in range(3)], y0


def coefs(code, full_range, height=0):
    """(q, y0): q = round(2^14 x exact) as nine ints, row major.  None for "off" (BT.601 studio)."""
    code = resolve(code, height)
    assert code is not None
    if code in (5, 6) and not full_range:
        return None
    m, y0 = exact(code, full_range)
    q = [int((v * ONE + F(1, 2)).__floor__()) for row in m for v in row]
    return q, y0


def convert_px(q, y0, y, cb, cr):
    """Arrays (or ints) of one source triple each -> (Y', Cb', Cr') int64 arrays."""
    y, u, v = np.asarray(y, dtype=np.int64) - y0, np.asarray(cb, dtype=np.int64) - 128, np.asarray(cr, dtype=np.int64) - 128
    yy = 16 + ((q[0] * y + q[1] * u + q[2] * v + 8192) >> 14)
    bb = 128 + ((q[4] * u + q[5] * v + 8192) >> 14)
    rr = 128 + ((q[7] * u + q[8] * v + 8192) >> 14)
    return tuple(np.clip(c, 0, 255) for c in (yy, bb, rr))


def convert(picture, rect, q, y0):
    """(..., 101376) I420 pictures of 352 x 192 with the samples inside rect = (x, y, w, h) (None: the frame) converted."""
    pic = np.array(picture, dtype=np.uint8)
    flat = pic.reshape(-1, M.FRAME_BYTES)
    x, y, w, h = rect or (0, 0, M.W, M.H)
    for p in flat:
        Y = p[:M.Y_BYTES].reshape(M.H, M.W)[y:y + h, x:x + w]
        U = p[M.Y_BYTES:M.Y_BYTES + M.C_BYTES].reshape(M.CH, M.CW)[y // 2:(y + h) // 2, x // 2:(x + w) // 2]
        V = p[M.Y_BYTES + M.C_BYTES:].reshape(M.CH, M.CW)[y // 2:(y + h) // 2, x // 2:(x + w) // 2]
        u2, v2 = (np.repeat(np.repeat(c, 2, axis=0), 2, axis=1) for c in (U, V))  # the 2 x 2 block's chroma, unconverted
        yy = convert_px(q, y0, Y, u2, v2)[0]
        _, bb, rr = convert_px(q, y0, 0, U, V)
        Y[...], U[...], V[...] = yy, bb, rr
    return pic


def source_limit(limit, full_range):
    """The largest source luma whose converted value, the chroma terms at zero, is <= limit (0 when there is none)."""
    if not full_range:
        return limit
    q, y0 = coefs(6, True)
    ok = [y for y in range(256) if int(convert_px(q, y0, y, 128, 128)[0]) <= limit]
    return max(ok, default=0)


if __name__ == "__main__":
    for c in CODES:
        for fr in (0, 1):
            print(c, fr, coefs(c, fr))
