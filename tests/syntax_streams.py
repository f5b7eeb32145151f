"""Directed MPEG-1 video streams, written bit by bit (test input only).

The generator (espflix_amd/gen) is a good workload and a narrow sample of the syntax: forward_f_code 1 or 2, vectors of a
few pels, and whichever VLC codes its content happens to need.  The families here reach the rest on purpose:

  codes()    every entry of every code book (address increments and escapes, macroblock types, patterns, motion codes,
             DCT run / level pairs in both positions and signs, escapes, dct_dc_size, quantiser scales)
  vectors()  one P picture per forward_f_code 1 ... 7 x full_pel 0 / 1: every motion code the picture's geometry can
             reach, the residuals 0, 2^r - 1 and one between, the ends of the range, wraps, predictor resets
  windows()  every alignment of k_recon's 9 x 9 window fetch, and windows flush with every edge and corner
  outside()  vectors that leave the picture -- undefined in the reference (it reads outside its frame buffers), defined
             by the oracle as a clamp of the coordinates; compared with the oracle only
  coefs()    the path from coefficient to pixel inside the reference's domain: every scan position alone under the default
             and under loaded matrices, the dequantiser's rounding classes, blocks of 64 coefficients by the wave
  range()    the same path outside the domain (oracle only): every AC coefficient saturated in the sign patterns that
             maximise the IDCT's multiplied operands and its residuals, and intra DC predictors walked far out of 0 ... 255

Every stream starts with the sequence header, GOP header and I picture of gen.Batch(0, 1, 1, 12, 0) (as
common.stuffing_es does); what follows is written here.  A family returns a list of Stream: the elementary stream and a
manifest of what the writer MEANT -- per hand-written picture its type, f_code, full_pel and the quantiser matrices in force,
per macroblock its address, type, vector in half-pels, pattern, quantiser and every coded block's (scan position, level)
list -- which tests/test_syntax_streams.py holds against the oracle's parse
trace.  The VLC codes come from tests/golden/codebooks.json (the reference's own books, expanded); dct_dc_size
(ISO 11172-2 tables B-5a / B-5b), which that file lacks, is written out below.

Domain condition of the reference: it clamps reconstructed pixels through a 768-entry table (index -256 ... 511), and an
intra block of one coefficient is stored without a clamp.  The writer therefore keeps the sum of |dequantised coefficient|
of a block <= 900 (no basis function of the 8 x 8 IDCT exceeds a quarter of its coefficient: residual within +-225 of a
0 ... 255 prediction) and every intra DC value within 0 ... 255, and asserts both.  (A non-intra coefficient at scan position 0
is flat, an eighth of its value; Writer.pred_range narrows the prediction a family has arranged for.  Writer(domain=False)
drops both assertions: streams for the oracle alone.)
"""
import functools
import json
import os
from dataclasses import dataclass, field

import numpy as np

import common

MBW, MBH = 22, 12
W, H = 352, 192
X_MAX, Y_MAX = 2 * (W - 17) + 1, 2 * (H - 17) + 1   # largest half-pel position of a 17 x 17 fetch: 671, 351

T_SKIPPED, T_INTRA, T_PATTERN, T_FORWARD, T_QUANT = "skipped", 1, 2, 8, 16   # macroblock_type flags as the reference names them

DC_LUMA = ["100", "00", "01", "101", "110", "1110", "11110", "111110", "1111110"]          # B-5a, dct_dc_size 0 ... 8
DC_CHROMA = ["00", "01", "10", "110", "1110", "11110", "111110", "1111110", "11111110"]    # B-5b
ESCAPE = (0b000001, 6)
EOB = (0b10, 2)


@functools.lru_cache(maxsize=None)
def books():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codebooks.json")
    with open(path) as f:
        j = json.load(f)
    tree = lambda name: {v: (c, n) for c, n, v in j[name]}
    return {"mba": tree("macroblock_address_increment"), "type_i": tree("macroblock_type_I"), "type_p": tree("macroblock_type_P"),
            "cbp": tree("coded_block_pattern"), "motion": tree("motion_vec"), "dct": {(r, l): (c, n) for c, n, r, l in j["dct"]}}


@functools.lru_cache(maxsize=None)
def head() -> bytes:
    from espflix_amd import gen
    return gen.Batch(0, 1, 1, 12, 0).es(0).tobytes()


@dataclass
class Stream:
    name: str
    es: bytes
    pictures: list = field(default_factory=list)   # manifest; entry 0 is None (the generator's I picture)

    def array(self):
        return np.frombuffer(self.es, dtype=np.uint8)

    def macroblocks(self):
        return sum(len(p["mbs"]) for p in self.pictures if p)


ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# ISO 11172-2 2.4.3.2, default intra quantiser matrix in raster order (tests/test_syntax_streams.py holds it against the oracle's)
DEFAULT_INTRA = [8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
                 22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83]
_AAN = [1.0] + [2 ** 0.5 * float(np.cos(k * np.pi / 16)) for k in range(1, 8)]
PREMUL = [[int(32 * _AAN[r] * _AAN[c] + 0.5) for c in range(8)] for r in range(8)]   # scale_dct_q (player.cpp:161-170), [row][column]


def by_scan(sent=None, default=None):
    """The matrix entry applied at each scan position.  A loaded matrix is stored in arrival order and indexed by the RASTER
    position (player.cpp:646-651, 1113): scan position n meets the ZIGZAG[n]-th byte sent."""
    if sent is None:
        return [default[ZIGZAG[n]] for n in range(64)]
    return [sent[ZIGZAG[n]] for n in range(64)]


def dequant(level: int, q: int, m: int, intra: bool) -> int:
    """player.cpp:1110-1121 in plain integers: matrix entry m, truncation toward zero, even values moved toward zero (0
    becomes 1), saturation."""
    v = 2 * level
    if not intra:
        v += -1 if v < 0 else 1
    p = v * q * m
    v = abs(p) // 16 * (1 if p >= 0 else -1)
    if v % 2 == 0:
        v -= 1 if v > 0 else -1
    return max(-2048, min(2047, v))


def dequant_non_intra(level: int, q: int) -> int:
    """player.cpp:1110-1121 with the default non-intra matrix (16)."""
    v = 2 * level + (1 if level > 0 else -1)
    v = int(v * q * 16 / 16)
    if v % 2 == 0:
        v -= 1 if v > 0 else -1
    return max(-2048, min(2047, v))


mutation = None   # (stream, picture, macroblock address, block, coefficient index, "sign" / "move"): see rebuild()


def mutate(coefs, k, kind):
    """One coefficient of a block's list with its sign flipped, or moved one scan position on (the next one closes up)."""
    coefs = [c if len(c) == 3 else (c[0], c[1], "vlc") for c in coefs]
    run, level, form = coefs[k]
    if kind == "sign":
        coefs[k] = _level(run, -level) if form == "vlc" else (run, -level, form)
    else:
        coefs[k] = _level(run + 1, level) if form == "vlc" else (run + 1, level, form)
        if k + 1 < len(coefs):
            r2, l2, f2 = coefs[k + 1]
            assert r2 > 0
            coefs[k + 1] = _level(r2 - 1, l2) if f2 == "vlc" else (r2 - 1, l2, f2)
    return coefs


class Writer:
    """Pictures, slices and macroblocks; keeps the manifest and the reference's predictors while it writes."""

    def __init__(self, name, domain=True):
        self.name = name
        self.domain = domain          # assert the reference's domain condition (module docstring)
        self.pred_range = (0, 248)    # what a non-intra block's prediction can hold
        self.b = common._Bits()
        self.codes = []               # where start codes were written: done() finds no other

        def start_code(code):
            common._Bits.start_code(self.b, code)
            self.codes.append(len(self.b.out) - 4)
        self.b.start_code = start_code
        self.pictures = [None]
        self.pic = None
        self.tref = 0
        self.intra_m, self.non_intra_m = by_scan(default=DEFAULT_INTRA), [16] * 64
        self.custom = False

    # ---- headers ------------------------------------------------------------------------------------------------------
    def sequence(self, intra=None, non_intra=None):
        """A further sequence header (and GOP header, as the generator sends them) in front of the next picture; intra /
        non_intra: 64 bytes in the order they are sent, or None: the default returns."""
        b = self.b
        b.start_code(0xB3)
        b.put(W, 12)
        b.put(H, 12)
        b.put(1, 4)
        b.put(4, 4)
        b.put(3750, 18)
        b.put(1, 1)
        b.put(20, 10)
        b.put(0, 1)
        for m in (intra, non_intra):
            b.put(m is not None, 1)
            for v in m or []:
                assert 1 <= v <= 255
                b.put(v, 8)
        b.start_code(0xB8)
        b.put(1 << 12, 25)
        b.put(1, 1)
        b.put(0, 6)
        self.intra_m = by_scan(intra, DEFAULT_INTRA)
        self.non_intra_m = by_scan(non_intra, [16] * 64)
        self.custom = intra is not None or non_intra is not None

    def picture(self, f_code=1, full_pel=0, intra=False):
        self.tref += 1
        b = self.b
        b.start_code(0x00)
        b.put(self.tref, 10)
        b.put(1 if intra else 2, 3)
        b.put(0xFFFF, 16)      # vbv_delay
        if not intra:
            b.put(full_pel, 1)
            b.put(f_code, 3)
        b.put(0, 1)            # extra_bit_picture
        self.pic = dict(type=1 if intra else 2, f_code=f_code, full_pel=full_pel, mbs=[], custom=self.custom,
                        intra_m=list(self.intra_m), non_intra_m=list(self.non_intra_m))
        self.pictures.append(self.pic)
        self.r_size = f_code - 1
        self.unit = 2 if full_pel else 1

    def slice(self, row, q):
        self.b.start_code(row + 1)
        self.b.put(q, 5)
        self.b.put(0, 1)       # extra_bit_slice
        self.q = q
        self.addr = row * MBW - 1
        self.first = True
        self.reset()

    def reset(self):
        self.pred = [0, 0]
        self.dc = [128, 128, 128]   # luminance, Cr, Cb

    # ---- macroblock layer ---------------------------------------------------------------------------------------------
    def increment(self, inc, stuffing=0):
        bk = books()["mba"]
        for _ in range(stuffing):
            self.b.put(*bk[34])
        n = inc
        while n > 33:
            self.b.put(*bk[35])
            n -= 33
        self.b.put(*bk[n])
        if self.first:
            assert inc == 1   # (the reference ignores the first increment of a slice: kept legal)
            self.addr += 1
            self.first = False
            return
        for _ in range(inc - 1):
            self.addr += 1
            self.pic["mbs"].append(dict(addr=self.addr, type=T_SKIPPED, mv=(0, 0), cbp=0, q=0, blocks=[]))
        if inc > 1:
            self.reset()
        self.addr += 1

    def motion_delta(self, comp, code, residual):
        """One component by its motion code and residual; returns the vector in the picture's units (motion_vector(),
        player.cpp:891-910)."""
        self.b.put(*books()["motion"][code])
        scale = 1 << self.r_size
        if code and self.r_size:
            self.b.put(residual, self.r_size)
            delta = ((abs(code) - 1) << self.r_size) + residual + 1
            delta = -delta if code < 0 else delta
        else:
            delta = code
        m = self.pred[comp] + delta
        if m > 16 * scale - 1:
            m -= 32 * scale
        elif m < -16 * scale:
            m += 32 * scale
        self.pred[comp] = m
        return m

    def encode_target(self, comp, target):
        """(code, residual) that takes the predictor to `target` (units of the picture), through a wrap where needed."""
        scale = 1 << self.r_size
        assert -16 * scale <= target < 16 * scale
        d = (target - self.pred[comp] + 16 * scale) % (32 * scale) - 16 * scale   # -16 scale ... 16 scale - 1
        if d == 0:
            return 0, 0
        a = abs(d) - 1
        code = (a >> self.r_size) + 1
        return (code if d > 0 else -code), a & (scale - 1)

    def mb(self, inc=1, type=T_FORWARD, mv=None, codes=None, cbp=None, quant=None, blocks=None, stuffing=0, dc=None):
        """mv: target vector in half-pels, or codes = ((code, residual), (code, residual)).  blocks: for each coded block
        of the pattern a list of coefficients (run, level) / (run, level, form), form "vlc" (default), "short", "long"
        (level -256 and a coded level 0 exist in the long form only).  dc: for an intra macroblock six differentials
        (default 0).  The manifest keeps per coded block its [(scan position, level)], an intra block's first entry being
        (0, DC value)."""
        P = self.pic
        self.increment(inc, stuffing)
        if quant is not None:
            type |= T_QUANT
        self.b.put(*books()["type_i" if P["type"] == 1 else "type_p"][type])
        if quant is not None:
            self.b.put(quant, 5)
            self.q = quant
        vec = (0, 0)
        if type & T_INTRA:
            self.pred = [0, 0]
        else:
            self.dc = [128, 128, 128]
            if type & T_FORWARD:
                if codes is None:
                    assert mv[0] % self.unit == 0 and mv[1] % self.unit == 0
                    codes = [self.encode_target(c, mv[c] // self.unit) for c in (0, 1)]
                vec = tuple(self.motion_delta(c, *codes[c]) * self.unit for c in (0, 1))
                assert mv is None or vec == tuple(mv), (vec, mv)
            else:
                self.pred = [0, 0]
        if type & T_PATTERN:
            self.b.put(*books()["cbp"][cbp])
        else:
            cbp = 63 if type & T_INTRA else 0
        blocks = list(blocks or [])
        entries = []
        for blk in range(6):
            if cbp & (0x20 >> blk):
                default = [] if type & T_INTRA else [(0, 1)]   # (a coded non-intra block holds at least one coefficient)
                entries.append(self.block(blk, bool(type & T_INTRA), blocks.pop(0) if blocks else default, dc[blk] if dc else 0))
        assert not blocks
        P["mbs"].append(dict(addr=self.addr, type=type, mv=vec, cbp=cbp, q=self.q, blocks=entries))
        return vec

    # ---- block layer --------------------------------------------------------------------------------------------------
    def block(self, blk, intra, coefs, dc_diff=0):
        b = self.b
        n, flat, ac = 0, 0, 0
        entries = []
        zero_seen = False
        if mutation and mutation[:4] == (self.name, len(self.pictures) - 1, self.addr, blk):
            coefs = mutate(coefs, *mutation[4:])
        if intra:
            size = 0 if dc_diff == 0 else abs(dc_diff).bit_length()
            assert size <= 8
            code = (DC_LUMA if blk < 4 else DC_CHROMA)[size]
            b.put(int(code, 2), len(code))
            if size:
                b.put(dc_diff if dc_diff > 0 else dc_diff + (1 << size) - 1, size)
            k = 0 if blk < 4 else blk - 3
            self.dc[k] += dc_diff
            assert not self.domain or 0 <= self.dc[k] <= 255, "intra DC leaves 0 ... 255"
            entries.append((0, self.dc[k]))
            n = 1
        for c in coefs:
            run, level, form = c if len(c) == 3 else (c[0], c[1], "vlc")
            assert -256 <= level <= 255 and (level not in (0, -256) or form == "long")
            assert level == 0 or not zero_seen, "a coded level 0 stands behind the last real coefficient"
            zero_seen |= level == 0
            if form == "vlc" and (run, abs(level)) == (0, 1):   # "1s" as a block's first code, "11s" later
                b.put(0b11 if n else 0b1, 2 if n else 1)
                b.put(level < 0, 1)
            elif form == "vlc":
                b.put(*books()["dct"][(run, abs(level))])
                b.put(level < 0, 1)
            else:
                b.put(*ESCAPE)
                b.put(run, 6)
                if form == "short":                              # one byte, -127 ... 127
                    assert -127 <= level <= 127 and level
                    b.put(level & 0xFF, 8)
                elif level >= 0:                                 # 00 xx
                    b.put(0, 8)
                    b.put(level, 8)
                else:                                            # 80 xx = xx - 256
                    b.put(0x80, 8)
                    b.put(level + 256, 8)
            n += run
            assert n <= 63, "coefficient beyond scan position 63"
            v = abs(dequant(level, self.q, (self.intra_m if intra else self.non_intra_m)[n], intra))
            if n == 0:
                flat += v
            else:
                ac += v
            entries.append((n, level))
            n += 1
        if self.domain:
            # |residual| <= flat / 8 + ac / 4; the clamp table takes -256 ... 511
            bound = -(-(flat + 2 * ac) // 8)
            lo, hi = (self.dc[0 if blk < 4 else blk - 3],) * 2 if intra else self.pred_range
            assert (flat + ac <= 900 or self.pred_range != (0, 248)) and lo - bound >= -256 and hi + bound <= 511, \
                "block outside the reference's clamp table domain"
        b.put(*EOB)
        return entries

    def done(self):
        self.b.align()
        # (a coded level 0 is 16 zero bits: with a run of 0 in front and another escape behind it would make 23)
        out = bytes(self.b.out)
        found = [i for i in range(len(out) - 2) if out[i:i + 3] == b"\x00\x00\x01"]
        assert found == self.codes, f"the macroblock data emulates a start code at {sorted(set(found) - set(self.codes))}"
        return Stream(self.name, head() + bytes(self.b.out), self.pictures)


# ---- geometry shared by the writer, the tests and the NumPy prediction ----------------------------------------------------
def mb_xy(addr):
    return addr % MBW, addr // MBW


def fetch_inside(addr, mv):
    """The 17 x 17 fetch of a vector lies inside the picture (SURVEY 8a stream constraint)."""
    x, y = mb_xy(addr)
    X, Y = 32 * x + mv[0], 32 * y + mv[1]
    return 0 <= X <= X_MAX + (1 - X % 2) and 0 <= Y <= Y_MAX + (1 - Y % 2)


def block_windows(addr, mv):
    """Per block of a macroblock what k_recon's window fetch works from: (blk, px0, py0, hx, hy, pw, ph)."""
    x, y = mb_xy(addr)
    X, Y = 32 * x + mv[0], 32 * y + mv[1]
    out = []
    for blk in range(6):
        luma = blk < 4
        PX = X + (blk & 1) * 16 if luma else X >> 1
        PY = Y + (blk >> 1) * 16 if luma else Y >> 1
        out.append((blk, PX >> 1, PY >> 1, PX & 1, PY & 1, W if luma else W // 2, H if luma else H // 2))
    return out


def alignment_sets(mbs):
    """From (addr, mv) of motion macroblocks: luma {(px0 & 3, hx, hy)}, chroma {(blk, px0 & 3, hx, hy, py0 & 7)} and the flush
    cases {(plane kind, side, half-pel flag at that side)} of windows that lie inside; corners as (kind, 'corner', side pair)."""
    luma, chroma, flush = set(), set(), set()
    for addr, mv in mbs:
        for blk, px0, py0, hx, hy, pw, ph in block_windows(addr, mv):
            if not (px0 >= 0 and py0 >= 0 and px0 + 8 + hx <= pw and py0 + 8 + hy <= ph):
                continue
            if blk < 4:
                luma.add((px0 & 3, hx, hy))
            else:
                chroma.add((blk, px0 & 3, hx, hy, py0 & 7))
            kind = "luma13" if blk in (1, 3) else ("luma" if blk < 4 else ("cr" if blk == 4 else "cb"))
            sides = []
            if px0 == 0:
                sides.append(("left", hx))
            if px0 + 8 + hx == pw:
                sides.append(("right", hx))
            if py0 == 0:
                sides.append(("top", hy))
            if py0 + 8 + hy == ph:
                sides.append(("bottom", hy))
            for s in sides:
                flush.add((kind, s[0], s[1]))
            if len(sides) == 2:
                flush.add((kind, "corner", sides[0][0] + "-" + sides[1][0], sides[0][1], sides[1][1]))
    return luma, chroma, flush


def planes(frame):
    """A frame as the decoder stores it (12 strips of 16 rows of 352 luma + 176 chroma bytes; Cr in a strip's upper eight rows,
    Cb in its lower eight) -> (Y 192 x 352, Cr 96 x 176, Cb 96 x 176)."""
    f = np.asarray(frame, dtype=np.uint8).reshape(12, 16, 528)
    return f[:, :, :352].reshape(192, 352), f[:, :8, 352:].reshape(96, 176), f[:, 8:, 352:].reshape(96, 176)


def mocomp(plane, pos_x, pos_y, size):
    """The four cases of mocomp() (player.cpp:733-821) at a half-pel position inside a plane; coordinates are clamped the way
    the oracle defines vectors that leave the picture (no effect inside)."""
    ph, pw = plane.shape
    hx, hy = pos_x & 1, pos_y & 1
    ys = np.clip((pos_y >> 1) + np.arange(size + 1), 0, ph - 1)
    xs = np.clip((pos_x >> 1) + np.arange(size + 1), 0, pw - 1)
    w = plane[np.ix_(ys, xs)].astype(np.int32)
    a, b, c, d = w[:size, :size], w[:size, 1:], w[1:, :size], w[1:, 1:]
    if not hx and not hy:
        return a.astype(np.uint8)
    if hx and not hy:
        return ((a + b + 1) >> 1).astype(np.uint8)
    if not hx:
        return ((a + c + 1) >> 1).astype(np.uint8)
    return ((a + b + c + d + 2) >> 2).astype(np.uint8)


def predict_mb(ref_planes, addr, mv):
    """predict() (player.cpp:870-889): luma at the vector, chroma at the floor of the halved POSITION."""
    x, y = mb_xy(addr)
    X, Y = 32 * x + mv[0], 32 * y + mv[1]
    return mocomp(ref_planes[0], X, Y, 16), mocomp(ref_planes[1], X >> 1, Y >> 1, 8), mocomp(ref_planes[2], X >> 1, Y >> 1, 8)


def predict_picture(ref_frame, mbs):
    """A P picture of motion-only / skipped macroblocks from its reference picture; macroblocks the list does not name keep
    the value 0 and are reported in the returned mask as not predicted."""
    rp = planes(ref_frame)
    out = [np.zeros_like(p) for p in rp]
    mask = np.zeros(MBW * MBH, dtype=bool)
    for addr, mv in mbs:
        x, y = mb_xy(addr)
        l, cr, cb = predict_mb(rp, addr, mv)
        out[0][16 * y:16 * y + 16, 16 * x:16 * x + 16] = l
        out[1][8 * y:8 * y + 8, 8 * x:8 * x + 8] = cr
        out[2][8 * y:8 * y + 8, 8 * x:8 * x + 8] = cb
        mask[addr] = True
    return out, mask


def mb_pixels(pl, addr):
    x, y = mb_xy(addr)
    return (pl[0][16 * y:16 * y + 16, 16 * x:16 * x + 16], pl[1][8 * y:8 * y + 8, 8 * x:8 * x + 8], pl[2][8 * y:8 * y + 8, 8 * x:8 * x + 8])


# ---- family: codes ------------------------------------------------------------------------------------------------------
ESCAPE_LEVELS = [1, -1, 127, -127, 128, -128, 255, -255]


def _codes_mba():
    """Address increments 1 ... 33 and escape + 1 ... 33 (34 ... 66): one slice per picture that spans its rows, the skipped
    macroblocks between two coded ones copy the previous picture.  2211 addresses do not fit five pictures: two streams."""
    incs = list(range(1, 67))
    rng = np.random.default_rng(3)
    rng.shuffle(incs)
    streams, w, room = [], None, 0
    while incs:
        if w is None or len(w.pictures) == 8:
            if w:
                streams.append(w.done())
            w = Writer(f"codes_mba_{len(streams)}")
        w.picture(f_code=1)
        w.slice(0, 4)
        w.mb(mv=(0, 0))
        room = MBW * MBH - 1
        while incs and min(incs) <= room:
            k = next(i for i in incs if i <= room)
            incs.remove(k)
            room -= k
            # small vectors in the interior, none at the picture's border
            x, y = mb_xy(w.addr + k)
            inner = 0 < x < MBW - 1 and 0 < y < MBH - 1
            w.mb(inc=k, mv=(int(rng.integers(-3, 4)), int(rng.integers(-3, 4))) if inner else (0, 0), stuffing=int(k % 5 == 0))
        while room:   # the rest of the picture, in ones
            w.mb(mv=(0, 0))
            room -= 1
    streams.append(w.done())
    return streams


def _codes_main():
    """Macroblock types, patterns, motion codes at f_code 1, the DCT book, escapes, quantiser scales; then a hand-written I
    picture with both I types and every dct_dc_size."""
    bk = books()
    w = Writer("codes_main")
    rng = np.random.default_rng(5)

    # picture 1: all 63 patterns (pattern-only and motion + pattern macroblocks) carrying the DCT book: each entry with both
    # signs, once as a block's first coefficient and once later in it; quantiser 1 keeps the largest level (40) at 81
    entries = sorted(bk["dct"])
    jobs = []
    for (run, level) in entries + [(0, 1)]:
        for s in (1, -1):
            jobs.append([(run, s * level), (run, -s * level)])       # first, later: position run, then 2 run + 1 <= 63
    jobs.append([(31, 1), (31, -1)])                                   # ... the second lands exactly on scan position 63
    w.picture(f_code=1)
    patterns = list(range(1, 64))
    pat_i = 0
    row = 0
    w.slice(0, 1)
    col = 0
    while jobs or pat_i < 63:
        cbp = patterns[pat_i % 63]
        pat_i += 1
        nblk = bin(cbp).count("1")
        blocks = [jobs.pop(0) if jobs else [(0, 1)] for _ in range(nblk)]
        if col == MBW:
            row, col = row + 1, 0
            w.slice(row, 1)
        if pat_i % 2:
            w.mb(type=T_PATTERN, cbp=cbp, blocks=blocks)
        else:
            w.mb(type=T_FORWARD | T_PATTERN, mv=(0, 0), cbp=cbp, blocks=blocks)
        col += 1
    while row < MBH:
        while col < MBW:
            w.mb(mv=(0, 0))
            col += 1
        row, col = row + 1, 0
        if row < MBH:
            w.slice(row, 1)

    # picture 2: all 33 motion codes in each component at f_code 1 (the range is -16 ... 15 half-pels: +-16 and the
    # far codes wrap), in the interior rows; escapes in every form in rows 0 and 11
    w.picture(f_code=1)
    esc = []
    for run in (0, 63):
        for level in ESCAPE_LEVELS:
            forms = ["short", "long"] if abs(level) <= 127 else ["long"]
            for form in forms:
                esc.append([(run, level, form)])                       # as the first coefficient
                if run == 0:
                    esc.append([(1, 1), (0, level, form)])             # and later in a block
    esc.append([(0, 1), (62, -255, "long")])                           # an escape that lands on scan position 63
    hcodes = [c for k in range(17) for c in ((k, -k) if k else (0,))]
    vcodes = hcodes[::-1]
    for row in range(MBH):
        w.slice(row, 1)
        for col in range(MBW):
            if row in (0, MBH - 1) or col in (0, MBW - 1):
                if esc and col not in (0, MBW - 1):
                    w.mb(type=T_PATTERN, cbp=32, blocks=[esc.pop(0)])
                else:
                    w.mb(mv=(0, 0))
            else:
                hc = hcodes.pop(0) if hcodes else int(rng.integers(-16, 17))
                vc = vcodes.pop(0) if vcodes else int(rng.integers(-16, 17))
                w.mb(codes=((hc, 0), (vc, 0)))
    assert not esc and not hcodes and not vcodes

    # pictures 3 ... 5: every P macroblock type; quantiser_scale 1 ... 31 in slice headers and as a macroblock's own
    # (level 1 at quantiser 31 dequantises to 93)
    w.picture(f_code=1)
    qs = list(range(1, 32))
    types = [T_FORWARD | T_PATTERN, T_PATTERN, T_FORWARD, T_INTRA, T_FORWARD | T_PATTERN | T_QUANT, T_PATTERN | T_QUANT,
             T_INTRA | T_QUANT]
    # (31 slice headers do not fit the 12 rows of one picture: pictures 3, 4 and 5 share them)
    for pic in range(3):
        if pic:
            w.picture(f_code=1)
        for row in range(MBH):
            sq = qs[(pic * MBH + row) % 31]
            w.slice(row, sq)
            for col in range(MBW):
                k = (pic * MBH + row) * MBW + col
                t = types[k % 7]
                mq = qs[(k // 7) % 31] if t & T_QUANT else None
                kw = dict(type=t & ~T_QUANT, quant=mq)
                if t & T_FORWARD:
                    inner = 0 < col < MBW - 1 and 0 < row < MBH - 1
                    kw["mv"] = (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))) if inner else (0, 0)
                if t & T_PATTERN:
                    kw["cbp"] = int(rng.integers(1, 64))
                    kw["blocks"] = [[(int(rng.integers(0, 3)), int(rng.choice([-1, 1])))] for _ in range(bin(kw["cbp"]).count("1"))]
                if t & T_INTRA:
                    kw["dc"] = [int(d) for d in rng.integers(-20, 21, 6)]
                    kw["blocks"] = [[(0, int(rng.choice([-1, 1])))] if b % 2 else [] for b in range(6)]
                w.mb(**kw)

    # picture 6: an I picture with both I types; dct_dc_size 0 ... 8 with both signs of the differential, for luminance and
    # for each chrominance predictor: from 128 down to 0, up again, in halving steps (every value stays inside 0 ... 255)
    walk = []
    for size in range(8, 0, -1):
        walk += [-(1 << (size - 1)), 1 << (size - 1)]
    walk.append(0)
    w.picture(intra=True)
    luma = list(walk)
    chroma = list(walk)
    for row in range(MBH):
        w.slice(row, 2 + row)
        for col in range(MBW):
            if row == 0:
                dc = [luma.pop(0) if luma else 0 for _ in range(4)] + ([chroma[0]] * 2 if chroma else [0, 0])
                chroma = chroma[1:]
            else:
                dc = [int(d) for d in rng.integers(-6, 7, 6)]
                dc = [d if 8 <= w.dc[0 if b < 4 else b - 3] + 4 * d <= 240 else 0 for b, d in enumerate(dc)]
                for b in range(1, 4):
                    dc[b] = 0
            quant = (row + col) % 31 + 1 if (row * MBW + col) % 3 == 0 else None
            w.mb(type=T_INTRA, quant=quant, dc=dc,
                 blocks=[[(0, 1)] if (b + col) % 4 == 0 and (quant or 2 + row) <= 31 else [] for b in range(6)])
    assert not luma and not chroma

    # picture 7: a P picture on top of the hand-written I picture (its vectors read what the I picture left)
    w.picture(f_code=2)
    for row in range(MBH):
        w.slice(row, 3)
        for col in range(MBW):
            inner = 0 < col < MBW - 1 and 0 < row < MBH - 1
            w.mb(mv=(int(rng.integers(-9, 10)), int(rng.integers(-9, 10))) if inner else (0, 0))
    return [w.done()]


def codes():
    return _codes_mba() + _codes_main()


# ---- family: vectors ------------------------------------------------------------------------------------------------------
def reachable(comp, f_code, full_pel):
    """What the picture's geometry lets one component of a vector do while the 17 x 17 fetch stays inside the picture.  The
    predictor passes between neighbours of a row: positions 32 x + h of macroblocks x and x + 1 lie in 0 ... 671, so a positive
    step is at most 639 half-pels; vertically both share the row, 0 ... 351.  In units of the picture (half-pels, or pels
    with full_pel) that is D = 639 // u or 351 // u.  A motion code of magnitude k needs a step of at least
    ((k - 1) << r_size) + 1: k <= ((D - 1) >> r_size) + 1.  A wrap needs two in-picture vectors 16 * scale apart or more.
    Returns (largest code magnitude, wraps reachable, lower end inside, upper end inside)."""
    u = 2 if full_pel else 1
    r = f_code - 1
    scale = 1 << r
    D = (639 if comp == 0 else 351) // u
    span = (672 if comp == 0 else 352)
    return (min(16, ((D - 1) >> r) + 1), 16 * scale <= D, 16 * scale * u <= span, (16 * scale - 1) * u <= (X_MAX if comp == 0 else Y_MAX))


def _allowed(comp, pos, u):
    """Vectors (in units) of macroblock column / row `pos` that keep the fetch inside: lo ... hi."""
    top = X_MAX if comp == 0 else Y_MAX
    return -((32 * pos) // u), (top + (u == 2) - 32 * pos) // u   # (an even position needs no 17th pixel: 672 / 352 with full_pel)


RESET_ROW = 6


def _vector_picture(w, f_code, full_pel, rng):
    """One P picture of "motion, not coded" macroblocks (but for the two macroblocks a reset needs).  Macroblocks come in
    pairs of columns (0, 1), (2, 3) ...: the first of a pair puts the predictor where the second's goal needs it."""
    u = 2 if full_pel else 1
    r = f_code - 1
    scale = 1 << r
    lo_m, hi_m = -16 * scale, 16 * scale - 1
    w.picture(f_code=f_code, full_pel=full_pel)

    def goals(comp):
        kmax, wraps, lo_in, hi_in = reachable(comp, f_code, full_pel)
        res = [0, scale - 1, scale // 2 - 1 if scale > 2 else 0]   # (r_size 1 has no third value)
        out = []
        n = 0
        for k in range(1, kmax + 1):
            for s in (1, -1):
                out.append(("code", s * k, [res[(n + i) % 3] for i in range(3)] if r else [0]))   # (the first that fits)
                n += 1
        if r:
            for s in (1, -1):   # each residual kind with either sign once more, at the smallest code
                for rr in res:
                    out.append(("code", s, [rr]))
        if lo_in:
            out.append(("target", lo_m))
        if hi_in:
            out.append(("target", hi_m))
        if wraps:
            out += [("wrap", 1), ("wrap", -1)]
        return out

    def step(pred, code, residual):
        d = ((abs(code) - 1) << r) + residual + 1 if (code and r) else abs(code)
        m = pred + (d if code > 0 else -d)
        wrapped = 0
        if m > hi_m:
            m, wrapped = m - 32 * scale, 1
        elif m < lo_m:
            m, wrapped = m + 32 * scale, -1
        return m, wrapped

    def place(comp, goal, pos_a, pos_b):
        """(predictor at the pair's first macroblock, (code, residual) or target at its second) or None."""
        la, ha = _allowed(comp, pos_a, u)
        lb, hb = _allowed(comp, pos_b, u)
        la, ha, lb, hb = max(la, lo_m), min(ha, hi_m), max(lb, lo_m), min(hb, hi_m)
        if la > ha or lb > hb:
            return None
        cands = sorted({la, ha, (la + ha) // 2, la + 1, ha - 1} | {int(v) for v in rng.integers(la, ha + 1, 24)})
        rng.shuffle(cands)
        for p in cands:
            if not la <= p <= ha:
                continue
            if goal[0] == "code":
                for rr in goal[2]:
                    m, wrapped = step(p, goal[1], rr)
                    if lb <= m <= hb and not wrapped:
                        return p, (goal[1], rr)
            elif goal[0] == "target":
                if lb <= goal[1] <= hb and p != goal[1]:
                    return p, goal[1]
            else:
                for k in range(16, 0, -1):
                    for rr in (scale - 1, 0):
                        m, wrapped = step(p, goal[1] * k, rr if r else 0)
                        if wrapped == goal[1] and lb <= m <= hb:
                            return p, (goal[1] * k, rr if r else 0)
        return None

    rows = [y for y in range(MBH) if y != RESET_ROW]
    slots = {(y, c): [None, None] for y in rows for c in range(0, MBW, 2) if (y, c) != (RESET_ROW + 1, 0)}
    for comp in (0, 1):
        for g in goals(comp):
            order = list(slots)
            rng.shuffle(order)
            for (y, c) in order:
                if slots[(y, c)][comp] is not None:
                    continue
                got = place(comp, g, c, c + 1) if comp == 0 else place(comp, g, y, y)
                if got:
                    slots[(y, c)][comp] = got
                    break
            else:
                # a code whose un-wrapped step does not fit may still be reachable through a wrap (small f_code)
                if g[0] == "code":
                    for (y, c) in order:
                        if slots[(y, c)][comp] is None:
                            la, ha = _allowed(comp, c if comp == 0 else y, u)
                            lb, hb = _allowed(comp, c + 1 if comp == 0 else y, u)
                            for p in range(max(la, lo_m), min(ha, hi_m) + 1):
                                m, _ = step(p, g[1], g[2][0])
                                if max(lb, lo_m) <= m <= min(hb, hi_m):
                                    slots[(y, c)][comp] = (p, (g[1], g[2][0]))
                                    break
                            if slots[(y, c)][comp]:
                                break
                    else:
                        raise AssertionError(f"no place for {g} comp {comp} f_code {f_code} full_pel {full_pel}")
                else:
                    raise AssertionError(f"no place for {g} comp {comp} f_code {f_code} full_pel {full_pel}")

    for y in range(MBH):
        w.slice(y, 8)
        if y == RESET_ROW:
            _reset_row(w, y, u, lo_m, hi_m)
            continue
        for c in range(0, MBW, 2):
            if (y, c) == (RESET_ROW + 1, 0):   # behind the reset by the slice header: a small delta
                w.mb(codes=((1, 0), (1, 0)))
                w.mb(mv=(0, 0))
                continue
            first, second = [], []
            for comp in (0, 1):
                s = slots[(y, c)][comp]
                if s is None:
                    first.append(w.encode_target(comp, 0))
                    second.append(None)
                else:
                    first.append(w.encode_target(comp, s[0]))
                    second.append(s[1])
            w.mb(codes=first)
            codes2 = []
            for comp in (0, 1):
                t = second[comp]
                codes2.append(w.encode_target(comp, 0) if t is None else (t if isinstance(t, tuple) else w.encode_target(comp, t)))
            w.mb(codes=codes2)


def _reset_row(w, y, u, lo_m, hi_m):
    """A large predictor, then each reset of the predictor (player.cpp:1300 and motion_vectors(false)): a skipped macroblock,
    an intra one, a pattern-only one, a new slice -- and a small coded delta behind each.  A decoder that misses the reset
    lands far off."""
    def big(col):
        lo, hi = _allowed(0, col, u)
        lv, hv = _allowed(1, y, u)
        h = min(hi, hi_m) if col < MBW // 2 else max(lo, lo_m)
        v = min(hv, hi_m) if col % 2 else max(lv, lo_m)
        return h * u, v * u

    col = 0
    for kind in ("skipped", "intra", "pattern", "skipped", "intra", "pattern"):
        w.mb(inc=1, mv=big(col))
        col += 1
        if kind == "skipped":
            w.mb(inc=2, codes=((1, 0), (-1, 0)))
            col += 2
        elif kind == "intra":
            w.mb(type=T_INTRA, dc=[3, 0, 0, 0, -3, 3])
            w.mb(codes=((-1, 0), (1, 0)))
            col += 2
        else:
            w.mb(type=T_PATTERN, cbp=33, blocks=[[(0, 2)], [(1, -1)]])
            w.mb(codes=((1, 0), (1, 0)))
            col += 2
    while col < MBW - 1:
        w.mb(mv=(0, 0))
        col += 1
    w.mb(mv=big(col))   # ... and the next row's slice header resets it: that row's first delta is small


def vectors():
    out = []
    for full_pel in (0, 1):
        w = Writer(f"vectors_fp{full_pel}")
        rng = np.random.default_rng(20 + full_pel)
        for f_code in range(1, 8):
            _vector_picture(w, f_code, full_pel, rng)
        out.append(w.done())
    w = Writer("vectors_changing")   # f_code and full_pel change on every P picture
    rng = np.random.default_rng(29)
    for f_code, full_pel in ((1, 0), (7, 0), (2, 1), (4, 0)):
        _vector_picture(w, f_code, full_pel, rng)
    out.append(w.done())
    return out


# ---- family: windows ------------------------------------------------------------------------------------------------------
def _window_vector(k, xb, yb, x, y, rng):
    """Chroma alignment k = 0 ... 127: (X >> 1) & 7 = k & 7 and (Y >> 1) & 15 = k >> 3; luma half-pel bits xb, yb; the free high
    part of the vector at random inside the picture."""
    X0, Y0 = 32 * x, 32 * y
    hs = [h for h in range(-64, 64) if ((X0 + h) >> 1) & 7 == k & 7 and (X0 + h) & 1 == xb and 0 <= X0 + h <= X_MAX]
    vs = [v for v in range(-64, 64) if ((Y0 + v) >> 1) & 15 == k >> 3 and (Y0 + v) & 1 == yb and 0 <= Y0 + v <= Y_MAX]
    return int(rng.choice(hs)), int(rng.choice(vs))


def _alignment_pictures(w, rng, outside_every=0):
    """Four motion-only pictures (vectors of -64 ... 63 half-pels): picture (xb, yb) runs every macroblock through the 128
    chroma alignments at those luma half-pel bits.  outside_every = 8: one macroblock in eight points outside instead, just
    beyond an edge the f_code (6 then: -512 ... 511) lets it reach."""
    n = 0
    for xb, yb in ((0, 0), (1, 0), (0, 1), (1, 1)):
        w.picture(f_code=6 if outside_every else 3)
        for y in range(MBH):
            w.slice(y, 8)
            for x in range(MBW):
                k = (n * 37 + 11) % 128   # 37 is odd: 264 macroblocks pass every residue of 128 twice
                n += 1
                mv = _window_vector(k, xb, yb, x, y, rng)
                if outside_every and (n - 1) % outside_every == ((n - 1) // outside_every * 3) % outside_every:   # (its place in the eight moves)
                    far = int(rng.integers(1, 40))
                    opts = [(mv[0], -far - 32 * y), (mv[0], Y_MAX + far - 32 * y)]
                    if 32 * x + far <= 512:
                        opts.append((-far - 32 * x, mv[1]))
                    if X_MAX + far - 32 * x <= 511:
                        opts.append((X_MAX + far - 32 * x, mv[1]))
                    mv = opts[(n // outside_every) % len(opts)]
                w.mb(mv=mv)


def _flush_picture(w, rng, variant):
    """Windows flush with the picture's edges and corners: the macroblocks of the two outer columns / rows point at the
    half-pel positions 0 ... 3 (left, top: luma is flush at 0 and 1, without and with a half-pel step; chroma, at half the
    position, at 0 / 1 and 2 / 3) or 670 ... 672, 350 ... 352 (right, bottom: the last positions with a half-pel step, and the
    last without one).  The four macroblocks of a corner take every pair of these over the four variants."""
    lo, hi_x, hi_y = [0, 1, 2, 3], [X_MAX - 1, X_MAX, X_MAX + 1], [Y_MAX - 1, Y_MAX, Y_MAX + 1]
    w.picture(f_code=3)
    for y in range(MBH):
        w.slice(y, 8)
        for x in range(MBW):
            xo = lo if x < 2 else (hi_x if x >= MBW - 2 else None)
            yo = lo if y < 2 else (hi_y if y >= MBH - 2 else None)
            k = y * MBW + x + variant
            h, v = _window_vector(int(rng.integers(0, 128)), k & 1, (k >> 1) & 1, x, y, rng)
            if xo and yo:
                j = variant * 4 + (y & 1) * 2 + (x & 1)
                X, Y = xo[j % len(xo)], yo[(j // len(xo)) % len(yo)]
                h, v = X - 32 * x, Y - 32 * y
            elif xo:
                h = xo[k % len(xo)] - 32 * x
            elif yo:
                v = yo[k % len(yo)] - 32 * y
            w.mb(mv=(h, v))


def windows():
    w = Writer("windows_align")
    _alignment_pictures(w, np.random.default_rng(31))
    a = w.done()
    w = Writer("windows_flush")
    rng = np.random.default_rng(32)
    for variant in range(4):
        _flush_picture(w, rng, variant)
    return [a, w.done()]


# ---- family: outside ------------------------------------------------------------------------------------------------------
def outside():
    """Vectors that leave the picture.  The reference reads outside its frame there (undefined); the oracle clamps."""
    out = []
    rng = np.random.default_rng(41)
    w = Writer("outside_near_far")
    # picture 1: one half-pel beyond each edge, and beyond each corner, from the border macroblocks (f_code 1)
    w.picture(f_code=1)
    for y in range(MBH):
        w.slice(y, 8)
        for x in range(MBW):
            h = -1 if x == 0 else (X_MAX + 2 - 32 * x if x == MBW - 1 else 0)
            v = -1 if y == 0 else (Y_MAX + 2 - 32 * y if y == MBH - 1 else 0)
            if (x + y) % 3 == 0 and 0 < x < MBW - 1 and 0 < y < MBH - 1:
                h, v = int(rng.integers(-8, 8)), int(rng.integers(-8, 8))
            w.mb(mv=(h, v))
    # pictures 2 / 3: far beyond, every motion code with every kind of residual at f_code 7, without and with full_pel
    # (-2048 ... 2046 half-pels)
    for full_pel in (0, 1):
        w.picture(f_code=7, full_pel=full_pel)
        n = 0
        for y in range(MBH):
            w.slice(y, 8)
            for x in range(MBW):
                ch = (n % 33) - 16
                cv = ((n * 7 + 3) % 33) - 16
                res = [0, 63, 21, 42][(n // 33) % 4]
                if n == 40:
                    w.mb(mv=(-1024 * (1 + full_pel), -1024 * (1 + full_pel)))
                elif n == 41:
                    w.mb(mv=(1023 * (1 + full_pel), 1023 * (1 + full_pel)))
                else:
                    w.mb(codes=((ch, res), (cv, 63 - res)))
                n += 1
    # picture 4: beyond the corners by more than a macroblock (f_code 4: -128 ... 127), small vectors elsewhere
    w.picture(f_code=4)
    for y in range(MBH):
        w.slice(y, 8)
        for x in range(MBW):
            side_x = -1 if x < 3 else (1 if x >= MBW - 3 else 0)
            side_y = -1 if y < 3 else (1 if y >= MBH - 3 else 0)
            if side_x and side_y:
                w.mb(mv=(100 * side_x, 100 * side_y))
            elif side_x or side_y:
                w.mb(mv=(0, 0))
            else:
                w.mb(mv=(int(rng.integers(-20, 20)), int(rng.integers(-20, 20))))
    out.append(w.done())
    w = Writer("outside_one_in_eight")
    _alignment_pictures(w, np.random.default_rng(43), outside_every=8)
    out.append(w.done())
    return out


# ---- the IDCT in integers (families coefs and range, and their tests) -----------------------------------------------------
OPERANDS = ("i1 - i7", "i5 - i3", "(i1 + i7) - (i3 + i5)", "i2 - i6")   # what one pass multiplies (by 473 / 196, 362, 362)


def idct_pass(x, exact=False):
    """One 8-point pass of the reference's scaled integer IDCT (player.cpp:938-995) along axis 0 of an integer array; returns
    (the eight outputs, the four multiplied operands in the order of OPERANDS).  exact: the same linear map in floating
    point without the rounding shifts -- what the sign patterns and the L1 bounds are computed from."""
    i0, i1, i2, i3, i4, i5, i6, i7 = x
    r = (lambda p: p / 256.0) if exact else (lambda p: (p + 128) >> 8)
    b1, b3, b4, t1, t2, b6 = i4, i2 + i6, i5 - i3, i1 + i7, i3 + i5, i1 - i7
    b7 = t1 + t2
    x4 = r(b6 * 473 - b4 * 196) - b7
    x0 = x4 - r((t1 - t2) * 362)
    x1, x2, x3 = i0 - b1, r((i2 - i6) * 362) - b3, i0 + b1
    y3, y4, y5, y6 = x1 + x2, x3 + b3, x1 - x2, x3 - b3
    y7 = -x0 - r(b4 * 473 + b6 * 196)
    return (np.stack([b7 + y4, x4 + y3, y5 - x0, y6 - y7, y6 + y7, x0 + y5, y3 - x4, y4 - b7]),
            np.stack([b6, b4, t1 - t2, i2 - i6]))


def idct_block(b, exact=False):
    """b[row, column, ...]: pre-multiplied coefficients (an intra DC as value << 8).  Returns (residual[row, column, ...],
    column-pass operands [operand, column, ...], row-pass operands [operand, row, ...])."""
    b = np.asarray(b, dtype=np.float64 if exact else np.int64)
    c, col_ops = idct_pass(b, exact)
    r, row_ops = idct_pass(np.swapaxes(c, 0, 1), exact)
    r = np.swapaxes(r, 0, 1)
    return (r / 256.0 if exact else (r + 128) >> 8), col_ops, row_ops


def block_values(entries, q, matrix, intra):
    """[(scan position, level)] of a manifest -> the 8 x 8 pre-multiplied block idct_block() takes."""
    b = np.zeros(64, dtype=np.int64)
    for k, (n, level) in enumerate(entries):
        zz = ZIGZAG[n]
        b[zz] = level << 8 if (intra and k == 0) else dequant(level, q, matrix[n], intra) * PREMUL[zz >> 3][zz & 7]
    return b.reshape(8, 8)


@functools.lru_cache(maxsize=None)
def idct_weights():
    """The linear maps from the 64 dequantised coefficients (raster) to the operands and residuals: (column-pass operands
    [4, 8, 64], row-pass operands [4, 8, 64], residual [8, 8, 64])."""
    basis = np.zeros((8, 8, 64))
    for k in range(64):
        basis[k >> 3, k & 7, k] = PREMUL[k >> 3][k & 7]
    res, col, row = idct_block(basis, exact=True)
    return col, row, res


def sign_pattern(weights, negate=False, ac_only=False):
    """64 levels in scan order, +-255 (at quantiser 31 both saturate: +2047 / -2048), that drive sum(weights x coefficient) as
    far up (down with negate) as it goes; ac_only leaves scan position 0 out (an intra block's DC)."""
    out = []
    for n in range(1 if ac_only else 0, 64):
        up = weights[ZIGZAG[n]] >= 0
        out.append((0, 255 if up != negate else -255, "long"))
    return out


@functools.lru_cache(maxsize=None)
def range_patterns():
    """[(name, weights[64] by raster position)]: per pass and multiplied operand the line (column / row) whose L1 norm is
    the largest, then the residuals of pixels (0, 0), (7, 7) and (3, 5)."""
    col, row, res = idct_weights()
    out = []
    for tag, w in (("column", col), ("row", row)):
        for op in range(4):
            line = int(np.argmax(np.abs(w[op]).sum(axis=1)))
            out.append((f"{tag} pass {OPERANDS[op]} of line {line}", w[op, line], (tag, op, line)))
    for y, x in ((0, 0), (7, 7), (3, 5)):
        out.append((f"residual of pixel ({y}, {x})", res[y, x], ("pixel", y, x)))
    return out


def recon_order(mb, blk):
    """Where k_recon's block order (by macroblock row; inside it the 44 upper luminance blocks, the 44 lower ones, 22 Cr,
    22 Cb) puts a block: wave = the result // 64."""
    y, x = divmod(mb, MBW)
    rr = 44 * (blk >> 1) + 2 * x + (blk & 1) if blk < 4 else 88 + 22 * (blk - 4) + x
    return 132 * y + rr


# ---- family: coefs --------------------------------------------------------------------------------------------------------
CUSTOM_INTRA = [8 + 3 * i for i in range(64)]          # as sent: 64 distinct entries, the first 8
CUSTOM_NON_INTRA = [255 - 3 * i for i in range(64)]    # 255 ... 66


def _flat_intra_picture(w, q, value=lambda x, y: 128):
    """An I picture of DC-only blocks: every pixel of macroblock (x, y) is value(x, y)."""
    w.picture(intra=True)
    for y in range(MBH):
        w.slice(y, q)
        for x in range(MBW):
            v = value(x, y)
            w.mb(type=T_INTRA, dc=[v - w.dc[0], 0, 0, 0, v - w.dc[1], v - w.dc[2]])


def _position_pictures(w, rng):
    """A P picture whose 1584 blocks hold one coefficient each, block j at scan position j % 64 (position 0: the "n == 1"
    shortcut), the sign changing every 64 blocks; then an I picture whose macroblock k holds, in each block, the DC and one
    coefficient at scan position k % 63 + 1, with either sign, beside DC differentials of zero and not.  Level 1 at quantiser
    16: 3 x the non-intra entry (at most 765), 2 x the intra entry (at most 394)."""
    w.picture(f_code=2)
    j = 0
    for y in range(MBH):
        w.slice(y, 16)
        for x in range(MBW):
            blocks = []
            for _ in range(6):
                n, s = j % 64, 1 if (j // 64) % 2 == 0 else -1
                blocks.append([_level(n, s)])
                j += 1
            inner = 0 < x < MBW - 1 and 0 < y < MBH - 1
            if (x + y) % 2 and inner:
                w.mb(type=T_FORWARD | T_PATTERN, mv=(int(rng.integers(-6, 7)), int(rng.integers(-6, 7))), cbp=63, blocks=blocks)
            else:
                w.mb(type=T_PATTERN, cbp=63, blocks=blocks)
    w.picture(intra=True)
    for y in range(MBH):
        w.slice(y, 16)
        for x in range(MBW):
            k = y * MBW + x
            n, variant = k % 63 + 1, k // 63
            dc = [0 if (k + b) % 3 == 0 else int(rng.integers(-9, 10)) for b in range(6)]
            dc = [d if 16 <= w.dc[0 if b < 4 else b - 3] + 4 * d <= 232 else 0 for b, d in enumerate(dc)]
            blocks = []
            for b in range(6):
                s = 1 if (b + variant) % 2 == 0 else -1
                blocks.append([_level(n - 1, s)])
            w.mb(type=T_INTRA, dc=dc, blocks=blocks)


def _coefs_positions():
    w = Writer("coefs_positions")
    _position_pictures(w, np.random.default_rng(51))
    return w.done()


def _coefs_matrices():
    """The pictures of coefs_positions under loaded matrices, then again behind a sequence header that loads none."""
    w = Writer("coefs_matrices")
    rng = np.random.default_rng(51)
    w.sequence(CUSTOM_INTRA, CUSTOM_NON_INTRA)
    _position_pictures(w, rng)
    w.sequence()
    _position_pictures(w, rng)
    return w.done()


# (level, quantiser) pairs of coefs_rounding per non-intra entry at scan position 0; the product is (2 level +- 1) q m
ROUNDING = {
    3: [(227, 24), (237, 23), (188, 29), (-227, 24), (-237, 23), (-188, 29),        # 2047.5, 2048.4, 2049.9 and their negatives
        (5, 16), (-5, 16), (7, 31), (-7, 31), (13, 9), (-13, 9)],                    # 33 exactly, 87.2, 45.6 -> 45
    255: [(-256, 31), (255, 31), (40, 20), (-40, 20), (1, 1), (-1, 1)],             # the largest product; far beyond; 47.8
    16: [(1, 16), (-1, 16), (3, 16), (-3, 16), (2, 7), (-2, 7), (1, 11), (-1, 11),  # 3, 7 exactly; 35; 33 / 16 = 2 -> 1
         (4, 5), (-4, 5), (100, 3), (-100, 3), (127, 31), (-128, 31)],               # 45 / 16 = 2 -> 1; 603; beyond
}


def _level(run, level):
    form = "vlc" if (run, abs(level)) in books()["dct"] or (run, abs(level)) == (0, 1) else ("short" if abs(level) <= 127 else "long")
    return (run, level, form)


def _coefs_rounding():
    """Non-intra blocks whose only coefficient stands at scan position 0 (the "n == 1" shortcut: residual floor(v / 8)) and the
    same coefficient beside +-1 at scan position 1 (the IDCT path), on a flat prediction of 128 (an I picture written here;
    every P picture uses a macroblock row that the pictures before it only copied).
    One P picture per non-intra matrix entry at scan position 0: 3 and 255 (loaded; the first header loads the non-intra
    matrix alone) and the default 16.  Then coded levels of 0: behind a non-intra coefficient, and in intra blocks behind
    a coefficient chosen, with the integer IDCT above, so that the 1 a coded 0 dequantises to changes a pixel."""
    w = Writer("coefs_rounding")
    _flat_intra_picture(w, 8)
    w.pred_range = (128, 128)
    for row, (m, cases) in zip((1, 3, 5), ROUNDING.items()):   # (a row of its own each: what it predicts from is still 128)
        if m == 16:
            w.sequence()
        else:
            w.sequence(None if m == 3 else [8] + [255 - i for i in range(1, 64)], [m] + [16] * 63)
        w.picture(f_code=1)
        for y in range(MBH):
            w.slice(y, 8)
            for x in range(MBW):
                if y != row or not 1 <= x <= len(cases):
                    w.mb(mv=(0, 0))
                    continue
                level, q = cases[x - 1]
                one = [_level(0, level)]
                w.mb(type=T_PATTERN, cbp=63, quant=q,
                     blocks=[one, one + [(0, 1)], one, one + [(0, -1)], one, one + [(0, 1 if x % 4 < 2 else -1)]])
    # coded zeros: non-intra, under the default matrix (quantiser 31: (0 + 1) x 31 x 16 / 16 = 31)
    w.picture(f_code=1)
    for y in range(MBH):
        w.slice(y, 31)
        for x in range(MBW):
            if y == 7 and 0 < x < 8:
                w.mb(type=T_PATTERN, cbp=63, blocks=[[(0, 1), (x, 0, "long")], [(x, -1), (0, 0, "long")], [(0, 2), (62, 0, "long")],
                                                       [(1, 1), (1, 0, "long"), (0, 0, "long")], [(0, 1), (x, 0, "long")], [(3, -1), (5 * x, 0, "long")]])
            else:
                w.mb(mv=(0, 0))
    # ... and intra: a coded 0 becomes the coefficient 1, 62 at most after the pre-multiplier, which no pixel shows unless
    # another coefficient has brought one to the edge of a rounding step
    w.picture(intra=True)
    def shows(level, pos):
        with_zero = [(0, 128), (1, level), (pos, 0)]
        return not np.array_equal(idct_block(block_values(with_zero, 8, w.intra_m, True))[0],
                                  idct_block(block_values(with_zero[:2], 8, w.intra_m, True))[0])
    for y in range(MBH):
        w.slice(y, 8)
        for x in range(MBW):
            if y != 9 or not 0 < x < 8:
                w.mb(type=T_INTRA)
                continue
            blocks = []
            for b in range(6):
                pos = (4, 7, 12, 4, 12, 7)[b]   # raster (1, 1), (1, 2), (2, 2)
                level = next(l for l in range(x + b, 51) if shows(l, pos))   # (16 level <= 800: inside the domain)
                blocks.append([_level(0, level if b % 2 else -level), (pos - 2, 0, "long")])
            w.mb(type=T_INTRA, blocks=blocks)
    return w.done()


def dense_kind(b, y):
    """What block b (k_recon's order) of macroblock row y holds in coefs_dense: "full" (all 64 scan positions), "empty" (an
    intra block: its DC alone), "dc" (one entry at scan position 0), "one" (one entry elsewhere)."""
    if y < 2:
        return "full"
    if y < 4:
        return "full" if b % 2 == 0 else "empty"
    if y < 6:
        return ("full", "dc", "one")[b % 3]
    if y < 8:
        return "full" if b % 63 == 0 else "empty"
    if y < 10:
        return "full" if b % 65 == 0 else ("empty" if b % 2 else "one")
    return "empty"


def _coefs_dense():
    """Two macroblock rows in which every block codes all 64 scan positions with +-1 ("1s" / "11s", quantiser 1: sum 192) -- a
    wave of k_recon then holds 64 x 64 entries -- then rows in which full blocks alternate with empty ones, DC-only ones
    and one-entry ones (levels of 8 ... 30, to be seen at quantiser 1) in periods 2, 3, 63 and 65 of k_recon's block order; as
    a P picture and as an I picture."""
    w = Writer("coefs_dense")
    rng = np.random.default_rng(53)
    full = lambda first: [(0, int(s)) for s in rng.choice([-1, 1], 64 - first)]
    for intra in (False, True):
        w.picture(f_code=1, intra=intra)
        for y in range(MBH):
            w.slice(y, 1)
            for x in range(MBW):
                blocks, cbp = [], 0
                for blk in range(6):
                    b = recon_order(y * MBW + x, blk)
                    kind = dense_kind(b, y)
                    if intra:
                        blocks.append({"full": full(1), "empty": [], "dc": [], "one": [_level(b % 63, (20 + b % 11) * (1 - 2 * (b % 2)))]}[kind])
                    elif kind != "empty":
                        cbp |= 0x20 >> blk
                        blocks.append({"full": full(0), "dc": [_level(0, (8 + b % 9) * (1 - 2 * (b % 2)))],
                                   "one": [_level(b % 63 + 1, (20 + b % 11) * (1 - 2 * (b % 2)))]}[kind])
                if intra:
                    w.mb(type=T_INTRA, blocks=blocks, dc=[int(d) for d in rng.integers(-2, 3, 6)])
                elif cbp:
                    w.mb(type=T_PATTERN, cbp=cbp, blocks=blocks)
                else:
                    w.mb(mv=(0, 0))
    return w.done()


def coefs():
    return [_coefs_positions(), _coefs_matrices(), _coefs_rounding(), _coefs_dense()]


# ---- family: range --------------------------------------------------------------------------------------------------------
def _range_idct():
    """Every AC coefficient saturated (level +-255 at quantiser 31), in the sign patterns of range_patterns() and their
    negations: non-intra (scan position 0 saturated too) on predictions of 0 and of 248, then intra."""
    w = Writer("range_idct", domain=False)
    _flat_intra_picture(w, 31, lambda x, y: 0 if x < MBW // 2 else 248)
    pats = [(w_, neg) for _, w_, _ in range_patterns() for neg in (False, True)]
    groups = [pats[i:i + 6] for i in range(0, len(pats), 6)]
    groups[-1] += pats[:6 - len(groups[-1])]
    w.picture(f_code=1)
    for y in range(MBH):
        w.slice(y, 31)
        for x in range(MBW):
            g = x if x < MBW // 2 else x - MBW // 2
            if y == 0 and g < len(groups):
                w.mb(type=T_PATTERN, cbp=63, blocks=[sign_pattern(w_, neg) for w_, neg in groups[g]])
            else:
                w.mb(mv=(0, 0))
    w.picture(intra=True)
    for y in range(MBH):
        w.slice(y, 31)
        for x in range(MBW):
            if y == 0 and x < len(groups):
                w.mb(type=T_INTRA, blocks=[sign_pattern(w_, neg, ac_only=True) for w_, neg in groups[x]])
            else:
                w.mb(type=T_INTRA)
    return w.done()


DC_TARGETS = [-1, -255, 256, 511, 4660, -4660, 18500, -18500, 32767, -32767, 32768, -32768, 40000, -40000]
DC_PATTERN_FROM = 18500


def max_ac_residual():
    """(pixel weights, y, x) of the pixel, among those range_idct aims at, whose AC-only residual goes furthest."""
    best = max((p for p in range_patterns() if p[2][0] == "pixel"), key=lambda p: np.abs(p[1][1:]).sum())
    return best[1], best[2][1], best[2][2]


def _dc_walk(targets, back_to=100, start=128):
    """[(differential, coefficients)] of one DC predictor from `start`: in steps of +-255 to each target in turn; there a DC-only
    block, blocks with +1 and with -1 at scan position 1 and, from +-18 500 outward, a block whose AC coefficients carry
    the residual further the same way; at last back to `back_to`, and small steps there."""
    seq, cur = [], start
    def go(v):
        nonlocal cur
        while True:
            d = max(-255, min(255, v - cur))
            seq.append((d, []))
            cur += d
            if cur == v:
                return
    for v in targets:
        go(v)
        seq.append((0, [(0, 1)]))
        seq.append((0, [(0, -1)]))
        if abs(v) >= DC_PATTERN_FROM:
            seq.append((0, sign_pattern(max_ac_residual()[0], negate=v < 0, ac_only=True)))
    if back_to is not None:
        go(back_to)
        seq += [(0, []), (7, []), (0, [(0, 1)]), (-7, [])]
    return seq


def _range_dc():
    """I pictures of one slice each (quantiser 31).  Picture 1 walks the luminance predictor: up through the positive
    targets to 40 000, back into 0 ... 255, down through the negative ones, back.  A macroblock holds one block of each
    chrominance predictor, so a picture's 264 reach +-33 660 and back at the most: picture 2 takes Cr up and Cb down to
    +-18 500 and back, picture 3 on to +-40 000 (the picture ends out there); pictures 4 and 5 likewise with Cr down, Cb up."""
    w = Writer("range_dc", domain=False)
    pos, neg = [v for v in DC_TARGETS if v > 0], [v for v in DC_TARGETS if v < 0]
    near = lambda t: [v for v in t if abs(v) <= DC_PATTERN_FROM]
    far = lambda t: [v for v in t if abs(v) > DC_PATTERN_FROM]
    luma = _dc_walk(pos) + _dc_walk(neg, start=100)
    plans = [(luma, None, None), (None, _dc_walk(near(pos)), _dc_walk(near(neg))), (None, _dc_walk(far(pos), None), _dc_walk(far(neg), None)),
             (None, _dc_walk(near(neg)), _dc_walk(near(pos))), (None, _dc_walk(far(neg), None), _dc_walk(far(pos), None))]
    for y_seq, cr_seq, cb_seq in plans:
        y_seq, cr_seq, cb_seq = list(y_seq or []), list(cr_seq or []), list(cb_seq or [])
        assert len(y_seq) <= 4 * MBW * MBH and len(cr_seq) <= MBW * MBH and len(cb_seq) <= MBW * MBH
        w.picture(intra=True)
        w.slice(0, 31)
        for _ in range(MBW * MBH):
            blks = [y_seq.pop(0) if y_seq else (0, []) for _ in range(4)] + [cr_seq.pop(0) if cr_seq else (0, [])] + \
                   [cb_seq.pop(0) if cb_seq else (0, [])]
            w.mb(type=T_INTRA, dc=[d for d, _ in blks], blocks=[c for _, c in blks])
    return w.done()


def range_():
    return [_range_idct(), _range_dc()]


BUILDERS = {"coefs_positions": _coefs_positions, "coefs_matrices": _coefs_matrices, "coefs_rounding": _coefs_rounding,
            "coefs_dense": _coefs_dense, "range_idct": _range_idct, "range_dc": _range_dc}


def rebuild(name, change):
    """Stream `name` of coefs / range written again with one coefficient changed: change = (picture, macroblock address,
    block, index into the block's coefficient list, "sign" / "move").  Everything else keeps its bytes."""
    global mutation
    mutation = (name,) + tuple(change)
    try:
        return BUILDERS[name]()
    finally:
        mutation = None


FAMILIES = {"codes": codes, "vectors": vectors, "windows": windows, "outside": outside, "coefs": coefs, "range": range_}


@functools.lru_cache(maxsize=None)
def family(name):
    return FAMILIES[name]()


def all_streams(names=tuple(FAMILIES)):
    return [s for n in names for s in family(n)]
