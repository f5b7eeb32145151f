"""Directed MPEG-1 video streams, written bit by bit (test input only).

The generator (espflix_amd/gen) is a good workload and a narrow sample of the syntax: forward_f_code 1 or 2, vectors of a
few pels, and whichever VLC codes its content happens to need.  The four families here reach the rest on purpose:

  codes()    every entry of every code book (address increments and escapes, macroblock types, patterns, motion codes,
             DCT run / level pairs in both positions and signs, escapes, dct_dc_size, quantiser scales)
  vectors()  one P picture per forward_f_code 1 ... 7 x full_pel 0 / 1: every motion code the picture's geometry can
             reach, the residuals 0, 2^r - 1 and one between, the ends of the range, wraps, predictor resets
  windows()  every alignment of k_recon's 9 x 9 window fetch, and windows flush with every edge and corner
  outside()  vectors that leave the picture -- undefined in the reference (it reads outside its frame buffers), defined
             by the oracle as a clamp of the coordinates; compared with the oracle only

Every stream starts with the sequence header, GOP header and I picture of gen.Batch(0, 1, 1, 12, 0) (as
common.stuffing_es does); what follows is written here.  A family returns a list of Stream: the elementary stream and a
manifest of what the writer MEANT -- per hand-written picture its type, f_code and full_pel, per macroblock its address,
type, vector in half-pels, pattern and quantiser -- which tests/test_syntax_streams.py holds against the oracle's parse
trace.  The VLC codes come from tests/golden/codebooks.json (the reference's own books, expanded); dct_dc_size
(ISO 11172-2 tables B-5a / B-5b), which that file lacks, is written out below.

Domain condition of the reference: it clamps reconstructed pixels through a 768-entry table (index -256 ... 511), and an
intra block of one coefficient is stored without a clamp.  The writer therefore keeps the sum of |dequantised coefficient|
of a block <= 900 (no basis function of the 8 x 8 IDCT exceeds a quarter of its coefficient: residual within +-225 of a
0 ... 255 prediction) and every intra DC value within 0 ... 255, and asserts both.
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


def dequant_non_intra(level: int, q: int) -> int:
    """player.cpp:1110-1121 with the default non-intra matrix (16)."""
    v = 2 * level + (1 if level > 0 else -1)
    v = int(v * q * 16 / 16)
    if v % 2 == 0:
        v -= 1 if v > 0 else -1
    return max(-2048, min(2047, v))


class Writer:
    """Pictures, slices and macroblocks; keeps the manifest and the reference's predictors while it writes."""

    def __init__(self, name):
        self.name = name
        self.b = common._Bits()
        self.pictures = [None]
        self.pic = None
        self.tref = 0

    # ---- headers ------------------------------------------------------------------------------------------------------
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
        self.pic = dict(type=1 if intra else 2, f_code=f_code, full_pel=full_pel, mbs=[])
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
            self.pic["mbs"].append(dict(addr=self.addr, type=T_SKIPPED, mv=(0, 0), cbp=0, q=0))
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
        of the pattern a list of coefficients (run, level) / (run, level, form), form "vlc" (default), "short", "long".
        dc: for an intra macroblock six differentials (default 0)."""
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
        for blk in range(6):
            if cbp & (0x20 >> blk):
                default = [] if type & T_INTRA else [(0, 1)]   # (a coded non-intra block holds at least one coefficient)
                self.block(blk, bool(type & T_INTRA), blocks.pop(0) if blocks else default, dc[blk] if dc else 0)
        assert not blocks
        P["mbs"].append(dict(addr=self.addr, type=type, mv=vec, cbp=cbp, q=self.q))
        return vec

    # ---- block layer --------------------------------------------------------------------------------------------------
    def block(self, blk, intra, coefs, dc_diff=0):
        b = self.b
        n, total = 0, 0
        if intra:
            size = 0 if dc_diff == 0 else abs(dc_diff).bit_length()
            code = (DC_LUMA if blk < 4 else DC_CHROMA)[size]
            b.put(int(code, 2), len(code))
            if size:
                b.put(dc_diff if dc_diff > 0 else dc_diff + (1 << size) - 1, size)
            k = 0 if blk < 4 else blk - 3
            self.dc[k] += dc_diff
            assert 0 <= self.dc[k] <= 255, "intra DC leaves 0 ... 255"
            n = 1
        for c in coefs:
            run, level, form = c if len(c) == 3 else (c[0], c[1], "vlc")
            assert level != 0 and -255 <= level <= 255
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
                    assert -127 <= level <= 127
                    b.put(level & 0xFF, 8)
                elif level > 0:                                  # 00 xx
                    b.put(0, 8)
                    b.put(level, 8)
                else:                                            # 80 xx = xx - 256
                    b.put(0x80, 8)
                    b.put(level + 256, 8)
            n += run
            assert n <= 63, "coefficient beyond scan position 63"
            if intra:
                assert n in (1, 2)   # default intra matrix entry 16 at both: same arithmetic as below without the +-1
                v = int(2 * level * self.q * 16 / 16)
                total += abs(v - (1 if v > 0 else -1) if v % 2 == 0 else v)
            else:
                total += abs(dequant_non_intra(level, self.q))
            n += 1
        assert total <= 900, "block outside the reference's clamp table domain"
        b.put(*EOB)

    def done(self):
        self.b.align()
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


FAMILIES = {"codes": codes, "vectors": vectors, "windows": windows, "outside": outside}


@functools.lru_cache(maxsize=None)
def family(name):
    return FAMILIES[name]()


def all_streams(names=("codes", "vectors", "windows", "outside")):
    return [s for n in names for s in family(n)]
