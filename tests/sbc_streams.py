"""Directed SBC frames for the audio decoder's tests (k_sbc.hip): written field by field from a plain-Python bit allocation, each
stream with a manifest of what was written -- per frame, channel and subband the scale factor, the field width the writer
expects and, per block, the codes.  Test input only; tests/syntax_streams.py is the video side's counterpart.

Four families (CALLS below; a call is a set of equally long streams of one frame size, what one efx_sbc_decode takes):
  alloc    the bit allocation: every sampling frequency x allocation method x bitpool 0..128 under four geometries, the frames
           of a stream walking a fixed list of scale-factor shapes; sample bits are random, so one wrong width misplaces every
           field behind it;
  dequant  IQUANT: every code of every field width at every scale factor, as one-frame streams, as long streams (mono and
           dual channel) and behind a rejected frame (the general kernel);
  phase    wide and narrow fields at every bit phase: odd bitpools, odd frame sizes, frames whose widths are mixed, in a
           layout per bit-field reader of the frame-parallel kernels;
  range    full-scale input: scale factor 15 and constant or alternating extreme codes, which wrap the 32-bit sums of the
           synthesis filter and drive its output into the clip.
"""
import functools
import zlib

import numpy as np

# ---- the model: A2DP Appendix B 12.6.3 as the reference decoder writes it out (sbc_decoder.cpp:142-240, 263-270) --------------
OFFSET8 = ((-2, 0, 0, 0, 0, 0, 0, 1), (-3, 0, 0, 0, 0, 0, 1, 2), (-4, 0, 0, 0, 0, 0, 1, 2), (-4, 0, 0, 0, 0, 0, 1, 2))  # 16, 32, 44.1, 48 kHz


def bitneed(freq: int, alloc: int, scale) -> list:
    need = []
    for sb, s in enumerate(scale):
        if alloc:          # SNR
            need.append(s)
        elif s == 0:       # loudness
            need.append(-5)
        else:
            loud = s - OFFSET8[freq][sb]
            need.append(loud // 2 if loud > 0 else loud)
    return need


@functools.lru_cache(maxsize=None)
def allocate(freq: int, alloc: int, bitpool: int, scale: tuple) -> tuple:
    """Field widths of the eight subbands of one channel."""
    need = bitneed(freq, alloc, scale)
    bitcount, slicecount, bitslice = 0, 0, max(0, max(need)) + 1
    while True:
        bitslice -= 1
        bitcount += slicecount
        slicecount = 0
        for n in need:
            if bitslice + 1 < n < bitslice + 16:
                slicecount += 1
            elif n == bitslice + 1:
                slicecount += 2
        if bitcount + slicecount >= bitpool:
            break
        assert bitslice > -64, "a bitpool the slices never reach (above 128)"
    if bitcount + slicecount == bitpool:
        bitcount += slicecount
        bitslice -= 1
    bits = [0 if n < bitslice + 2 else min(n - bitslice, 16) for n in need]
    for sb in range(8):
        if bitcount >= bitpool:
            break
        if 2 <= bits[sb] < 16:
            bits[sb] += 1
            bitcount += 1
        elif need[sb] == bitslice + 1 and bitpool > bitcount + 1:
            bits[sb] = 2
            bitcount += 2
    for sb in range(8):
        if bitcount >= bitpool:
            break
        if bits[sb] < 16:
            bits[sb] += 1
            bitcount += 1
    return tuple(bits)


def iquant(code: int, width: int, scale: int) -> int:
    """Python integers: the left shift wrapped to int32, the division truncating toward zero."""
    n = (((code << 1) | 1) << scale) & 0xFFFFFFFF
    if n & 0x80000000:
        n -= 1 << 32
    d = (1 << width) - 1
    q = abs(n) // d
    return (-q if n < 0 else q) - (1 << scale)


@functools.lru_cache(maxsize=2)
def iquant_table(width: int) -> np.ndarray:
    """iquant() of every code of a width at every scale factor, int32 [16, 2^width]: the same steps in int64, which holds every
    intermediate value exactly (tests/test_sbc_directed.py holds each entry to iquant() itself)."""
    code, scale = np.arange(1 << width, dtype=np.int64)[None, :], np.arange(16, dtype=np.int64)[:, None]
    n = (((code << 1) | 1) << scale) & 0xFFFFFFFF
    n = np.where(n & 0x80000000, n - (1 << 32), n)
    q = np.abs(n) // ((1 << width) - 1)
    return (np.where(n < 0, -q, q) - (1 << scale)).astype(np.int32)


def frame_bytes(blocks: int, channels: int, bitpool: int) -> int:
    return 4 + channels * 4 + (blocks * channels * bitpool + 7) // 8


def seed_of(name: str) -> int:
    return zlib.crc32(name.encode())


# ---- streams and their manifests --------------------------------------------------------------------------------------------
class Stream:
    """data: frames x fb bytes.  Per frame: ok (it decodes as written; False: its sync byte is broken), freq, blocks, alloc,
    bitpool; scale and width [frame, channel, subband]; codes [frame, block, channel, subband] (blocks beyond a frame's own
    and fields of width 0 hold 0).  mode / channels hold for the whole stream."""

    def __init__(self, name, fb, mode, parts):
        self.name, self.fb, self.mode, self.channels = name, fb, mode, 1 if mode == 0 else 2
        bmax = max(p["codes"].shape[1] for p in parts)
        if len(parts) > 1:
            pad = [np.pad(p["codes"], ((0, 0), (0, bmax - p["codes"].shape[1]), (0, 0), (0, 0))) for p in parts]
            parts = [{k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "codes"}]
            parts[0]["codes"] = np.concatenate(pad)
        for k, v in parts[0].items():
            setattr(self, k, v)
        self.data = self.data.reshape(-1)
        self.frames = self.data.size // fb

    def fields(self):
        """(width, bit position from the stream's first byte) of every field written into a frame that decodes."""
        ws, ps = [], []
        for f in np.flatnonzero(self.ok):
            w = np.broadcast_to(self.width[f][None], (int(self.blocks[f]), self.channels, 8)).reshape(-1).astype(np.int64)
            pos = np.cumsum(w) - w + (int(f) * self.fb + 4 + 4 * self.channels) * 8
            ws.append(w[w > 0])
            ps.append(pos[w > 0])
        return np.concatenate(ws), np.concatenate(ps)

    def implied_lengths(self):
        """What get_samples() returns for each frame if it reads the manifest's widths: the bytes its lazy reader has fetched."""
        per_block = self.width.astype(np.int64).sum(axis=(1, 2))
        return 4 + 4 * self.channels + (self.blocks.astype(np.int64) * per_block + 7) // 8


def last_frame_samples(stream) -> np.ndarray:
    """The decoder's sb_sample[16][2][8] after a stream whose last frame decodes and whose earlier frames, if any, left
    nothing there: iquant() of the last frame's codes, zeros elsewhere."""
    f = stream.frames - 1
    blocks = int(stream.blocks[f])
    assert stream.ok[f]
    out = np.zeros((16, 2, 8), dtype=np.int32)
    for c in range(stream.channels):
        for sb in range(8):
            w = int(stream.width[f, c, sb])
            if w:
                out[:blocks, c, sb] = iquant_table(w)[int(stream.scale[f, c, sb]), stream.codes[f, :blocks, c, sb]]
    return out


class Call:
    def __init__(self, name, streams):
        self.name, self.streams = name, streams
        self.family = name.split("/")[0]
        self.fb, self.frames = streams[0].fb, streams[0].frames
        assert all(s.fb == self.fb and s.frames == self.frames for s in streams), name


def write_frames(fb, freq, blocks, mode, alloc, bitpool, scale, codes=None, rng=None, ok=True):
    """F frames of one block count: a dict of Stream's per-frame arrays.  freq / alloc / bitpool: one value or one per frame;
    scale [F, channels, 8]; codes [F, blocks, channels, 8], or random ones from rng."""
    scale = np.asarray(scale, dtype=np.uint8)
    F, ch, _ = scale.shape
    assert ch == (1 if mode == 0 else 2)
    freq, alloc, bitpool = (np.broadcast_to(np.asarray(x, dtype=np.uint8), (F,)).copy() for x in (freq, alloc, bitpool))
    width = np.empty((F, ch, 8), dtype=np.uint8)
    for f in range(F):
        for c in range(ch):
            width[f, c] = allocate(int(freq[f]), int(alloc[f]), int(bitpool[f]), tuple(scale[f, c].tolist()))
    mask = ((1 << width.astype(np.uint32)) - 1)[:, None]
    if codes is None:
        codes = rng.integers(0, 1 << 16, (F, blocks, ch, 8), dtype=np.uint32) & mask
    codes = np.asarray(codes, dtype=np.uint32)
    assert codes.shape == (F, blocks, ch, 8) and ((codes & ~mask) == 0).all(), "a code wider than its field"
    w = np.broadcast_to(width[:, None], (F, blocks, ch, 8)).reshape(F, -1).astype(np.int64)
    end = np.cumsum(w, axis=1)
    pos = end - w + (4 + 4 * ch) * 8
    assert (4 + 4 * ch + (end[:, -1] + 7) // 8 <= fb).all(), "a frame longer than the frame size"
    v = codes.reshape(F, -1).astype(np.int64) << (24 - (pos & 7) - w)   # the field inside the three bytes it can touch
    idx = np.arange(F)[:, None] * fb + (pos >> 3)
    flat = np.zeros(F * fb + 3)
    for k, sh in enumerate((16, 8, 0)):
        flat += np.bincount((idx + k).ravel(), weights=((v >> sh) & 255).ravel(), minlength=F * fb + 3)  # (fields do not overlap: a sum is an OR)
    data = flat[:F * fb].astype(np.uint8).reshape(F, fb)
    data[:, 0] = 0x9C if ok else 0x9D
    data[:, 1] = (freq << 6) | ({4: 0, 8: 1, 12: 2, 16: 3}[blocks] << 4) | (mode << 2) | (alloc << 1) | 1
    data[:, 2] = bitpool
    data[:, 3] = (np.arange(F) * 37 + 11) & 0xFF   # the CRC byte, which the reference ignores
    sf = scale.reshape(F, ch * 8)
    data[:, 4:4 + ch * 4] = (sf[:, 0::2] << 4) | sf[:, 1::2]
    return dict(data=data, ok=np.full(F, ok), freq=freq, blocks=np.full(F, blocks, dtype=np.uint8), alloc=alloc, bitpool=bitpool,
                scale=scale, width=width, codes=codes.astype(np.uint16))


def _slice(part, a, b):
    return {k: v[a:b] for k, v in part.items()}


def _broken(part):
    """The same frames with a bad sync byte: the decoder rejects them and synthesises what its state holds."""
    out = {k: v.copy() for k, v in part.items()}
    out["data"][:, 0] = 0x9D
    out["ok"][:] = False
    return out


# ---- alloc -------------------------------------------------------------------------------------------------------------------------
GEOMETRIES = {"mono16": (16, 0), "mono12": (12, 0), "dual8": (8, 1), "stereo4": (4, 2)}   # blocks, mode
BITPOOLS = range(129)


@functools.lru_cache(maxsize=None)
def alloc_shapes() -> np.ndarray:
    """[52, 8] scale factors: uniform 0..15, four ramps, one subband at 15 over zeros and the inverse, 16 seeded random."""
    sh = [[s] * 8 for s in range(16)]
    sh += [list(range(0, 16, 2)), list(range(15, 0, -2)), list(range(8, 16)), list(range(7, -1, -1))]
    for j in range(8):
        one = [15 if k == j else 0 for k in range(8)]
        sh += [one, [15 - x for x in one]]
    sh += np.random.default_rng(0x5BC).integers(0, 16, (16, 8)).tolist()
    return np.array(sh, dtype=np.uint8)


def alloc_call(geometry: str, bitpool: int) -> Call:
    blocks, mode = GEOMETRIES[geometry]
    ch = 1 if mode == 0 else 2
    shapes = alloc_shapes()
    scale = np.stack([shapes, shapes[:, ::-1]], axis=1)[:, :ch]   # the second channel takes the shape reversed
    fb = frame_bytes(blocks, ch, bitpool)
    streams = []
    for freq in range(4):
        for alloc in range(2):
            name = f"alloc/{geometry}/bp{bitpool}/f{freq}a{alloc}"
            part = write_frames(fb, freq, blocks, mode, alloc, bitpool, scale, rng=np.random.default_rng(seed_of(name)))
            streams.append(Stream(name, fb, mode, [part]))
    return Call(f"alloc/{geometry}/bp{bitpool}", streams)


# ---- dequant -----------------------------------------------------------------------------------------------------------------------
WIDTHS = range(1, 17)


@functools.lru_cache(maxsize=4)
def _dequant_parts(b: int):
    """(mono, dual): frames that hold every code of width b at every scale factor -- scale factor s in all subbands, SNR,
    bitpool 8 b, 16 blocks: 128 codes a frame (b = 1: bitpool 1 gives subband 0 one bit, 16 codes a frame)."""
    per = max(1, (1 << b) // 128)
    if b == 1:
        codes = np.zeros((1, 16, 1, 8), dtype=np.uint32)
        codes[0, :, 0, 0] = np.arange(16) & 1
    else:
        codes = (np.arange(per * 128, dtype=np.uint32) % (1 << b)).reshape(per, 16, 1, 8)
    codes = np.tile(codes, (16, 1, 1, 1))
    scale = np.repeat(np.arange(16, dtype=np.uint8), per)[:, None, None] * np.ones((1, 1, 8), dtype=np.uint8)
    bp = 1 if b == 1 else 8 * b
    mono = write_frames(frame_bytes(16, 1, bp), 3, 16, 0, 1, bp, scale, codes)
    dual = write_frames(frame_bytes(16, 2, bp), 3, 16, 1, 1, bp, np.repeat(scale, 2, axis=1), np.repeat(codes, 2, axis=2))
    for part in (mono, dual):
        want = np.zeros(8, dtype=np.uint8)
        want[:1 if b == 1 else 8] = b
        assert (part["width"] == want).all(), b
    return mono, dual


def dequant_samples(b: int) -> np.ndarray:
    """last_frame_samples() of every stream of the `one` and `gen` layouts at once: int32 [stream, 16, 2, 8]."""
    mono, _ = _dequant_parts(b)
    out = np.zeros((mono["data"].shape[0], 16, 2, 8), dtype=np.int32)
    x = iquant_table(b)[mono["scale"][:, None, 0, :].astype(np.int64), mono["codes"][:, :, 0, :].astype(np.int64)]
    out[:, :, 0, :] = np.where(mono["width"][:, None, 0, :] > 0, x, 0)
    return out


DEQUANT_LAYOUTS = ("one", "gen", "long_mono", "long_dual")


def dequant_call(layout: str, b: int) -> Call:
    """one: every frame a stream of its own.  gen: the same behind a copy of itself with a bad sync byte -- a general stream,
    k_sbc_gen's.  long_mono / long_dual: all frames back to back in one stream."""
    mono, dual = _dequant_parts(b)
    F, name = mono["data"].shape[0], f"dequant/{layout}/b{b}"
    if layout == "one":
        streams = [Stream(f"{name}/{i}", mono["data"].shape[1], 0, [_slice(mono, i, i + 1)]) for i in range(F)]
    elif layout == "gen":
        bad = _broken(mono)
        both = {k: np.stack([bad[k], mono[k]], axis=1).reshape((2 * F,) + mono[k].shape[1:]) for k in mono}
        streams = [Stream(f"{name}/{i}", mono["data"].shape[1], 0, [_slice(both, 2 * i, 2 * i + 2)]) for i in range(F)]
    elif layout == "long_mono":
        streams = [Stream(name, mono["data"].shape[1], 0, [mono])]
    else:
        streams = [Stream(name, dual["data"].shape[1], 1, [dual])]
    return Call(name, streams)


# ---- phase -------------------------------------------------------------------------------------------------------------------------
def _phase_candidates(rng, bitpools, blocks_of, n):
    """Frames whose widths are mixed: random scale factors (SNR spreads the widths as the scale factors are spread), odd
    bitpools; kept when the allocation model gives at least four different widths."""
    out = []
    while len(out) < n:
        freq, alloc, bp = int(rng.integers(0, 4)), int(rng.integers(0, 2)), int(rng.choice(bitpools))
        scale = rng.integers(0, 16, 8)
        if len(out) % 3 == 2:   # a few loud subbands over silence: the bit left over goes to a silent one, a field of width 1
            scale[rng.integers(0, 8, int(rng.integers(3, 7)))] = 0
        scale = tuple(int(x) for x in scale)
        w = allocate(freq, alloc, bp, scale)
        # (a bitpool of 121 or more leaves widths 9..16 only, most of them 16: three different ones are a mix there)
        if len(set(w) - {0}) >= (4 if bp < 100 else 3) or (1 in w and len(set(w) - {0}) >= 2):
            out.append((freq, alloc, bp, scale, w, blocks_of(len(out))))
    return out


def _phase_stream(name, fb, frames, modulus, bitpools, blocks_of=lambda f: 16, first_bad=False):
    """A mono stream of `frames` frames of fb bytes, chosen greedily from the candidates so that the (width, bit position
    modulo `modulus`) pairs of its fields fill up.  blocks_of(frame): the frame's block count."""
    rng = np.random.default_rng(seed_of(name))
    seen = np.zeros((17, modulus), dtype=bool)
    chosen = []
    for f in range(frames):
        blocks = blocks_of(f)
        best, best_new = None, -1
        for cand in _phase_candidates(rng, bitpools(f) if callable(bitpools) else bitpools, lambda i: blocks, 24):
            w = np.tile(np.array(cand[4], dtype=np.int64), blocks)
            pos = np.cumsum(w) - w + (f * fb + 8) * 8
            new = np.zeros_like(seen)
            if not (first_bad and f == 0):
                new[w[w > 0], pos[w > 0] % modulus] = True
            gain = int((new & ~seen).sum())
            if gain > best_new:
                best, best_new, best_set = cand, gain, new
        seen |= best_set
        chosen.append(best)
    parts = []
    for f, (freq, alloc, bp, scale, _, blocks) in enumerate(chosen):
        part = write_frames(fb, freq, blocks, 0, alloc, bp, np.array(scale, dtype=np.uint8).reshape(1, 1, 8), rng=rng)
        parts.append(_broken(part) if first_bad and f == 0 else part)
    return Stream(name, fb, 0, parts)


PHASE_LAYOUTS = ("staged", "global", "gen")


@functools.lru_cache(maxsize=None)
def phase_call(layout: str) -> Call:
    """staged  small odd bitpools, 135-byte frames: the 19 frames a work item of k_sbc_par_mono reaches fit its 4 KB stage;
    global  263-byte frames (bitpool 127's, one byte of padding), 35 frames: a reach of 17 does not fit, the fields are read
            from global memory.  Every other frame has a bitpool 121..127; a frame's widths then add up to 121 or more, none
            is below 9 -- narrower fields come from the frames between them, of a smaller bitpool;
    gen     a bad sync byte in frame 0, sixteen blocks up to frame 7, twelve from frame 8: a general stream of two granules,
            both k_sbc_gen's.
    Frame sizes are odd, so a frame starts at every byte phase of a dword."""
    name = f"phase/{layout}"
    odd = lambda a, b: list(range(a | 1, b + 1, 2))
    if layout == "staged":
        streams = [_phase_stream(f"{name}/{i}", 135, 24, 32, odd(3, 63)) for i in range(3)]
    elif layout == "global":
        streams = [_phase_stream(f"{name}/{i}", 263, 35, 8, lambda f: odd(5, 119) if f & 1 else odd(121, 127)) for i in range(2)]
    else:
        streams = [_phase_stream(f"{name}/{i}", 263, 16, 8, odd(5, 127), blocks_of=lambda f: 16 if f < 8 else 12, first_bad=True)
                   for i in range(4)]
    return Call(name, streams)


# ---- range -------------------------------------------------------------------------------------------------------------------------
RANGE_CALLS = [(w, m) for w in (16, 2) for m in (0, 1)]
RANGE_FRAMES = 3   # 48 blocks: the filter's ten blocks of memory fill several times over


def range_call(width: int, mode: int) -> Call:
    """Scale factor 15 in every subband, SNR, bitpool 8 x width: every field `width` bits.  Subband j alone (the others carry
    the code next to zero) and all eight together; the extreme codes constant (both signs) and alternating from block to
    block (both phases); dual channel: the same on both channels."""
    ch = 1 if mode == 0 else 2
    top, mid = (1 << width) - 1, (1 << (width - 1)) - 1   # (2 mid + 1 = 2^width - 1: the sample is exactly 0)
    fb = frame_bytes(16, ch, 8 * width)
    scale = np.full((RANGE_FRAMES, ch, 8), 15, dtype=np.uint8)
    blk = np.arange(RANGE_FRAMES * 16)
    patterns = {"max": np.full(blk.size, top), "min": np.zeros(blk.size, dtype=np.int64), "alt": np.where(blk & 1, top, 0),
                "tla": np.where(blk & 1, 0, top)}
    todo = [(sel, pname, pat) for sel in list(range(8)) + ["all"] for pname, pat in patterns.items()]
    if width == 16:
        # Below the wrap the filter's steady answer to a constant sample x in one subband is +-2 x in most outputs (x = about
        # code - 32767 here): twelve levels across |2 x| = 0x7FFF, the lowest and the highest subband, leave outputs on
        # both sides of the clip's edge, the last unclipped values included.
        todo += [(sel, f"lvl{c}", np.full(blk.size, c)) for sel in (0, 7) for c in range(16384, 16396)]
    streams = []
    for sel, pname, pat in todo:
        codes = np.full((RANGE_FRAMES * 16, ch, 8), mid, dtype=np.uint32)
        if sel == "all":
            codes[:] = pat[:, None, None]
        else:
            codes[:, :, sel] = pat[:, None]
        name = f"range/w{width}m{mode}/sb{sel}/{pname}"
        part = write_frames(fb, 3, 16, mode, 1, 8 * width, scale, codes.reshape(RANGE_FRAMES, 16, ch, 8))
        assert (part["width"] == width).all()
        streams.append(Stream(name, fb, mode, [part]))
    return Call(f"range/w{width}m{mode}", streams)


# ---- every call, in the order of the golden file ----------------------------------------------------------------------------
def call_names(families=("alloc", "dequant", "phase", "range")):
    out = []
    if "alloc" in families:
        out += [("alloc", g, bp) for g in GEOMETRIES for bp in BITPOOLS]
    if "dequant" in families:
        out += [("dequant", lay, b) for b in WIDTHS for lay in DEQUANT_LAYOUTS]
    if "phase" in families:
        out += [("phase", lay) for lay in PHASE_LAYOUTS]
    if "range" in families:
        out += [("range", w, m) for w, m in RANGE_CALLS]
    return out


def call_name(key) -> str:
    return {"alloc": "alloc/{}/bp{}", "dequant": "dequant/{}/b{}", "phase": "phase/{}", "range": "range/w{}m{}"}[key[0]].format(*key[1:])


def make_call(key) -> Call:
    return {"alloc": alloc_call, "dequant": dequant_call, "phase": phase_call, "range": range_call}[key[0]](*key[1:])
