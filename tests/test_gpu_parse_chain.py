"""k_parse's two serial chains under load they rarely see in generator streams, hand-built with tests/syntax_streams.py's
Writer and held against the oracle, bit-exact:

  pass 1  the ring top-up: lanes that eat 28 bits per code word beside lanes whose slices hold one macroblock (consecutive
          top-ups of three and four 16-byte groups), slice payloads at every offset modulo 16, a slice that ends 1 ... 16
          bytes before the end of the batch's last stream (the zero guard), slice headers with extra_bit_slice groups;
  pass 2  the macroblock chain: dct_dc_size 0 ... 8 in both signs and quantiser changes in all-intra pictures; P pictures
          in which, on the same trip, a wave holds intra lanes, inter lanes and lanes inside skipped runs (increments 2, 33,
          34 and more, runs that reach a slice's last macroblock, predictor resets), a one-macroblock slice beside a
          264-macroblock slice; and the rare paths -- an abandoned intra block, a slice that runs on through the next start
          code -- beside ordinary lanes.

Every batch interleaves its directed streams with generator streams, so that their slices sit in the same parse waves (the
slices of one picture index lie side by side, stream after stream).  Two frame buffers, as in the reference: the last two
pictures of every stream are compared."""
import copy

import pytest

import oracle
import syntax_streams as ss
from syntax_streams import T_FORWARD, T_INTRA, T_PATTERN

pytestmark = pytest.mark.gpu

PICTURES = 4   # the generator's I picture and at most three hand-written ones


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def neighbours():
    """Generator streams and what the oracle makes of them; computed once, never changed."""
    from espflix_amd import gen
    b = gen.Batch(0, 32, PICTURES, 12, 0)
    out = []
    for k in range(32):
        es = b.es(k)
        n, h, _, _ = oracle.decode(es, 0)
        out.append((es, n, [int(x) for x in h]))
    return out


def run_batch(efx, neighbours, directed, damaged=(), last=None):
    """Decodes directed[0], generator 0, directed[1], generator 1 ... (`last`, if given, closes the batch).  Streams named in
    `damaged` are exact or flagged; every other stream is exact with status 0."""
    streams, want = [], []
    for i, s in enumerate(directed):
        es, n, h = neighbours[i % len(neighbours)]
        streams += [s.array(), es]
        want += [(s.name, None), (None, (n, h))]
    if last is not None:
        streams.append(last.array())
        want.append((last.name, None))
    assert len(streams) <= 128
    dec = efx.Decoder(max_streams=len(streams), max_pictures=PICTURES, ring_depth=2,
                      max_stream_bytes=sum(len(s) for s in streams) + 4096)
    dec.upload(streams, efx.FORMAT_ES)
    dec.decode()
    hashes = dec.frame_hashes()
    got = [(dec.stream_status(i), dec.picture_count(i),
            [int(hashes[i, dec.picture_slot(p, i)]) for p in range(max(0, dec.picture_count(i) - 2), dec.picture_count(i))])
           for i in range(len(streams))]
    dec.close()
    flagged = 0
    for i, ((name, known), (status, n, tail)) in enumerate(zip(want, got)):
        if known is None:
            on, oh, _, _ = oracle.decode(streams[i], 0)
            known = (on, [int(x) for x in oh])
        if name in damaged and status != 0:
            flagged += 1
            continue
        assert status == 0 and n == known[0], (i, name, status, n, known[0])
        assert tail == known[1][max(0, n - 2):], (i, name)
    return flagged


# ---- pieces ------------------------------------------------------------------------------------------------------------
def fat_mb(w, inc=1):
    """Pattern 63, 62 long-form escapes of level +-1 per block at quantiser 1: 28 bits per code word, 1302 bytes."""
    blocks = [[(0, 1 if (i + j) & 1 else -1, "long") for i in range(62)] for j in range(6)]
    w.mb(inc=inc, type=T_FORWARD | T_PATTERN, mv=(0, 0), cbp=63, blocks=blocks)


def slice_header(w, row, q, extra=(), zeros=0):
    """Writer.slice() with `zeros` zero bytes in front of the start code and extra_bit_slice groups in the header."""
    w.b.align()
    w.b.out += bytes(zeros)
    w.b.start_code(row + 1)
    w.b.put(q, 5)
    for info in extra:
        w.b.put(1, 1)
        w.b.put(info, 8)
    w.b.put(0, 1)
    w.q, w.addr, w.first = q, row * ss.MBW - 1, True
    w.reset()


class DcWalk:
    """Differentials of every dct_dc_size 0 ... 8 in both signs, with whatever moves keep the predictor inside 0 ... 255."""

    def __init__(self, at=0):
        self.p, self.at, self.want = 128, at, None

    def next(self):
        if self.want is None:
            size, sign = (self.at // 2) % 9, 1 if self.at % 2 == 0 else -1
            self.at += 1
            self.want = sign * (0 if size == 0 else min((1 << (size - 1)) + self.at % 3, (1 << size) - 1))
        d = self.want
        if 0 <= self.p + d <= 255:
            self.want = None
        else:
            d = (0 if d > 0 else 255) - self.p   # (a move to the end of the range from which the wanted one fits)
        self.p += d
        return d


def intra_mb(w, walks, inc=1, quant=None, ac=False):
    for k, wk in enumerate(walks):   # (the predictors as the writer holds them: 128 after a run of skipped macroblocks)
        wk.p = 128 if inc > 1 else w.dc[k]
    y, cr, cb = walks
    dc = [y.next(), y.next(), y.next(), y.next(), cr.next(), cb.next()]
    blocks = [[(0, 1)], [], [(1, -1)], [(0, 2), (0, -1)], [], [(0, -2)]] if ac else None
    w.mb(inc=inc, type=T_INTRA, quant=quant, blocks=blocks, dc=dc)


def small_vector(addr, k):
    col, row = ss.mb_xy(addr)
    if k % 3 == 0:
        return (0, 0)
    return (2, 2) if col < ss.MBW - 1 and row < ss.MBH - 1 else (-2, -2)


def inter_mb(w, addr, k, inc=1):
    """forward, pattern-only and forward + pattern macroblocks in turn"""
    kind = k % 3
    if kind == 0:
        w.mb(inc=inc, type=T_FORWARD, mv=small_vector(addr, k // 3))
    elif kind == 1:
        w.mb(inc=inc, type=T_PATTERN, cbp=[1, 32, 63, 18][k // 3 % 4], quant=(3 + k % 7) if k % 2 else None)
    else:
        w.mb(inc=inc, type=T_FORWARD | T_PATTERN, mv=small_vector(addr, k // 3 + 1), cbp=[4, 60, 33][k // 3 % 3],
             blocks=None)


def mixed_rows(w, phase, q=4, pictures=1):
    """P pictures of 12 slices: along every row intra macroblocks among forward, pattern-only and skipped ones; over the
    rows and phases an intra macroblock at every column."""
    for p in range(pictures):
        w.picture(f_code=1)
        for row in range(ss.MBH):
            w.slice(row, q)
            inc = 1
            for col in range(ss.MBW):
                kind = (col + row + phase + p) % 5
                addr = row * ss.MBW + col
                if kind in (2, 3) and 0 < col < ss.MBW - 1:   # skipped: a run of two, then a predictor reset
                    inc += 1
                    continue
                if kind == 0 or (kind == 4 and col % 2):
                    walks = (DcWalk(addr), DcWalk(addr + 5), DcWalk(addr + 11))   # (after a reset every walk starts at 128)
                    intra_mb(w, walks, inc=inc, quant=(2 + col % 9) if kind == 4 else None, ac=col % 3 == 0)
                else:
                    inter_mb(w, addr, col + row, inc=inc)
                inc = 1
    return w.done()


def whole_picture_slice(name, steps):
    """One slice of 264 macroblocks: coded macroblocks `steps` apart (2, 33, 34 and the address escape), intra ones among
    them, and a last run of skipped macroblocks that reaches the slice's last macroblock."""
    w = ss.Writer(name)
    w.picture(f_code=1)
    w.slice(0, 5)
    last = ss.MBW * ss.MBH - 1
    k, inc = 0, 1
    while True:
        addr = w.addr + inc
        if k % 2 == 0:
            intra_mb(w, (DcWalk(k), DcWalk(k + 3), DcWalk(k + 7)), inc=inc, ac=k % 4 == 0)
        else:
            inter_mb(w, addr, k, inc=inc)
        if addr == last:
            break
        inc = steps[k % len(steps)]
        k += 1
        if last - w.addr < 75:
            inc = last - w.addr   # (a run of skipped macroblocks up to the last one)
    return w.done()


def one_mb_slices(name, intra):
    w = ss.Writer(name)
    w.picture(f_code=1)
    for row in range(ss.MBH):
        w.slice(row, 6)
        if intra and row % 2 == 0:
            intra_mb(w, (DcWalk(row), DcWalk(row + 1), DcWalk(row + 2)))
        else:
            inter_mb(w, row * ss.MBW, row)
    return w.done()


# ---- pass 1 ------------------------------------------------------------------------------------------------------------
def test_consumption_extremes_in_one_wave(efx, neighbours):
    """Lanes with 1302 ... 2604 bytes of 28-bit code words beside one-macroblock slices of the same picture and the
    generator's slices."""
    directed = []
    for v in range(8):
        w = ss.Writer(f"fat{v}")
        for p in range(2):
            w.picture(f_code=1)
            for row in range(ss.MBH):
                w.slice(row, 1)
                if (row + v + p) % 4 == 0:
                    fat_mb(w)
                    if v % 2:
                        fat_mb(w)
                else:
                    w.mb(type=T_FORWARD, mv=(0, 0))
        directed.append(w.done())
    assert min(len(s.es) for s in directed) > 2 * 3 * 1302
    run_batch(efx, neighbours, directed)


def aligned_stream(z):
    w = ss.Writer(f"align{z}")
    w.picture(f_code=1)
    for row in range(ss.MBH):
        extra = [(), (0x55,), (0xFF, 0x00, 0xA7)][(row + z) % 3] if row % 4 == 1 else ()
        slice_header(w, row, 3 + row, extra=extra, zeros=z)
        for col in range(ss.MBW):
            if col == 0:
                w.mb(type=T_FORWARD, mv=(0, 0), stuffing=(z + row) % 4)
            else:
                inter_mb(w, row * ss.MBW + col, col + z)
    return w.done()


def payload_offsets(s):
    """Offsets modulo 16 of the slice payloads of the hand-written pictures, relative to the stream's first byte."""
    es, at, out = s.es, len(ss.head()), set()
    while True:
        at = es.find(b"\x00\x00\x01", at)
        if at < 0:
            return out
        if 1 <= es[at + 3] <= 0xAF:
            out.add((at + 4) % 16)
        at += 3


def test_slice_payload_at_every_offset(efx, neighbours):
    """Zero bytes in front of the start codes and macroblock stuffing move the payloads over all 16 offsets of the
    16-byte groups a top-up fetches; some headers carry one or three extra_bit_slice groups."""
    directed = [aligned_stream(z) for z in range(16)]
    # (every stream starts on a multiple of 16 bytes in the decoder's buffer)
    assert set().union(*(payload_offsets(s) for s in directed)) == set(range(16))
    run_batch(efx, neighbours, directed)


@pytest.mark.parametrize("tail", range(1, 17))
def test_slice_ends_just_before_the_end_of_the_batch(efx, neighbours, tail):
    """The last slice of the batch's last stream ends `tail` bytes before the end of the stream: what its lane reads ahead
    of that lies in the zero guard."""
    w = ss.Writer(f"tail{tail}")
    w.picture(f_code=1)
    for row in range(ss.MBH):
        w.slice(row, 4)
        if row == ss.MBH - 1:
            fat_mb(w)   # (the lane that reads furthest ahead is the one that consumes fastest)
        else:
            w.mb(type=T_FORWARD, mv=(0, 0))
    s = w.done()
    s = ss.Stream(s.name, s.es + bytes(tail), s.pictures)
    run_batch(efx, neighbours, [aligned_stream(tail % 16)], last=s)


# ---- pass 2 ------------------------------------------------------------------------------------------------------------
def test_intra_pictures_dc_sizes_and_quantiser_changes(efx, neighbours):
    directed = []
    for v in range(6):
        w = ss.Writer(f"intra{v}")
        for p in range(2):
            w.picture(intra=True)
            for row in range(ss.MBH):
                w.slice(row, 2 + (row + v) % 6)
                walks = (DcWalk(row + v), DcWalk(3 * row + v), DcWalk(5 * row + 2 * v + p))
                for col in range(ss.MBW):
                    intra_mb(w, walks, quant=(1 + (col * 7 + row) % 12) if (col + v) % 5 == 2 else None, ac=(col + row) % 3 == 0)
        directed.append(w.done())
    # every dct_dc_size in both signs is among what one walk hands out over a slice
    wk, sizes = DcWalk(0), set()
    for _ in range(4 * ss.MBW):
        d = wk.next()
        sizes.add((abs(d).bit_length(), d > 0))
    assert sizes >= {(s, sign) for s in range(1, 9) for sign in (False, True)} | {(0, False)}
    run_batch(efx, neighbours, directed)


def test_intra_inter_and_skipped_lanes_on_the_same_trip(efx, neighbours):
    directed = [mixed_rows(ss.Writer(f"mixed{v}"), v, q=3 + v, pictures=2) for v in range(5)]
    directed.append(whole_picture_slice("whole_a", [2, 1, 33, 1, 34, 2, 1, 40]))
    directed.append(one_mb_slices("single_a", intra=True))
    directed.append(whole_picture_slice("whole_b", [34, 1, 2, 67, 1, 33]))
    directed.append(one_mb_slices("single_b", intra=False))
    run_batch(efx, neighbours, directed)


# ---- the rare paths beside the common one ----------------------------------------------------------------------------------
def abandoned_block_stream():
    """Row 5 holds an intra macroblock whose first block runs beyond scan position 63 (the reference abandons the block and
    goes on with the next one, player.cpp:1106-1107)."""
    w = ss.Writer("abandoned")
    w.picture(f_code=1)
    for row in range(ss.MBH):
        w.slice(row, 4)
        for col in range(ss.MBW):
            if row == 5 and col == 3:
                w.increment(1)
                w.b.put(*ss.books()["type_p"][T_INTRA])
                w.pred = [0, 0]
                w.b.put(int(ss.DC_LUMA[0], 2), len(ss.DC_LUMA[0]))
                for _ in range(2):   # scan positions 41 and 82
                    w.b.put(*ss.ESCAPE)
                    w.b.put(40, 6)
                    w.b.put(1, 8)
                for blk in range(1, 6):
                    code = (ss.DC_LUMA if blk < 4 else ss.DC_CHROMA)[0]
                    w.b.put(int(code, 2), len(code))
                    w.b.put(*ss.EOB)
            else:
                inter_mb(w, row * ss.MBW + col, col + row)
    return w.done()


def runs_on_stream():
    """Row 7 ends in an escape whose 16 level bits are the first two bytes of the next start code: its lane runs on through
    the start code into the bytes of row 8."""
    w = ss.Writer("runs_on")
    w.picture(f_code=1)
    for row in range(ss.MBH):
        w.slice(row, 4)
        for col in range(ss.MBW - 1):
            inter_mb(w, row * ss.MBW + col, col + row)
        if row != 7:
            w.mb(type=T_FORWARD, mv=(0, 0))
            continue
        for stuffing in range(8):   # (a stuffing code has 11 bits: one of eight counts ends the escape on a byte boundary)
            t = copy.deepcopy(w)
            t.increment(1, stuffing)
            t.b.put(*ss.books()["type_p"][T_FORWARD | T_PATTERN])
            t.b.put(*ss.books()["motion"][0])
            t.b.put(*ss.books()["motion"][0])
            t.b.put(*ss.books()["cbp"][32])
            t.b.put(0b10, 2)   # run 0, level +1
            t.b.put(*ss.ESCAPE)
            t.b.put(1, 6)
            if t.b.n == 0:
                break
        assert t.b.n == 0
        w = t
    return w.done()


def test_rare_paths_beside_ordinary_lanes(efx, neighbours):
    directed = [mixed_rows(ss.Writer("mixed_l"), 1), abandoned_block_stream(), mixed_rows(ss.Writer("mixed_m"), 2),
                runs_on_stream(), mixed_rows(ss.Writer("mixed_r"), 3)]
    flagged = run_batch(efx, neighbours, directed, damaged=("abandoned", "runs_on"))
    assert flagged >= 1   # (the slice that swallowed a start code cannot pass for undamaged)
