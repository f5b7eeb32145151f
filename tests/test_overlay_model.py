"""The rule of efx_overlay: whole calls on the host through espflix_amd/csrc/overlay_px.h with the kernel's own walk
(tests/overlay_model_main.cpp, built here with the host compiler) against the NumPy model of include/efx.h's definition
(tests/overlay_model.py) on the directed cases the device runs too (tests/test_gpu_overlay.py takes them from here), the
properties the definition states, the validity rule clause by clause, the record dtypes against the header, the time
spans and the atlas packer.  No GPU."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import overlay_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PICTURE = M.W, M.H, M.PICTURE


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def alpha(rng, h, w):
    """An alpha mask with every kind of byte: noise, and runs of 0 and of 255."""
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    a[rng.random((h, w)) < 0.15] = 0
    a[rng.random((h, w)) < 0.15] = 255
    return a


def rgba(rng, h, w):
    """RGBA with random colours and alpha; where it is high enough, a row of alpha 0 and one of 255."""
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[:, :, 3] = alpha(rng, h, w)
    if h >= 3:
        px[1, :, 3], px[2, :, 3] = 0, 255
    return px


class Case:
    """One call: specs are dicts with a `bitmap` ((h, w) alpha or (h, w, 4) RGBA), `pad` (bytes of pitch beyond the row; a
    multiple of 4 for RGBA) and the event's fields; the bitmaps lie one behind the other in an atlas with gaps, whose
    every byte outside the bitmaps is fill.  raw: records appended as they are (invalid ones)."""

    def __init__(self, specs, n_streams=1, n_pictures=1, first_picture=0, seed=0, raw=(), atlas_bytes=None, slack=0):
        self.n_streams, self.n_pictures, self.first_picture = n_streams, n_pictures, first_picture
        rng = np.random.default_rng(seed)
        self.pictures = rng.integers(0, 256, (n_streams, n_pictures, PICTURE), dtype=np.uint8)
        self.placed, recs, size = [], [], 0
        for s in specs:
            s = dict(s)
            b, pad = s.pop("bitmap"), s.pop("pad", 0)
            h, w = b.shape[:2]
            kind = M.RGBA if b.ndim == 3 else M.A8
            pitch = w * (4 if kind else 1) + pad
            offset = (size + 3) // 4 * 4 if kind else size
            self.placed.append((offset, pitch, np.ascontiguousarray(b).reshape(h, -1)))
            size = offset + (h - 1) * pitch + w * (4 if kind else 1) + 5
            recs.append(M.event(offset=offset, pitch=pitch, w=w, h=h, kind=kind, **s))
        self.size = size - 5 if specs else 0
        self.atlas_bytes = self.size if atlas_bytes is None else atlas_bytes
        self.alloc = (max(self.size, self.atlas_bytes) + slack + 15) // 16 * 16  # what a test allocates for the atlas
        self.events = M.events(recs + list(raw))

    def atlas(self, fill_seed):
        """The allocation's bytes: the bitmaps, and noise that depends on fill_seed everywhere else."""
        out = np.random.default_rng(1000 + fill_seed).integers(0, 256, self.alloc, dtype=np.uint8)
        for offset, pitch, rows in self.placed:
            for r, row in enumerate(rows):
                out[offset + r * pitch:offset + r * pitch + row.size] = row
        return out

    def want(self, fill_seed=1):
        return M.overlay(self.pictures, self.events, self.atlas(fill_seed), self.atlas_bytes, self.first_picture)


def one_per_picture(specs, **kw):
    """Event k on picture k alone."""
    return Case([dict(s, first=k, last=k) for k, s in enumerate(specs)], n_pictures=len(specs), **kw)


def alignment(seed=10):
    """A 21 x 5 mask at each x in 0 .. 16 and y in 0, 1: every byte alignment against the 16-byte chunk, both parities of
    the chroma sites.  A pitch of 21 puts the rows at every alignment in the atlas too."""
    rng = np.random.default_rng(seed)
    return one_per_picture([dict(bitmap=alpha(rng, 5, 21), x=x, y=y, colour=0x40C0F0) for y in (0, 1) for x in range(17)], seed=seed)


def sizes(seed=11):
    rng = np.random.default_rng(seed)
    a = lambda h, w: alpha(rng, h, w)
    specs = [dict(bitmap=a(1, 1), x=0, y=0), dict(bitmap=a(1, 1), x=351, y=191), dict(bitmap=a(1, 1), x=1, y=1),
             dict(bitmap=a(192, 352), x=0, y=0, colour=0x10FF20), dict(bitmap=a(200, 400), x=-24, y=-4, colour=0xFF0000, pad=3),
             # over each edge and each corner by an odd amount
             dict(bitmap=a(9, 30), x=-7, y=40), dict(bitmap=a(9, 30), x=352 - 23, y=41), dict(bitmap=a(9, 30), x=100, y=-3),
             dict(bitmap=a(9, 30), x=101, y=192 - 4), dict(bitmap=a(9, 30), x=-5, y=-3), dict(bitmap=a(9, 30), x=352 - 9, y=-1),
             dict(bitmap=rgba(rng, 9, 30), x=-11, y=192 - 5), dict(bitmap=rgba(rng, 9, 30), x=352 - 17, y=192 - 7, pad=8)]
    return one_per_picture(specs, seed=seed)


def outside(seed=12):
    """Wholly outside on each side, one stream each: nothing may be touched."""
    rng = np.random.default_rng(seed)
    at = [(-30, 50), (352, 50), (60, -9), (60, 192)]
    return Case([dict(bitmap=alpha(rng, 9, 30), x=x, y=y, stream=k) for k, (x, y) in enumerate(at)], n_streams=4, seed=seed)


def kinds(seed=13):
    rng = np.random.default_rng(seed)
    specs = [dict(bitmap=rgba(rng, 24, 48), x=290, y=10), dict(bitmap=rgba(rng, 24, 48), x=3, y=151, pad=20),
             dict(bitmap=rgba(rng, 7, 5), x=33, y=77, pad=4), dict(bitmap=alpha(rng, 7, 45), x=15, y=9, pad=0, colour=0x000000),
             dict(bitmap=alpha(rng, 7, 45), x=16, y=8, pad=19, colour=0xFFFF00)]
    return one_per_picture(specs, seed=seed)


def gains(seed=14):
    rng = np.random.default_rng(seed)
    mask, logo = alpha(rng, 12, 40), rgba(rng, 12, 40)
    specs = [dict(bitmap=b, x=20 + 3 * k, y=30 + k, opacity=op) for k, op in enumerate((0, 1, 128, 255, 256)) for b in (mask, logo)]
    return one_per_picture(specs, seed=seed)


def fades(seed=15):
    """Pictures 13 .. 19 of a title: one event fades in from 10 (picture 0 of the call is mid-fade), one ends at 22 with a
    fade-out of 6 (the call ends mid-fade), one does both inside the call, one is a single picture with both fades."""
    rng = np.random.default_rng(seed)
    specs = [dict(bitmap=alpha(rng, 10, 50), x=5, y=5, first=10, last=30, fade_in=6),
             dict(bitmap=rgba(rng, 10, 50), x=70, y=5, first=0, last=22, fade_out=6),
             dict(bitmap=alpha(rng, 10, 50), x=135, y=6, first=14, last=18, fade_in=3, fade_out=2, opacity=200),
             dict(bitmap=alpha(rng, 10, 50), x=200, y=7, first=16, last=16, fade_in=3, fade_out=5)]
    return Case(specs, n_pictures=7, first_picture=13, seed=seed)


def order(seed=16, reverse=False):
    """Two and three events over each other (picture 0 and 1), and one that overlaps only another's corner (picture 2)."""
    rng = np.random.default_rng(seed)
    specs = [dict(bitmap=alpha(rng, 20, 60) | 64, x=40, y=40, colour=0xFFFFFF, first=0, last=1),
             dict(bitmap=rgba(rng, 20, 60), x=61, y=47, first=0, last=1),
             dict(bitmap=alpha(rng, 20, 60) | 64, x=55, y=51, colour=0x000000, first=1, last=1),
             dict(bitmap=alpha(rng, 11, 33) | 128, x=200, y=100, colour=0x2040FF, first=2, last=2),
             dict(bitmap=alpha(rng, 11, 33) | 128, x=232, y=110, colour=0xFF4020, first=2, last=2)]
    return Case(specs[::-1] if reverse else specs, n_pictures=3, seed=seed)


def streams(n_streams, n_pictures, seed=17):
    """stream = -1, 0, 2 and 7 (never in the call), on pictures 0, 2 and 4 only."""
    rng = np.random.default_rng(seed)
    specs = []
    for k, stream in enumerate((-1, 0, 2, 7)):
        for p in (0, 2, 4):
            specs.append(dict(bitmap=alpha(rng, 9, 37), x=10 + 80 * k + p, y=20 + 30 * k, stream=stream, first=p, last=p, colour=0x80FF00 + k))
    return Case(specs, n_streams=n_streams, n_pictures=n_pictures, seed=seed + n_streams + 10 * n_pictures)


def listed(n, seed=18):
    """A list of n events whose first and last are shown on picture 0; the fillers are valid events of other pictures."""
    rng = np.random.default_rng(seed)
    mask = alpha(rng, 6, 26)
    shown = [dict(bitmap=alpha(rng, 9, 37), x=31, y=17, colour=0x123456), dict(bitmap=rgba(rng, 9, 37), x=50, y=21)]
    specs = [dict(shown[0])] if n else []
    specs += [dict(bitmap=mask, x=k % 300, y=k % 150, first=5 + k, last=9 + k) for k in range(n - 2)]
    if n > 1:
        specs.append(dict(shown[1]))
    return Case(specs, n_pictures=2, seed=seed)


def invalid_records(c, inside):
    """One record per clause of the validity rule, each a copy of a valid event of case c with one field beyond its
    limit.  inside: an offset that lies beyond atlas_bytes but inside the allocation."""
    base = c.events[0]

    def bad(**kw):
        e = base.copy()
        for k, v in kw.items():
            e[k] = v
        return e
    w, h = int(base["w"]), int(base["h"])
    return [bad(kind=2), bad(first=-1), bad(first=3, last=2), bad(last=1 << 40), bad(stream=-2), bad(x=-4097), bad(x=4096), bad(y=-4097),
            bad(y=4096), bad(w=0), bad(w=4097, pitch=4097), bad(h=0), bad(h=4097), bad(opacity=257), bad(fade_in=32768),
            bad(fade_out=32768), bad(pitch=w - 1), bad(kind=M.RGBA, colour=0, pitch=4 * w, offset=2), bad(kind=M.RGBA, colour=0, pitch=4 * w + 2, offset=0),
            bad(offset=inside), bad(offset=c.atlas_bytes - (h - 1) * int(base["pitch"]) - w + 1), bad(colour=1 << 24),
            bad(kind=M.RGBA, colour=1, pitch=4 * w, offset=0), bad(reserved0=1), bad(reserved=1)]


def with_invalid(seed=19):
    """Valid events with every invalid record between them: atlas_bytes ends with the last bitmap, the allocation goes on."""
    rng = np.random.default_rng(seed)
    specs = [dict(bitmap=alpha(rng, 8, 30), x=12, y=14, colour=0xFF00FF), dict(bitmap=rgba(rng, 8, 30), x=200, y=100)]
    c = Case(specs, n_streams=2, seed=seed, slack=512)
    c.events = M.events([c.events[0]] + invalid_records(c, inside=c.atlas_bytes + 64) + [c.events[1]])
    return c


def cases():
    """name -> Case: what the host program and the device are both compared with the model on."""
    out = {"alignment": alignment(), "sizes": sizes(), "outside": outside(), "kinds": kinds(), "gains": gains(), "fades": fades(),
           "order": order(), "order reversed": order(reverse=True), "invalid": with_invalid()}
    for n_streams in (1, 3):
        for n_pictures in (1, 5):
            out[f"streams {n_streams} x {n_pictures}"] = streams(n_streams, n_pictures)
    return out


# ---- the host program ------------------------------------------------------------------------------------------------------------
def compile_main(tmp, name, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build overlay_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "overlay_model_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return compile_main(tmp_path_factory.mktemp("overlay_px"), "drv", "-O2")


def host_call(exe, c, fill_seed=1, pictures=None, first_picture=None):
    """One call of the host program: (pictures, status words)."""
    pics = c.pictures if pictures is None else pictures
    first = c.first_picture if first_picture is None else first_picture
    data = c.events.tobytes() + c.atlas(fill_seed)[:c.atlas_bytes].tobytes() + np.ascontiguousarray(pics).tobytes()
    r = subprocess.run([exe, "call", str(pics.shape[0]), str(pics.shape[1]), str(len(c.events)), str(first), str(c.atlas_bytes)],
                       input=data, capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.frombuffer(r.stdout, dtype=np.uint8)
    return out[:pics.size].reshape(pics.shape), out[pics.size:].view(np.uint32)


def scan_step(exe):
    return int(subprocess.run([exe, "step"], check=True, capture_output=True, text=True, timeout=60).stdout)


@pytest.mark.parametrize("name", list(cases()))
def test_host_program_equals_the_model(host, name):
    c = cases()[name]
    want = c.want(fill_seed=2)
    assert np.array_equal(want, c.want(fill_seed=1)), "the model reads bytes between the bitmaps"
    got, st = host_call(host, c, fill_seed=1)
    assert np.array_equal(got, want), name
    assert st.tolist() == [M.status(c.events, c.atlas_bytes)] * c.n_streams
    assert name in ("outside",) or not np.array_equal(want, c.pictures), "nothing was drawn: the case is vacuous"


def test_outside_and_other_streams_leave_the_pictures_alone():
    c = outside()
    assert np.array_equal(c.want(), c.pictures)
    c = streams(3, 5)
    want = c.want()
    assert np.array_equal(want[:, [1, 3]], c.pictures[:, [1, 3]]) and not np.array_equal(want[1, 0], c.pictures[1, 0])
    only_all = M.overlay(c.pictures, c.events[c.events["stream"] == -1], c.atlas(1), c.atlas_bytes)
    assert np.array_equal(want[1], only_all[1]), "stream 1 is shown an event of stream 0, 2 or 7"
    assert not np.array_equal(want[0], only_all[0]) and not np.array_equal(want[2], only_all[2])


def test_order_matters():
    a, b = order().want(), order(reverse=True).want()
    assert not np.array_equal(a[0, 0], b[0, 0]) and not np.array_equal(a[0, 1], b[0, 1]) and not np.array_equal(a[0, 2], b[0, 2])
    # the header's numbers: white then black at a = 128 on Y = 100, and the other way round
    white, black = int(M.ycbcr(255, 255, 255)[0]), int(M.ycbcr(0, 0, 0)[0])
    assert (white, black) == (235, 16)
    assert int(M.luma(M.luma(100, white, 128), black, 128)) == 92 and int(M.luma(M.luma(100, black, 128), white, 128)) == 147


@pytest.mark.parametrize("n", [0, 1, "step - 1", "step", "step + 1", "4 steps + 1"])
def test_list_lengths_around_the_scan_step(host, n):
    step = scan_step(host)
    n = eval(n.replace("steps", "* step"), {"step": step}) if isinstance(n, str) else n
    c = listed(n)
    want = c.want()
    got, st = host_call(host, c)
    assert np.array_equal(got, want) and not st.any()
    assert np.array_equal(want[0, 1], c.pictures[0, 1]) and (n == 0 or not np.array_equal(want[0, 0], c.pictures[0, 0]))
    if n > 1:
        assert not np.array_equal(want, M.overlay(c.pictures, c.events[:-1], c.atlas(1), c.atlas_bytes)), "the last event is not seen"


def pieces(seed=30):
    """Two streams of 12 pictures with events that begin, fade and end on either side of picture 5."""
    rng = np.random.default_rng(seed)
    specs = [dict(bitmap=alpha(rng, 14, 90), x=100, y=150, first=2, last=9, fade_in=4, fade_out=4),
             dict(bitmap=rgba(rng, 24, 48), x=296, y=8, first=0, last=11, opacity=180),
             dict(bitmap=alpha(rng, 14, 90), x=130, y=158, first=4, last=6, colour=0xFFFF00, stream=1)]
    return Case(specs, n_streams=2, n_pictures=12, seed=seed)


def test_pieces_equal_one_long_call(host):
    """Pictures 0 .. 11 as one call against 0 .. 4 and 5 .. 11 with first_picture = 5."""
    c = pieces()
    whole = c.want()
    for call in (lambda p, f: M.overlay(p, c.events, c.atlas(1), c.atlas_bytes, f), lambda p, f: host_call(host, c, pictures=p, first_picture=f)[0]):
        assert np.array_equal(call(c.pictures, 0), whole)
        assert np.array_equal(np.concatenate([call(c.pictures[:, :5], 0), call(c.pictures[:, 5:], 5)], axis=1), whole)
    assert not np.array_equal(M.overlay(c.pictures[:, 5:], c.events, c.atlas(1), c.atlas_bytes, 0), whole[:, 5:]), "first_picture does not matter here"


def test_sanitized_host_program_on_a_clipped_pitched_rgba_case(tmp_path):
    """-fsanitize=address,undefined: the blocks are exactly the events, the atlas rounded up to 16 and the pictures, so a
    16-byte access in front of the atlas, beyond its end or outside a picture ends the program."""
    exe = compile_main(tmp_path, "drv_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
    rng = np.random.default_rng(31)
    # (the first bitmap begins with the atlas, the last one's only byte ends it: both ends lie next to an access)
    specs = [dict(bitmap=rgba(rng, 9, 30), x=-11, y=-3, pad=8), dict(bitmap=rgba(rng, 9, 30), x=352 - 17, y=192 - 7, pad=12),
             dict(bitmap=alpha(rng, 3, 5), x=-2, y=100), dict(bitmap=alpha(rng, 1, 1), x=351, y=0)]
    c = Case(specs, seed=31)
    got, st = host_call(exe, c)
    assert np.array_equal(got, c.want()) and not st.any()


# ---- the arithmetic --------------------------------------------------------------------------------------------------------------
def test_division_identities_over_their_whole_ranges(host):
    t = np.arange(65025 + 1, dtype=np.int64)
    assert np.array_equal((t + 128 + ((t + 128) >> 8)) >> 8, (2 * t + 255) // 510)
    n = np.arange(260610 + 1, dtype=np.int64)
    assert np.array_equal((n * 4210753) >> 32, n // 1020) and np.array_equal((n * 263173) >> 28, n // 1020)
    # ... and overlay_px.h's own functions, the packed luma blend and the gain of four bytes among them
    r = subprocess.run([host, "divide"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok"


def test_alpha_0_and_255():
    """a = 0 leaves every byte; a = 255 gives the colour exactly, luma and both chroma planes."""
    y = np.arange(256)
    for c in (0, 16, 100, 235, 255):
        assert np.array_equal(M.luma(y, c, 0), y) and np.all(M.luma(y, c, 255) == c)
        four0, four255 = np.zeros((4, 256), dtype=np.int64), np.full((4, 256), 255)
        assert np.array_equal(M.chroma(y, four0, np.full((4, 256), c)), y) and np.all(M.chroma(y, four255, np.full((4, 256), c)) == c)
    rng = np.random.default_rng(32)
    for bitmap, colour in ((np.zeros((8, 10), dtype=np.uint8), 0xFF8800), (np.full((8, 10), 255, dtype=np.uint8), 0xFF8800)):
        c = Case([dict(bitmap=bitmap, x=20, y=30, colour=colour)], seed=32)
        want = c.want()
        if not bitmap.any():
            assert np.array_equal(want, c.pictures)
            continue
        cy, cb, cr = (int(v) for v in M.ycbcr(0xFF, 0x88, 0x00))
        assert np.all(want[0, 0, :M.CB].reshape(H, W)[30:38, 20:30] == cy)
        assert np.all(want[0, 0, M.CB:M.CR].reshape(H // 2, W // 2)[15:19, 10:15] == cb)
        assert np.all(want[0, 0, M.CR:].reshape(H // 2, W // 2)[15:19, 10:15] == cr)
        changed = want != c.pictures
        assert changed[0, 0, :M.CB].reshape(H, W)[30:38, 20:30].sum() == changed[0, 0, :M.CB].sum(), "luma outside the rectangle changed"
    px = rgba(rng, 6, 6)
    px[:, :, 3] = 255
    c = Case([dict(bitmap=px, x=100, y=50)], seed=33)
    want = c.want()
    cy, cb, cr = M.ycbcr(px[:, :, 0], px[:, :, 1], px[:, :, 2])
    assert np.array_equal(want[0, 0, :M.CB].reshape(H, W)[50:56, 100:106], cy)
    mean = lambda v: (v.reshape(3, 2, 3, 2).transpose(0, 2, 1, 3).reshape(3, 3, 4).sum(axis=2) * 255 + 510) // 1020
    assert np.array_equal(want[0, 0, M.CB:M.CR].reshape(H // 2, W // 2)[25:28, 50:53], mean(cb))
    assert np.array_equal(want[0, 0, M.CR:].reshape(H // 2, W // 2)[25:28, 50:53], mean(cr))


def test_chroma_lies_between_its_extremes():
    rng = np.random.default_rng(34)
    C, a, c = rng.integers(0, 256, 50000), rng.integers(0, 256, (4, 50000)), rng.integers(0, 256, (4, 50000))
    a[:, :1000], a[:, 1000:2000] = 0, 255
    out = M.chroma(C, a, c)
    assert np.all(out >= np.minimum(C, c.min(axis=0))) and np.all(out <= np.maximum(C, c.max(axis=0)))
    assert (C * (1020 - a.sum(axis=0)) + (a * c).sum(axis=0) + 510).max() <= 260610


def test_gain():
    e = M.event(first=10, last=20, fade_in=3, fade_out=2, opacity=256)
    assert [M.gain(e, p) for p in range(10, 21)] == [64, 128, 192, 256, 256, 256, 256, 256, 256, 170, 85]
    for fades in (dict(), dict(fade_in=5), dict(fade_out=7), dict(fade_in=32767, fade_out=32767)):
        assert all(M.gain(M.event(first=0, last=9, opacity=0, **fades), p) == 0 for p in range(10))
    assert all(M.gain(M.event(first=0, last=9, opacity=256), p) == 256 for p in range(10))
    # one picture with both fades: the smaller side counts
    one = M.event(first=7, last=7, fade_in=3, fade_out=1, opacity=256)
    assert M.gain(one, 7) == (256 * min(256 // 4, 256 // 2) + 128) >> 8 == 64
    assert M.gain(M.event(first=7, last=7, fade_in=1, fade_out=1, opacity=255), 7) == (255 * 128 + 128) >> 8
    assert all(0 <= M.gain(M.event(first=0, last=40, fade_in=fi, fade_out=fo, opacity=op), p) <= 256
               for fi in (0, 1, 7, 100) for fo in (0, 2, 50) for op in (0, 1, 255, 256) for p in (0, 1, 20, 39, 40))
    a = (np.arange(256) * 256 + 128) >> 8
    assert a[255] == 255 and a.max() == 255, "A = 255 at g = 256 gives 255"


# ---- the validity rule ----------------------------------------------------------------------------------------------------------
def test_validity_clause_by_clause():
    """One event per clause at its limit (valid) and one just past it; efx_overlay_check gives the model's index."""
    import espflix_amd as efx
    lib = efx.load_library()

    def check(evs, atlas_bytes):
        evs = M.events(evs)
        got = lib.efx_overlay_check(evs.ctypes.data, len(evs), atlas_bytes)
        assert got == M.check(evs, atlas_bytes) == efx.overlay_check(evs, atlas_bytes)
        return got
    A = 1 << 20
    ok = dict(w=8, h=4, pitch=8)
    at_limit = [dict(kind=M.RGBA, pitch=32, colour=0), dict(first=0, last=0), dict(first=5, last=5), dict(last=(1 << 40) - 1), dict(stream=-1),
                dict(stream=1 << 30), dict(x=-4096), dict(x=4095), dict(y=-4096), dict(y=4095), dict(w=1, pitch=1), dict(w=4096, pitch=4096),
                dict(h=1), dict(h=4096, pitch=8), dict(opacity=256), dict(fade_in=32767), dict(fade_out=32767), dict(pitch=8),
                dict(kind=M.RGBA, pitch=36, offset=4, colour=0), dict(offset=A - 3 * 8 - 8), dict(colour=(1 << 24) - 1)]
    past = [dict(kind=2), dict(kind=255), dict(first=-1), dict(first=6, last=5), dict(last=1 << 40), dict(stream=-2), dict(x=-4097), dict(x=4096),
            dict(y=-4097), dict(y=4096), dict(w=0), dict(w=4097, pitch=4097), dict(h=0), dict(h=4097), dict(opacity=257),
            dict(fade_in=32768), dict(fade_out=32768), dict(pitch=7), dict(kind=M.RGBA, pitch=31, colour=0), dict(kind=M.RGBA, pitch=34, colour=0),
            dict(kind=M.RGBA, pitch=32, offset=2, colour=0), dict(offset=A - 3 * 8 - 7), dict(offset=A + 1), dict(offset=(1 << 64) - 8),
            dict(colour=1 << 24), dict(kind=M.RGBA, pitch=32, colour=1), dict(reserved0=1), dict(reserved=1)]
    good = [M.event(**{**ok, **kw}) for kw in at_limit]
    for e in good:
        assert M.valid(e, A), e
    assert check(good, A) == -1
    for kw in past:
        e = M.event(**{**ok, **kw})
        assert not M.valid(e, A), kw
        assert check(good[:3] + [e] + good[3:], A) == 3, kw
        assert check([e], A) == 0, kw
    assert check([], A) == -1 and lib.efx_overlay_check(None, 5, A) == -1
    assert check(good[:2], 0) == 0 and check([M.event(w=1, h=1)], 1) == -1 and check([M.event(w=1, h=1)], 0) == 0
    c = with_invalid()
    assert [M.valid(e, c.atlas_bytes) for e in c.events] == [True] + [False] * (len(c.events) - 2) + [True]
    assert check(list(c.events), c.atlas_bytes) == 1


# ---- the binding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_name,py_name", [("efx_overlay_event", "OVERLAY_EVENT_DTYPE"), ("efx_overlay_opts", "OVERLAY_OPTS_DTYPE")])
def test_record_dtypes_match_the_header(tmp_path, c_name, py_name):
    """The dtypes against the structs as the host C compiler lays them out: size, and every field's name, order, offset and
    size; the event is the 64-byte record of the header's table, which the model's own dtype restates."""
    from espflix_amd import _abi
    import espflix_amd as efx
    import test_abi_layout as A
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a host C compiler is needed to lay out include/efx.h"
    dt = getattr(_abi, py_name)
    assert getattr(efx, py_name) is dt and list(dt.names) == A.header_fields(c_name)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "efx.h"', "int main(void) {", f'  printf("%zu\\n", sizeof({c_name}));']
    for f in dt.names:
        lines.append(f'  printf("%zu %zu\\n", offsetof({c_name}, {f}), sizeof((({c_name} *)0)->{f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert dt.itemsize == int(out[0])
    for name, line in zip(dt.names, out[1:]):
        sub, offset = dt.fields[name][:2]
        assert [offset, sub.itemsize] == [int(v) for v in line.split()], name
    assert sum(dt.fields[n][0].itemsize for n in dt.names) == dt.itemsize, "a hole: the header has a field the dtype lacks"
    if c_name == "efx_overlay_event":
        assert dt == M.EVENT and dt.itemsize == 64
        table = dict(first=0, last=8, offset=16, stream=24, x=28, y=32, pitch=36, colour=40, w=44, h=46, opacity=48, fade_in=50, fade_out=52,
                     kind=54, reserved0=55, reserved=56)
        assert {n: dt.fields[n][1] for n in dt.names} == table
    hdr = open(os.path.join(ROOT, "include", "efx.h")).read()
    assert "#define EFX_OVERLAY_BAD_EVENT 8192u" in hdr and efx.OVERLAY_BAD_EVENT == M.BAD_EVENT == 8192
    assert "#define EFX_OVL_A8   0" in hdr and "#define EFX_OVL_RGBA 1" in hdr and (efx.OVL_A8, efx.OVL_RGBA) == (M.A8, M.RGBA) == (0, 1)
    assert "#define EFX_OVERLAY_MAX_EVENTS 4096" in hdr and efx.OVERLAY_MAX_EVENTS == 4096


def test_overlay_span():
    """first = ceil(start x fps), last = ceil(end x fps) - 1, exactly: boundaries on and between pictures."""
    import espflix_amd as efx
    assert efx.overlay_span(24, 1, 2) == (24, 47) and efx.overlay_span(24, 0, 1) == (0, 23)
    assert efx.overlay_span(24, Fraction(1, 48), Fraction(3, 48)) == (1, 1)       # between pictures: 0.5 .. 1.5
    assert efx.overlay_span(25, "1/25", "2/25") == (1, 1) and efx.overlay_span(25, 0.5, 1.5) == (13, 37)
    assert efx.overlay_span(25, Fraction(1, 50), Fraction(101, 50)) == (1, 50)
    ntsc = Fraction(30000, 1001)
    assert efx.overlay_span("30000/1001", Fraction(1001, 30000), Fraction(2002, 30000)) == (1, 1)  # on pictures 1 and 2
    assert efx.overlay_span(ntsc, Fraction(1001, 30000) + Fraction(1, 10 ** 9), Fraction(3003, 30000)) == (2, 2)
    assert efx.overlay_span(ntsc, 0, Fraction(1001, 30000) - Fraction(1, 10 ** 9)) == (0, 0)
    assert efx.overlay_span(ntsc, 10, 20) == (300, 599) and efx.overlay_span(ntsc, Fraction(1001, 100), 20) == (300, 599)
    assert efx.overlay_span(ntsc, Fraction(1001, 100) + Fraction(1, 10 ** 12), 20) == (301, 599)
    for empty in ((24, 1, 1), (24, 2, 1), (24, Fraction(1, 100), Fraction(2, 100)), (ntsc, Fraction(1, 1000), Fraction(33, 1000)), (25, -1, 1)):
        with pytest.raises(ValueError):
            efx.overlay_span(*empty)


def test_atlas_packer():
    """Array objects shared by several events are packed once; offsets are multiples of 16; the records are valid."""
    import espflix_amd as efx
    rng = np.random.default_rng(35)
    text, logo, dot = alpha(rng, 5, 21), rgba(rng, 7, 9), alpha(rng, 1, 1)
    ovs = [efx.Overlay(text, 0, 3, 1, 2), efx.Overlay(logo, 0, 99, 300, 8, stream=1, opacity=200), efx.Overlay(text, 4, 5, -3, 190, colour=(1, 2, 3)),
           efx.Overlay(dot, 7, 7, 0, 0, fade_in=2, fade_out=3), efx.Overlay(logo, 100, 199, 300, 8), efx.Overlay(text.copy(), 9, 9, 0, 0)]
    events, atlas = efx.overlay_pack(ovs)
    assert events.dtype == efx.OVERLAY_EVENT_DTYPE and atlas.dtype == np.uint8 and atlas.size % 16 == 0
    assert all(int(o) % 16 == 0 for o in events["offset"])
    assert events["offset"][0] == events["offset"][2] and events["offset"][1] == events["offset"][4] and events["offset"][5] != events["offset"][0]
    assert atlas.size == sum((b.size + 15) // 16 * 16 for b in (text, logo, dot, text))
    assert efx.overlay_check(events, atlas.size) == -1 == M.check(events, atlas.size)
    for o, e in zip(ovs, events):
        h, w = o.bitmap.shape[:2]
        bpp = 4 if o.bitmap.ndim == 3 else 1
        rows = np.stack([atlas[int(e["offset"]) + r * int(e["pitch"]):][:w * bpp] for r in range(h)])
        assert np.array_equal(rows, o.bitmap.reshape(h, -1)) and (int(e["w"]), int(e["h"]), int(e["kind"])) == (w, h, bpp == 4)
    assert events["colour"].tolist() == [0xFFFFFF, 0, 0x010203, 0xFFFFFF, 0, 0xFFFFFF]
    assert events[1]["stream"] == 1 and events[1]["opacity"] == 200 and (events[3]["fade_in"], events[3]["fade_out"]) == (2, 3)
    assert (events[2]["x"], events[2]["y"], events[2]["first"], events[2]["last"]) == (-3, 190, 4, 5)
    # the model draws from the packed atlas what it draws from the bitmaps laid out by hand
    pics = rng.integers(0, 256, (2, 6, PICTURE), dtype=np.uint8)
    c = Case([dict(bitmap=o.bitmap, x=o.x, y=o.y, first=o.first, last=o.last, stream=o.stream, opacity=o.opacity, fade_in=o.fade_in,
                   fade_out=o.fade_out, **({} if o.bitmap.ndim == 3 else dict(colour=o.colour[0] << 16 | o.colour[1] << 8 | o.colour[2])))
              for o in ovs], seed=36)
    assert np.array_equal(M.overlay(pics, events, atlas), M.overlay(pics, c.events, c.atlas(1), c.atlas_bytes))
    assert efx.overlay_pack([])[0].size == 0 and efx.overlay_pack([])[1].size == 0
    for bad in (efx.Overlay(text.astype(np.int16), 0, 0, 0, 0), efx.Overlay(np.zeros((2, 2, 3), np.uint8), 0, 0, 0, 0),
                efx.Overlay(text, 0, 0, 0, 0, opacity=70000), efx.Overlay(text, 0, 0, 0, 0, colour=(256, 0, 0))):
        with pytest.raises(ValueError, match="event 1 "):
            efx.overlay_pack([ovs[0], bad])
