"""NumPy model of efx_import_surfaces / efx_detect_crop_surfaces (include/efx.h, "surfaces"): the reduction of a 16-bit
sample, the conventional layouts, the checks, and the canonical I420 image of a surface.  Everything behind the canonical
image is the unmodified model of the packed formats (import_model.py, crop_model.py).  It shares no code with
espflix_amd/csrc/surface_px.h."""
from dataclasses import dataclass, field, replace

import numpy as np

import crop_model
import import_model

PLANAR8, SEMI8, PLANAR16, SEMI16 = 0, 1, 2, 3
# kind: (efx_surface_kind, layout, shift, swap_uv)
KINDS = {"i420": (0, PLANAR8, 0, 0), "yv12": (1, PLANAR8, 0, 0), "nv12": (2, SEMI8, 0, 0), "nv21": (3, SEMI8, 0, 1),
         "p010": (4, SEMI16, 8, 0), "p012": (5, SEMI16, 8, 0), "p016": (6, SEMI16, 8, 0),
         "i010": (7, PLANAR16, 2, 0), "i012": (8, PLANAR16, 4, 0), "i016": (9, PLANAR16, 8, 0)}
MAX_PITCH, MAX_BYTES = 1 << 20, 1 << 40

# The smallest shapes at which the loaders can still go wrong: kind, width, height, pitch, plane rows, images, crop,
# destination rectangle.  The GPU tests run all of them, the host program all but the two 1080p ones.
GEOMETRIES = [
    ("nv21", 2, 2, 0, 0, 3, None, None),
    ("yv12", 16, 16, 0, 0, 3, None, None),
    ("nv12", 34, 18, 50, 0, 3, (2, 2, 30, 14), (16, 8, 320, 160)),  # rows start on every byte phase of a 16-byte piece
    ("p010", 34, 18, 74, 0, 3, None, None),
    ("i010", 354, 194, 712, 0, 3, None, None),
    ("p016", 4096, 16, 0, 0, 1, None, None),                        # the widest raw row and the widest pair row
    ("nv12", 1920, 1080, 2048, 1088, 2, None, None),
    ("p010", 1920, 1080, 4096, 1088, 1, None, None),
]


@dataclass
class Surface:
    layout: int
    shift: int
    swap_uv: int
    width: int
    height: int
    offset: list = field(default_factory=lambda: [0, 0, 0])
    pitch: list = field(default_factory=lambda: [0, 0, 0])
    bytes: int = 0

    @property
    def words(self):
        return self.layout in (PLANAR16, SEMI16)

    @property
    def semi(self):
        return self.layout in (SEMI8, SEMI16)

    def planes(self):
        """(plane, rows, samples per row) of every plane that is read; a pair row counts width samples."""
        if self.semi:
            return [(0, self.height, self.width), (1, self.height // 2, self.width)]
        return [(0, self.height, self.width), (1, self.height // 2, self.width // 2), (2, self.height // 2, self.width // 2)]

    def args(self):
        """The fields in efx_surface's order, for a command line."""
        return [self.layout, self.shift, self.swap_uv, self.width, self.height, *self.offset, *self.pitch, self.bytes]


def reduce(w, shift):
    """min(255, (w + (1 << (shift - 1))) >> shift) of uint16 samples."""
    return np.minimum(255, (np.asarray(w).astype(np.int64) + (1 << (shift - 1))) >> shift).astype(np.uint8)


def check(s):
    """True for a surface efx_import_surfaces accepts."""
    if s.layout not in (PLANAR8, SEMI8, PLANAR16, SEMI16):
        return False
    if (not 1 <= s.shift <= 8) if s.words else s.shift != 0:
        return False
    if s.swap_uv not in ((0, 1) if s.semi else (0,)):
        return False
    if not (2 <= s.width <= 4096 and 2 <= s.height <= 4096) or (s.width | s.height) & 1:
        return False
    if not 0 <= s.bytes < MAX_BYTES:
        return False
    B = 2 if s.words else 1
    for p, rows, samples in s.planes():
        if s.words and (s.offset[p] | s.pitch[p]) & 1:
            return False
        if not samples * B <= s.pitch[p] <= MAX_PITCH:
            return False
        if s.offset[p] < 0 or s.offset[p] + (rows - 1) * s.pitch[p] + samples * B > s.bytes:
            return False
    return True


def layout(kind, width, height, pitch=0, plane_rows=0):
    """efx_surface_layout: the conventional layout, None for rejected arguments."""
    if kind not in KINDS:
        return None
    _, lay, shift, swap = KINDS[kind]
    s = Surface(lay, shift, swap, width, height)
    B = 2 if s.words else 1
    P, R = pitch or width * B, plane_rows or height
    if R < height or R & 1 or (not s.semi and P % (2 * B)):
        return None
    s.pitch[0] = P
    s.offset[1] = P * R
    if s.semi:
        s.pitch[1] = P
    else:
        s.pitch[1] = s.pitch[2] = P // 2
        s.offset[2] = P * R + (P // 2) * (R // 2)
        if kind == "yv12":
            s.offset[1], s.offset[2] = s.offset[2], s.offset[1]
    s.bytes = P * R * 3 // 2
    return s if check(s) else None


def rejected_surfaces():
    """(what, surface) for every rejected case of include/efx.h."""
    nv12, p010, i010, i420 = (layout(k, 34, 18, p) for k, p in (("nv12", 50), ("p010", 74), ("i010", 72), ("i420", 36)))
    return [("layout", replace(nv12, layout=4)), ("layout", replace(nv12, layout=-1)),
           ("shift", replace(p010, shift=0)), ("shift", replace(p010, shift=9)), ("shift", replace(nv12, shift=1)),
           ("swap", replace(i420, swap_uv=1)), ("swap", replace(i010, swap_uv=1)), ("swap", replace(nv12, swap_uv=2)),
           ("size", replace(nv12, width=33)), ("size", replace(nv12, height=17)), ("size", replace(nv12, width=0)),
           ("size", replace(nv12, width=4098, pitch=[4098, 4098, 0], bytes=1 << 20)),
           ("odd", replace(p010, offset=[1, p010.offset[1], 0])), ("odd", replace(p010, pitch=[75, 74, 0])),
           ("odd", replace(i010, offset=[0, i010.offset[1], i010.offset[2] + 1])),
           ("pitch", replace(nv12, pitch=[33, 50, 0])), ("pitch", replace(nv12, pitch=[50, 33, 0])),
           ("pitch", replace(p010, pitch=[66, 74, 0])), ("pitch", replace(i010, pitch=[72, 32, 36])),
           ("pitch", replace(i420, pitch=[36, 18, 16])),
           ("pitch", replace(nv12, pitch=[(1 << 20) + 1, 50, 0], bytes=1 << 30)),
           ("beyond", replace(nv12, bytes=nv12.bytes - 17)), ("beyond", replace(i420, offset=[0, i420.offset[1], i420.bytes - 17])),
           ("beyond", replace(nv12, offset=[nv12.bytes, nv12.offset[1], 0])), ("beyond", replace(nv12, bytes=0)),
           ("bytes", replace(nv12, bytes=1 << 40))]


def field_of(s, bottom):
    """One field of an interlaced surface: every pitch doubled, the height halved, the offsets one pitch on for the
    bottom field."""
    assert s.height % 4 == 0
    return replace(s, height=s.height // 2, pitch=[2 * p for p in s.pitch],
                   offset=[o + (p if bottom else 0) for o, p in zip(s.offset, s.pitch)])


def _byte_index(s, p, rows, samples):
    B = 2 if s.words else 1
    return s.offset[p] + np.arange(rows, dtype=np.int64)[:, None] * s.pitch[p] + np.arange(samples * B, dtype=np.int64)[None, :]


def sample_mask(s):
    """Boolean array over the image's bytes: True where a sample lies (everything else is padding)."""
    m = np.zeros(s.bytes, dtype=bool)
    for p, rows, samples in s.planes():
        m[_byte_index(s, p, rows, samples).reshape(-1)] = True
    return m


def plane_samples(img, s, p, rows, samples):
    """The samples of a plane, reduced: (rows, samples) uint8."""
    raw = np.asarray(img, dtype=np.uint8).reshape(-1)[_byte_index(s, p, rows, samples)]
    if not s.words:
        return raw
    w = raw[:, 0::2].astype(np.uint16) | (raw[:, 1::2].astype(np.uint16) << 8)
    return reduce(w, s.shift)


def canonical(img, s):
    """The packed I420 picture (width * height * 3 / 2 bytes) of one image of the surface."""
    pl = [plane_samples(img, s, *t) for t in s.planes()]
    if s.semi:
        first, second = pl[1][:, 0::2], pl[1][:, 1::2]
        cb, cr = (second, first) if s.swap_uv else (first, second)
    else:
        cb, cr = pl[1], pl[2]
    return np.concatenate([pl[0].reshape(-1), cb.reshape(-1), cr.reshape(-1)])


def canonicals(srcs, s):
    return np.stack([canonical(x, s) for x in srcs])


def import_images(srcs, s, crop=None, dst=None):
    """What efx_import_surfaces writes: efx_import_frames' result for the canonical images."""
    return import_model.import_images(canonicals(srcs, s), "i420", s.width, s.height, crop, dst)


def detect(srcs, s, images_per_stream=None, limit=24, rnd=16):
    """(sums, records) of efx_detect_crop_surfaces: efx_detect_crop's for the canonical images."""
    return crop_model.detect(canonicals(srcs, s), "i420", s.width, s.height, images_per_stream, limit, rnd)


def sources(n, s, seed):
    """n images of distinct content, padding included: noise (words: full random 16-bit values), two-level noise (all
    bits clear or set), a ramp with noise in its low bits.  The padding is noise throughout."""
    rng = np.random.default_rng(seed)
    mask = sample_mask(s)
    out = rng.integers(0, 256, (n, s.bytes), dtype=np.uint8)
    for i in range(n):
        if i % 3 == 1:
            v = rng.integers(0, 2, s.bytes, dtype=np.uint8) * 255
            if s.words:
                v = np.repeat(v[0::2], 2)[:s.bytes]
        elif i % 3 == 2:
            if s.words:
                w = ((np.arange(s.bytes // 2 + 1) * 37 // max(1, s.width)) * 64 + rng.integers(0, 256, s.bytes // 2 + 1)) & 0xFFFF
                v = w.astype("<u2").view(np.uint8)[:s.bytes]
            else:
                v = ((np.arange(s.bytes) * 7 // max(1, s.width) + rng.integers(0, 4, s.bytes)) & 0xFF).astype(np.uint8)
        else:
            continue
        out[i, mask] = v[mask]
    return out


def refill_padding(srcs, s, seed):
    """The same samples with other noise in the pitch padding, the unused plane rows and between the planes."""
    rng = np.random.default_rng(seed)
    mask = sample_mask(s)
    out = rng.integers(0, 256, srcs.shape, dtype=np.uint8)
    out[:, mask] = srcs[:, mask]
    return out


def boxed(n, s, box, seed, black=16):
    """n images of noise inside box = (x, y, w, h) on a black border (luma `black`, words: black << 6 as P010 keeps it),
    chroma noise."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (n, s.bytes), dtype=np.uint8)
    x, y, w, h = box
    idx = _byte_index(s, 0, s.height, s.width)
    B = 2 if s.words else 1
    inside = np.zeros((s.height, s.width * B), dtype=bool)
    inside[y:y + h, x * B:(x + w) * B] = True
    level = np.zeros(s.width * B, dtype=np.uint8)
    if s.words:
        word = black << s.shift  # (P010: 16 << 8 = 64 << 6)
        level[0::2], level[1::2] = word & 0xFF, word >> 8
    else:
        level[:] = black
    for i in range(n):
        rows = out[i][idx]
        out[i][idx] = np.where(inside, rows, level[None, :])
    return out
