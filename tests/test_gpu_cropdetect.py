"""efx_detect_crop (k_cropdetect): the black borders of I420 / RGB24 / RGBP source pictures found on the device, row and
column sums and records bit for bit against the NumPy model of include/efx.h's definition (tests/crop_model.py)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import crop_model as M
import import_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
SUMS_FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def dec(efx):
    d = efx.Decoder(max_streams=2, max_pictures=2, ring_depth=3)
    yield d
    d.close()


def src_bytes(fmt, w, h):
    return w * h * 3 // 2 if fmt == "i420" else w * h * 3


def run_detect(dec, src, fmt, w, h, per, limit=24, rnd=16, full=False, src_stride=None, sums_stride=0, with_sums=True,
               src_fill=0, tail=0):
    """One efx_detect_crop over src (n, bytes): (sums (n, sums_stride or h + w rounded up to 4) uint32 or None, records
    (n_streams + tail, 8) int32).  The source gaps hold src_fill, the sums buffer SUMS_FILL, `tail` more records and one
    more image's room of sums behind the outputs hold their fill, for the caller to check."""
    n, size = src.shape
    stride = src_stride or (size + 15) // 16 * 16
    host = np.full((n + 1, stride), src_fill, dtype=np.uint8)
    host[:n, :size] = src
    sbuf = dec.alloc((n + 1) * stride)
    sbuf.upload(host)
    n_streams = n // per
    ss = sums_stride or (h + w + 3) // 4 * 4
    rbuf = dec.alloc(32 * (n_streams + tail))
    rbuf.upload(np.full(8 * (n_streams + tail), 0x5A5A5A5A, dtype=np.int32))
    ubuf = None
    if with_sums:
        ubuf = dec.alloc(4 * ss * (n + 1))
        ubuf.upload(np.full(ss * (n + 1), SUMS_FILL, dtype=np.uint32))
    try:
        dec.detect_crop_to(sbuf, rbuf, n_streams=n_streams, images_per_stream=per, fmt=fmt, width=w, height=h, limit=limit,
                           round=rnd, full_range=full, src_stride=0 if src_stride is None else src_stride, sums=ubuf,
                           sums_stride=sums_stride)
        dec.sync()
        recs = rbuf.download(np.int32, 8 * (n_streams + tail)).reshape(-1, 8)
        sums = ubuf.download(np.uint32, ss * (n + 1)).reshape(n + 1, ss) if with_sums else None
        return sums, recs
    finally:
        for b in (sbuf, rbuf, ubuf):
            if b is not None:
                b.free()


def assert_sums(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} sums differ, first (image, index) = {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])] if bad.size else ''} != {want[tuple(bad[0])] if bad.size else ''}"


GEOMETRIES = [
    # fmt, width, height, streams, images per stream, full range
    ("rgbp", 2, 2, 2, 3, False),
    ("i420", 16, 16, 2, 3, False),
    ("rgb24", 333, 77, 2, 3, False),
    ("rgb24", 333, 77, 2, 3, True),
    ("i420", 354, 194, 2, 3, False),
    ("rgb24", 1920, 1080, 2, 3, False),
    ("rgbp", 353, 193, 2, 3, False),
    ("i420", 4096, 4096, 1, 1, False),
    ("rgb24", 30, 4094, 2, 3, False),
]


def noise_case(fmt, w, h, n_streams, per, full):
    """Noise images, limit = floor(mean luma of the case's images), and the model's sums and records."""
    rng = np.random.default_rng(w * 31 + h + int(full))
    # (studio-swing RGB: components 0 .. 250 have a mean luma near 123.4, uniform bytes one near 125.6 -- floor() of that
    # would leave the limit 0.6 below the mean, most of a standard deviation of the 4094-row column sums)
    top = 251 if fmt != "i420" and not full else 256
    src = rng.integers(0, top, (n_streams * per, src_bytes(fmt, w, h)), dtype=np.uint8)
    want_sums, _ = M.detect(src, fmt, w, h, per, 0, 16, full)
    limit = int(want_sums[:, :h].sum() // (len(src) * w * h))
    _, want_recs = M.detect(src, fmt, w, h, per, limit, 16, full)
    return src, limit, want_sums, want_recs


@pytest.mark.parametrize("fmt,w,h,n_streams,per,full", GEOMETRIES)
def test_geometry_matrix(dec, fmt, w, h, n_streams, per, full):
    src, limit, want_sums, want_recs = noise_case(fmt, w, h, n_streams, per, full)
    # the limit sits in the middle of the sums: an off-by-one byte in any edge line flips a classification
    rows = np.concatenate([M.classify(s, w, h, limit)[0] for s in want_sums])
    cols = np.concatenate([M.classify(s, w, h, limit)[1] for s in want_sums])
    for cls in (rows, cols):
        assert 0.2 <= cls.mean() <= 0.8, (fmt, w, h, limit, float(cls.mean()))
    sums, recs = run_detect(dec, src, fmt, w, h, per, limit=limit, full=full)
    assert_sums(sums[:-1, :h + w], want_sums, f"{fmt} {w}x{h}")
    assert np.array_equal(recs, want_recs), (recs.tolist(), want_recs.tolist())
    # the library's own scratch gives the same records
    _, recs = run_detect(dec, src, fmt, w, h, per, limit=limit, full=full, with_sums=False)
    assert np.array_equal(recs, want_recs)


@pytest.mark.parametrize("fmt,w,h", [("rgb24", 320, 180), ("i420", 64, 48), ("rgbp", 80, 50)])
def test_padded_strides(dec, fmt, w, h):
    """src_stride = size + 64 with 0xFF in the gaps, a sums_stride larger than needed: the same results, and nothing
    between or behind the outputs is written."""
    n_streams, per = 2, 3
    src, limit, want_sums, want_recs = noise_case(fmt, w, h, n_streams, per, False)
    size = src.shape[1]
    assert size % 16 == 0
    ss = (h + w + 3) // 4 * 4 + 8
    sums, recs = run_detect(dec, src, fmt, w, h, per, limit=limit, src_stride=size + 64, sums_stride=ss, src_fill=0xFF, tail=2)
    assert_sums(sums[:-1, :h + w], want_sums, f"padded {fmt}")
    assert (sums[:-1, h + w:] == SUMS_FILL).all() and (sums[-1] == SUMS_FILL).all()
    assert np.array_equal(recs[:n_streams], want_recs)
    assert (recs[n_streams:] == 0x5A5A5A5A).all()


def boxed(rng, fmt, w, h, box):
    """One picture: bright noise inside box = (x1, y1, x2, y2) inclusive, black outside (None: all black).  RGB black
    is 0, 0, 0; I420 black is Y 16 with noise in the chroma planes, which the detector never reads."""
    if fmt == "i420":
        p = np.full((h, w), 16, dtype=np.uint8)
        if box:
            x1, y1, x2, y2 = box
            p[y1:y2 + 1, x1:x2 + 1] = rng.integers(60, 256, (y2 + 1 - y1, x2 + 1 - x1))
        return np.concatenate([p.reshape(-1), rng.integers(0, 256, w * h // 2, dtype=np.uint8)])
    p = np.zeros((h, w, 3), dtype=np.uint8)
    if box:
        x1, y1, x2, y2 = box
        p[y1:y2 + 1, x1:x2 + 1] = rng.integers(60, 256, (y2 + 1 - y1, x2 + 1 - x1, 3))
    return (p if fmt == "rgb24" else p.transpose(2, 0, 1)).reshape(-1)


# five streams of three pictures each; a stream is a list of boxes
STRUCTURED_A = ("i420", 1920, 1080, False, 24, [
    [(0, 140, 1919, 939)] * 3,        # letterboxed: picture rows 140 .. 939
    [(240, 0, 1679, 1079)] * 3,       # pillarboxed
    [(200, 100, 1719, 979)] * 3,      # windowboxed
    [(0, 0, 1919, 1079)] * 3,         # to the edges: the whole picture, rounded
    [(1, 1, 1918, 1078)] * 3,         # bars of exactly one line
])
STRUCTURED_B = ("rgb24", 333, 77, True, 0, [
    [(7, 3, 301, 61)] * 3,                                        # bounds on odd coordinates
    [(100, 10, 100, 60)] * 3,                                     # a strip one column wide: the x axis fails
    [(20, 6, 280, 70), None, (20, 6, 280, 70)],                   # an all-black image between two contributing ones
    [None, None, None],                                           # an all-black stream
    [(20, 5, 200, 50), (40, 2, 300, 40), (10, 20, 150, 70)],      # different bars: the union
])
STRUCTURED_WANT = {
    # (set, round): stream -> record, worked out by hand from the definition
    ("A", 16): {0: [0, 140, 1920, 800, 0, 140, 1919, 939], 3: [0, 4, 1920, 1072, 0, 0, 1919, 1079],
                4: [8, 4, 1904, 1072, 1, 1, 1918, 1078]},
    ("A", 2): {0: [0, 140, 1920, 800, 0, 140, 1919, 939], 3: [0, 0, 1920, 1080, 0, 0, 1919, 1079],
               4: [2, 2, 1916, 1076, 1, 1, 1918, 1078]},
    ("B", 2): {0: [8, 4, 294, 58, 7, 3, 301, 61], 1: [0, 0, 333, 77, 100, 10, 100, 60], 2: [20, 6, 260, 64, 20, 6, 280, 70],
               3: [0, 0, 333, 77, 333, 77, -1, -1], 4: [10, 2, 290, 68, 10, 2, 300, 70]},
    ("B", 16): {1: [0, 0, 333, 77, 100, 10, 100, 60], 3: [0, 0, 333, 77, 333, 77, -1, -1],
                4: [10, 4, 288, 64, 10, 2, 300, 70]},
}


@pytest.mark.parametrize("name,case", [("A", STRUCTURED_A), ("B", STRUCTURED_B)])
def test_structured_pictures(dec, name, case):
    fmt, w, h, full, limit, streams = case
    rng = np.random.default_rng(len(name) + w)
    src = np.stack([boxed(rng, fmt, w, h, box) for stream in streams for box in stream])
    for rnd in (2, 16):
        want_sums, want_recs = M.detect(src, fmt, w, h, 3, limit, rnd, full)
        for stream, rec in STRUCTURED_WANT[(name, rnd)].items():
            assert want_recs[stream].tolist() == rec, (name, rnd, stream)
        sums, recs = run_detect(dec, src, fmt, w, h, 3, limit=limit, rnd=rnd, full=full)
        assert_sums(sums[:-1, :h + w], want_sums, f"structured {name}")
        assert np.array_equal(recs, want_recs), (rnd, recs.tolist(), want_recs.tolist())
        assert len({tuple(r) for r in recs.tolist()}) == len(streams)
        x, y, rw, rh = recs[:, 0], recs[:, 1], recs[:, 2], recs[:, 3]
        assert not ((x | y) & 1).any() and (x >= 0).all() and (y >= 0).all() and (x + rw <= w).all() and (y + rh <= h).all()


@pytest.mark.parametrize("limit", [0, 24, 255])
def test_threshold_edge(dec, limit):
    """A row of W pixels at `limit` is black, the same row with one pixel at limit + 1 is picture; likewise a column."""
    w, h = 64, 48
    def image(extra):
        p = np.full((h, w), limit, dtype=np.uint8)
        for x, y in extra:
            p[y, x] = limit + 1
        return np.concatenate([p.reshape(-1), np.full(w * h // 2, 128, dtype=np.uint8)])
    extras = [[]] if limit == 255 else [[], [(9, 5)], [(9, 5), (40, 30)], [(63, 0), (0, 47)]]
    src = np.stack([image(e) for e in extras])
    sums, recs = run_detect(dec, src, "i420", w, h, 1, limit=limit, rnd=2)
    want_sums, want_recs = M.detect(src, "i420", w, h, 1, limit, 2)
    assert_sums(sums[:-1, :h + w], want_sums, "threshold")
    assert np.array_equal(recs, want_recs)
    assert recs[0].tolist() == [0, 0, w, h, w, h, -1, -1]      # every sum equals limit x n: black
    if limit < 255:
        assert recs[1].tolist() == [0, 0, w, h, 9, 5, 9, 5]     # one row and one column one above: picture
        assert recs[2].tolist() == [10, 6, 30, 24, 9, 5, 40, 30]
        assert recs[3].tolist() == [0, 0, w, h, 0, 0, 63, 47]
    # at 255 nothing is ever picture, whatever the image holds
    if limit == 255:
        rng = np.random.default_rng(1)
        noise = rng.integers(250, 256, (2, w * h * 3 // 2), dtype=np.uint8)
        _, recs = run_detect(dec, noise, "i420", w, h, 2, limit=255)
        assert recs[0].tolist() == [0, 0, w, h, w, h, -1, -1]


def test_saturated_image(dec):
    w = h = 4096
    src = np.full((1, w * h * 3 // 2), 255, dtype=np.uint8)
    sums, recs = run_detect(dec, src, "i420", w, h, 1, limit=254)
    assert (sums[0, :h + w] == 1044480).all()
    assert recs[0].tolist() == [0, 0, w, h, 0, 0, w - 1, h - 1]


def test_many_streams_and_scratch_growth(dec):
    """256 streams of one image: the grid and the stream indexing; then the library's scratch, small, large, small."""
    n, w, h = 256, 64, 48
    rng = np.random.default_rng(9)
    boxes = [(i % 29, i % 13, 34 + (i * 7) % 30, 20 + (i * 5) % 28) for i in range(n)]
    src = np.stack([boxed(rng, "rgb24", w, h, b) for b in boxes])
    want_sums, want_recs = M.detect(src, "rgb24", w, h, 1, 24, 2)
    assert len({tuple(r) for r in want_recs.tolist()}) > 200
    sums, recs = run_detect(dec, src, "rgb24", w, h, 1, rnd=2)
    assert_sums(sums[:-1, :h + w], want_sums, "256 streams")
    assert np.array_equal(recs, want_recs)
    for count in (4, 256, 8):
        _, recs = run_detect(dec, src[:count], "rgb24", w, h, 1, rnd=2, with_sums=False)
        assert np.array_equal(recs, want_recs[:count]), count
    _, recs = run_detect(dec, src, "rgb24", w, h, 64, rnd=2, with_sums=False)
    assert np.array_equal(recs, M.detect(src, "rgb24", w, h, 64, 24, 2)[1])


def test_python_surface(efx, dec):
    """detect_crop on arrays of every format against detect_crop_to; import_pictures(crop="auto") with fit="cover" and
    fit="letterbox" against the import model called with the model's rectangle; unknown strings."""
    w, h, n = 200, 120, 4
    rng = np.random.default_rng(21)
    boxes = [(30, 11, 169, 100), (32, 14, 160, 101), None, (31, 13, 171, 98)]
    flat = np.stack([boxed(rng, "rgb24", w, h, b) for b in boxes])
    rgb = flat.reshape(n, h, w, 3)
    _, want1 = M.detect(flat, "rgb24", w, h, None, 24, 16)
    _, want2 = M.detect(flat, "rgb24", w, h, 2, 24, 2)
    assert want1[0].tolist() == [36, 16, 128, 80, 30, 11, 171, 101]
    _, direct = run_detect(dec, flat, "rgb24", w, h, n)
    got = dec.detect_crop(rgb)
    assert got.dtype == np.int32 and got.shape == (1, 8) and np.array_equal(got, want1) and np.array_equal(got, direct)
    assert np.array_equal(dec.detect_crop(rgb, images_per_stream=2, round=2), want2)
    chw = np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))
    assert np.array_equal(dec.detect_crop(chw), want1)
    yuv = np.stack([boxed(rng, "i420", w, h, b) for b in boxes])
    assert np.array_equal(dec.detect_crop(yuv, width=w, height=h, limit=30, round=4), M.detect(yuv, "i420", w, h, None, 30, 4)[1])
    with pytest.raises(ValueError):
        dec.detect_crop(rgb, images_per_stream=3)
    with pytest.raises(ValueError):
        dec.detect_crop(yuv)

    crop = tuple(int(v) for v in want1[0, :4])
    cover = M.cover_crop(w, h, crop)
    assert cover == (36, 22, 128, 68) and efx.cover_crop(w, h, crop) == cover
    got = dec.import_pictures(rgb, crop="auto", fit="cover")
    assert np.array_equal(got, import_model.import_images(flat, "rgb24", w, h, cover))
    got = dec.import_pictures(rgb, crop="auto", fit="letterbox")
    assert np.array_equal(got, import_model.import_images(flat, "rgb24", w, h, crop, import_model.letterbox_rect(128, 80)))
    got = dec.import_pictures(yuv, width=w, height=h, crop="auto", crop_limit=30, crop_round=4)
    crop4 = tuple(int(v) for v in M.detect(yuv, "i420", w, h, None, 30, 4)[1][0, :4])
    assert np.array_equal(got, import_model.import_images(yuv, "i420", w, h, crop4))
    got = dec.import_pictures(rgb, crop=(10, 20, 180, 40), fit="cover")
    assert np.array_equal(got, import_model.import_images(flat, "rgb24", w, h, M.cover_crop(w, h, (10, 20, 180, 40))))
    got = dec.import_pictures(rgb, fit="cover")
    assert np.array_equal(got, import_model.import_images(flat, "rgb24", w, h, M.cover_crop(w, h)))
    for bad in (dict(fit="fill"), dict(fit="auto"), dict(crop="detect"), dict(crop="")):
        with pytest.raises(ValueError):
            dec.import_pictures(rgb, **bad)


def test_queued_detection_and_import(dec):
    """detect_crop_to, import_to and a second detect_crop_to of another geometry queued on the stream without a sync in
    between: every result is right."""
    rng = np.random.default_rng(5)
    w, h, n = 333, 77, 3
    a = np.stack([boxed(rng, "rgb24", w, h, (21, 9, 300, 66)) for _ in range(n)])
    b = np.stack([boxed(rng, "i420", 64, 48, (10, 4, 50, 40)) for _ in range(n)])
    bufs = []
    def up(src):
        size = src.shape[1]
        stride = (size + 15) // 16 * 16
        host = np.zeros((len(src), stride), dtype=np.uint8)
        host[:, :size] = src
        buf = dec.alloc(host.size)
        buf.upload(host)
        bufs.append(buf)
        return buf
    sa, sb = up(a), up(b)
    ra, rb, pics = dec.alloc(32), dec.alloc(32), dec.alloc(n * import_model.FRAME_BYTES)
    bufs += [ra, rb, pics]
    dec.detect_crop_to(sa, ra, n_streams=1, images_per_stream=n, fmt="rgb24", width=w, height=h, full_range=True, limit=0)
    dec.import_to(sa, pics, n_images=n, fmt="rgb24", width=w, height=h, crop=(22, 10, 272, 56))
    dec.detect_crop_to(sb, rb, n_streams=1, images_per_stream=n, fmt="i420", width=64, height=48, round=2)
    dec.sync()
    assert np.array_equal(ra.download(np.int32, 8), M.detect(a, "rgb24", w, h, None, 0, 16, True)[1][0])
    assert ra.download(np.int32, 8).tolist() == [24, 14, 272, 48, 21, 9, 300, 66]
    assert np.array_equal(rb.download(np.int32, 8), M.detect(b, "i420", 64, 48, None, 24, 2)[1][0])
    got = pics.download(np.uint8, n * import_model.FRAME_BYTES).reshape(n, -1)
    assert np.array_equal(got, import_model.import_images(a, "rgb24", w, h, (22, 10, 272, 56)))
    for buf in bufs:
        buf.free()


def test_argument_errors(efx, dec):
    lib, ctx = dec._lib, dec._ctx
    src, rects, sums = dec.alloc(1 << 20), dec.alloc(1024), dec.alloc(1 << 16)
    I420, RGB24, RGBP = efx.PIX_I420, efx.PIX_RGB24, efx.PIX_RGBP

    def call(s=src.ptr, r=rects.ptr, u=sums.ptr, ns=2, per=3, fmt=RGB24, w=64, h=48, full=0, limit=24, rnd=16, ss=0, us=0):
        o = efx._CropOpts(ns, per, fmt, w, h, full, limit, rnd, ss, us)
        return lib.efx_detect_crop(ctx, C.byref(o), s, r, u)

    assert call() == 0 and call(u=None) == 0
    assert call(s=None) == ARG and call(r=None) == ARG
    assert call(s=src.ptr + 8) == ARG and call(r=rects.ptr + 4) == ARG and call(u=sums.ptr + 8) == ARG
    assert lib.efx_detect_crop(ctx, None, src.ptr, rects.ptr, None) == ARG
    assert call(ns=0) == ARG and call(ns=-1) == ARG and call(per=0) == ARG and call(per=-2) == ARG
    assert call(ns=1 << 16, per=1 << 15) == ARG and call(ns=(1 << 31) - 1, per=2) == ARG
    assert call(fmt=3) == ARG and call(fmt=-1) == ARG
    assert call(w=1) == ARG and call(h=1) == ARG and call(w=4097) == ARG and call(h=4097) == ARG and call(w=0) == ARG
    assert call(fmt=I420, w=63) == ARG and call(fmt=I420, h=47) == ARG and call(fmt=I420) == 0 and call(w=63, h=47) == 0
    assert call(fmt=RGBP, w=63, h=47) == 0
    assert call(limit=-1) == ARG and call(limit=256) == ARG and call(limit=0) == 0 and call(limit=255) == 0
    assert call(rnd=0) == ARG and call(rnd=1) == ARG and call(rnd=15) == ARG and call(rnd=66) == ARG and call(rnd=-2) == ARG
    assert call(rnd=2) == 0 and call(rnd=64) == 0
    size = 64 * 48 * 3
    assert call(ss=size - 16) == ARG and call(ss=size + 8) == ARG and call(ss=size + 16) == 0
    assert call(w=63, h=47, ss=63 * 47 * 3) == ARG and call(w=63, h=47, ss=(63 * 47 * 3 + 15) // 16 * 16) == 0
    assert call(us=108) == ARG and call(us=114) == ARG and call(us=112) == 0 and call(us=116) == 0
    assert call(w=63, h=47, us=108) == ARG and call(w=63, h=47, us=112) == 0
    dec.sync()
    for b in (src, rects, sums):
        b.free()
    with pytest.raises(ValueError):
        dec.detect_crop_to(0, 0, n_streams=1, images_per_stream=1, fmt="yuv444", width=16, height=16)
    with pytest.raises(efx.EfxError) as e:
        dec.detect_crop_to(0, 0, n_streams=1, images_per_stream=1, fmt="rgb24", width=16, height=16)
    assert e.value.status == ARG


TORCH_CHILD = textwrap.dedent("""
    import os
    import sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
    import espflix_amd as efx
    import crop_model as M
    import import_model

    torch.cuda.set_stream(torch.cuda.Stream())
    dec = efx.Decoder(2, 2, device=torch.cuda.current_device(), hip_stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(13)
    checked = 0
    for n, h, w in ((4, 77, 333), (2, 360, 640)):   # (an image size that is no multiple of 16, and one that is)
        host = np.zeros((n, h, w, 3), dtype=np.uint8)
        for i in range(n):
            host[i, 9 + i:h - 7, 41:w - 30 - i] = rng.integers(60, 256, (h - 16 - i, w - 71 - i, 3))
        flat = host.reshape(n, -1)
        want = M.detect(flat, "rgb24", w, h, 2, 24, 16)[1]
        t = torch.from_numpy(host).cuda()
        got = dec.detect_crop(t, images_per_stream=2)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want)
        assert np.array_equal(dec.detect_crop(host, images_per_stream=2), want)
        chw = t.permute(0, 3, 1, 2).contiguous()
        assert np.array_equal(dec.detect_crop(chw, images_per_stream=2), want)
        crop = tuple(int(v) for v in M.detect(flat, "rgb24", w, h, None, 24, 16)[1][0, :4])
        pics = dec.import_pictures(t, crop="auto", fit="cover", sync=False)
        assert isinstance(pics, torch.Tensor)
        assert np.array_equal(pics.cpu().numpy(), import_model.import_images(flat, "rgb24", w, h, M.cover_crop(w, h, crop)))
        checked += 1
    dec.close()
    print("torch crop ok", checked)
""")


def test_torch_tensor_input(efx, tmp_path):
    """In a child process (torch's HIP runtime must come up first): detect_crop and import_pictures(crop="auto") on
    cuda tensors agree with the array path and the model."""
    script = tmp_path / "torch_crop.py"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch crop ok 2" in r.stdout
