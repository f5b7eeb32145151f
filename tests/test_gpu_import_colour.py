"""The import's colour conversion on the device (efx_import_set_colour; k_import_surf*_c): BT.709, full-range and other
YCbCr sources to BT.601 studio swing inside the import kernels.  The expected bytes are always
colour_model.convert(import_model.import_images(...)), bit for bit (tests/colour_model.py, tests/import_model.py,
tests/surface_model.py)."""
import ctypes as C

import numpy as np
import pytest

import colour_model as K
import import_model as M
import surface_model as S

pytestmark = pytest.mark.gpu

ARG = -1
BLACK = (16, 128, 128)


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def dec(efx):
    d = efx.Decoder(max_streams=16, max_pictures=4, ring_depth=5)
    yield d
    d.close()


def assert_same(got, want, what):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first (image, byte) = {bad[0].tolist()}"


def converted(plain, rect, code, full, height):
    return K.convert(plain, rect, *K.coefs(code, full, height))


def random_i420(n, w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, w * h * 3 // 2), dtype=np.uint8)


def import_i420(dec, src, w, h, rect=None, crop=None, **kw):
    """import_to on packed I420 images: (n, 101376)."""
    n, size = src.shape
    stride = (size + 15) // 16 * 16
    host = np.zeros((n, stride), dtype=np.uint8)
    host[:, :size] = src
    sbuf, dbuf = dec.alloc(n * stride), dec.alloc(n * M.FRAME_BYTES)
    try:
        sbuf.upload(host)
        dec.import_to(sbuf, dbuf, n_images=n, fmt="i420", width=w, height=h, crop=crop, dst_rect=rect, src_stride=stride, **kw)
        dec.sync()
        return dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES)
    finally:
        sbuf.free()
        dbuf.free()


def set_colour(efx, dec, code, full):
    return dec._lib.efx_import_set_colour(dec._ctx, C.byref(efx._ImportColour(code, full)))


@pytest.mark.parametrize("code,full", [(c, r) for c in (1, 4, 7, 9) for r in (0, 1)] + [(6, 1)])
def test_matrices_and_ranges(dec, code, full):
    """Uniformly random bytes 0 .. 255, so every clamp is reached."""
    w, h = 64, 48
    src = random_i420(3, w, h, 100 + code)
    got = dec.import_pictures(src, fmt="i420", width=w, height=h, fit="stretch", matrix=code, src_range="full" if full else "studio")
    plain = M.import_images(src, "i420", w, h)
    want = converted(plain, None, code, full, h)
    assert_same(got, want, f"matrix {code} range {full}")
    assert not np.array_equal(want, plain)


@pytest.mark.parametrize("rect", [(18, 6, 36, 20), (336, 176, 16, 16)])
def test_rectangles(dec, rect):
    """BT.709 full range into a rectangle that begins and ends inside a band and inside a lane's column pair, and into
    the smallest rectangle at the frame's bottom-right corner: every byte outside is (16, 128, 128)."""
    w, h = 64, 48
    src = random_i420(3, w, h, 7 + rect[0])
    got = import_i420(dec, src, w, h, rect, matrix="bt709", src_range="full")
    assert_same(got, converted(M.import_images(src, "i420", w, h, None, rect), rect, 1, 1, h), f"rectangle {rect}")
    x, y, rw, rh = rect
    for plane, (off, pw, ph, s) in enumerate(((0, M.W, M.H, 1), (M.Y_BYTES, M.CW, M.CH, 2), (M.Y_BYTES + M.C_BYTES, M.CW, M.CH, 2))):
        p = got[:, off:off + pw * ph].reshape(3, ph, pw)
        outside = np.ones((ph, pw), dtype=bool)
        outside[y // s:(y + rh) // s, x // s:(x + rw) // s] = False
        assert (p[:, outside] == BLACK[plane]).all()


@pytest.mark.parametrize("kind,pitch", [("nv12", 50), ("nv21", 50), ("p010", 74), ("i010", 80), ("yv12", 38)])
def test_layouts(efx, dec, kind, pitch):
    """Every surface kernel: a pitch wider than a row, plane rows above the height, a crop at odd multiples of 2."""
    w, h, rows, n, crop = 34, 18, 20, 3, (2, 6, 28, 10)
    s = S.layout(kind, w, h, pitch, rows)
    src = S.sources(n, s, 55 + pitch)
    got = dec.import_pictures(src, fmt=kind, width=w, height=h, pitch=pitch, plane_rows=rows, crop=crop, matrix="bt709", src_range="studio")
    plain = S.import_images(src, s, crop)
    assert_same(got, converted(plain, None, 1, 0, h), kind)
    assert not np.array_equal(got, plain)


def test_off(efx, dec):
    w, n = 16, 2
    for h in (576, 578):
        src = random_i420(n, w, h, h)
        plain = M.import_images(src, "i420", w, h)
        kw = dict(fmt="i420", width=w, height=h)
        got709 = dec.import_pictures(src, matrix="bt709", **kw)          # a converted call first
        assert_same(got709, converted(plain, None, 1, 0, h), "bt709")
        assert_same(dec.import_pictures(src, matrix=None, **kw), plain, "None after a converted call")
        assert_same(dec.import_pictures(src, matrix="bt601", **kw), plain, "bt601")
        assert_same(dec.import_pictures(src, matrix=6, src_range="studio", **kw), plain, "code 6 studio")
        assert_same(dec.import_pictures(src, matrix="auto", **kw), plain if h == 576 else got709, f"auto at {h} lines")
    # an RGB import ignores a conversion set on the context
    rgb = np.random.default_rng(4).integers(0, 256, (2, 20, 24, 3), dtype=np.uint8)
    want = M.import_images(rgb, "rgb24", 24, 20)
    assert set_colour(efx, dec, 1, 1) == 0
    try:
        assert_same(dec.import_pictures(rgb), want, "rgb24 with a conversion set")
    finally:
        assert dec._lib.efx_import_set_colour(dec._ctx, None) == 0
    for kw in (dict(matrix="bt709"), dict(src_range="full")):
        with pytest.raises(ValueError):
            dec.import_pictures(rgb, **kw)
    with pytest.raises(ValueError):
        dec.import_pictures(random_i420(1, 16, 16, 1), fmt="i420", width=16, height=16, matrix="bt470")


def test_queued_calls_keep_their_matrix(dec):
    """Two calls of different matrices into different outputs without a synchronisation between them."""
    w, h, n = 64, 48, 2
    src = random_i420(n, w, h, 21)
    sbuf = dec.alloc(src.size)
    sbuf.upload(src)
    jobs = [(1, 0, dec.alloc(n * M.FRAME_BYTES)), (9, 1, dec.alloc(n * M.FRAME_BYTES))]
    for code, full, dbuf in jobs:
        dec.import_to(sbuf, dbuf, n_images=n, fmt="i420", width=w, height=h, matrix=code, src_range="full" if full else "studio")
    dec.sync()
    plain = M.import_images(src, "i420", w, h)
    for code, full, dbuf in jobs:
        assert_same(dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES), converted(plain, None, code, full, h), f"queued {code}")
        dbuf.free()
    sbuf.free()


def test_setting_that_stays(dec):
    """set_import_colour() holds for the calls that follow; a call's own matrix= overrides it for that call only."""
    w, h = 64, 48
    src = random_i420(2, w, h, 5)
    plain = M.import_images(src, "i420", w, h)
    kw = dict(fmt="i420", width=w, height=h)
    dec.set_import_colour("bt709", "full")
    try:
        assert_same(dec.import_pictures(src, **kw), converted(plain, None, 1, 1, h), "the setting")
        assert_same(dec.import_pictures(src, matrix="smpte240m", **kw), converted(plain, None, 7, 0, h), "the call's own")
        assert_same(dec.import_pictures(src, matrix="bt601", **kw), plain, "the call's own: off")
        assert_same(dec.import_pictures(src, **kw), converted(plain, None, 1, 1, h), "the setting again")
        with pytest.raises(ValueError):
            dec.set_import_colour("bt470")
        assert_same(dec.import_pictures(src, **kw), converted(plain, None, 1, 1, h), "after a rejected setting")
    finally:
        dec.set_import_colour()
    assert_same(dec.import_pictures(src, **kw), plain, "switched off")


def test_bars_on_the_device(dec):
    """The six BT.709 bars, white and black as flat 16 x 16 NV12 surfaces: within +-1 of the BT.601 triples (which do not
    depend on the code under test) and exactly the model's."""
    bars = [(b709, b601) for _, b709, b601 in K.BARS] + [((235, 128, 128), (235, 128, 128)), (BLACK, BLACK)]
    s = S.layout("nv12", 16, 16)
    src = np.zeros((len(bars), s.bytes), dtype=np.uint8)
    for i, ((y, cb, cr), _) in enumerate(bars):
        src[i, :256] = y
        src[i, 256::2], src[i, 257::2] = cb, cr
    got = dec.import_pictures(src, fmt="nv12", width=16, height=16, matrix="bt709")
    assert_same(got, converted(S.import_images(src, s), None, 1, 0, 16), "bars")
    for i, (_, b601) in enumerate(bars):
        planes = (got[i, :M.Y_BYTES], got[i, M.Y_BYTES:M.Y_BYTES + M.C_BYTES], got[i, M.Y_BYTES + M.C_BYTES:])
        for p, want in zip(planes, b601):
            assert np.abs(p.astype(int) - want).max() <= 1, (i, want, int(p.min()), int(p.max()))


def test_errors_leave_the_setting(efx, dec):
    w, h = 64, 48
    src = random_i420(2, w, h, 33)
    assert set_colour(efx, dec, 1, 1) == 0
    try:
        for code, full in ((0, 0), (3, 0), (8, 0), (10, 0), (1, 2), (1, -1)):
            assert set_colour(efx, dec, code, full) == ARG, (code, full)
            assert dec._lib.efx_last_error(dec._ctx).startswith(b"efx_import_set_colour: ")
        # the next import still runs with the previous setting
        assert_same(import_i420(dec, src, w, h), converted(M.import_images(src, "i420", w, h), None, 1, 1, h), "after the errors")
    finally:
        assert dec._lib.efx_import_set_colour(dec._ctx, None) == 0
    assert_same(import_i420(dec, src, w, h), M.import_images(src, "i420", w, h), "switched off")
    q, y0 = (C.c_int32 * 9)(), C.c_int()
    for code, full in ((0, 0), (3, 0), (8, 0), (10, 0), (1, 2)):
        assert dec._lib.efx_import_colour_coefs(code, full, 1080, q, C.byref(y0)) == ARG
    assert dec._lib.efx_import_colour_coefs(1, 0, 1080, None, C.byref(y0)) == ARG
    with pytest.raises(efx.EfxError) as e:
        import_i420(dec, src, w, h, matrix=8)
    assert e.value.status == ARG


def test_crop_of_a_full_range_source(dec):
    """Borders of luma 0 .. 9 around content of luma >= 40, full range: detect_crop(src_range="full") finds what
    detect_crop finds on the same picture mapped to studio swing, and import_pictures(crop="auto") cuts it off."""
    w, h, box = 64, 48, (8, 6, 48, 36)
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, (1, w * h * 3 // 2), dtype=np.uint8)
    y = rng.integers(0, 10, (h, w), dtype=np.uint8)
    y[box[1]:box[1] + box[3], box[0]:box[0] + box[2]] = rng.integers(40, 256, (box[3], box[2]), dtype=np.uint8)
    src[0, :w * h] = y.reshape(-1)
    q, y0 = K.coefs(6, 1)
    studio = src.copy()
    studio[0, :w * h] = K.convert_px(q, y0, y.reshape(-1), 128, 128)[0]
    kw = dict(fmt="i420", width=w, height=h)
    got = dec.detect_crop(src, src_range="full", **kw)
    assert np.array_equal(got, dec.detect_crop(studio, **kw))
    assert tuple(got[0, 4:]) == (box[0], box[1], box[0] + box[2] - 1, box[1] + box[3] - 1)
    crop = tuple(int(v) for v in got[0, :4])
    # a dim frame of luma 15 around the content is picture in full range (it converts to 29) and black at the plain limit
    dim = src.copy()
    yd = y.copy()
    yd[4:44, 4:60] = np.maximum(yd[4:44, 4:60], 15)
    dim[0, :w * h] = yd.reshape(-1)
    assert tuple(dec.detect_crop(dim, src_range="full", **kw)[0, 4:]) == (4, 4, 59, 43)
    assert tuple(dec.detect_crop(dim, **kw)[0, 4:]) == tuple(got[0, 4:])
    pic = dec.import_pictures(src, crop="auto", matrix="bt709", src_range="full", **kw)
    assert_same(pic, converted(M.import_images(src, "i420", w, h, crop), None, 1, 1, h), "crop=auto of a full-range source")
