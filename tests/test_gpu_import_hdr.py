"""The import's HDR stage on the device (efx_import_set_hdr; k_import_surf*_h): HDR10 sources (PQ, BT.2020) tone-mapped to
BT.601 SDR inside the import kernels.  The expected bytes are always hdr_model.import_images(...) -- tonemap(import10(the
canonical image)) -- fed with the library's own tables, bit for bit (tests/hdr_model.py, tests/surface_model.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import colour_model as K
import hdr_model as H
import import_model as M
import surface_model as S

pytestmark = pytest.mark.gpu

ARG = -1
RECT = (6, 10, 100, 52)   # starts and ends inside bands, leaves bands fully outside


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


@functools.lru_cache(maxsize=None)
def setting(peak=1000, full=0, prim=9, matrix=9, height=0):
    """The model's setting with the library's own tables."""
    import espflix_amd
    t = espflix_amd.hdr_tables(peak, primaries=prim, matrix=matrix, src_range="full" if full else "studio", height=height)
    return H.Setting(peak, full, prim, matrix, height, pq=t["pq"], gam=t["gamma"])


def assert_same(got, want, what):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first (image, byte) = {bad[0].tolist()}"


def random_i420(n, w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, w * h * 3 // 2), dtype=np.uint8)


def import_i420(dec, src, w, h, rect=None, **kw):
    """import_to (efx_import_frames) on packed I420 images: (n, 101376)."""
    n, size = src.shape
    stride = (size + 15) // 16 * 16
    host = np.zeros((n, stride), dtype=np.uint8)
    host[:, :size] = src
    sbuf, dbuf = dec.alloc(n * stride), dec.alloc(n * M.FRAME_BYTES)
    try:
        sbuf.upload(host)
        dec.import_to(sbuf, dbuf, n_images=n, fmt="i420", width=w, height=h, dst_rect=rect, src_stride=stride, **kw)
        dec.sync()
        return dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES)
    finally:
        sbuf.free()
        dbuf.free()


def set_hdr(efx, dec, transfer=16, primaries=9, matrix=9, full=0, peak=1000):
    return dec._lib.efx_import_set_hdr(dec._ctx, C.byref(efx._ImportHdr(transfer, primaries, matrix, full, peak)))


# kind, pitch, plane rows: I420 pitched, NV12, I010 (shift 2), P010 (shift 8)
LAYOUTS = [("i420", 80, 50), ("nv12", 0, 0), ("i010", 0, 0), ("p010", 144, 50)]


@pytest.mark.parametrize("rect", [None, RECT], ids=["frame", "rect"])
@pytest.mark.parametrize("kind,pitch,rows", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_layouts(dec, kind, pitch, rows, rect):
    """Every _h kernel, a 64 x 48 source into the full frame and into a rectangle: every byte outside is (16, 128, 128)."""
    w, h, n = 64, 48, 2
    s = S.layout(kind, w, h, pitch, rows)
    src = S.sources(n, s, 31 + len(kind) + pitch)
    if rect is None:
        got = dec.import_pictures(src, fmt=kind, width=w, height=h, pitch=pitch, plane_rows=rows, transfer="pq", primaries="bt2020", peak_nits=1000)
    else:
        got = import_surface(dec, src, kind, w, h, pitch, rows, rect, transfer="pq")
    want = H.import_images(setting(), S.canonicals(src, s), w, h, None, rect)
    assert_same(got, want, f"{kind} {rect}")
    assert not np.array_equal(got, S.import_images(src, s, None, rect))


def import_surface(dec, src, kind, w, h, pitch, rows, rect=None, pad=0, **kw):
    """import_to with surface=: images `stride` apart, stride = the surface's bytes rounded up to 16 + pad."""
    import espflix_amd
    sf = espflix_amd.surface_layout(kind, w, h, pitch, rows)
    n = len(src)
    raw = np.ascontiguousarray(src).view(np.uint8).reshape(n, -1)
    stride = (sf.bytes + 15) // 16 * 16 + pad
    host = np.random.default_rng(1).integers(0, 256, (n, stride), dtype=np.uint8)   # noise between the images
    host[:, :sf.bytes] = raw
    sbuf, dbuf = dec.alloc(n * stride), dec.alloc(n * M.FRAME_BYTES)
    try:
        sbuf.upload(host)
        dec.import_to(sbuf, dbuf, n_images=n, fmt="i420", width=w, height=h, dst_rect=rect, src_stride=stride, surface=sf, **kw)
        dec.sync()
        return dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES)
    finally:
        sbuf.free()
        dbuf.free()


def test_rectangle_border(dec):
    w, h = 64, 48
    s = S.layout("nv12", w, h)
    src = S.sources(2, s, 77)
    got = import_surface(dec, src, "nv12", w, h, 0, 0, RECT, transfer="pq", peak_nits=1000)
    x, y, rw, rh = RECT
    for plane, (off, pw, ph, sub, black) in enumerate(((0, M.W, M.H, 1, 16), (M.Y_BYTES, M.CW, M.CH, 2, 128), (M.Y_BYTES + M.C_BYTES, M.CW, M.CH, 2, 128))):
        p = got[:, off:off + pw * ph].reshape(2, ph, pw)
        outside = np.ones((ph, pw), dtype=bool)
        outside[y // sub:(y + rh) // sub, x // sub:(x + rw) // sub] = False
        assert (p[:, outside] == black).all(), plane


def test_half_size(dec):
    """352 x 192 from 704 x 384 P010: both columns of every lane, every band full."""
    w, h = 704, 384
    s = S.layout("p010", w, h)
    src = S.sources(1, s, 5)
    got = dec.import_pictures(src, fmt="p010", width=w, height=h, transfer="pq")
    assert_same(got, H.import_images(setting(), S.canonicals(src, s), w, h), "704 x 384")


def test_smallest_source(dec):
    s = S.layout("p010", 2, 2)
    src = S.sources(3, s, 9)
    got = dec.import_pictures(src, fmt="p010", width=2, height=2, transfer="pq")
    assert_same(got, H.import_images(setting(), S.canonicals(src, s), 2, 2), "2 x 2")


def test_nv21_swaps_the_chroma(dec):
    w, h = 64, 48
    s21, s12 = S.layout("nv21", w, h), S.layout("nv12", w, h)
    src = S.sources(2, s21, 12)
    got = dec.import_pictures(src, fmt="nv21", width=w, height=h, transfer="pq")
    assert_same(got, H.import_images(setting(), S.canonicals(src, s21), w, h), "nv21")
    assert not np.array_equal(got, H.import_images(setting(), S.canonicals(src, s12), w, h))


@pytest.mark.parametrize("prim", [9, 1])
def test_full_range(dec, prim):
    w, h = 64, 48
    s = S.layout("i010", w, h)
    src = S.sources(2, s, 40 + prim)
    got = dec.import_pictures(src, fmt="i010", width=w, height=h, transfer="pq", primaries=prim, src_range="full")
    assert_same(got, H.import_images(setting(1000, 1, prim), S.canonicals(src, s), w, h), f"full range, primaries {prim}")
    assert not np.array_equal(got, H.import_images(setting(1000, 0, prim), S.canonicals(src, s), w, h))


@pytest.mark.parametrize("peak", [400, 1000, 4000])
def test_peaks(dec, peak):
    w, h = 64, 48
    s = S.layout("p010", w, h)
    src = S.sources(2, s, peak)
    got = dec.import_pictures(src, fmt="p010", width=w, height=h, transfer="pq", peak_nits=peak, matrix="bt2020")
    assert_same(got, H.import_images(setting(peak), S.canonicals(src, s), w, h), f"peak {peak}")
    other = H.import_images(setting(400 if peak != 400 else 1000), S.canonicals(src, s), w, h)
    assert not np.array_equal(got, other)


def test_other_matrix(dec):
    """The struct carries its own matrix: BT.709 matrix and primaries, and code 2 resolved by the height."""
    w, h = 64, 48
    s = S.layout("nv12", w, h)
    src = S.sources(2, s, 3)
    got = dec.import_pictures(src, fmt="nv12", width=w, height=h, transfer="pq", primaries="bt709", matrix="bt709")
    assert_same(got, H.import_images(setting(1000, 0, 1, 1), S.canonicals(src, s), w, h), "bt709")
    got = dec.import_pictures(src, fmt="nv12", width=w, height=h, transfer="pq", matrix="auto")
    assert_same(got, H.import_images(setting(1000, 0, 9, 6), S.canonicals(src, s), w, h), "auto at 48 lines: bt601")


def test_padded_stride(dec):
    """Three images 48 bytes further apart than their size, noise between them."""
    w, h = 34, 18
    s = S.layout("p010", w, h, 74, 20)
    src = S.sources(3, s, 8)
    got = import_surface(dec, src, "p010", w, h, 74, 20, None, 48, transfer="pq")
    assert_same(got, H.import_images(setting(), S.canonicals(src, s), w, h), "padded stride")


def test_packed_i420_through_import_frames(dec):
    w, h = 64, 48
    src = random_i420(3, w, h, 17)
    got = import_i420(dec, src, w, h, None, transfer="pq", peak_nits=4000)
    assert_same(got, H.import_images(setting(4000), src, w, h), "efx_import_frames")
    got = import_i420(dec, src, w, h, RECT, transfer="pq", peak_nits=4000)
    assert_same(got, H.import_images(setting(4000), src, w, h, None, RECT), "efx_import_frames into a rectangle")


def test_queued_calls_keep_their_tables(dec):
    """Two calls with different peaks (neither used before in this context) into different outputs, no synchronisation
    between them; then the first setting again, which finds its copy."""
    w, h, n = 64, 48, 2
    src = random_i420(n, w, h, 21)
    sbuf = dec.alloc(src.size)
    sbuf.upload(src)
    jobs = [(617, dec.alloc(n * M.FRAME_BYTES)), (2350, dec.alloc(n * M.FRAME_BYTES)), (617, dec.alloc(n * M.FRAME_BYTES))]
    for peak, dbuf in jobs:
        dec.import_to(sbuf, dbuf, n_images=n, fmt="i420", width=w, height=h, transfer="pq", peak_nits=peak)
    dec.sync()
    for peak, dbuf in jobs:
        assert_same(dbuf.download(np.uint8, n * M.FRAME_BYTES).reshape(n, M.FRAME_BYTES), H.import_images(setting(peak), src, w, h), f"queued {peak}")
        dbuf.free()
    sbuf.free()


def test_set_then_off(efx, dec):
    """While HDR is on the colour setting is superseded; after NULL the bytes equal an import that never had the setting,
    and the colour setting applies again.  RGB sources ignore the setting."""
    w, h = 64, 48
    src = random_i420(2, w, h, 5)
    plain = M.import_images(src, "i420", w, h)
    before = import_i420(dec, src, w, h)
    assert_same(before, plain, "before")
    dec.set_import_colour("bt709", "full")
    try:
        coloured = K.convert(plain, None, *K.coefs(1, 1, h))
        assert_same(import_i420(dec, src, w, h), coloured, "the colour setting")
        dec.set_import_hdr("pq", "bt2020", peak_nits=400)
        try:
            hdr = H.import_images(setting(400), src, w, h)
            assert_same(import_i420(dec, src, w, h), hdr, "HDR supersedes the colour setting")
            assert_same(import_i420(dec, src, w, h, transfer="pq", peak_nits=4000), H.import_images(setting(4000), src, w, h), "the call's own")
            assert_same(import_i420(dec, src, w, h), hdr, "the setting again")
            rgb = np.random.default_rng(4).integers(0, 256, (2, 20, 24, 3), dtype=np.uint8)
            assert_same(dec.import_pictures(rgb), M.import_images(rgb, "rgb24", 24, 20), "rgb24 with HDR set")
            for kw in (dict(transfer="pq"), dict(transfer="pq", peak_nits=400)):
                with pytest.raises(ValueError):
                    dec.import_pictures(rgb, **kw)
        finally:
            dec.set_import_hdr()
        assert_same(import_i420(dec, src, w, h), coloured, "HDR off: the colour setting applies again")
    finally:
        dec.set_import_colour()
    assert_same(import_i420(dec, src, w, h), before, "everything off")


def test_errors_leave_the_setting(efx, dec):
    w, h = 64, 48
    src = random_i420(2, w, h, 33)
    assert set_hdr(efx, dec, peak=400) == 0
    try:
        bad = [dict(transfer=1), dict(transfer=18), dict(transfer=0), dict(primaries=5), dict(primaries=2), dict(matrix=0), dict(matrix=8),
               dict(matrix=10), dict(full=2), dict(full=-1), dict(peak=199), dict(peak=10001), dict(peak=-5)]
        for kw in bad:
            assert set_hdr(efx, dec, **kw) == ARG, kw
            assert dec._lib.efx_last_error(dec._ctx).startswith(b"efx_import_set_hdr: ")
        # the next import still runs with the previous setting
        assert_same(import_i420(dec, src, w, h), H.import_images(setting(400), src, w, h), "after the errors")
        for peak in (0, 200, 10000):
            assert set_hdr(efx, dec, peak=peak) == 0
        assert_same(import_i420(dec, src, w, h), H.import_images(setting(10000), src, w, h), "peak 10000")
    finally:
        assert dec._lib.efx_import_set_hdr(dec._ctx, None) == 0
    assert_same(import_i420(dec, src, w, h), M.import_images(src, "i420", w, h), "switched off")
    assert dec._lib.efx_import_set_hdr(None, None) == ARG
    h_bad = efx._ImportHdr(16, 9, 9, 0, 150)
    assert dec._lib.efx_import_hdr_tables(C.byref(h_bad), 0, None, 0) == ARG
    with pytest.raises(efx.EfxError) as e:
        import_i420(dec, src, w, h, transfer="pq", peak_nits=150)
    assert e.value.status == ARG
    assert_same(import_i420(dec, src, w, h), M.import_images(src, "i420", w, h), "after a rejected call")
    with pytest.raises(ValueError):
        import_i420(dec, src, w, h, peak_nits=1000)    # peak_nits without a transfer
