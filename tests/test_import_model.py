"""The arithmetic of k_import (espflix_amd/csrc/import_px.h, built here with the host compiler) against the NumPy model
of include/efx.h's formulas (tests/import_model.py), the model against Pillow's bilinear resize, and a whole import on the
host with the kernel's index arithmetic (tests/import_model_main.cpp) under the address and undefined-behaviour
sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import import_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"i420": 0, "rgb24": 1, "rgbp": 2}
TAP_D = (2, 8, 16, 88, 96, 176, 192, 352)
TAP_EXTRA = [(1920, 352), (1080, 192), (4096, 352), (2304, 192), (4096, 128), (333, 352)]
STUDIO_ANCHORS = [((255, 255, 255), (235, 128, 128)), ((0, 0, 0), (16, 128, 128)), ((255, 0, 0), (82, 90, 240))]
# (source width, height, destination width, height) of the comparison with Pillow
PILLOW_GEOMETRIES = [(704, 384, 352, 192), (1920, 1080, 352, 192), (4096, 2304, 352, 192), (3840, 2160, 352, 192),
                     (1234, 987, 350, 190), (354, 194, 352, 192), (353, 193, 352, 192), (2, 2, 352, 192), (333, 77, 352, 192),
                     (176, 96, 352, 192), (100, 50, 352, 192), (16, 4096, 352, 144), (17, 4093, 30, 128)]


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build import_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "import_model_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("import_px"), "drv", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("import_px_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def header_taps(driver, S, D):
    r = subprocess.run([driver, "taps", str(S), str(D)], capture_output=True, check=True, timeout=120)
    rec = np.frombuffer(r.stdout, dtype=np.int32).reshape(D, 2 + M.MAX_TAPS)
    return rec[:, 0], rec[:, 1], rec[:, 2:]


def check_taps(driver, S, D):
    start, count, coef = header_taps(driver, S, D)
    ws, wc, wk = M.windows(S, D)
    assert np.array_equal(start, ws) and np.array_equal(count, wc), (S, D)
    assert np.array_equal(coef, wk), (S, D)
    assert (coef.sum(axis=1) == M.ONE).all() and (coef >= 0).all() and count.min() >= 1, (S, D)
    assert (start >= 0).all() and (start + count <= S).all(), (S, D)
    # luma and the chroma of an I420 source stay within 66 taps when S <= 32 D
    assert S > M.MAX_RATIO * D or count.max() <= 66, (S, D)
    if S == D:
        assert np.array_equal(start, np.arange(D)) and (count == 1).all() and (coef[:, 0] == M.ONE).all()


@pytest.mark.parametrize("D", TAP_D)
def test_header_taps_match_model(driver, D):
    for S in range(1, 81):
        if S <= 2 * M.MAX_RATIO * D:  # (2 x: the chroma of an RGB source)
            check_taps(driver, S, D)


@pytest.mark.parametrize("S,D", TAP_EXTRA + [(4094, 64), (4096, 64), (352, 352), (192, 192)])
def test_header_taps_match_model_large(driver, S, D):
    check_taps(driver, S, D)


def test_model_taps_are_the_formula():
    """The vectorised model against the formula of efx.h evaluated tap by tap."""
    for S, D in ((5, 16), (333, 352), (1080, 192), (80, 2), (7, 7)):
        k = M.tap_matrix(S, D)
        for d in (0, 1, D // 2, D - 1):
            u = [max(0, 2 * max(S, D) - abs((2 * s + 1) * D - (2 * d + 1) * S)) for s in range(S)]
            want = [x * 16384 // sum(u) for x in u]
            want[u.index(max(u))] += 16384 - sum(want)
            assert k[d].tolist() == want
            nz = np.flatnonzero(np.array(u))
            assert (np.diff(nz) == 1).all()  # the window is contiguous


def test_constant_planes_stay_constant():
    for (w, h, dw, dh) in ((333, 77, 352, 192), (1920, 1080, 352, 192), (2, 2, 16, 16), (100, 3000, 16, 94)):
        for v in (0, 1, 16, 128, 254, 255):
            assert (M.resample(np.full((h, w), v, dtype=np.uint8), dw, dh) == v).all(), (w, h, dw, dh, v)


def test_same_size_is_a_copy():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, M.FRAME_BYTES, dtype=np.uint8)
    assert np.array_equal(M.import_image(src, "i420", 352, 192), src)


@pytest.mark.parametrize("full_range", [False, True])
def test_header_matrix_matches_model_everywhere(driver, full_range):
    r = subprocess.run([driver, "matrix", str(int(full_range))], capture_output=True, check=True, timeout=300)
    got = np.frombuffer(r.stdout, dtype=np.uint32).reshape(256, 256, 256)
    want = np.empty((256, 256, 256), dtype=np.uint32)
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for red in range(256):
        y, cb, cr = M.rgb_to_ycbcr(np.full_like(g, red), g, b, full_range)
        want[red] = y.astype(np.uint32) | (cb.astype(np.uint32) << 8) | (cr.astype(np.uint32) << 16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} triples differ, first (R, G, B) = {bad[0].tolist()}"
    if not full_range:
        for (r_, g_, b_), yuv in STUDIO_ANCHORS:
            w = int(got[r_, g_, b_])
            assert (w & 0xFF, (w >> 8) & 0xFF, w >> 16) == yuv
        assert (int(got[0, 0, 255]) >> 8) & 0xFF == 240  # blue: Cb 240


def test_model_anchors():
    for rgb, yuv in STUDIO_ANCHORS:
        assert tuple(int(c) for c in M.rgb_to_ycbcr(*rgb)) == yuv
    assert int(M.rgb_to_ycbcr(0, 0, 255)[1]) == 240
    assert tuple(int(c) for c in M.rgb_to_ycbcr(255, 255, 255, True)) == (255, 128, 128)
    assert tuple(int(c) for c in M.rgb_to_ycbcr(0, 0, 0, True)) == (0, 128, 128)


def planes_for(w, h, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    return {"noise": rng.integers(0, 256, (h, w), dtype=np.uint8),
            "two-level": (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8),
            "smooth": ((np.sin(xx / 37.0) + np.cos(yy / 23.0) + 2) * 63.75).astype(np.uint8)}


@pytest.mark.parametrize("w,h,dw,dh", PILLOW_GEOMETRIES)
def test_model_against_pillow(w, h, dw, dh):
    """|model - Pillow| <= 1 on every sample: one rounding step of each implementation (Pillow rounds to 8 bits between
    its passes, the model to 16)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(w * 4099 + h)
    for kind, p in planes_for(w, h, rng).items():
        want = np.asarray(Image.fromarray(p).resize((dw, dh), Image.BILINEAR)).astype(np.int64)
        d = np.abs(M.resample(p, dw, dh) - want)
        print(f"{w}x{h} -> {dw}x{dh} {kind}: worst {d.max()}, equal {(d == 0).mean():.3f}")
        assert d.max() <= 1, (kind, int(d.max()))


def test_model_against_pillow_fixture():
    """The same condition against results Pillow left in tests/golden/import_pillow.npz (make_import_pillow.py)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "import_pillow.npz"))
    n = sum(1 for k in z.files if k.startswith("src"))
    assert n >= 6
    for i in range(n):
        src, want = z[f"src{i}"], z[f"dst{i}"].astype(np.int64)
        d = np.abs(M.resample(src, want.shape[1], want.shape[0]) - want)
        assert d.max() <= 1, (i, src.shape, want.shape, int(d.max()))


def test_letterbox_rectangle():
    import espflix_amd as efx
    assert M.letterbox_rect(992, 546) == (2, 0, 348, 192)
    assert M.letterbox_rect(1920, 1080) == (6, 0, 340, 192)
    assert M.letterbox_rect(352, 192) == (0, 0, 352, 192)
    assert M.letterbox_rect(1920, 800) == (0, 22, 352, 146)
    assert M.letterbox_rect(4096, 2) == (0, 88, 352, 16)
    assert M.letterbox_rect(30, 4094) == (168, 0, 16, 192)
    for w, h in [(992, 546), (1920, 1080), (352, 192), (1920, 800), (4096, 2), (30, 4094), (333, 77), (2, 2), (640, 480),
                 (3, 4000), (1000, 547)]:
        x, y, dw, dh = efx.letterbox_rect(w, h)
        assert (x, y, dw, dh) == M.letterbox_rect(w, h)
        assert not (x | y | dw | dh) & 1 and dw >= 16 and dh >= 16 and x >= 0 and y >= 0 and x + dw <= 352 and y + dh <= 192
        assert dw == 352 or dh == 192
        # the largest even rectangle of that ratio: two more rows (columns) would no longer fit it
        if dw == 352 and dh > 16:
            assert dh * w <= 352 * h < (dh + 2) * w
        if dh == 192 and dw > 16 and dw < 352:
            assert dw * h <= 192 * w < (dw + 2) * h
        assert abs((352 - dw) - 2 * x) <= 2 and abs((192 - dh) - 2 * y) <= 2


def test_src_bytes_and_shape_rules():
    import espflix_amd as efx
    for fmt in ("i420", "rgb24", "rgbp"):
        for w, h in ((2, 2), (333, 77), (352, 192), (4096, 4096), (4097, 2), (1, 2), (2, 4098), (16, 17)):
            assert efx.import_src_bytes(fmt, w, h) == M.src_bytes(fmt, w, h), (fmt, w, h)
    assert efx.import_src_bytes(3, 16, 16) == 0 and efx.import_src_bytes("yuv444", 16, 16) == 0
    assert efx._import_geometry((5, 77, 333, 3), None, None, None) == ("rgb24", 5, 333, 77)
    assert efx._import_geometry((5, 3, 77, 333), None, None, None) == ("rgbp", 5, 333, 77)
    assert efx._import_geometry((2, 16 * 16 * 3 // 2), None, 16, 16) == ("i420", 2, 16, 16)
    for shape, fmt, w, h in (((5, 77, 333), None, None, None), ((2, 384), None, None, None), ((2, 385), "i420", 16, 16),
                             ((5, 77, 333, 4), "rgb24", None, None), ((5, 77, 333, 3), "rgb24", 334, None)):
        with pytest.raises(ValueError):
            efx._import_geometry(shape, fmt, w, h)


SANITIZED_CASES = [
    # fmt, width, height, crop, destination rectangle, full range
    ("rgbp", 2, 2, None, None, False),
    ("rgb24", 333, 77, (7, 3, 321, 71), (2, 6, 348, 180), True),   # odd crop offset: rows start on every byte phase
    ("rgb24", 333, 77, None, None, False),
    ("i420", 4096, 2304, None, None, False),
    ("i420", 354, 194, (2, 2, 352, 192), (0, 0, 352, 192), False),
]


@pytest.mark.parametrize("fmt,w,h,crop,rect,full", SANITIZED_CASES)
def test_whole_import_under_sanitizers(sanitized, tmp_path, fmt, w, h, crop, rect, full):
    """The kernel's addressing on the host, source and output in heap blocks of exactly the contract's sizes: the run is
    clean under -fsanitize=address,undefined and the output is the model's."""
    rng = np.random.default_rng(w + h)
    src = rng.integers(0, 256, M.src_bytes(fmt, w, h), dtype=np.uint8)
    (tmp_path / "src.bin").write_bytes(src.tobytes())
    c, r = crop or (0, 0, w, h), rect or (0, 0, M.W, M.H)
    run = subprocess.run([sanitized, str(FMT[fmt]), str(w), str(h), *map(str, c), *map(str, r), str(int(full)),
                          str(tmp_path / "src.bin"), str(tmp_path / "dst.bin")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    got = np.fromfile(tmp_path / "dst.bin", dtype=np.uint8)
    want = M.import_image(src, fmt, w, h, c, r, full)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]}"
