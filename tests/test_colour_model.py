"""The arithmetic of the import's colour conversion (espflix_amd/csrc/colour_px.h, built here with the host compiler)
against the NumPy model of include/efx.h's definition (tests/colour_model.py): the coefficient table against Fractions,
the integer pixel against the exact affine map over all 2^24 triples, the 8-bit bars of BT.709 and BT.601, and whole
pictures converted with the kernels' index arithmetic (tests/colour_model_main.cpp), also under the address and
undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import colour_model as K
import import_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the issue's check values, literally: rows (Y'; Cb'; Cr')
CHECK_ROWS = {(1, 0): [16384, 1627, 3141, 0, 16218, -1813, 0, -1187, 16112],
              (1, 1): [14071, 1429, 2759, 0, 14246, -1593, 0, -1043, 14153],
              (6, 1): [14071, 0, 0, 0, 14392, 0, 0, 0, 14392]}
IDENTITY = [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]
SETTINGS = [(c, r) for c in K.CODES for r in (0, 1)]


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build colour_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "colour_model_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("colour_px"), "drv", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("colour_px_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def header_coefs(driver, code, full, height=0):
    """(rc, q, y0) of colour::coefs."""
    r = subprocess.run([driver, "coefs", str(code), str(full), str(height)], capture_output=True, text=True, check=True, timeout=60)
    v = [int(x) for x in r.stdout.split()]
    return v[0], v[1:10], v[10]


def header_pixels(driver, code, full, triples):
    args = [str(int(c)) for t in triples for c in t]
    r = subprocess.run([driver, "pixels", str(code), str(full), *args], capture_output=True, text=True, check=True, timeout=60)
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def test_model_check_rows():
    for (code, full), want in CHECK_ROWS.items():
        assert K.coefs(code, full)[0] == want
    assert K.coefs(5, 0) is None and K.coefs(6, 0) is None


@pytest.mark.parametrize("code,full", SETTINGS)
def test_header_table_is_the_rounded_exact_matrix(driver, code, full):
    rc, q, y0 = header_coefs(driver, code, full)
    want = K.coefs(code, full)
    if want is None:
        assert (rc, q, y0) == (0, IDENTITY, 16)
    else:
        assert (rc, q, y0) == (1, *want)
        assert q[3] == 0 and q[6] == 0  # converted chroma never depends on luma
    if (code, full) in CHECK_ROWS:
        assert q == CHECK_ROWS[(code, full)]
    assert y0 == (0 if full else 16)
    assert max(abs(v) for v in q) < 1 << 15


def test_header_rejects_other_codes(driver):
    for code in K.INVALID_CODES:
        assert header_coefs(driver, code, 0)[0] == -1, code
    for full in (2, -1):
        assert header_coefs(driver, 1, full)[0] == -1


def test_unspecified_resolves_by_height(driver):
    for full in (0, 1):
        assert header_coefs(driver, 2, full, 576) == header_coefs(driver, 6, full)
        assert header_coefs(driver, 2, full, 578) == header_coefs(driver, 1, full)
        assert header_coefs(driver, 2, full, 0) == header_coefs(driver, 6, full)
    assert header_coefs(driver, 2, 0, 576)[0] == 0 and header_coefs(driver, 2, 1, 576)[0] == 1


@pytest.mark.parametrize("code,full", SETTINGS)
def test_precision_over_all_triples(driver, code, full):
    """|integer result - rounded exact map| <= 1 for every (Y, Cb, Cr): the shift rounds to half a step of the result,
    the exact map's own rounding is another half, and the coefficients' rounding (each within 2^-15 of its exact value,
    times samples of at most 255 + 128 + 128) adds under 0.03, so two results that differ lie on neighbouring integers."""
    r = subprocess.run([driver, "precision", str(code), str(full)], capture_output=True, text=True, check=True, timeout=600)
    worst, differing, total = (int(x) for x in r.stdout.split())
    print(f"matrix {code} range {full}: worst {worst}, differing triples {differing} of {total} ({differing / total:.5f})")
    assert total == 1 << 24
    assert worst <= 1


def test_bars(driver):
    """The 8-bit bars of BT.709 become the bars of BT.601 within +-1 (independent of the code under test), and the header
    gives exactly the model's values."""
    q, y0 = K.coefs(1, 0)
    got = header_pixels(driver, 1, 0, [b709 for _, b709, _ in K.BARS])
    for (name, b709, b601), g in zip(K.BARS, got):
        assert max(abs(a - b) for a, b in zip(g, b601)) <= 1, (name, g, b601)
        assert g == tuple(int(c) for c in K.convert_px(q, y0, *b709)), name
    assert got[0] == (82, 90, 240) and got[4] == (169, 166, 16)  # red and cyan: one off; the rest exact
    assert [g for i, g in enumerate(got) if i not in (0, 4)] == [b601 for i, (_, _, b601) in enumerate(K.BARS) if i not in (0, 4)]


def test_greys_and_range_ends(driver):
    greys = [(y, 128, 128) for y in range(256)]
    for code in K.CODES:
        assert header_pixels(driver, code, 0, greys) == greys, code  # every grey of a studio source maps to itself
        assert header_pixels(driver, code, 1, [(0, 128, 128), (255, 128, 128)]) == [(16, 128, 128), (235, 128, 128)], code


@pytest.mark.parametrize("code,full", [(1, 0), (1, 1), (6, 1), (9, 0)])
def test_header_pixels_match_model(driver, code, full):
    rng = np.random.default_rng(code * 2 + full)
    t = rng.integers(0, 256, (300, 3))
    t[:8] = [(0, 0, 0), (255, 255, 255), (0, 255, 255), (255, 0, 0), (0, 0, 255), (255, 255, 0), (16, 16, 240), (235, 240, 16)]
    q, y0 = K.coefs(code, full)
    want = np.stack(K.convert_px(q, y0, t[:, 0], t[:, 1], t[:, 2]), axis=1)
    assert np.array_equal(np.array(header_pixels(driver, code, full, t)), want)


def test_model_convert_is_the_definition():
    """The vectorised picture model against the formula of efx.h evaluated sample by sample on a small rectangle."""
    rng = np.random.default_rng(5)
    pic = rng.integers(0, 256, M.FRAME_BYTES, dtype=np.uint8)
    q, y0 = K.coefs(1, 1)
    rect = (18, 6, 6, 4)
    got = K.convert(pic, rect, q, y0)
    want = pic.copy()
    Y, U, V = want[:M.Y_BYTES].reshape(M.H, M.W), want[M.Y_BYTES:M.Y_BYTES + M.C_BYTES].reshape(M.CH, M.CW), want[M.Y_BYTES + M.C_BYTES:].reshape(M.CH, M.CW)
    clamp = lambda v: min(255, max(0, v))
    for cy in range(3, 5):
        for cx in range(9, 12):
            u, v = int(U[cy, cx]) - 128, int(V[cy, cx]) - 128
            for yy in (2 * cy, 2 * cy + 1):
                for xx in (2 * cx, 2 * cx + 1):
                    Y[yy, xx] = clamp(16 + ((q[0] * (int(Y[yy, xx]) - y0) + q[1] * u + q[2] * v + 8192) >> 14))
            U[cy, cx] = clamp(128 + ((q[4] * u + q[5] * v + 8192) >> 14))
            V[cy, cx] = clamp(128 + ((q[7] * u + q[8] * v + 8192) >> 14))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, pic)


# matrix, range, height, destination rectangle
PICTURE_CASES = [
    (1, 1, 0, (0, 0, 352, 192)),
    (1, 1, 0, (18, 6, 36, 20)),      # begins and ends inside a band and inside a lane's column pair
    (9, 0, 0, (336, 176, 16, 16)),   # the smallest rectangle, at the frame's bottom-right corner
    (2, 0, 1080, (6, 0, 340, 192)),  # unspecified, an HD source
    (6, 1, 0, (0, 22, 352, 146)),
]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
@pytest.mark.parametrize("code,full,height,rect", PICTURE_CASES)
def test_whole_picture(request, tmp_path, which, code, full, height, rect):
    """The kernels' band and item arithmetic on the host, each band in a heap block of exactly its size: the result is
    the model's, and the sanitizer build runs clean."""
    exe = request.getfixturevalue("driver" if which == "plain" else "sanitized")
    rng = np.random.default_rng(code + rect[0])
    pic = rng.integers(0, 256, M.FRAME_BYTES, dtype=np.uint8)
    (tmp_path / "src.bin").write_bytes(pic.tobytes())
    run = subprocess.run([exe, "picture", str(code), str(full), str(height), *map(str, rect), str(tmp_path / "src.bin"),
                          str(tmp_path / "dst.bin")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    got = np.fromfile(tmp_path / "dst.bin", dtype=np.uint8)
    q, y0 = K.coefs(code, full, height)
    want = K.convert(pic, rect, q, y0)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]}"
    outside = np.ones((M.H, M.W), dtype=bool)
    outside[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = False
    assert np.array_equal(got[:M.Y_BYTES].reshape(M.H, M.W)[outside], pic[:M.Y_BYTES].reshape(M.H, M.W)[outside])


def test_python_helpers():
    import espflix_amd as efx
    assert efx.colour_source_limit(24, "full") == 9 and efx.colour_source_limit(24, "studio") == 24
    for limit in (0, 15, 16, 17, 24, 100, 234, 235, 255):
        assert efx.colour_source_limit(limit, "full") == K.source_limit(limit, True), limit
        assert efx.colour_source_limit(limit, "studio") == limit
    for name, code in K.NAMES.items():
        for rng, full in (("studio", 0), ("full", 1)):
            for height in (576, 578):
                want = K.coefs(code, full, height)
                on, q, y0 = efx.colour_coefs(name, rng, height)
                assert efx.colour_coefs(code, rng, height) == (on, q, y0)
                assert (on, q, y0) == ((False, IDENTITY, 16) if want is None else (True, *want)), (name, rng, height)
    assert efx.colour_coefs("auto", "studio", 576)[0] is False
    assert efx.colour_coefs("auto", "studio", 578) == efx.colour_coefs("bt709", "studio")
    assert efx.colour_coefs(2, "full", 576) == efx.colour_coefs("bt601", "full")
    for bad in (0, 3, 8, 10, "bt470", "rgb"):
        with pytest.raises(ValueError):
            efx.colour_coefs(bad)
    with pytest.raises(ValueError):
        efx.colour_coefs("bt709", "limited")
    with pytest.raises(ValueError):
        efx.colour_source_limit(24, "pc")
