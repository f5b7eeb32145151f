"""The arithmetic of k_quality (espflix_amd/csrc/quality_px.h, built here with the host compiler) against the NumPy model of
include/efx.h's definition (tests/quality_model.py), against the closed-form anchors and the properties the definition
states, and whole comparisons on the host with the kernel's index arithmetic (tests/quality_model_main.cpp), also under
the address and undefined-behaviour sanitizers.  No GPU."""
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import encode_model
import quality_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = sum(M.WINDOWS)


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build quality_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "quality_model_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("quality_px"), "drv", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("quality_px_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.fixture(params=["plain", "sanitized"])
def exe(request, driver, sanitized):
    return driver if request.param == "plain" else sanitized


def run_compare(exe, tmp, ref, test, ref_max):
    """The driver's records, maps and windows for (n, 101376) pairs."""
    ref, test = np.ascontiguousarray(ref, dtype=np.uint8).reshape(-1, M.PIC), np.ascontiguousarray(test, dtype=np.uint8).reshape(-1, M.PIC)
    n = len(ref)
    (tmp / "ref.bin").write_bytes(ref.tobytes())
    (tmp / "test.bin").write_bytes(test.tobytes())
    run = subprocess.run([exe, "compare", str(n), str(ref_max), str(tmp / "ref.bin"), str(tmp / "test.bin"), str(tmp / "recs.bin"),
                          str(tmp / "mb.bin"), str(tmp / "q.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    recs = np.fromfile(tmp / "recs.bin", dtype=np.uint64).reshape(n, 6)
    return (recs[:, :3].copy(), recs[:, 3:].view(np.int64).copy(), np.fromfile(tmp / "mb.bin", dtype=np.uint32).reshape(n, 264),
            np.fromfile(tmp / "q.bin", dtype=np.int32).reshape(n, NQ))


def checkerboard(rows, cols):
    y, x = np.mgrid[0:rows, 0:cols]
    return (((x + y) & 1) * 255).astype(np.uint8)


def anchors():
    """(reference, test) of the three anchor pairs, the property on all three planes."""
    rng = np.random.default_rng(11)
    same = rng.integers(0, 256, M.PIC, dtype=np.uint8)
    lo, hi = np.zeros(M.PIC, np.uint8), np.full(M.PIC, 255, np.uint8)
    board = M.image_of(checkerboard(192, 352), checkerboard(96, 176), checkerboard(96, 176))
    return np.stack([same, lo, board]), np.stack([same, hi, 255 - board])


@functools.lru_cache(maxsize=None)
def case(name):
    """(reference, test, ref_max) of a named case; pictures are noise on all three planes."""
    rng = np.random.default_rng(sum(map(ord, name)))
    noise = lambda n: rng.integers(0, 256, (n, M.PIC), dtype=np.uint8)
    if name == "anchors":
        return (*anchors(), 0)
    if name == "noise":
        return noise(2), noise(2), 0
    if name == "plus_minus_6":
        ref = noise(2)
        return ref, np.clip(ref.astype(np.int64) + rng.integers(-6, 7, ref.shape), 0, 255).astype(np.uint8), 0
    if name == "flat":
        lo, hi = np.zeros(M.PIC, np.uint8), np.full(M.PIC, 255, np.uint8)
        return np.stack([lo, lo, hi, hi]), np.stack([lo, hi, lo, hi]), 0
    if name.startswith("bright_"):
        ref = rng.integers(249, 256, (2, M.PIC), dtype=np.uint8)
        return ref, rng.integers(200, 256, (2, M.PIC), dtype=np.uint8), int(name.split("_")[1])
    raise KeyError(name)


CASES = ["anchors", "noise", "plus_minus_6", "flat", "bright_248", "bright_255", "bright_1"]


@functools.lru_cache(maxsize=None)
def model_of(name):
    """The model's records, maps and windows of a case, made once."""
    ref, test, ref_max = case(name)
    sse, ssim, mb = M.compare_batch(ref, test, ref_max)
    q = np.array([[v for a, b in zip(M.planes(r), M.planes(t)) for row in M.plane_q(np.minimum(a, ref_max or 255), b) for v in row]
                  for r, t in zip(ref, test)], dtype=np.int64)
    return sse, ssim, mb, q


def test_model_anchors():
    """The closed-form numbers of the definition, from the model alone."""
    sse, ssim, mb, _ = model_of("anchors")
    assert sse[0].tolist() == [0, 0, 0] and ssim[0].tolist() == [4089 * 65536, 989 * 65536, 989 * 65536]
    assert ssim[0].tolist() == [267976704, 64815104, 64815104]
    assert sse[1].tolist() == [4394649600, 1098662400, 1098662400] and ssim[1].tolist() == [0, 0, 0]
    assert sse[2].tolist() == [4394649600, 1098662400, 1098662400]
    assert ssim[2].tolist() == [4089 * -65304, 989 * -65304, 989 * -65304] and ssim[2, 0] == -267028056
    assert (mb[1] == 256 * 65025).all() and (mb[0] == 0).all()


@pytest.mark.parametrize("name", CASES)
def test_header_equals_model(exe, tmp_path, name):
    ref, test, ref_max = case(name)
    want_sse, want_ssim, want_mb, want_q = model_of(name)
    sse, ssim, mb, q = run_compare(exe, tmp_path, ref, test, ref_max)
    assert np.array_equal(sse, want_sse), (sse.tolist(), want_sse.tolist())
    assert np.array_equal(ssim, want_ssim), (ssim.tolist(), want_ssim.tolist())
    assert np.array_equal(mb, want_mb)
    assert np.array_equal(q, want_q), f"{np.count_nonzero(q != want_q)} windows differ"
    assert q.min() >= -65536 and q.max() <= 65536
    assert np.array_equal(mb.astype(np.uint64).sum(axis=1), sse[:, 0])
    if name == "anchors":
        assert ssim.tolist() == [[267976704, 64815104, 64815104], [0, 0, 0], [-267028056, 989 * -65304, 989 * -65304]]
        assert sse[:, 0].tolist() == [0, 4394649600, 4394649600]


@pytest.mark.parametrize("name", ["anchors", "noise", "plus_minus_6", "flat"])
def test_swapped_pair_gives_the_same_record(driver, tmp_path, name):
    ref, test, ref_max = case(name)
    assert ref_max == 0
    sse, ssim, mb, _ = run_compare(driver, tmp_path, test, ref, 0)
    want_sse, want_ssim, want_mb, _ = model_of(name)
    assert np.array_equal(sse, want_sse) and np.array_equal(ssim, want_ssim) and np.array_equal(mb, want_mb)


@pytest.mark.parametrize("name", CASES)
def test_mean_ssim_is_within_2_to_minus_16_of_float64(name):
    ref, test, ref_max = case(name)
    _, ssim, _, _ = model_of(name)
    for k, (r, t) in enumerate(zip(ref, test)):
        for p, (a, b) in enumerate(zip(M.planes(r), M.planes(t))):
            exact = M.plane_ssim_float(np.minimum(a, ref_max or 255), b)
            assert abs(M.mean_ssim(int(ssim[k, p]), p) - exact) < 2.0 ** -16, (name, k, p)


def test_luma_psnr_is_encode_models():
    import espflix_amd as efx
    for name in ("bright_248", "plus_minus_6", "noise"):
        ref, test, _ = case(name)
        sse, _, _ = M.compare_batch(ref, test, 248)
        want = encode_model.luma_psnr(ref, test)
        assert abs(np.mean([M.psnr(int(s), M.SAMPLES[0]) for s in sse[:, 0]]) - want) < 1e-9
        assert abs(np.mean([efx.compare_psnr(int(s), M.SAMPLES[0]) for s in sse[:, 0]]) - want) < 1e-9


def test_host_helpers():
    import espflix_amd as efx
    assert efx.compare_psnr(0, 67584) == math.inf
    assert abs(efx.compare_psnr(67584, 67584) - 10 * math.log10(65025)) < 1e-12
    assert efx.compare_ssim(4089 * 65536, 0) == 1.0 and efx.compare_ssim(989 * 65536, 1) == 1.0 and efx.compare_ssim(-989 * 65536, 2) == -1.0
    assert math.isnan(efx.compare_ssim(1, 3)) and math.isnan(efx.compare_ssim(1, -1))
    assert abs(efx.compare_ssim(-267028056, 0) - M.mean_ssim(-267028056, 0)) < 1e-15


def test_q16_quotient(driver):
    """|num| == den, num < 0, random pairs, and the window with the largest den the cases above produce."""
    big = 289_999_999_999_999_999
    pairs = [(big, big), (-big, big), (big - 1, big), (1 - big, big), (-1, 3), (1, 3), (0, 416 * 235963), (416 * 235963, 416 * 235963),
             (-(big // 2), big), (big // 2 + 1, big), (1, big)]
    m = 4424967041   # (den = 65536 m: quotients that are whole numbers, where an estimate falls to either side)
    for k in (1, 2, 3, 1000, 21845, 32768, 65535):
        pairs += [(k * m, 65536 * m), (k * m - 1, 65536 * m), (-k * m, 65536 * m), (k * m + 1, 65536 * m)]
    rng = np.random.default_rng(5)
    for _ in range(200):
        den = int(rng.integers(1, big))
        pairs.append((int(rng.integers(-den, den + 1)), den))
    out = subprocess.run([driver, "q16", *(str(v) for p in pairs for v in p)], capture_output=True, text=True, check=True, timeout=60)
    got = [int(v) for v in out.stdout.split()]
    assert got == [M.quotient(n, d) for n, d in pairs]
    assert got[:6] == [65536, -65536, 65535, -65535, -21845, 21845]
    # the largest den (and the most negative num) among the windows of every case
    best, lowest = None, None
    for name in CASES:
        ref, test, ref_max = case(name)
        for r, t in zip(ref, test):
            for a, b in zip(M.planes(r), M.planes(t)):
                S = [v.reshape(-1).tolist() for v in M.window_sums(np.minimum(a, ref_max or 255), b)]
                for s in zip(*S):
                    n, d = M.num_den(*s)
                    if best is None or d > best[1]:
                        best = (s, d)
                    if lowest is None or n < lowest[1]:
                        lowest = (s, n)
    for s, _ in (best, lowest):
        n, d = M.num_den(*s)
        assert abs(n) <= d < 2.9e17
        out = subprocess.run([driver, "window", *(str(v) for v in s)], capture_output=True, text=True, check=True, timeout=60)
        assert [int(v) for v in out.stdout.split()] == [n, d, M.quotient(n, d)]
    assert lowest[1] < 0


def test_clamp_on_packed_bytes(driver, sanitized):
    for exe in (driver, sanitized):
        run = subprocess.run([exe, "clamp"], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]


def test_binding_declares_the_entry_points():
    import ctypes as C
    import espflix_amd as efx
    for name in ("efx_compare_pictures", "efx_compare_psnr", "efx_compare_ssim"):
        assert name in efx._SYMBOLS
    assert C.sizeof(efx._CompareOpts) == 8 + 3 * C.sizeof(C.c_size_t) and C.sizeof(efx._CompareRec) == 48
