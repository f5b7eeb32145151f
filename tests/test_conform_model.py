"""The rule of efx_conform_rate (espflix_amd/csrc/conform_sel.h, built here with the host compiler) against the model of
include/efx.h's definition (tests/conform_model.py), against brute force of the slot rule and against the properties the
definition states, and whole calls on the host with the kernel's item arithmetic (tests/conform_model_main.cpp) under the
address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import conform_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_N = 48
TOP = (1 << 31) - 1


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build conform_sel.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "conform_model_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("conform_sel_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.fixture(scope="module")
def header(sanitized):
    """What conform_sel.h says: {(source rate, code): (A, B, [outputs(N) for N = 0 .. MAX_N], [source(n)])}."""
    out = {}
    for r in M.SOURCES:
        for code in range(1, 9):
            w = np.frombuffer(subprocess.run([sanitized, "table", str(r.numerator), str(r.denominator), str(code), str(MAX_N)],
                                             capture_output=True, check=True, timeout=120).stdout, dtype=np.int64)
            assert int(w[0]) == 1, (r, code)
            nout = [int(v) for v in w[3:4 + MAX_N]]
            src = [int(v) for v in w[4 + MAX_N:]]
            assert len(src) == nout[-1]
            out[(r, code)] = (int(w[1]), int(w[2]), nout, src)
    return out


def test_header_matches_model_and_brute_force(header):
    """13 source rates x 8 codes: the reduced ratio, the count after every N = 0 .. 48 and every output's source are the
    model's, and both are what the slot rule gives by brute force."""
    for (r, code), (A, B, nout, src) in header.items():
        assert (A, B) == M.ratio(r, code), (r, code)
        assert nout == [M.outputs(N, r, code) for N in range(MAX_N + 1)], (r, code)
        assert src == [M.source(n, r, code) for n in range(len(src))], (r, code)
        for N in (0, 1, 2, 7, MAX_N):
            assert M.brute_sources(N, r, code) == src[:nout[N]], (r, code, N)
        # nearest slot: every output's source is the last picture whose slot is at or before it
        for n, i in enumerate(src):
            assert M.slot(i, r, code) <= n < M.slot(i + 1, r, code), (r, code, n)


def test_pieces_concatenate_to_the_whole(header):
    """Every call window inside 48 pictures: its outputs' sources lie inside it, and the calls of every split into two and
    three pieces write the outputs of the one long call, in order."""
    for (r, code), (_, _, nout, src) in header.items():
        for first in range(MAX_N):
            for n in range(1, MAX_N - first + 1):
                assert M.count(first, n, r, code) == nout[first + n] - nout[first]
                assert all(first <= i < first + n for i in src[nout[first]:nout[first + n]]), (r, code, first, n)
        for a in range(1, MAX_N):
            for b in range(a, MAX_N):
                cuts = [0, a, b, MAX_N]
                got = [i for lo, hi in zip(cuts, cuts[1:]) for i in src[nout[lo]:nout[hi]]]
                assert got == src, (r, code, a, b)


def test_identity_and_simple_ratios(header):
    for code in range(1, 9):
        _, _, nout, src = header[(M.RATES[code], code)]
        assert nout == list(range(MAX_N + 1)) and src == list(range(MAX_N)), code
    assert header[(Fraction(50), 3)][3] == [2 * n for n in range(MAX_N // 2)]
    assert header[(Fraction(15), 5)][3] == [n // 2 for n in range(2 * MAX_N)]


def test_argument_bounds(sanitized):
    out = [int(v) for v in np.frombuffer(subprocess.run([sanitized, "args"], capture_output=True, check=True, timeout=60).stdout,
                                         dtype=np.int64)]
    assert out[:13] == [-1] * 13
    big = Fraction(2147483647, 17895696)  # against 60 Hz: A = 2^31 - 1, B = 2^31 - 128
    assert M.ratio(big, 8) == (2147483647, 2147483520)
    assert out[13] == 2 and out[14] == 128
    assert out[15] == M.count(TOP - 3, 3, big, 8) and out[15] >= 1
    whole = M.count(0, TOP, big, 8)
    assert out[16] == M.source(whole - 1, big, 8) < TOP
    assert out[17] == whole
    assert out[18] == M.source(TOP, Fraction(25), 4) and out[19] == M.source(TOP, big, 8)


def test_library_entry_points_are_the_header():
    """efx_conform_count and efx_conform_source of the built library (host only) against the model."""
    import espflix_amd as efx
    for r in M.SOURCES:
        for code in (1, 2, 4, 8):
            for first in (0, 1, 7, 1000):
                for n in (0, 1, 2, 25):
                    assert efx.conform_count(r, M.RATES[code], first, n) == M.count(first, n, r, code)
            lib = efx.load_library()
            for n in (0, 1, 5, 1001, TOP):
                assert lib.efx_conform_source(r.numerator, r.denominator, code, n) == M.source(n, r, code)
    lib = efx.load_library()
    assert lib.efx_conform_count(25, 1, 9, 0, 1) == -1 and lib.efx_conform_count(25, 1, 4, TOP, 1) == -1
    assert lib.efx_conform_source(25, 1, 4, -1) == -1 and lib.efx_conform_source(0, 1, 4, 0) == -1


@pytest.mark.parametrize("rate,code,first,calls", [
    ("15/1", 5, 0, [4]), ("50/1", 3, 0, [7]), ("60/1", 1, 0, [3, 4]), ("25/1", 2, 0, [1, 2, 3]),
    ("1000000/41667", 4, 5, [6]), ("24/1", 2, 3, [2, 1]), ("120/1", 4, 0, [1, 1, 5]),
    ("2147483647/17895696", 8, (1 << 31) - 4, [1, 2]),
])
def test_whole_calls_on_the_host_under_sanitizers(sanitized, rate, code, first, calls):
    """2 streams through k_conform's item arithmetic on exactly sized heap blocks: every output byte is its source's, the
    pads between streams keep their fill, pieces concatenate, and the sanitizers see no access outside."""
    num, den = rate.split("/")
    r = subprocess.run([sanitized, "gather", num, den, str(code), "2", str(first)] + [str(c) for c in calls], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
