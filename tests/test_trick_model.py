"""The selection rule of efx_trick_pick (espflix_amd/csrc/trick_sel.h, built here with the host compiler) against the NumPy
model of include/efx.h's definition (tests/trick_model.py) and against the properties the definition states, and a whole
pick on the host with the kernel's item arithmetic (tests/trick_model_main.cpp) under the address and undefined-behaviour
sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import trick_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEEDS = [1, 2, 3, 15, 255]
MAX_TOTAL = 64


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build trick_sel.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "trick_model_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("trick_sel_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.fixture(scope="module")
def header(sanitized):
    """What trick_sel.h says: per speed, {(first, n): (k0, [(j, fwd image, k)])} of every call window inside 64 pictures and
    {total: [rwd image of pick k]}."""
    out = {}
    for speed in SPEEDS:
        w = np.frombuffer(subprocess.run([sanitized, "windows", str(speed), str(MAX_TOTAL)], capture_output=True, check=True,
                                         timeout=120).stdout, dtype=np.int64)
        pos, windows = 0, {}
        for first in range(MAX_TOTAL):
            for n in range(1, MAX_TOTAL - first + 1):
                c, k0 = int(w[pos]), int(w[pos + 1])
                assert c >= 0
                windows[(first, n)] = (k0, [tuple(int(v) for v in w[pos + 2 + 3 * i:pos + 5 + 3 * i]) for i in range(c)])
                pos += 2 + 3 * c
        assert pos == len(w)
        r = np.frombuffer(subprocess.run([sanitized, "rwd", str(speed), str(MAX_TOTAL)], capture_output=True, check=True,
                                         timeout=120).stdout, dtype=np.int64)
        pos, rwd = 0, {}
        for total in range(1, MAX_TOTAL + 1):
            K = int(r[pos])
            rwd[total] = [int(v) for v in r[pos + 1:pos + 1 + K]]
            pos += 1 + K
        assert pos == len(r)
        out[speed] = (windows, rwd)
    return out


@pytest.mark.parametrize("speed", SPEEDS)
def test_header_matches_model_for_every_call(header, speed):
    """efx_trick_count and the placement functions for every call (first, n) inside titles of 1 .. 64 pictures."""
    windows, rwd = header[speed]
    for (first, n), (k0, picks) in windows.items():
        assert len(picks) == M.count(first, n, speed), (first, n)
        total = first + n  # the shortest title that holds the call
        want = M.placements(first, n, speed, total)
        got = [(j, f, rwd[total][k]) for j, f, k in picks]
        assert got == want, (first, n)
        assert all((first + j) % speed == 0 and k == (first + j) // speed for j, _, k in picks), (first, n)
    for total in range(1, MAX_TOTAL + 1):
        assert len(rwd[total]) == M.total_picks(total, speed)
        assert [r for _, _, r in M.placements(0, total, speed, total)] == rwd[total]


@pytest.mark.parametrize("speed", SPEEDS)
def test_every_split_into_two_and_three_calls(header, speed):
    """The picks of the pieces concatenated are the picks of one call, and the rwd images are the fwd images reversed:
    titles of 1 .. 64 pictures, every split into two and three calls."""
    windows, rwd = header[speed]
    for total in range(1, MAX_TOTAL + 1):
        one = [j for j, _, _ in M.placements(0, total, speed, total)]  # the model's picks of the whole title
        K = len(one)
        assert one == [t for t in range(total) if t % speed == 0]
        for parts in (1, 2, 3):
            for calls in M.splits(total, parts):
                fwd, rev = [], [None] * K
                for first, n in calls:
                    k0, picks = windows[(first, n)]
                    piece = [None] * len(picks)
                    for j, f, k in picks:
                        assert piece[f] is None
                        piece[f] = first + j
                        assert rev[rwd[total][k]] is None  # every rwd image is written once
                        rev[rwd[total][k]] = first + j
                    fwd += piece
                assert fwd == one, (total, calls)
                assert rev == one[::-1], (total, calls)


def test_invalid_and_largest_arguments(sanitized):
    out = np.frombuffer(subprocess.run([sanitized, "invalid"], capture_output=True, check=True, timeout=60).stdout, dtype=np.int64)
    assert list(out[:6]) == [-1] * 6
    first, n = (1 << 40) - 1, (1 << 31) - 1
    assert int(out[6]) == n and int(out[7]) == -(-(first + n) // 255) - -(-first // 255)


def test_library_entry_point_is_the_header():
    """efx_trick_count of the built library (host only) against the model."""
    import espflix_amd as efx
    efx.load_library()
    for speed in SPEEDS:
        for first in (0, 1, 14, 15, 16, 254, 255, 1000):
            for n in (0, 1, 2, 15, 16, 300):
                assert efx.trick_count(first, n, speed) == M.count(first, n, speed)
    assert efx.trick_count(-1, 1, 15) == -1 and efx.trick_count(0, 1, 0) == -1 and efx.trick_count(0, 1, 256) == -1
    assert efx.trick_count(1 << 40, 1, 15) == -1 and efx.trick_count(0, -1, 15) == -1


@pytest.mark.parametrize("speed,calls", [(1, [7, 7, 7]), (2, [5, 16]), (3, [7, 7, 7]), (3, [5, 16]), (15, [1, 3, 17]), (15, [21])])
def test_whole_pick_on_the_host_under_sanitizers(sanitized, speed, calls):
    """2 streams x 21 pictures through k_trick's item arithmetic on exactly sized heap blocks: every picked byte lands where
    the placement functions say, the pads between streams keep their fill, and the sanitizers see no access outside."""
    r = subprocess.run([sanitized, "gather", str(speed), "2", str(sum(calls))] + [str(c) for c in calls], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
