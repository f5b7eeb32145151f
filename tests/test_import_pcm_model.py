"""The arithmetic of k_import_pcm (espflix_amd/csrc/import_pcm.h, built here with the host compiler into
tests/import_pcm_model_main.cpp, which runs whole calls with the kernel's addressing -- once plainly, once under the
address and undefined-behaviour sanitizers) against the NumPy model of include/efx.h's formulas
(tests/import_pcm_model.py); the output counts; the prototype table of the library, of the model and of
tests/golden/import_pcm_table.npy; and a float64 yardstick that shares no code with any of them.  No GPU.

Regenerate tests/golden/import_pcm_quality.json (the yardstick's and the integer path's SNRs) with
`python tests/test_import_pcm_model.py`."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import import_pcm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_NPY = os.path.join(ROOT, "tests", "golden", "import_pcm_table.npy")
QUALITY_JSON = os.path.join(ROOT, "tests", "golden", "import_pcm_quality.json")
BIG = (1 << 33) + 5
# pieces a stream is fed in: odd points, pieces shorter than the history (127), then the rest
PIECES = (1, 5, 126, 127, 1000, 37, 3)
TOTAL = 9000  # frames: the rest is more than one tile of 1024 outputs at every ratio
MIX = {1: None, 2: None, 6: (9598, 9598, 6786, -10, 3388, 3388)}  # (5.1: -3 dB centre and surrounds, a token LFE)


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build import_pcm.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "import_pcm_model_main.cpp"), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    return str(exe)


@pytest.fixture(scope="module")
def table_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("import_pcm_table") / "table.bin"
    np.load(TABLE_NPY).astype(np.int32).tofile(path)
    return str(path)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("import_pcm"), "drv", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("import_pcm_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def run_driver(exe, table_file, tmp, frames, r, o, layout, mix, first_in, pieces):
    """frames: [n_in, channels] int16 of one stream, fed in `pieces`.  Returns (samples, state as 128 int16)."""
    ch = frames.shape[1]
    at, blocks = 0, []
    for n in pieces:
        part = frames[at:at + n]
        blocks.append(part.reshape(-1) if layout == M.INTERLEAVED else part.T.reshape(-1))
        at += n
    assert at == frames.shape[0]
    src, dst, st = tmp / "src.bin", tmp / "dst.bin", tmp / "state.bin"
    np.concatenate(blocks).astype(np.int16).tofile(src)
    w = list(mix or ()) + [0] * (8 - len(mix or ()))
    run = subprocess.run([exe, "run", table_file, str(r), str(o), str(ch), str(layout), str(first_in), *map(str, w), str(src),
                          str(dst), str(st), *map(str, pieces)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    return np.fromfile(dst, dtype=np.int16), np.fromfile(st, dtype=np.int16)


def full_scale_noise(n, ch, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (n, ch), dtype=np.int64).astype(np.int16)
    # runs of the extremes on every channel at once: the downmix and the final clamp see +-32767 and -32768
    x[40:200] = 32767
    x[300:460] = -32768
    x[500:520:2] = -32767
    return x


@pytest.mark.parametrize("layout", [M.INTERLEAVED, M.PLANAR], ids=["interleaved", "planar"])
@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("r,o", M.RATE_PAIRS)
def test_header_matches_model(driver, sanitized, table_file, tmp_path, r, o, ch, layout):
    """One stream fed in pieces, through the kernel's addressing on the host: the plain and the sanitizer build give the
    model's samples of ONE call and leave its history, from a fresh stream and at first_in = 2^33 + 5."""
    x = full_scale_noise(TOTAL, ch, r + 7 * ch)
    pieces = PIECES + (TOTAL - sum(PIECES),)
    for first_in, exe in ((0, driver), (BIG, sanitized), (0, sanitized), (BIG, driver)):
        want, hist = M.import_pcm(x.reshape(1, -1), r, o, ch, M.INTERLEAVED, MIX[ch], first_in)
        assert want.shape[1] == M.out_samples(r, o, first_in, TOTAL)
        got, state = run_driver(exe, table_file, tmp_path, x, r, o, layout, MIX[ch], first_in, pieces)
        bad = np.flatnonzero(got != want[0])
        assert got.shape == want[0].shape and bad.size == 0, f"first_in {first_in}: {bad.size} samples differ, first at {bad[:1]}"
        if r != o:
            assert np.array_equal(state, M.state_bytes(hist)[0])
        else:
            assert not state.any()  # equal rates: the state is not used
    if r != o:
        assert np.abs(want).max() == 32767 or want.min() == -32768  # the final clamp was reached


def test_model_in_pieces_is_the_model_in_one():
    r, o, ch = 44100, 48000, 2
    x = full_scale_noise(3000, ch, 1)
    whole, hist = M.import_pcm(x.reshape(1, -1), r, o, ch)
    parts, h, at = [], None, 0
    for n in (1, 5, 126, 127, 1000, 1741):
        y, h = M.import_pcm(x[at:at + n].reshape(1, -1), r, o, ch, first_in=at, hist=h)
        parts.append(y[0])
        at += n
    assert np.array_equal(np.concatenate(parts), whole[0]) and np.array_equal(h, hist)


def test_model_is_the_formula_tap_by_tap():
    """The vectorised model against include/efx.h's formulas in plain Python integers, for a few outputs."""
    T = [int(v) for v in M.table()]
    rng = np.random.default_rng(5)
    for r, o in ((44100, 48000), (96000, 48000), (22050, 16000), (8000, 48000)):
        m = rng.integers(-32768, 32768, 700, dtype=np.int64)
        y, _ = M.resample(m[None], r, o)
        Mx, W = max(r, o), M.delay(r, o)
        for n in (0, 1, 17, y.shape[1] - 1):
            a = n * r
            fl, acc = a // o, 0
            for j in range(fl - 2 * W + 1, fl + 1):
                e = abs(j * o - a + W * o)
                q, rho = divmod(e * M.P, Mx)
                if q < 16 * M.P and j >= 0:
                    f = rho * 4096 // Mx
                    acc += (T[q] + (((T[q + 1] - T[q]) * f) >> 12)) * int(m[j])
            if r > o:
                acc = acc * o // r
            assert int(y[0, n]) == max(-32768, min(32767, (acc + (1 << (M.Q - 1))) >> M.Q)), (r, o, n)


def test_output_counts(driver):
    import espflix_amd as efx
    lib = efx.load_library()
    rng = np.random.default_rng(2)
    for r, o in M.RATE_PAIRS + [(192000, 48000), (64000, 16000), (8000, 16000)]:
        W = -(-16 * max(r, o) // o) if r != o else 0
        assert M.delay(r, o) == W == lib.efx_import_pcm_delay(r, o) and W <= 64
        for first in (0, 1, 12345, BIG, (1 << 40) - 50001):  # (first + 50000 stays below 2^40)
            cuts = np.sort(rng.integers(0, 50000, 6))
            total = M.out_samples(r, o, first, int(cuts[-1]))
            assert total == -(-(first + int(cuts[-1])) * o // r) - -(-first * o // r)
            parts, at = 0, 0
            for c in cuts:
                n = int(c) - at
                k = M.out_samples(r, o, first + at, n)
                assert lib.efx_import_pcm_out_samples(r, o, first + at, n) == k
                parts, at = parts + k, int(c)
            assert parts == total, (r, o, first)
        out = subprocess.run([driver, "counts", str(r), str(o), str(BIG), "4321"], capture_output=True, text=True, check=True)
        assert out.stdout.split() == [str(M.out_samples(r, o, BIG, 4321)), str(W)]
    assert efx.import_pcm_out_samples(44100, 48000, 0, 44100) == 48000 and efx.import_pcm_delay(44100, 48000) == 16
    assert efx.import_pcm_delay(96000, 48000) == 32 and efx.import_pcm_delay(48000, 48000) == 0
    for bad in ((7999, 48000, 0, 1), (192001, 48000, 0, 1), (44100, 44101, 0, 1), (64001, 16000, 0, 1), (44100, 48000, -1, 1),
                (44100, 48000, 1 << 40, 1), (44100, 48000, 0, -1)):
        assert lib.efx_import_pcm_out_samples(*bad) == -1, bad
    assert lib.efx_import_pcm_delay(7999, 48000) == -1 and lib.efx_import_pcm_delay(48000, 22050) == -1
    assert lib.efx_import_pcm_state_bytes() == 256 == efx.import_pcm_state_bytes() == M.STATE_BYTES
    assert lib.efx_import_pcm_out_samples(8000, 48000, 0, 1 << 30) == -1  # more than 2^31 - 1 samples


def test_table_of_library_model_and_golden():
    import espflix_amd as efx
    lib = efx.load_library()
    assert lib.efx_import_pcm_filter(None, 0) == M.TABLE_LEN == 16 * M.P + 1
    got = np.full(M.TABLE_LEN + 3, 77, dtype=np.int32)
    assert lib.efx_import_pcm_filter(got.ctypes.data_as(C.c_void_p), M.TABLE_LEN) == M.TABLE_LEN
    assert (got[M.TABLE_LEN:] == 77).all()
    golden = np.load(TABLE_NPY)
    assert golden.dtype == np.int32 and golden.shape == (M.TABLE_LEN,)
    assert np.array_equal(got[:M.TABLE_LEN], golden) and np.array_equal(M.table(), golden)
    assert np.array_equal(efx.import_pcm_filter(), golden)
    assert golden[0] == round(0.97 * 2 ** M.Q) and golden[-1] == 0 and abs(int(golden[-2])) < 100
    # the interpolated product fits 32 bits with room: |T[i + 1] - T[i]| < 2^14
    assert np.abs(np.diff(golden.astype(np.int64))).max() < (1 << 14)
    # the largest sum of |k| over the phases, the reason for the final clamp
    worst = max(np.abs(golden[ph::M.P].astype(np.int64)).sum() + np.abs(golden[M.P - ph::M.P].astype(np.int64)).sum()
                for ph in range(1, M.P))
    print("largest sum of |k| / 2^Q:", worst / 2 ** M.Q)
    assert 1.0 < worst / 2 ** M.Q < 2.3


# ---- the yardstick: float64, its own evaluation of p, shares nothing with the model or the header ----------------------------
PASS_BAND = [(44100, 48000, 1000), (44100, 48000, 10000), (44100, 48000, 16000), (8000, 48000, 1000), (8000, 48000, 3000),
             (96000, 48000, 1000), (96000, 48000, 15000)]
STOP_BAND = [(96000, 48000, 30000), (192000, 48000, 50000)]
AMPLITUDE, SECONDS = 30000, 0.1


def tone(r, hz):
    j = np.arange(int(round(SECONDS * r)))
    return np.round(AMPLITUDE * np.sin(2 * np.pi * hz * j / r)).astype(np.int16)


def yardstick(x, r, o):
    """y[n] = sum over j of p((j - (n r / o - W)) o / M) x[j] (x o / r when r > o), p in float64 with NumPy's sinc and i0,
    rounded to int16."""
    Mx = max(r, o)
    W = math.ceil(16 * Mx / o)
    n_out = math.ceil(x.size * o / r)
    centre = np.arange(n_out, dtype=np.float64) * r / o - W
    # every frame within 16 M / o of the centre, and one more on each side
    j = np.floor(centre)[:, None] + np.arange(-W - 1, W + 3, dtype=np.float64)[None, :]
    u = (j - centre[:, None]) * o / Mx
    inside = (np.abs(u) < 16) & (j >= 0) & (j < x.size)
    uc = np.where(inside, u, 0.0)
    p = np.where(inside, 0.97 * np.sinc(0.97 * uc) * np.i0(9 * np.sqrt(1 - (uc / 16) ** 2)) / np.i0(9.0), 0.0)
    y = (p * x.astype(np.float64)[np.clip(j, 0, x.size - 1).astype(np.int64)]).sum(axis=1)
    if r > o:
        y *= o / r
    return np.clip(np.rint(y), -32768, 32767).astype(np.int64)


def snr_against_the_sine(y, r, o, hz):
    """SNR of y against the analytic sine at time n r / o - W, over the outputs whose taps all lie inside the input."""
    W = math.ceil(16 * max(r, o) / o)
    n = np.arange(y.size)
    s = AMPLITUDE * np.sin(2 * np.pi * hz * (n * r / o - W) / r)
    first = math.ceil(2 * W * o / r) + 1
    d = y[first:] - s[first:]
    return 10 * math.log10((s[first:] ** 2).sum() / (d ** 2).sum())


def quality(driver, table_file, tmp):
    out = {}
    for r, o, hz in PASS_BAND:
        x = tone(r, hz)
        got, _ = run_driver(driver, table_file, tmp, x[:, None], r, o, M.INTERLEAVED, None, 0, (x.size,))
        out[f"{r}_{o}_{hz}"] = {"float64": round(snr_against_the_sine(yardstick(x, r, o), r, o, hz), 4),
                                "integer": round(snr_against_the_sine(got.astype(np.int64), r, o, hz), 4)}
    return out


def test_pass_band_against_the_float64_yardstick(driver, table_file, tmp_path):
    """Tones of amplitude 30000, 0.1 s: the integer path's SNR against the analytic sine is no more than 3.01 dB below
    that of the float64 evaluation of p rounded to int16 -- integer coefficients may add at most as much noise as the
    final rounding adds.  Both figures are those recorded in tests/golden/import_pcm_quality.json (0.01 dB)."""
    recorded = json.load(open(QUALITY_JSON))
    got = quality(driver, table_file, tmp_path)
    assert sorted(got) == sorted(recorded)
    failures = []
    for name, v in got.items():
        print(f"{name:20s} float64 {v['float64']:6.2f} dB | integer {v['integer']:6.2f} dB")
        assert abs(v["float64"] - recorded[name]["float64"]) <= 0.01 and abs(v["integer"] - recorded[name]["integer"]) <= 0.01, name
        if v["integer"] < v["float64"] - 3.01:
            failures.append((name, v))
    assert not failures, failures


@pytest.mark.parametrize("r,o,hz", STOP_BAND)
def test_stop_band_is_silent(driver, table_file, tmp_path, r, o, hz):
    """A tone above the output's Nyquist frequency: the float64 output rounds to all zeros, the integer path stays within 1."""
    x = tone(r, hz)
    skip = math.ceil(2 * math.ceil(16 * r / o) * o / r) + 1  # (the onset of the tone is not a stop-band signal)
    yf = yardstick(x, r, o)
    assert not yf[skip:].any()
    got, _ = run_driver(driver, table_file, tmp_path, x[:, None], r, o, M.INTERLEAVED, None, 0, (x.size,))
    print(f"{r} -> {o}, {hz} Hz: largest |y| {np.abs(got[skip:]).max()}")
    assert np.abs(got[skip:].astype(np.int64)).max() <= 1


if __name__ == "__main__":
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        tmp = pathlib.Path(d)
        if not os.path.exists(TABLE_NPY):
            np.save(TABLE_NPY, M.table().astype(np.int32))
        np.load(TABLE_NPY).astype(np.int32).tofile(tmp / "table.bin")
        res = quality(build(tmp, "drv", ["-O2"]), str(tmp / "table.bin"), tmp)
    for name, v in res.items():
        print(f"{name:20s} float64 {v['float64']:7.3f} dB | integer {v['integer']:7.3f} dB")
    with open(QUALITY_JSON, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    sys.exit(0)
