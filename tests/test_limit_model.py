"""The arithmetic of k_limit_peaks / k_pcm_limit (espflix_amd/csrc/limit_px.h, built here with the host compiler into
tests/limit_model_main.cpp -- once plainly, once under the address and undefined-behaviour sanitizers) against the NumPy
model of include/efx.h's rule (tests/limit_model.py); the rule's invariants; the halo; the header's quotients over their
whole ranges; the stream gain against the loudness model's gain; the peaky title the limiter was built for; the two option
records against the header.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import limit_model as M
import loudness_model as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_M1 = 29204  # -1 dBFS: loudness_model.thresholds(rate)[2]


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build limit_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "limit_model_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("limit"), "drv", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("limit_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def host_limit(exe, tmp, x, rate, H, G, C, first=0, row=None, peaks_first=0):
    src, pk, dst, gn = tmp / "x.bin", tmp / "p.bin", tmp / "y.bin", tmp / "g.bin"
    np.ascontiguousarray(x, dtype=np.int16).tofile(src)
    if row is not None:
        np.ascontiguousarray(row, dtype=np.uint16).tofile(pk)
    run(exe, "limit", rate, H, G, C, first, peaks_first, src, pk if row is not None else "-", dst, gn)
    return np.fromfile(dst, dtype=np.int16), np.fromfile(gn, dtype=np.uint16).astype(np.int64)


def host_peaks(exe, tmp, x, rate):
    src, dst = tmp / "px.bin", tmp / "pp.bin"
    np.ascontiguousarray(x, dtype=np.int16).tofile(src)
    run(exe, "peaks", rate, src, dst)
    return np.fromfile(dst, dtype=np.uint16)


# ---- the streams ---------------------------------------------------------------------------------------------------------------
def lengths(rate):
    bk = M.BLOCK[rate]
    return sorted({1, 7, bk - 1, bk, bk + 1, 65 * bk + 3})


def streams(rate, n, seed):
    """name -> int16 [n]: random ones of three kinds, and the directed ones."""
    rng = np.random.default_rng(seed)
    bk = M.BLOCK[rate]
    quiet = rng.integers(-900, 901, n)
    spiky = quiet.copy()
    spiky[rng.random(n) < 2.0 / bk / 8] = 32767
    spiky[rng.random(n) < 2.0 / bk / 8] = -32768
    loud = rng.integers(-32768, 32768, n)
    ramp = (np.arange(n) * 97 % 65536 - 32768)
    return {"quiet": quiet, "spiky": spiky, "loud": loud, "ramp": ramp, "silent": np.zeros(n, np.int64), "floor": np.full(n, -32768),
            "lone": np.where(np.arange(n) == n // 2, 32767, 0)}


def check_invariants(x, y, g, rate, G, C):
    bk = M.BLOCK[rate]
    r = M.required(M.peaks(x, rate), G, C)
    assert np.abs(y.astype(np.int64)).max(initial=0) <= C
    assert (g <= np.repeat(r, bk)[:len(x)]).all() and (g >= 0).all()
    if (r >= G).all():
        assert np.array_equal(y, L.apply_gain(x, G))


# ---- the header against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", L.RATES)
def test_header_equals_the_model(driver, tmp_path, rate):
    """Every length x H x C x G on one kind of stream each (the kinds go round), and every kind at the longest length."""
    cases = []
    kinds = list(streams(rate, 1, 0))
    k = 0
    for n in lengths(rate):
        for H in (1, 32, 64):
            for C in (1, C_M1, 32767):
                for G in (1, 4096, 32767):
                    cases.append((n, kinds[k % len(kinds)], H, C, G))
                    k += 1
    n = lengths(rate)[-1]
    cases += [(n, kind, 32, C_M1, 32767) for kind in kinds] + [(n, kind, 1, 32767, 4096) for kind in kinds]
    for n, kind, H, C, G in cases:
        x = streams(rate, n, n + H)[kind].astype(np.int16)
        want, wg = M.limit(x, rate, G, C, H, want_gains=True)
        got, gg = host_limit(driver, tmp_path, x, rate, H, G, C)
        assert np.array_equal(host_peaks(driver, tmp_path, x, rate), M.peaks(x, rate)), (n, kind)
        assert np.array_equal(gg, wg) and np.array_equal(got, want), (n, kind, H, C, G)
        check_invariants(x, want, wg, rate, G, C)


def test_sanitized_host_program(sanitized, tmp_path):
    for rate, n, H in ((16000, 17, 1), (44100, 65 * 48 + 3, 64), (32000, 31, 32)):
        x = streams(rate, n, 5)["spiky"].astype(np.int16)
        got, _ = host_limit(sanitized, tmp_path, x, rate, H, 32767, C_M1)
        assert np.array_equal(got, M.limit(x, rate, 32767, C_M1, H))
        assert np.array_equal(host_peaks(sanitized, tmp_path, x, rate), M.peaks(x, rate))


def test_full_scale_negative_counts_as_32768():
    x = np.zeros(100, np.int16)
    x[40] = -32768
    assert M.peaks(x, 16000).tolist() == [0, 0, 32768, 0, 0, 0, 0]
    y, g = M.limit(x, 16000, 4096, 32767, 1, want_gains=True)
    assert g[40] == 4096 * 32767 // 32768 == 4095 and y[40] == -32760 and abs(int(y[40])) <= 32767


def test_unlimited_stream_is_pcm_gain_bit_for_bit():
    rng = np.random.default_rng(3)
    for rate in L.RATES:
        x = rng.integers(-2000, 2001, 70 * M.BLOCK[rate] + 5).astype(np.int16)
        for G in (1, 4095, 4096, 32767):
            assert 2000 * G <= 4096 * C_M1
            assert np.array_equal(M.limit(x, rate, G, C_M1, 32), L.apply_gain(x, G))


# ---- the halo --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (1, 3, 32, 64))
def test_a_piece_needs_2H_plus_1_blocks_either_side_and_no_more(driver, tmp_path, H):
    rate, G, C = 16000, 32767, C_M1
    bk = M.BLOCK[rate]
    b0, b1 = 2 * H + 4, 2 * H + 9              # the piece: blocks b0 .. b1 - 1
    nb = b1 + 2 * H + 4
    rng = np.random.default_rng(H)
    x = rng.integers(-300, 301, nb * bk).astype(np.int16)
    x[rng.integers(0, nb * bk, 12)] = 30000
    whole = M.limit(x, rate, G, C, H)
    p = M.peaks(x, rate)
    lo, hi = b0 - 2 * H - 1, b1 + 2 * H        # the halo, inclusive
    row = np.zeros_like(p)
    row[lo:hi + 1] = p[lo:hi + 1]
    piece = x[b0 * bk:b1 * bk]
    for r, pf in ((row, 0), (p[lo:hi + 1], lo)):  # zeros elsewhere; or a row that holds the halo only
        got = M.limit(piece, rate, G, C, H, first_sample=b0 * bk, row=r, peaks_first=pf)
        assert np.array_equal(got, whole[b0 * bk:b1 * bk])
        assert np.array_equal(host_limit(driver, tmp_path, piece, rate, H, G, C, first=b0 * bk, row=r, peaks_first=pf)[0], got)
    # a lone full-scale sample at the halo's edge shows in the piece; one block further out it does not
    quiet = np.full(nb * bk, 100, np.int16)
    base = M.limit(quiet, rate, G, C, H)[b0 * bk:b1 * bk]
    for blk, shows in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False)):
        z = quiet.copy()
        z[blk * bk + 3] = 32767
        got = M.limit(z, rate, G, C, H)[b0 * bk:b1 * bk]
        assert (not np.array_equal(got, base)) == shows, (blk, shows)


# ---- the quotients and the gain ------------------------------------------------------------------------------------------------
def test_quotients_over_their_whole_ranges(driver):
    """floor(n / Bk) as a multiply and a shift for every numerator of the three block lengths, the piece-to-block quotient,
    the numerator's steps modulo 2^32, required() against 64-bit division for p = 1 .. 32768, the average, the peak."""
    assert run(driver, "quotients").strip() == "ok"


def test_stream_gain_is_the_uncapped_loudness_gain(driver):
    rng = np.random.default_rng(9)
    for rate in L.RATES:
        step = L.step_of(rate)
        _, T, C = L.thresholds(rate)
        for mean in [0, 1, 5, 10 ** 6, 10 ** 12, 10 ** 15, 2 ** 55] + [int(v) for v in rng.integers(1, 2 ** 50, 20)]:
            for n_gated in (0, 1, 77):
                G = M.stream_gain(mean, n_gated, T, step)
                assert int(run(driver, "gain", mean, n_gated, T, step)) == G and 1 <= G <= 32767
                assert G == L.gain_q12(mean, n_gated, 1, T, 32767, step)      # peak 1: the cap 4096 x 32767 never binds
                # gain_q12 itself, now made from the stream gain, gives what the loudness model's rule gives: a peak of 0, one
                # that does not bind, ones that do
                for peak in (0, 1, 1000, 32768):
                    want = L.gain_q12(mean, n_gated, peak, T, C, step)
                    assert want == (L.UNITY if n_gated == 0 or peak == 0 else max(1, min(G, 4096 * C // peak)))
                    assert int(run(driver, "capped", mean, n_gated, peak, T, C, step)) == want
    assert M.stream_gain(123, 0, 10 ** 9, 1600) == 4096


def test_binding_limit_gain_and_block():
    import espflix_amd as efx
    for rate in L.RATES:
        assert efx.limit_block(rate) == M.BLOCK[rate]
        _, T, _ = L.thresholds(rate)
        for mean, n in ((0, 0), (0, 3), (10 ** 9, 3), (10 ** 14, 1), (2 ** 55, 9)):
            assert efx.limit_gain(mean, n, T, rate) == M.stream_gain(mean, n, T, L.step_of(rate))
    assert efx.limit_block(22050) == 0 and efx.limit_gain(1, 1, 1, 22050) == 0 and efx.limit_gain(1, 1, 1 << 40, 48000) == 0


# ---- the title the limiter was built for ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (16000, 48000))
def test_peaky_title_reaches_the_target(rate):
    """Noise and a tone at -31.1 LUFS with 6 ms of full-scale bursts, target -23 LUFS, ceiling -1 dBFS, H = 32.  Measured
    with the loudness model: the linear chain leaves it at -31.96 (16 kHz) / -31.90 LUFS (48 kHz); limited it comes to
    -24.36 / -24.32 LUFS with an output peak of 29203 / 29201 against C = 29204.

    The peak: the loudest block of a neighbourhood has the smallest r there, so both its nodes are r and its loudest
    sample p comes out as (p floor(4096 C / p) + 2048) >> 12, which lies in C - 8 .. C for p <= 32768 (the floor loses less
    than p of 4096 C).  The output peak is therefore the ceiling to within those 8, and never above it."""
    x = M.peaky_title(rate)
    abs_thr, T, C = L.thresholds(rate, -23.0, -1.0)
    assert C == C_M1
    rec, before = L.measure(x, rate)
    G = M.stream_gain(int(rec["gated_mean"]), int(rec["n_gated"]), T, L.step_of(rate))
    linear = L.measure(L.apply_gain(x, int(rec["gain_q12"])), rate)[1]
    y, g = M.limit(x, rate, G, C, 32, want_gains=True)
    limited = L.measure(y, rate)[1]
    peak = int(np.abs(y.astype(np.int64)).max())
    print(f"{rate}: in {before:.2f} LUFS, G {G}, capped {int(rec['gain_q12'])}, linear {linear:.2f}, limited {limited:.2f}, "
          f"peak {peak} of {C}, touched {(g < G).mean():.4f}")
    assert linear < -23.0 - 8.0
    assert abs(limited - -23.0) < 2.0
    assert C - 8 <= peak <= C
    check_invariants(x, y, g, rate, G, C)


# ---- the binding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_name,py_name", [("efx_limit_peaks_opts", "LIMIT_PEAKS_OPTS_DTYPE"), ("efx_limit_opts", "LIMIT_OPTS_DTYPE")])
def test_record_dtypes_match_the_header(tmp_path, c_name, py_name):
    """The dtypes against the structs as the host C compiler lays them out: size, and every field's name, order, offset and
    size."""
    from espflix_amd import _abi
    import espflix_amd as efx
    import test_abi_layout as A
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a host C compiler is needed to lay out include/efx.h"
    dt = getattr(_abi, py_name)
    assert getattr(efx, py_name) is dt and list(dt.names) == A.header_fields(c_name)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "efx.h"', "int main(void) {", f'  printf("%zu\\n", sizeof({c_name}));']
    for f in dt.names:
        lines.append(f'  printf("%zu %zu\\n", offsetof({c_name}, {f}), sizeof((({c_name} *)0)->{f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert dt.itemsize == int(out[0])
    for name, line in zip(dt.names, out[1:]):
        sub, offset = dt.fields[name][:2]
        assert [offset, sub.itemsize] == [int(v) for v in line.split()], name
    assert sum(dt.fields[n][0].itemsize for n in dt.names) == dt.itemsize, "a hole: the header has a field the dtype lacks"
