"""The rule of efx_denoise: whole calls on the host through espflix_amd/csrc/denoise_px.h with the kernel's own walk
(tests/denoise_model_main.cpp, built here with the host compiler) against the NumPy model of include/efx.h's definition
(tests/denoise_model.py), the properties the definition has, the record dtype of its options against the header, and
what it is worth on a noisy moving picture.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_model as M
import surface_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (4, 2), (18, 6), (34, 10)]
FRAMES = [1, 2, 5]
THRESHOLDS = [0, 1, 7, 64]
NAMES = ("luma_spatial", "chroma_spatial", "luma_temporal", "chroma_temporal")


def compile_main(tmp, name, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build denoise_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "denoise_model_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return compile_main(tmp_path_factory.mktemp("denoise_px"), "drv", "-O2")


def host_call(exe, srcs, s, n_streams=1, prev=None, **thr):
    """One call of the host program: (n_streams * n_frames, w h 3 / 2), or the exit status of a refused call."""
    n_frames = len(srcs) // n_streams
    data = np.ascontiguousarray(srcs).tobytes() + (np.ascontiguousarray(prev).tobytes() if prev is not None else b"")
    r = subprocess.run([exe, "call", *[str(v) for v in s.args()], str(n_streams), str(n_frames), *[str(thr.get(k, 0)) for k in NAMES],
                        "1" if prev is not None else "0"], input=data, capture_output=True, timeout=300)
    if r.returncode:
        return r.returncode
    return np.frombuffer(r.stdout, dtype=np.uint8).reshape(n_streams * n_frames, s.width * s.height * 3 // 2)


def surfaces(w, h):
    """The layouts a size runs in: packed and pitched planar (YV12 by swapped offsets), NV12 with a pitch and NV21."""
    return [("i420", S.layout("i420", w, h)), ("yv12 pitched", S.layout("yv12", w, h, (w + 9) // 2 * 2, h + 2)),
            ("nv12", S.layout("nv12", w, h, w + 5)), ("nv21", S.layout("nv21", w, h))]


def directed(n, s, seed):
    """n images of one stream that the thresholds cut through: a static ramp with a step in it and noise of a few levels
    that changes from frame to frame, a block of 0 and one of 255 that swap every frame.  The padding is noise."""
    rng = np.random.default_rng(seed)
    at = np.arange(s.bytes)
    base = (at * 5 // max(1, s.width)) % 200 + np.where(at % max(2, s.width) >= s.width // 2, 40, 0)
    out = np.empty((n, s.bytes), dtype=np.uint8)
    mask = S.sample_mask(s)
    for t in range(n):
        v = base + rng.integers(0, 9, s.bytes) - 4
        lo, hi = (0, 255) if t & 1 else (255, 0)
        v[: s.bytes // 7] = lo
        v[s.bytes // 7: s.bytes // 5] = hi
        img = rng.integers(0, 256, s.bytes)
        img[mask] = np.clip(v, 0, 255)[mask]
        out[t] = img
    return out


def settings():
    """All four thresholds alike at every listed value, and one setting in which all four differ."""
    return [dict.fromkeys(NAMES, t) for t in THRESHOLDS] + [dict(luma_spatial=7, chroma_spatial=1, luma_temporal=64, chroma_temporal=0),
                                                           dict(luma_spatial=0, chroma_spatial=64, luma_temporal=1, chroma_temporal=7)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_header_matches_model(host, w, h):
    """Random and directed planes, every layout, 1, 2 and 5 frames, thresholds 0, 1, 7 and 64: the header's walk writes what
    the definition says, byte for byte."""
    for k, (name, s) in enumerate(surfaces(w, h)):
        assert s is not None and M.accepts(s), name
        for make in (S.sources, directed):
            for n in FRAMES:
                srcs = make(n, s, 100 * w + 10 * k + n)
                for thr in settings():
                    got = host_call(host, srcs, s, **thr)
                    assert not isinstance(got, int), (name, n, thr, got)
                    assert np.array_equal(got, M.denoise(srcs, s, **thr)), (name, make.__name__, n, thr)


def test_wide_planes_and_streams_on_the_host(host):
    """A plane wider than a tile (its chroma planes no longer share a wave), more bands than one, and three streams."""
    tile, band = (int(v) for v in subprocess.run([host, "tile"], capture_output=True, text=True, check=True).stdout.split())
    assert (tile, band) == (992, 4)
    thr = dict(luma_spatial=7, chroma_spatial=5, luma_temporal=9, chroma_temporal=12)
    s = S.layout("nv12", tile + 2, 4)
    srcs = directed(2, s, 5)
    assert np.array_equal(host_call(host, srcs, s, **thr), M.denoise(srcs, s, **thr))
    s = S.layout("i420", 18, 2 * band + 2)
    srcs = np.concatenate([directed(2, s, 6 + i) for i in range(3)])
    got = host_call(host, srcs, s, n_streams=3, **thr)
    assert np.array_equal(got, M.denoise(srcs, s, 3, **thr))
    assert np.array_equal(got[2:4], M.denoise(srcs[2:4], s, **thr)), "streams see each other"


def test_refused_calls_on_the_host(host):
    s = S.layout("i420", 18, 6)
    srcs = S.sources(1, s, 1)
    for thr in (dict(luma_spatial=65), dict(chroma_spatial=-1), dict(luma_temporal=65), dict(chroma_temporal=-1)):
        assert host_call(host, srcs, s, **thr) == 1, thr
    assert not M.accepts(S.layout("p010", 18, 6)) and host_call(host, srcs, S.layout("p010", 18, 6)) == 1


def test_sanitized_pitched_nv12_call(tmp_path):
    """The stand-alone program under the address and undefined-behaviour sanitizers, once: a pitched 18 x 6 NV12 call of
    two streams with a previous output, on blocks of exactly the bytes the contract names."""
    exe = compile_main(tmp_path, "drv_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
    s = S.layout("nv12", 18, 6, 23, 8)
    srcs = np.concatenate([directed(3, s, 7), S.sources(3, s, 8)])
    prev = np.random.default_rng(9).integers(0, 256, (2, 18 * 6 * 3 // 2), dtype=np.uint8)
    thr = dict(luma_spatial=12, chroma_spatial=9, luma_temporal=24, chroma_temporal=64)
    got = host_call(exe, srcs, s, n_streams=2, prev=prev, **thr)
    assert not isinstance(got, int), got
    assert np.array_equal(got, M.denoise(srcs, s, 2, prev=prev, **thr))


def test_temporal_step_exhaustively(host):
    """For all s, P in 0 .. 255 and Tt in 1 .. 64: out lies between s and P, out == P only when |s - P| <= 1, k <= 256,
    a a Q < 2^24 where it is used, the step is symmetric in the sign of d, and the header's packed step gives the same."""
    s, P = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    a = np.abs(s - P)
    r = subprocess.run([host, "blend"], capture_output=True, timeout=300)
    assert r.returncode == 0 and len(r.stdout) == 64 * 65536
    header = np.frombuffer(r.stdout, dtype=np.uint8).reshape(64, 256, 256)
    for tt in range(1, 65):
        out = M.temporal(s, P, tt)
        assert np.array_equal(out, header[tt - 1]), tt
        assert np.all((out >= np.minimum(s, P)) & (out <= np.maximum(s, P))), tt
        assert np.all(a[out == P] <= 1), tt
        k = M.blend_k(a, tt)
        assert k.max() <= 256 and k.min() >= 64, tt
        q = 12582912 // (tt * tt)
        assert (a[a < tt] ** 2 * q).max(initial=0) < 1 << 24, tt
        assert np.array_equal(out - P, -(M.temporal(P, s, tt) - s)), tt
        assert np.array_equal(out[a >= tt], s[a >= tt]), tt
    assert np.array_equal(M.temporal(s, P, 0), s) and np.array_equal(M.temporal(s, None, 24), s)


def test_all_thresholds_zero_is_the_identity(host):
    for name, s in surfaces(34, 10):
        srcs = S.sources(3, s, 11)
        want = S.canonicals(srcs, s)
        assert np.array_equal(M.denoise(srcs, s), want) and np.array_equal(host_call(host, srcs, s), want), name


def test_a_constant_plane_is_a_fixed_point(host):
    s = S.layout("i420", 18, 6)
    for level in (0, 1, 128, 255):
        srcs = np.full((3, s.bytes), level, dtype=np.uint8)
        thr = dict(luma_spatial=64, chroma_spatial=7, luma_temporal=64, chroma_temporal=1)
        assert np.all(M.denoise(srcs, s, **thr) == level) and np.all(host_call(host, srcs, s, **thr) == level)


def test_pieces_with_prev_equal_the_whole(host):
    """Two streams of 5 frames as pieces of 2 + 3 with the last output of the first piece as prev: model and header."""
    thr = dict(luma_spatial=7, chroma_spatial=3, luma_temporal=24, chroma_temporal=12)
    for name, s in surfaces(34, 10):
        a, b = directed(5, s, 12), directed(5, s, 13)
        whole = M.denoise(np.concatenate([a, b]), s, 2, **thr)
        for call in (lambda srcs, **kw: M.denoise(srcs, s, **kw), lambda srcs, **kw: host_call(host, srcs, s, **kw)):
            first = call(np.concatenate([a[:2], b[:2]]), n_streams=2, **thr)
            second = call(np.concatenate([a[2:], b[2:]]), n_streams=2, prev=first[[1, 3]], **thr)
            joined = np.concatenate([first[0:2], second[0:3], first[2:4], second[3:6]])
            assert np.array_equal(joined, whole), name
        assert not np.array_equal(M.denoise(np.concatenate([a[2:], b[2:]]), s, 2, **thr), whole[[2, 3, 4, 7, 8, 9]]), "prev does not matter here"


def test_options_dtype_matches_the_header(tmp_path):
    """DENOISE_OPTS_DTYPE against efx_denoise_opts as the host C compiler lays it out: size, and every field's name, order,
    offset and size."""
    from espflix_amd import _abi
    import espflix_amd as efx
    import test_abi_layout as A
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a host C compiler is needed to lay out include/efx.h"
    dt = _abi.DENOISE_OPTS_DTYPE
    assert efx.DENOISE_OPTS_DTYPE is dt and list(dt.names) == A.header_fields("efx_denoise_opts")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "efx.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(efx_denoise_opts));']
    for f in dt.names:
        lines.append(f'  printf("%zu %zu\\n", offsetof(efx_denoise_opts, {f}), sizeof(((efx_denoise_opts *)0)->{f}));')
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


def test_thresholds_for_a_noise_level():
    import espflix_amd as efx
    assert efx.denoise_thresholds(6) == (12, 12, 24, 24) == M.thresholds(6)
    assert efx.denoise_thresholds(3) == (6, 6, 12, 12) and efx.denoise_thresholds(0) == (0, 0, 0, 0)
    assert efx.denoise_thresholds(1.3) == (3, 3, 5, 5) and efx.denoise_thresholds(40) == (64, 64, 64, 64)
    for sigma in (0.2, 2.5, 7.75, 15.9, 16.1):
        assert efx.denoise_thresholds(sigma) == M.thresholds(sigma)
    with pytest.raises(ValueError):
        efx.denoise_thresholds(-1)


# ---- what it is worth -------------------------------------------------------------------------------------------------------------
W, H, N = 64, 48, 16


def scene():
    """The clean scene: a smooth gradient with two hard edges and a 12-wide bright block moving 3 pels a frame."""
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    base = (96 + 40 * np.sin(x / 7) + 30 * np.cos(y / 5)).astype(np.int64)
    base[:, 40:] = 200
    base[10:20, 5:25] = 30
    clean = np.repeat(base[None], N, axis=0)
    for t in range(N):
        x0 = 3 * t % 52
        clean[t, 24:36, x0:x0 + 12] = 235
    return clean


def psnr(a, b):
    """Mean over frames 4 .. 15 of the frame's PSNR."""
    mse = ((a[4:].astype(np.float64) - b[4:]) ** 2).mean(axis=(1, 2))
    return float(np.mean(10 * np.log10(255.0 ** 2 / mse)))


def test_quality_on_the_noisy_moving_scene(host):
    """sigma = 6 at Ts = 12, Tt = 24: the gains a NumPy prototype of the rule measured were +2.35 spatial, +4.62 temporal
    and +7.19 dB both (include/efx.h's settings); the floors sit about a quarter below.  The largest error in the moving
    block's rows stays within 5 of the noisy input's."""
    clean = scene()
    noise = np.rint(np.random.default_rng(1).normal(0, 6, clean.shape)).astype(np.int64)
    noisy = np.clip(clean + noise, 0, 255).astype(np.uint8)
    before = psnr(noisy, clean)
    # (the header's walk on the same frames, as the luma of I420 pictures with flat chroma, must give the model's pictures)
    surface = S.layout("i420", W, H)
    i420 = np.concatenate([noisy.reshape(N, -1), np.full((N, W * H // 2), 128, dtype=np.uint8)], axis=1)
    worst_in = np.abs(noisy[:, 24:36].astype(np.int64) - clean[:, 24:36]).max()
    for name, ts, tt, floor in (("spatial", 12, 0, 1.8), ("temporal", 0, 24, 3.5), ("both", 12, 24, 6.0)):
        out = M.denoise_plane(noisy, ts, tt)
        assert np.array_equal(host_call(host, i420, surface, luma_spatial=ts, luma_temporal=tt)[:, :W * H].reshape(N, H, W), out), name
        gain = psnr(out, clean) - before
        worst = np.abs(out[:, 24:36].astype(np.int64) - clean[:, 24:36]).max()
        print(f"{name}: {before:.2f} dB -> +{gain:.2f} dB; largest error in rows 24 .. 35: {worst} (noisy: {worst_in})")
        assert gain >= floor, (name, gain)
        assert worst <= worst_in + 5, (name, worst, worst_in)
    print(f"a clean input through both steps: {psnr(M.denoise_plane(clean.astype(np.uint8), 12, 24), clean):.2f} dB")
