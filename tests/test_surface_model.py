"""The arithmetic of the surface loaders (espflix_amd/csrc/surface_px.h, built here with the host compiler) against the
NumPy model of include/efx.h's definition (tests/surface_model.py): the reduction of every word at every shift, the
conventional layouts and the checks; and whole imports and detections on the host with the kernels' index arithmetic
(tests/surface_model_main.cpp) under the address and undefined-behaviour sanitizers, the source in a heap block of exactly
the memory contract's size.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import surface_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_GEOMETRIES = [g for g in S.GEOMETRIES if g[1:3] != (1920, 1080)]


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build surface_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "surface_model_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("surface_px"), "drv", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("surface_px_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def test_model_reduction_anchors():
    assert int(S.reduce(940 << 6, 8)) == 235          # P010 white
    assert int(S.reduce(1023 << 6, 8)) == 255
    assert int(S.reduce(0xFFFF, 8)) == 255            # (a wrapping packed add turns this into 0)
    assert int(S.reduce(64, 2)) == 16                 # yuv420p10le black
    assert int(S.reduce(64 << 6, 8)) == 16 and int(S.reduce(256, 4)) == 16
    for shift in range(1, 9):
        assert int(S.reduce(0xFFFF, shift)) == 255 and int(S.reduce(0, shift)) == 0
    # a reduced 10-bit sample is off by at most 0.75 of an 8-bit step: half a step of rounding, 0.75 where 1023 saturates
    w = np.arange(1024)
    assert np.abs(S.reduce(w, 2).astype(float) - np.minimum(w / 4, 255.75)).max() <= 0.75


@pytest.mark.parametrize("shift", range(1, 9))
def test_header_reduction_matches_model_everywhere(driver, shift):
    """All 65536 words through reduce() and through the packed reduce4() (which also exits 3 when a 0xFFFF beside the
    word does not come out as 255)."""
    r = subprocess.run([driver, "reduce", str(shift)], capture_output=True, timeout=120)
    assert r.returncode == 0, "the packed reduction lets 0xFFFF wrap"
    got = np.frombuffer(r.stdout, dtype=np.uint8).reshape(2, 65536)
    want = S.reduce(np.arange(65536), shift)
    for path, g in zip(("reduce", "reduce4"), got):
        bad = np.flatnonzero(g != want)
        assert bad.size == 0, f"{path}, shift {shift}: {bad.size} words differ, first {bad[0]}"
    if shift == 8:
        assert got[0, 940 << 6] == 235 and got[0, 1023 << 6] == 255 and got[0, 0xFFFF] == 255 and got[1, 0xFFFF] == 255
    if shift == 2:
        assert got[0, 64] == 16 and got[1, 64] == 16


LAYOUT_CASES = [(k, w, h, p, r) for k in S.KINDS for (w, h, p, r) in
                ((1920, 1080, 0, 0), (1920, 1080, 4096, 1088), (34, 18, 76, 20), (2, 2, 0, 0), (4096, 4096, 0, 0),
                 (16, 16, 8, 0), (16, 16, 0, 14), (16, 16, 0, 17), (17, 16, 0, 0), (16, 4098, 0, 0), (34, 18, 70, 0),
                 (34, 18, 1 << 20, 0), (34, 18, (1 << 20) + 4, 0))]


def header_layout(driver, kind, w, h, pitch, rows):
    r = subprocess.run([driver, "layout", str(S.KINDS[kind][0]), str(w), str(h), str(pitch), str(rows)], capture_output=True,
                       text=True, check=True, timeout=60)
    v = [int(x) for x in r.stdout.split()]
    return v[0], S.Surface(*v[1:6], v[6:9], v[9:12], v[12])


def test_layout_helper(driver):
    import espflix_amd as efx
    lib = efx.load_library()
    rejected = 0
    for kind, w, h, pitch, rows in LAYOUT_CASES:
        want = S.layout(kind, w, h, pitch, rows)
        got_bytes, got = header_layout(driver, kind, w, h, pitch, rows)
        lib_s = efx._Surface()
        lib_bytes = lib.efx_surface_layout(S.KINDS[kind][0], w, h, pitch, rows, C.byref(lib_s))
        if want is None:
            rejected += 1
            assert got_bytes == 0 and lib_bytes == 0, (kind, w, h, pitch, rows)
            with pytest.raises(ValueError):
                efx.surface_layout(kind, w, h, pitch, rows)
            continue
        assert got_bytes == want.bytes == lib_bytes and got == want, (kind, w, h, pitch, rows, got, want)
        py = efx.surface_layout(kind, w, h, pitch, rows)
        for s in (lib_s, py):
            assert S.Surface(s.layout, s.shift, s.swap_uv, s.width, s.height, list(s.offset), list(s.pitch), s.bytes) == want
    assert rejected >= 5 * len(S.KINDS)
    nv12 = S.layout("nv12", 1920, 1080, 2048, 1088)
    assert nv12.offset[1] == 2_228_224 and nv12.bytes == 3_342_336 and nv12.pitch[1] == 2048
    yv12, i420 = S.layout("yv12", 16, 16), S.layout("i420", 16, 16)
    assert yv12.offset[2] == 256 and yv12.offset[1] == 320 and i420.offset[1] == 256 and i420.offset[2] == 320  # Cr first
    assert S.layout("p010", 1920, 1080).pitch[0] == 3840 and S.layout("p010", 1920, 1080).shift == 8
    assert S.layout("i010", 16, 16).shift == 2 and S.layout("i012", 16, 16).shift == 4 and S.layout("nv21", 16, 16).swap_uv == 1
    assert lib.efx_surface_layout(10, 16, 16, 0, 0, C.byref(efx._Surface())) == 0
    assert lib.efx_surface_layout(-1, 16, 16, 0, 0, C.byref(efx._Surface())) == 0
    assert lib.efx_surface_layout(2, 16, 16, 0, 0, None) == 0
    with pytest.raises(ValueError):
        efx.surface_layout("yuyv", 16, 16)


def test_checks(driver):
    for kind, w, h, pitch, rows, *_ in S.GEOMETRIES:
        s = S.layout(kind, w, h, pitch, rows)
        assert S.check(s)
        r = subprocess.run([driver, "check", *map(str, s.args())], capture_output=True, text=True, check=True)
        assert int(r.stdout) == 0
    # the last row may end exactly at bytes, and not one byte beyond
    s = S.layout("nv12", 34, 18, 50)
    tight = replace(s, bytes=s.offset[1] + 8 * 50 + 34)
    for t, ok in ((tight, True), (replace(tight, bytes=tight.bytes - 1), False)):
        assert S.check(t) == ok
        r = subprocess.run([driver, "check", *map(str, t.args())], capture_output=True, text=True, check=True)
        assert (int(r.stdout) == 0) == ok
    for what, b in S.rejected_surfaces():
        assert not S.check(b), (what, b)
        r = subprocess.run([driver, "check", *map(str, b.args())], capture_output=True, text=True, check=True)
        assert int(r.stdout) != 0, (what, b)


def test_canonical_image_and_fields():
    """The model's canonical image against samples written plane by plane, and the field recipe against row slicing."""
    rng = np.random.default_rng(7)
    w, h = 8, 8
    y = rng.integers(0, 1 << 16, (h, w)).astype(np.uint16)
    cb, cr = (rng.integers(0, 1 << 16, (h // 2, w // 2)).astype(np.uint16) for _ in range(2))
    s = S.layout("p010", w, h, 24, 10)
    img = rng.integers(0, 256, s.bytes, dtype=np.uint8)
    words = img.view("<u2")
    for r in range(h):
        words[r * 12:r * 12 + w] = y[r]
    for r in range(h // 2):
        words[(s.offset[1] + r * 24) // 2:(s.offset[1] + r * 24) // 2 + w] = np.stack([cb[r], cr[r]], axis=1).reshape(-1)
    want = np.concatenate([S.reduce(p, 8).reshape(-1) for p in (y, cb, cr)])
    assert np.array_equal(S.canonical(img, s), want)
    swapped = np.concatenate([S.reduce(p, 8).reshape(-1) for p in (y, cr, cb)])
    assert np.array_equal(S.canonical(img, replace(s, swap_uv=1)), swapped)
    frame = S.canonical(img, s)
    fy, fu, fv = frame[:64].reshape(8, 8), frame[64:80].reshape(4, 4), frame[80:].reshape(4, 4)
    for bottom in (0, 1):
        f = S.field_of(s, bottom)
        assert S.check(f) and f.height == 4 and f.pitch[0] == 48
        want = np.concatenate([p[bottom::2].reshape(-1) for p in (fy, fu, fv)])
        assert np.array_equal(S.canonical(img, f), want)


def run_host(exe, mode, s, tail, src, stride, tmp_path):
    n = len(src)
    (tmp_path / "src.bin").write_bytes(src.tobytes())
    run = subprocess.run([exe, mode, *map(str, s.args()), *map(str, tail), str(tmp_path / "src.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    return n


@pytest.mark.parametrize("kind,w,h,pitch,rows,n,crop,rect", HOST_GEOMETRIES)
def test_whole_import_and_detection_under_sanitizers(sanitized, tmp_path, kind, w, h, pitch, rows, n, crop, rect):
    """The kernels' addressing on the host, the source in a heap block of exactly src_stride x (n - 1) + bytes rounded up
    to 16: the run is clean under -fsanitize=address,undefined and the outputs are the model's."""
    s = S.layout(kind, w, h, pitch, rows)
    src = S.sources(n, s, w * 31 + h)
    stride = (s.bytes + 15) // 16 * 16 + (32 if n > 1 else 0)
    c, r = crop or (0, 0, w, h), rect or (0, 0, 352, 192)
    run_host(sanitized, "import", s, [n, stride, *c, *r], src, stride, tmp_path)
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(n, -1)
    want = S.import_images(src, s, c, r)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first (image, byte) = {bad[0].tolist()}"

    box = (2 * (w // 8), 2 * (h // 8), w - 4 * (w // 8), h - 4 * (h // 8)) if w >= 16 else (0, 0, w, h)
    src = S.boxed(n, s, box, w + h)
    run_host(sanitized, "crop", s, [1, n, stride, 24, 2], src, stride, tmp_path)
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.uint32)
    sums, recs = S.detect(src, s, None, 24, 2)
    assert np.array_equal(raw[:n * (h + w)].reshape(n, h + w), sums)
    assert np.array_equal(raw[n * (h + w):].view(np.int32).reshape(1, 8), recs)
    if w >= 16:
        assert tuple(recs[0, :4]) == box
