"""The arithmetic of k_cropdetect (espflix_amd/csrc/crop_px.h, built here with the host compiler) against the NumPy model
of include/efx.h's definition (tests/crop_model.py) and against the properties the definition states, cover_crop against
its defining inequalities, and a whole detection on the host with the kernels' index arithmetic
(tests/crop_model_main.cpp) under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import crop_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"i420": 0, "rgb24": 1, "rgbp": 2}


def src_bytes(fmt, w, h):
    return w * h * 3 // 2 if fmt == "i420" else w * h * 3


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build crop_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "crop_model_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("crop_px"), "drv", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("crop_px_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.mark.parametrize("full_range", [False, True])
def test_header_luma_matches_model_everywhere(driver, full_range):
    """All 2^24 triples; the driver also exits 1 when a luma is not the low byte of ipx::ycbcr."""
    r = subprocess.run([driver, "luma", str(int(full_range))], capture_output=True, timeout=300)
    assert r.returncode == 0, "cpx::luma differs from the low byte of ipx::ycbcr"
    got = np.frombuffer(r.stdout, dtype=np.uint8).reshape(256, 256, 256)
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for red in range(256):
        want = M.rgb_luma(np.full_like(g, red), g, b, full_range)
        bad = np.argwhere(got[red] != want)
        assert bad.size == 0, f"R = {red}: {len(bad)} triples differ, first (G, B) = {bad[0].tolist()}"
    if not full_range:
        assert got[0, 0, 0] == 16 and got[255, 255, 255] == 235 and got[255, 0, 0] == 82
    else:
        assert got[0, 0, 0] == 0 and got[255, 255, 255] == 255


@pytest.mark.parametrize("r", [2, 4, 16, 64])
def test_header_rounding_matches_model_and_its_properties(driver, r):
    out = subprocess.run([driver, "round", str(r)], capture_output=True, check=True, timeout=60)
    rec = np.frombuffer(out.stdout, dtype=np.int32).reshape(-1, 3)
    k = 0
    for a in range(70):
        for b in range(a, 70):
            ok, pos, length = (int(v) for v in rec[k])
            k += 1
            want = M.round_axis(a, b, r)
            assert (ok == 1) == (want is not None), (a, b, r)
            # the axis fails exactly when no two lines from an even position fit
            a_even = a + (a & 1)
            assert (ok == 1) == (b + 1 - a_even >= 2), (a, b, r)
            if not ok:
                continue
            assert (pos, length) == want, (a, b, r)
            avail = b + 1 - a_even
            assert pos % 2 == 0 and length % 2 == 0 and length >= 2, (a, b, r)
            assert pos >= a and pos + length <= b + 1, (a, b, r)              # inside the detected picture
            if avail >= r:
                assert length % r == 0 and avail - length < r, (a, b, r)      # the largest multiple of r
            else:
                assert avail - length <= 1, (a, b, r)                         # the largest even length
            before, behind = pos - a_even, (a_even + avail) - (pos + length)
            assert 0 <= before <= behind <= before + 3, (a, b, r)             # centred to within one even step
    assert k == len(rec)


def test_model_rounding_examples():
    assert M.round_axis(140, 939, 16) == (140, 800)
    assert M.round_axis(0, 1919, 16) == (0, 1920)
    assert M.round_axis(0, 1079, 16) == (4, 1072)
    assert M.round_axis(1, 1, 2) is None and M.round_axis(0, 0, 2) is None and M.round_axis(1, 2, 2) is None
    assert M.round_axis(0, 1, 16) == (0, 2) and M.round_axis(1, 3, 16) == (2, 2)


def test_model_record_rules():
    """Classification (equality is black), contribution and union, on sums written by hand."""
    W, H = 8, 6
    def s(rows, cols):
        return np.array(rows + cols, dtype=np.uint32)
    black = s([0] * H, [0] * W)
    at_limit = s([24 * W] * H, [24 * H] * W)
    assert M.image_bounds(black, W, H, 24) is None and M.image_bounds(at_limit, W, H, 24) is None
    one = s([0, 0, 24 * W + 1, 0, 0, 0], [0, 0, 0, 24 * H + 1, 24 * H, 0, 0, 0])
    assert M.image_bounds(one, W, H, 24) == (3, 2, 3, 2)
    rows_only = s([999] * H, [24 * H] * W)   # picture rows, no picture column: contributes nothing
    assert M.image_bounds(rows_only, W, H, 24) is None
    a = s([0, 900, 900, 900, 0, 0], [0, 0, 900, 900, 900, 0, 0, 0])
    b = s([0, 0, 900, 900, 900, 0], [0, 0, 0, 900, 900, 900, 900, 0])
    assert M.record([a], W, H, 24, 2).tolist() == [2, 2, 2, 2, 2, 1, 4, 3]
    assert M.record([a, black, b, rows_only], W, H, 24, 2).tolist() == [2, 2, 4, 2, 2, 1, 6, 4]
    assert M.record([black, at_limit], W, H, 24, 2).tolist() == [0, 0, W, H, W, H, -1, -1]
    assert M.record([one], W, H, 24, 2).tolist() == [0, 0, W, H, 3, 2, 3, 2]  # an axis fails: the whole picture


def test_cover_crop():
    import espflix_amd as efx
    assert efx.cover_crop(1280, 546) == (140, 0, 1000, 546)
    assert M.cover_crop(1280, 546) == (140, 0, 1000, 546)
    assert efx.cover_crop(352, 192) == (0, 0, 352, 192)
    assert efx.cover_crop(1920, 1080) == (0, 16, 1920, 1046)
    assert efx.cover_crop(1920, 1080, (0, 140, 1920, 800)) == (226, 140, 1466, 800)
    cases = [((1280, 546), None), ((1920, 1080), None), ((352, 192), None), ((1920, 1080), (0, 140, 1920, 800)),
             ((1920, 1080), (240, 0, 1440, 1080)), ((4096, 4096), (2, 4, 4000, 300)), ((333, 77), None), ((30, 4094), None),
             ((640, 480), (16, 32, 600, 400)), ((2000, 1000), (10, 12, 22, 12)), ((704, 384), None), ((100, 100), (6, 8, 11, 6))]
    for (W, H), region in cases:
        x, y, w, h = region or (0, 0, W, H)
        cx, cy, cw, ch = efx.cover_crop(W, H, region)
        assert (cx, cy, cw, ch) == M.cover_crop(W, H, region), (W, H, region)
        assert cw >= 1 and ch >= 1 and cx >= x and cy >= y and cx + cw <= x + w and cy + ch <= y + h   # inside the region
        assert (cw == w) != (ch == h) or (cw, ch) == (w, h)                                           # one side is kept
        # the largest even side of the frame's shape: two more columns (rows) would no longer fit it
        if ch == h and cw != w:
            assert cw % 2 == 0 and cw * 192 <= h * 352 < (cw + 2) * 192
        if cw == w and ch != h:
            assert ch % 2 == 0 and ch * 352 <= w * 192 < (ch + 2) * 352
        # an even step from the region's corner, centred to within one
        assert (cx - x) % 2 == 0 and (cy - y) % 2 == 0
        assert 0 <= (w - cw) - 2 * (cx - x) <= 3 and 0 <= (h - ch) - 2 * (cy - y) <= 3
    for bad in ((0, 0, 0, 10), (0, 0, 10, 0), (-2, 0, 10, 10), (0, 0, 101, 10), (0, 95, 10, 10), (0, 0, 100, 1), (0, 0, 1, 100)):
        with pytest.raises(ValueError):
            efx.cover_crop(100, 100, bad)


def test_binding_declares_the_entry_point():
    import ctypes as C
    import espflix_amd as efx
    assert "efx_detect_crop" in efx._SYMBOLS
    assert C.sizeof(efx._CropOpts) == 8 * 4 + 2 * C.sizeof(C.c_size_t)


def boxed(rng, n, fmt, w, h):
    """Noise pictures with black bars of different widths, so that records are not the whole picture."""
    out = np.zeros((n, src_bytes(fmt, w, h)), dtype=np.uint8)
    for i in range(n):
        x0, y0 = min(w // 5 + i, w - 1), min(h // 7 + 2 * i, h - 1)
        x1, y1 = max(x0 + 1, w - w // 6 - i), max(y0 + 1, h - h // 9)
        if fmt == "i420":
            p = np.full((h, w), 16, dtype=np.uint8)
            p[y0:y1, x0:x1] = rng.integers(60, 256, (y1 - y0, x1 - x0))
            out[i, :w * h] = p.reshape(-1)
            out[i, w * h:] = rng.integers(0, 256, w * h // 2)   # (chroma: never read)
        else:
            p = np.zeros((h, w, 3), dtype=np.uint8)
            p[y0:y1, x0:x1] = rng.integers(60, 256, (y1 - y0, x1 - x0, 3))
            out[i] = (p if fmt == "rgb24" else p.transpose(2, 0, 1)).reshape(-1)
    return out


SANITIZED_CASES = [
    # fmt, width, height, streams, images per stream, full range, pictures
    ("rgbp", 2, 2, 2, 3, False, "noise"),
    ("rgb24", 333, 77, 2, 3, False, "noise"),
    ("rgb24", 333, 77, 2, 3, True, "boxed"),
    ("i420", 354, 194, 2, 3, False, "boxed"),
    ("i420", 354, 194, 1, 5, False, "noise"),
    ("i420", 4096, 2304, 1, 1, False, "noise"),
    ("rgbp", 353, 193, 1, 2, True, "boxed"),
    ("rgb24", 4096, 66, 1, 1, False, "noise"),
]


@pytest.mark.parametrize("fmt,w,h,n_streams,per,full,kind", SANITIZED_CASES)
def test_whole_detection_under_sanitizers(sanitized, tmp_path, fmt, w, h, n_streams, per, full, kind):
    """The kernels' addressing on the host, every image, its sums and the records in heap blocks of exactly the
    contract's sizes: the run is clean under -fsanitize=address,undefined and sums and records are the model's."""
    rng = np.random.default_rng(w * 7 + h)
    n = n_streams * per
    if kind == "noise":
        src = rng.integers(0, 256, (n, src_bytes(fmt, w, h)), dtype=np.uint8)
        limit = int(np.mean([M.luma(s, fmt, w, h, full).mean() for s in src]))
    else:
        src, limit = boxed(rng, n, fmt, w, h), 24
    (tmp_path / "src.bin").write_bytes(src.tobytes())
    run = subprocess.run([sanitized, "detect", str(FMT[fmt]), str(w), str(h), str(int(full)), str(limit), "16", str(n_streams),
                          str(per), str(tmp_path / "src.bin"), str(tmp_path / "sums.bin"), str(tmp_path / "recs.bin")],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    got_sums = np.fromfile(tmp_path / "sums.bin", dtype=np.uint32).reshape(n, h + w)
    got_recs = np.fromfile(tmp_path / "recs.bin", dtype=np.int32).reshape(n_streams, 8)
    want_sums, want_recs = M.detect(src, fmt, w, h, per, limit, 16, full)
    bad = np.argwhere(got_sums != want_sums)
    assert bad.size == 0, f"{len(bad)} sums differ, first (image, index) = {bad[0].tolist()}"
    assert np.array_equal(got_recs, want_recs), (got_recs.tolist(), want_recs.tolist())
    if kind == "boxed":
        assert (got_recs[:, 2] < w).all() and (got_recs[:, 3] < h).all() and (got_recs[:, 6] > got_recs[:, 4]).all()
