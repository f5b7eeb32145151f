"""The arithmetic of the import's HDR stage (espflix_amd/csrc/hdr_px.h, built here with the host compiler) against the
NumPy integer model of include/efx.h's definition and against a float64 yardstick that shares no code with the header
(tests/hdr_model.py): the coefficients against Fractions, the library's tables against a golden file and a float64
recomputation, the item over a lattice of 67 M triples and 1 M random 2 x 2 blocks per setting, the exact properties of
grey, import10 against the 8-bit import, and whole HDR imports with the kernels' index arithmetic
(tests/hdr_model_main.cpp), also under the address and undefined-behaviour sanitizers.  No GPU.

`python tests/test_hdr_model.py --record` rewrites tests/golden/import_hdr_tables_1000.npy and
tests/golden/import_hdr_accuracy.json from the library as built."""
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import colour_model as K
import hdr_model as H
import import_model as M
import surface_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_TABLES = os.path.join(ROOT, "tests", "golden", "import_hdr_tables_1000.npy")
GOLDEN_ACCURACY = os.path.join(ROOT, "tests", "golden", "import_hdr_accuracy.json")
SETTING_IDS = [f"peak{p}-{'full' if f else 'studio'}-prim{c}" for p, f, c in H.SETTINGS]
N_BLOCKS = 1 << 20
SHARE_TOLERANCE = 1e-4   # the yardstick's pow() is the platform's: a rounding may fall the other way for a few inputs in 10^5


def build(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build hdr_px.h"
    exe = tmp / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "espflix_amd", "csrc"), os.path.join(ROOT, "tests", "hdr_model_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("hdr_px"), "drv", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("hdr_px_san"), "drv_san",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def library_tables(peak, full=0, prim=9, matrix=9, height=0):
    import espflix_amd as efx
    return efx.hdr_tables(peak, primaries=prim, matrix=matrix, src_range="full" if full else "studio", height=height)


def setting_of(t, peak, full, prim, matrix=9, height=0):
    """The model's setting fed with the library's own tables; its coefficients are the model's own."""
    return H.Setting(peak, full, prim, matrix, height, pq=t["pq"], gam=t["gamma"])


def tables_file(tmp_path, t):
    path = tmp_path / "tables.bin"
    path.write_bytes(t["raw"].tobytes())
    return str(path)


def header_blocks(driver, tmp_path, t, blocks):
    """(n, 6) uint16 (Y10 x 4, Cb10, Cr10) -> (n, 6) uint8 (Y' x 4, Cb', Cr') through hdr::tonemap_block."""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint16)
    (tmp_path / "in.bin").write_bytes(blocks.tobytes())
    subprocess.run([driver, "blocks", tables_file(tmp_path, t), str(len(blocks)), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                   check=True, capture_output=True, text=True, timeout=600)
    return np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(-1, 6)


def shares(diff):
    """[share that differs by 0, share that differs by 1, the maximum]."""
    d = np.bincount(np.asarray(diff).ravel(), minlength=2)
    return [float(d[0] / d.sum()), float(d[1] / d.sum()), int(np.flatnonzero(d).max())]


# ---- coefficients ----------------------------------------------------------------------------------------------------------------
def header_coefs(driver, prim, matrix, full, peak, height=0):
    r = subprocess.run([driver, "coefs", str(prim), str(matrix), str(full), str(peak), str(height)], capture_output=True, text=True,
                       check=True, timeout=60)
    v = [int(x) for x in r.stdout.split()]
    return v[0], v[1:6], v[6], v[7:16], v[16]


@pytest.mark.parametrize("code", K.CODES)
def test_header_coefficients_are_the_rounded_exact_values(driver, code):
    for full in (0, 1):
        for prim in (9, 1):
            ok, q, y0, g, peak = header_coefs(driver, prim, code, full, 0)
            assert ok == 1 and peak == 1000
            assert (q, y0) == H.matrix_coefs(code, full)
            assert g == H.gamut_coefs(prim)
            assert y0 == (0 if full else 64)
    assert header_coefs(driver, 9, 2, 0, 400, 578)[1] == H.matrix_coefs(1, 0)[0]   # unspecified: by height, as the colour stage
    assert header_coefs(driver, 9, 2, 0, 400, 576)[1] == H.matrix_coefs(6, 0)[0]


def test_gamut_matrix():
    want = [(1.6605, -0.5876, -0.0728), (-0.1246, 1.1329, -0.0083), (-0.0182, -0.1006, 1.1187)]   # BT.2087, as the issue gives it
    exact = H.gamut_exact(9)
    for row, w in zip(exact, want):
        assert [round(float(v), 4) for v in row] == list(w)
    for prim in (9, 1):
        g = H.gamut_coefs(prim)
        assert [sum(g[3 * i:3 * i + 3]) for i in range(3)] == [H.GAMUT_ONE] * 3    # every row sums to exactly one
    assert H.gamut_coefs(1) == [H.GAMUT_ONE, 0, 0, 0, H.GAMUT_ONE, 0, 0, 0, H.GAMUT_ONE]
    flat = [v for row in exact for v in row]
    assert max(abs(q - v * H.GAMUT_ONE) for q, v in zip(H.gamut_coefs(9), flat)) <= 1.5   # rounded, the diagonal at most one further


def test_header_rejects_other_settings(driver):
    for prim, matrix, full, peak in ((5, 9, 0, 1000), (0, 9, 0, 1000), (9, 0, 0, 1000), (9, 8, 0, 1000), (9, 10, 0, 1000), (9, 9, 2, 1000),
                                     (9, 9, -1, 1000), (9, 9, 0, 199), (9, 9, 0, 10001), (9, 9, 0, -1)):
        assert header_coefs(driver, prim, matrix, full, peak)[0] == 0, (prim, matrix, full, peak)
    for peak in (0, 200, 10000):
        assert header_coefs(driver, 9, 9, 0, peak)[0] == 1


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def golden_tables_array(t):
    return np.concatenate([t["pq"].astype(np.uint32), t["gamma"].astype(np.uint32)])


def test_tables_equal_the_golden_file():
    """Pins the platform's pow(), as import_pcm_table.npy pins sin()."""
    t = library_tables(1000)
    assert len(t["pq"]) == H.PQ_ENTRIES and len(t["gamma"]) == H.GAM_ENTRIES
    assert np.array_equal(golden_tables_array(t), np.load(GOLDEN_TABLES))
    assert np.array_equal(library_tables(0)["raw"], t["raw"])    # peak 0 means 1000


@pytest.mark.parametrize("peak", H.PEAKS + (200, 10000))
def test_tables_against_float64(peak):
    t = library_tables(peak)
    pq, gam = H.tables(peak)
    assert np.abs(t["pq"].astype(np.int64) - pq).max() <= 1
    assert np.abs(t["gamma"].astype(np.int64) - gam).max() <= 1
    assert t["pq"][0] == 0 and t["pq"][-1] == H.LIN_ONE and t["gamma"][0] == 0 and t["gamma"][-1] == H.E_ONE
    assert (np.diff(t["pq"].astype(np.int64)) >= 0).all() and (np.diff(t["gamma"].astype(np.int64)) >= 0).all()
    # every entry at or above the peak's code is 1
    first = int(np.ceil(float(H.pq_inverse(peak)) * (H.PQ_ENTRIES - 1)))
    assert (t["pq"][first:] == H.LIN_ONE).all()
    assert t["matrix"] == H.matrix_coefs(9, 0)[0] and t["gamut"] == H.gamut_coefs(9) and t["y0"] == 64 and t["peak_nits"] == peak


# ---- the item: the lattice and random blocks --------------------------------------------------------------------------------------
def measure_lattice(driver, tmp_path, peak, full, prim):
    """Every Y10 x every fourth Cb10 x every fourth Cr10: (bytes that differ between the header and the integer model,
    shares(|integer Y' - yardstick Y'|))."""
    t = library_tables(peak, full, prim)
    out = tmp_path / "lattice.bin"
    subprocess.run([driver, "lattice", tables_file(tmp_path, t), str(out)], check=True, capture_output=True, text=True, timeout=1200)
    got = np.memmap(out, dtype=np.uint8, mode="r").reshape(3, 1021, 256, 256)
    s = setting_of(t, peak, full, prim)
    c = np.arange(256) * 4
    cb, cr = np.meshgrid(c, c, indexing="ij")
    def chunk(y0):
        ys = np.arange(y0, min(1021, y0 + 8))
        Y = np.broadcast_to(ys[:, None, None], (len(ys), 256, 256))
        CB, CR = np.broadcast_to(cb, Y.shape), np.broadcast_to(cr, Y.shape)
        rgb = H.sdr_rgb(s, Y, CB, CR)
        yy = H.luma(rgb)
        b, r = H.chroma([4 * x for x in rgb])
        differs = int((yy != got[0, ys]).sum() + (b != got[1, ys]).sum() + (r != got[2, ys]).sum())
        want = H.yard_luma(H.yard_rgb(peak, full, prim, 9, Y, CB, CR))
        return differs, np.bincount(np.minimum(np.abs(yy - want), 7).ravel(), minlength=8)

    # (NumPy works outside the interpreter's lock: a few threads take the 128 chunks side by side)
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        parts = list(pool.map(chunk, range(0, 1021, 8)))
    differing, hist = sum(p[0] for p in parts), sum(p[1] for p in parts)
    del got
    os.remove(out)
    return differing, [float(hist[0] / hist.sum()), float(hist[1] / hist.sum()), int(np.flatnonzero(hist).max())]


def random_blocks(seed):
    """Half of the blocks uniform over all codes (mostly outside every gamut: the clamps), half pictures' kind: four
    neighbouring luma samples around a site of moderate chroma."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1021, (N_BLOCKS, 6))
    h = N_BLOCKS // 2
    base = rng.integers(64, 941, (h, 1))
    b[h:, :4] = np.clip(base + rng.integers(-40, 41, (h, 4)), 0, 1020)
    b[h:, 4:] = rng.integers(512 - 160, 512 + 161, (h, 2))
    return b


def measure_blocks(driver, tmp_path, peak, full, prim):
    """1 M random 2 x 2 blocks: (bytes that differ between the header and the integer model, shares per Y', Cb', Cr'
    against the yardstick)."""
    t = library_tables(peak, full, prim)
    blocks = random_blocks(peak + 2 * full + prim)
    got = header_blocks(driver, tmp_path, t, blocks).astype(np.int64)
    s = setting_of(t, peak, full, prim)
    yy, cb, cr = H.item(s, blocks[:, :4], blocks[:, 4], blocks[:, 5])
    differing = int((yy != got[:, :4]).sum() + (cb != got[:, 4]).sum() + (cr != got[:, 5]).sum())
    yard = H.yard_rgb(peak, full, prim, 9, blocks[:, :4], blocks[:, 4:5], blocks[:, 5:6])
    wy = H.yard_luma(yard)
    wb, wr = H.yard_chroma([c.mean(axis=-1) for c in yard])
    return differing, {"y": shares(np.abs(yy - wy)), "cb": shares(np.abs(cb - wb)), "cr": shares(np.abs(cr - wr))}


def assert_recorded(got, recorded, what):
    assert got[2] <= 1, f"{what}: the integer result is {got[2]} from the rounded yardstick"
    assert got[2] == recorded[2], (what, got, recorded)
    assert abs(got[0] - recorded[0]) <= SHARE_TOLERANCE and abs(got[1] - recorded[1]) <= SHARE_TOLERANCE, (what, got, recorded)


@pytest.mark.parametrize("peak,full,prim", H.SETTINGS, ids=SETTING_IDS)
def test_lattice_model_match_and_yardstick(driver, tmp_path, peak, full, prim):
    """Model match: hdr_px.h equals the NumPy integer model bit for bit on every Y10 x every fourth Cb10 x every fourth
    Cr10 (Y', and the Cb', Cr' of a block of four such pixels).  Float64 yardstick: on the same lattice the integer Y' is
    never more than 1 from the rounded yardstick; the shares are the recorded ones."""
    differing, y = measure_lattice(driver, tmp_path, peak, full, prim)
    print(f"peak {peak} range {full} primaries {prim}: {differing} bytes differ from the model; Y' against the yardstick: "
          f"{y[0]:.6f} equal, {y[1]:.6f} one off, maximum {y[2]}")
    assert differing == 0
    with open(GOLDEN_ACCURACY) as f:
        recorded = json.load(f)["lattice"][f"{peak}/{full}/{prim}"]
    assert_recorded(y, recorded["y"], "lattice Y'")


@pytest.mark.parametrize("peak,full,prim", H.SETTINGS, ids=SETTING_IDS)
def test_random_blocks_model_match_and_yardstick(driver, tmp_path, peak, full, prim):
    """1 M random 2 x 2 blocks: the header equals the model bit for bit, and Y', Cb' and Cr' -- chroma from the mean of
    the four pixels' R', G', B' -- are never more than 1 from the rounded yardstick."""
    differing, got = measure_blocks(driver, tmp_path, peak, full, prim)
    print(f"peak {peak} range {full} primaries {prim}: {differing} bytes differ from the model; against the yardstick: {got}")
    assert differing == 0
    with open(GOLDEN_ACCURACY) as f:
        recorded = json.load(f)["blocks"][f"{peak}/{full}/{prim}"]
    for plane in ("y", "cb", "cr"):
        assert_recorded(got[plane], recorded[plane], f"blocks {plane}")


# ---- exact properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", [9, 1, 6])
@pytest.mark.parametrize("peak,full,prim", H.SETTINGS + [(200, 0, 9), (10000, 1, 9)], ids=SETTING_IDS + ["peak200", "peak10000"])
def test_grey(driver, tmp_path, peak, full, prim, matrix):
    """Cb10 = Cr10 = 512: Cb' = Cr' = 128 for every Y10, Y' never falls, studio black gives 16, every Y10 at or above the
    code of peak_nits gives 235."""
    t = library_tables(peak, full, prim, matrix)
    y = np.arange(1021)
    blocks = np.stack([y, y, y, y, np.full(1021, 512), np.full(1021, 512)], axis=1)
    got = header_blocks(driver, tmp_path, t, blocks).astype(int)
    assert (got[:, 4:] == 128).all()
    assert (got[:, :4] == got[:, :1]).all()
    assert (np.diff(got[:, 0]) >= 0).all()
    assert got[0 if full else 64, 0] == 16 and (got[:1 if full else 65, 0] == 16).all()
    code = H.peak_code(peak, full)
    assert code <= 1020 and (got[code:, 0] == 235).all() and got[:, 0].max() == 235
    # and four different greys in one block are still grey
    mixed = np.stack([y, y[::-1], (y + 300) % 1021, (y * 7) % 1021, np.full(1021, 512), np.full(1021, 512)], axis=1)
    assert (header_blocks(driver, tmp_path, t, mixed)[:, 4:] == 128).all()


# ---- import10 and whole imports ----------------------------------------------------------------------------------------------------
# kind, width, height, pitch, plane rows, images, crop, destination rectangle
IMPORT_CASES = [
    ("i420", 64, 48, 80, 50, 2, None, None),                       # pitched planar bytes
    ("nv12", 64, 48, 0, 0, 2, None, (6, 10, 100, 52)),             # the rectangle starts and ends inside bands
    ("i010", 64, 48, 0, 0, 2, (2, 6, 28, 10), (6, 10, 100, 52)),   # planar words, shift 2
    ("p010", 34, 18, 74, 20, 3, (2, 6, 28, 10), None),             # pair words, shift 8
    ("nv21", 2, 2, 0, 0, 1, None, None),
    ("p010", 704, 384, 0, 0, 1, None, None),                       # both columns of a lane
]
IMPORT_IDS = [f"{c[0]}-{c[1]}x{c[2]}" + ("-rect" if c[7] else "") for c in IMPORT_CASES]


def run_import(exe, tmp_path, t, s, src, n, crop, rect):
    stride = (s.bytes + 15) // 16 * 16 + 32
    (tmp_path / "src.bin").write_bytes(np.ascontiguousarray(src).tobytes())
    crop = crop or (0, 0, s.width, s.height)
    rect = rect or (0, 0, M.W, M.H)
    run = subprocess.run([exe, "import", tables_file(tmp_path, t), *map(str, s.args()), str(n), str(stride), *map(str, crop), *map(str, rect),
                          str(tmp_path / "src.bin"), str(tmp_path / "dst.bin"), str(tmp_path / "dst10.bin")],
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    return (np.fromfile(tmp_path / "dst.bin", dtype=np.uint8).reshape(n, M.FRAME_BYTES),
            np.fromfile(tmp_path / "dst10.bin", dtype=np.uint16).reshape(n, M.FRAME_BYTES))


# (the plain build alone takes the large picture: the sanitizer build sees the same addressing on the small ones)
IMPORT_RUNS = [(which, *c) for which in ("plain", "sanitized") for c in IMPORT_CASES if which == "plain" or c[1] <= 64]
IMPORT_RUN_IDS = [f"{which}-{i}" for which in ("plain", "sanitized") for c, i in zip(IMPORT_CASES, IMPORT_IDS) if which == "plain" or c[1] <= 64]


@pytest.mark.parametrize("which,kind,w,h,pitch,rows,n,crop,rect", IMPORT_RUNS, ids=IMPORT_RUN_IDS)
def test_whole_imports(request, tmp_path, which, kind, w, h, pitch, rows, n, crop, rect):
    """The kernels' band walk, 10-bit band and HDR stage on the host for all four layouts, the source in a heap block of
    exactly the memory contract's size: the bytes are tonemap(import10(canonical image)) of the model, import10 is within
    2 of four times the 8-bit import (the two roundings are independent), and the sanitizer build runs clean."""
    exe = request.getfixturevalue("driver" if which == "plain" else "sanitized")
    s = S.layout(kind, w, h, pitch, rows)
    src = S.sources(n, s, 91 + w)
    t = library_tables(1000)
    got, got10 = run_import(exe, tmp_path, t, s, src, n, crop, rect)
    canon = S.canonicals(src, s)
    want = H.import_images(setting_of(t, 1000, 0, 9), canon, w, h, crop, rect)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first (image, byte) = {bad[0].tolist()}"
    # import10 against the model's, and against the 8-bit import
    x, y, rw, rh = rect or (0, 0, M.W, M.H)
    v8 = M.import_images(canon, "i420", w, h, crop, rect).astype(int)
    for i in range(n):
        y10, cb10, cr10 = H.import10(canon[i], w, h, crop, rect)
        planes = ((0, M.W, 1, y10), (M.Y_BYTES, M.CW, 2, cb10), (M.Y_BYTES + M.C_BYTES, M.CW, 2, cr10))
        for off, pw, sub, want10 in planes:
            sl = (slice(y // sub, (y + rh) // sub), slice(x // sub, (x + rw) // sub))
            g10 = got10[i, off:off + pw * (M.H // sub)].reshape(M.H // sub, pw)[sl].astype(int)
            assert np.array_equal(g10, want10)
            assert g10.max() <= 1020
            g8 = v8[i, off:off + pw * (M.H // sub)].reshape(M.H // sub, pw)[sl]
            assert np.abs(4 * g8 - g10).max() <= 2
    if rect:
        outside = np.ones((M.H, M.W), dtype=bool)
        outside[y:y + rh, x:x + rw] = False
        assert (got[:, :M.Y_BYTES].reshape(n, M.H, M.W)[:, outside] == 16).all()
        assert not (got[:, M.Y_BYTES:].reshape(n, 2, M.CH, M.CW)[:, :, outside[::2, ::2]] != 128).any()


def test_python_helpers():
    import espflix_amd as efx
    t = efx.hdr_tables()
    assert t["peak_nits"] == 1000 and t["y0"] == 64 and len(t["raw"]) == 64 + 4 * (len(t["pq"]) + 3) + 2 * 1224
    assert efx.hdr_tables(400, "bt709", "bt709", "full")["gamut"] == H.gamut_coefs(1)
    assert efx.hdr_tables(400, 1, 1, "full")["matrix"] == H.matrix_coefs(1, 1)[0]
    assert efx.hdr_tables(400, matrix="auto", height=1080)["matrix"] == H.matrix_coefs(1, 0)[0]
    for kw in (dict(peak_nits=199), dict(peak_nits=10001), dict(primaries=5), dict(primaries="dci"), dict(matrix=8), dict(matrix="bt470"),
               dict(src_range="limited"), dict(transfer=18), dict(transfer="hlg")):
        with pytest.raises(ValueError):
            efx.hdr_tables(**kw)
    lib = efx.load_library()
    import ctypes as C
    assert lib.efx_import_hdr_tables(None, 0, None, 0) == -1
    h = efx._ImportHdr(16, 9, 9, 0, 1000)
    size = lib.efx_import_hdr_tables(C.byref(h), 0, None, 0)
    small = np.full(size, 0xAB, dtype=np.uint8)
    assert lib.efx_import_hdr_tables(C.byref(h), 0, small.ctypes.data, size - 1) == size and (small == 0xAB).all()   # too small: untouched


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_hdr_model.py --record")
    import pathlib
    import tempfile

    sys.path.insert(0, ROOT)
    np.save(GOLDEN_TABLES, golden_tables_array(library_tables(1000)))
    with tempfile.TemporaryDirectory() as d:
        tmp = pathlib.Path(d)
        drv = build(tmp, "drv", ["-O2"])
        record = {"what": "share of results equal to the rounded float64 yardstick, share one off, the maximum difference; "
                          "key: peak_nits / full_range / primaries",
                  "lattice": {}, "blocks": {}}
        for peak, full, prim in H.SETTINGS:
            differing, y = measure_lattice(drv, tmp, peak, full, prim)
            differing_b, b = measure_blocks(drv, tmp, peak, full, prim)
            print(peak, full, prim, differing, y, differing_b, b, flush=True)
            record["lattice"][f"{peak}/{full}/{prim}"] = {"y": y}
            record["blocks"][f"{peak}/{full}/{prim}"] = b
        with open(GOLDEN_ACCURACY, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
