"""The per-pixel arithmetic of k_export (espflix_amd/csrc/export_px.h, built here with the host compiler) against the
NumPy model of include/efx.h's formulas (tests/export_model.py), and the model against fixed anchors.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import common
import export_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUDIO_ANCHORS = [((235, 128, 128), (255, 255, 255)), ((16, 128, 128), (0, 0, 0)), ((126, 128, 128), (128, 128, 128)),
                  ((81, 90, 240), (255, 0, 0)), ((145, 54, 34), (0, 255, 1)), ((41, 240, 110), (0, 0, 255))]
FULL_ANCHORS = [((255, 128, 128), (255, 255, 255)), ((76, 85, 255), (254, 0, 0)), ((29, 255, 107), (0, 0, 254))]

# Host driver of export_px.h: mode 0 = px::rgb over every (Y, U, V) triple (Y major, V minor) of one range, packed
# 0x00BBGGRR; mode 1 = px::bilinear over 4-byte neighbourhoods read from stdin; mode 2 = px::near_tap for x in 0 .. n-1.
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "export_px.h"
using namespace efx;
int main(int argc, char** argv)
{
    const int mode = atoi(argv[1]), arg = atoi(argv[2]);
    if (mode == 0) {
        const px::Matrix m = px::matrix(arg);
        std::vector<uint32_t> out(1 << 16);
        for (int y = 0; y < 256; y++) {
            for (int u = 0; u < 256; u++)
                for (int v = 0; v < 256; v++)
                    out[u * 256 + v] = px::rgb(m, y, u, v);
            fwrite(out.data(), 4, out.size(), stdout);
        }
    } else if (mode == 1) {
        unsigned char c[4];
        while (fread(c, 1, 4, stdin) == 4) {
            const int r = px::bilinear(c[0], c[1], c[2], c[3]);
            fwrite(&r, 4, 1, stdout);
        }
    } else {
        for (int x = 0; x < arg; x++) {
            const int t = px::near_tap(x, arg / 2 - 1);
            fwrite(&t, 4, 1, stdout);
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build export_px.h"
    d = tmp_path_factory.mktemp("export_px")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "espflix_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


def run(driver, mode, arg, data=None):
    r = subprocess.run([driver, str(mode), str(arg)], input=data, capture_output=True, check=True, timeout=300)
    return np.frombuffer(r.stdout, dtype=np.int32 if mode else np.uint32)


@pytest.mark.parametrize("full_range,anchors", [(False, STUDIO_ANCHORS), (True, FULL_ANCHORS)])
def test_model_anchors(full_range, anchors):
    yuv = np.array([a for a, _ in anchors])
    got = M.ycbcr_to_rgb(yuv[:, 0], yuv[:, 1], yuv[:, 2], full_range)
    assert got.tolist() == [list(b) for _, b in anchors]


def test_strip_i420_round_trip():
    frames = common.random_frames(3).reshape(2, M.FRAME_BYTES)
    i420 = M.strip_to_i420(frames)
    assert i420.shape == frames.shape
    assert np.array_equal(M.i420_to_strip(i420), frames)
    # plane mapping: strip rows 0-7 of strip k are Cb (U) rows 8k ... 8k + 7
    y, u, v = M.planes(frames[0])
    s = frames[0].reshape(12, 16, 528)
    assert np.array_equal(u[8 * 5 + 3], s[5, 3, 352:]) and np.array_equal(v[8 * 5 + 3], s[5, 11, 352:])
    assert np.array_equal(y[16 * 7 + 9], s[7, 9, :352])


@pytest.mark.parametrize("full_range", [False, True])
def test_header_matrix_matches_model_everywhere(driver, full_range):
    got = run(driver, 0, int(full_range)).reshape(256, 256, 256)
    y, u, v = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    want = M.ycbcr_to_rgb(y, u, v, full_range).astype(np.uint32)
    want = want[..., 0] | (want[..., 1] << 8) | (want[..., 2] << 16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} triples differ, first (Y, U, V) = {bad[0].tolist()}"
    # the anchors through the header itself
    for (yy, uu, vv), rgb in (FULL_ANCHORS if full_range else STUDIO_ANCHORS):
        w = int(got[yy, uu, vv])
        assert (w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF) == rgb


def test_header_bilinear_taps_match_model(driver):
    rng = np.random.default_rng(1)
    c = rng.integers(0, 256, size=(200000, 4), dtype=np.uint8)
    c[:4] = [[0, 0, 0, 0], [255, 255, 255, 255], [255, 0, 0, 0], [0, 255, 255, 255]]
    got = run(driver, 1, 0, c.tobytes())
    assert np.array_equal(got, M.bilinear4(c[:, 0], c[:, 1], c[:, 2], c[:, 3]))


@pytest.mark.parametrize("n", [M.W, M.H])
def test_header_neighbour_tap_matches_model(driver, n):
    _, c1 = M.near_index(n)
    assert np.array_equal(run(driver, 2, n), c1)


def test_model_upsampling_is_the_formula():
    """The vectorised model against the formula of efx.h evaluated pixel by pixel at the edges and inside."""
    rng = np.random.default_rng(2)
    c = rng.integers(0, 256, size=(M.CH, M.CW)).astype(np.int32)
    up = M.upsample(c, "bilinear")
    near = M.upsample(c, "nearest")
    for y in (0, 1, 2, 95, 96, 190, 191):
        for x in (0, 1, 2, 3, 174, 175, 350, 351):
            cx0, cy0 = x >> 1, y >> 1
            cx1 = min(max(cx0 + (1 if x & 1 else -1), 0), 175)
            cy1 = min(max(cy0 + (1 if y & 1 else -1), 0), 95)
            want = (9 * c[cy0, cx0] + 3 * c[cy0, cx1] + 3 * c[cy1, cx0] + c[cy1, cx1] + 8) >> 4
            assert up[y, x] == want and near[y, x] == c[cy0, cx0]
