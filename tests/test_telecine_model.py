"""The rule of efx_detelecine: whole calls on the host through espflix_amd/csrc/telecine_px.h with the kernels' own walk
(tests/telecine_model_main.cpp, built here with the host compiler under the address and undefined-behaviour sanitizers)
against the NumPy model of include/efx.h's definition (tests/telecine_model.py), the corner cases of the decision, and
what the rule is for: synthetic 2-3 pulldown comes back as the film.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surface_model as S
import telecine_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 8), (18, 8), (34, 12), (70, 20)]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build telecine_px.h"
    exe = tmp_path_factory.mktemp("telecine_px_san") / "drv_san"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "telecine_model_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


def host_call(exe, srcs, s, n_streams=1, first_field=M.TOP, lead=0, nt=10):
    """One call of the host program: (outputs (n_streams, n_out, w h 3 / 2), records (n_streams, n)), or the exit status of
    a refused call."""
    n_frames = len(srcs) // n_streams
    r = subprocess.run([exe, "call", *[str(v) for v in s.args()], str(n_streams), str(n_frames), str(first_field), str(lead), str(nt)],
                       input=np.ascontiguousarray(srcs).tobytes(), capture_output=True, timeout=300)
    if r.returncode:
        return r.returncode
    image, n = s.width * s.height * 3 // 2, n_frames - lead
    n_out = M.count(n_frames, lead)
    assert len(r.stdout) == n_streams * (n_out * image + n * 32)
    outs = np.frombuffer(r.stdout[:n_streams * n_out * image], dtype=np.uint8).reshape(n_streams, n_out, image)
    return outs, np.frombuffer(r.stdout[n_streams * n_out * image:], dtype=M.INFO).reshape(n_streams, n)


def same(got, want):
    return not isinstance(got, int) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def surfaces(w, h):
    """The layouts a size runs in: packed I420, pitched YV12 (swapped offsets), NV12 with a pitch, NV21."""
    return [("i420", S.layout("i420", w, h)), ("yv12 pitched", S.layout("yv12", w, h, (w + 9) // 2 * 2, h + 2)),
            ("nv12", S.layout("nv12", w, h, w + 5)), ("nv21", S.layout("nv21", w, h))]


def pulled(n, s, seed):
    """n <= 13 source images in which matches of both kinds occur: the luma is a vertical ramp (which has no comb) that
    starts again every 32 rows and rises by 8 from image to image, with a little noise, and in every third image the odd
    rows are lifted by 40 -- such an image is combed as it stands, and top field first its earlier field pairs better with
    the previous image's later field.  Chroma and padding are noise."""
    srcs = S.sources(n, s, seed)
    rng = np.random.default_rng(seed + 1)
    for i in range(n):
        for r in range(s.height):
            at = s.offset[0] + r * s.pitch[0]
            srcs[i, at:at + s.width] = 40 + 2 * (r % 32) + 8 * i + (40 if i % 3 == 1 and r & 1 else 0) + rng.integers(0, 3, s.width)
    return srcs


@pytest.mark.parametrize("w,h", SIZES)
def test_header_matches_model(sanitized, w, h):
    """Both parities of every layout, 11 frames (two whole cycles and a partial one): the header's walk writes what the
    definition says, byte for byte, records included, and the sanitizers see no access outside the blocks."""
    for k, (name, s) in enumerate(surfaces(w, h)):
        assert s is not None and M.accepts(s), name
        for srcs in (S.sources(11, s, 100 * w + k), pulled(11, s, 200 * w + k)):
            for first_field in (M.TOP, M.BOTTOM):
                got = host_call(sanitized, srcs, s, 1, first_field)
                assert same(got, M.detelecine(srcs, s, 1, first_field)), (name, first_field)
                assert got[0].shape[1] == 9 and sorted(got[1]["out"][0].tolist()) == [-1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8]


def test_both_matches_occur():
    """The sources of the test above exercise match p as well as match c (else half of the rule would go unchecked)."""
    s = S.layout("i420", 34, 12)
    seen = set()
    for srcs in (S.sources(11, s, 3400), pulled(11, s, 6800)):
        seen |= set(M.detelecine(srcs, s, 1)[1]["match"][0].tolist())
    assert seen == {0, 1}


def test_streams_pieces_and_short_calls(sanitized):
    """Two streams do not see each other; pieces of 5 + 5 + 3 processed frames with lead equal the whole, records included
    once `out` is counted on; 1-frame and 4-frame calls drop nothing."""
    s = S.layout("nv12", 34, 12, 40)
    srcs = S.sources(12, s, 7)
    two = host_call(sanitized, srcs, s, 2, M.BOTTOM)
    assert same(two, M.detelecine(srcs, s, 2, M.BOTTOM))
    alone = M.detelecine(srcs[6:], s, 1, M.BOTTOM)
    assert np.array_equal(two[0][1], alone[0][0]) and np.array_equal(two[1][1], alone[1][0])
    assert two[1][1]["diff"][0] == M.NO_DIFF and two[1][1]["comb_p"][0] == 0 and two[1][1]["match"][0] == 0
    title = S.sources(13, s, 8)
    whole = host_call(sanitized, title, s, 1, M.TOP)
    parts = [host_call(sanitized, title[0:5], s, 1, M.TOP), host_call(sanitized, title[4:10], s, 1, M.TOP, 1),
             host_call(sanitized, title[9:13], s, 1, M.TOP, 1)]
    assert [p[0].shape[1] for p in parts] == [4, 4, 3]
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), whole[0])
    recs, base = [], 0
    for outs, info in parts:
        info = info.copy()
        info["out"][info["out"] >= 0] += base
        base += outs.shape[1]
        recs.append(info)
    assert np.array_equal(np.concatenate(recs, axis=1), whole[1])
    for n in (1, 4):
        got = host_call(sanitized, title[:n], s, 1, M.TOP)
        assert same(got, M.detelecine(title[:n], s, 1, M.TOP)) and got[0].shape[1] == n and got[1]["out"][0].tolist() == list(range(n))
    led = host_call(sanitized, title[:2], s, 1, M.TOP, 1)
    assert same(led, M.detelecine(title[:2], s, 1, M.TOP, 1)) and led[0].shape[1] == 1 and led[1]["diff"][0, 0] != M.NO_DIFF


def test_noise_threshold_extremes(sanitized):
    s = S.layout("i420", 34, 12)
    srcs = S.sources(6, s, 9)
    for nt in (0, 255):
        got = host_call(sanitized, srcs, s, 1, M.TOP, 0, nt)
        assert same(got, M.detelecine(srcs, s, 1, M.TOP, 0, nt))
    assert np.all(got[1]["comb_c"] == 0) and np.all(got[1]["comb_p"] == 0) and np.all(got[1]["match"] == 0)   # nt = 255: v - 1530 <= 0
    assert host_call(sanitized, srcs, s, 1, M.TOP, 0, 256) == 1 and host_call(sanitized, srcs, s, 1, M.TOP, 0, -1) == 1


def flat(w, h, value, rows=None):
    """A packed I420 picture of one value, its luma rows `rows` = {row: value} set."""
    y = np.full((h, w), value, dtype=np.uint8)
    for r, v in (rows or {}).items():
        y[r] = v
    return np.concatenate([y.reshape(-1), np.full(w * h // 2, 128, dtype=np.uint8)])


def test_tie_in_d_drops_the_lowest_t(sanitized):
    """Five frames of which frames 1, 2 and 4 repeat their predecessor's earlier field (D = 0): frame 1 goes."""
    w, h = 18, 8
    s = S.layout("i420", w, h)
    values = [10, 10, 10, 60, 60, 90, 90]
    frames = np.stack([flat(w, h, v) for v in values])
    got = host_call(sanitized, frames, s, 1, M.TOP, 0, 10)
    assert same(got, M.detelecine(frames, s, 1, M.TOP, 0, 10))
    assert got[1]["diff"][0].tolist()[1:5] == [0, 0, 50 * w * h // 2, 0] and got[1]["out"][0].tolist() == [0, -1, 1, 2, 3, 4, 5]
    led = host_call(sanitized, frames, s, 1, M.TOP, 1, 10)   # processed: frames 1 .. 6, D = 0, 0, x, 0, x, 0
    assert same(led, M.detelecine(frames, s, 1, M.TOP, 1, 10)) and led[1]["out"][0].tolist() == [-1, 0, 1, 2, 3, 4]


def test_threshold_boundary(sanitized):
    """Flat frames with one comb row: 4 cp = 3 cc gives c, one count less in cp gives p.  With nt = 0 a row of value
    f + a at luma row r (4 <= r <= h - 5) of a flat plane adds (4 + 3 + 3 + 1 + 1) a per column.  Top field first, r = 5 (a
    later-field row): cc comes from F[t]'s row 5 (a = 4), cp from F[t - 1]'s (a = 3, then a = 3 with one column at 2)."""
    w, h = 4, 12
    s = S.layout("i420", w, h)
    cur = flat(w, h, 100, {5: 104})
    prev = flat(w, h, 100, {5: 103})
    got = host_call(sanitized, np.stack([prev, cur]), s, 1, M.TOP, 1, 0)
    assert same(got, M.detelecine(np.stack([prev, cur]), s, 1, M.TOP, 1, 0))
    rec = got[1][0, 0]
    assert rec["comb_c"] == 12 * 4 * w and rec["comb_p"] == 12 * 3 * w and 4 * int(rec["comb_p"]) == 3 * int(rec["comb_c"]) and rec["match"] == 0
    assert np.array_equal(got[0][0, 0], cur)
    y = prev[:w * h].reshape(h, w).copy()
    y[5, 0] = 102   # the smallest step a sample can make: 12 less in cp
    less = np.concatenate([y.reshape(-1), prev[w * h:]])
    got = host_call(sanitized, np.stack([less, cur]), s, 1, M.TOP, 1, 0)
    assert same(got, M.detelecine(np.stack([less, cur]), s, 1, M.TOP, 1, 0))
    rec = got[1][0, 0]
    assert rec["comb_p"] == 12 * 3 * w - 12 and rec["match"] == 1
    assert np.array_equal(got[0][0, 0], M.weave(cur, less, w, h, 0))


def test_refusals_and_count(sanitized):
    ok = S.layout("i420", 18, 8)
    srcs = S.sources(2, ok, 3)
    assert host_call(sanitized, srcs, S.layout("i420", 18, 10), 1) == 1   # height not a multiple of 4
    assert host_call(sanitized, srcs, S.layout("i420", 18, 4), 1) == 1    # below 8
    assert host_call(sanitized, srcs, S.layout("p010", 18, 8), 1) == 1    # a 16-bit layout
    assert host_call(sanitized, srcs, ok, 1, 2) == 1 and host_call(sanitized, srcs, ok, 1, 0, 2) == 1
    assert host_call(sanitized, srcs[:1], ok, 1, 0, 1) == 1               # lead >= n_frames
    for n, lead in [(1, 0), (2, 1), (5, 0), (6, 1), (11, 0), (12, 1), (0, 0), (1, 1), (3, 2), (3, -1), ((1 << 31) - 1, 0), ((1 << 31) - 1, 1)]:
        r = subprocess.run([sanitized, "count", str(n), str(lead)], capture_output=True, text=True, check=True)
        assert int(r.stdout) == M.count(n, lead), (n, lead)
    assert M.count(11, 0) == 9 and M.count(6, 1) == 4 and M.count(1, 1) == -1 and M.count(4, 0) == 4


def test_library_entry_point_is_the_header():
    """efx_detelecine_count of the built library (host only) against the model."""
    import espflix_amd as efx
    for n, lead in [(1, 0), (5, 0), (6, 1), (2, 2), (1, 1), (0, 0), ((1 << 31) - 1, 1), (30, 0)]:
        assert efx.load_library().efx_detelecine_count(n, lead) == M.count(n, lead)
    assert efx.detelecine_count(30) == 24 and efx.detelecine_count(31, lead=True) == 24


def test_a_sum_beyond_32_bits_stays_exact(sanitized):
    """4096 x 4096 alternating 0 / 255 lines: v = 1530 on each of the 4092 rows that have one."""
    r = subprocess.run([sanitized, "stripes", "4096", "4096", "0"], capture_output=True, text=True, check=True, timeout=300)
    assert int(r.stdout) == 1530 * 4092 * 4096 and int(r.stdout) > 1 << 32
    r = subprocess.run([sanitized, "stripes", "4096", "4096", "10"], capture_output=True, text=True, check=True, timeout=300)
    assert int(r.stdout) == (1530 - 60) * 4092 * 4096


# ---- what the rule is for: pulldown comes back as the film ----------------------------------------------------------------------
W, H = 34, 12


def film_frames(n, seed):
    """A smooth texture that moves 3 samples to the right and 1 line down per film frame: packed I420, values 40 .. 215."""
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 6.28, 3)
    frames = []
    for k in range(n):
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        x, y = x - 3 * k, y - k
        v = 128 + 50 * np.sin(2 * np.pi * x / 11 + ph[0]) + 25 * np.cos(2 * np.pi * (x + 2 * y) / 23 + ph[1]) + 12 * np.sin(2 * np.pi * y / 9 + ph[2])
        c = 128 + 40 * np.sin(2 * np.pi * (x[::2, ::2] + y[::2, ::2]) / 17 + ph[0])
        frames.append(np.concatenate([np.rint(v).reshape(-1), np.rint(c).reshape(-1), np.rint(255 - c).reshape(-1)]).astype(np.uint8))
    return np.stack(frames)


def recovered(film, video, early, outs, info, noise):
    """From the second cycle on, the outputs of the whole cycles are the film frames in order, each once.  (A last partial
    cycle drops nothing, so it may show a film frame twice.)"""
    kept = [j for j in range(len(video)) if info["out"][j] >= 0]
    assert [int(info["out"][j]) for j in kept] == list(range(len(outs)))
    last = 4 * (len(video) // 5)
    ks = [early[j] for j in kept[4:last]]
    assert len(ks) >= 4 and ks == list(range(ks[0], ks[0] + len(ks))), ks
    for m, k in zip(range(4, last), ks):
        err = np.abs(outs[m].astype(int) - film[k].astype(int)).max()
        assert err <= noise, (m, k, err)


@pytest.mark.parametrize("noise", [0, 2])
def test_pulldown_comes_back_as_the_film(noise):
    """15 film frames telecined at four phases (0 .. 3 field slots cut off in front), five offsets of the stream's start in
    the cadence and both parities, clean and with independent +-2 noise per video frame."""
    film = film_frames(15, 1)
    rng = np.random.default_rng(2)
    for p in (M.TOP, M.BOTTOM):
        for phase in range(4):
            for start in range(5):
                video, early = M.telecine(film, W, H, p, phase, start)
                if noise:
                    video = np.clip(video.astype(int) + rng.integers(-noise, noise + 1, video.shape), 0, 255).astype(np.uint8)
                outs, info = M.detelecine_i420(video, W, H, p)
                recovered(film, video, early, outs, info, noise)
