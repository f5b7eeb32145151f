"""The float64 yardstick of the loudness tests: ITU-R BS.1770-4 / EBU R 128 integrated loudness of one mono int16 stream,
the K-weighting run serially with the whole history by tests/loudness_float_main.cpp (double, built here with the host
compiler), the gating in float64 below.  Shares no code with tests/loudness_model.py or espflix_amd/csrc/loudness_px.h."""
import atexit
import functools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _exe():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build tests/loudness_float_main.cpp"
    tmp = tempfile.mkdtemp(prefix="loudness_float_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, "loudness_float")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "loudness_float_main.cpp"), "-o", out],
                   check=True, capture_output=True, text=True)
    return out


def block_mean_squares(x, rate):
    """Mean squares of the K-weighted 400 ms blocks every 100 ms, full scale = 1: float64 [n_blocks]."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "pcm.bin"), os.path.join(d, "blocks.bin")
        np.ascontiguousarray(x, dtype=np.int16).tofile(src)
        subprocess.run([_exe(), str(rate), src, dst], check=True, timeout=600)
        return np.fromfile(dst, dtype=np.float64)


def to_lufs(ms):
    return -0.691 + 10.0 * math.log10(ms) if ms > 0 else -math.inf


def integrated(x, rate):
    """(integrated loudness in LUFS, -inf when nothing passes the gates; maximum momentary loudness; blocks; gated blocks)."""
    z = block_mean_squares(x, rate)
    momentary = to_lufs(float(z.max())) if z.size else -math.inf
    above = z[z > 10.0 ** ((-70.0 + 0.691) / 10.0)]
    if not above.size:
        return -math.inf, momentary, int(z.size), 0
    gated = above[above > 0.1 * above.mean()]  # 10 LU below the loudness of what passed the absolute gate
    return to_lufs(float(gated.mean())), momentary, int(z.size), int(gated.size)
