"""Host build of the encoder's arithmetic (espflix_amd/csrc/enc_core.h through tests/enc_model_main.cpp) and the test
sources of the encoder tests.  The host model makes the decisions k_encode.hip makes, so its bytes are the device's."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

import export_model as M
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = M.FRAME_BYTES
W, H = 352, 192


def build(out_dir: str) -> str:
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build enc_core.h"
    exe = os.path.join(out_dir, "enc_model")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "enc_model_main.cpp"), "-o", exe], check=True)
    return exe


def encode(exe: str, pics, gop=12, qscale=8, search=7, fmt=1, first_pts=0):
    """One stream of the (n, 101376) I420 pictures: (stream bytes, reconstruction (n, 101376))."""
    pics = np.ascontiguousarray(pics, dtype=np.uint8).reshape(-1, PIC)
    with tempfile.TemporaryDirectory() as td:
        src, out, rec = (os.path.join(td, n) for n in ("in.i420", "out.bin", "rec.i420"))
        pics.tofile(src)
        subprocess.run([exe, src, str(len(pics)), str(gop), str(qscale), str(search), str(fmt), str(first_pts), out, rec],
                       check=True, timeout=600)
        return open(out, "rb").read(), np.fromfile(rec, dtype=np.uint8).reshape(-1, PIC)


def build_blocks(out_dir: str) -> str:
    """tests/enc_blocks_main.cpp: enc_core.h's fdct8 and code_block on single blocks."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build enc_core.h"
    exe = os.path.join(out_dir, "enc_blocks")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "enc_blocks_main.cpp"), "-o", exe], check=True)
    return exe


def _run_blocks(exe: str, mode: str, data: np.ndarray, width: int) -> np.ndarray:
    with tempfile.TemporaryDirectory() as td:
        src, out = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        data.tofile(src)
        subprocess.run([exe, mode, src, out], check=True, timeout=600)
        return np.fromfile(out, dtype=np.int32).reshape(-1, width)


def fdct_blocks(exe: str, blocks) -> np.ndarray:
    """fdct8 of (n, 8, 8) integer blocks: (n, 8, 8) int32, 8 x the standard 2-D DCT."""
    blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1, 64)
    return _run_blocks(exe, "fdct", blocks, 64).reshape(-1, 8, 8)


def code_blocks(exe: str, intra, q, src, pred):
    """code_block on n blocks (intra / q per block, src / pred (n, 8, 8) uint8): fdct8's output (n, 8, 8), the levels in
    scan order (n, 64) and whether the halving loop ran (n)."""
    n = len(src)
    rec = np.empty((n, 130), dtype=np.uint8)
    rec[:, 0] = intra
    rec[:, 1] = q
    rec[:, 2:66] = np.asarray(src, dtype=np.uint8).reshape(n, 64)
    rec[:, 66:] = np.asarray(pred, dtype=np.uint8).reshape(n, 64)
    out = _run_blocks(exe, "code", rec, 129)
    return out[:, :64].reshape(n, 8, 8), out[:, 64:128], out[:, 128].astype(bool)


def luma_psnr(src, recon) -> float:
    """Mean luma PSNR of recon against src, source values above 248 taken as 248 (the decoder's clamp)."""
    y0 = np.minimum(np.asarray(src).reshape(-1, PIC)[:, :W * H].astype(np.float64), 248)
    y1 = np.asarray(recon).reshape(-1, PIC)[:, :W * H].astype(np.float64)
    mse = np.maximum(((y0 - y1) ** 2).mean(axis=1), 1e-10)
    return float(np.mean(10 * np.log10(255.0 ** 2 / mse)))


def p_vectors(stream: bytes, fmt: int):
    """Every macroblock of the P pictures as the test oracle parses them: (picture, address, intra, skipped, h, v), h / v
    the half-pel luma vector (its parse trace, efxo_set_trace)."""
    import ctypes as C
    out, cur = [], {"pic": -1, "type": 0}

    def cb(_user, kind, a, b, c, e):
        if kind == 0:    # slice: a = picture index, c & 15 = picture_coding_type
            cur["pic"], cur["type"] = a, c & 15
        elif kind == 1 and cur["type"] == 2:
            out.append((cur["pic"], a, b & 1, (b >> 1) & 1, c, e))

    FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int)
    fn = FN(cb)
    L = oracle.lib()
    L.efxo_set_trace.argtypes = [FN, C.c_void_p]
    data = np.frombuffer(stream, dtype=np.uint8).copy()
    L.efxo_set_trace(fn, None)
    try:
        L.efxo_decode(data.ctypes.data, data.size, fmt, 1, None, None, None, 0)
    finally:
        L.efxo_set_trace(FN(), None)
    return out


# -- sources ------------------------------------------------------------------------------------

def texture(seed: int, w: int = W + 64, h: int = H + 64) -> np.ndarray:
    """A smooth random texture (block-averaged noise), larger than a picture so that it can move."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, size=(h // 4 + 2, w // 4 + 2)).astype(np.float64)
    t = np.kron(t, np.ones((4, 4)))
    k = np.ones(5) / 5
    t = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, t)
    t = np.apply_along_axis(lambda c: np.convolve(c, k, mode="same"), 0, t)
    return np.clip(t[:h, :w], 0, 255).astype(np.uint8)


def moving(n: int, seed: int = 7, steps=((3, 1), (-2, 2), (1, -3), (4, 0), (-3, -2), (0, 4), (2, 2), (-4, 1))) -> np.ndarray:
    """n I420 pictures of a texture that moves by the given (dx, dy) luma steps, in half pels: even steps are full-pel
    motion, odd ones half-pel (the picture is taken from a texture at twice the resolution)."""
    big = texture(seed, 2 * (W + 64), 2 * (H + 64)).astype(np.int32)
    out = np.empty((n, PIC), dtype=np.uint8)
    x, y = 64, 64
    for p in range(n):
        if p:
            dx, dy = steps[(p - 1) % len(steps)]
            x, y = x + dx, y + dy
        full = big[y:y + 2 * H, x:x + 2 * W]
        luma = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + 2) // 4
        ch = (luma[0::2, 0::2] + luma[0::2, 1::2] + luma[1::2, 0::2] + luma[1::2, 1::2] + 2) // 4
        out[p, :W * H] = luma.reshape(-1)
        out[p, W * H:W * H + W * H // 4] = (128 + (ch - 128) // 2).reshape(-1)
        out[p, W * H + W * H // 4:] = (255 - ch).reshape(-1)
    return out


def checkerboard(n: int) -> np.ndarray:
    yy, xx = np.mgrid[0:H, 0:W]
    luma = np.where(((xx ^ yy) & 1) == 1, 255, 0).astype(np.uint8)
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    ch = np.where(((cx // 2 ^ cy // 2) & 1) == 1, 255, 0).astype(np.uint8).reshape(-1)
    pic = np.concatenate([luma.reshape(-1), ch, 255 - ch])
    return np.stack([pic if p % 2 == 0 else 255 - pic for p in range(n)])


def flat(n: int, value: int) -> np.ndarray:
    return np.full((n, PIC), value, dtype=np.uint8)


def noise(seed: int = 11) -> np.ndarray:
    """Two pictures of full-range random bytes."""
    import common
    return common.random_frames(seed).reshape(2, -1)[:, :PIC]


# -- checks shared by the host-model tests (test_encode_yardstick.py) and the device tests (test_gpu_encode.py) -----------

def mb_tables(stream: bytes, fmt: int) -> dict:
    """{picture: (intra, h, v)} of the P pictures of a stream, (12, 22) arrays from the oracle's parse trace; a skipped
    macroblock is inter with the zero vector, the vector of an intra macroblock reads 0."""
    out = {}
    for pic, addr, intra, _skipped, h, v in p_vectors(stream, fmt):
        t = out.setdefault(pic, tuple(np.full((12, 22), -99, dtype=np.int64) for _ in range(3)))
        t[0][addr // 22, addr % 22] = intra
        t[1][addr // 22, addr % 22] = 0 if intra else h
        t[2][addr // 22, addr % 22] = 0 if intra else v
    return out


def check_decisions(stream: bytes, fmt: int, pics, recon, gop: int, search: int) -> int:
    """Every macroblock of every P picture carries the (intra, h, v) the exhaustive search model (encode_float.decisions)
    derives from the source picture and the encoder's own previous reconstruction.  Exact.  Returns the macroblocks
    compared."""
    import encode_float as F
    tables = mb_tables(stream, fmt)
    want_pics = [p for p in range(len(pics)) if p % gop]
    assert sorted(tables) == want_pics, (sorted(tables), want_pics)
    for p in want_pics:
        got = tables[p]
        assert (got[0] >= 0).all(), f"picture {p}: the stream lacks macroblocks"
        want = F.decisions(pics[p], recon[p - 1], search)
        for name, g, w in zip(("intra", "h", "v"), got, want):
            bad = np.argwhere(g != w)
            assert not len(bad), (f"search {search} picture {p}: {name} differs from the search model in {len(bad)} macroblocks; "
                                  f"first (row, column) {tuple(bad[0])}: encoder (intra, h, v) = "
                                  f"{tuple(int(t[tuple(bad[0])]) for t in got)}, model {tuple(int(t[tuple(bad[0])]) for t in want)}")
    return 264 * len(want_pics)


PSNR_JSON = os.path.join(ROOT, "tests", "golden", "encode_psnr.json")
QUALITY_Q = (1, 2, 4, 8, 16, 31)
QUALITY_GOP, QUALITY_SEARCH = 4, 7


def quality_sources(clip_i420: dict) -> dict:
    """The three 12-picture sources of the quality check; clip_i420: every picture of the two clips as I420."""
    return {"splash": clip_i420["splash"][14:26], "vmedia": clip_i420["vmedia"][14:26], "moving": moving(12)}


def neighbour_q(q: int) -> int:
    return q + 1 if q < 31 else 30


def check_quality(record: dict, name: str, q: int, pics, recon, what: str) -> list:
    """The encoder's mean luma PSNR of the I pictures and of the P pictures is at least the float yardstick's
    (tests/golden/encode_psnr.json) less the recorded margin, a quarter of the yardstick's own step to the neighbouring
    qscale.  Returns the failures (and prints every figure)."""
    import encode_float as F
    got = F.psnr_by_type(pics, recon, QUALITY_GOP)
    rec = record["cases"][f"{name}_q{q}"]
    failures = []
    for t, g in zip("IP", got):
        print(f"{what} {name:7s} q {q:2d} {t}: {g:7.3f} dB, yardstick {rec[t]:7.3f} dB ({g - rec[t]:+.3f}), margin {rec[t + '_margin']:.3f}")
        if not g >= rec[t] - rec[t + "_margin"]:
            failures.append((name, q, t, round(g, 3), rec[t], rec[t + "_margin"]))
    return failures
