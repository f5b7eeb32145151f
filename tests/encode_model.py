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
