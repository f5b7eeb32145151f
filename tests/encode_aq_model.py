"""Host build of the encoder with adaptive quantisation (espflix_amd/csrc/enc_aq.h + enc_core.h + enc_rate.h through
tests/enc_aq_model_main.cpp), the rule of include/efx.h ("adaptive quantisation") restated in NumPy independently of the
header, the sources of both test files and the reader that takes every macroblock's quantiser back out of a stream (the
oracle's parse trace).  The host model makes the decisions k_encode.hip makes, so its bytes and maps are the device's."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

import encode_model as E
import oracle

ROOT = E.ROOT
PIC = E.PIC
W, H = E.W, E.H
T_INTRA, T_PATTERN, T_FORWARD, T_QUANT = 1, 2, 8, 16   # macroblock_type flags (oracle/efx_oracle.h, EFXO_SYM_TYPE)
# (picture type, flags) of the four quant variants the encoder can write
QUANT_TYPES = {(1, T_INTRA | T_QUANT), (2, T_INTRA | T_QUANT), (2, T_PATTERN | T_QUANT), (2, T_FORWARD | T_PATTERN | T_QUANT)}


def build(out_dir: str) -> str:
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build enc_aq.h, enc_core.h and enc_rate.h"
    exe = os.path.join(out_dir, "enc_aq_model")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "enc_aq_model_main.cpp"), "-o", exe], check=True)
    return exe


def lengths(exe: str) -> dict:
    """The code lengths the bound beside enc_core.h's kMbMaxBits rests on, from the encoder's own tables."""
    words = subprocess.run([exe, "lengths"], check=True, capture_output=True, text=True).stdout.split()
    return {k: int(v) for k, v in zip(words[0::2], words[1::2])}


@dataclass
class AqResult:
    stream: bytes
    recon: np.ndarray       # (n, 101376)
    qscales: np.ndarray     # (n,) uint8: the pictures' quantisers
    maps: np.ndarray        # (n, 12, 22) uint8: the macroblocks'
    slice_len: np.ndarray   # (n, 12) uint32
    status: int             # ENCODE_VBV or 0
    state: bytes            # hand to the next call as state= to continue the stream (cont = 1)


def encode(exe: str, pics, *, aq: int, bitrate: int = 0, vbv_bits: int = 250_000, qmin: int = 3, qmax: int = 31, gop=12, qscale=8,
           search=7, fmt=1, first_pts=0, state: bytes | None = None) -> AqResult:
    """One stream of the (n, 101376) I420 pictures at strength `aq` (0 = off): at qscale, or with bitrate under rate
    control; state: a previous result's, to continue its stream."""
    pics = np.ascontiguousarray(pics, dtype=np.uint8).reshape(-1, PIC)
    with tempfile.TemporaryDirectory() as td:
        src, out, rec, qf, s_in, s_out, mf, lf = (os.path.join(td, n) for n in ("in.i420", "out.bin", "rec.i420", "q.bin", "s.in",
                                                                                "s.out", "mq.bin", "len.bin"))
        pics.tofile(src)
        if state is not None:
            open(s_in, "wb").write(state)
        subprocess.run([exe, src, str(len(pics)), str(gop), str(qscale), str(search), str(fmt), str(first_pts), str(bitrate),
                        str(vbv_bits), str(qmin), str(qmax), out, rec, qf, s_in if state is not None else "-", s_out, str(aq), mf, lf],
                       check=True, timeout=600)
        q = np.fromfile(qf, dtype=np.uint8)
        return AqResult(open(out, "rb").read(), np.fromfile(rec, dtype=np.uint8).reshape(-1, PIC), q[:-4].copy(),
                        np.fromfile(mf, dtype=np.uint8).reshape(-1, 12, 22), np.fromfile(lf, dtype=np.uint32).reshape(-1, 12),
                        int(q[-4:].view(np.uint32)[0]), open(s_out, "rb").read())


# -- the rule of include/efx.h, restated ------------------------------------------------------------

def activities(pic) -> np.ndarray:
    """a of the 264 macroblocks of one I420 picture, (12, 22) int64."""
    luma = np.asarray(pic).reshape(-1)[:W * H].astype(np.int64).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(H // 8, W // 8, 64)
    mean = (luma.sum(axis=-1) + 32) >> 6
    d = np.abs(luma - mean[..., None]).sum(axis=-1)
    return 1 + d.reshape(12, 2, 22, 2).min(axis=(1, 3))


def mq_map(pic, q: int, s: int, lo: int = 1, hi: int = 31) -> np.ndarray:
    """mq of the 264 macroblocks of one I420 picture coded at q with strength s, (12, 22) int64."""
    a = activities(pic)
    avg = (int(a.sum()) + 132) // 264
    num, den = (256 + s) * a + 256 * avg, 256 * a + (256 + s) * avg
    return np.clip((q * num + den // 2) // den, lo, hi)


# -- what a stream says ----------------------------------------------------------------------------

def trace(stream: bytes, fmt: int) -> list:
    """Per picture of the stream, from the oracle's parse trace: {"type": picture type, "slice_q": {row: the slice header's
    quantiser}, "mbs": [(address, macroblock_type flags or None for a skipped one, quantiser in force)]}."""
    pics, cur = [], {"flags": None}

    def cb(_user, kind, a, b, c, e):
        if kind == 0:      # slice: a = picture index, b = start code, c & 15 = picture type
            while len(pics) <= a:
                pics.append({"type": c & 15, "slice_q": {}, "mbs": []})
            cur["pic"], cur["row"] = pics[a], b - 1
        elif kind == 7 and a == 5 and c == 0:   # EFXO_SYM_QSCALE of a slice header
            cur["pic"]["slice_q"][cur["row"]] = b
        elif kind == 7 and a == 1:              # EFXO_SYM_TYPE
            cur["flags"] = b
        elif kind == 1:                         # EFXO_T_MB
            cur["pic"]["mbs"].append((a, None if b & 2 else cur["flags"], b >> 2))

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
    return pics


def check_stream(stream: bytes, fmt: int, maps, what: str = "") -> set:
    """Every slice header carries the map's column 0, every coded macroblock (intra, or with a pattern) is decoded at the
    map's quantiser, and a macroblock carries the quant flag exactly when that differs from the one in force before it.
    Returns the (picture type, macroblock_type flags) seen with the quant flag."""
    pics = trace(stream, fmt)
    assert len(pics) == len(maps), (what, len(pics), len(maps))
    seen = set()
    for p, (pic, m) in enumerate(zip(pics, maps)):
        assert pic["slice_q"] == {r: int(m[r, 0]) for r in range(12)}, (what, p, pic["slice_q"])
        cur = {}
        for addr, flags, q in pic["mbs"]:
            r, c = divmod(addr, 22)
            before = cur.get(r, int(m[r, 0]))
            if flags is None:   # skipped: no quantiser
                continue
            if flags & (T_INTRA | T_PATTERN):
                assert q == int(m[r, c]), (what, p, r, c, q, int(m[r, c]))
                assert bool(flags & T_QUANT) == (q != before), (what, p, r, c, flags, q, before)
                if flags & T_QUANT:
                    seen.add((pic["type"], flags))
            else:
                assert q == before and not flags & T_QUANT, (what, p, r, c, flags, q, before)
            cur[r] = q
    return seen


# -- sources ------------------------------------------------------------------------------------

ODD_AT = [(0, 15), (0, 16), (0, 21), (11, 15), (11, 16), (11, 21), (5, 0)]   # the seam between a lane's two word sets, the last tail lane


def _i420(luma, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    ch = rng.integers(96, 160, size=(2, H // 16, W // 16)).astype(np.uint8)   # one chroma value per macroblock
    return np.concatenate([np.asarray(luma, dtype=np.uint8).reshape(-1), np.kron(ch[0], np.ones((8, 8), np.uint8)).reshape(-1),
                           np.kron(ch[1], np.ones((8, 8), np.uint8)).reshape(-1)])


def directed(n: int = 3) -> np.ndarray:
    """n pictures made to bring out every quant variant.  Rows 0 .. 7: a texture that moves, its contrast set per
    macroblock of the screen (five steps, so neighbours differ in activity and the motion-compensated residual is
    coded: forward + pattern).  Rows 8 .. 11: the same but still, with fresh small noise per picture (pattern, zero
    vector).  A few macroblocks are flat at a brightness that changes by 60 per picture (intra in P pictures, and the
    smoothest of all, next to textured neighbours)."""
    big = E.texture(21, W + 64, H + 64).astype(np.int32)
    rr, cc = np.mgrid[0:12, 0:22]
    gain = np.kron((rr * 3 + cc * 2) % 5, np.ones((16, 16), dtype=np.int64))
    out = np.empty((n, PIC), dtype=np.uint8)
    for p in range(n):
        rng = np.random.default_rng(100 + p)
        tex = big[32:32 + H, 32:32 + W].copy()
        tex[:128] = big[32 + 2 * p:32 + 2 * p + 128, 32 + 3 * p:32 + 3 * p + W]
        luma = 128 + (tex - 128) * gain // 4
        luma[128:] += rng.integers(-6, 7, size=(H - 128, W))
        for k, (r, c) in enumerate([(1, 3), (2, 16), (4, 9), (6, 20), (9, 5), (10, 15)]):
            luma[16 * r:16 * r + 16, 16 * c:16 * c + 16] = 40 + 60 * p + 4 * k
        out[p] = _i420(np.clip(luma, 0, 255), 300 + p)
    return out


def tiled(n: int = 3) -> np.ndarray:
    """Pictures whose 264 macroblocks are copies of one 16 x 16 tile (chroma too), a different tile per picture."""
    out = np.empty((n, PIC), dtype=np.uint8)
    for p in range(n):
        rng = np.random.default_rng(40 + p)
        t = rng.integers(0, 249, size=(16, 16)).astype(np.uint8)
        ch = rng.integers(0, 249, size=(2, 8, 8)).astype(np.uint8)
        out[p] = np.concatenate([np.tile(t, (12, 22)).reshape(-1), np.tile(ch[0], (12, 22)).reshape(-1), np.tile(ch[1], (12, 22)).reshape(-1)])
    return out


def one_odd(kind: str, r: int, c: int, seed: int = 5) -> np.ndarray:
    """One picture: "noise_in_flat": flat 128 with full-range noise in macroblock (r, c); "faint_in_flat": the same with
    noise of 0 .. 3 around 128; "flat_in_noise": full-range noise with macroblock (r, c) flat 128."""
    rng = np.random.default_rng(seed + 31 * r + c)
    noise = rng.integers(0, 249, size=(H, W))
    luma = np.full((H, W), 128, dtype=np.int64) if kind != "flat_in_noise" else noise.copy()
    box = (slice(16 * r, 16 * r + 16), slice(16 * c, 16 * c + 16))
    luma[box] = {"noise_in_flat": noise[box], "faint_in_flat": 128 + noise[box] % 4, "flat_in_noise": 128}[kind]
    return np.concatenate([luma.astype(np.uint8).reshape(-1), np.full(PIC - W * H, 128, dtype=np.uint8)])
