"""Host build of the encoder at a picture rate (espflix_amd/csrc/enc_core.h + enc_rate.h through
tests/enc_picture_rate_model_main.cpp) and what the picture-rate tests share: the rewrite that turns a 30000/1001 Hz
elementary stream into the stream of another code, and the buffer model of include/efx.h with every picture's own gain."""
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

import conform_model as C
import encode_model as E

ROOT = E.ROOT
PIC = E.PIC
pts_offset = C.pts_offset
NOMINAL = C.NOMINAL


def build(out_dir: str) -> str:
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build enc_core.h and enc_rate.h"
    exe = os.path.join(out_dir, "enc_picture_rate_model")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "enc_picture_rate_model_main.cpp"), "-o", exe], check=True)
    return exe


@dataclass
class Result:
    stream: bytes
    recon: np.ndarray     # (n, 101376)
    qscales: np.ndarray   # (n,) uint8
    status: int           # ENCODE_VBV or 0
    level: int            # the buffer model's level after the last picture (rate control)
    state: bytes          # hand to the next call as state= to continue the stream (cont = 1)


def encode(exe: str, pics, *, code: int, bitrate: int = 0, vbv_bits: int = 250_000, qmin: int = 3, qmax: int = 31, gop=12, qscale=8,
           search=7, fmt=1, first_pts=0, state: bytes | None = None) -> Result:
    """One stream of the (n, 101376) I420 pictures at picture_rate `code`; bitrate 0: the fixed quantiser qscale."""
    pics = np.ascontiguousarray(pics, dtype=np.uint8).reshape(-1, PIC)
    with tempfile.TemporaryDirectory() as td:
        src, out, rec, qf, s_in, s_out = (os.path.join(td, n) for n in ("in.i420", "out.bin", "rec.i420", "q.bin", "s.in", "s.out"))
        pics.tofile(src)
        if state is not None:
            open(s_in, "wb").write(state)
        subprocess.run([exe, src, str(len(pics)), str(gop), str(qscale), str(search), str(fmt), str(first_pts), str(code),
                        str(bitrate), str(vbv_bits), str(qmin), str(qmax), out, rec, qf, s_in if state is not None else "-", s_out],
                       check=True, timeout=600)
        q = np.fromfile(qf, dtype=np.uint8)
        return Result(open(out, "rb").read(), np.fromfile(rec, dtype=np.uint8).reshape(-1, PIC), q[:-12].copy(),
                      int(q[-12:-8].view(np.uint32)[0]), int(q[-8:].view(np.int64)[0]), open(s_out, "rb").read())


def time_code(n: int, F: int) -> int:
    """The 25 bits of a GOP header for picture n at F pictures a second, drop_frame 0."""
    return ((n // (3600 * F)) % 24) << 19 | ((n // (60 * F)) % 60) << 13 | 1 << 12 | ((n // F) % 60) << 6 | n % F


def rewrite_es(es: bytes, code: int, first_picture: int = 0) -> bytes:
    """An elementary stream of the encoder with nothing changed but the picture_rate nibble of every sequence header and
    the time code of every GOP header, which becomes that of the picture behind it (counted from first_picture) at the
    code's nominal rate."""
    a = np.frombuffer(es, dtype=np.uint8).copy()
    idx = np.flatnonzero((a[:-3] == 0) & (a[1:-2] == 0) & (a[2:-1] == 1))
    n = first_picture
    for i in idx:
        c = int(a[i + 3])
        if c == 0xB3:
            a[i + 7] = (int(a[i + 7]) & 0xF0) | code
        elif c == 0xB8:
            w = int.from_bytes(a[i + 4:i + 8].tobytes(), "big")
            w = (time_code(n, NOMINAL[code]) << 7) | (w & 0x7F)
            a[i + 4:i + 8] = np.frombuffer(w.to_bytes(4, "big"), dtype=np.uint8)
        elif c == 0x00:
            n += 1
    return a.tobytes()


def sequence_codes(es: bytes) -> list:
    """The picture_rate nibble of every sequence header."""
    a = np.frombuffer(es, dtype=np.uint8)
    idx = np.flatnonzero((a[:-7] == 0) & (a[1:-6] == 0) & (a[2:-5] == 1) & (a[3:-4] == 0xB3))
    return [int(a[i + 7]) & 15 for i in idx]


def vbv(sizes, bitrate: int, vbv_bits: int, code: int, first_picture: int = 0, level=None):
    """include/efx.h's buffer model with G_k = bitrate x (offset(k + 1) - offset(k)): (underflow seen, final level)."""
    cap = vbv_bits * 90000
    F = cap if level is None else level
    under = False
    for k, b in enumerate(sizes, first_picture):
        F -= 8 * 90000 * b
        under |= F < 0
        F = min(cap, F + bitrate * (pts_offset(code, k + 1) - pts_offset(code, k)))
    return under, F


def ts_pts(ts: bytes, pid: int = 0x100) -> list:
    """The PTS of every PES of one PID of a transport stream."""
    a = np.frombuffer(ts, dtype=np.uint8).reshape(-1, 188)
    out = []
    for p in a:
        if not p[1] & 0x40 or ((int(p[1]) & 0x1F) << 8 | int(p[2])) != pid:
            continue
        o = 4 + (1 + int(p[4]) if p[3] & 0x20 else 0)
        h = p[o:o + 14]
        assert h[0] == 0 and h[1] == 0 and h[2] == 1 and h[7] & 0x80
        b = [int(v) for v in h[9:14]]
        out.append((b[0] >> 1 & 7) << 30 | b[1] << 22 | (b[2] >> 1) << 15 | b[3] << 7 | b[4] >> 1)
    return out
