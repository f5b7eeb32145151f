"""Host build of the rate-controlled encoder (espflix_amd/csrc/enc_core.h + enc_rate.h through
tests/enc_rate_model_main.cpp), the sources of the rate-control tests and the checks both test files share: the buffer
model of include/efx.h restated in Python integers, and the parsers that take picture sizes and quantisers back out of a
stream.  The host model makes the decisions k_encode.hip makes, so its bytes and quantisers are the device's."""
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

import encode_model as E

ROOT = E.ROOT
PIC = E.PIC
ENCODE_VBV = 4096
PROFILE = dict(vbv_bits=250_000, qmin=3, qmax=31)   # the reference indexer's -bufsize 0.25M -qmin 3


def build(out_dir: str) -> str:
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build enc_core.h and enc_rate.h"
    exe = os.path.join(out_dir, "enc_rate_model")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "enc_rate_model_main.cpp"), "-o", exe], check=True)
    return exe


@dataclass
class RateResult:
    stream: bytes
    recon: np.ndarray     # (n, 101376)
    qscales: np.ndarray   # (n,) uint8
    status: int           # ENCODE_VBV or 0
    state: bytes          # hand to the next call as state= to continue the stream (cont = 1)


def encode(exe: str, pics, *, bitrate: int, vbv_bits: int = 250_000, qmin: int = 3, qmax: int = 31, gop=12, qscale=8, search=7,
           fmt=1, first_pts=0, state: bytes | None = None) -> RateResult:
    """One stream of the (n, 101376) I420 pictures at `bitrate`; state: a previous result's, to continue its stream."""
    pics = np.ascontiguousarray(pics, dtype=np.uint8).reshape(-1, PIC)
    with tempfile.TemporaryDirectory() as td:
        src, out, rec, qf, s_in, s_out = (os.path.join(td, n) for n in ("in.i420", "out.bin", "rec.i420", "q.bin", "s.in", "s.out"))
        pics.tofile(src)
        if state is not None:
            open(s_in, "wb").write(state)
        subprocess.run([exe, src, str(len(pics)), str(gop), str(qscale), str(search), str(fmt), str(first_pts), str(bitrate),
                        str(vbv_bits), str(qmin), str(qmax), out, rec, qf, s_in if state is not None else "-", s_out],
                       check=True, timeout=600)
        q = np.fromfile(qf, dtype=np.uint8)
        return RateResult(open(out, "rb").read(), np.fromfile(rec, dtype=np.uint8).reshape(-1, PIC), q[:-4].copy(),
                          int(q[-4:].view(np.uint32)[0]), open(s_out, "rb").read())


# -- sources ------------------------------------------------------------------------------------

def sources(clip_i420: dict) -> dict:
    """V: vmedia's 72 pictures.  X: an easy stretch of the splash clip, then a cut to hard content on a P picture (picture
    18 of 36), an I picture six pictures later.  N: 4 pictures of uniform random bytes 0..248."""
    v = np.asarray(clip_i420["vmedia"]).reshape(-1, PIC)
    s = np.asarray(clip_i420["splash"]).reshape(-1, PIC)
    assert len(v) == 72 and len(s) >= 58
    n = np.random.default_rng(1).integers(0, 249, size=(4, PIC)).astype(np.uint8)
    return {"V": v, "X": np.concatenate([s[40:58], v[48:66]]), "N": n}


# -- parsers ------------------------------------------------------------------------------------

def ts_picture_bytes(ts: bytes) -> list:
    """Bytes of every picture of a video-only transport stream: its whole packets, from one payload_unit_start to the
    next."""
    a = np.frombuffer(ts, dtype=np.uint8)
    assert a.size % 188 == 0 and (a[0::188] == 0x47).all()
    starts = np.flatnonzero(a[1::188] & 0x40)
    assert len(starts) and starts[0] == 0
    edges = list(starts) + [a.size // 188]
    return [int(b - c) * 188 for c, b in zip(edges, edges[1:])]


def ts_payload(ts: bytes, pid: int = 0x100) -> bytes:
    """The PES bytes of one PID."""
    a = np.frombuffer(ts, dtype=np.uint8).reshape(-1, 188)
    out = []
    for p in a:
        if ((int(p[1]) & 0x1F) << 8 | int(p[2])) != pid:
            continue
        o = 4
        if p[3] & 0x20:
            o += 1 + int(p[4])
        if p[3] & 0x10:
            out.append(p[o:].tobytes())
    return b"".join(out)


def es_pictures(es: bytes) -> list:
    """[(bytes, [the five bits after every slice start code])] per picture of an elementary stream.  A picture begins at
    its sequence header when it has one (a GOP header follows it), else at its picture start code.  PES bytes may be given
    too (their E0 start codes are passed over; the byte counts then mean nothing)."""
    a = np.frombuffer(es, dtype=np.uint8)
    idx = np.flatnonzero((a[:-3] == 0) & (a[1:-2] == 0) & (a[2:-1] == 1))
    begins, quants, prev = [], [], None
    for i in idx:
        code = int(a[i + 3])
        if code == 0xB3 or (code == 0x00 and prev != 0xB8):
            begins.append(int(i))
            quants.append([])
        elif 1 <= code <= 0xAF:
            quants[-1].append(int(a[i + 4]) >> 3)
        prev = code
    edges = begins + [a.size]
    return [(b - c, q) for c, b, q in zip(edges, edges[1:], quants)]


def picture_sizes_and_quants(stream: bytes, fmt: int):
    """(bytes each picture appended to the output in `fmt`, the quantisers of its slices)."""
    if fmt == 1:
        sizes = ts_picture_bytes(stream)
        quants = [q for _, q in es_pictures(ts_payload(stream))]
    else:
        pics = es_pictures(stream)
        sizes, quants = [b for b, _ in pics], [q for _, q in pics]
    assert len(sizes) == len(quants)
    return sizes, quants


# -- the buffer model of include/efx.h, restated ----------------------------------------------------

def vbv(sizes, bitrate: int, vbv_bits: int, level=None):
    """Units 1/90000 bit.  C = vbv_bits x 90000, G = bitrate x 3003, cost = 8 x 90000 x bytes.  A fresh stream starts
    full; per picture: F -= cost; F < 0 is an underflow; F = min(C, F + G).  Returns (underflow seen, the level every
    picture started with, the lowest level after a picture's cost, the final level)."""
    C, G = vbv_bits * 90000, bitrate * 3003
    F = C if level is None else level
    under, before, low = False, [], C
    for b in sizes:
        before.append(F)
        F -= 8 * 90000 * b
        under |= F < 0
        low = min(low, F)
        F = min(C, F + G)
    return under, before, low, F


def check_stream(stream: bytes, fmt: int, qscales, status: int, *, bitrate: int, vbv_bits: int, qmin: int, qmax: int, qscale: int,
                 what: str = ""):
    """The honest status bit and quantisers of one fresh stream; returns (underflow, levels before each picture, lowest)."""
    sizes, quants = picture_sizes_and_quants(stream, fmt)
    assert len(sizes) == len(qscales), (what, len(sizes), len(qscales))
    for p, (qs, q) in enumerate(zip(quants, qscales)):
        assert len(qs) == 12 and all(x == int(q) for x in qs), (what, p, qs, int(q))
        assert qmin <= int(q) <= qmax, (what, p, int(q))
    assert int(qscales[0]) == min(max(qscale, qmin), qmax), (what, int(qscales[0]))
    under, before, low, _ = vbv(sizes, bitrate, vbv_bits)
    print(f"{what}: {bitrate} bit/s, {sum(sizes)} bytes, lowest level {low // 720000} bytes, underflow {under}, "
          f"q {[int(q) for q in qscales]}")
    assert bool(status & ENCODE_VBV) == under, (what, status, under, low)
    assert status & ~ENCODE_VBV == 0, (what, status)
    return under, before, low
