"""Host build of the encoder with scene cuts (espflix_amd/csrc/enc_core.h + enc_rate.h + enc_cut.h through
tests/enc_cut_model_main.cpp), the sources of the scene-cut tests and the checks both test files share: the measure of
include/efx.h ("scene cuts") restated in NumPy, and the parser that takes picture types, temporal references and GOP headers
back out of an elementary stream.  The host model makes the decisions k_encode.hip makes, so its bytes, picture types and
sums are the device's."""
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

import encode_model as E

ROOT = E.ROOT
PIC = E.PIC
W, H = E.W, E.H
FLOOR = 8192           # enc_cut.h: kCutFloor
THRESHOLD = 144        # scene_cut=True
TYPE_I, TYPE_P, TYPE_CUT = 1, 2, 5
INFO = np.dtype([("cut_i", "<u4"), ("cut_p", "<u4"), ("type", "u1"), ("pad", "u1", 3)])


def build(out_dir: str) -> str:
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build enc_core.h, enc_rate.h and enc_cut.h"
    exe = os.path.join(out_dir, "enc_cut_model")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "enc_cut_model_main.cpp"), "-o", exe], check=True)
    return exe


@dataclass
class CutResult:
    stream: bytes
    recon: np.ndarray     # (n, 101376)
    qscales: np.ndarray   # (n,) uint8
    status: int           # ENCODE_VBV or 0
    types: np.ndarray     # (n,) uint8: 1 I, 2 P, 5 I by the cut rule alone
    cut_i: np.ndarray     # (n,) uint32
    cut_p: np.ndarray     # (n,) uint32
    state: bytes          # hand to the next call as state= to continue the stream (cont = 1)

    @property
    def scores(self):
        return scores(self.cut_i, self.cut_p)


def scores(cut_i, cut_p) -> np.ndarray:
    """round(256 cut_p / cut_i) per picture (256 where cut_i is 0)."""
    ci, cp = np.asarray(cut_i, dtype=np.int64), np.asarray(cut_p, dtype=np.int64)
    return np.where(ci > 0, (512 * cp + np.maximum(ci, 1)) // (2 * np.maximum(ci, 1)), 256)


def encode(exe: str, pics, *, scene_cut: int = 0, min_gop: int | None = None, bitrate: int = 0, vbv_bits: int = 250_000,
           qmin: int = 3, qmax: int = 31, gop=12, qscale=8, search=7, fmt=1, first_pts=0, code=4,
           state: bytes | None = None) -> CutResult:
    """One stream of the (n, 101376) I420 pictures.  scene_cut: the threshold (0 = off); min_gop defaults to
    max(1, gop // 2); bitrate 0: every picture at qscale.  state: a previous result's, to continue its stream."""
    pics = np.ascontiguousarray(pics, dtype=np.uint8).reshape(-1, PIC)
    min_gop = max(1, gop // 2) if min_gop is None else min_gop
    with tempfile.TemporaryDirectory() as td:
        src, out, rec, qf, inf, s_in, s_out = (os.path.join(td, n) for n in ("in.i420", "out.bin", "rec.i420", "q.bin", "info.bin",
                                                                             "s.in", "s.out"))
        pics.tofile(src)
        if state is not None:
            open(s_in, "wb").write(state)
        subprocess.run([exe, src, str(len(pics)), str(gop), str(qscale), str(search), str(fmt), str(first_pts), str(code),
                        str(bitrate), str(vbv_bits), str(qmin), str(qmax), str(scene_cut), str(min_gop), out, rec, qf, inf,
                        s_in if state is not None else "-", s_out], check=True, timeout=600)
        q = np.fromfile(qf, dtype=np.uint8)
        info = np.fromfile(inf, dtype=INFO)
        return CutResult(open(out, "rb").read(), np.fromfile(rec, dtype=np.uint8).reshape(-1, PIC), q[:-4].copy(),
                         int(q[-4:].view(np.uint32)[0]), info["type"].copy(), info["cut_i"].copy(), info["cut_p"].copy(),
                         open(s_out, "rb").read())


# -- sources ------------------------------------------------------------------------------------

def pan(n: int = 36, cut_at: int = 20, step=(4, 0), seeds=(21, 22)) -> np.ndarray:
    """n I420 pictures: the 352 x 192 window of a smooth random texture moves by `step` luma pels per picture (multiples of
    4: the measure searches the 4 x 4 decimated picture in whole pels); from picture cut_at on the texture is another one."""
    out = np.empty((n, PIC), dtype=np.uint8)
    big = [E.texture(s, W + 4 * n * abs(step[0]) + 8, H + 4 * n * abs(step[1]) + 8) for s in seeds]
    for p in range(n):
        t = big[0] if p < cut_at else big[1]
        x, y = p * abs(step[0]), p * abs(step[1])
        luma = t[y:y + H, x:x + W].astype(np.int32)
        ch = (luma[0::2, 0::2] + luma[0::2, 1::2] + luma[1::2, 0::2] + luma[1::2, 1::2] + 2) // 4
        out[p, :W * H] = luma.reshape(-1)
        out[p, W * H:W * H + W * H // 4] = (128 + (ch - 128) // 2).reshape(-1)
        out[p, W * H + W * H // 4:] = (255 - ch).reshape(-1)
    return out


# -- the measure of include/efx.h, restated ----------------------------------------------------------

def decimate(pic) -> np.ndarray:
    """(48, 88) int64: (sum of each 4 x 4 block of the luma + 8) >> 4."""
    y = np.asarray(pic).reshape(-1)[:W * H].astype(np.int64).reshape(H // 4, 4, W // 4, 4)
    return (y.sum(axis=(1, 3)) + 8) >> 4


def measure(pics):
    """(cut_i, cut_p) of every picture of one fresh stream, each picture against the previous source picture."""
    ci, cp, prev = [], [], None
    for pic in np.asarray(pics).reshape(-1, PIC):
        d = decimate(pic)
        blocks = d.reshape(12, 4, 22, 4).transpose(0, 2, 1, 3)                   # (r, c, 4, 4)
        mean = (blocks.sum(axis=(2, 3)) + 8) >> 4
        dev = np.abs(blocks - mean[:, :, None, None]).sum(axis=(2, 3))
        best = dev.copy()
        if prev is not None:
            best = np.full((12, 22), 1 << 40, dtype=np.int64)
            for dy in range(-4, 5):
                for dx in range(-4, 5):
                    # macroblocks whose block at (4 r + dy, 4 c + dx) lies wholly inside the picture
                    r0, r1 = (1 if dy < 0 else 0), (11 if dy > 0 else 12)
                    c0, c1 = (1 if dx < 0 else 0), (21 if dx > 0 else 22)
                    ref = prev[4 * r0 + dy:4 * r1 + dy, 4 * c0 + dx:4 * c1 + dx]
                    ref = ref.reshape(r1 - r0, 4, c1 - c0, 4).transpose(0, 2, 1, 3)
                    sad = np.abs(blocks[r0:r1, c0:c1] - ref).sum(axis=(2, 3))
                    best[r0:r1, c0:c1] = np.minimum(best[r0:r1, c0:c1], sad)
        ci.append(int(dev.sum()))
        cp.append(int(np.minimum(dev, best).sum()))
        prev = d
    return np.array(ci, dtype=np.uint32), np.array(cp, dtype=np.uint32)


def decide(cut_i, cut_p, *, gop: int, threshold: int, min_gop: int) -> list:
    """The rule of include/efx.h on a fresh stream: the type of every picture."""
    types, g = [], 0
    for k, (ci, cp) in enumerate(zip(cut_i, cut_p)):
        ci, cp = int(ci), int(cp)
        if k == 0 or g == gop:
            t = TYPE_I
        elif threshold > 0 and g >= min_gop and cp > FLOOR and 256 * cp > threshold * ci:
            t = TYPE_CUT
        else:
            t = TYPE_P
        g = g + 1 if t == TYPE_P else 1
        types.append(t)
    return types


# -- parser ------------------------------------------------------------------------------------

def es_headers(es: bytes) -> list:
    """[(picture_coding_type, temporal_reference, sequence header ahead, GOP time code's picture count or None)] per
    picture of an elementary stream (PES bytes may be given too)."""
    a = np.frombuffer(es, dtype=np.uint8)
    idx = np.flatnonzero((a[:-3] == 0) & (a[1:-2] == 0) & (a[2:-1] == 1))
    out, seq, gop_pictures = [], False, None
    for i in idx:
        code = int(a[i + 3])
        if code == 0xB3:
            seq = True
        elif code == 0xB8:
            tc = int.from_bytes(a[i + 4:i + 8].tobytes(), "big") >> 7    # the 25 bits of the time code
            gop_pictures = (tc & 63, (tc >> 6) & 63, (tc >> 13) & 63, (tc >> 19) & 31)   # pictures, seconds, minutes, hours
        elif code == 0x00:
            v = int.from_bytes(a[i + 4:i + 6].tobytes(), "big")
            out.append(((v >> 3) & 7, v >> 6, seq, gop_pictures))
            seq, gop_pictures = False, None
    return out


def check_headers(es: bytes, types, what: str = "", fps_nominal: int = 30, first_picture: int = 0):
    """Every I picture (types 1 and 5) carries a sequence and a GOP header whose time code counts the stream's pictures;
    temporal_reference is 0 for an I picture and the pictures since the last I picture for a P picture."""
    hdr = es_headers(es)
    assert len(hdr) == len(types), (what, len(hdr), len(types))
    g = None
    for k, ((ptype, tref, seq, tc), t) in enumerate(zip(hdr, types)):
        n = first_picture + k
        if int(t) in (TYPE_I, TYPE_CUT):
            want_tc = (n % fps_nominal, n // fps_nominal % 60, n // (60 * fps_nominal) % 60, n // (3600 * fps_nominal) % 24)
            assert (ptype, tref, seq, tc) == (1, 0, True, want_tc), (what, k, ptype, tref, seq, tc, want_tc)
            g = 1
        else:
            assert g is not None or first_picture, (what, k)
            if g is not None:
                assert (ptype, tref, seq, tc) == (2, g, False, None), (what, k, ptype, tref, seq, tc, g)
                g += 1
            else:
                assert (ptype, seq, tc) == (2, False, None), (what, k)
