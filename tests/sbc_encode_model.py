"""Host build of the SBC encoder's arithmetic (espflix_amd/csrc/sbc_enc_core.h through tests/sbc_enc_model_main.cpp), the
test signals, a NumPy parser of SBC frames and the gain / SNR fit of the SBC encoder tests.  The host model makes the
decisions k_sbc_enc.hip makes, so its bytes are the device's."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIST = 72
STATE_BYTES = 2 * HIST * 2
DELAY = 73                   # samples between PCM in and PCM out: 80-tap prototype, 8 subbands
RATE = 48000
OFFSET8 = [[-2, 0, 0, 0, 0, 0, 0, 1], [-3, 0, 0, 0, 0, 0, 1, 2], [-4, 0, 0, 0, 0, 0, 1, 2], [-4, 0, 0, 0, 0, 0, 1, 2]]


def frame_bytes(blocks: int, channels: int, bitpool: int) -> int:
    return 4 + 4 * channels + (blocks * channels * bitpool + 7) // 8


def build(out_dir: str) -> str:
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to build sbc_enc_core.h"
    exe = os.path.join(out_dir, "sbc_enc_model")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sbc_enc_model_main.cpp"), "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=1)
def model_exe() -> str:
    """The model binary, built once per process into a directory of its own."""
    d = tempfile.mkdtemp(prefix="sbc_enc_model_")
    return build(d)


def encode(exe, pcm, *, blocks=16, mode=0, allocation=0, bitpool=28, frequency=3, layout=0, state=None, check=True):
    """pcm: int16 [n_streams, n_frames x blocks x 8 x channels] (or one stream, 1-D).  Returns (frames uint8 [n_streams,
    n_frames, frame_bytes], max |S| uint32 [n_streams, n_frames, channels, 8], state uint8 [n_streams, 288], status): status
    3 = a 32-bit intermediate differed from its 64-bit evaluation (raises unless check=False)."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    if pcm.ndim == 1:
        pcm = pcm[None]
    ch = 2 if mode else 1
    n, per = pcm.shape[0], blocks * 8 * ch
    assert pcm.shape[1] % per == 0
    n_frames = pcm.shape[1] // per
    fb = frame_bytes(blocks, ch, bitpool)
    with tempfile.TemporaryDirectory() as td:
        p = {k: os.path.join(td, k) for k in ("pcm", "st_in", "st_out", "frames", "maxabs")}
        pcm.tofile(p["pcm"])
        st_in = "-"
        if state is not None:
            np.ascontiguousarray(state, dtype=np.uint8).reshape(n, STATE_BYTES).tofile(p["st_in"])
            st_in = p["st_in"]
        r = subprocess.run([exe, p["pcm"]] + [str(v) for v in (n, n_frames, frequency, blocks, mode, allocation, bitpool, layout)] +
                           [st_in, p["st_out"], p["frames"], p["maxabs"]], timeout=1200)
        assert r.returncode in (0, 3), r.returncode
        if check:
            assert r.returncode == 0, "a 32-bit intermediate of the analysis wrapped"
        return (np.fromfile(p["frames"], dtype=np.uint8).reshape(n, n_frames, fb),
                np.fromfile(p["maxabs"], dtype=np.uint32).reshape(n, n_frames, ch, 8),
                np.fromfile(p["st_out"], dtype=np.uint8).reshape(n, STATE_BYTES), r.returncode)


# -- signals (int16, 48 kHz) -------------------------------------------------------------------

def signal(name: str, n: int = 60 * 128, seed: int = 1) -> np.ndarray:
    t = np.arange(n) / RATE
    rng = np.random.default_rng(seed)
    if name == "sine":
        x = 32768 * 10 ** (-6 / 20) * np.sin(2 * np.pi * 1000 * t)
    elif name == "chord":
        x = 6000 * (np.sin(2 * np.pi * 220 * t) + np.sin(2 * np.pi * 1330 * t) + np.sin(2 * np.pi * 5100 * t))
    elif name == "lowpass":
        x = np.convolve(rng.normal(0, 3000, n + 7), np.ones(8) / 8, mode="valid")
    elif name == "white":
        x = rng.normal(0, 8000, n)
    elif name == "square":
        x = np.where(np.sin(2 * np.pi * 440 * t) >= 0, 32767.0, -32768.0)
    elif name == "silence":
        x = np.zeros(n)
    elif name == "one":
        x = np.ones(n)
    else:
        raise KeyError(name)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


SIGNALS = ("sine", "chord", "lowpass", "white", "square")


def worst_case(blocks: int = 16, n_frames: int = 8) -> np.ndarray:
    """[16, samples]: for each folded window sum T[k] two inputs that put full scale on every one of its taps with the sign
    of the tap's coefficient (32767 / -32768, and the mirrored -32768 / 32767), the other taps signed so that subband k's
    matrix row adds up too: every tenth block of the periodic signal meets the analysis' bounds."""
    from math import cos, pi
    taps = _proto()
    sign = lambda v: 1 if v >= 0 else -1
    n = n_frames * blocks * 8
    out = []
    for k in range(8):
        first = 4 + k
        second = -1 if k == 0 else (4 - k if k <= 4 else 20 - k)
        x = np.zeros(80, dtype=np.int64)
        for i in range(80):
            x[i] = sign(taps[i]) * sign(cos((k + 0.5) * ((i % 16) - 4) * pi / 8))
        for j in range(5):
            x[first + 16 * j] = sign(taps[first + 16 * j])
            if second >= 0:
                x[second + 16 * j] = sign(taps[second + 16 * j]) * (1 if k <= 4 else -1)
        pat = x[::-1]  # X[n] is the sample n places back from the block's newest: the pattern ends on a block's last sample
        for flip in (1, -1):
            line = np.where(pat * flip > 0, 32767, -32768)
            out.append(np.tile(line, n // 80 + 1)[:n].astype(np.int16))
    return np.stack(out)


def _proto() -> np.ndarray:
    """Proto_8_80 as espflix_amd/csrc/sbc_proto.h holds it."""
    import re
    src = open(os.path.join(ROOT, "espflix_amd", "csrc", "sbc_proto.h")).read()
    body = src[src.index("kSbcProtoHalf[41]"):]
    half = np.array([float(v) for v in re.findall(r"-?\d\.\d+E[+-]\d+", body[:body.index("};")])])
    assert half.size == 41
    full = np.empty(80)
    for i in range(80):
        h = i if i <= 40 else 80 - i
        full[i] = -half[h] if (i > 40 and h in (16, 32)) else half[h]
    return full


# -- frames ------------------------------------------------------------------------------------

def crc8(data) -> int:
    crc = 0x0F
    for b in data:
        crc ^= int(b)
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1D) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


def allocation_bits(frequency: int, allocation: int, bitpool: int, scale) -> list:
    """The decoder's bit allocation (reference src/sbc_decoder.cpp:142-233), one channel."""
    need = []
    for sb, s in enumerate(scale):
        s = int(s)
        if allocation:
            need.append(s)
        elif s == 0:
            need.append(-5)
        else:
            l = s - OFFSET8[frequency][sb]
            need.append(l // 2 if l > 0 else l)
    bitcount, slicecount, bitslice = 0, 0, max(0, max(need)) + 1
    while True:
        bitslice -= 1
        bitcount += slicecount
        slicecount = 0
        for v in need:
            if bitslice + 1 < v < bitslice + 16:
                slicecount += 1
            elif v == bitslice + 1:
                slicecount += 2
        if bitcount + slicecount >= bitpool:
            break
    if bitcount + slicecount == bitpool:
        bitcount += slicecount
        bitslice -= 1
    bits = [0 if v < bitslice + 2 else min(v - bitslice, 16) for v in need]
    for sb in range(8):
        if bitcount >= bitpool:
            break
        if 2 <= bits[sb] < 16:
            bits[sb] += 1
            bitcount += 1
        elif need[sb] == bitslice + 1 and bitpool > bitcount + 1:
            bits[sb] = 2
            bitcount += 2
    for sb in range(8):
        if bitcount >= bitpool:
            break
        if bits[sb] < 16:
            bits[sb] += 1
            bitcount += 1
    return bits


def parse_frame(frame) -> dict:
    """Header fields, scale factors [ch][8], bit widths [ch][8] (this file's copy of the allocation), the quantised samples
    [blk][ch][8] (-1 where a subband has no bits) and the byte the sample bits end in."""
    f = np.asarray(frame, dtype=np.uint8)
    h = dict(sync=int(f[0]), frequency=int(f[1]) >> 6, blocks=4 * (((int(f[1]) >> 4) & 3) + 1), mode=(int(f[1]) >> 2) & 3,
             allocation=(int(f[1]) >> 1) & 1, subbands=8 if f[1] & 1 else 4, bitpool=int(f[2]), crc=int(f[3]))
    ch = 2 if h["mode"] else 1
    sf = np.empty((ch, 8), dtype=np.int64)
    for c in range(ch):
        for sb in range(8):
            b = int(f[4 + (c * 8 + sb) // 2])
            sf[c, sb] = b & 15 if sb & 1 else b >> 4
    bits = [allocation_bits(h["frequency"], h["allocation"], h["bitpool"], sf[c]) for c in range(ch)]
    stream = np.unpackbits(f[4 + 4 * ch:])
    q = np.full((h["blocks"], ch, 8), -1, dtype=np.int64)
    pos = 0
    for blk in range(h["blocks"]):
        for c in range(ch):
            for sb in range(8):
                n = bits[c][sb]
                if n:
                    assert pos + n <= stream.size, "the sample bits run past the frame"
                    q[blk, c, sb] = int("".join(map(str, stream[pos:pos + n])), 2)
                    pos += n
    h.update(channels=ch, scale=sf, bits=np.array(bits), q=q, end=4 + 4 * ch + (pos + 7) // 8,
             crc_want=crc8(f[1:3].tolist() + f[4:4 + 4 * ch].tolist()))
    return h


# -- gain, delay and SNR -------------------------------------------------------------------------

def fit(src: np.ndarray, dec: np.ndarray, delay: int = DELAY, skip: int = 256):
    """Least-squares gain of dec against src delayed by `delay`, and the SNR of the fit in dB, the first `skip` output samples
    dropped."""
    n = min(len(src), len(dec) - delay)
    x = np.asarray(src[:n], dtype=np.float64)[skip:]
    y = np.asarray(dec[delay:delay + n], dtype=np.float64)[skip:]
    g = float(np.dot(x, y) / max(np.dot(x, x), 1e-30))
    err = y - g * x
    snr = 10 * np.log10(max(np.dot(g * x, g * x), 1e-30) / max(np.dot(err, err), 1e-30))
    return g, float(snr)


def best_delay(src: np.ndarray, dec: np.ndarray, lo: int = 60, hi: int = 90) -> int:
    return max(range(lo, hi), key=lambda d: fit(src, dec, d)[1])


def deplanar(pcm: np.ndarray, blocks: int, channels: int) -> np.ndarray:
    """The decoder's output (per frame: channel 0's samples, then channel 1's) as [channels, samples]."""
    return np.asarray(pcm).reshape(-1, channels, blocks * 8).transpose(1, 0, 2).reshape(channels, -1)
