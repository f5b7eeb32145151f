"""efx_conform_rate (k_conform.hip) on the device against tests/conform_model.py, byte for byte: drops, repeats, copies,
calls without outputs, pieces against the whole, a title index near 2^31, every refused argument, and Decoder.conform."""
import os
import pickle
import subprocess
import sys
import textwrap
from fractions import Fraction

import numpy as np
import pytest

import conform_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = 101376
PAD = 64        # bytes between streams in every padded region
FILL = 0xA5
ARG = -1
TOP = (1 << 31) - 1


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def title():
    """2 streams x 7 pictures of random bytes."""
    return np.random.default_rng(2027).integers(0, 256, (2, 7, PIC), dtype=np.uint8)


class Region:
    """n_streams x (images + one spare image) x 101376 bytes + a pad per stream, filled with FILL, on the device."""

    def __init__(self, dec, n_streams, images):
        self.n, self.images = n_streams, images
        self.stride = (images + 1) * PIC + PAD
        self.buf = dec.alloc(n_streams * self.stride)
        self.buf.upload(np.full(n_streams * self.stride, FILL, dtype=np.uint8))
        self.want = np.full((n_streams, self.stride), FILL, dtype=np.uint8)  # what the model expects there

    def expect(self, images):
        """images (n, k, 101376) from image 0 on."""
        k = images.shape[1]
        self.want[:, :k * PIC] = images.reshape(self.n, k * PIC)

    def check(self, what):
        got = self.buf.download(np.uint8, self.n * self.stride).reshape(self.n, self.stride)
        bad = np.argwhere(got != self.want)
        assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at (stream, byte) {bad[0].tolist()}"

    def free(self):
        self.buf.free()


def upload_padded(dec, pictures):
    """(n, P, 101376) pictures with a pad behind every stream: (buffer, stride)."""
    n, P, _ = pictures.shape
    stride = P * PIC + PAD
    host = np.full((n, stride), 0x5A, dtype=np.uint8)
    host[:, :P * PIC] = pictures.reshape(n, -1)
    buf = dec.alloc(n * stride)
    buf.upload(host)
    return buf, stride


def run_call(efx, dec, pictures, first, fps_in, code, what):
    """One call on padded regions against the model; returns the outputs (n, k, 101376)."""
    n, P, _ = pictures.shape
    want = M.conform(pictures, first, fps_in, code)
    src, src_stride = upload_padded(dec, pictures)
    dst = Region(dec, n, want.shape[1])
    got = dec.conform_to(src, dst.buf, n_streams=n, n_pictures=P, fps_in=fps_in, fps_out=M.RATES[code], first_picture=first,
                         src_stride=src_stride, dst_stride=dst.stride)
    dec.sync()
    assert got == want.shape[1] == efx.conform_count(fps_in, M.RATES[code], first, P) == M.count(first, P, fps_in, code), what
    dst.expect(want)
    dst.check(what)
    src.free()
    dst.free()
    return want


def test_one_stream_one_output(efx, title):
    """6336 items: six full runs and a tail of 192."""
    dec = efx.Decoder(1, 1)
    out = run_call(efx, dec, title[:1, :1], 0, Fraction(25), 3, "1 x 1")
    dec.close()
    assert out.shape == (1, 1, PIC)


CASES = [("15 -> 30", Fraction(15), 5, 4), ("50 -> 25", Fraction(50), 3, 7), ("60 -> 24000/1001", Fraction(60), 1, 7),
         ("25 -> 24", Fraction(25), 2, 7), ("1000000/41667 -> 30000/1001", Fraction(1000000, 41667), 4, 6),
         ("24 -> 24", Fraction(24), 2, 5)]


@pytest.mark.parametrize("what,fps_in,code,P", CASES, ids=[c[0] for c in CASES])
def test_two_streams_match_model(efx, title, what, fps_in, code, P):
    """Repeats (15 -> 30), drops (50 -> 25, 60 -> 24000/1001), a near rate, a container rate and a copy: padded strides,
    a spare image behind each stream; every byte outside the output images keeps its fill."""
    dec = efx.Decoder(2, 1)
    out = run_call(efx, dec, title[:, :P], 0, fps_in, code, what)
    dec.close()
    idx = [M.source(n, fps_in, code) for n in range(out.shape[1])]
    assert out.shape[1] >= 2 and np.array_equal(out, title[:, idx])
    if fps_in == M.RATES[code]:
        assert idx == list(range(P))
    if what == "15 -> 30":
        assert idx == [0, 0, 1, 1, 2, 2, 3, 3]
    if what == "50 -> 25":
        assert idx == [0, 2, 4, 6]


def test_call_without_outputs_writes_nothing(efx, title):
    """120 -> 30, one source picture offered: no outputs, EFX_OK, no byte written."""
    dec = efx.Decoder(2, 1)
    assert efx.conform_count(120, 30, 0, 1) == 0 and efx.conform_count(120, 30, 0, 2) == 1
    src, src_stride = upload_padded(dec, title[:, :1])
    dst = Region(dec, 2, 1)
    assert dec.conform_to(src, dst.buf, n_streams=2, n_pictures=1, fps_in=120, fps_out=30, src_stride=src_stride,
                          dst_stride=dst.stride) == 0
    dec.sync()
    dst.check("no outputs")
    dec.close()


@pytest.mark.parametrize("fps_in,code", [(Fraction(15), 5), (Fraction(50), 3), (Fraction(25), 2)])
def test_pieces_concatenate_to_the_whole(efx, title, fps_in, code):
    """Pieces of 1, 2 and 3 source pictures, first_picture carried on, against one call of 6."""
    dec = efx.Decoder(2, 1)
    whole = run_call(efx, dec, title[:, :6], 0, fps_in, code, "whole")
    parts, first = [], 0
    for cnt in (1, 2, 3):
        parts.append(run_call(efx, dec, title[:, first:first + cnt], first, fps_in, code, f"piece ({first}, {cnt})"))
        first += cnt
    dec.close()
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


def test_first_picture_near_2_to_31(efx, title):
    """The last three pictures a title can hold, with A = 2^31 - 1 and B = 2^31 - 128: (2 n + 1) A is just below 2^63."""
    big = Fraction(2147483647, 17895696)
    assert M.ratio(big, 8) == (2147483647, 2147483520)
    dec = efx.Decoder(2, 1)
    out = run_call(efx, dec, title[:, :3], TOP - 3, big, 8, "near 2^31")
    out25 = run_call(efx, dec, title[:, :3], TOP - 3, Fraction(50), 3, "50 -> 25 near 2^31")
    dec.close()
    assert out.shape[1] >= 1 and out25.shape[1] >= 1


def test_argument_errors(efx, title):
    """Every EFX_ERR_ARG case of include/efx.h returns its status and leaves the destination alone."""
    dec = efx.Decoder(2, 1)
    lib = efx.load_library()
    src, src_stride = upload_padded(dec, title[:, :6])
    dst = Region(dec, 2, 6)
    ok = dict(n_streams=2, n_pictures=6, in_num=25, in_den=1, out_code=2, first_picture=0, src_stride=src_stride, dst_stride=dst.stride)

    def status(s, d, **kw):
        f = {**ok, **kw}
        o = efx._ConformOpts(f["n_streams"], f["n_pictures"], f["in_num"], f["in_den"], f["out_code"], f["first_picture"],
                             f["src_stride"], f["dst_stride"])
        import ctypes
        return lib.efx_conform_rate(dec._ctx, ctypes.byref(o), s, d)

    S, D = src.ptr, dst.buf.ptr
    cases = [
        (S, D, dict(n_streams=0)), (S, D, dict(n_pictures=0)), (S, D, dict(in_num=0)), (S, D, dict(in_den=0)), (S, D, dict(in_num=-25)),
        (S, D, dict(out_code=0)), (S, D, dict(out_code=9)), (S, D, dict(first_picture=-1)),
        (S, D, dict(in_num=2147483647, in_den=17895698, out_code=8)),          # B = 2^31 + 112
        (S, D, dict(first_picture=TOP - 5)),                                   # first_picture + n_pictures = 2^31
        (S, D, dict(in_num=25, out_code=8, first_picture=TOP - 6)),            # the last output's index above 2^31 - 1
        (S, D, dict(in_num=1537, out_code=2)), (S, D, dict(in_num=1, in_den=3, out_code=2)),  # more than 64 : 1 apart
        (None, D, {}), (S, None, {}), (S + 8, D, {}), (S, D + 4, {}),
        (S, D, dict(src_stride=6 * PIC - 16)), (S, D, dict(src_stride=6 * PIC + 8)),
        (S, D, dict(dst_stride=5 * PIC)), (S, D, dict(dst_stride=6 * PIC + 8)),   # 25 -> 24 of 6 pictures: 6 outputs
    ]
    assert M.count(0, 6, Fraction(25), 2) == 6
    for k, (s, d, kw) in enumerate(cases):
        assert status(s, d, **kw) == ARG, (k, kw)
    dec.sync()
    dst.check("after the refused calls")
    assert status(S, D) == 0
    assert status(S, D, in_num=1536, n_pictures=1) == 0   # exactly 64 : 1 (no outputs from one picture)
    dec.sync()
    dec.close()


def test_decoder_conform_array(efx, title):
    dec = efx.Decoder(2, 1)
    for fps_in, fps_out, code in ((15, 30, 5), (Fraction(50), "25", 3), (23.976, "24000/1001", 1), (12.5, 25.0, 3)):
        out = dec.conform(title, fps_in, fps_out)
        assert isinstance(out, np.ndarray) and np.array_equal(out, M.conform(title, 0, efx._rate(fps_in), code))
    assert dec.conform(title[:, :1], 120, 30).shape == (2, 0, PIC)
    out = dec.conform(title[:, 2:5], 50, 25, first_picture=2)
    assert np.array_equal(out, M.conform(title[:, 2:5], 2, Fraction(50), 3))
    with pytest.raises(ValueError):
        dec.conform(title, 25, 15)
    dec.close()


TORCH_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    import espflix_amd as efx

    title = np.random.default_rng(2027).integers(0, 256, (2, 7, 101376), dtype=np.uint8)
    dec = efx.Decoder(2, 1, device=torch.cuda.current_device())
    t = torch.from_numpy(title).cuda()
    out = [dec.conform(t, 15, 30), dec.conform(t, 60, "24000/1001"), dec.conform(t[:, :1], 120, 30)]
    assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in out)
    dec.close()
    pickle.dump([o.cpu().numpy() for o in out], open(sys.argv[2], "wb"))
    print("conform ok")
""")


def test_decoder_conform_tensor(efx, title, tmp_path):
    """A tensor in, a tensor out (a process of its own: torch's HIP runtime first)."""
    script, out = tmp_path / "conform_tensor.py", tmp_path / "out.pkl"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "conform ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    up, down, none = pickle.load(open(out, "rb"))
    assert np.array_equal(up, M.conform(title, 0, Fraction(15), 5))
    assert np.array_equal(down, M.conform(title, 0, Fraction(60), 1))
    assert none.shape == (2, 0, PIC)
