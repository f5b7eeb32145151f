"""efx_compare_pictures (k_quality): the sums of squared errors, the Q16 SSIM sums and the macroblock maps of picture
batches made on the device, bit for bit against the NumPy model of include/efx.h's definition (tests/quality_model.py),
and encode(quality=True) against compare() of the same encode's reconstruction."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import encode_model as E
import quality_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
PIC = M.PIC
W, H = M.W, M.H
CB, CR = W * H, W * H + W * H // 4
FILL = 0x5A
MB_FILL = 0x5A5A5A5A
REC_FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def dec(efx):
    d = efx.Decoder(max_streams=2, max_pictures=2, ring_depth=3)
    yield d
    d.close()


@pytest.fixture(scope="module")
def base():
    """One noise picture: the reference of the one-pel cases."""
    return np.random.default_rng(3).integers(0, 256, PIC, dtype=np.uint8)


class Run:
    """One or more efx_compare_pictures calls over (n, 101376) pairs, into buffers with a guard record and a guard map
    behind the outputs.  Input gaps hold 0xA5, outputs 0x5A before the first call."""

    def __init__(self, dec, ref, test=None, *, ref_stride=0, test_stride=0, mb_stride=0, with_mb=True):
        self.dec, self.n = dec, len(ref)
        self.strides = (ref_stride, test_stride, mb_stride)
        self.bufs = []
        self.ref = self._upload(ref, ref_stride or PIC)
        self.test = self.ref if test is None else self._upload(test, test_stride or PIC)
        self.mbs = mb_stride or 264
        self.recs = self._filled(48 * (self.n + 1))
        self.mb = self._filled(4 * self.mbs * (self.n + 1)) if with_mb else None

    def _upload(self, pics, stride):
        host = np.full((len(pics), stride), 0xA5, dtype=np.uint8)
        host[:, :PIC] = pics
        buf = self.dec.alloc(host.size)
        buf.upload(host)
        self.bufs.append(buf)
        return buf

    def _filled(self, nbytes):
        buf = self.dec.alloc(nbytes)
        buf.upload(np.full(nbytes, FILL, dtype=np.uint8))
        self.bufs.append(buf)
        return buf

    def call(self, ref_max=0):
        """(sse (n, 3) uint64, ssim (n, 3) int64, maps (n, 264) uint32 or None); the guards are checked."""
        rs, ts, ms = self.strides
        self.dec.compare_to(self.ref, self.test, self.recs, n_images=self.n, ref_max=ref_max, ref_stride=rs, test_stride=ts,
                            mb_sse=self.mb, mb_stride=ms)
        self.dec.sync()
        recs = self.recs.download(np.uint64, 6 * (self.n + 1)).reshape(-1, 6)
        assert (recs[self.n] == REC_FILL).all(), "the record behind the last image was written"
        mb = None
        if self.mb is not None:
            maps = self.mb.download(np.uint32, self.mbs * (self.n + 1)).reshape(-1, self.mbs)
            assert (maps[self.n] == MB_FILL).all() and (maps[:, 264:] == MB_FILL).all(), "words between or behind the maps were written"
            mb = maps[:self.n, :264].copy()
        return recs[:self.n, :3].copy(), recs[:self.n, 3:].view(np.int64).copy(), mb

    def free(self):
        for b in self.bufs:
            b.free()


def compare_on_device(dec, ref, test, ref_max=0, **kw):
    run = Run(dec, ref, test, **kw)
    try:
        return run.call(ref_max)
    finally:
        run.free()


def assert_model(got, ref, test, ref_max=0):
    sse, ssim, mb = got
    want_sse, want_ssim, want_mb = M.compare_batch(ref, test, ref_max)
    bad = np.argwhere(sse != want_sse)
    assert bad.size == 0, f"{len(bad)} SSE differ, first (image, plane) = {bad[0].tolist()}"
    bad = np.argwhere(ssim != want_ssim)
    assert bad.size == 0, f"{len(bad)} SSIM sums differ, first (image, plane) = {bad[0].tolist()}: " \
                          f"{ssim[tuple(bad[0])] if bad.size else ''} != {want_ssim[tuple(bad[0])] if bad.size else ''}"
    if mb is not None:
        bad = np.argwhere(mb != want_mb)
        assert bad.size == 0, f"{len(bad)} macroblock SSE differ, first (image, macroblock) = {bad[0].tolist()}"
        assert np.array_equal(mb.astype(np.uint64).sum(axis=1), sse[:, 0])


def checkerboard(rows, cols):
    y, x = np.mgrid[0:rows, 0:cols]
    return (((x + y) & 1) * 255).astype(np.uint8)


def test_anchors(dec, base):
    """Identical pictures, all 0 against all 255 and the checkerboard against its inverse, on all three planes."""
    board = M.image_of(checkerboard(H, W), checkerboard(H // 2, W // 2), checkerboard(H // 2, W // 2))
    ref = np.stack([base, np.zeros(PIC, np.uint8), board])
    test = np.stack([base, np.full(PIC, 255, np.uint8), 255 - board])
    got = compare_on_device(dec, ref, test)
    sse, ssim, mb = got
    assert sse.tolist() == [[0, 0, 0], [4394649600, 1098662400, 1098662400], [4394649600, 1098662400, 1098662400]]
    assert ssim.tolist() == [[267976704, 64815104, 64815104], [0, 0, 0], [-267028056, 989 * -65304, 989 * -65304]]
    assert (mb[0] == 0).all() and (mb[1:] == 256 * 65025).all()
    assert_model(got, ref, test)


@pytest.mark.parametrize("n", [1, 3, 67])
def test_noise_against_the_model(dec, n):
    rng = np.random.default_rng(n)
    ref = rng.integers(0, 256, (n, PIC), dtype=np.uint8)
    test = np.clip(ref.astype(np.int64) + rng.integers(-9, 10, ref.shape), 0, 255).astype(np.uint8)
    test[0] = rng.integers(0, 256, PIC)   # (one unrelated pair: negative windows)
    assert_model(compare_on_device(dec, ref, test), ref, test)


def test_one_buffer_as_reference_and_test(dec):
    ref = np.random.default_rng(8).integers(0, 256, (3, PIC), dtype=np.uint8)
    sse, ssim, mb = compare_on_device(dec, ref, None)
    assert (sse == 0).all() and (mb == 0).all() and ssim.tolist() == [[267976704, 64815104, 64815104]] * 3


def one_pel_pairs(base, offsets):
    """Pairs that differ from the base in one byte each."""
    test = np.repeat(base[None], len(offsets), axis=0)
    for k, o in enumerate(offsets):
        test[k, o] ^= 0x80
    return np.repeat(base[None], len(offsets), axis=0), test


def test_one_pel_luma_sweep(dec, base):
    """192 pairs, a pel of every luma row: wherever the kernel's bands or its halo rows meet."""
    ref, test = one_pel_pairs(base, [y * W + (7 * y) % W for y in range(H)])
    got = compare_on_device(dec, ref, test)
    assert (got[0][:, 0] == 128 * 128).all() and (got[0][:, 1:] == 0).all()
    assert_model(got, ref, test)


@pytest.mark.parametrize("plane", [1, 2])
def test_one_pel_chroma_sweep(dec, base, plane):
    first = CB if plane == 1 else CR
    ref, test = one_pel_pairs(base, [first + y * (W // 2) + (7 * y) % (W // 2) for y in range(H // 2)])
    got = compare_on_device(dec, ref, test)
    assert (got[0][:, plane] == 128 * 128).all() and (got[0][:, 3 - plane] == 0).all() and (got[0][:, 0] == 0).all()
    assert_model(got, ref, test)


def test_corners(dec, base):
    luma = [(0, 0), (3, 3), (4, 4), (351, 191)]
    offsets = [y * W + x for x, y in luma] + [CB, CR - 1, CR, PIC - 1]
    ref, test = one_pel_pairs(base, offsets)
    got = compare_on_device(dec, ref, test)
    assert_model(got, ref, test)
    assert [int(np.flatnonzero(m)[0]) for m in got[2][:4]] == [0, 0, 0, 263]


def test_strides_and_guards(dec):
    rng = np.random.default_rng(21)
    ref = rng.integers(0, 256, (3, PIC), dtype=np.uint8)
    test = np.clip(ref.astype(np.int64) + rng.integers(-20, 21, ref.shape), 0, 255).astype(np.uint8)
    packed = compare_on_device(dec, ref, test)
    assert_model(packed, ref, test)
    strided = compare_on_device(dec, ref, test, ref_stride=PIC + 16, test_stride=PIC + 4096, mb_stride=268)
    for a, b in zip(strided, packed):
        assert np.array_equal(a, b)
    sse, ssim, mb = compare_on_device(dec, ref, test, ref_stride=PIC + 4096, test_stride=PIC + 16, with_mb=False)
    assert mb is None and np.array_equal(sse, packed[0]) and np.array_equal(ssim, packed[1])


def test_repeated_call_writes_the_records_in_full(dec):
    rng = np.random.default_rng(22)
    ref, test = rng.integers(0, 256, (3, PIC), dtype=np.uint8), rng.integers(0, 256, (3, PIC), dtype=np.uint8)
    run = Run(dec, ref, test, mb_stride=272)
    try:
        first = run.call()
        second = run.call()
    finally:
        run.free()
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    assert_model(second, ref, test)


def test_reference_clamp(dec):
    rng = np.random.default_rng(23)
    ref = rng.integers(0, 256, (3, PIC), dtype=np.uint8)
    ref[1] = rng.integers(244, 256, PIC)
    ref[2, ::3] = 255
    test = np.clip(ref.astype(np.int64) + rng.integers(-5, 6, ref.shape), 0, 250).astype(np.uint8)
    run = Run(dec, ref, test)
    try:
        got = {m: run.call(m) for m in (248, 0, 255, 1, 128)}
    finally:
        run.free()
    for m in (248, 0, 1, 128):
        assert_model(got[m], ref, test, m)
    for a, b in zip(got[0], got[255]):
        assert np.array_equal(a, b)
    assert (got[248][0][:, 0] != got[0][0][:, 0]).all()
    assert E.luma_psnr(ref, test) == pytest.approx(np.mean([M.psnr(int(s), M.SAMPLES[0]) for s in got[248][0][:, 0]]), abs=1e-9)


def test_offsets_above_32_bits(efx, dec):
    """Three images with test_stride = 2^31 + 16: the last one lies above 2^32.  Only the three images are uploaded."""
    stride = (1 << 31) + 16
    rng = np.random.default_rng(24)
    ref, test = rng.integers(0, 256, (3, PIC), dtype=np.uint8), rng.integers(0, 256, (3, PIC), dtype=np.uint8)
    try:
        big = dec.alloc(2 * stride + PIC)
    except efx.EfxError:
        pytest.skip("the device refused a 4.3 GB buffer")
    run = Run(dec, ref, None)
    try:
        for k in range(3):
            row = np.ascontiguousarray(test[k])
            assert dec._lib.efx_memcpy_h2d(dec._ctx, big.ptr + k * stride, row.ctypes.data, PIC) == 0
        run.test, run.strides = big, (0, stride, 0)
        got = run.call()
        run.ref, run.test, run.strides = big, run.ref, (stride, 0, 0)
        swapped = run.call()
    finally:
        run.free()
        big.free()
    assert_model(got, ref, test)
    for a, b in zip(got, swapped):
        assert np.array_equal(a, b)


def test_argument_errors(efx, dec):
    lib, ctx = dec._lib, dec._ctx
    ref, test = dec.alloc(2 * PIC + 4096), dec.alloc(2 * PIC + 4096)
    recs, mb = dec.alloc(256), dec.alloc(4096)
    recs.upload(np.full(256, FILL, dtype=np.uint8))
    mb.upload(np.full(4096, FILL, dtype=np.uint8))

    def call(r=ref.ptr, t=test.ptr, c=recs.ptr, m=mb.ptr, n=2, ref_max=0, rs=0, ts=0, ms=0):
        o = efx._CompareOpts(n, ref_max, rs, ts, ms)
        return lib.efx_compare_pictures(ctx, C.byref(o), r, t, c, m)

    bad = [dict(r=None), dict(t=None), dict(c=None), dict(r=ref.ptr + 8), dict(t=test.ptr + 4), dict(c=recs.ptr + 8), dict(m=mb.ptr + 8),
           dict(n=0), dict(n=-1), dict(ref_max=-1), dict(ref_max=256), dict(rs=PIC - 16), dict(rs=PIC + 8), dict(ts=PIC - 16),
           dict(ts=PIC + 8), dict(ms=260), dict(ms=266), dict(rs=16), dict(ms=4)]
    for kw in bad:
        assert call(**kw) == ARG, kw
    assert lib.efx_compare_pictures(ctx, None, ref.ptr, test.ptr, recs.ptr, None) == ARG
    dec.sync()
    assert (recs.download(np.uint8, 256) == FILL).all() and (mb.download(np.uint8, 4096) == FILL).all(), "a refused call wrote"
    good = [dict(), dict(m=None), dict(ref_max=255), dict(ref_max=1), dict(rs=PIC + 16, ts=PIC + 2048), dict(ms=268), dict(r=ref.ptr, t=ref.ptr)]
    for kw in good:
        assert call(**kw) == 0, kw
    dec.sync()
    for b in (ref, test, recs, mb):
        b.free()
    with pytest.raises(efx.EfxError) as e:
        dec.compare_to(0, 0, 0, n_images=1)
    assert e.value.status == ARG
    with pytest.raises(ValueError):
        dec.compare(np.zeros((2, PIC), np.uint8), np.zeros((3, PIC), np.uint8))
    with pytest.raises(ValueError):
        dec.compare(np.zeros((2, PIC - 1), np.uint8), np.zeros((2, PIC - 1), np.uint8))


@pytest.fixture(scope="module")
def clip_streams(efx, clips):
    """(3, 6, 101376): six pictures from three places of the clips the encode tests use."""
    out = []
    for name, first in (("splash", 0), ("splash", 40), ("vmedia", 20)):
        d = efx.Decoder(1, 100, ring_depth=101, max_stream_bytes=len(clips[name]) + 4096)
        d.upload([clips[name]], efx.FORMAT_TS)
        d.decode()
        out.append(np.concatenate([d.export_host("i420", picture=p) for p in range(first, first + 6)]))
        d.close()
    return np.stack(out)


def test_encode_with_quality(efx, clip_streams):
    pics = clip_streams
    dec = efx.Decoder(3, 6)
    try:
        plain = dec.encode(pics, gop=3)
        with_q = dec.encode(pics, gop=3, quality=True)
        with_r = dec.encode(pics, gop=3, recon=True)
        both = dec.encode(pics, gop=3, recon=True, quality=True)
        assert plain.quality is None and with_r.quality is None and with_q.recon is None
        assert plain.streams == with_q.streams == with_r.streams == both.streams
        assert np.array_equal(both.recon, with_r.recon)
        q = with_q.quality
        assert q.sse.shape == q.ssim_q16.shape == q.psnr.shape == q.ssim.shape == (3, 6, 3) and q.mb_sse is None
        assert q.sse.dtype == np.uint64 and q.ssim_q16.dtype == np.int64 and q.psnr.dtype == np.float64
        want = dec.compare(pics, with_r.recon, ref_max=248, macroblocks=True)
        for r in (q, both.quality):
            assert np.array_equal(r.sse, want.sse) and np.array_equal(r.ssim_q16, want.ssim_q16)
            assert np.array_equal(r.psnr, want.psnr) and np.array_equal(r.ssim, want.ssim)
        assert want.mb_sse.shape == (3, 6, 12, 22) and want.mb_sse.dtype == np.uint32
        sse, ssim, mb = M.compare_batch(pics, with_r.recon, 248)
        assert np.array_equal(want.sse.reshape(-1, 3), sse) and np.array_equal(want.ssim_q16.reshape(-1, 3), ssim)
        assert np.array_equal(want.mb_sse.reshape(-1, 264), mb)
        # the mean luma PSNR is encode_model.luma_psnr's.  A picture of these clips that the encoder reconstructs exactly has
        # sse 0 and PSNR +infinity here, while luma_psnr floors its mean squared error at 1e-10: such pictures enter the
        # mean with that floor's value, every other picture with its own
        luma, exact = q.psnr[..., 0], q.sse[..., 0] == 0
        assert np.isinf(luma[exact]).all() and np.isfinite(luma[~exact]).all() and not exact.all()
        floor_db = 10 * np.log10(255.0 ** 2 / 1e-10)
        assert float(np.where(exact, floor_db, luma).mean()) == pytest.approx(E.luma_psnr(pics, with_r.recon), abs=1e-9)
        for i in range(3):
            for p in np.flatnonzero(~exact[i]):
                assert luma[i, p] == pytest.approx(E.luma_psnr(pics[i, p], with_r.recon[i, p]), abs=1e-9)
        assert (q.ssim > 0).all() and (q.ssim <= 1).all() and (q.psnr[..., 0] > 20).all()
        # a stream that fills its region: the pictures that were not written give zeros, the others their numbers
        room = max(len(s) for s in plain.streams) // 2 // 16 * 16
        short = dec.encode(pics, gop=3, quality=True, dst_stride=room)
        lost = short.types == 0
        assert lost.any() and not lost.all()
        assert (short.quality.sse[lost] == 0).all() and (short.quality.ssim_q16[lost] == 0).all()
        assert (short.quality.psnr[lost] == 0).all() and (short.quality.ssim[lost] == 0).all()
        assert np.array_equal(short.quality.sse[~lost], q.sse[~lost]) and np.array_equal(short.quality.ssim_q16[~lost], q.ssim_q16[~lost])
    finally:
        dec.close()


TORCH_CHILD = textwrap.dedent("""
    import os
    import sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    import espflix_amd as efx

    pics = np.load(sys.argv[2])
    n, P = pics.shape[:2]
    torch.cuda.set_stream(torch.cuda.Stream())
    dec = efx.Decoder(n, P, device=torch.cuda.current_device(), hip_stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(31)
    test = np.clip(pics.astype(np.int64) + rng.integers(-7, 8, pics.shape), 0, 255).astype(np.uint8)
    same = lambda a, b: all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("sse", "ssim_q16", "psnr", "ssim"))
    host = dec.compare(pics, test, ref_max=248, macroblocks=True)
    t_ref, t_test = torch.from_numpy(pics).cuda(), torch.from_numpy(test).cuda()
    dev = dec.compare(t_ref, t_test, ref_max=248, macroblocks=True)
    assert same(host, dev) and np.array_equal(host.mb_sse, dev.mb_sse) and host.sse.shape == (n, P, 3)
    assert same(dec.compare(t_ref, test, ref_max=248), host)          # (a tensor against an array)
    flat = dec.compare(t_ref.view(-1, 101376)[1:], t_test.view(-1, 101376)[1:], ref_max=248)   # (a view that starts inside)
    assert np.array_equal(flat.sse, host.sse.reshape(-1, 3)[1:])
    own = dec.compare(t_ref, t_ref)
    assert (own.sse == 0).all() and (own.ssim == 1).all() and np.isinf(own.psnr).all()
    print("torch compare ok")

    a = dec.encode(pics, gop=3, quality=True)
    b = dec.encode(t_ref, gop=3, quality=True, recon=True)
    assert a.streams == b.streams and same(a.quality, b.quality) and isinstance(b.recon, torch.Tensor)
    assert same(dec.compare(t_ref, b.recon, ref_max=248), a.quality)
    pcm = np.zeros((n, 128 * 6), dtype=np.int16)
    titles, st = dec.encode_av(pics, pcm, gop=3)
    titles_q, st_q, qual = dec.encode_av(pics, pcm, gop=3, quality=True)
    assert titles == titles_q and np.array_equal(st, st_q) and same(qual, a.quality)
    dec.close()
    print("torch encode ok")
""")


def test_torch_tensors_and_encode_av(efx, clip_streams, tmp_path):
    """In a child process (torch's HIP runtime must come up first): compare() gives the same result for an array as for
    the same data in a tensor, encode(quality=True) likewise, and encode_av(quality=True) returns the same quality
    beside unchanged titles."""
    script = tmp_path / "torch_quality.py"
    script.write_text(TORCH_CHILD)
    np.save(tmp_path / "pics.npy", clip_streams)
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "pics.npy")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch compare ok" in r.stdout and "torch encode ok" in r.stdout
