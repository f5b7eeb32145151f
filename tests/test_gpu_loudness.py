"""efx_loudness_steps / efx_loudness_gate / efx_pcm_gain (k_loudness.hip): BS.1770-4 programme loudness of mono PCM and
the levelling gain on the device, bit for bit against the NumPy model of include/efx.h's formulas
(tests/loudness_model.py); normalize() and encode_av(loudness=) against the float64 yardstick (tests/loudness_float.py)."""
import ctypes as C
import functools
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import loudness_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
POISON, CANARY = 0x5A5B, 0x7B
MAX_STREAMS = 65
PIECES_16K = (1, 5, 799, 800, 801, 1599, 1600, 1601, 4807)


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def dec(efx):
    d = efx.Decoder(max_streams=MAX_STREAMS, max_pictures=1, ring_depth=2)
    yield d
    d.close()


def r8(v):
    return (v + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def signal(n, samples, seed=0):
    """[n, samples] int16, every stream different: full-scale noise with runs of both extremes, then quieter streams."""
    rng = np.random.default_rng(1000 * n + samples + seed)
    x = rng.integers(-32768, 32768, (n, samples), dtype=np.int64)
    x[:, 3::97] = 32767
    x[:, 5::89] = -32768
    x[:, 40:200] = 32767
    x[1::3] //= 7
    x[2::3] //= 300
    x = x.astype(np.int16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(n, samples, rate, seed=0):
    """(step records [n, n_steps], state [n, H]) of signal(n, samples, seed): computed once, shared, left unchanged."""
    x = signal(n, samples, seed)
    recs, st = M.step_records(x, rate), M.state(x, rate)
    recs.setflags(write=False)
    st.setflags(write=False)
    return recs, st


def device_steps(dec, x, rate, pieces=None):
    """efx_loudness_steps over x [n, samples] in `pieces` (queued back to back), padded strides.  Returns (records [n,
    n_steps], state [n, H] int16) after checking that nothing but the records and the state was written."""
    n, samples = x.shape
    pieces = pieces or (samples,)
    n_steps = M.step_count(rate, 0, samples)
    ss, H = n_steps + 3, M.hist_of(rate)
    d_st, d_steps = dec.alloc(n * 2 * H), dec.alloc(16 * n * ss)
    bufs, hosts = [d_st, d_steps], []
    try:
        d_st.upload(np.zeros(n * H, dtype=np.int16))
        d_steps.upload(np.full(16 * n * ss, CANARY, dtype=np.uint8))
        at = 0
        for p in pieces:
            ps = r8(p) + 8
            host = np.full((n, ps), POISON, dtype=np.int16)  # poison behind every stream's samples
            host[:, :p] = x[:, at:at + p]
            d_pcm = dec.alloc(2 * n * ps)
            bufs.append(d_pcm)
            d_pcm.upload(host)
            hosts.append((d_pcm, host))
            got = dec.loudness_steps_to(d_pcm, d_st, d_steps, n_streams=n, n_samples=p, rate=rate, first_sample=at, pcm_stride=ps,
                                        steps_stride=ss)
            assert got == M.step_count(rate, at, p)
            at += p
        assert at == samples
        dec.sync()
        raw = d_steps.download(np.uint8, 16 * n * ss).reshape(n, ss, 16)
        assert (raw[:, n_steps:] == CANARY).all(), "records behind a stream's steps were written"
        for d_pcm, host in hosts:
            assert np.array_equal(d_pcm.download(np.int16, host.size).reshape(host.shape), host), "the samples were written"
        recs = np.ascontiguousarray(raw[:, :n_steps]).view(M.STEP_DTYPE).reshape(n, n_steps)
        return recs, d_st.download(np.int16, n * H).reshape(n, H)
    finally:
        for b in bufs:
            b.free()


def assert_steps(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, f"{what}: {len(bad)} records differ, first at {bad[:1]}: {got[tuple(bad[0])] if len(bad) else ''}"


# ---- efx_loudness_steps -------------------------------------------------------------------------------------------------------
LENGTHS_16K = {"no_step": 1599, "3_steps": 4800, "4_steps": 6400, "4_steps_1": 6401, "67_steps_123": 67 * 1600 + 123}


@pytest.mark.parametrize("length", list(LENGTHS_16K), ids=list(LENGTHS_16K))
@pytest.mark.parametrize("n", [1, 3, 65])
def test_steps_16k(dec, n, length):
    samples = LENGTHS_16K[length]
    want, want_state = reference(n, samples, 16000)
    got, state = device_steps(dec, signal(n, samples), 16000)
    assert got.shape[1] == samples // 1600
    assert_steps(got, want, f"{n} x {length}")
    assert np.array_equal(state, want_state)
    assert (got["zero"] == 0).all()


@pytest.mark.parametrize("rate", [32000, 44100, 48000])
def test_steps_other_rates(dec, rate):
    """(44100: rows 8820 bytes apart, every row at another offset inside its 16-byte piece)"""
    n, samples = 3, 66 * M.step_of(rate) + 77
    want, want_state = reference(n, samples, rate)
    got, state = device_steps(dec, signal(n, samples), rate)
    assert_steps(got, want, str(rate))
    assert np.array_equal(state, want_state)


@pytest.mark.parametrize("rate", [16000, 44100])
def test_pieces_queued_back_to_back(dec, rate):
    """Pieces of any length without a sync in between give the records and the final state of one call."""
    n = 3
    scale = rate / 16000
    pieces = tuple(int(p * scale) if p > 5 else p for p in PIECES_16K)
    samples = 13 * M.step_of(rate) + 123
    pieces += (samples - sum(pieces),)
    assert pieces[-1] > 0
    want, want_state = reference(n, samples, rate)
    got, state = device_steps(dec, signal(n, samples), rate, pieces)
    assert_steps(got, want, "pieces")
    assert np.array_equal(state, want_state)


# ---- efx_loudness_gate --------------------------------------------------------------------------------------------------------
def device_gate(dec, recs, rate, thr, state=None):
    """recs: STEP_DTYPE [n, n_steps].  Returns REC_DTYPE [n]; a canary behind the records stays."""
    n, n_steps = recs.shape
    ss = n_steps + 2
    host = np.zeros((n, ss), dtype=M.STEP_DTYPE)
    host["energy"], host["peak"] = 0xFFFFFFFFFFFF, 40000  # what a read past n_steps would add
    host[:, :n_steps] = recs
    d_steps, d_recs = dec.alloc(max(16, host.nbytes)), dec.alloc(32 * n + 32)
    d_st = None
    try:
        d_steps.upload(host)
        d_recs.upload(np.full(32 * n + 32, CANARY, dtype=np.uint8))
        if state is not None:
            d_st = dec.alloc(state.nbytes)
            d_st.upload(state)
        dec.loudness_gate_to(d_steps, d_st, d_recs, n_streams=n, n_steps=n_steps, rate=rate, thresholds=thr, steps_stride=ss)
        dec.sync()
        raw = d_recs.download(np.uint8, 32 * n + 32)
        assert (raw[32 * n:] == CANARY).all()
        return raw[:32 * n].view(M.REC_DTYPE)
    finally:
        for b in (d_steps, d_recs, d_st):
            if b is not None:
                b.free()


def loud_quiet(rate):
    rng = np.random.default_rng(rate)
    x = rng.normal(0.0, 3276.8, 2 * rate + 77)
    x[rate:] *= 10.0 ** (-15.0 / 20.0)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def gate_streams():
    """name -> (samples, records, state) at 16 kHz, through the model."""
    rate = 16000
    rng = np.random.default_rng(4)
    long = (rng.normal(0.0, 2000.0, 600 * 1600 + 321) * np.repeat(10.0 ** (rng.integers(-30, 1, 601) / 20.0), 1600)[:600 * 1600 + 321])
    long = np.clip(np.round(long), -32768, 32767).astype(np.int16)
    long[100 * 1600:120 * 1600] = 0  # blocks under the absolute gate
    long[-5] = -32768  # the largest sample is a pending one
    xs = {"loud_quiet": loud_quiet(rate), "silence": np.zeros(8000 + 9, dtype=np.int16), "3_steps": signal(1, 4800 + 200)[0] // 3,
          "4_steps": signal(1, 6400)[0] // 3, "600_steps": long}
    return {k: (x, M.step_records(x, rate)[0], M.state(x, rate)[0]) for k, x in xs.items()}


@pytest.mark.parametrize("name", ["loud_quiet", "silence", "3_steps", "4_steps", "600_steps"])
def test_gate(dec, name):
    rate = 16000
    x, recs, state = gate_streams()[name]
    for target, peak in ((-23.0, -1.0), (-16.0, -6.0)):
        thr = M.thresholds(rate, target, peak)
        for st in (None, state):
            want = M.gate(recs, rate, thr, st)
            got = device_gate(dec, recs[None], rate, thr, None if st is None else st[None])[0]
            assert got == want, (name, target, st is not None, got, want)
    full, bare = M.gate(recs, rate, M.thresholds(rate), state), M.gate(recs, rate, M.thresholds(rate))
    if name == "loud_quiet":
        assert 0 < full["n_gated"] < full["n_abs"]
    if name == "silence":
        assert full["n_blocks"] == 2 and full["n_abs"] == 0 and full["gain_q12"] == 4096
    if name == "3_steps":
        assert full["n_blocks"] == 0 and full["gain_q12"] == 4096 and full["peak"] > 0
    if name == "600_steps":
        assert full["n_blocks"] == 597 and 0 < full["n_gated"] < full["n_abs"] < 597
        assert full["peak"] == 32768 > bare["peak"]  # the pending samples count only with the state


def test_gate_65_streams(dec):
    """65 streams of different contents in one call, real records and energies next to the top of their range."""
    rate, n = 44100, 65
    recs, state = reference(n, 9 * 4410 + 50, rate, seed=3)
    thr = M.thresholds(rate)
    got = device_gate(dec, recs, rate, thr, state)
    for i in range(n):
        assert got[i] == M.gate(recs[i], rate, thr, state[i]), i
    assert len({int(g) for g in got["gain_q12"]}) > 3
    rng = np.random.default_rng(6)
    big = np.zeros((n, 300), dtype=M.STEP_DTYPE)
    big["energy"] = rng.integers(0, 1 << 53, big.shape, dtype=np.uint64) >> rng.integers(0, 40, big.shape).astype(np.uint64)
    big["energy"][::5] = (1 << 54) - 1  # 4 x step x (3.4 x 2^19)^2: sums of blocks pass 64 bits
    big["peak"] = rng.integers(0, 32769, big.shape)
    got = device_gate(dec, big, rate, thr)
    for i in range(n):
        assert got[i] == M.gate(big[i], rate, thr), i


# ---- efx_pcm_gain -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 7, 8, 9, 4099])
def test_pcm_gain(dec, samples):
    n = 5
    x = signal(n, samples, seed=5)
    gains = np.array([1, 4096, 32767, 5000, 4095])
    recs = np.zeros(n, dtype=M.REC_DTYPE)
    recs["gain_q12"] = gains
    stride, ds = r8(samples) + 8, r8(samples) + 16
    host = np.full((n, stride), POISON, dtype=np.int16)
    host[:, :samples] = x
    d_src, d_dst, d_recs = dec.alloc(host.nbytes), dec.alloc(2 * n * ds), dec.alloc(recs.nbytes)
    try:
        d_recs.upload(recs)
        for use_recs, in_place in ((True, False), (False, False), (True, True), (False, True)):
            d_src.upload(host)
            d_dst.upload(np.full(n * ds, POISON + 1, dtype=np.int16))
            want = np.stack([M.apply_gain(x[i], gains[i] if use_recs else 7001) for i in range(n)])
            dst, dst_stride = (d_src, stride) if in_place else (d_dst, ds)
            dec.pcm_gain_to(d_src, d_recs if use_recs else None, dst, n_streams=n, n_samples=samples, fixed_gain_q12=7001,
                            src_stride=stride, dst_stride=dst_stride)
            dec.sync()
            out = dst.download(np.int16, n * dst_stride).reshape(n, dst_stride)
            assert np.array_equal(out[:, :samples], want), (samples, use_recs, in_place)
            assert (out[:, samples:] == (POISON if in_place else POISON + 1)).all(), "samples behind a stream's were written"
            if not in_place:
                assert np.array_equal(d_src.download(np.int16, host.size).reshape(host.shape), host)
    finally:
        for b in (d_src, d_dst, d_recs):
            b.free()
    assert np.array_equal(M.apply_gain(x[1], 4096), x[1])


# ---- Decoder.loudness / normalize / encode_av(loudness=) --------------------------------------------------------------------------
PTS0 = 129003


def av_inputs():
    """Two streams of six pictures with 0.8 s of the same sound 12 dB apart, 48 kHz mono in whole SBC frames."""
    import encode_model as E
    pics = np.stack([E.moving(6, seed=30 + i) for i in range(2)])
    t = np.arange(300 * 128)
    rng = np.random.default_rng(12)
    s = 6000 * np.sin(2 * np.pi * 440 * t / 48000) + 3000 * np.sin(2 * np.pi * 2500 * t / 48000) + rng.normal(0, 500, t.size)
    pcm = np.stack([np.round(s), np.round(s * 10.0 ** (-12.0 / 20.0))]).astype(np.int16)
    return pics, pcm


AV_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import test_gpu_loudness as T

    pics, pcm = T.av_inputs()
    dec = efx.Decoder(2, 1, 2, device=torch.cuda.current_device())
    res = dec.loudness(pcm, 48000)
    scaled, res2 = dec.normalize(pcm, 48000)
    scaled_t, res3 = dec.normalize(torch.from_numpy(pcm).cuda(), 48000, target=-16.0, peak=-3.0)
    assert isinstance(scaled, np.ndarray) and isinstance(scaled_t, torch.Tensor) and scaled_t.is_cuda
    before = torch.from_numpy(pcm).cuda()
    plain, st = dec.encode_av(torch.from_numpy(pics).cuda(), before, qscale=6, gop=6, first_pts=T.PTS0)
    assert (st == 0).all()
    none, st = dec.encode_av(torch.from_numpy(pics).cuda(), before, qscale=6, gop=6, first_pts=T.PTS0, loudness=None)
    assert (st == 0).all()
    # between encode_to and mux_to nothing may wait for the stream: an upload does (efx_memcpy_h2d synchronises it)
    queued, late = [False], []
    enc_to, mux_to, upload, dsync = dec.encode_to, dec.mux_to, efx.DeviceBuffer.upload, dec.sync
    dec.encode_to = lambda *a, **k: (enc_to(*a, **k), queued.__setitem__(0, True))[0]
    dec.mux_to = lambda *a, **k: (queued.__setitem__(0, False), mux_to(*a, **k))[1]
    dec.sync = lambda: (late.append("sync") if queued[0] else None, dsync())[1]
    efx.DeviceBuffer.upload = lambda self, arr: (late.append("upload") if queued[0] else None, upload(self, arr))[1]
    level, st = dec.encode_av(torch.from_numpy(pics).cuda(), before, qscale=6, gop=6, first_pts=T.PTS0, loudness=-23.0)
    efx.DeviceBuffer.upload = upload
    del dec.encode_to, dec.mux_to, dec.sync
    assert not late, f"encode_av(loudness=) synchronised between the encode and the mux: {late}"
    assert (st == 0).all() and np.array_equal(before.cpu().numpy(), pcm)  # the caller's tensor is not scaled
    video = dec.encode(torch.from_numpy(pics).cuda(), qscale=6, gop=6, first_pts=T.PTS0).streams
    frames = dec.sbc_encode(pcm).cpu().numpy()
    frames_scaled = dec.sbc_encode(scaled).cpu().numpy()
    pickle.dump(dict(res=res, res2=res2, res3=res3, scaled=scaled, scaled_t=scaled_t.cpu().numpy(), plain=plain, none=none,
                     level=level, video=video, frames=frames, frames_scaled=frames_scaled), open(sys.argv[2], "wb"))
    dec.close()
    print("loudness av ok")
""")


def test_normalize_and_encode_av(tmp_path):
    """Two streams of the same content 12 dB apart: both end within 0.1 LU of -23 by the yardstick, the title's SBC frames
    are sbc_encode of that scaled PCM, and loudness=None gives the bytes encode_av gives without the keyword.  In a child
    process (tensors: torch's HIP runtime first)."""
    import loudness_float as Y
    import mux_model as X
    script, out = tmp_path / "loudness_av.py", tmp_path / "out.pkl"
    script.write_text(AV_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "loudness av ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    o = pickle.load(open(out, "rb"))
    pics, pcm = av_inputs()
    res = o["res"]
    for i in range(2):
        rec, lufs = M.measure(pcm[i], 48000)
        assert res.integrated[i] == pytest.approx(lufs, abs=1e-9) and res.gain_q12[i] == rec["gain_q12"] == o["res2"].gain_q12[i]
        assert res.n_blocks[i] == rec["n_blocks"] == 5 and res.n_gated[i] == rec["n_gated"]
        assert res.peak_dbfs[i] == pytest.approx(20 * np.log10(int(rec["peak"]) / 32768.0)) and res.momentary_max[i] >= res.integrated[i]
        assert np.array_equal(o["scaled"][i], M.apply_gain(pcm[i], int(rec["gain_q12"])))
        after = Y.integrated(o["scaled"][i], 48000)[0]
        print(f"stream {i}: {res.integrated[i]:.3f} LUFS, gain {res.gain_db[i]:.3f} dB, after: {after:.4f} LUFS (float64)")
        assert abs(after + 23.0) <= 0.1
        rec16, _ = M.measure(pcm[i], 48000, target=-16.0, peak=-3.0)
        assert np.array_equal(o["scaled_t"][i], M.apply_gain(pcm[i], int(rec16["gain_q12"])))
    assert abs((res.integrated[0] - res.integrated[1]) - 12.0) < 0.05 and abs((res.gain_db[1] - res.gain_db[0]) - 12.0) < 0.05
    assert o["none"] == o["plain"]
    fb = o["frames"].shape[2]
    for i in range(2):
        v = np.frombuffer(o["video"][i], dtype=np.uint8)
        assert o["plain"][i] == X.mux(v, o["frames"][i].reshape(-1), frame_bytes=fb, first_pts=PTS0)[0], i
        assert o["level"][i] == X.mux(v, o["frames_scaled"][i].reshape(-1), frame_bytes=fb, first_pts=PTS0)[0], i
        assert o["level"][i] != o["plain"][i]


# ---- arguments ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(efx, dec):
    lib, ctx = dec._lib, dec._ctx
    pcm, st, steps, recs = dec.alloc(2 * 2 * 8000), dec.alloc(2 * 14400), dec.alloc(16 * 2 * 16), dec.alloc(128)
    try:
        def steps_call(p=pcm.ptr, t=st.ptr, s=steps.ptr, **kw):
            a = dict(n_streams=2, n_samples=6400, rate=16000, first_step=0, first_sample=0, pcm_stride=6400, steps_stride=8)
            a.update(kw)
            return lib.efx_loudness_steps(ctx, C.byref(efx._LoudnessStepsOpts(*a.values())), p, t, s)

        assert steps_call() == 4
        assert lib.efx_loudness_steps(ctx, None, pcm.ptr, st.ptr, steps.ptr) == ARG
        assert steps_call(rate=22050) == ARG and steps_call(rate=0) == ARG and steps_call(rate=8000) == ARG
        assert steps_call(p=None) == ARG and steps_call(t=None) == ARG and steps_call(s=None) == ARG
        assert steps_call(p=pcm.ptr + 8) == ARG and steps_call(t=st.ptr + 2) == ARG and steps_call(s=steps.ptr + 8) == ARG
        assert steps_call(pcm_stride=6392) == ARG and steps_call(pcm_stride=6404) == ARG and steps_call(pcm_stride=6408) == 4
        assert steps_call(steps_stride=3) == ARG and steps_call(steps_stride=4) == 4 and steps_call(first_step=5, steps_stride=8) == ARG
        assert steps_call(n_samples=0) == ARG and steps_call(n_samples=-3) == ARG and steps_call(n_samples=1599) == 0
        assert steps_call(n_streams=0) == ARG and steps_call(n_streams=MAX_STREAMS + 1) == ARG and steps_call(n_streams=-1) == ARG
        assert steps_call(first_step=-1) == ARG and steps_call(first_sample=-1) == ARG and steps_call(first_sample=1 << 40) == ARG

        thr = M.thresholds(16000)

        def gate_call(s=steps.ptr, t=None, r=recs.ptr, **kw):
            a = dict(n_streams=2, n_steps=4, rate=16000, abs_thr=thr[0], target_ms=thr[1], ceiling=thr[2], steps_stride=8)
            a.update(kw)
            return lib.efx_loudness_gate(ctx, C.byref(efx._LoudnessGateOpts(*a.values())), s, t, r)

        assert gate_call() == 0 and gate_call(t=st.ptr) == 0 and gate_call(n_steps=0) == 0
        assert lib.efx_loudness_gate(ctx, None, steps.ptr, None, recs.ptr) == ARG
        assert gate_call(rate=44101) == ARG and gate_call(s=None) == ARG and gate_call(r=None) == ARG
        assert gate_call(s=steps.ptr + 8) == ARG and gate_call(r=recs.ptr + 16) == 0 and gate_call(r=recs.ptr + 8) == ARG
        assert gate_call(t=st.ptr + 8) == ARG
        assert gate_call(steps_stride=3) == ARG and gate_call(n_steps=-1) == ARG and gate_call(n_steps=(1 << 24) + 1, steps_stride=1 << 25) == ARG
        assert gate_call(n_streams=0) == ARG and gate_call(n_streams=MAX_STREAMS + 1) == ARG
        assert gate_call(ceiling=0) == ARG and gate_call(ceiling=32768) == ARG and gate_call(target_ms=1 << 40) == ARG

        def gain_call(s=pcm.ptr, r=None, d=pcm.ptr, **kw):
            a = dict(n_streams=2, n_samples=100, fixed_gain_q12=4096, src_stride=104, dst_stride=104)
            a.update(kw)
            return lib.efx_pcm_gain(ctx, C.byref(efx._PcmGainOpts(*a.values())), s, r, d)

        assert gain_call() == 0 and gain_call(r=recs.ptr) == 0 and gain_call(r=recs.ptr, fixed_gain_q12=0) == 0
        assert lib.efx_pcm_gain(ctx, None, pcm.ptr, None, pcm.ptr) == ARG
        assert gain_call(s=None) == ARG and gain_call(d=None) == ARG and gain_call(s=pcm.ptr + 2) == ARG and gain_call(d=pcm.ptr + 8) == ARG
        assert gain_call(r=recs.ptr + 4) == ARG
        assert gain_call(src_stride=96) == ARG and gain_call(src_stride=100) == ARG and gain_call(dst_stride=96) == ARG
        assert gain_call(dst_stride=108) == ARG and gain_call(d=steps.ptr, dst_stride=112) == 0
        assert gain_call(n_samples=0) == ARG and gain_call(n_samples=-1) == ARG and gain_call(n_streams=0) == ARG
        assert gain_call(n_streams=MAX_STREAMS + 1) == ARG
        assert gain_call(fixed_gain_q12=0) == ARG and gain_call(fixed_gain_q12=32768) == ARG and gain_call(fixed_gain_q12=32767) == 0
        dec.sync()
        with pytest.raises(efx.EfxError) as e:
            dec.loudness_steps_to(pcm, st, steps, n_streams=2, n_samples=6400, rate=11025)
        assert e.value.status == ARG
    finally:
        for b in (pcm, st, steps, recs):
            b.free()
