"""efx_import_pcm (k_import_pcm): int16 PCM of any rate and channel count downmixed and resampled to the SBC rates on the
device, bit for bit against the NumPy model of include/efx.h's formulas (tests/import_pcm_model.py)."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import import_pcm_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
BIG = (1 << 33) + 5
TILE = 1024
POISON, CANARY = 0x5A5B, 0x7B7C
MIX = {1: None, 2: None, 6: (9598, 9598, 6786, -10, 3388, 3388)}
MAX_STREAMS = 65


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


def noise(n, n_in, ch, seed):
    """Full-scale noise [n, n_in, ch] with both extremes, every stream different."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (n, n_in, ch), dtype=np.int64).astype(np.int16)
    x[:, 3::97] = 32767
    x[:, 5::89] = -32768
    return x


def pack(x, layout, stride):
    """[n, n_in, ch] -> [n, stride] elements in `layout`, poison behind the n_in x ch elements."""
    n, n_in, ch = x.shape
    host = np.full((n, stride), POISON, dtype=np.int16)
    host[:, :n_in * ch] = (x if layout == M.INTERLEAVED else x.transpose(0, 2, 1)).reshape(n, -1)
    return host


def device_import(dec, x, r, o, layout, mix=None, first_in=0, state=None, sync=True):
    """One efx_import_pcm of x [n, n_in, ch] with padded strides.  Returns (samples [n, n_out], state [n, 128] int16) after
    checking that nothing but the samples was written."""
    n, n_in, ch = x.shape
    n_out = M.out_samples(r, o, first_in, n_in)
    ss, ds = r8(n_in * ch) + 8, r8(n_out) + 8
    d_src, d_dst, d_st = dec.alloc(2 * n * ss), dec.alloc(2 * n * ds), dec.alloc(n * M.STATE_BYTES)
    try:
        d_src.upload(pack(x, layout, ss))
        d_dst.upload(np.full(n * ds, CANARY, dtype=np.int16))
        d_st.upload(np.zeros((n, M.STATE_BYTES // 2), dtype=np.int16) if state is None else state)
        got = dec.import_pcm_to(d_src, d_st, d_dst, n_streams=n, n_in=n_in, in_rate=r, out_rate=o, channels=ch, layout=layout,
                                weights=mix, first_in=first_in, src_stride=ss, dst_stride=ds)
        assert got == n_out
        dec.sync()
        out = d_dst.download(np.int16, n * ds).reshape(n, ds)
        assert (out[:, n_out:] == CANARY).all(), "samples behind a stream's output were written"
        return out[:, :n_out], d_st.download(np.int16, n * M.STATE_BYTES // 2).reshape(n, -1)
    finally:
        for b in (d_src, d_dst, d_st):
            b.free()


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} samples differ, first (stream, sample) = {bad[0].tolist()}"


def frames_for(r, o, outputs):
    """The fewest input frames of a fresh stream that give at least `outputs` samples."""
    return (outputs - 1) * r // o + 1


@pytest.mark.parametrize("layout", [M.INTERLEAVED, M.PLANAR], ids=["interleaved", "planar"])
@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("r,o", M.RATE_PAIRS)
def test_matrix(dec, r, o, ch, layout):
    """1, 3 and 65 streams x calls of 1 frame, 2 W - 2 frames (shorter than the history), one tile + 1 and three tiles + 7
    samples: the model's samples and the model's history; canaries between the streams' outputs survive, poison behind
    the source elements changes nothing."""
    W = M.delay(r, o)
    sizes = [1, max(2 * W - 2, 2), frames_for(r, o, TILE + 1), frames_for(r, o, 3 * TILE + 7)]
    assert M.out_samples(r, o, 0, sizes[2]) > TILE and M.out_samples(r, o, 0, sizes[3]) >= 3 * TILE + 7 and sizes[3] <= 20000
    for n in (1, 3, MAX_STREAMS):
        for n_in in sizes:
            x = noise(n, n_in, ch, r + 31 * n + n_in)
            want, hist = M.import_pcm(x.reshape(n, -1), r, o, ch, M.INTERLEAVED, MIX[ch])
            got, state = device_import(dec, x, r, o, layout, MIX[ch])
            assert_same(got, want, f"{n} streams x {n_in} frames")
            if r != o:
                assert_same(state, M.state_bytes(hist), f"state, {n} streams x {n_in} frames")
            else:
                assert not state.any()
            if n > 1 and want.shape[1] > 8:
                assert len({w.tobytes() for w in want}) == n


@pytest.mark.parametrize("first_in", [0, BIG], ids=["fresh", "first_in_2^33+5"])
@pytest.mark.parametrize("r,o", M.RATE_PAIRS)
def test_pieces_are_one_call(dec, r, o, first_in):
    """The same input in one call and in pieces of 1, 5, 126, 127 and 1000 frames and the rest, the state carried on."""
    n, ch, total = 3, 2, 9000
    x = noise(n, total, ch, r + 1)
    want, hist = M.import_pcm(x.reshape(n, -1), r, o, ch, first_in=first_in)
    whole, st_whole = device_import(dec, x, r, o, M.INTERLEAVED, first_in=first_in)
    assert_same(whole, want, "one call")
    parts, state, at = [], None, 0
    for k in (1, 5, 126, 127, 1000, total - 1259):
        y, state = device_import(dec, x[:, at:at + k], r, o, M.PLANAR if k == 126 else M.INTERLEAVED, first_in=first_in + at,
                                 state=state)
        parts.append(y)
        at += k
    assert_same(np.concatenate(parts, axis=1), want, "pieces")
    if r != o:
        assert_same(state, M.state_bytes(hist), "state after the pieces")
        assert_same(st_whole, M.state_bytes(hist), "state after one call")


def test_queued_calls_keep_their_rates(dec):
    """Four calls with four rate pairs, channel counts and layouts queued back to back: each gives its own result."""
    jobs = [(44100, 48000, 2, M.INTERLEAVED, 3000), (96000, 48000, 6, M.PLANAR, 5000), (8000, 16000, 1, M.INTERLEAVED, 700),
            (48000, 48000, 2, M.PLANAR, 1500)]
    n, queued = 3, []
    for k, (r, o, ch, layout, n_in) in enumerate(jobs):
        x = noise(n, n_in, ch, 50 + k)
        n_out = M.out_samples(r, o, 0, n_in)
        ss, ds = r8(n_in * ch), r8(n_out)
        d_src, d_dst, d_st = dec.alloc(2 * n * ss), dec.alloc(2 * n * ds), dec.alloc(n * M.STATE_BYTES)
        d_src.upload(pack(x, layout, ss))
        d_st.upload(np.zeros(n * M.STATE_BYTES, dtype=np.uint8))
        queued.append((x, n_out, ds, d_src, d_dst, d_st))
    for (r, o, ch, layout, n_in), (x, n_out, ds, d_src, d_dst, d_st) in zip(jobs, queued):
        dec.import_pcm_to(d_src, d_st, d_dst, n_streams=n, n_in=n_in, in_rate=r, out_rate=o, channels=ch, layout=layout,
                          weights=MIX[ch])
    dec.sync()
    for (r, o, ch, layout, n_in), (x, n_out, ds, d_src, d_dst, d_st) in zip(jobs, queued):
        got = d_dst.download(np.int16, n * ds).reshape(n, ds)[:, :n_out]
        want, _ = M.import_pcm(x.reshape(n, -1), r, o, ch, M.INTERLEAVED, MIX[ch])
        assert_same(got, want, f"queued {r} -> {o}")
        for b in (d_src, d_dst, d_st):
            b.free()


def sbc_frames(efx, dec, pcm):
    """efx_sbc_encode (mono, 16 blocks, bitpool 28, fresh encoders) of [n, frames x 128] samples."""
    n, n_frames = pcm.shape[0], pcm.shape[1] // 128
    fb = efx.sbc_frame_bytes(16, 1, 28)
    d_pcm, d_st = dec.alloc(pcm.nbytes), dec.alloc(n * efx.sbc_enc_state_bytes())
    d_pcm.upload(pcm)
    d_st.upload(np.zeros(n * efx.sbc_enc_state_bytes(), dtype=np.uint8))
    stride = (n_frames * fb + 15) // 16 * 16
    d_fr = dec.alloc(n * stride)
    dec.sbc_encode_to(d_pcm, d_st, d_fr, n_streams=n, n_frames=n_frames, frame_stride=stride)
    dec.sync()
    out = d_fr.download(np.uint8, n * stride).reshape(n, stride)[:, :n_frames * fb].reshape(n, n_frames, fb)
    for b in (d_pcm, d_st, d_fr):
        b.free()
    return out


def padded_model(x, r, o, ch):
    """The model's samples of a fresh stream, zero-padded to whole SBC frames of 128."""
    want, _ = M.import_pcm(x.reshape(x.shape[0], -1), r, o, ch)
    out = np.zeros((x.shape[0], -(-want.shape[1] // 128) * 128), dtype=np.int16)
    out[:, :want.shape[1]] = want
    return out


def test_import_then_sbc_encode_without_a_sync(efx, dec):
    """import_pcm_to -> sbc_encode_to queued back to back: the frames are those of the model's samples."""
    n, r, o, ch, n_in = 3, 44100, 48000, 2, 8000
    x = noise(n, n_in, ch, 77) // 4
    want = padded_model(x, r, o, ch)
    n_frames, fb = want.shape[1] // 128, efx.sbc_frame_bytes(16, 1, 28)
    ss, stride = r8(n_in * ch), (n_frames * fb + 15) // 16 * 16
    d_src, d_ist, d_pcm = dec.alloc(2 * n * ss), dec.alloc(n * M.STATE_BYTES), dec.alloc(want.nbytes)
    d_st, d_fr = dec.alloc(n * efx.sbc_enc_state_bytes()), dec.alloc(n * stride)
    d_src.upload(pack(x, M.INTERLEAVED, ss))
    d_ist.upload(np.zeros(n * M.STATE_BYTES, dtype=np.uint8))
    d_pcm.upload(np.zeros_like(want))
    d_st.upload(np.zeros(n * efx.sbc_enc_state_bytes(), dtype=np.uint8))
    dec.import_pcm_to(d_src, d_ist, d_pcm, n_streams=n, n_in=n_in, in_rate=r, out_rate=o, channels=ch, dst_stride=want.shape[1])
    dec.sbc_encode_to(d_pcm, d_st, d_fr, n_streams=n, n_frames=n_frames, frame_stride=stride)
    dec.sync()
    got = d_fr.download(np.uint8, n * stride).reshape(n, stride)[:, :n_frames * fb].reshape(n, n_frames, fb)
    assert_same(d_pcm.download(np.int16, want.size).reshape(want.shape), want, "samples")
    for b in (d_src, d_ist, d_pcm, d_st, d_fr):
        b.free()
    assert np.array_equal(got, sbc_frames(efx, dec, want))


AV_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import import_pcm_model as M
    import test_gpu_import_pcm as T

    pics, pcm48, stereo = T.av_inputs()
    n = pics.shape[0]
    dec = efx.Decoder(n, 1, 2, device=torch.cuda.current_device())
    new, st = dec.encode_av(torch.from_numpy(pics).cuda(), torch.from_numpy(stereo).cuda(), qscale=6, gop=6, first_pts=T.PTS0,
                            pcm_rate=44100)
    assert (st == 0).all()
    planar, st = dec.encode_av(pics, np.ascontiguousarray(stereo.transpose(0, 2, 1)), qscale=6, gop=6, first_pts=T.PTS0,
                               pcm_rate=44100, pcm_layout="planar")
    assert (st == 0).all() and planar == new
    old, st = dec.encode_av(torch.from_numpy(pics).cuda(), torch.from_numpy(pcm48).cuda(), qscale=6, gop=6, first_pts=T.PTS0)
    assert (st == 0).all()
    video = dec.encode(torch.from_numpy(pics).cuda(), qscale=6, gop=6, first_pts=T.PTS0).streams
    frames48 = dec.sbc_encode(pcm48).cpu().numpy()

    # Decoder.import_pcm: arrays and tensors, one call and continued calls, flush
    want, _ = M.import_pcm(stereo.reshape(n, -1), 44100, 48000, 2)
    got = dec.import_pcm(stereo, rate=44100)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int16 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    t = torch.from_numpy(stereo).cuda()
    a = dec.import_pcm(t[:, :1001], rate=44100)
    b = dec.import_pcm(t[:, 1001:], rate=44100, cont=True, flush=True)
    W = efx.import_pcm_delay(44100, 48000)
    flushed, _ = M.import_pcm(np.concatenate([stereo, np.zeros((n, W, 2), dtype=np.int16)], axis=1).reshape(n, -1), 44100, 48000, 2)
    assert np.array_equal(torch.cat([a, b], dim=1).cpu().numpy(), flushed) and flushed.shape[1] > want.shape[1]
    mono = np.ascontiguousarray(stereo[:, :, 0])
    assert np.array_equal(dec.import_pcm(mono, rate=96000, out_rate=32000).cpu().numpy(), M.import_pcm(mono, 96000, 32000, 1)[0])
    pl = dec.import_pcm(np.ascontiguousarray(stereo.transpose(0, 2, 1)), rate=44100, layout="planar", weights=(20000, -12768))
    assert np.array_equal(pl.cpu().numpy(), M.import_pcm(stereo.reshape(n, -1), 44100, 48000, 2, mix=(20000, -12768))[0])
    try:
        dec.import_pcm(stereo, rate=22050, cont=True)
        raise SystemExit("cont with other rates was accepted")
    except efx.EfxError:
        pass
    pickle.dump((new, old, video, frames48), open(sys.argv[2], "wb"))
    dec.close()
    print("import_pcm av ok")
""")
PTS0 = 129003


def av_inputs():
    """Two streams of six pictures with 0.2 s of sound: 48 kHz mono (whole frames) and 44.1 kHz stereo."""
    import encode_model as E
    n, P = 2, 6
    pics = np.stack([E.moving(P, seed=30 + i) for i in range(n)])
    t48 = np.arange(75 * 128)
    pcm48 = np.stack([np.round(9000 * np.sin(2 * np.pi * (440 + 110 * i) * t48 / 48000)) for i in range(n)]).astype(np.int16)
    t44 = np.arange(8820)
    rng = np.random.default_rng(8)
    stereo = np.stack([np.stack([np.round(9000 * np.sin(2 * np.pi * (440 + 110 * i) * t44 / 44100)),
                                 np.round(7000 * np.sin(2 * np.pi * 1000 * t44 / 44100)) + rng.integers(-300, 300, t44.size)], axis=-1)
                       for i in range(n)]).astype(np.int16)
    return pics, pcm48, stereo


def test_encode_av_with_pcm_rate(efx, tmp_path):
    """encode_av(pcm_rate=44100, stereo): the title is the multiplex of encode()'s video with the SBC frames of the model's
    samples, and its audio payload through efx_demux_audio is those frames; without the new arguments encode_av gives the
    bytes it gave before.  Decoder.import_pcm in the same child process (tensors: torch's HIP runtime first)."""
    import mux_model as X
    script, out = tmp_path / "import_pcm_av.py", tmp_path / "titles.pkl"
    script.write_text(AV_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "import_pcm av ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    new, old, video, frames48 = pickle.load(open(out, "rb"))
    pics, pcm48, stereo = av_inputs()
    n = pics.shape[0]
    d = efx.Decoder(n, 1, 2, max_stream_bytes=sum(len(t) for t in new) + 8192)
    want = sbc_frames(efx, d, padded_model(stereo, 44100, 48000, 2))
    n_frames, fb = want.shape[1], want.shape[2]
    assert n_frames == 75 and fb == 64
    arrs = [np.frombuffer(t, dtype=np.uint8) for t in new]
    stride = (max(a.size for a in arrs) + 15) // 16 * 16
    d_au, d_len = d.alloc(n * stride), d.alloc(4 * n)
    d.demux_audio(arrs, d_au, stride, d_len)
    d.sync()
    assert (d_len.download(np.uint32, n) == n_frames * fb).all()
    audio = d_au.download(np.uint8, n * stride).reshape(n, stride)[:, :n_frames * fb].reshape(n, n_frames, fb)
    d.close()
    assert np.array_equal(audio, want)
    for i in range(n):
        v = np.frombuffer(video[i], dtype=np.uint8)
        assert new[i] == X.mux(v, want[i].reshape(-1), frame_bytes=fb, first_pts=PTS0)[0], i
        assert old[i] == X.mux(v, frames48[i].reshape(-1), frame_bytes=fb, first_pts=PTS0)[0], i


def test_argument_errors(efx, dec):
    lib, ctx = dec._lib, dec._ctx
    src, st, dst = dec.alloc(1 << 16), dec.alloc(4 * 256), dec.alloc(1 << 16)
    good = dict(n_streams=2, n_in=1000, in_rate=44100, out_rate=48000, channels=2, layout=efx.PCM_INTERLEAVED, mix=(0,) * 8,
                first_in=0, src_stride=2000, dst_stride=1096)

    def call(s=src.ptr, t=st.ptr, d=dst.ptr, **change):
        a = dict(good, **change)
        o = efx._ImportPcmOpts(a["n_streams"], a["n_in"], a["in_rate"], a["out_rate"], a["channels"], a["layout"],
                               (C.c_int * 8)(*a["mix"]), a["first_in"], a["src_stride"], a["dst_stride"])
        return lib.efx_import_pcm(ctx, C.byref(o), s, t, d)

    assert call() == 0 and M.out_samples(44100, 48000, 0, 1000) == 1089
    assert lib.efx_import_pcm(ctx, None, src.ptr, st.ptr, dst.ptr) == ARG
    # pointers: NULL, misaligned; the state may only be missing when the rates are equal
    assert call(s=None) == ARG and call(t=None) == ARG and call(d=None) == ARG
    assert call(s=src.ptr + 8) == ARG and call(t=st.ptr + 4) == ARG and call(d=dst.ptr + 2) == ARG
    assert call(t=None, in_rate=48000, dst_stride=1000) == 0 and call(t=st.ptr + 4, in_rate=48000, dst_stride=1000) == ARG
    # fields out of range
    assert call(n_streams=0) == ARG and call(n_streams=MAX_STREAMS + 1) == ARG and call(n_streams=-1) == ARG
    assert call(n_in=0) == ARG and call(n_in=-5) == ARG
    assert call(in_rate=7999) == ARG and call(in_rate=192001) == ARG and call(in_rate=8000, dst_stride=6000) == 0
    assert call(in_rate=192000, dst_stride=256) == 0 and call(in_rate=64001, out_rate=16000) == ARG
    assert call(in_rate=64000, out_rate=16000) == 0
    assert call(out_rate=22050) == ARG and call(out_rate=0) == ARG and call(out_rate=96000) == ARG
    for o in M.OUT_RATES:
        assert call(out_rate=o) == 0
    assert call(channels=0) == ARG and call(channels=9) == ARG and call(channels=8, src_stride=8000) == 0
    assert call(layout=0) == ARG and call(layout=3) == ARG and call(layout=efx.PCM_PLANAR) == 0
    # the weights: sum of |w| over the channels
    assert call(mix=(16384, -16384, 0, 0, 0, 0, 0, 0)) == 0 and call(mix=(16384, -16385, 0, 0, 0, 0, 0, 0)) == ARG
    assert call(mix=(32769, 0, 0, 0, 0, 0, 0, 0)) == ARG and call(mix=(-(1 << 31), 0, 0, 0, 0, 0, 0, 0)) == ARG
    assert call(mix=(16384, 16384, 99999, 0, 0, 0, 0, 0)) == 0  # (behind the channels: not a weight)
    # first_in
    assert call(first_in=-1) == ARG and call(first_in=1 << 40) == ARG and call(first_in=(1 << 40) - 1) == 0
    # strides: too small, not a multiple of 8
    assert call(src_stride=1992) == ARG and call(src_stride=2004) == ARG and call(src_stride=2008) == 0
    assert call(dst_stride=1088) == ARG and call(dst_stride=1092) == ARG and call(dst_stride=1104) == 0
    assert call(n_in=1001, src_stride=2000) == ARG
    dec.sync()
    for b in (src, st, dst):
        b.free()
    with pytest.raises(efx.EfxError) as e:
        dec.import_pcm_to(0, 0, 0, n_streams=1, n_in=10, in_rate=44100)
    assert e.value.status == ARG
