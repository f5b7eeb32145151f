"""efx_limit_peaks / efx_pcm_limit (k_limit.hip): the look-ahead peak limiter on the device, every result bit for bit against
the NumPy model of include/efx.h's rule (tests/limit_model.py); pieces against one call; normalize(limiter=True) and
encode_av(loudness=, limiter=True) in a child process."""
import functools
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import limit_model as M
import loudness_model as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
POISON, CANARY = 0x5A5B, 0xABCD
MAX_STREAMS = 65
C_M1 = 29204
# gated_mean, n_gated of the records the limit tests hand out, stream i taking entry (i + 1) % 4: G of about 4096, 10000, 32767 (the
# clamp) and the 4096 of a stream nothing of which passed the gates
REC_KINDS = ((10 ** 13, 5), (17 * 10 ** 11, 9), (10 ** 11, 1), (5, 0))


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


def lengths(rate):
    """1, 7, 15, 16, 17 and a workgroup's tile of blocks +- 1 sample."""
    t = M.BLOCK[rate] * M.TILE
    return (1, 7, 15, 16, 17, t - 1, t, t + 1)


@functools.lru_cache(maxsize=None)
def signal(n, samples, rate, seams=False):
    """[n, samples] int16, every stream different: quiet noise with lone samples of both extremes (stream 1: none, its
    gain is never reduced; stream 2: full-scale noise); seams: full scale on both sides of every tile seam."""
    rng = np.random.default_rng(100 * n + samples + rate)
    x = rng.integers(-900, 901, (n, samples), dtype=np.int64)
    hit = rng.random((n, samples))
    x[hit < 0.002] = 32767
    x[hit > 0.998] = -32768
    if n > 1:
        x[1] = rng.integers(-900, 901, samples)
    if n > 2:
        x[2] = rng.integers(-32768, 32768, samples)
    if seams:
        t = M.BLOCK[rate] * M.TILE
        for s in range(t, samples, t):
            x[:, s - 1] = -32768
            x[:, s] = 32767
    x = x.astype(np.int16)
    x.setflags(write=False)
    return x


def records(n, rate):
    """(REC_DTYPE [n], G [n]) with the target of -23 LUFS."""
    recs = np.zeros(n, dtype=L.REC_DTYPE)
    T = L.thresholds(rate)[1]
    for i in range(n):
        recs["gated_mean"][i], recs["n_gated"][i] = REC_KINDS[(i + 1) % 4]
    recs["gain_q12"] = 77  # (the capped gain of the record is not what the limiter reads)
    return recs, [M.stream_gain(int(r["gated_mean"]), int(r["n_gated"]), T, L.step_of(rate)) for r in recs]


def device_peaks(dec, x, rate, first_block=0, peaks_first=0):
    """efx_limit_peaks over x [n, samples] as a piece that begins at block first_block; returns the rows' entries of the
    piece after checking the guards around them and the samples."""
    n, samples = x.shape
    bk = M.BLOCK[rate]
    nb, e0 = -(-samples // bk), first_block - peaks_first
    ps, stride = e0 + nb + 5, r8(samples) + 8
    host = np.full((n, stride), POISON, dtype=np.int16)  # poison behind every stream's samples: read, it would be a peak
    host[:, :samples] = x
    d_pcm, d_pk = dec.alloc(host.nbytes), dec.alloc(2 * n * ps)
    try:
        d_pcm.upload(host)
        d_pk.upload(np.full(n * ps, CANARY, dtype=np.uint16))
        dec.limit_peaks_to(d_pcm, d_pk, n_streams=n, n_samples=samples, rate=rate, first_sample=first_block * bk, peaks_first=peaks_first,
                           pcm_stride=stride, peaks_stride=ps)
        dec.sync()
        rows = d_pk.download(np.uint16, n * ps).reshape(n, ps)
        assert (rows[:, :e0] == CANARY).all() and (rows[:, e0 + nb:] == CANARY).all(), "entries outside the piece's were written"
        assert np.array_equal(d_pcm.download(np.int16, host.size).reshape(host.shape), host), "the samples were written"
        return rows[:, e0:e0 + nb]
    finally:
        d_pcm.free()
        d_pk.free()


def device_limit(dec, x, rate, H, C, *, recs=None, fixed=4096, in_place=False, half_window=None):
    """peaks -> limit over whole streams x [n, samples], padded strides; returns y [n, samples] after checking the padding
    of the destination (and the source, out of place)."""
    n, samples = x.shape
    nb = -(-samples // M.BLOCK[rate])
    stride, ds, ps = r8(samples) + 8, r8(samples) + 16, nb + 3
    host = np.full((n, stride), POISON, dtype=np.int16)
    host[:, :samples] = x
    d_src, d_dst, d_pk = dec.alloc(host.nbytes), dec.alloc(2 * n * ds), dec.alloc(2 * n * ps)
    d_recs = dec.alloc(32 * n) if recs is not None else None
    try:
        d_src.upload(host)
        d_dst.upload(np.full(n * ds, POISON + 1, dtype=np.int16))
        d_pk.upload(np.full(n * ps, 60000, dtype=np.uint16))  # (entries behind n_peaks: read, they would silence the end)
        if recs is not None:
            d_recs.upload(recs)
        dst, dst_stride = (d_src, stride) if in_place else (d_dst, ds)
        dec.limit_peaks_to(d_src, d_pk, n_streams=n, n_samples=samples, rate=rate, pcm_stride=stride, peaks_stride=ps)
        dec.pcm_limit_to(d_src, d_pk, d_recs, dst, n_streams=n, n_samples=samples, rate=rate, n_peaks=nb,
                         half_window=H if half_window is None else half_window, thresholds=(0, L.thresholds(rate)[1], C),
                         fixed_gain_q12=fixed, src_stride=stride, dst_stride=dst_stride, peaks_stride=ps)
        dec.sync()
        out = dst.download(np.int16, n * dst_stride).reshape(n, dst_stride)
        assert (out[:, samples:] == (POISON if in_place else POISON + 1)).all(), "samples behind a stream's were written"
        if not in_place:
            assert np.array_equal(d_src.download(np.int16, host.size).reshape(host.shape), host), "the source was written"
        return out[:, :samples]
    finally:
        for b in (d_src, d_dst, d_pk, d_recs):
            if b is not None:
                b.free()


def assert_streams(got, x, rate, gains, C, H, what):
    for i in range(x.shape[0]):
        want = M.limit(x[i], rate, gains[i], C, H)
        bad = np.flatnonzero(got[i] != want)
        assert bad.size == 0, f"{what}, stream {i} (G {gains[i]}): {bad.size} samples differ, first at {bad[:3]}"


# ---- efx_limit_peaks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("rate", [16000, 44100])
def test_peaks(dec, rate, n):
    for samples in lengths(rate):
        x = signal(n, samples, rate)
        want = np.stack([M.peaks(x[i], rate) for i in range(n)])
        assert np.array_equal(device_peaks(dec, x, rate), want), samples
        assert np.array_equal(device_peaks(dec, x, rate, first_block=5, peaks_first=2), want), samples
    full = np.full((n, 3 * M.BLOCK[rate]), -32768, dtype=np.int16)
    full[:, M.BLOCK[rate]:] = 32767
    assert device_peaks(dec, full, rate, first_block=9, peaks_first=9).tolist() == [[32768, 32767, 32767]] * n


# ---- efx_pcm_limit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("H", [1, 32, 64])
@pytest.mark.parametrize("rate", [16000, 44100])
def test_limit(dec, rate, H, n):
    """The shapes of test_peaks: 1, 3 and 65 streams at every length, gains from records (stream i's is kind (i + 1) % 4:
    three streams have the one with n_gated = 0) and C = 29204, out of place and in place; then, at 17 samples and at a
    tile and a sample, C = 1 and fixed gains."""
    t = M.BLOCK[rate] * M.TILE
    recs, gains = records(n, rate)
    assert n < 3 or (len(set(gains)) >= 3 and 4096 in gains and 32767 in gains)
    for samples in lengths(rate):
        x = signal(n, samples, rate)
        want = np.stack([M.limit(x[i], rate, gains[i], C_M1, H) for i in range(n)])
        for in_place in (False, True):
            got = device_limit(dec, x, rate, H, C_M1, recs=recs, in_place=in_place)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{samples} samples, in place {in_place}: {len(bad)} samples differ, first (stream, sample) {bad[:3].tolist()}"
    for samples in (17, t + 1):
        x = signal(n, samples, rate)
        assert_streams(device_limit(dec, x, rate, H, 1, recs=recs), x, rate, gains, 1, H, f"{samples}, C = 1")
        for fixed in (1, 7001, 32767):
            got = device_limit(dec, x, rate, H, C_M1, fixed=fixed, in_place=fixed == 7001)
            assert_streams(got, x, rate, [fixed] * n, C_M1, H, f"{samples}, fixed gain {fixed}")
            # the stream without loud samples (900 G <= 4096 C for every G): efx_pcm_gain's output, bit for bit
            if n > 1:
                assert np.array_equal(got[1], L.apply_gain(x[1], fixed))


@pytest.mark.parametrize("H", [1, 32, 64])
def test_limit_across_tile_seams(dec, H):
    """Three tiles and a ragged fourth with full-scale samples on both sides of every seam."""
    rate = 16000
    samples = 3 * M.BLOCK[rate] * M.TILE + 37
    x = signal(3, samples, rate, seams=True)
    recs, gains = records(3, rate)
    for in_place in (False, True):
        got = device_limit(dec, x, rate, H, C_M1, recs=recs, in_place=in_place)
        assert_streams(got, x, rate, gains, C_M1, H, f"seams, in place {in_place}")
        assert np.abs(got.astype(np.int64)).max() <= C_M1


def test_limit_48k_and_default_window(dec):
    rate, samples = 48000, 48 * M.TILE + 49
    x = signal(3, samples, rate, seams=True)
    recs, gains = records(3, rate)
    assert_streams(device_limit(dec, x, rate, 32, C_M1, recs=recs, half_window=0), x, rate, gains, C_M1, 32, "48 kHz, half_window 0")
    x = signal(2, 700, 32000)
    assert_streams(device_limit(dec, x, 32000, 5, C_M1, fixed=20000), x, 32000, [20000] * 2, C_M1, 5, "32 kHz")


# ---- pieces ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [16000, 44100])
def test_pieces_queued_back_to_back_equal_one_call(dec, rate):
    """Three pieces of a 700-block stream, the last ragged: six launches queued without a synchronise, the peaks in one
    row per stream; then the middle piece again with a row that holds little more than its halo."""
    bk, H, n = M.BLOCK[rate], 32, 3
    samples = 699 * bk + 5
    cuts = (0, 300, 556, 700)
    x = signal(n, samples, rate, seams=True)
    recs, gains = records(n, rate)
    stride, ps = r8(samples) + 8, 704
    host = np.full((n, stride), POISON, dtype=np.int16)
    host[:, :samples] = x
    d_src, d_dst, d_pk, d_recs, d_mid = dec.alloc(host.nbytes), dec.alloc(host.nbytes), dec.alloc(2 * n * ps), dec.alloc(32 * n), dec.alloc(host.nbytes)
    try:
        d_src.upload(host)
        d_dst.upload(np.full(host.size, POISON + 1, dtype=np.int16))
        d_mid.upload(np.full(host.size, POISON + 2, dtype=np.int16))
        d_pk.upload(np.full(n * ps, CANARY, dtype=np.uint16))
        d_recs.upload(recs)
        thr = (0, L.thresholds(rate)[1], C_M1)
        spans = [(b0 * bk, min(b1 * bk, samples) - b0 * bk) for b0, b1 in zip(cuts, cuts[1:])]
        for first, count in spans:
            dec.limit_peaks_to(d_src.ptr + 2 * first, d_pk, n_streams=n, n_samples=count, rate=rate, first_sample=first, pcm_stride=stride,
                               peaks_stride=ps)
        for first, count in spans:
            dec.pcm_limit_to(d_src.ptr + 2 * first, d_pk, d_recs, d_dst.ptr + 2 * first, n_streams=n, n_samples=count, rate=rate, n_peaks=700,
                             half_window=H, first_sample=first, thresholds=thr, src_stride=stride, dst_stride=stride, peaks_stride=ps)
        pf = 232  # a multiple of 8 (the row's pointer stays aligned) at or below 300 - 2H - 1
        first, count = spans[1]
        dec.pcm_limit_to(d_src.ptr + 2 * first, d_pk.ptr + 2 * pf, d_recs, d_mid.ptr + 2 * first, n_streams=n, n_samples=count, rate=rate,
                         n_peaks=556 + 2 * H + 1 - pf, half_window=H, first_sample=first, peaks_first=pf, thresholds=thr, src_stride=stride,
                         dst_stride=stride, peaks_stride=ps)
        dec.sync()
        rows = d_pk.download(np.uint16, n * ps).reshape(n, ps)
        assert np.array_equal(rows[:, :700], np.stack([M.peaks(x[i], rate) for i in range(n)])) and (rows[:, 700:] == CANARY).all()
        out = d_dst.download(np.int16, host.size).reshape(host.shape)
        assert (out[:, samples:] == POISON + 1).all()
        assert_streams(out[:, :samples], x, rate, gains, C_M1, H, "three pieces")
        mid = d_mid.download(np.int16, host.size).reshape(host.shape)
        assert np.array_equal(mid[:, first:first + count], out[:, first:first + count]), "the middle piece from its halo"
        assert (mid[:, :first] == POISON + 2).all() and (mid[:, first + count:] == POISON + 2).all()
    finally:
        for b in (d_src, d_dst, d_pk, d_recs, d_mid):
            b.free()


# ---- Decoder.limit / normalize(limiter=True) / encode_av(loudness=, limiter=True) -----------------------------------------------
PTS0 = 129003


def av_pcm():
    """Two streams of 2 s at 48 kHz in whole SBC frames: noise and a tone at about -31 LUFS, stream 0 with a 2 ms burst
    near full scale, stream 1 without (its peak cap does not bind)."""
    n = 750 * 128
    t = np.arange(n) / 48000
    rng = np.random.default_rng(1)
    x = np.stack([rng.normal(0, 400, n) + 800 * np.sin(2 * np.pi * 440 * t) for _ in range(2)])
    for s in (0.9,):
        i0, i1 = int(s * 48000), int((s + 0.002) * 48000)
        x[0, i0:i1] += 31000 * np.sin(2 * np.pi * 1000 * t[i0:i1])
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


AV_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import limit_model as M
    import test_gpu_limit as T
    import test_gpu_loudness as TL

    title = np.stack([M.peaky_title(16000), M.peaky_title(16000) // 40])
    pics, _ = TL.av_inputs()
    pcm = T.av_pcm()
    dec = efx.Decoder(3, 1, 2, device=torch.cuda.current_device())
    out = {}
    out["norm_plain"], out["res_plain"] = dec.normalize(title, 16000)
    out["norm_lim"], out["res_lim"] = dec.normalize(title, 16000, limiter=True)
    out["norm_lim_h5"], _ = dec.normalize(torch.from_numpy(title).cuda(), 16000, limiter=True, half_window=5, target=-20.0, peak=-3.0)
    out["norm_lim_h5"] = out["norm_lim_h5"].cpu().numpy()
    out["limit"] = dec.limit(title, 16000, gain_q12=9000, peak=-2.0, half_window=7)
    p, a = torch.from_numpy(pics).cuda(), torch.from_numpy(pcm).cuda()
    kw = dict(qscale=6, gop=6, first_pts=T.PTS0)
    out["plain"], st0 = dec.encode_av(p, a, **kw)
    out["off"], st1 = dec.encode_av(p, a, limiter=False, half_window=9, **kw)
    out["lim_no_loudness"], st2 = dec.encode_av(p, a, limiter=True, **kw)
    out["level"], st3 = dec.encode_av(p, a, loudness=-23.0, **kw)
    out["level_off"], st4 = dec.encode_av(p, a, loudness=-23.0, limiter=False, **kw)
    out["level_lim"], st5 = dec.encode_av(p, a, loudness=-23.0, limiter=True, **kw)
    assert all((s == 0).all() for s in (st0, st1, st2, st3, st4, st5))
    assert np.array_equal(a.cpu().numpy(), pcm)  # the caller's tensor is not scaled

    def decoded(titles):
        arrs = [np.frombuffer(t, dtype=np.uint8) for t in titles]
        n, fb, n_frames = len(arrs), efx.sbc_frame_bytes(16, 1, 28), pcm.shape[1] // 128
        stride = (max(a.size for a in arrs) + 15) // 16 * 16
        d = efx.Decoder(n, 1, 2, device=torch.cuda.current_device(), max_stream_bytes=3 * sum(a.size for a in arrs) + 4096 * n)
        d_au, d_len = d.alloc(n * stride), d.alloc(4 * n)
        d.demux_audio(arrs, d_au, stride, d_len)
        assert (d_len.download(np.uint32, n) == n_frames * fb).all()
        d_st, d_out, d_cnt = d.alloc(n * efx.sbc_state_bytes()), d.alloc(n * n_frames * 256), d.alloc(4 * n)
        d_st.upload(np.zeros(n * efx.sbc_state_bytes(), dtype=np.uint8))
        d.sbc_decode(n, d_au, stride, fb, n_frames, d_st, d_out, n_frames * 128, None, d_cnt)
        d.sync()
        got = d_out.download(np.int16, n * n_frames * 128).reshape(n, -1)
        d.close()
        return got

    out["pcm_level"], out["pcm_level_lim"] = decoded(out["level"]), decoded(out["level_lim"])
    pickle.dump(out, open(sys.argv[2], "wb"))
    dec.close()
    print("limit av ok")
""")


def test_normalize_and_encode_av_with_the_limiter(tmp_path):
    """In a child process (tensors: torch's HIP runtime first).  normalize(limiter=True) on the peaky test title (12.3 s at 16 kHz)
    and on a copy 32 dB quieter, whose cap does not bind; Decoder.limit; encode_av with and without the keywords."""
    script, path = tmp_path / "limit_av.py", tmp_path / "out.pkl"
    script.write_text(AV_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "limit av ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    o = pickle.load(open(path, "rb"))
    rate = 16000
    title = np.stack([M.peaky_title(rate), M.peaky_title(rate) // 40])
    for key, target, peak, H in (("norm_lim", -23.0, -1.0, 32), ("norm_lim_h5", -20.0, -3.0, 5)):
        thr = L.thresholds(rate, target, peak)
        for i in range(2):
            rec, _ = L.measure(title[i], rate, target, peak)
            G = M.stream_gain(int(rec["gated_mean"]), int(rec["n_gated"]), thr[1], L.step_of(rate))
            assert np.array_equal(o[key][i], M.limit(title[i], rate, G, thr[2], H)), (key, i)
            if key == "norm_lim":
                assert o["res_lim"].gain_q12[i] == o["res_plain"].gain_q12[i] == rec["gain_q12"]  # the record's capped gain
                assert (G > rec["gain_q12"]) == (i == 0)
    assert np.array_equal(o["norm_lim"][1], o["norm_plain"][1]) and not np.array_equal(o["norm_lim"][0], o["norm_plain"][0])
    before, plain, lim = (L.measure(v, rate)[1] for v in (title[0], o["norm_plain"][0], o["norm_lim"][0]))
    print(f"normalize: {before:.2f} LUFS -> {plain:.2f} linear, {lim:.2f} limited")
    assert abs(lim + 23.0) < abs(plain + 23.0) and abs(lim + 23.0) < 2.0
    C2 = L.thresholds(rate, -23.0, -2.0)[2]
    for i in range(2):
        assert np.array_equal(o["limit"][i], M.limit(title[i], rate, 9000, C2, 7))
    # encode_av: without the keyword, with it off, and with it but without loudness=: the bytes of before
    assert o["off"] == o["plain"] and o["lim_no_loudness"] == o["plain"] and o["level_off"] == o["level"]
    assert o["level_lim"][0] != o["level"][0] and o["level_lim"][1] == o["level"][1]  # (stream 1: the cap does not bind)
    a, b = L.measure(o["pcm_level"][0], 48000)[1], L.measure(o["pcm_level_lim"][0], 48000)[1]
    print(f"encode_av: decoded title at {a:.2f} LUFS with loudness=-23, {b:.2f} LUFS with limiter=True")
    assert abs(b + 23.0) < abs(a + 23.0)


# ---- arguments ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(efx, dec):
    lib, ctx = dec._lib, dec._ctx
    pcm, pk, recs, dst = dec.alloc(2 * 2 * 1608), dec.alloc(2 * 2 * 112), dec.alloc(64), dec.alloc(2 * 2 * 1608)
    try:
        recs.upload(np.zeros(2, dtype=L.REC_DTYPE))

        def peaks_call(p=pcm.ptr, k=pk.ptr, **kw):
            a = dict(n_streams=2, n_samples=1600, rate=16000, reserved=0, first_sample=0, peaks_first=0, pcm_stride=1600, peaks_stride=100)
            a.update(kw)
            o = np.zeros(1, dtype=efx.LIMIT_PEAKS_OPTS_DTYPE)
            o[0] = tuple(a.values())
            return lib.efx_limit_peaks(ctx, o.ctypes.data, p, k)

        assert peaks_call() == 0 and peaks_call(n_samples=1593) == 0 and peaks_call(pcm_stride=1608) == 0
        assert lib.efx_limit_peaks(ctx, None, pcm.ptr, pk.ptr) == ARG
        assert peaks_call(rate=22050) == ARG and peaks_call(rate=0) == ARG
        assert peaks_call(p=None) == ARG and peaks_call(k=None) == ARG and peaks_call(p=pcm.ptr + 8) == ARG and peaks_call(k=pk.ptr + 2) == ARG
        assert peaks_call(n_streams=0) == ARG and peaks_call(n_streams=MAX_STREAMS + 1) == ARG
        assert peaks_call(n_samples=0) == ARG and peaks_call(n_samples=-16) == ARG
        assert peaks_call(first_sample=-16) == ARG and peaks_call(first_sample=8) == ARG and peaks_call(first_sample=1 << 40) == ARG
        assert peaks_call(first_sample=160, peaks_stride=110) == 0 and peaks_call(first_sample=160, peaks_stride=109) == ARG
        assert peaks_call(first_sample=160, peaks_first=10) == 0 and peaks_call(first_sample=160, peaks_first=11) == ARG
        assert peaks_call(peaks_first=-1) == ARG
        assert peaks_call(pcm_stride=1592) == ARG and peaks_call(pcm_stride=1604) == ARG and peaks_call(peaks_stride=99) == ARG
        assert peaks_call(rate=48000, first_sample=16) == ARG and peaks_call(rate=48000, first_sample=48, n_samples=1500) == 0

        thr = L.thresholds(16000)

        def limit_call(s=pcm.ptr, k=pk.ptr, r=None, d=dst.ptr, **kw):
            a = dict(n_streams=2, n_samples=1600, rate=16000, half_window=32, ceiling=thr[2], fixed_gain_q12=4096, n_peaks=100, reserved=0,
                     first_sample=0, peaks_first=0, target_ms=thr[1], src_stride=1600, dst_stride=1608, peaks_stride=100)
            a.update(kw)
            o = np.zeros(1, dtype=efx.LIMIT_OPTS_DTYPE)
            o[0] = tuple(a.values())
            return lib.efx_pcm_limit(ctx, o.ctypes.data, s, k, r, d)

        assert limit_call() == 0 and limit_call(r=recs.ptr) == 0 and limit_call(d=pcm.ptr, dst_stride=1600) == 0
        assert lib.efx_pcm_limit(ctx, None, pcm.ptr, pk.ptr, None, dst.ptr) == ARG
        assert limit_call(rate=8000) == ARG and limit_call(rate=44101) == ARG
        assert limit_call(s=None) == ARG and limit_call(k=None) == ARG and limit_call(d=None) == ARG
        assert limit_call(s=pcm.ptr + 2) == ARG and limit_call(k=pk.ptr + 8) == ARG and limit_call(d=dst.ptr + 8) == ARG
        assert limit_call(r=recs.ptr + 8) == ARG and limit_call(r=recs.ptr + 16) == 0
        assert limit_call(n_streams=0) == ARG and limit_call(n_streams=MAX_STREAMS + 1) == ARG
        assert limit_call(n_samples=0) == ARG and limit_call(n_samples=-1) == ARG
        assert limit_call(half_window=-1) == ARG and limit_call(half_window=65) == ARG and limit_call(half_window=64) == 0
        assert limit_call(half_window=0) == 0 and limit_call(half_window=1) == 0
        assert limit_call(ceiling=0) == ARG and limit_call(ceiling=32768) == ARG and limit_call(ceiling=1) == 0
        assert limit_call(fixed_gain_q12=0) == ARG and limit_call(fixed_gain_q12=32768) == ARG and limit_call(r=recs.ptr, fixed_gain_q12=0) == 0
        assert limit_call(r=recs.ptr, target_ms=1 << 40) == ARG and limit_call(target_ms=1 << 40) == 0
        assert limit_call(n_peaks=0) == ARG and limit_call(n_peaks=101) == ARG and limit_call(n_peaks=1) == 0
        assert limit_call(first_sample=-16) == ARG and limit_call(first_sample=24) == ARG and limit_call(first_sample=1 << 40) == ARG
        assert limit_call(first_sample=1 << 30) == 0 and limit_call(peaks_first=-1) == ARG and limit_call(peaks_first=1 << 40) == ARG
        assert limit_call(peaks_first=5000) == 0
        assert limit_call(src_stride=1592) == ARG and limit_call(src_stride=1604) == ARG and limit_call(dst_stride=1592) == ARG
        assert limit_call(dst_stride=1604) == ARG and limit_call(peaks_stride=99) == ARG
        assert limit_call(d=pcm.ptr, dst_stride=1608) == ARG and limit_call(d=pcm.ptr, src_stride=1608, dst_stride=1608) == 0  # in place
        dec.sync()
        with pytest.raises(efx.EfxError) as e:
            dec.pcm_limit_to(pcm, pk, None, dst, n_streams=2, n_samples=1600, rate=16000, n_peaks=100, half_window=70)
        assert e.value.status == ARG
        with pytest.raises(efx.EfxError) as e:
            dec.limit_peaks_to(pcm, pk, n_streams=2, n_samples=1600, rate=11025)
        assert e.value.status == ARG
    finally:
        for b in (pcm, pk, recs, dst):
            b.free()
