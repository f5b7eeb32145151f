"""efx_mux_av (k_mux.hip) on the device against tests/mux_model.py, and the whole chain pictures + PCM -> efx_encode ->
efx_sbc_encode -> efx_mux_av -> a title that the library, the test oracle and (where built) the unmodified reference
player all play."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import encode_model as E
import export_model as XM
import mux_model as X
import oracle
import sbc_encode_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = 64
PTS0 = 129003


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def videos(clips, tmp_path_factory):
    exe = E.build(str(tmp_path_factory.mktemp("enc_model")))
    enc, _ = E.encode(exe, E.moving(24), gop=12, qscale=6, search=7, fmt=1, first_pts=9000)
    enc = np.frombuffer(enc, dtype=np.uint8).copy()
    splash = X.video_only(clips["splash"])
    units = X.video_units(splash)
    return [splash, X.video_only(clips["vmedia"]), enc, splash[:units[40][0] * 188].copy(), enc[:0].copy()]


def r16(v):
    return (v + 15) // 16 * 16


def prepare_mux(efx, dec, videos, frames, dst_stride=None, frame_bytes=FB, **opt):
    """videos: list of uint8 arrays; frames [n, n_frames x frame_bytes].  Allocates and uploads the buffers of one efx_mux_av
    (every upload synchronises the library's stream first: efx_memcpy_h2d) and returns what launch_mux and collect_mux need."""
    n = len(videos)
    n_frames = frames.shape[1] // frame_bytes
    v_stride, a_stride = r16(max(1, max(v.size for v in videos))) + 16, r16(max(1, frames.shape[1])) + 16
    fpp = opt.get("frames_per_pes", 8)
    stride = dst_stride or efx.mux_bound(v_stride, n_frames, frame_bytes, fpp)
    host_v = np.full((n, v_stride), 0xEE, dtype=np.uint8)
    for i, v in enumerate(videos):
        host_v[i, :v.size] = v
    host_a = np.full((n, a_stride), 0xDD, dtype=np.uint8)
    host_a[:, :frames.shape[1]] = frames
    d_v, d_a, d_dst, d_meta = dec.alloc(host_v.size), dec.alloc(host_a.size), dec.alloc(n * stride), dec.alloc(3 * r16(4 * n))
    d_v.upload(host_v)
    d_a.upload(host_a)
    d_dst.upload(np.full(n * stride, 0xA5, dtype=np.uint8))
    meta = np.full(3 * r16(4 * n) // 4, 0xFFFFFFFF, dtype=np.uint32)
    meta[:n] = [v.size for v in videos]
    d_meta.upload(meta)
    args = dict(n_streams=n, frame_bytes=frame_bytes, n_frames=n_frames, video_stride=v_stride, audio_stride=a_stride,
                dst_stride=stride, **opt)
    return n, stride, (d_v, d_a, d_dst, d_meta), args


def launch_mux(dec, prepared):
    """efx_mux_av on prepared buffers: one asynchronous launch, no copy and nothing synchronised."""
    n, _, (d_v, d_a, d_dst, d_meta), args = prepared
    p_len, p_st = d_meta.ptr + r16(4 * n), d_meta.ptr + 2 * r16(4 * n)
    dec.mux_to(d_v, d_meta.ptr, d_a if args["n_frames"] else None, d_dst, p_len, p_st, **args)


def collect_mux(dec, prepared):
    """(titles, status, the output regions [n, stride]) of a launch_mux, after a dec.sync()."""
    n, stride, (d_v, d_a, d_dst, d_meta), _ = prepared
    try:
        meta = d_meta.download(np.uint32, 3 * r16(4 * n) // 4)
        region = d_dst.download(np.uint8, n * stride).reshape(n, stride)
    finally:
        for b in (d_v, d_a, d_dst, d_meta):
            b.free()
    lens, st = meta[r16(4 * n) // 4:][:n], meta[2 * r16(4 * n) // 4:][:n]
    for i in range(n):
        assert (region[i, lens[i]:] == 0xA5).all(), f"stream {i}: bytes behind the title were written"
    return [region[i, :lens[i]].tobytes() for i in range(n)], st, region


def device_mux(efx, dec, videos, frames, dst_stride=None, frame_bytes=FB, **opt):
    """prepare_mux, launch_mux, a synchronisation, collect_mux."""
    prepared = prepare_mux(efx, dec, videos, frames, dst_stride, frame_bytes, **opt)
    launch_mux(dec, prepared)
    dec.sync()
    return collect_mux(dec, prepared)


@pytest.mark.parametrize("fpp,pid", [(8, 0x101), (1, 0x102), (32, 0x102)])
def test_bytes_equal_the_model(efx, videos, fpp, pid):
    """Item 10: streams of different length in one batch (99, 72, 24 and 40 pictures and an empty video), the audio starting
    in the middle of the title's time line."""
    rng = np.random.default_rng(fpp)
    n_frames = 777
    frames = rng.integers(0, 256, size=(len(videos), n_frames * FB), dtype=np.uint8)
    opt = dict(frames_per_pes=fpp, audio_pid=pid, audio_first_pts=9000 + 20 * 3003, audio_first_frame=5, audio_cc=11)
    dec = efx.Decoder(len(videos), 1, 2)
    titles, st, _ = device_mux(efx, dec, videos, frames, **opt)
    dec.close()
    assert (st == 0).all()
    for i, v in enumerate(videos):
        want, wst = X.mux(v, frames[i], frame_bytes=FB, frames_per_pes=fpp, pid=pid, first_pts=opt["audio_first_pts"], first_frame=5, cc=11)
        assert wst == 0 and titles[i] == want, i
    assert efx.mux_audio_packets(n_frames, FB, fpp) == X.audio_packets(n_frames, FB, fpp)


def test_no_audio_full_and_bad_video(efx, videos):
    """Item 10: an empty audio list copies the video; an output region one packet too small gives EFX_MUX_FULL, length 0 and
    an untouched region, the neighbours intact; a damaged video input gives EFX_MUX_BAD_VIDEO."""
    dec = efx.Decoder(len(videos), 1, 2)
    titles, st, _ = device_mux(efx, dec, videos, np.zeros((len(videos), 0), dtype=np.uint8))
    assert (st == 0).all() and all(t == v.tobytes() for t, v in zip(titles, videos))

    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, size=(len(videos), 300 * FB), dtype=np.uint8)
    want = [X.mux(v, frames[i], frame_bytes=FB, first_pts=9000) for i, v in enumerate(videos)]
    longest = max(len(w[0]) for w in want)
    tight = (longest - 188) // 16 * 16 + 16  # a multiple of 16 that holds everything but the longest title's last packet
    assert longest - 188 < tight < longest
    titles, st, region = device_mux(efx, dec, videos, frames, dst_stride=tight, audio_first_pts=9000)
    for i, (w, _) in enumerate(want):
        if len(w) == longest:
            assert st[i] == efx.MUX_FULL and titles[i] == b"" and (region[i] == 0xA5).all()
        else:
            assert st[i] == 0 and titles[i] == w

    damaged = [v.copy() for v in videos]
    damaged[0][188 * 7] = 0x46          # a packet without its sync byte
    damaged[1][188 * 5 + 2] = 0x01      # a packet of another PID
    damaged[2] = damaged[2][:-3]        # not a whole number of packets
    damaged[3] = damaged[3][188:]       # begins inside a PES
    titles, st, region = device_mux(efx, dec, damaged, frames, audio_first_pts=9000)
    for i in range(4):
        assert st[i] == efx.MUX_BAD_VIDEO and titles[i] == b"" and (region[i] == 0xA5).all(), i
    assert st[4] == 0 and titles[4] == want[4][0]
    dec.close()


def test_invalid_arguments(efx):
    dec = efx.Decoder(2, 1, 2)
    d = dec.alloc(1 << 16)
    good = dict(n_streams=2, frame_bytes=64, n_frames=4, video_stride=1024, audio_stride=256, dst_stride=4096)
    meta = np.zeros(64, dtype=np.uint32)
    d.upload(meta)
    args = (d.ptr + 8192, d.ptr, d.ptr + 16384, d.ptr + 32768, d.ptr + 64, d.ptr + 128)
    dec.mux_to(*args, **good)
    dec.sync()
    for change in (dict(n_streams=0), dict(n_streams=3), dict(audio_pid=0x100), dict(audio_pid=0x103), dict(frame_bytes=0),
                   dict(n_frames=-1), dict(frames_per_pes=0), dict(frames_per_pes=33), dict(samples_per_frame=0), dict(sample_rate=0),
                   dict(audio_first_pts=-1), dict(audio_first_pts=1 << 33), dict(audio_first_frame=-1), dict(audio_cc=16), dict(audio_cc=-1),
                   dict(video_stride=1000), dict(audio_stride=248), dict(audio_stride=240), dict(dst_stride=4104), dict(dst_stride=1 << 32)):
        with pytest.raises(efx.EfxError) as e:
            dec.mux_to(*args, **dict(good, **change))
        assert e.value.status == -1, change
    for k in range(6):
        for bad in (None, args[k] + 4):
            a = list(args)
            a[k] = bad
            with pytest.raises(efx.EfxError) as e:
                dec.mux_to(*a, **good)
            assert e.value.status == -1, (k, bad)
    assert efx.mux_bound(1880, 9, 64, 8) == r16(1880 + 188 * X.audio_packets(9, 64, 8))
    assert efx.mux_bound(0, 1, 64, 33) == 0 and efx.mux_audio_packets(-1, 64, 8) == -1
    dec.close()


def chain_inputs(n, P):
    pics = np.stack([E.moving(P, seed=20 + i) for i in range(n)])
    n_frames = -(-P * 3003 * 48000 // (90000 * 128))
    pcm = np.stack([M.signal(("chord", "lowpass", "sine")[i % 3], n_frames * 128, seed=i) for i in range(n)])
    return pics, pcm, n_frames


def check_titles(efx, titles, recon, pcm, n_frames, first_pts):
    """Item 11: what a title must be, for every stream."""
    n, P = recon.shape[0], recon.shape[1]
    arrs = [np.frombuffer(t, dtype=np.uint8) for t in titles]
    want_frames = M.encode(M.model_exe(), pcm)[0]
    dec = efx.Decoder(max(n, 3), P, ring_depth=P + 1, max_stream_bytes=3 * sum(a.size for a in arrs) + 4096 * n)  # (3: the index below)
    dec.upload(arrs, efx.FORMAT_TS)
    dec.decode()
    for i in range(n):
        assert dec.stream_status(i) == 0 and dec.picture_count(i) == P
        assert [dec.picture_pts(i, p) for p in range(P)] == [first_pts + 3003 * p for p in range(P)]
    for p in range(P):
        assert np.array_equal(dec.export_host("i420", picture=p), recon[:, p]), p
    # the audio: demultiplexed on the device, decoded on the device
    stride = r16(max(a.size for a in arrs))
    d_au, d_len = dec.alloc(n * stride), dec.alloc(4 * n)
    dec.demux_audio(arrs, d_au, stride, d_len)
    assert (d_len.download(np.uint32, n) == n_frames * FB).all()
    audio = d_au.download(np.uint8, n * stride).reshape(n, stride)[:, :n_frames * FB]
    assert np.array_equal(audio.reshape(n, n_frames, FB), want_frames)
    d_st, d_out, d_cnt = dec.alloc(n * efx.sbc_state_bytes()), dec.alloc(n * n_frames * 256), dec.alloc(4 * n)
    d_st.upload(np.zeros(n * efx.sbc_state_bytes(), dtype=np.uint8))
    dec.sbc_decode(n, d_au, stride, FB, n_frames, d_st, d_out, n_frames * 128, None, d_cnt)
    dec.sync()
    out = d_out.download(np.int16, n * n_frames * 128).reshape(n, -1)
    for i in range(n):
        want, _ = oracle.sbc_decode(want_frames[i].reshape(-1), FB)
        assert np.array_equal(out[i], want), i
        assert np.array_equal(oracle.ts_audio_es(arrs[i]), want_frames[i].reshape(-1))
        if i % 3 != 1:  # (chord and sine: the float yardstick's SNR is above 40 dB there, not for the low-passed noise)
            g, _ = M.fit(pcm[i], out[i])
            assert abs(g - 1) < 0.005 and M.best_delay(pcm[i], out[i]) == M.DELAY, (i, g)
    # the trick-play index of (title, title, title)
    three = [arrs[0]] * 3
    res = dec.index_streams(three, trick_speed=[1, 15, 15])
    assert efx.idx_build([r for r, _ in res], [s for _, s in res]) == oracle.make_idx(three)
    dec.close()
    for i in range(n):
        cnt, _, pts, fr = oracle.decode(arrs[i], 1, flush_last=True, want_frames=True)
        assert cnt == P and np.array_equal(fr, XM.i420_to_strip(recon[i])) and list(pts) == [first_pts + 3003 * p for p in range(P)]
        if oracle.have_ref():
            from espflix_amd import gen
            hashes, rpts, _ = oracle.ref_decode(arrs[i], flush_last=True)
            assert [int(h) for h in hashes] == [gen.fnv1a64(s) for s in XM.i420_to_strip(recon[i])]
            assert list(rpts) == list(pts)
            assert np.array_equal(oracle.ref_audio_es(arrs[i]), want_frames[i].reshape(-1))


def test_chain_without_synchronisation(efx):
    """Item 11: pictures + PCM -> efx_encode (TS) -> efx_sbc_encode -> efx_mux_av, queued back to back."""
    n, P = 3, 12
    pics, pcm, n_frames = chain_inputs(n, P)
    dec = efx.Decoder(n, 1, 2)
    v_stride, a_stride = efx.encode_bound(efx.FORMAT_TS, P), r16(n_frames * FB)
    stride = efx.mux_bound(v_stride, n_frames, FB, 8)
    d_pic, d_rec, d_v = dec.alloc(pics.size), dec.alloc(pics.size), dec.alloc(n * v_stride)
    d_pcm, d_state, d_a = dec.alloc(pcm.nbytes), dec.alloc(n * efx.sbc_enc_state_bytes()), dec.alloc(n * a_stride)
    d_dst, d_meta = dec.alloc(n * stride), dec.alloc(4 * 16)
    d_pic.upload(pics)
    d_pcm.upload(pcm)
    d_state.upload(np.zeros(n * efx.sbc_enc_state_bytes(), dtype=np.uint8))
    p = [d_meta.ptr + 16 * k for k in range(4)]
    dec.encode_to(d_pic, d_v, p[0], p[1], n_streams=n, n_pictures=P, qscale=6, gop=6, search=7, fmt=efx.FORMAT_TS, first_pts=PTS0,
                  dst_stride=v_stride, recon=d_rec)
    dec.sbc_encode_to(d_pcm, d_state, d_a, n_streams=n, n_frames=n_frames, frame_stride=a_stride)
    dec.mux_to(d_v, p[0], d_a, d_dst, p[2], p[3], n_streams=n, frame_bytes=FB, n_frames=n_frames, video_stride=v_stride,
               audio_stride=a_stride, dst_stride=stride, audio_first_pts=PTS0)
    dec.sync()
    meta = d_meta.download(np.uint32, 16)
    assert (meta[4:4 + n] == 0).all() and (meta[12:12 + n] == 0).all()
    region = d_dst.download(np.uint8, n * stride).reshape(n, stride)
    titles = [region[i, :meta[8 + i]].tobytes() for i in range(n)]
    video = d_v.download(np.uint8, n * v_stride).reshape(n, v_stride)
    frames = d_a.download(np.uint8, n * a_stride).reshape(n, a_stride)[:, :n_frames * FB]
    recon = d_rec.download(np.uint8, pics.size).reshape(pics.shape)
    dec.close()
    for i in range(n):
        want, st = X.mux(video[i, :meta[i]], frames[i], frame_bytes=FB, first_pts=PTS0)
        assert st == 0 and titles[i] == want
    check_titles(efx, titles, recon, pcm, n_frames, PTS0)


AV_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import test_gpu_mux as T

    pics, pcm, n_frames = T.chain_inputs(2, 12)
    dec = efx.Decoder(2, 1, 2, device=torch.cuda.current_device())
    titles, st = dec.encode_av(torch.from_numpy(pics).cuda(), torch.from_numpy(pcm).cuda(), qscale=6, gop=6, first_pts=T.PTS0)
    assert (st == 0).all()
    rec = dec.encode(torch.from_numpy(pics).cuda(), qscale=6, gop=6, first_pts=T.PTS0, recon=True)
    pickle.dump((titles, rec.recon.cpu().numpy(), rec.streams), open(sys.argv[2], "wb"))
    print("encode_av ok")
""")


def test_encode_av(efx, tmp_path):
    """Item 11 through Decoder.encode_av (tensors in: a process of its own, torch's HIP runtime first)."""
    import pickle
    script, out = tmp_path / "encode_av.py", tmp_path / "titles.pkl"
    script.write_text(AV_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "encode_av ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    titles, recon, video = pickle.load(open(out, "rb"))
    pics, pcm, n_frames = chain_inputs(2, 12)
    frames = M.encode(M.model_exe(), pcm)[0]
    for i in range(2):
        assert titles[i] == X.mux(np.frombuffer(video[i], dtype=np.uint8), frames[i], frame_bytes=FB, first_pts=PTS0)[0]
    check_titles(efx, titles, recon, pcm, n_frames, PTS0)
