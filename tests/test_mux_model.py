"""The A/V multiplexer's rules (include/efx.h: efx_mux_av) as tests/mux_model.py restates them, no GPU: a multiplexed title
plays like its video alone plus exactly its audio -- through the test oracle, and through the unmodified reference player
where oracle/_ref is built."""
import numpy as np
import pytest

import encode_model as E
import mux_model as X
import oracle

FB = 64  # mono, 48 kHz, 16 blocks, bitpool 28: the frames the player plays


@pytest.fixture(scope="module")
def videos(clips, tmp_path_factory):
    exe = E.build(str(tmp_path_factory.mktemp("enc_model")))
    enc, _ = E.encode(exe, E.moving(24), gop=12, qscale=6, search=7, fmt=1, first_pts=9000)
    return {"splash": X.video_only(clips["splash"]), "vmedia": X.video_only(clips["vmedia"]),
            "encoded": np.frombuffer(enc, dtype=np.uint8).copy()}


def audio_for(video: np.ndarray, seed: int):
    """Random 64-byte frames that start at the first video PTS and last as long as the video does."""
    units = X.video_units(video)
    pts = [u[2] for u in units if u[2] is not None]
    n_frames = int(np.ceil((max(pts) + 3003 - pts[0]) * 48000 / 90000 / 128))
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=n_frames * FB, dtype=np.uint8), pts[0]


@pytest.mark.parametrize("name", ["splash", "vmedia", "encoded"])
@pytest.mark.parametrize("fpp", [1, 8, 32])
@pytest.mark.parametrize("pid", [0x101, 0x102])
def test_title_plays_like_its_parts(videos, name, fpp, pid):
    video = videos[name]
    frames, first = audio_for(video, fpp * 7 + pid)
    title, status, units = X.mux(video, frames, frame_bytes=FB, frames_per_pes=fpp, pid=pid, first_pts=first, cc=5, want_units=True)
    assert status == 0 and len(title) % 188 == 0
    title = np.frombuffer(title, dtype=np.uint8)
    # pictures and PTS of the video alone; exactly the frames
    n0, h0, p0, _ = oracle.decode(video, 1)
    n1, h1, p1, _ = oracle.decode(title, 1)
    assert n0 == n1 > 0 and np.array_equal(h0, h1) and np.array_equal(p0, p1)
    assert np.array_equal(oracle.ts_audio_es(title), frames)
    assert oracle.ts_audio_es(video).size == 0
    if oracle.have_ref():
        rh0, rp0, _ = oracle.ref_decode(video)
        rh1, rp1, _ = oracle.ref_decode(title)
        assert np.array_equal(rh0, rh1) and np.array_equal(rp0, rp1) and rh1.size == n0
        assert np.array_equal(oracle.ref_audio_es(title), frames)
    # the sequence starts of the video alone, same PTS, at the packets the model put them
    f0, l0, sp0, so0 = oracle.ts_sequences(video)
    f1, l1, sp1, so1 = oracle.ts_sequences(title)
    assert (f0, l0) == (f1, l1) and np.array_equal(sp0, sp1)
    v_units = [u for u in units if u[0] == "v"]
    first_of = {u[0]: k for k, u in enumerate(X.video_units(video))}
    assert [v_units[first_of[int(o)]][2] for o in so0] == [int(o) for o in so1]
    # PES units in PTS order, audio first at ties, the order inside each kind kept, the title gapless
    at, reach, last_audio = 0, -1, -1
    for kind, pts, start, n in units:
        assert start == at
        at += n
        if kind == "v":
            reach = max(reach, pts if pts is not None else reach)
        else:
            assert pts > last_audio
            last_audio = pts
    assert at * 188 == title.size
    last_video_pts = -1
    for k, (kind, pts, start, n) in enumerate(units):
        if kind == "v":
            if pts is not None:
                # no audio at or before this PTS comes later
                assert all(u[1] > pts for u in units[k + 1:] if u[0] == "a")
                last_video_pts = max(last_video_pts, pts)
        else:
            # an audio PES follows only video that is strictly earlier, unless no video is left
            later_video = [u for u in units[k + 1:] if u[0] == "v"]
            assert last_video_pts < pts or not later_video
    # continuity counters per PID
    pk = title.reshape(-1, 188)
    pids = ((pk[:, 1].astype(int) & 0x1F) << 8) | pk[:, 2]
    assert set(pids.tolist()) == {0x100, pid}
    cc = pk[pids == pid][:, 3] & 15
    assert cc[0] == 5 and np.array_equal(cc, (5 + np.arange(cc.size)) & 15)
    assert np.array_equal(pk[pids == 0x100].reshape(-1), video)


def test_audio_between_two_pictures_is_bounded(videos):
    """8 x 64-byte frames per PES: a picture lasts 3 003 ticks, a PES 1 920, so at most two PES (1 024 audio bytes) lie
    between two video PES starts."""
    video = videos["encoded"]
    frames, first = audio_for(video, 1)
    _, status, units = X.mux(video, frames, frame_bytes=FB, frames_per_pes=8, first_pts=first, want_units=True)
    assert status == 0
    n_frames, run, audio_seen = frames.size // FB, 0, 0
    last_video = max(k for k, u in enumerate(units) if u[0] == "v")
    for k, (kind, pts, start, n) in enumerate(units[:last_video]):
        if kind == "v":
            run = 0
        else:
            run += min(8, n_frames - 8 * audio_seen) * FB
            audio_seen += 1
            assert run <= 1024
    assert audio_seen > 10


def test_statuses_and_continuation(videos):
    video = videos["encoded"]
    frames, first = audio_for(video, 2)
    n = frames.size // FB
    whole, st = X.mux(video, frames, frame_bytes=FB, frames_per_pes=8, first_pts=first)
    assert st == 0
    assert X.mux(video, frames, frame_bytes=FB, dst_stride=len(whole) - 188)[1] == X.MUX_FULL
    assert X.mux(video, frames, frame_bytes=FB, dst_stride=len(whole), first_pts=first)[0] == whole
    bad = video.copy()
    bad[188 * 3] = 0x46
    assert X.mux(bad, frames, frame_bytes=FB)[1] == X.MUX_BAD_VIDEO
    assert X.mux(video[:-1], frames, frame_bytes=FB)[1] == X.MUX_BAD_VIDEO
    assert X.mux(video[188:], frames, frame_bytes=FB)[1] == X.MUX_BAD_VIDEO
    # no audio: the video unchanged
    assert X.mux(video, frames[:0], frame_bytes=FB) == (video.tobytes(), 0)
    # the audio of a title in two calls: the frames' PTS and the continuity counter run on
    half = (n // 2) // 8 * 8
    a, _ = X.mux(video[:0], frames[:half * FB], frame_bytes=FB, first_pts=first, cc=3)
    b, _ = X.mux(video[:0], frames[half * FB:], frame_bytes=FB, first_pts=first, first_frame=half,
                 cc=(3 + X.audio_packets(half, FB, 8)) & 15)
    both, _ = X.mux(video[:0], frames, frame_bytes=FB, first_pts=first, cc=3)
    assert a + b == both
