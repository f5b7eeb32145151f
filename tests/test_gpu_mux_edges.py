"""efx_mux_av (k_mux.hip) on the device against tests/mux_model.py, byte for byte, on the hand-built video of
tests/mux_streams.py and audio of odd frame sizes: every stuffing length, the PTS formula at the four SBC rates and with a
product that needs 64 bits, ties, PES starts the parser must and must not read, the seams between pass 1's chunks of 256
packets, every status, batches, reuse of one context without synchronisation, and the way back through the audio
demultiplexer.  Each case first asserts, from the model alone, that the condition it aims at occurs (Case.cover)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mux_model as X
import mux_streams as S
import oracle
from test_gpu_mux import collect_mux, device_mux, launch_mux, prepare_mux

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = S.families()
CASES = [c for cases in FAMILIES.values() for c in cases] + [S.batch(1), S.batch(65)]
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    assert (espflix_amd.MUX_FULL, espflix_amd.MUX_BAD_VIDEO) == (X.MUX_FULL, X.MUX_BAD_VIDEO)
    return espflix_amd


@pytest.fixture(scope="module")
def dec(efx):
    d = efx.Decoder(65, 1, 2)
    yield d
    d.close()


def compare(case, got):
    """Title bytes, length and status of every stream; a rejected stream's region untouched (device_mux has checked the
    0xA5 fill behind every title, which with regions side by side is the neighbours' as well)."""
    titles, st, region = got
    want = case.model()
    assert len(titles) == len(want)
    for i, (w, wst, _) in enumerate(want):
        assert st[i] == wst, (case.name, i, int(st[i]), wst)
        assert len(titles[i]) == len(w), (case.name, i, len(titles[i]), len(w))
        if titles[i] != w:
            a, b = np.frombuffer(titles[i], dtype=np.uint8), np.frombuffer(w, dtype=np.uint8)
            at = int(np.flatnonzero(a != b)[0])
            assert False, f"{case.name}, stream {i}: first difference in output packet {at // 188}, byte {at % 188}"
        if wst:
            assert (region[i] == 0xA5).all(), (case.name, i)


def run(efx, dec, case):
    case.cover()
    got = device_mux(efx, dec, case.videos, case.frames, dst_stride=case.dst_stride, frame_bytes=case.fb, **case.opt)
    compare(case, got)
    return got[0]


@pytest.mark.parametrize("name", list(BY_NAME))
def test_device_equals_the_model(efx, dec, name):
    """Families a to f (one launch each) and the PTS wrap: include/efx.h says video PTS are compared as written and audio
    PTS before they are masked to 33 bits; 'pts_wrap' pins that, and that the PTS bytes written are masked."""
    run(efx, dec, BY_NAME[name])


def test_three_calls_queued_without_synchronisation(efx):
    """On one context: few audio PES, then many (the library reallocates its video_before scratch while the first launch
    may still run), then few again.  Every buffer of the three calls is allocated and uploaded first -- an upload
    synchronises the library's stream -- so that the three efx_mux_av follow each other with no copy and no synchronisation
    of the test's in between; one synchronisation, then the three results."""
    few, many, again = BY_NAME["stuff_fb85_fpp4_n22"], BY_NAME["seams"], BY_NAME["video_shapes"]
    assert few.n_pes * len(few.videos) < again.n_pes * len(again.videos) < many.n_pes * len(many.videos)
    cases = (few, many, again)
    for c in cases:
        c.cover()
    d = efx.Decoder(16, 1, 2)
    try:
        prepared = [prepare_mux(efx, d, c.videos, c.frames, dst_stride=c.dst_stride, frame_bytes=c.fb, **c.opt) for c in cases]
        for p in prepared:
            launch_mux(d, p)
        d.sync()
        for c, p in zip(cases, prepared):
            compare(c, collect_mux(d, p))
    finally:
        d.close()


def test_audio_of_a_title_in_two_calls(efx, dec):
    """audio_first_frame and audio_cc passed on through efx_mux_audio_packets: the packets equal the one-call audio."""
    fb, fpp, n, half = 85, 4, 22, 12
    frames = np.random.default_rng(5).integers(0, 256, size=(1, n * fb), dtype=np.uint8)
    none = [np.zeros(0, dtype=np.uint8)]
    opt = dict(frame_bytes=fb, frames_per_pes=fpp, audio_first_pts=4321, samples_per_frame=96, sample_rate=44100)
    ap = efx.mux_audio_packets(half, fb, fpp)
    assert ap == X.audio_packets(half, fb, fpp) and (13 + ap) // 16 > 0
    a = device_mux(efx, dec, none, frames[:, :half * fb], audio_cc=13, **opt)
    b = device_mux(efx, dec, none, frames[:, half * fb:], audio_cc=(13 + ap) & 15, audio_first_frame=half, **opt)
    both = device_mux(efx, dec, none, frames, audio_cc=13, **opt)
    assert (a[1] == 0).all() and (b[1] == 0).all() and (both[1] == 0).all()
    assert a[0][0] + b[0][0] == both[0][0]
    assert both[0][0] == X.mux(none[0], frames[0], frame_bytes=fb, frames_per_pes=fpp, first_pts=4321, spf=96, rate=44100, cc=13)[0]


ROUND_TRIP = [c.name for c in FAMILIES["stuffing"]] + ["pts_spf96_rate44100", "pts_first_frame_30e6", "video_shapes", "seams", "exactly_fits", "pts_wrap", "batch1"]


def test_round_trip(efx, dec):
    """One title of every family (all of a's), as the device wrote it, taken apart again: the oracle's audio demultiplexer
    and k_demux_audio on the device return the frames, the PID-0x100 packets are the video.  Every stuffing length of
    family a is here: k_demux_audio meets adaptation_field_length 0 from this writer."""
    titles, frames, videos = [], [], []
    for name in ROUND_TRIP:
        c = BY_NAME[name]
        i = c.names.index("p799") if name == "seams" else 0
        t = run(efx, dec, c)[i]
        assert c.model()[i][1] == 0
        titles.append(np.frombuffer(t, dtype=np.uint8))
        frames.append(c.frames[i])
        videos.append(c.videos[i])
    for t, f, v, name in zip(titles, frames, videos, ROUND_TRIP):
        assert np.array_equal(oracle.ts_audio_es(t), f), name
        assert np.array_equal(X.video_only(t), v), name
    n = len(titles)
    d = efx.Decoder(n, 1, 2, max_stream_bytes=sum(t.size for t in titles) + 4096 * n)
    try:
        stride = (max(t.size for t in titles) + 255) & ~255
        d_audio, d_len = d.alloc(n * stride), d.alloc(4 * n)
        d.demux_audio(titles, d_audio, stride, d_len)
        lens = d_len.download(np.uint32, n)
        audio = d_audio.download(np.uint8, n * stride).reshape(n, stride)
    finally:
        d.close()
    for i, name in enumerate(ROUND_TRIP):
        assert lens[i] == frames[i].size and np.array_equal(audio[i, :lens[i]], frames[i]), name


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import espflix_amd as efx, mux_model as X, mux_streams as S
efx.load_library()
r16 = S.r16
dec = efx.Decoder(3, 1, 2)
#             fb  fpp frames: frames x fb and 188 x the audio packets are multiples of 16
for fb, fpp, n_frames in ((169, 1, 16), (170, 1, 8), (171, 1, 16), (172, 1, 4), (168, 1, 4), (16, 3, 11), (2048, 1, 1), (1, 32, 112)):
    ap = X.audio_packets(n_frames, fb, fpp)
    assert (n_frames * fb) % 16 == 0 and ap % 4 == 0
    T, D = 9000, fpp * 240
    videos = [S.shapes_video(T, D), S.seam_stream(257, T - 500, T + n_frames * 240 + 500, seed=fb),
              S.seam_stream(260, T, T + n_frames * 240, seed=fb + 1)]
    frames = np.random.default_rng(fb).integers(0, 256, size=(3, n_frames * fb), dtype=np.uint8)
    totals = [v.size + ap * 188 for v in videos]
    v_stride, a_stride, stride = r16(max(v.size for v in videos)), r16(n_frames * fb), r16(max(totals))
    assert videos[2].size % 16 == 0 and totals[2] % 16 == 0
    # every buffer ends with its last valid byte
    d_v, d_a, d_dst = dec.alloc(2 * v_stride + videos[2].size), dec.alloc(2 * a_stride + n_frames * fb), dec.alloc(2 * stride + totals[2])
    d_vlen, d_len, d_st = dec.alloc(16), dec.alloc(16), dec.alloc(16)
    host_v = np.zeros(2 * v_stride + videos[2].size, dtype=np.uint8)
    host_a = np.zeros(2 * a_stride + n_frames * fb, dtype=np.uint8)
    for i in range(3):
        host_v[i * v_stride:i * v_stride + videos[i].size] = videos[i]
        host_a[i * a_stride:i * a_stride + n_frames * fb] = frames[i]
    d_v.upload(host_v); d_a.upload(host_a)
    d_dst.upload(np.full(2 * stride + totals[2], 0xA5, dtype=np.uint8))
    d_vlen.upload(np.array([v.size for v in videos] + [0xFFFFFFFF], dtype=np.uint32))
    opt = dict(frames_per_pes=fpp, audio_first_pts=T, audio_cc=14)
    dec.mux_to(d_v, d_vlen, d_a, d_dst, d_len, d_st, n_streams=3, frame_bytes=fb, n_frames=n_frames, video_stride=v_stride,
               audio_stride=a_stride, dst_stride=stride, **opt)
    dec.sync()
    lens, st = d_len.download(np.uint32, 3), d_st.download(np.uint32, 3)
    out = d_dst.download(np.uint8, 2 * stride + totals[2])
    for i in range(3):
        want, wst = X.mux(videos[i], frames[i], frame_bytes=fb, frames_per_pes=fpp, first_pts=T, cc=14)
        assert wst == 0 == st[i] and lens[i] == len(want) == totals[i], (fb, i)
        assert out[i * stride:i * stride + lens[i]].tobytes() == want, (fb, i)
        assert (out[i * stride + lens[i]:(i + 1) * stride] == 0xA5).all(), (fb, i)
    for b in (d_v, d_a, d_dst, d_vlen, d_len, d_st):
        b.free()
dec.close()
print("GUARD_OK")
"""


@pytest.mark.parametrize("guard", ["1", "2"])
def test_every_buffer_of_a_call_under_the_guard_page_allocator(guard):
    """EFX_GUARD: every device buffer is its own mapping that ends (1) or starts (2) on an unmapped page.  The last stream's
    video ends with its last packet, the audio with the last frame, the destination with the last title, and video_len,
    len and status are 3 entries rounded up to 16 bytes.  This confirms what k_mux.hip reads and writes; the argument, with
    n_pkts = video_len / 188, per stream:
      video_len[s], len[s], status[s]: s < n_streams.
      pass 0: one aligned dword at packet i's first byte, i < n_pkts (the bases and strides are multiples of 16, 188 of 4);
        video_start_pts on packet 0 only when n_pkts > 0.  video_start_pts reads p[3], p[4], then p[off .. off + 2] and
        p[off + 7] only behind `off + 9 <= 188` (&& short-circuits) and the PTS p[off + 9 .. off + 13] only behind
        `off + 14 <= 188`: all inside the packet's 188 bytes.
      pass 1: p[1] of packet i < n_pkts; src[d] with d < n_here x 47 dwords, n_here <= n_pkts - i0: inside the video.  Stores
        to output packet i + audio_packets_of(incl) <= n_pkts - 1 + audio_packets, 47 dwords: inside total = (n_pkts +
        audio_packets) x 188 <= dst_stride (else EFX_MUX_FULL returned before any store).  video_before[j] for excl <= j <
        incl <= n_pes (audio_upto returns at most n_pes): inside the stream's n_pes entries of the library's scratch.
      pass 2: ap < audio_packets, j <= n_pes - 1, video_before[j] <= n_pkts, so the output packet is below n_pkts +
        audio_packets; frames[j x fpp x fb + pp - 14] with pp < 14 + n_fr x fb and n_fr = min(fpp, n_frames - j x fpp): below
        n_frames x fb.  With n_frames = 0 neither loop runs and the audio pointer is not read."""
    env = dict(os.environ, EFX_GUARD=guard)
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GUARD_OK" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-1500:])
    assert f"libefx: EFX_GUARD={guard}" in r.stderr  # the allocator was in force
