"""Pins the CPU restatement against the reference ITSELF, run live: the unmodified reference
sources compiled into oracle/_ref by `make ref`.  Skipped where those binaries are absent."""
import ctypes

import numpy as np
import pytest

import common
import oracle
from espflix_amd import gen

pytestmark = pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref not built (needs /root/reference)")


@pytest.mark.parametrize("clip", ["splash", "vmedia"])
def test_clips_frame_by_frame(clip, clips):
    rh, rpts, rframes = oracle.ref_decode(clips[clip], flush_last=True, want_frames=True)
    n, h, pts, frames = oracle.decode(clips[clip], 1, want_frames=True)
    assert n == len(rh) and (h == rh).all() and (pts == rpts).all()
    assert np.array_equal(frames, rframes)


@pytest.mark.parametrize("flags", [0, 2, 4, 8, 16, 2 | 4 | 16, 64, 128, 64 | 128 | 4 | 2, 256, 256 | 4 | 8 | 64])
def test_fresh_synthetic_streams(flags):
    """Stream ids beyond the committed golden set."""
    b = gen.Batch(100, 6, 24, 12, flags)   # two GOPs: sequence header repeated mid-stream
    for k in range(6):
        rh, rpts, _ = oracle.ref_decode(b.ts(k))
        n, h, pts, _ = oracle.decode(b.ts(k), 1)
        assert n == len(rh) == 24 and (h == rh).all() and (pts == rpts).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_composite_random_frames(seed):
    fr = common.random_frames(seed)
    for ntsc in (True, False):
        assert np.array_equal(oracle.video_field(fr, ntsc, 0, 2), oracle.ref_video_field(fr, ntsc, 2))


def test_video_tables():
    for ntsc in (True, False):
        params, ctab, dither = oracle.ref_video_params(ntsc)
        assert np.array_equal(params, oracle.video_params(ntsc))
        assert np.array_equal(ctab, oracle.color_tab(ntsc))


@pytest.mark.parametrize("k", [0, 5])
def test_pdm_random(k):
    pcm = common.pdm_pcm(k, 30)
    ref = oracle.ref_pdm(pcm, silence_every=5, beep_at=2)
    st = np.zeros(3, dtype=np.int32)
    beep = ctypes.c_int(0)
    words = []
    for c in range(30):
        if c == 2:
            beep.value = 5
        words.append(oracle.write_pcm_16(st, beep, None if (c % 5) == 4 else pcm[c * 128:(c + 1) * 128]))
    assert np.array_equal(np.concatenate(words), ref)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_hostile_muxing_pts_latch(seed, clips):
    """PES boundaries a few bytes either side of the picture start codes, PTS absent / with DTS /
    header stuffing, random payload sizes, interleaved null / audio / adaptation-only packets: the
    restatement's demux and its PTS latch (look-ahead of the bit reader) follow the reference."""
    b = gen.Batch(200 + seed, 2, 8)
    clip_es = oracle.ts_to_es(clips["vmedia"]).tobytes()
    es_list = [b.es(0).tobytes(), b.es(1).tobytes(), clip_es[:common.picture_offsets(clip_es)[10]]]  # whole pictures
    for i, es in enumerate(es_list):
        ts = np.frombuffer(common.hostile_ts(es, 10 * seed + i), dtype=np.uint8)
        rh, rpts, _ = oracle.ref_decode(ts)
        n, h, pts, _ = oracle.decode(ts, 1)
        assert n == len(rh) and (h == rh).all(), (seed, i)
        assert (pts == rpts).all(), (seed, i, pts.tolist(), rpts.tolist())


@pytest.mark.parametrize("first_with_pts", [1, 2, 3, 5])
def test_no_push_and_no_swap_before_the_first_pts(first_with_pts):
    """flush_picture() while _last_pts == -1 (player.cpp:692-702): pictures ahead of the first PES PTS are decoded
    over each other and never pushed."""
    from espflix_amd import gen
    es = gen.Batch(50, 1, 8, 12, 0).es(0).tobytes()
    ts = np.frombuffer(common.late_pts_ts(es, first_with_pts), dtype=np.uint8)
    n, h, pts, _ = oracle.decode(ts, 1, flush_last=True)
    rh, rpts, _ = oracle.ref_decode(ts, flush_last=True)
    assert n == len(rh) == 8 - first_with_pts
    assert (h == rh).all() and list(pts) == list(rpts)


@pytest.mark.parametrize("ntsc", [True, False])
@pytest.mark.parametrize("case", common.DISPLAY_CASES, ids=[c[0] for c in common.DISPLAY_CASES])
def test_display_state_hscroll_and_overlay(case, ntsc):
    """The two-frame slide (_hscroll) and the overlay / progress bar (composite()) of video_isr."""
    name, front, hs, ov_seed, blend, progress = case
    fr = common.random_frames(77)
    fr = np.minimum(fr, 248)
    n = len(hs) if hs is not None else 6
    ov = common.overlay_bytes(ov_seed) if ov_seed is not None else None
    ref = oracle.ref_video_field_ex(fr, ntsc, n, front, hs, ov if ov is not None else (np.zeros(1280, np.uint8) if blend else None),
                                    blend, progress)
    got = oracle.video_field_ex(fr, ntsc, 0, n, front, hs, ov, blend, progress)
    assert np.array_equal(ref, got)


def test_sbc_tables():
    syn, pro = oracle.sbc_tables()
    rsyn, rpro = oracle.ref_sbc_tables()
    assert np.array_equal(syn, rsyn) and np.array_equal(pro, rpro)


@pytest.mark.parametrize("case", common.SBC_CASES, ids=[c[0] for c in common.SBC_CASES])
def test_sbc_synthetic_frames(case):
    name, kw, n, probe = case
    fr = common.sbc_frames(common.seed_of(name), n, **kw)
    ch = 1 if kw["mode"] == 0 else 2
    fb = common.sbc_frame_bytes(kw["blocks"], ch, kw["bitpool"])
    rpcm, rret = oracle.ref_sbc_decode(fr, fb, probe)
    pcm, ret = oracle.sbc_decode(fr, fb, probe)
    assert ret == rret and all(r[0] == fb for r in ret)
    assert np.array_equal(pcm, rpcm)


@pytest.mark.parametrize("clip", ["splash", "vmedia"])
def test_sbc_clip_audio(clip, clips):
    """The clips' own audio (PID 0x102), 128 samples per frame, decoded as decode_audio() does:
    the first frame is probed for the frame size (64 bytes in splash, 48 in vmedia) and thereby
    synthesised twice."""
    es = oracle.ts_audio_es(clips[clip])
    assert es.size >= 48 * 100 and es[0] == 0x9C
    fb = oracle.sbc_decode(es[:64], 64)[1][0][0]
    assert fb == common.CLIP_SBC_FRAME_BYTES[clip]
    n = es.size // fb
    rpcm, rret = oracle.ref_sbc_decode(es[:n * fb], fb, True)
    pcm, ret = oracle.sbc_decode(es[:n * fb], fb, True)
    assert ret == rret and all(r == (fb, 256) for r in ret)
    assert np.array_equal(pcm, rpcm) and np.abs(pcm.astype(int)).max() > 1000


def test_sbc_rejected_frames_resynthesise_state():
    """Bad sync byte / joint stereo / 4 subbands: what sbc_decoder() does with the stale state."""
    fr = common.sbc_frames(5, 12, freq=3, blocks=16, mode=0, alloc=0, bitpool=28).reshape(12, -1).copy()
    fr[3, 0] = 0x9D                       # bad sync: previous samples are synthesised again
    fr[6, 1] |= 0x0C                      # joint stereo: geometry changes to 2 channels, stale samples
    fr[9, 1] &= 0xFE                      # 4 subbands: returns -1 without synthesis
    rpcm, rret = oracle.ref_sbc_decode(fr.reshape(-1), fr.shape[1])
    pcm, ret = oracle.sbc_decode(fr.reshape(-1), fr.shape[1])
    assert ret == rret and np.array_equal(pcm, rpcm)
    assert ret[3][0] == -1 and ret[6][0] == -1 and ret[9][0] == -1


def test_trick_play_index_file(clips):
    """video.idx as the reference indexer writes it (indexer.cpp make_index + merge_index) and the
    player's own idx_hdr arithmetic (espflix.cpp:589-627) on it."""
    titles = common.index_titles() + [("clips", [clips["vmedia"], clips["splash"], clips["vmedia"]])]
    for name, streams in titles:
        ref = oracle.ref_make_idx(streams)
        got = oracle.make_idx(streams)
        assert len(got) == len(ref) > oracle.IDX_HDR_BYTES, name
        assert np.array_equal(oracle.idx_masked(got), oracle.idx_masked(ref)), name
        first, last = np.frombuffer(ref[8:24], dtype=np.int64)
        q = common.index_queries(int(first), int(last))
        want = oracle.ref_idx_query(ref, q)
        assert [oracle.idx_query(ref, p, s) for p, s in q] == want, name


def test_trick_play_index_edge_streams():
    """common.index_edge_streams() as the main stream of a title whose trick streams are two short valid ones: the
    restatement's origin rule (indexer.cpp:129-131), its (int)abs(int64) truncation and `mine = 0x7FFFFFF` (185-189)
    against what the reference indexer writes, and the recorded hashes of tests/golden/index_edges.json.
    Left out, because the reference cannot take them (they run against the restatement only, tests/test_gpu_index.py):
    common.INDEX_EDGE_NOT_FOR_REFERENCE -- `tie` and `cross256_sorted`, whose runs of equal sequence PTS make
    indexer.cpp:136 divide by zero.  (Streams without a sequence start, which the indexer indexes an empty vector for,
    are not among the edge streams.)"""
    import json
    import os
    with open(os.path.join(oracle.ROOT, "tests", "golden", "index_edges.json")) as f:
        recorded = json.load(f)
    small = np.frombuffer(common.index_small_ts(), dtype=np.uint8)
    assert sorted(common.INDEX_EDGE_NOT_FOR_REFERENCE) == ["cross256_sorted", "tie"]
    ran = []
    for name, ts in common.index_edge_streams():
        if name in common.INDEX_EDGE_NOT_FOR_REFERENCE:
            continue
        title = [np.frombuffer(ts, dtype=np.uint8), small, small]
        ref = oracle.ref_make_idx(title)
        got = oracle.make_idx(title)
        assert len(got) == len(ref) > oracle.IDX_HDR_BYTES, name
        assert np.array_equal(oracle.idx_masked(got), oracle.idx_masked(ref)), name
        assert f"{oracle.fnv1a64(oracle.idx_masked(ref)):016x}" == recorded[name], name
        ran.append(name)
    assert sorted(ran) == sorted(recorded) and len(ran) >= 13


@pytest.mark.parametrize("name", ["late_open", "long_open_long_closed", "boundaries", "hostile_long"])
def test_audio_bytes_pushed_across_chunks_and_rounds(name):
    """common.audio_gate_streams(): the _audio_pts gate held open and closed over thousands of packets, inside whole
    video streams the reference player reads to the end.  (common.audio_gate_cut_streams() cut the video, so the player
    does not return from them: restatement only, tests/test_gpu_demux_audio.py.)"""
    a = np.frombuffer(common.audio_gate_streams()[name], dtype=np.uint8)
    ref = oracle.ref_audio_es(a)
    got = oracle.ts_audio_es(a)
    assert 0 < ref.size < common.audio_payload_offered(a.tobytes()) and np.array_equal(ref, got)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_audio_bytes_pushed(seed, clips):
    """What push_audio() receives (MpegDecoder::demux, player.cpp:421-433): for the clips and for a
    video stream with hostile audio muxed in (PES with / without PTS: the _audio_pts gate)."""
    b = gen.Batch(400 + seed, 1, 8)
    cases = [common.interleave_audio(b.ts(0).tobytes(), seed)]
    if seed == 1:
        cases += [clips["splash"].tobytes(), clips["vmedia"].tobytes()]
    for ts in cases:
        a = np.frombuffer(ts, dtype=np.uint8)
        ref = oracle.ref_audio_es(a)
        got = oracle.ts_audio_es(a)
        assert ref.size > 0 and np.array_equal(ref, got)
