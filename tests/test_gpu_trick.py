"""efx_trick_pick (k_trick.hip) on the device against tests/trick_model.py, bit for bit, from I420 pictures and from the
frame rings; the fast-forward and rewind streams of Decoder.trick_streams against the encoder's own bytes; and the title
directory of Decoder.make_title -- video.ts, video_fwd.ts, video_rwd.ts, video.idx -- against the index oracle, the player's
index arithmetic (espflix.cpp:589-627) and a seek into the trick streams."""
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import common
import encode_model as E
import oracle
import trick_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = M.FRAME_BYTES
PTS0 = 129003
PAD = 64        # bytes between streams in every padded region
FILL = 0xA5
ARG, STATE = -1, -5


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def random_title():
    """2 streams x 21 pictures of random bytes."""
    return np.random.default_rng(2026).integers(0, 256, (2, 21, PIC), dtype=np.uint8)


class Region:
    """n_streams x (images + one spare image) x 101376 bytes + a pad per stream, filled with FILL, on the device."""

    def __init__(self, dec, n_streams, images):
        self.n, self.images = n_streams, images
        self.stride = (images + 1) * PIC + PAD
        self.buf = dec.alloc(n_streams * self.stride)
        self.buf.upload(np.full(n_streams * self.stride, FILL, dtype=np.uint8))
        self.want = np.full((n_streams, self.stride), FILL, dtype=np.uint8)  # what the model expects there

    def images_of(self, a):
        return a[:, :(self.images + 1) * PIC].reshape(self.n, self.images + 1, PIC)

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


@pytest.mark.parametrize("calls", [(7, 7, 7), (5, 16)])
@pytest.mark.parametrize("speed", [1, 2, 3, 15])
def test_i420_source_matches_model(efx, random_title, speed, calls):
    """Every call of a title offered piecewise, first_picture carried on: fwd only, rwd only and both, padded strides, a
    spare image behind each region; every byte outside the picked images keeps its fill."""
    dec = efx.Decoder(2, 1)
    n, total, _ = random_title.shape
    K = M.total_picks(total, speed)
    for mode in ("fwd", "rwd", "both"):
        rwd = Region(dec, n, K) if mode != "fwd" else None
        first = 0
        for cnt in calls:
            piece = random_title[:, first:first + cnt]
            src, src_stride = upload_padded(dec, piece)
            picks = M.count(first, cnt, speed)
            fwd = Region(dec, n, picks) if mode != "rwd" else None
            got = dec.trick_pick_to(src, fwd and fwd.buf, rwd and rwd.buf, n_streams=n, n_pictures=cnt, speed=speed,
                                    first_picture=first, total_pictures=total if rwd else 0, src_stride=src_stride,
                                    fwd_stride=fwd.stride if fwd else 0, rwd_stride=rwd.stride if rwd else 0)
            dec.sync()
            assert got == picks == efx.trick_count(first, cnt, speed)
            M.pick(piece, first, speed, total, fwd and fwd.images_of(fwd.want), rwd and rwd.images_of(rwd.want))
            if fwd:
                fwd.check(f"{mode}: fwd region of call ({first}, {cnt})")
                fwd.free()
            if rwd:
                rwd.check(f"{mode}: rwd region after call ({first}, {cnt})")
            src.free()
            first += cnt
        if rwd:
            # the whole title's picks, reversed
            assert np.array_equal(rwd.images_of(rwd.want)[:, :K], random_title[:, ::speed][:, ::-1])
            rwd.free()
    dec.close()


def test_call_without_picks_writes_nothing(efx, random_title):
    """3 pictures from first_picture = 1 at speed 15: no picks, EFX_OK, no byte written."""
    dec = efx.Decoder(2, 1)
    src, src_stride = upload_padded(dec, random_title[:, 1:4])
    fwd, rwd = Region(dec, 2, 1), Region(dec, 2, 2)
    assert efx.trick_count(1, 3, 15) == 0
    assert dec.trick_pick_to(src, fwd.buf, rwd.buf, n_streams=2, n_pictures=3, speed=15, first_picture=1, total_pictures=21,
                             src_stride=src_stride, fwd_stride=fwd.stride, rwd_stride=rwd.stride) == 0
    dec.sync()
    fwd.check("fwd")
    rwd.check("rwd")
    dec.close()


def test_ring_source_is_the_i420_export(efx):
    """2 streams x 14 pictures decoded as two pieces of 7 into a ring of 8: every picked image is what
    export_host("i420", picture=j) gives for that piece; first_stream = 1, n_streams = 1 picks stream 1 only."""
    from espflix_amd import gen
    b = gen.Batch(700, 2, 14, 12, 0)
    ts = [b.ts(i) for i in range(2)]
    dec = efx.Decoder(max_streams=2, max_pictures=7, ring_depth=8, max_stream_bytes=sum(len(t) for t in ts) + 8192)
    dec.upload(ts, efx.FORMAT_TS)
    speed, total = 3, 14
    K = M.total_picks(total, speed)
    rwd, rwd1 = Region(dec, 2, K), Region(dec, 1, K)
    for first in (0, 7):
        dec.decode(first_picture=first, n_pictures=7)
        assert [dec.picture_count(i) for i in range(2)] == [7, 7]
        exports = np.stack([dec.export_host("i420", picture=j) for j in range(7)], axis=1)  # (2, 7, 101376)
        picks = M.count(first, 7, speed)
        fwd, fwd1 = Region(dec, 2, picks), Region(dec, 1, picks)
        assert dec.trick_pick_to(None, fwd.buf, rwd.buf, n_streams=2, n_pictures=7, speed=speed, first_picture=first,
                                 total_pictures=total, source=efx.TRICK_FROM_RING, fwd_stride=fwd.stride,
                                 rwd_stride=rwd.stride) == picks
        dec.trick_pick_to(None, fwd1.buf, rwd1.buf, n_streams=1, first_stream=1, n_pictures=7, speed=speed, first_picture=first,
                          total_pictures=total, source=efx.TRICK_FROM_RING, fwd_stride=fwd1.stride, rwd_stride=rwd1.stride)
        dec.sync()
        M.pick(exports, first, speed, total, fwd.images_of(fwd.want), rwd.images_of(rwd.want))
        M.pick(exports[1:], first, speed, total, fwd1.images_of(fwd1.want), rwd1.images_of(rwd1.want))
        assert len(M.placements(first, 7, speed, total)) == picks > 0
        fwd.check(f"fwd of the piece from {first}")
        fwd1.check(f"fwd of stream 1, piece from {first}")
        rwd.check(f"rwd after the piece from {first}")
        rwd1.check(f"rwd of stream 1 after the piece from {first}")
        # the export is unchanged by the picks in between
        assert np.array_equal(dec.export_host("i420", picture=6), exports[:, 6])
    dec.close()


def test_argument_and_state_errors(efx, random_title):
    """Every EFX_ERR_ARG / EFX_ERR_STATE case of include/efx.h returns its status and leaves the destinations alone."""
    dec = efx.Decoder(max_streams=2, max_pictures=7, ring_depth=4)
    src, src_stride = upload_padded(dec, random_title[:, :6])
    fwd, rwd = Region(dec, 2, 2), Region(dec, 2, 7)
    ok = dict(n_streams=2, n_pictures=6, speed=3, first_picture=0, total_pictures=21, src_stride=src_stride,
              fwd_stride=fwd.stride, rwd_stride=rwd.stride)
    I, R = efx.TRICK_FROM_I420, efx.TRICK_FROM_RING

    def status(s, f, r, **kw):
        with pytest.raises(efx.EfxError) as e:
            dec.trick_pick_to(s, f, r, **{**ok, **kw})
        return e.value.status

    S, F, W = src.ptr, fwd.buf.ptr, rwd.buf.ptr
    arg_cases = [
        (S, F, W, dict(n_streams=0)), (S, F, W, dict(n_pictures=0)), (S, F, W, dict(speed=0)), (S, F, W, dict(speed=256)),
        (S, F, W, dict(source=2)), (S, F, W, dict(source=-1)), (S, F, W, dict(first_picture=-1)),
        (S, F, W, dict(first_picture=1 << 40, total_pictures=(1 << 40) + 6)),
        (S, None, None, {}),                                   # both destinations NULL
        (None, F, W, {}),                                      # the I420 source without src_device
        (S, F, W, dict(source=R)),                             # the ring source with one
        (None, F, W, dict(source=R, first_stream=-1)),
        (None, F, W, dict(source=R, n_pictures=8)),            # above max_pictures
        (S + 8, F, W, {}), (S, F + 8, W, {}), (S, F, W + 8, {}), (S, F + 4, None, {}), (S, None, W + 1, {}),  # alignment
        (S, F, W, dict(src_stride=6 * PIC - 16)), (S, F, W, dict(src_stride=6 * PIC + 8)),
        (S, F, W, dict(fwd_stride=2 * PIC - 16)), (S, F, W, dict(fwd_stride=2 * PIC + 8)),
        (S, F, W, dict(rwd_stride=7 * PIC - 16)), (S, F, W, dict(rwd_stride=7 * PIC + 8)),
        (S, F, W, dict(total_pictures=5)),                     # below first_picture + n_pictures
        (S, F, W, dict(first_picture=16, total_pictures=21)),  # 16 + 6 > 21
    ]
    for k, (s, f, r, kw) in enumerate(arg_cases):
        assert status(s, f, r, **kw) == ARG, (k, kw)
    # strides of a region that is not given are not read; total_pictures is read only with rwd_device
    dec.trick_pick_to(S, F, None, **{**ok, "rwd_stride": 8, "total_pictures": 0})
    dec.sync()
    M.pick(random_title[:, :6], 0, 3, 21, fwd.images_of(fwd.want), None)
    fwd.check("fwd alone")
    ring = dict(source=R, n_pictures=3)
    assert status(None, F, W, **ring) == STATE                                  # no decode yet
    from espflix_amd import gen
    dec.upload([gen.Batch(701, 1, 3, 12, 0).ts(0)], efx.FORMAT_TS)
    dec.decode(first_picture=0, n_pictures=3)
    assert status(None, F, W, **ring) == STATE                                  # two streams, one decoded
    assert status(None, F, W, **ring, n_streams=1, first_stream=1) == STATE
    assert status(None, F, W, **ring, n_streams=1, first_stream=2) == STATE     # beyond max_streams as well
    assert status(None, F, W, source=R, n_pictures=4, n_streams=1) == STATE     # n_pictures >= ring_depth
    assert status(None, F, W, source=R, n_pictures=7, n_streams=1) == STATE
    dec.sync()
    fwd.check("fwd after the refused calls")
    rwd.check("rwd after the refused calls")
    dec.close()


def moving_title(n_pictures):
    """2 streams of smooth moving content (the encode tests' texture), (2, n_pictures, 101376)."""
    return np.stack([E.moving(n_pictures, seed=7), E.moving(n_pictures, seed=11)])


@pytest.mark.parametrize("bitrate", [None, 400_000])
def test_trick_streams_are_the_encoders(efx, bitrate):
    """fwd is encode() of every third picture, rwd encode() of the same reversed, although fwd is made in pieces of 7
    pictures with continuation (which carries the rate controller's state); both decode to 7 pictures at first_pts + 3003 k.
    Status 0 at a fixed quantiser; at 400 kbit/s the status is the encoder's own (GOPs of 3 pictures of this content do not
    fit the buffer model at that rate: ENCODE_VBV, from encode() and from trick_streams alike)."""
    pics = moving_title(19)
    dec = efx.Decoder(2, 1)
    opts = dict(gop=3, qscale=8, search=3, first_pts=PTS0, bitrate=bitrate)
    fwd, rwd, st = dec.trick_streams(pics, speed=3, piece=7, **opts)
    assert st.shape == (2, 2) and st.dtype == np.uint32
    picks = np.ascontiguousarray(pics[:, ::3])
    want_f = dec.encode(picks, **opts)
    want_r = dec.encode(np.ascontiguousarray(picks[:, ::-1]), **opts)
    # ... and in one piece, and picture by picture
    fwd1, rwd1, _ = dec.trick_streams(pics, speed=3, **opts)
    fwd2, rwd2, _ = dec.trick_streams(pics, speed=3, piece=1, **opts)
    dec.close()
    assert np.array_equal(st[0], want_f.status) and np.array_equal(st[1], want_r.status)
    if bitrate is None:
        assert (st == 0).all()
    else:
        assert not (st & ~np.uint32(efx.ENCODE_VBV)).any()
    for i in range(2):
        assert fwd[i] == want_f.streams[i], f"fwd stream {i}"
        assert rwd[i] == want_r.streams[i], f"rwd stream {i}"
        assert fwd1[i] == fwd[i] == fwd2[i] and rwd1[i] == rwd[i] == rwd2[i]
        for ts in (fwd[i], rwd[i]):
            a = np.frombuffer(ts, dtype=np.uint8)
            n, hashes, pts, _ = oracle.decode(a, 1, flush_last=True)
            assert n == 7 and list(pts) == [PTS0 + 3003 * k for k in range(7)]
            if oracle.have_ref():
                rh, rp, _ = oracle.ref_decode(a, flush_last=True)
                assert [int(h) for h in rh] == [int(h) for h in hashes] and list(rp) == list(pts)


# ---- the title directory -------------------------------------------------------------------------------------------------------
TITLE_PICTURES, TITLE_SPEED = 31, 3


def title_inputs():
    pics = moving_title(TITLE_PICTURES)
    t = np.arange(48000)
    pcm = np.stack([np.round(6000 * np.sin(2 * np.pi * f * t / 48000)).astype(np.int16) for f in (440, 1000)])
    return pics, pcm


TITLE_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import test_gpu_trick as T

    pics, pcm = T.title_inputs()
    # (max_streams 3: make_title indexes a title's three streams in one call; the second decoder, of 2, one by one)
    dec = efx.Decoder(3, 1, 2, device=torch.cuda.current_device(), max_stream_bytes=8 << 20)
    titles, st = dec.make_title(torch.from_numpy(pics).cuda(), torch.from_numpy(pcm).cuda(), speed=T.TITLE_SPEED, qscale=8,
                                gop=12, search=3, first_pts=T.PTS0)
    # ... and at the indexer's own speed, 15: three picks, one GOP of each trick stream
    dec.close()
    dec = efx.Decoder(2, 1, 2, device=torch.cuda.current_device(), max_stream_bytes=8 << 20)
    titles15, st15 = dec.make_title(torch.from_numpy(pics).cuda(), torch.from_numpy(pcm).cuda(), speed=15, qscale=8, gop=12,
                                    search=3, first_pts=T.PTS0)
    dec.close()
    pickle.dump((titles, st, titles15, st15), open(sys.argv[2], "wb"))
    print("make_title ok")
""")


@pytest.fixture(scope="module")
def titles(efx, tmp_path_factory):
    """Decoder.make_title on 2 streams x 31 pictures + 1 s of 48 kHz PCM, speed 3 (tensors in: a process of its own,
    torch's HIP runtime first)."""
    tmp = tmp_path_factory.mktemp("make_title")
    script, out = tmp / "make_title.py", tmp / "titles.pkl"
    script.write_text(TITLE_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "make_title ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    made, st, made15, st15 = pickle.load(open(out, "rb"))
    for m, s in ((made, st), (made15, st15)):
        assert s.shape == (3, 2) and (s == 0).all()
        assert [sorted(t) for t in m] == [["video.idx", "video.ts", "video_fwd.ts", "video_rwd.ts"]] * 2
    return made, made15


def oracle_idx(three, speed, ref=False):
    """video.idx of the index oracle (or of the compiled reference indexer) for a title whose trick streams run at `speed`.
    Both write the indexer's fixed trick_speed of 15 into the fwd and rwd records (indexer.cpp:308-309 with make_index's
    argument; oracle/efx_oracle.c), whatever the streams hold: for another speed those two words -- bytes 60-63 and 92-95
    of the file -- are set to it, every other byte is theirs."""
    idx = bytearray(oracle.ref_make_idx(three) if ref else oracle.make_idx(three))
    for off in (60, 92):
        assert int.from_bytes(idx[off:off + 4], "little") == 15
        idx[off:off + 4] = int(speed).to_bytes(4, "little")
    return bytes(idx)


def decoded(efx, ts, max_pictures=40):
    """[(pts, FNV-1a-64 of the ring frame)] of every picture of a transport stream, and its status."""
    dec = efx.Decoder(1, max_pictures, max_pictures + 1, max_stream_bytes=len(ts) + 8192)
    dec.upload([np.frombuffer(ts, dtype=np.uint8)], efx.FORMAT_TS)
    dec.decode()
    h = dec.frame_hashes()
    out = [(dec.picture_pts(0, p), int(h[0, dec.picture_slot(p)])) for p in range(dec.picture_count(0))]
    status = dec.stream_status(0)
    dec.close()
    return out, status


def test_title_directory(efx, titles):
    """make_title at speed 3, and at speed 15 for the index file byte for byte as the oracle and the reference write it."""
    titles, titles15 = titles
    for i, t in enumerate(titles15):
        three = [np.frombuffer(t[k], dtype=np.uint8) for k in ("video.ts", "video_fwd.ts", "video_rwd.ts")]
        assert t["video.idx"] == oracle.make_idx(three)
        if oracle.have_ref():
            # (the reference leaves the tail padding of its three records unset: masked, as test_oracle_vs_ref.py does)
            assert np.array_equal(oracle.idx_masked(t["video.idx"]), oracle.idx_masked(oracle.ref_make_idx(three)))
        assert t["video.ts"] == titles[i]["video.ts"]  # the title itself does not depend on the speed
        for ts in three[1:]:
            assert oracle.decode(ts, 1, flush_last=True)[0] == M.total_picks(TITLE_PICTURES, 15)
    N, speed = TITLE_PICTURES, TITLE_SPEED
    K = M.total_picks(N, speed)
    pts_main = lambda t: PTS0 + 3003 * t
    pts_trick = lambda k: PTS0 + 3003 * k
    for t in titles:
        main, fwd, rwd, idx = (t[k] for k in ("video.ts", "video_fwd.ts", "video_rwd.ts", "video.idx"))
        three = [np.frombuffer(s, dtype=np.uint8) for s in (main, fwd, rwd)]
        assert idx == oracle_idx(three, speed)
        if oracle.have_ref():
            assert np.array_equal(oracle.idx_masked(idx), oracle.idx_masked(oracle_idx(three, speed, ref=True)))
        bound = (speed - 1) * 3003 + 1
        for k in range(K):
            assert abs(efx.idx_pts2pts(idx, pts_trick(k), 1) - pts_main(speed * k)) <= bound, k
            # rwd picture m shows pick K - 1 - m
            assert abs(efx.idx_pts2pts(idx, pts_trick(k), -1) - pts_main(speed * (K - 1 - k))) <= bound, k
        first, last = (int(v) for v in np.frombuffer(idx[8:24], dtype=np.int64))
        assert (first, last) == (pts_main(0), pts_main(N - 1))
        for speed_sign, ts in ((1, fwd), (-1, rwd)):
            full, status = decoded(efx, ts)
            assert status == 0 and [p for p, _ in full] == [pts_trick(k) for k in range(K)]
            packets = set()
            for pts, sp in common.index_queries(first, last):
                if sp != speed_sign:
                    continue
                off = efx.idx_pts2offset(idx, pts, sp)
                assert off + 4 <= len(idx)
                packets.add(int(np.frombuffer(idx[off:off + 4], dtype=np.uint32)[0]))
            assert packets  # (speed -1: the player's unsigned arithmetic sends every probe of this range to the last sample)
            for packet in sorted(packets):
                pkt = ts[packet * 188:packet * 188 + 188]
                assert len(pkt) == 188 and pkt[0] == 0x47 and pkt[1] & 0x40 and ((pkt[1] & 0x1F) << 8 | pkt[2]) == 0x100
                payload = pkt[4 + (1 + pkt[4] if pkt[3] & 0x20 else 0):]
                assert payload[:4] == b"\x00\x00\x01\xe0"                               # a PES starts here ...
                assert payload[9 + payload[8]:][:4] == b"\x00\x00\x01\xb3"              # ... with a sequence header
                tail, status = decoded(efx, ts[packet * 188:])
                assert status == 0 and 0 < len(tail) <= K
                assert tail == full[K - len(tail):], (speed_sign, packet)              # closed GOP: the same pictures


def test_transcode_route(efx, titles):
    """trick_streams(title=...) on the finished video.ts: decoded in pieces of 11 pictures, picked from the frame rings."""
    titles, _ = titles
    mains = [t["video.ts"] for t in titles]
    cap = sum(len(m) for m in mains) + 16384
    opts = dict(gop=3, qscale=8, search=3, first_pts=PTS0)
    dec = efx.Decoder(2, 11, 12, max_stream_bytes=cap)
    fwd, rwd, st = dec.trick_streams(title=mains, speed=TITLE_SPEED, **opts)
    assert (st == 0).all()
    with pytest.raises(ValueError):
        dec.trick_streams(title=[mains[0], titles[1]["video_fwd.ts"]], speed=TITLE_SPEED, **opts)
    dec.close()
    for ts in fwd + rwd:
        assert oracle.decode(np.frombuffer(ts, dtype=np.uint8), 1, flush_last=True)[0] == 11
    dec = efx.Decoder(2, TITLE_PICTURES, TITLE_PICTURES + 1, max_stream_bytes=cap)
    dec.upload(mains, efx.FORMAT_TS)
    dec.decode()
    assert [dec.picture_count(i) for i in range(2)] == [TITLE_PICTURES] * 2
    picks = np.stack([dec.export_host("i420", picture=p) for p in range(0, TITLE_PICTURES, TITLE_SPEED)], axis=1)
    want_f = dec.encode(picks, **opts).streams
    want_r = dec.encode(np.ascontiguousarray(picks[:, ::-1]), **opts).streams
    dec.close()
    assert fwd == want_f and rwd == want_r
