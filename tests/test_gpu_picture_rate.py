"""efx_encode_set_picture_rate on the device: every code's streams against the host build of the same headers
(tests/picture_rate_model.py) byte for byte, against the 30000/1001 Hz stream with only its headers rewritten, and decoded
by the test oracle and the compiled reference; the PTS wrap; continuation; rate control with every picture's own gain;
Decoder.make_poster; and a 24 Hz title directory of Decoder.make_title."""
import ctypes
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import conform_model as C
import encode_model as E
import encode_rate_model as R
import export_model as M
import oracle
import picture_rate_model as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = M.FRAME_BYTES
PTS0 = 129003
WRAP = 1 << 33
KW = dict(qscale=6, gop=3, search=3)
ARG, STATE = -1, -5


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return P.build(str(tmp_path_factory.mktemp("picture_rate_model")))


@pytest.fixture(scope="module")
def pics():
    return E.moving(7)


@pytest.fixture(scope="module")
def es4(tmp_path_factory, pics):
    """encode_model's 30000/1001 Hz elementary stream of the first 5 pictures and its reconstruction: computed once."""
    exe = E.build(str(tmp_path_factory.mktemp("enc_model")))
    return E.encode(exe, pics[:5], fmt=0, **KW)


def fnv_pictures(i420):
    from espflix_amd import gen
    return [gen.fnv1a64(s) for s in M.i420_to_strip(np.asarray(i420).reshape(-1, PIC))]


def decode_check(stream, fmt, recon, pts):
    """The oracle, and for transport streams the reference, return frames equal to recon and, with PES, the PTS."""
    a = np.frombuffer(stream, dtype=np.uint8)
    n, hashes, got_pts, frames = oracle.decode(a, fmt, flush_last=True, want_frames=True)
    assert n == len(recon) and np.array_equal(frames, M.i420_to_strip(recon))
    if fmt == 1:
        assert list(got_pts) == pts
        if oracle.have_ref():
            rh, rp, _ = oracle.ref_decode(a, flush_last=True)
            assert [int(h) for h in rh] == fnv_pictures(recon) and list(rp) == pts


@pytest.mark.parametrize("fmt", [0, 1], ids=["es", "ts"])
@pytest.mark.parametrize("code", range(1, 9))
def test_fixed_quantiser(efx, model, pics, es4, code, fmt):
    dec = efx.Decoder(1, 1)
    r = dec.encode(pics[None, :5], fmt=fmt, first_pts=PTS0, recon=True, fps=C.RATES[code], **KW)
    dec.close()
    want = P.encode(model, pics[:5], code=code, fmt=fmt, first_pts=PTS0, **KW)
    assert int(r.status[0]) == 0
    assert r.streams[0] == want.stream, "bytes differ from the host model"
    assert np.array_equal(r.recon[0], want.recon)
    es = r.streams[0] if fmt == 0 else R.ts_payload(r.streams[0])
    assert P.sequence_codes(es) == [code, code]
    if fmt == 0:
        # the slices do not depend on the rate: the 30000/1001 Hz stream with its rate nibbles and time codes rewritten
        assert r.streams[0] == P.rewrite_es(es4[0], code) and np.array_equal(r.recon[0], es4[1])
    pts = [PTS0 + C.pts_offset(code, k) for k in range(5)]
    if fmt == 1:
        assert P.ts_pts(r.streams[0]) == pts
    decode_check(r.streams[0], fmt, r.recon[0], pts)


def test_pts_wrap(efx, model, pics):
    """24000/1001 Hz from two pictures below 2^33: pictures 2 .. 4 carry the PTS modulo 2^33."""
    first = WRAP - C.pts_offset(1, 2)
    dec = efx.Decoder(1, 1)
    r = dec.encode(pics[None, :5], fmt=efx.FORMAT_TS, first_pts=first, recon=True, fps="24000/1001", **KW)
    dec.close()
    pts = [(first + C.pts_offset(1, k)) % WRAP for k in range(5)]
    assert pts[:3] == [WRAP - 7507, WRAP - 3754, 0] and pts[3:] == [3754, 7508]
    assert P.ts_pts(r.streams[0]) == pts
    assert r.streams[0] == P.encode(model, pics[:5], code=1, fmt=1, first_pts=first, **KW).stream
    decode_check(r.streams[0], 1, r.recon[0], pts)


def raw_encode(efx, dec, pictures, cont, first_pts=PTS0):
    """efx_encode as a C caller makes it, without the Python layer's efx_encode_set_picture_rate: one stream's bytes."""
    n = len(pictures)
    src, dst, meta = dec.alloc(n * PIC), dec.alloc(efx.encode_bound(efx.FORMAT_TS, n)), dec.alloc(32)
    src.upload(np.ascontiguousarray(pictures))
    o = efx._EncodeOpts(1, n, efx.FORMAT_TS, KW["qscale"], KW["gop"], KW["search"], 1 if cont else 0, first_pts, n * PIC,
                        efx.encode_bound(efx.FORMAT_TS, n))
    st = dec._lib.efx_encode(dec._ctx, ctypes.byref(o), src.ptr, dst.ptr, meta.ptr, meta.ptr + 16, None)
    assert st == 0, st
    dec.sync()
    length, status = (int(v) for v in meta.download(np.uint32, 8)[[0, 4]])
    assert status == 0
    out = dst.download(np.uint8, length).tobytes()
    for b in (src, dst, meta):
        b.free()
    return out


def test_continuation_keeps_the_rate(efx, model, pics):
    """3 + 4 pictures at 24000/1001 Hz equal one call of 7 (the 3753 / 3754 steps cross the boundary), whatever rate is set in
    between; the next fresh call takes that rate; a bad code is refused and changes nothing."""
    lib = efx.load_library()
    dec = efx.Decoder(1, 1)
    whole = dec.encode(pics[None], fmt=efx.FORMAT_TS, first_pts=PTS0, fps="24000/1001", **KW)
    want = P.encode(model, pics, code=1, fmt=1, first_pts=PTS0, **KW)
    assert whole.streams[0] == want.stream
    pts = P.ts_pts(whole.streams[0])
    assert [b - a for a, b in zip(pts, pts[1:])] == [3753, 3754, 3754, 3754, 3753, 3754]
    a = dec.encode(pics[None, :3], fmt=efx.FORMAT_TS, first_pts=PTS0, fps="24000/1001", **KW)
    b = dec.encode(pics[None, 3:], fmt=efx.FORMAT_TS, cont=True, fps=23.976, **KW)
    assert a.streams[0] + b.streams[0] == whole.streams[0]
    # ... through the C entry points: the rate set between the calls does not reach the continued stream
    assert lib.efx_encode_set_picture_rate(dec._ctx, 1) == 0
    a = raw_encode(efx, dec, pics[:3], cont=False)
    assert lib.efx_encode_set_picture_rate(dec._ctx, 3) == 0
    for bad in (0, 9, -1, 4096):
        assert lib.efx_encode_set_picture_rate(dec._ctx, bad) == ARG
    b = raw_encode(efx, dec, pics[3:], cont=True)
    assert a + b == whole.streams[0]
    fresh = raw_encode(efx, dec, pics[:3], cont=False)       # the new rate, which the refused codes left in place
    assert fresh == P.encode(model, pics[:3], code=3, fmt=1, first_pts=PTS0, **KW).stream
    # the Python layer: a keyword that is not given means 30000/1001, and cont refuses another rate
    plain = dec.encode(pics[None, :3], fmt=efx.FORMAT_TS, first_pts=PTS0, **KW)
    assert plain.streams[0] == P.encode(model, pics[:3], code=4, fmt=1, first_pts=PTS0, **KW).stream
    dec.encode(pics[None, :3], fmt=efx.FORMAT_TS, first_pts=PTS0, fps=25, **KW)
    with pytest.raises(ValueError):
        dec.encode(pics[None, 3:], fmt=efx.FORMAT_TS, cont=True, fps=24, **KW)
    with pytest.raises(ValueError):
        dec.encode(pics[None, :3], fmt=efx.FORMAT_TS, fps=15, **KW)
    c = dec.encode(pics[None, 3:], fmt=efx.FORMAT_TS, cont=True, **KW)
    assert P.ts_pts(c.streams[0]) == [PTS0 + 3600 * k for k in range(3, 7)]
    dec.close()
    # a fresh context runs at code 4
    dec = efx.Decoder(1, 1)
    assert raw_encode(efx, dec, pics[:3], cont=False) == plain.streams[0]
    dec.close()


@pytest.fixture(scope="module")
def clip(clips):
    """Pictures 24 .. 30 of the vmedia clip as the oracle decodes them: at 800 kbit/s the picture rate decides the
    quantisers."""
    n, _, _, frames = oracle.decode(clips["vmedia"], 1, flush_last=True, want_frames=True)
    assert n == 72
    return M.strip_to_i420(frames[24:31]).reshape(7, PIC)


@pytest.mark.parametrize("bitrate,vbv_bits", [(800_000, 120_000), (400_000, 100_000)])
@pytest.mark.parametrize("code", [2, 7])
def test_rate_control(efx, model, clip, code, bitrate, vbv_bits):
    """Bytes, quantisers and EFX_ENCODE_VBV equal the host model's; the buffer model of efx.h, restated in Python from the
    picture sizes with G_k = bitrate x (offset(k + 1) - offset(k)), ends at the host model's level; and the gain matters:
    at 800 kbit/s the quantisers are not those of 30000/1001 Hz, at 400 kbit/s the streams run into debt."""
    rate = dict(bitrate=bitrate, vbv_bits=vbv_bits, qmin=2, qmax=31)
    dec = efx.Decoder(1, 1)
    r = dec.encode(clip[None], fmt=efx.FORMAT_TS, first_pts=PTS0, recon=True, fps=C.RATES[code], **rate, **KW)
    # ... and continued: 3 + 4 pictures carry the level and the picture count that selects G_k
    a = dec.encode(clip[None, :3], fmt=efx.FORMAT_TS, first_pts=PTS0, fps=C.RATES[code], **rate, **KW)
    b = dec.encode(clip[None, 3:], fmt=efx.FORMAT_TS, cont=True, **rate, **KW)
    dec.close()
    want = P.encode(model, clip, code=code, fmt=1, first_pts=PTS0, **rate, **KW)
    print(f"code {code} at {bitrate} bit/s: q {[int(q) for q in r.qscales[0]]}, status {int(r.status[0])}, model level {want.level}")
    assert r.streams[0] == want.stream and np.array_equal(r.recon[0], want.recon)
    assert np.array_equal(r.qscales[0], want.qscales) and int(r.status[0]) == want.status
    assert a.streams[0] + b.streams[0] == r.streams[0] and int(a.status[0]) | int(b.status[0]) == want.status
    under, level = P.vbv(R.ts_picture_bytes(r.streams[0]), bitrate, vbv_bits, code)
    assert level == want.level and under == bool(want.status & R.ENCODE_VBV)
    at4 = P.encode(model, clip, code=4, fmt=1, first_pts=PTS0, **rate, **KW)
    if bitrate == 800_000:
        assert not np.array_equal(at4.qscales, want.qscales)
    else:  # (in debt from the second picture on, whatever the rate: qmax, and only the levels differ)
        assert want.status == R.ENCODE_VBV == efx.ENCODE_VBV and at4.level != want.level


def test_poster(efx):
    """make_poster of a 64 x 48 RGB image: one I picture at 24 Hz that decodes, with the flush load_poster relies on, to the
    encoder's reconstruction."""
    yy, xx = np.mgrid[0:48, 0:64]
    img = np.stack([4 * xx, 5 * yy, 2 * (xx + yy)], axis=-1).astype(np.uint8)
    dec = efx.Decoder(1, 1)
    poster = dec.make_poster(img)
    pic = dec.import_pictures(img[None])
    r = dec.encode(pic.reshape(1, 1, PIC), qscale=2, gop=1, fmt=efx.FORMAT_TS, fps=24, recon=True)
    small = dec.make_poster(img[None], qscale=9, fps=25, fit="letterbox")
    dec.close()
    assert poster == r.streams[0] and len(small) < len(poster)
    assert P.sequence_codes(R.ts_payload(poster)) == [2] and P.sequence_codes(R.ts_payload(small)) == [3]
    a = np.frombuffer(poster, dtype=np.uint8)
    n, _, pts, frames = oracle.decode(a, 1, flush_last=True, want_frames=True)
    assert n == 1 and list(pts) == [0] and np.array_equal(frames, M.i420_to_strip(r.recon[0]))
    assert oracle.decode(a, 1, flush_last=False)[0] == 0  # (without the flush the only picture stays in the decoder)
    if oracle.have_ref():
        rh, rp, _ = oracle.ref_decode(a, flush_last=True)
        assert [int(h) for h in rh] == fnv_pictures(r.recon[0]) and list(rp) == [0]


# ---- the title directory at 24 Hz ----------------------------------------------------------------------------------------
TITLE_PICTURES = 30


def title_inputs():
    pics = np.stack([E.moving(TITLE_PICTURES, seed=7), E.moving(TITLE_PICTURES, seed=11)])
    t = np.arange(468 * 128)  # 1.25 s of 48 kHz, in whole SBC frames
    pcm = np.stack([np.round(6000 * np.sin(2 * np.pi * f * t / 48000)).astype(np.int16) for f in (440, 1000)])
    yy, xx = np.mgrid[0:48, 0:64]
    poster = np.stack([4 * xx, 5 * yy, 2 * (xx + yy)], axis=-1).astype(np.uint8)
    return pics, pcm, poster


TITLE_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import test_gpu_picture_rate as T

    pics, pcm, poster = T.title_inputs()
    tp, tpcm = torch.from_numpy(pics).cuda(), torch.from_numpy(pcm).cuda()
    dec = efx.Decoder(3, 1, 2, device=torch.cuda.current_device(), max_stream_bytes=8 << 20)
    kw = dict(speed=15, qscale=8, gop=12, search=3, first_pts=T.PTS0)
    t24, st24 = dec.make_title(tp, tpcm, fps=24, poster=poster, **kw)
    t30, st30 = dec.make_title(tp, tpcm, **kw)
    video = dec.encode(tp, qscale=8, gop=12, search=3, first_pts=T.PTS0, fps=24, recon=True)
    # 15 Hz pictures conformed to 30 Hz: every picture twice
    up, st_up = dec.make_title(tp[:, :10], tpcm, fps=15, fps_out=30, **kw)
    refused = []
    for bad in (dict(fps=15), dict(fps=15, fps_out=15), dict(fps_out=30)):
        try:
            dec.make_title(tp[:, :10], tpcm, **bad, **kw)
        except ValueError:
            refused.append(True)
    poster_ts = dec.make_poster(poster)
    dec.close()
    pickle.dump((t24, st24, t30, st30, video.streams, video.recon.cpu().numpy(), up, st_up, refused, poster_ts), open(sys.argv[2], "wb"))
    print("make_title ok")
""")


@pytest.fixture(scope="module")
def titles(efx, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("make_title_24")
    script, out = tmp / "make_title.py", tmp / "titles.pkl"
    script.write_text(TITLE_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "make_title ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return pickle.load(open(out, "rb"))


def test_title_at_24_hz(efx, titles):
    """make_title(fps=24) on 2 streams x 30 pictures + 1.25 s of PCM: the video PES of all three streams step by 3750, the
    audio PES are where a 30000/1001 Hz title has them, video.idx is the index oracle's, and the reference decoder plays
    the title with the encoder's reconstruction."""
    t24, st24, t30, st30, video, recon, up, st_up, refused, poster_ts = titles
    assert (st24 == 0).all() and (st30 == 0).all() and (st_up == 0).all() and refused == [True] * 3
    assert [sorted(t) for t in t30] == [["video.idx", "video.ts", "video_fwd.ts", "video_rwd.ts"]] * 2
    assert [sorted(t) for t in t24] == [["poster.ts", "video.idx", "video.ts", "video_fwd.ts", "video_rwd.ts"]] * 2
    for i, t in enumerate(t24):
        assert t["poster.ts"] == poster_ts
        main, fwd, rwd = (t[k] for k in ("video.ts", "video_fwd.ts", "video_rwd.ts"))
        assert P.ts_pts(main) == [PTS0 + 3750 * k for k in range(TITLE_PICTURES)]
        assert P.ts_pts(fwd) == P.ts_pts(rwd) == [PTS0, PTS0 + 3750]
        for s in (main, fwd, rwd):
            assert set(P.sequence_codes(R.ts_payload(s))) == {2}
        audio = P.ts_pts(main, pid=0x101)
        assert len(audio) > 10 and audio == P.ts_pts(t30[i]["video.ts"], pid=0x101)
        assert P.ts_pts(t30[i]["video.ts"]) == [PTS0 + 3003 * k for k in range(TITLE_PICTURES)]
        three = [np.frombuffer(s, dtype=np.uint8) for s in (main, fwd, rwd)]
        assert t["video.idx"] == oracle.make_idx(three)
        if oracle.have_ref():
            assert np.array_equal(oracle.idx_masked(t["video.idx"]), oracle.idx_masked(oracle.ref_make_idx(three)))
        # the video PID's packets are encode(fps=24)'s, and they play as its reconstruction
        a = np.frombuffer(main, dtype=np.uint8).reshape(-1, 188)
        pid = ((a[:, 1].astype(int) & 0x1F) << 8) | a[:, 2]
        assert a[pid == 0x100].tobytes() == video[i]
        n, hashes, pts, _ = oracle.decode(three[0], 1, flush_last=True)
        assert n == TITLE_PICTURES and [int(h) for h in hashes] == fnv_pictures(recon[i])
        assert list(pts) == [PTS0 + 3750 * k for k in range(TITLE_PICTURES)]
        if oracle.have_ref():
            rh, rp, _ = oracle.ref_decode(three[0], flush_last=True)
            assert [int(h) for h in rh] == fnv_pictures(recon[i]) and list(rp) == list(pts)
    for t in up:
        assert P.ts_pts(t["video.ts"]) == [PTS0 + 3000 * k for k in range(20)]
        assert set(P.sequence_codes(R.ts_payload(t["video.ts"]))) == {5}
        n, hashes, _, _ = oracle.decode(np.frombuffer(t["video.ts"], dtype=np.uint8), 1, flush_last=True)
        assert n == 20
