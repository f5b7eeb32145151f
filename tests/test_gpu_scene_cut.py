"""Scene cuts on the device (efx_encode_set_scene_cut: k_enc_cut and the picture-type rule of enc_cut.h in k_enc_rows /
k_enc_pack) against the host build of the same arithmetic (tests/encode_cut_model.py) byte for byte -- streams, status,
reconstruction, quantisers and efx_encode_picture_info -- in one launch that codes an I picture in one stream and a P
picture in another.  tests/test_encode_cut_model.py checks the host model's behaviour (which pictures are cuts, the
headers, decodability); equality with it carries those results to the device."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import encode_cut_model as CM
import encode_model as E
import encode_rate_model as R
import export_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = M.FRAME_BYTES
PTS0 = 129003
RATE = dict(bitrate=400_000, vbv_bits=250_000, qmin=3, qmax=31)
KW = dict(qscale=8, gop=12, search=7, first_pts=PTS0)
CUT = dict(scene_cut=CM.THRESHOLD, min_gop=6)
I_AT = ([0, 12, 18, 30], [0, 12, 19, 31], [0, 12, 20, 32])   # X, vmedia[:36], the pan with its cut at 20


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return CM.build(str(tmp_path_factory.mktemp("enc_cut_model")))


@pytest.fixture(scope="module")
def three(efx, clips):
    """X, vmedia[:36] (the clips as the library decodes and exports them) and the synthetic pan."""
    out = {}
    for name in ("splash", "vmedia"):
        dec = efx.Decoder(1, 100, ring_depth=101, max_stream_bytes=len(clips[name]) + 4096)
        dec.upload([clips[name]], efx.FORMAT_TS)
        dec.decode()
        out[name] = np.concatenate([dec.export_host("i420", picture=p) for p in range(dec.picture_count(0))])
        dec.close()
    return np.stack([R.sources(out)["X"], out["vmedia"].reshape(-1, PIC)[:36], CM.pan()])


@pytest.fixture(scope="module")
def host(model, three):
    """The host model's encodings, computed once per (stream, format, rate control) and never changed."""
    done = {}

    def get(i, fmt, rc):
        if (i, fmt, rc) not in done:
            done[i, fmt, rc] = CM.encode(model, three[i], fmt=fmt, **(RATE if rc else {}), **CUT, **KW)
        return done[i, fmt, rc]
    return get


@pytest.fixture(scope="module")
def device_ts(efx, three):
    dec = efx.Decoder(3, 1)
    r = dec.encode(three, fmt=efx.FORMAT_TS, recon=True, **CUT, **KW)
    dec.close()
    return r


def same(r, i, want, what, rc=False):
    assert list(r.types[i]) == list(want.types), (what, list(r.types[i]), list(want.types))
    assert np.array_equal(r.cut_scores[i, :, 0], want.cut_i) and np.array_equal(r.cut_scores[i, :, 1], want.cut_p), \
        f"{what}: the sums differ from the host model"
    assert r.streams[i] == want.stream, f"{what}: bytes differ from the host model"
    assert int(r.status[i]) == want.status, (what, int(r.status[i]), want.status)
    assert np.array_equal(r.recon[i], want.recon), f"{what}: reconstruction differs from the host model"
    if rc:
        assert np.array_equal(r.qscales[i], want.qscales), (what, r.qscales[i], want.qscales)


@pytest.mark.parametrize("fmt,rc", [(1, False), (0, False), (1, True), (0, True)])
def test_device_equals_host(efx, three, host, device_ts, fmt, rc):
    """1: three streams in one call -- from picture 18 on their pictures have different types -- equal the host model
    stream by stream, and so does each stream encoded alone."""
    if fmt == 1 and not rc:
        r = device_ts
    else:
        dec = efx.Decoder(3, 1)
        r = dec.encode(three, fmt=fmt, recon=True, **(RATE if rc else {}), **CUT, **KW)
        dec.close()
    assert r.types.shape == (3, 36) and r.types.dtype == np.uint8 and r.cut_scores.shape == (3, 36, 2)
    for i in range(3):
        same(r, i, host(i, fmt, rc), f"stream {i} of 3, fmt {fmt}, rc {rc}", rc)
        assert [k for k in range(36) if int(r.types[i, k]) != efx.PICTURE_P] == I_AT[i]
        assert int(r.types[i, I_AT[i][2]]) == efx.PICTURE_CUT_I
    dec = efx.Decoder(1, 1)
    for i in range(3):
        alone = dec.encode(three[i][None], fmt=fmt, recon=True, **(RATE if rc else {}), **CUT, **KW)
        same(alone, 0, host(i, fmt, rc), f"stream {i} alone, fmt {fmt}, rc {rc}", rc)
    dec.close()


def test_option_off(efx, three, tmp_path_factory):
    """2: with the option off, or never set, encode() returns the bytes of the encoder without scene cuts: the existing
    host models.  The picture info then holds the periodic types and zero sums."""
    const = E.build(str(tmp_path_factory.mktemp("enc_model")))
    rc = R.build(str(tmp_path_factory.mktemp("enc_rate_model")))
    pics = three[0]
    want, want_rec = E.encode(const, pics, **KW)
    want_rc = R.encode(rc, pics, **RATE, **KW)
    dec = efx.Decoder(1, 1)
    never = dec.encode(pics[None], recon=True, **KW)
    dec.encode(pics[None, :2], **CUT, **KW)
    off = dec.encode(pics[None], recon=True, scene_cut=0, **KW)
    off_rc = dec.encode(pics[None], recon=True, scene_cut=None, **RATE, **KW)
    dec.close()
    for r in (never, off):
        assert r.streams[0] == want and np.array_equal(r.recon[0], want_rec)
        assert list(r.types[0]) == [1 if k % 12 == 0 else 2 for k in range(36)] and not r.cut_scores.any()
    assert off_rc.streams[0] == want_rc.stream and np.array_equal(off_rc.recon[0], want_rc.recon)
    assert np.array_equal(off_rc.qscales[0], want_rc.qscales) and int(off_rc.status[0]) == want_rc.status


def test_continuation(efx, three, device_ts):
    """3: 7 + 11 + 18 pictures with cont equal the single call; X's cut is the first picture of the third call."""
    dec = efx.Decoder(3, 1)
    parts, at = [], 0
    for n in (7, 11, 18):
        parts.append(dec.encode(three[:, at:at + n], fmt=efx.FORMAT_TS, recon=True, cont=at > 0, **CUT, **KW))
        at += n
    dec.close()
    for i in range(3):
        assert b"".join(p.streams[i] for p in parts) == device_ts.streams[i]
        assert np.array_equal(np.concatenate([p.recon[i] for p in parts]), device_ts.recon[i])
        assert np.array_equal(np.concatenate([p.types[i] for p in parts]), device_ts.types[i])
        assert np.array_equal(np.concatenate([p.cut_scores[i] for p in parts]), device_ts.cut_scores[i])
    assert int(parts[2].types[0, 0]) == efx.PICTURE_CUT_I


def test_efx_decode(efx, device_ts):
    """4: efx_decode of the device's streams: status 0, ring frames equal to the reconstruction."""
    from espflix_amd import gen
    streams, recons = device_ts.streams, device_ts.recon
    dec = efx.Decoder(3, 36, ring_depth=37, max_stream_bytes=sum(len(s) for s in streams) + 3 * 4096)
    dec.upload([np.frombuffer(s, dtype=np.uint8) for s in streams], efx.FORMAT_TS)
    dec.decode()
    hashes = dec.frame_hashes()
    for i in range(3):
        assert dec.stream_status(i) == 0 and dec.picture_count(i) == 36
        want = [gen.fnv1a64(s) for s in M.i420_to_strip(recons[i])]
        assert [int(hashes[i, dec.picture_slot(p, i)]) for p in range(36)] == want, f"stream {i}"
        assert [dec.picture_pts(i, p) for p in (0, 35)] == [PTS0, PTS0 + 35 * 3003]
    dec.close()


def test_index_lists_the_cut(efx, three, device_ts):
    """5: efx_index_streams takes the cut's sequence header as a seek point: the packet picture 18 of X starts at is among
    the index entries (and is not when the stream was made without scene cuts)."""
    dec = efx.Decoder(1, 1, max_stream_bytes=1 << 20)
    plain = dec.encode(three[0][None], **KW).streams[0]
    got = {}
    for name, ts in (("cut", device_ts.streams[0]), ("plain", plain)):
        packet = sum(R.ts_picture_bytes(ts)[:18]) // 188
        rec, samples = dec.index_streams([ts])[0]
        got[name] = packet in [int(s) for s in samples]
        a = np.frombuffer(ts, dtype=np.uint8).reshape(-1, 188)
        assert a[packet, 1] & 0x40, name
        assert (bytes(a[packet, 4:]).find(b"\x00\x00\x01\xb3") >= 0) == (name == "cut")
    dec.close()
    assert got == {"cut": True, "plain": False}, got


def raw_encode(efx, dec, pics, cont=0):
    """efx_encode as it is, without the setter calls of Decoder.encode_to: the types of one stream's pictures."""
    n = len(pics)
    src, dst, meta = dec.alloc(pics.size), dec.alloc(efx.encode_bound(efx.FORMAT_TS, n)), dec.alloc(64)
    src.upload(np.ascontiguousarray(pics))
    o = efx._EncodeOpts(1, n, efx.FORMAT_TS, 8, 12, 7, cont, PTS0, n * PIC, efx.encode_bound(efx.FORMAT_TS, n))
    st = dec._lib.efx_encode(dec._ctx, C.byref(o), src.ptr, dst.ptr, meta.ptr, meta.ptr + 16, None)
    types = [int(t) for t in dec.encode_picture_info(1)["type"][0]] if st == 0 else None
    for b in (src, dst, meta):
        b.free()
    return st, types


def test_errors(efx, three):
    """6: settings out of range are EFX_ERR_ARG and the earlier setting holds; a setter call between a cont = 0 call and
    its continuation does not change the continued streams; no picture info before the first encode."""
    x = three[0]
    dec = efx.Decoder(1, 1)
    setter = lambda t, m: dec._lib.efx_encode_set_scene_cut(dec._ctx, C.byref(efx._SceneCut(t, m)))
    assert dec._lib.efx_encode_picture_info(dec._ctx, 0, None, 0) == -5
    with pytest.raises(efx.EfxError) as e:
        dec.encode_picture_info(1)
    assert e.value.status == -5
    assert setter(CM.THRESHOLD, 6) == 0
    for bad in ((-1, 6), (257, 6), (CM.THRESHOLD, 0), (CM.THRESHOLD, 256)):
        assert setter(*bad) == -1, bad
    st, types = raw_encode(efx, dec, x[:24])            # the earlier setting holds: the cut at 18 is found
    assert st == 0 and [k for k, t in enumerate(types) if t != 2] == [0, 12, 18] and types[18] == 5
    for ok in ((1, 1), (256, 255), (0, 1)):
        assert setter(*ok) == 0, ok
    assert dec._lib.efx_encode_set_scene_cut(dec._ctx, None) == 0
    st, types = raw_encode(efx, dec, x[:24])            # NULL: off
    assert st == 0 and [k for k, t in enumerate(types) if t != 2] == [0, 12]
    for bad in (dict(scene_cut=-1), dict(scene_cut=257), dict(scene_cut=CM.THRESHOLD, min_gop=0), dict(scene_cut=CM.THRESHOLD, min_gop=256)):
        with pytest.raises(efx.EfxError) as e:
            dec.encode(x[None, :2], **bad, **KW)
        assert e.value.status == -1, bad
    # the streams started with scene cuts keep them, whatever is set before the continuation -- and the reverse
    whole = dec.encode(x[None], **CUT, **KW)
    first = dec.encode(x[None, :7], **CUT, **KW)
    assert dec._lib.efx_encode_set_scene_cut(dec._ctx, None) == 0
    rest = dec.encode(x[None, 7:], cont=True, **KW)
    assert first.streams[0] + rest.streams[0] == whole.streams[0]
    assert list(first.types[0]) + list(rest.types[0]) == list(whole.types[0])
    plain = dec.encode(x[None], **KW)
    first = dec.encode(x[None, :7], **KW)
    assert setter(CM.THRESHOLD, 6) == 0
    rest = dec.encode(x[None, 7:], cont=True, **CUT, **KW)
    assert first.streams[0] + rest.streams[0] == plain.streams[0] and not rest.cut_scores.any()
    assert dec._lib.efx_encode_picture_info(dec._ctx, 1, None, 0) == -1      # a stream the latest call did not have
    assert dec._lib.efx_encode_picture_info(dec._ctx, 0, None, 4) == -1      # nowhere to write
    assert dec._lib.efx_encode_picture_info(dec._ctx, 0, None, 0) == 29      # the count alone
    dec.close()


TITLE_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx

    pics = np.load(sys.argv[2])
    pcm = np.zeros((1, 57600), dtype=np.int16)   # 1.2 s of silence: 450 SBC frames of 128 samples
    tp, tpcm = torch.from_numpy(pics).cuda(), torch.from_numpy(pcm).cuda()
    dec = efx.Decoder(3, 1, 2, device=torch.cuda.current_device(), max_stream_bytes=8 << 20)
    kw = dict(speed=3, qscale=8, gop=12, search=3, first_pts=129003)
    cut, st_cut = dec.make_title(tp, tpcm, scene_cut=True, **kw)
    plain, st_plain = dec.make_title(tp, tpcm, **kw)
    video = dec.encode(tp, scene_cut=True, **{k: v for k, v in kw.items() if k != "speed"})
    dec.close()
    pickle.dump((cut, st_cut, plain, st_plain, video.streams, video.types), open(sys.argv[3], "wb"))
    print("make_title ok")
""")


def test_make_title(efx, three, tmp_path):
    """7: make_title(scene_cut=True) on X plus silence: video.ts carries the picture types of the cut rule (its video
    packets are encode(scene_cut=True)'s bytes); the trick streams are those made without the option."""
    script, src, out = tmp_path / "make_title.py", tmp_path / "x.npy", tmp_path / "titles.pkl"
    script.write_text(TITLE_CHILD)
    np.save(src, three[:1])
    r = subprocess.run([sys.executable, str(script), ROOT, str(src), str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "make_title ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    cut, st_cut, plain, st_plain, video, types = pickle.load(open(out, "rb"))
    assert (st_cut == 0).all() and (st_plain == 0).all()
    assert [k for k in range(36) if int(types[0, k]) != 2] == [0, 12, 18, 30] and int(types[0, 18]) == 5
    a = np.frombuffer(cut[0]["video.ts"], dtype=np.uint8).reshape(-1, 188)
    pid = ((a[:, 1].astype(int) & 0x1F) << 8) | a[:, 2]
    assert a[pid == 0x100].tobytes() == video[0]
    CM.check_headers(R.ts_payload(cut[0]["video.ts"]), types[0], "video.ts")
    assert cut[0]["video.ts"] != plain[0]["video.ts"]
    for k in ("video_fwd.ts", "video_rwd.ts"):
        assert cut[0][k] == plain[0][k], k
