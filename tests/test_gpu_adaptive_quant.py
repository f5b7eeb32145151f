"""Adaptive quantisation on the device (efx_encode_set_adaptive_quant: k_enc_aq and the per-macroblock quantisers of
k_enc_rows / write_slice) against the host build of the same arithmetic (tests/encode_aq_model.py) byte for byte --
streams, reconstruction, the maps of efx_encode_mb_quant, and under rate control the pictures' quantisers and the status.
tests/test_encode_aq_model.py checks the host model (the rule restated in NumPy, the oracle's parse of every macroblock's
quantiser, the anchors); equality with it carries those results to the device."""
import ctypes as C

import numpy as np
import pytest

import encode_aq_model as A
import encode_model as E
import encode_rate_model as R
import export_model as M
import oracle

pytestmark = pytest.mark.gpu

PIC = M.FRAME_BYTES
PTS0 = 129003
KW = dict(gop=12, search=7, first_pts=PTS0)
RATE = dict(bitrate=400_000, vbv_bits=250_000, qmin=3, qmax=31)


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return A.build(str(tmp_path_factory.mktemp("enc_aq_model")))


@pytest.fixture(scope="module")
def clip(clips):
    """vmedia's first twelve pictures (decoded on the host)."""
    _, _, _, frames = oracle.decode(clips["vmedia"], 1, flush_last=True, want_frames=True)
    return M.strip_to_i420(frames[:12]).reshape(12, PIC)


@pytest.fixture(scope="module")
def three(clip):
    """3 streams x 3 pictures: a golden clip's first pictures, the directed clip, noise."""
    noise = np.random.default_rng(2).integers(0, 249, size=(3, PIC)).astype(np.uint8)
    return np.stack([clip[:3], A.directed(3), noise])


@pytest.fixture(scope="module")
def host(model, three):
    """The host model's encodings, computed once per setting and never changed."""
    done = {}

    def get(i, q, s, fmt=1, search=7):
        key = (i, q, s, fmt, search)
        if key not in done:
            done[key] = A.encode(model, three[i], aq=s, qscale=q, fmt=fmt, **{**KW, "search": search})
        return done[key]
    return get


def device_maps(dec, n, P):
    return np.stack([np.stack([dec.encode_mb_quant(i, p) for p in range(P)]) for i in range(n)])


def same(r, maps, i, want, what):
    assert r.streams[i] == want.stream, f"{what}: bytes differ from the host model"
    assert np.array_equal(r.recon[i], want.recon), f"{what}: reconstruction differs from the host model"
    assert np.array_equal(maps[i], want.maps), f"{what}: the quantiser maps differ from the host model"
    assert int(r.status[i]) == want.status, (what, int(r.status[i]))


def decodes(efx, r, n, P, fmt):
    """efx_decode of the device's streams gives frames whose hashes are the reconstruction's."""
    from espflix_amd import gen
    dec = efx.Decoder(n, P, ring_depth=P + 1, max_stream_bytes=sum(len(s) for s in r.streams) + n * 4096)
    dec.upload([np.frombuffer(s, dtype=np.uint8) for s in r.streams], fmt)
    dec.decode()
    hashes = dec.frame_hashes()
    for i in range(n):
        assert dec.stream_status(i) == 0 and dec.picture_count(i) == P, (i, dec.stream_status(i), dec.picture_count(i))
        want = [gen.fnv1a64(s) for s in M.i420_to_strip(np.asarray(r.recon[i]))]
        assert [int(hashes[i, dec.picture_slot(p, i)]) for p in range(P)] == want, f"stream {i}"
    dec.close()


@pytest.mark.parametrize("q", [2, 8, 31])
@pytest.mark.parametrize("s", [64, 256])
def test_device_equals_host(efx, three, host, q, s):
    """1: three different streams in one call equal the host model stream by stream -- bytes, reconstruction, maps -- and
    efx_decode reads the streams back to the reconstruction (a quantiser coded differently from the one used shows
    here)."""
    dec = efx.Decoder(3, 1)
    r = dec.encode(three, fmt=efx.FORMAT_TS, recon=True, qscale=q, aq=s, **KW)
    maps = device_maps(dec, 3, 3)
    dec.close()
    assert maps.shape == (3, 3, 12, 22) and maps.dtype == np.uint8
    for i in range(3):
        same(r, maps, i, host(i, q, s), f"stream {i}, q {q}, strength {s}")
    assert len(np.unique(maps[1])) > 1 or q == 2
    decodes(efx, r, 3, 3, efx.FORMAT_TS)


@pytest.mark.parametrize("fmt,search", [(0, 7), (1, 15)])
def test_es_and_search_15(efx, three, host, fmt, search):
    """2: an elementary stream, and search 15 (f_code 2), once each."""
    dec = efx.Decoder(3, 1)
    r = dec.encode(three, fmt=fmt, recon=True, qscale=8, aq=256, **{**KW, "search": search})
    maps = device_maps(dec, 3, 3)
    dec.close()
    for i in range(3):
        same(r, maps, i, host(i, 8, 256, fmt, search), f"stream {i}, fmt {fmt}, search {search}")
    seen = A.check_stream(r.streams[1], fmt, maps[1], "the directed clip")
    assert seen == A.QUANT_TYPES, seen
    decodes(efx, r, 3, 3, fmt)


def test_rate_control(efx, model, clip, three):
    """3: efx_encode_rc, 1 stream x 12 pictures at 400 kbit/s into 250 000 bits, qmin 3: the model's bytes; qscale_out is
    the picture's quantiser, the one the model's controller chose, not a macroblock's."""
    pics = np.concatenate([clip[:9], three[1]])
    want = A.encode(model, pics, aq=256, qscale=8, fmt=1, **RATE, **KW)
    dec = efx.Decoder(1, 1)
    r = dec.encode(pics[None], fmt=efx.FORMAT_TS, recon=True, qscale=8, aq=256, **RATE, **KW)
    maps = device_maps(dec, 1, 12)
    dec.close()
    same(r, maps, 0, want, "rate control")
    assert np.array_equal(r.qscales[0], want.qscales), (r.qscales[0], want.qscales)
    assert maps.min() >= 3 and any(len(np.unique(m)) > 1 for m in maps[0])
    assert any((m != int(q)).any() for m, q in zip(maps[0], r.qscales[0]))
    decodes(efx, r, 1, 12, efx.FORMAT_TS)


def test_continuation(efx, model, clip, three):
    """4: 2 + 2 pictures with cont equal 4 at once; a setter call between the two does not change the continued streams."""
    pics = np.stack([np.concatenate([three[1][:2], clip[3:5]]), clip[:4], np.concatenate([clip[5:7], three[1][1:]])])
    dec = efx.Decoder(3, 1)
    whole = dec.encode(pics, recon=True, qscale=8, aq=64, **KW)
    whole_maps = device_maps(dec, 3, 4)
    a = dec.encode(pics[:, :2], recon=True, qscale=8, aq=64, **KW)
    a_maps = device_maps(dec, 3, 2)
    assert dec._lib.efx_encode_set_adaptive_quant(dec._ctx, C.byref(efx._AdaptiveQuant(256))) == 0
    b = dec.encode(pics[:, 2:], recon=True, qscale=8, aq=0, cont=True, **KW)
    b_maps = device_maps(dec, 3, 2)
    dec.close()
    for i in range(3):
        assert a.streams[i] + b.streams[i] == whole.streams[i], i
        assert np.array_equal(np.concatenate([a.recon[i], b.recon[i]]), whole.recon[i])
        assert np.array_equal(np.concatenate([a_maps[i], b_maps[i]]), whole_maps[i])
        want = A.encode(model, pics[i], aq=64, qscale=8, fmt=1, **KW)
        assert whole.streams[i] == want.stream and np.array_equal(whole_maps[i], want.maps)


def raw_encode(efx, dec, pics):
    """efx_encode as it is (qscale 8, TS), without the setter calls of Decoder.encode_to: (status, the streams' bytes)."""
    n, P = pics.shape[:2]
    stride = efx.encode_bound(efx.FORMAT_TS, P)
    src, dst, meta = dec.alloc(pics.size), dec.alloc(n * stride), dec.alloc(64)
    src.upload(np.ascontiguousarray(pics))
    o = efx._EncodeOpts(n, P, efx.FORMAT_TS, 8, KW["gop"], KW["search"], 0, PTS0, P * PIC, stride)
    st = dec._lib.efx_encode(dec._ctx, C.byref(o), src.ptr, dst.ptr, meta.ptr, meta.ptr + 16, None)
    dec.sync()
    lens = meta.download(np.uint32, n)
    out = dst.download(np.uint8, n * stride)
    for b in (src, dst, meta):
        b.free()
    return st, [out[i * stride:i * stride + int(lens[i])].tobytes() for i in range(n)]


def test_off_is_the_encoder_without_it(efx, three, tmp_path_factory):
    """5: a strength, then NULL: the bytes of a context that never set one (and of the plain host model);
    efx_encode_mb_quant then returns EFX_ERR_STATE."""
    plain = E.build(str(tmp_path_factory.mktemp("enc_model")))
    out = np.zeros(264, dtype=np.uint8)
    fresh = efx.Decoder(3, 1)
    st, never = raw_encode(efx, fresh, three)
    assert st == 0 and fresh._lib.efx_encode_mb_quant(fresh._ctx, 0, 0, out.ctypes.data) == -5
    fresh.close()
    dec = efx.Decoder(3, 1)
    assert dec._lib.efx_encode_mb_quant(dec._ctx, 0, 0, out.ctypes.data) == -5     # before the first encode
    on = dec.encode(three, qscale=8, aq=256, **KW)
    assert dec._lib.efx_encode_mb_quant(dec._ctx, 0, 0, out.ctypes.data) == 0 and out.min() >= 1
    assert dec._lib.efx_encode_set_adaptive_quant(dec._ctx, C.byref(efx._AdaptiveQuant(128))) == 0
    assert dec._lib.efx_encode_set_adaptive_quant(dec._ctx, None) == 0
    st, raw = raw_encode(efx, dec, three)
    assert st == 0 and dec._lib.efx_encode_mb_quant(dec._ctx, 0, 0, out.ctypes.data) == -5
    with pytest.raises(efx.EfxError) as e:
        dec.encode_mb_quant(0, 0)
    assert e.value.status == -5
    off = dec.encode(three, recon=True, qscale=8, aq=None, **KW)
    dec.close()
    for i in range(3):
        want, want_rec = E.encode(plain, three[i], qscale=8, **KW)
        assert never[i] == want and raw[i] == want
        assert off.streams[i] == want and np.array_equal(off.recon[i], want_rec)
    assert on.streams[1] != never[1]


def test_errors(efx, three):
    """6: a strength outside 0 .. 256 is EFX_ERR_ARG and the earlier setting stays; a stream or picture outside the
    latest call, or NULL, is EFX_ERR_ARG."""
    dec = efx.Decoder(3, 1)
    setter = lambda s: dec._lib.efx_encode_set_adaptive_quant(dec._ctx, C.byref(efx._AdaptiveQuant(s)))
    assert setter(64) == 0
    for bad in (-1, 257, 1 << 20):
        assert setter(bad) == -1, bad
    st, _ = raw_encode(efx, dec, three[:2])
    assert st == 0
    got = device_maps(dec, 2, 3)                      # the earlier setting holds: strength 64
    for i in range(2):
        assert np.array_equal(got[i], np.stack([A.mq_map(p, 8, 64) for p in three[i]])), i
    out = np.zeros(264, dtype=np.uint8)
    for stream, picture, ptr in ((2, 0, out.ctypes.data), (-1, 0, out.ctypes.data), (0, 3, out.ctypes.data), (0, -1, out.ctypes.data),
                                 (0, 0, None)):
        assert dec._lib.efx_encode_mb_quant(dec._ctx, stream, picture, ptr) == -1, (stream, picture)
    assert dec._lib.efx_encode_mb_quant(None, 0, 0, out.ctypes.data) == -1
    assert dec._lib.efx_encode_set_adaptive_quant(None, None) == -1
    for ok in (0, 1, 256):
        assert setter(ok) == 0, ok
    for bad in (dict(aq=-1), dict(aq=257)):
        with pytest.raises(efx.EfxError) as e:
            dec.encode(three[:, :1], qscale=8, **bad, **KW)
        assert e.value.status == -1, bad
    dec.close()


def test_full_stream_zeroes_the_map(efx, three):
    """A picture that does not fit is not written: its map reads all zero."""
    dec = efx.Decoder(1, 1)
    whole = dec.encode(three[1][None], qscale=8, aq=256, **KW)
    sizes = R.ts_picture_bytes(whole.streams[0])
    room = (sum(sizes[:2]) + 15) // 16 * 16
    assert len(sizes) == 3 and room < sum(sizes)
    r = dec.encode(three[1][None], qscale=8, aq=256, dst_stride=room, **KW)
    maps = device_maps(dec, 1, 3)
    dec.close()
    assert int(r.status[0]) & efx.ENCODE_FULL and r.streams[0] == whole.streams[0][:sum(sizes[:2])]
    assert maps[0, :2].min() >= 1 and not maps[0, 2].any()


def test_batch_independence(efx, three, host):
    """7: the directed clip's bytes are the same alone and in the batch."""
    dec = efx.Decoder(3, 1)
    alone = dec.encode(three[1][None], recon=True, qscale=8, aq=256, **KW)
    maps = device_maps(dec, 1, 3)
    dec.close()
    same(alone, maps, 0, host(1, 8, 256), "the directed clip alone")


def test_python_round_trip(efx, three):
    """8: encode(aq=True) is strength 256; its streams decode to its reconstruction."""
    dec = efx.Decoder(3, 1)
    t = dec.encode(three, recon=True, qscale=8, aq=True, **KW)
    t_maps = device_maps(dec, 3, 3)
    n = dec.encode(three, recon=True, qscale=8, aq=256, **KW)
    dec.close()
    assert efx.AQ_DEFAULT == 256 and t.streams == n.streams
    for i in range(3):
        assert np.array_equal(t_maps[i], np.stack([A.mq_map(p, 8, 256) for p in three[i]]))
    decodes(efx, t, 3, 3, efx.FORMAT_TS)
