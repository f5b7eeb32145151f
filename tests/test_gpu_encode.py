"""efx_encode (k_encode): I420 pictures in device memory -> MPEG-1 ES / TS on the device.  Every stream must decode with
efx_decode, the test oracle and (where built) the reference to exactly the reconstruction the encoder reports, and its bytes
must be those of the host build of the encoder's arithmetic (tests/encode_model.py) at every search radius.  Its search and
mode decisions must be those of the exhaustive search model and its quality that of the float64 yardstick encoder
(tests/encode_float.py; tests/test_encode_yardstick.py holds the same checks for the host build)."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import common
import encode_float as F
import encode_model as E
import export_model as M
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = M.FRAME_BYTES
PTS0 = 129003


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return E.build(str(tmp_path_factory.mktemp("enc_model")))


@pytest.fixture(scope="module")
def clip_pictures(efx, clips):
    """Every picture of the two clips, decoded by the library and exported as I420."""
    out = {}
    for name in ("splash", "vmedia"):
        dec = efx.Decoder(1, 100, ring_depth=101, max_stream_bytes=len(clips[name]) + 4096)
        dec.upload([clips[name]], efx.FORMAT_TS)
        dec.decode()
        n = dec.picture_count(0)
        out[name] = np.concatenate([dec.export_host("i420", picture=p) for p in range(n)])
        dec.close()
    assert len(out["splash"]) == 99 and len(out["vmedia"]) == 72
    return out


def fnv_pictures(i420):
    from espflix_amd import gen
    strips = M.i420_to_strip(np.asarray(i420).reshape(-1, PIC))
    return [gen.fnv1a64(s) for s in strips]


def efx_decode_check(efx, streams, fmt, recons):
    """efx_decode of every stream: status 0, every picture, ring frames equal to the reconstruction (FNV-1a-64), and the
    exported I420 of the last picture equal to it bit for bit."""
    P = max(len(r) for r in recons)
    dec = efx.Decoder(len(streams), P, ring_depth=P + 1, max_stream_bytes=sum(len(s) for s in streams) + 4096 * len(streams))
    dec.upload([np.frombuffer(s, dtype=np.uint8) for s in streams], fmt)
    dec.decode()
    hashes = dec.frame_hashes()
    for i, rec in enumerate(recons):
        assert dec.stream_status(i) == 0 and dec.picture_count(i) == len(rec), (i, dec.stream_status(i), dec.picture_count(i))
        want = fnv_pictures(rec)
        got = [int(hashes[i, dec.picture_slot(p, i)]) for p in range(len(rec))]
        assert got == want, f"stream {i}: decoded pictures differ from the reconstruction"
    last = len(recons[0]) - 1
    img = dec.export_host("i420", n_streams=1, picture=last)
    assert np.array_equal(img[0], recons[0][last])
    dec.close()


def oracle_check(stream, fmt, recon, first_pts=PTS0):
    n, _, pts, frames = oracle.decode(np.frombuffer(stream, dtype=np.uint8), fmt, flush_last=True, want_frames=True)
    assert n == len(recon)
    assert np.array_equal(frames, M.i420_to_strip(recon))
    if fmt == 1:
        assert list(pts) == [first_pts + 3003 * k for k in range(n)]


def ref_check(ts, recon, first_pts=PTS0):
    if not oracle.have_ref():
        return
    hashes, pts, _ = oracle.ref_decode(np.frombuffer(ts, dtype=np.uint8), flush_last=True)
    assert [int(h) for h in hashes] == fnv_pictures(recon)
    assert list(pts) == [first_pts + 3003 * k for k in range(len(recon))]


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("qscale,search", [(2, 7), (8, 7), (31, 7), (2, 15), (8, 15), (31, 15)])
def test_clip_round_trip(efx, model, clip_pictures, fmt, qscale, search):
    """1 (a)-(c): both clips, every picture, decoded by efx_decode, the oracle and the reference to the reconstruction."""
    dec = efx.Decoder(1, 1)
    streams, recons = [], []
    for name in ("splash", "vmedia"):
        pics = clip_pictures[name]
        r = dec.encode(pics[None], qscale=qscale, gop=12, search=search, fmt=fmt, first_pts=PTS0, recon=True)
        assert r.status[0] == 0
        streams.append(r.streams[0])
        recons.append(r.recon[0])
        oracle_check(r.streams[0], fmt, r.recon[0])
        if fmt == 1:
            ref_check(r.streams[0], r.recon[0])
        if name == "vmedia" and qscale == 8:
            want, want_rec = E.encode(model, pics, gop=12, qscale=qscale, search=search, fmt=fmt, first_pts=PTS0)
            assert r.streams[0] == want and np.array_equal(r.recon[0], want_rec), "device and host encoders differ"
    dec.close()
    efx_decode_check(efx, streams[:1], fmt, recons[:1])
    efx_decode_check(efx, streams[1:], fmt, recons[1:])


def test_quality_follows_qscale(efx, clip_pictures):
    dec = efx.Decoder(1, 1)
    pics = clip_pictures["vmedia"]
    psnr, size = {}, {}
    for q in (2, 4, 8, 31):
        r = dec.encode(pics[None], qscale=q, gop=12, search=7, recon=True)
        psnr[q], size[q] = E.luma_psnr(pics, r.recon[0]), len(r.streams[0])
    dec.close()
    print("vmedia luma PSNR / bytes per picture:", {q: (round(psnr[q], 2), size[q] / len(pics)) for q in psnr})
    assert psnr[2] >= psnr[8] >= psnr[31] and size[2] >= size[8] >= size[31]
    assert psnr[4] >= 32.0


def test_search_finds_motion(efx, model):
    pics = E.moving(12)
    dec = efx.Decoder(1, 1)
    r7 = dec.encode(pics[None], qscale=8, gop=12, search=7, fmt=0, recon=True)
    r0 = dec.encode(pics[None], qscale=8, gop=12, search=0, fmt=0, recon=True)
    dec.close()
    assert 2 * len(r7.streams[0]) <= len(r0.streams[0]), (len(r7.streams[0]), len(r0.streams[0]))
    for r, s in ((r7, 7), (r0, 0)):
        oracle_check(r.streams[0], 0, r.recon[0])
        want, _ = E.encode(model, pics, gop=12, qscale=8, search=s, fmt=0)
        assert r.streams[0] == want
    # search 0 is the zero vector only; search 7 finds full- and half-pel motion within +-7.5 pels
    v0 = [(h, v) for _, _, intra, _, h, v in E.p_vectors(r0.streams[0], 0) if not intra]
    v7 = [(h, v) for _, _, intra, _, h, v in E.p_vectors(r7.streams[0], 0) if not intra]
    assert v0 and all(h == 0 and v == 0 for h, v in v0)
    assert all(abs(h) <= 15 and abs(v) <= 15 for h, v in v7) and any(h & 1 or v & 1 for h, v in v7)


@pytest.mark.parametrize("search", range(16))
def test_radius_matrix(efx, model, search):
    """Every search radius (each gives k_enc_rows another window side, fill width and lane stride; 8 switches to
    forward_f_code 2) at qscale 1, 5 and 31 on the source whose vectors reach the window's edge, and the noise pictures
    at qscale 5: the device's bytes and reconstruction are the host model's, the oracle decodes the stream to the
    reconstruction, and the largest |h| and |v| of the inter macroblocks are 2 R + 1 (search 0: the zero vector)."""
    big = F.big_motion(5)
    dec = efx.Decoder(1, 1)
    for name, pics, q, fmt in (("big_motion", big, 1, 0), ("big_motion", big, 5, 1), ("big_motion", big, 31, 0),
                               ("noise", E.noise(), 5, 1)):
        r = dec.encode(pics[None], qscale=q, gop=12, search=search, fmt=fmt, first_pts=PTS0, recon=True)
        assert r.status[0] == 0
        want, want_rec = E.encode(model, pics, gop=12, qscale=q, search=search, fmt=fmt, first_pts=PTS0)
        assert r.streams[0] == want, f"{name} q {q}: device and host streams differ"
        assert np.array_equal(r.recon[0], want_rec), f"{name} q {q}: device and host reconstructions differ"
        oracle_check(r.streams[0], fmt, r.recon[0])
        if name == "big_motion":
            vec = [(h, v) for _, _, intra, _, h, v in E.p_vectors(r.streams[0], fmt) if not intra]
            reach = 2 * search + 1 if search else 0
            assert vec and max(abs(h) for h, _ in vec) == reach and max(abs(v) for _, v in vec) == reach, (q, reach)
    dec.close()


@pytest.mark.parametrize("search", [1, 6, 8, 14, 15])
def test_search_decisions_are_the_models(efx, search):
    """Every macroblock of every P picture of the device's streams: (intra, h, v) equals the exhaustive search model's
    (encode_float.decisions), with the device's own previous reconstruction as the reference picture.  Exact."""
    dec = efx.Decoder(1, 1)
    total = 0
    for pics in (F.big_motion(5), E.checkerboard(3), E.flat(3, 90)):
        r = dec.encode(pics[None], qscale=5, gop=len(pics), search=search, fmt=0, recon=True)
        assert r.status[0] == 0
        total += E.check_decisions(r.streams[0], 0, pics, r.recon[0], len(pics), search)
    dec.close()
    assert total == 264 * 8


@pytest.mark.parametrize("q", E.QUALITY_Q)
def test_quality_against_the_float_yardstick(efx, clip_pictures, q):
    """splash and vmedia (pictures 14..25) and the moving texture in one batch call, gop 4: the device's mean luma PSNR of
    the I pictures and of the P pictures is at least the float64 yardstick's (tests/golden/encode_psnr.json) less the
    recorded margin, a quarter of the yardstick's own step to the neighbouring qscale."""
    record = json.load(open(E.PSNR_JSON))
    sources = E.quality_sources(clip_pictures)
    dec = efx.Decoder(len(sources), 1)
    r = dec.encode(np.stack(list(sources.values())), qscale=q, gop=E.QUALITY_GOP, search=E.QUALITY_SEARCH, fmt=0, recon=True)
    dec.close()
    assert (r.status == 0).all()
    failures = []
    for i, (name, pics) in enumerate(sources.items()):
        failures += E.check_quality(record, name, q, pics, r.recon[i], "device")
    assert not failures, failures


@pytest.mark.parametrize("name", ["checker_q1", "noise", "flat0", "flat255"])
def test_domain_edges(efx, model, name):
    pics = {"checker_q1": E.checkerboard(4), "noise": common.random_frames(11).reshape(2, -1)[:, :PIC],
            "flat0": E.flat(3, 0), "flat255": E.flat(3, 255)}[name]
    q = 1 if name == "checker_q1" else 5
    dec = efx.Decoder(1, 1)
    for gop, search, n in ((12, 15, len(pics)), (1, 0, len(pics)), (12, 7, 1), (2, 0, len(pics))):
        r = dec.encode(pics[None, :n], qscale=q, gop=gop, search=search, fmt=1, first_pts=PTS0, recon=True)
        assert r.status[0] == 0
        oracle_check(r.streams[0], 1, r.recon[0])
        want, _ = E.encode(model, pics[:n], gop=gop, qscale=q, search=search, fmt=1, first_pts=PTS0)
        assert r.streams[0] == want
        efx_decode_check(efx, r.streams, 1, [r.recon[0]])
    dec.close()


@pytest.mark.parametrize("gop", [12, 10])
@pytest.mark.parametrize("fmt", [0, 1])
def test_continuation(efx, clip_pictures, gop, fmt):
    pics = np.stack([clip_pictures["splash"][:24], clip_pictures["vmedia"][:24]])
    dec = efx.Decoder(2, 1)
    whole = dec.encode(pics, gop=gop, fmt=fmt, first_pts=PTS0, recon=True)
    a = dec.encode(pics[:, :12], gop=gop, fmt=fmt, first_pts=PTS0, recon=True)
    b = dec.encode(pics[:, 12:], gop=gop, fmt=fmt, cont=True, recon=True)
    for i in range(2):
        assert a.streams[i] + b.streams[i] == whole.streams[i]
        assert np.array_equal(np.concatenate([a.recon[i], b.recon[i]]), whole.recon[i])
    oracle_check(whole.streams[0], fmt, whole.recon[0])
    # the EFX_ERR_STATE cases
    fresh = efx.Decoder(2, 1)
    with pytest.raises(efx.EfxError) as e:
        fresh.encode(pics[:, :2], gop=gop, fmt=fmt, cont=True)
    assert e.value.status == -5
    fresh.close()
    for kw in ({"gop": gop + 1, "fmt": fmt}, {"gop": gop, "fmt": 1 - fmt}):
        with pytest.raises(efx.EfxError) as e:
            dec.encode(pics[:, :2], cont=True, **kw)
        assert e.value.status == -5
    with pytest.raises(efx.EfxError) as e:
        dec.encode(pics[:1, :2], gop=gop, fmt=fmt, cont=True)
    assert e.value.status == -5
    # a stream that filled its region is not continued
    assert dec.encode(pics[:, :4], gop=gop, fmt=fmt, dst_stride=1024).status[0] == efx.ENCODE_FULL
    with pytest.raises(efx.EfxError) as e:
        dec.encode(pics[:, 4:6], gop=gop, fmt=fmt, cont=True)
    assert e.value.status == -5
    dec.close()


def test_cont_after_a_full_call_and_a_fresh_start(efx):
    """A call that filled a region, then a fresh call and, queued right behind it without a sync, a continuation: the
    continuation belongs to the fresh streams and is accepted, and the two calls make one stream."""
    pics = np.stack([E.moving(8, seed=s) for s in (4, 5)])
    dec = efx.Decoder(2, 1)
    whole = dec.encode(pics, fmt=1, first_pts=PTS0)
    assert dec.encode(pics[:, :4], fmt=1, dst_stride=1024).status[0] == efx.ENCODE_FULL  # (synchronised)
    n, half, stride = 2, 4 * PIC, 1 << 20
    src = dec.alloc(pics.size)
    src.upload(np.ascontiguousarray(pics))
    out = [dec.alloc(n * stride) for _ in range(2)]
    meta = [dec.alloc(64) for _ in range(2)]
    for k in range(2):
        dec.encode_to(src.ptr + k * half, out[k], meta[k].ptr, meta[k].ptr + 32, n_streams=n, n_pictures=4, fmt=1, cont=k == 1,
                      first_pts=PTS0, src_stride=8 * PIC, dst_stride=stride)
    dec.sync()
    for i in range(n):
        parts = []
        for k in range(2):
            m = meta[k].download(np.uint32, 16)
            assert m[8 + i] == 0
            parts.append(download_region(dec, out[k], i * stride, int(m[i])))
        assert parts[0] + parts[1] == whole.streams[i]
    dec.close()


def download_region(dec, buf, offset, nbytes):
    b = np.empty(nbytes, dtype=np.uint8)
    if nbytes:
        assert dec._lib.efx_memcpy_d2h(dec._ctx, b.ctypes.data, buf.ptr + offset, nbytes) == 0
    return b.tobytes()


def test_batch_independence(efx):
    N, P = 1024, 3
    base = E.moving(P, seed=3)
    # stream k: the moving texture rotated by 97 k bytes and xor-ed with k: distinct content per stream
    src = np.stack([np.roll(base, k * 97, axis=1) ^ np.uint8(k & 0x3F) for k in range(N)])
    dec = efx.Decoder(N, 1)
    full = dec.encode(src, gop=12, search=7, fmt=1, recon=True, dst_stride=P * 256 * 1024)
    assert (full.status == 0).all()
    rng = np.random.default_rng(1234)
    for i in sorted(rng.choice(N, 16, replace=False)):
        alone = dec.encode(src[i:i + 1], gop=12, search=7, fmt=1, dst_stride=P * 256 * 1024)
        assert alone.streams[0] == full.streams[i], i
    dec.close()
    efx_decode_check(efx, full.streams, 1, list(full.recon))


def test_output_full(efx):
    pics = np.stack([E.moving(12, seed=s) for s in (1, 2, 3)])
    pics[2] = E.flat(12, 128)  # a small stream: fits
    dec = efx.Decoder(3, 1)
    big = dec.encode(pics, gop=12, fmt=0, recon=True)
    sizes = [len(s) for s in big.streams]
    stride = (sizes[0] * 3 // 4 + 15) // 16 * 16
    n, P = 3, 12
    src, dst = dec.alloc(pics.size), dec.alloc(n * stride + 4096)
    meta = dec.alloc(64)
    src.upload(pics)
    dst.upload(np.full(n * stride + 4096, 0xA5, dtype=np.uint8))
    dec.encode_to(src, dst, meta.ptr, meta.ptr + 16, n_streams=n, n_pictures=P, gop=12, fmt=0, dst_stride=stride)
    dec.sync()
    lens = meta.download(np.uint32, 8)
    st = lens[4:4 + n]
    raw = dst.download(np.uint8, n * stride + 4096)
    for i in range(n):
        region = raw[i * stride:(i + 1) * stride]
        got = region[:lens[i]].tobytes()
        assert (region[lens[i]:] == 0xA5).all(), "bytes written beyond the stream's output"
        if sizes[i] <= stride:
            assert st[i] == 0 and got == big.streams[i]
        else:
            assert st[i] == efx.ENCODE_FULL and 0 < lens[i] <= stride
            assert big.streams[i].startswith(got)
            k, _, _, frames = oracle.decode(np.frombuffer(got, dtype=np.uint8), 0, flush_last=True, want_frames=True)
            assert k >= 1 and np.array_equal(frames, M.i420_to_strip(big.recon[i][:k]))
    assert (raw[n * stride:] == 0xA5).all()
    assert st[0] == efx.ENCODE_FULL
    dec.close()


def test_invalid_arguments(efx):
    dec = efx.Decoder(2, 1)
    src, dst, meta = dec.alloc(2 * PIC), dec.alloc(1 << 20), dec.alloc(64)
    good = dict(n_streams=1, n_pictures=2, qscale=8, gop=12, search=7, fmt=1, dst_stride=1 << 19)
    for bad in ({"n_streams": 0}, {"n_streams": 3}, {"n_pictures": 0}, {"n_pictures": 256}, {"qscale": 0}, {"qscale": 32},
                {"gop": 0}, {"gop": 256}, {"search": -1}, {"search": 16}, {"fmt": 2}, {"first_pts": -1},
                {"first_pts": 1 << 33}, {"src_stride": PIC}, {"src_stride": 2 * PIC + 8}, {"dst_stride": 1000}):
        with pytest.raises(efx.EfxError) as e:
            dec.encode_to(src, dst, meta.ptr, meta.ptr + 16, **{**good, **bad})
        assert e.value.status == -1, bad
    for ptrs in ((None, dst.ptr, meta.ptr, meta.ptr + 16), (src.ptr + 4, dst.ptr, meta.ptr, meta.ptr + 16),
                 (src.ptr, None, meta.ptr, meta.ptr + 16), (src.ptr, dst.ptr + 8, meta.ptr, meta.ptr + 16),
                 (src.ptr, dst.ptr, None, meta.ptr + 16), (src.ptr, dst.ptr, meta.ptr, None)):
        with pytest.raises(efx.EfxError) as e:
            dec.encode_to(*ptrs, **good)
        assert e.value.status == -1
    with pytest.raises(efx.EfxError) as e:
        dec.encode_to(src, dst, meta.ptr, meta.ptr + 16, recon=meta.ptr + 4, **good)
    assert e.value.status == -1
    st = dec._lib.efx_encode(dec._ctx, None, src.ptr, dst.ptr, meta.ptr, meta.ptr + 16, None)
    assert st == -1
    dec.close()


def test_isolation(efx, clips):
    """A context that decodes, encodes and decodes again ends like one that never encoded."""
    from espflix_amd import gen
    streams = gen.Batch(3, 4, 8, 12, 0, threads=4).all_es()

    def run(encode):
        dec = efx.Decoder(4, 8, ring_depth=9, max_stream_bytes=sum(len(s) for s in streams) + 4096)
        dec.upload(streams, efx.FORMAT_ES)
        dec.decode()
        if encode:
            pics = np.stack([dec.export_host("i420", picture=p) for p in range(4)], axis=1)
            r = dec.encode(pics, gop=3, search=15)
            assert (r.status == 0).all()
        dec.upload(streams, efx.FORMAT_ES)
        dec.decode()
        res = ([dec.picture_count(i) for i in range(4)], [dec.stream_status(i) for i in range(4)], dec.frame_hashes().tolist(),
               [dec.stream_state(i) for i in range(4)])
        dec.close()
        return res

    assert run(True) == run(False)


def test_index_of_encoded_ts(efx, clip_pictures):
    pics = clip_pictures["vmedia"]
    enc = efx.Decoder(1, 1)
    ts = enc.encode(pics[None], gop=12, fmt=1, first_pts=PTS0).streams[0]
    enc.close()
    streams = [np.frombuffer(ts, dtype=np.uint8)] * 3
    dec = efx.Decoder(3, 1, 2, max_stream_bytes=3 * len(ts) + 4096)
    first, last, sp, so = oracle.ts_sequences(streams[0])
    assert len(sp) == (len(pics) + 11) // 12
    res = dec.index_streams(streams, trick_speed=[1, 15, 15])
    idx = efx.idx_build([r for r, _ in res], [s for _, s in res])
    assert idx == oracle.make_idx(streams)
    dec.close()


TORCH_CHILD = textwrap.dedent("""
    import sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import encode_model as E
    import export_model as M
    import oracle

    torch.cuda.set_stream(torch.cuda.Stream())
    dec = efx.Decoder(2, 6, ring_depth=7, device=torch.cuda.current_device(), hip_stream=torch.cuda.current_stream().cuda_stream,
                      max_stream_bytes=4 << 20)
    pics = torch.from_numpy(np.stack([E.moving(6, seed=5), E.moving(6, seed=6)])).cuda()
    pics = pics.flip(0).flip(0) + 0  # produced on torch's stream
    r = dec.encode(pics, gop=4, search=7, recon=True)
    assert isinstance(r.recon, torch.Tensor) and (r.status == 0).all()
    rec = r.recon.cpu().numpy()
    dec.upload([np.frombuffer(s, dtype=np.uint8) for s in r.streams], efx.FORMAT_TS)
    dec.decode()
    for p in range(6):
        img = dec.export("i420", picture=p)
        assert np.array_equal(img.cpu().numpy(), rec[:, p]), p
    n, _, _, frames = oracle.decode(np.frombuffer(r.streams[1], dtype=np.uint8), 1, True, True)
    assert n == 6 and np.array_equal(frames, M.i420_to_strip(rec[1]))
    print("torch encode ok")
""")


def test_torch_tensor_in(efx, tmp_path):
    script = tmp_path / "torch_encode.py"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch encode ok" in r.stdout
