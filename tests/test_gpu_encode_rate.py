"""efx_encode_rc (k_encode: k_enc_act + the controller of enc_rate.h): the device against the host build of the same
arithmetic (tests/encode_rate_model.py) byte for byte -- streams, status, reconstruction and the quantiser of every picture
-- and against the buffer model of include/efx.h restated in Python.  tests/test_encode_rate_model.py checks the host
model's behaviour (conformance, the scene cut, quality); equality with it carries those results to the device."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import encode_model as E
import encode_rate_model as R
import export_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = M.FRAME_BYTES
PTS0 = 129003
RATE = dict(bitrate=400_000, vbv_bits=250_000, qmin=3, qmax=31)
KW = dict(qscale=8, gop=12, search=7, first_pts=PTS0)


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return R.build(str(tmp_path_factory.mktemp("enc_rate_model")))


@pytest.fixture(scope="module")
def src(efx, clips):
    """V, X and N from the clips as the library decodes and exports them."""
    out = {}
    for name in ("splash", "vmedia"):
        dec = efx.Decoder(1, 100, ring_depth=101, max_stream_bytes=len(clips[name]) + 4096)
        dec.upload([clips[name]], efx.FORMAT_TS)
        dec.decode()
        out[name] = np.concatenate([dec.export_host("i420", picture=p) for p in range(dec.picture_count(0))])
        dec.close()
    return R.sources(out)


@pytest.fixture(scope="module")
def three(src):
    return np.stack([src["X"], src["V"][24:60], src["V"][:36]])


@pytest.fixture(scope="module")
def host_ts(model, three):
    """The host model's encoding of the three streams at 400 kbit/s, TS: computed once, never changed."""
    return [R.encode(model, p, fmt=1, **RATE, **KW) for p in three]


@pytest.fixture(scope="module")
def device_ts(efx, three):
    dec = efx.Decoder(3, 1)
    r = dec.encode(three, fmt=efx.FORMAT_TS, recon=True, **RATE, **KW)
    dec.close()
    return r


def same(r, i, want, what):
    assert r.streams[i] == want.stream, f"{what}: bytes differ from the host model"
    assert int(r.status[i]) == want.status, (what, int(r.status[i]), want.status)
    assert np.array_equal(r.recon[i], want.recon), f"{what}: reconstruction differs from the host model"
    assert np.array_equal(r.qscales[i], want.qscales), (what, r.qscales[i], want.qscales)


def test_device_equals_host(efx, three, host_ts, device_ts):
    """1: three streams in one call equal the host model stream by stream, and the same streams encoded one per call
    (per-stream state; one quantiser for the twelve rows of a picture)."""
    assert device_ts.qscales.shape == (3, 36) and device_ts.qscales.dtype == np.uint8
    for i in range(3):
        same(device_ts, i, host_ts[i], f"stream {i} of 3")
        R.check_stream(device_ts.streams[i], 1, device_ts.qscales[i], int(device_ts.status[i]), qscale=KW["qscale"], what=f"stream {i}",
                       **RATE)
        assert len(set(int(q) for q in device_ts.qscales[i])) > 2
    dec = efx.Decoder(1, 1)
    for i in range(3):
        r = dec.encode(three[i][None], fmt=efx.FORMAT_TS, recon=True, **RATE, **KW)
        same(r, 0, host_ts[i], f"stream {i} alone")
    dec.close()


def test_es_and_constant_quantiser(efx, model, src):
    """2: ES (a picture costs its headers plus slices) equals the host model; qmin = qmax = 8 is encode(qscale=8)."""
    pics = src["X"]
    want = R.encode(model, pics, fmt=0, **RATE, **KW)
    dec = efx.Decoder(1, 1)
    r = dec.encode(pics[None], fmt=efx.FORMAT_ES, recon=True, **RATE, **KW)
    same(r, 0, want, "X, ES")
    R.check_stream(r.streams[0], 0, r.qscales[0], int(r.status[0]), qscale=KW["qscale"], what="X ES", **RATE)
    for fmt in (efx.FORMAT_ES, efx.FORMAT_TS):
        fixed = dec.encode(pics[None], fmt=fmt, recon=True, bitrate=400_000, vbv_bits=250_000, qmin=8, qmax=8, **{**KW, "qscale": 5})
        plain = dec.encode(pics[None], fmt=fmt, recon=True, **{**KW, "qscale": 8})
        assert fixed.streams[0] == plain.streams[0] and np.array_equal(fixed.recon, plain.recon)
        assert (fixed.qscales == 8).all() and plain.qscales is None
    dec.close()


def test_continuation(efx, three, host_ts, device_ts):
    """3: cont over 7 + 12 + 17 pictures equals the single call: bytes, reconstruction, quantisers."""
    dec = efx.Decoder(3, 1)
    parts, at = [], 0
    for n in (7, 12, 17):
        parts.append(dec.encode(three[:, at:at + n], fmt=efx.FORMAT_TS, recon=True, cont=at > 0, **RATE, **KW))
        at += n
    dec.close()
    for i in range(3):
        assert b"".join(p.streams[i] for p in parts) == device_ts.streams[i]
        assert np.array_equal(np.concatenate([p.recon[i] for p in parts]), device_ts.recon[i])
        assert np.array_equal(np.concatenate([p.qscales[i] for p in parts]), device_ts.qscales[i])


def test_errors(efx, src):
    """4: cont with another bitrate or vbv_bits, or across the two entry points: EFX_ERR_STATE; NULL-free bad rates:
    EFX_ERR_ARG; a fresh call afterwards works."""
    pics = src["X"][None, :2]
    dec = efx.Decoder(1, 1)
    first = dec.encode(pics, **RATE, **KW)
    for change in (dict(bitrate=500_000), dict(vbv_bits=200_000)):
        with pytest.raises(efx.EfxError) as e:
            dec.encode(pics, cont=True, **{**RATE, **change}, **KW)
        assert e.value.status == -5, change
    with pytest.raises(efx.EfxError) as e:
        dec.encode(pics, cont=True, **KW)          # efx_encode continuing efx_encode_rc's streams
    assert e.value.status == -5
    dec.encode(pics, cont=True, **{**RATE, "qmin": 5, "qmax": 20}, **{**KW, "search": 3})   # these may change
    dec.encode(pics, **KW)
    with pytest.raises(efx.EfxError) as e:
        dec.encode(pics, cont=True, **RATE, **KW)  # and the reverse
    assert e.value.status == -5
    for bad in (dict(bitrate=0), dict(bitrate=-1), dict(vbv_bits=0), dict(qmin=0), dict(qmax=32), dict(qmin=9, qmax=8)):
        with pytest.raises(efx.EfxError) as e:
            dec.encode(pics, **{**RATE, **bad}, **KW)
        assert e.value.status == -1, bad
    for ok in (dict(bitrate=64_000), dict(bitrate=20_000_000), dict(vbv_bits=16_000), dict(vbv_bits=4_000_000)):
        dec.encode(pics, **{**RATE, **ok}, **KW)
    again = dec.encode(pics, **RATE, **KW)
    dec.close()
    assert again.streams == first.streams and np.array_equal(again.qscales, first.qscales)


def test_noise_sets_the_bit(efx, model, src):
    """5: N at 400 kbit/s: EFX_ENCODE_VBV, in agreement with the verifier; pictures that start in debt are at qmax."""
    dec = efx.Decoder(1, 1)
    r = dec.encode(src["N"][None], fmt=efx.FORMAT_TS, recon=True, **RATE, **KW)
    dec.close()
    under, before, _ = R.check_stream(r.streams[0], 1, r.qscales[0], int(r.status[0]), qscale=KW["qscale"], what="N", **RATE)
    assert under and int(r.status[0]) == efx.ENCODE_VBV == R.ENCODE_VBV
    assert all(int(r.qscales[0, p]) == 31 for p, f in enumerate(before) if f <= 0)
    same(r, 0, R.encode(model, src["N"], fmt=1, **RATE, **KW), "N")


def test_full_stream_reports_zero_quantisers(efx, src):
    """A picture that does not fit is not written: quantiser 0, and the buffer model sees only the written ones."""
    pics = src["V"][None, :6]
    dec = efx.Decoder(1, 1)
    whole = dec.encode(pics, **RATE, **KW)
    sizes = R.ts_picture_bytes(whole.streams[0])
    room = (sum(sizes[:3]) + 15) // 16 * 16
    assert room < sum(sizes[:4])
    r = dec.encode(pics, dst_stride=room, **RATE, **KW)
    dec.close()
    assert int(r.status[0]) & efx.ENCODE_FULL and r.streams[0] == whole.streams[0][:sum(sizes[:3])]
    assert list(r.qscales[0, :3]) == list(whole.qscales[0, :3]) and (r.qscales[0, 3:] == 0).all()


def test_efx_decode(efx, device_ts):
    """6: efx_decode of the streams of 1: status 0, ring frames equal to the reconstruction."""
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


AV_CHILD = textwrap.dedent("""
    import pickle, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import test_gpu_mux as T

    pics, pcm, n_frames = T.chain_inputs(2, 12)
    rate = dict(bitrate=400_000, vbv_bits=250_000, qmin=3, qmax=31)
    dec = efx.Decoder(2, 1, 2, device=torch.cuda.current_device())
    tp, tpcm = torch.from_numpy(pics).cuda(), torch.from_numpy(pcm).cuda()
    rated, st_r = dec.encode_av(tp, tpcm, qscale=6, gop=6, first_pts=T.PTS0, **rate)
    plain, st_p = dec.encode_av(tp, tpcm, qscale=6, gop=6, first_pts=T.PTS0)
    v_rated = dec.encode(tp, qscale=6, gop=6, first_pts=T.PTS0, **rate)
    v_plain = dec.encode(tp, qscale=6, gop=6, first_pts=T.PTS0)
    assert (st_p == 0).all() and all(int(s) | efx.ENCODE_VBV == efx.ENCODE_VBV for s in st_r)
    pickle.dump((rated, plain, v_rated.streams, v_plain.streams, v_rated.qscales, st_r, v_rated.status), open(sys.argv[2], "wb"))
    print("encode_av ok")
""")


def test_encode_av_with_bitrate(efx, tmp_path):
    """7: the video PID's packets of an encode_av(bitrate=...) title are the bytes encode(bitrate=...) gives; without
    bitrate encode_av gives the bytes it gave before (the multiplex of encode()'s video with the SBC model's frames)."""
    import pickle
    import mux_model as X
    import sbc_encode_model as SM
    import test_gpu_mux as T
    script, out = tmp_path / "encode_av_rate.py", tmp_path / "titles.pkl"
    script.write_text(AV_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "encode_av ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    rated, plain, v_rated, v_plain, qscales, st_r, st_v = pickle.load(open(out, "rb"))
    pics, pcm, n_frames = T.chain_inputs(2, 12)
    frames = SM.encode(SM.model_exe(), pcm)[0]
    for i in range(2):
        a = np.frombuffer(rated[i], dtype=np.uint8).reshape(-1, 188)
        pid = ((a[:, 1].astype(int) & 0x1F) << 8) | a[:, 2]
        assert a[pid == 0x100].tobytes() == v_rated[i]
        assert v_rated[i] != v_plain[i] and len(set(int(q) for q in qscales[i])) > 1
        assert int(st_r[i]) == int(st_v[i])
        assert plain[i] == X.mux(np.frombuffer(v_plain[i], dtype=np.uint8), frames[i], frame_bytes=T.FB, first_pts=T.PTS0)[0]
