"""efx_sbc_encode (k_sbc_enc.hip) on the device against the host model of the same arithmetic (tests/sbc_enc_model_main.cpp
over espflix_amd/csrc/sbc_enc_core.h): the same bytes for every geometry, batch shape, layout and stride, across calls
through the state; the frames decode on the device (efx_sbc_decode) as the oracle decodes them; argument errors; isolation
from the decoders; one run under the guard-page allocator."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle
import sbc_encode_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return M.build(str(tmp_path_factory.mktemp("sbc_enc_model")))


def batch_pcm(n_streams: int, n_values: int, seed: int = 11) -> np.ndarray:
    """int16 [n_streams, n_values]: a different signal per stream -- a tone of its own pitch and level over noise of its own
    level, every eighth stream full-scale noise, every ninth silent."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_values)
    out = np.empty((n_streams, n_values), dtype=np.int16)
    for i in range(n_streams):
        if i % 9 == 8:
            out[i] = 0
        elif i % 8 == 7:
            out[i] = rng.integers(-32768, 32768, n_values)
        else:
            x = (2000 + 900 * (i % 31)) * np.sin(2 * np.pi * (110 + 37 * (i % 53)) * t / 48000) + rng.normal(0, 1 + 40 * (i % 7), n_values)
            out[i] = np.clip(np.round(x), -32768, 32767)
    return out


def device_encode(efx, dec, pcm, calls=None, pcm_pad=0, frame_pad=0, **opt):
    """pcm [n, values] through efx_sbc_encode in the given calls (frames per call; default one).  Returns (frames [n, n_frames,
    fb], state [n, 288], the frame regions as written [n, stride]).  pcm_pad / frame_pad: extra elements / 16-byte units between
    the streams' regions, filled with a pattern that must survive."""
    ch = 2 if opt.get("mode", 0) else 1
    blocks, bitpool = opt.get("blocks", 16), opt.get("bitpool", 28)
    per = blocks * 8 * ch
    n, n_frames = pcm.shape[0], pcm.shape[1] // per
    fb = efx.sbc_frame_bytes(blocks, ch, bitpool)
    assert fb == M.frame_bytes(blocks, ch, bitpool)
    pcm_stride = pcm.shape[1] + pcm_pad
    stride = (n_frames * fb + 15) // 16 * 16 + 16 * frame_pad
    host = np.full((n, pcm_stride), 0x5A5A, dtype=np.int16)
    host[:, :pcm.shape[1]] = pcm
    d_pcm, d_st, d_fr = dec.alloc(host.nbytes), dec.alloc(n * efx.sbc_enc_state_bytes()), dec.alloc(n * stride)
    d_pcm.upload(host)
    d_st.upload(np.zeros(n * efx.sbc_enc_state_bytes(), dtype=np.uint8))
    d_fr.upload(np.full(n * stride, 0xA5, dtype=np.uint8))
    at = 0
    for k in calls or [n_frames]:
        assert (at * fb) % 16 == 0 and (at * per * 2) % 16 == 0, "a call must begin on 16-byte boundaries of PCM and frames"
        dec.sbc_encode_to(d_pcm.ptr + at * per * 2, d_st, d_fr.ptr + at * fb, n_streams=n, n_frames=k, pcm_stride=pcm_stride,
                          frame_stride=stride, **opt)
        at += k
    assert at == n_frames
    dec.sync()
    region = d_fr.download(np.uint8, n * stride).reshape(n, stride)
    state = d_st.download(np.uint8, n * efx.sbc_enc_state_bytes()).reshape(n, -1)
    for b in (d_pcm, d_st, d_fr):
        b.free()
    assert (region[:, n_frames * fb:] == 0xA5).all(), "bytes between the streams' frame regions were written"
    return region[:, :n_frames * fb].reshape(n, n_frames, fb), state, region


@pytest.mark.parametrize("mode", [0, 1], ids=["mono", "dual"])
@pytest.mark.parametrize("blocks", [4, 8, 12, 16])
def test_matrix_equals_the_host_model(efx, exe, mode, blocks):
    """Item 7, the matrix of item 1: both allocations, bitpools 2, 19, 28, 53, 128, three streams of ten frames."""
    ch = 2 if mode else 1
    pcm = batch_pcm(3, 10 * blocks * 8 * ch, seed=blocks + mode)
    dec = efx.Decoder(3, 1, 2)
    for allocation in (0, 1):
        for bitpool in (2, 19, 28, 53, 128):
            opt = dict(blocks=blocks, mode=mode, allocation=allocation, bitpool=bitpool)
            want, _, want_state, _ = M.encode(exe, pcm, **opt)
            got, state, _ = device_encode(efx, dec, pcm, **opt)
            assert np.array_equal(got, want), opt
            assert np.array_equal(state, want_state), opt
    dec.close()


@pytest.mark.parametrize("n_streams,n_frames", [(1, 1), (3, 4000), (1025, 375)])
def test_batch_shapes(efx, exe, n_streams, n_frames):
    """Item 7: 1, 3 and 1 025 streams with a different signal each; 1, 4 000 and 375 frames per call (mono, 16 blocks,
    bitpool 28: the frames the player plays)."""
    pcm = batch_pcm(n_streams, n_frames * 128)
    dec = efx.Decoder(n_streams, 1, 2)
    want, _, want_state, _ = M.encode(exe, pcm)
    got, state, _ = device_encode(efx, dec, pcm)
    dec.close()
    assert np.array_equal(state, want_state)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:5]


@pytest.mark.parametrize("blocks,mode,bitpool", [(16, 0, 28), (16, 1, 53), (4, 1, 36), (8, 0, 32), (12, 1, 20)])
def test_layouts_strides_and_calls(efx, exe, blocks, mode, bitpool):
    """Item 7: both PCM layouts, strides larger than the minimum (odd in int16 units for the PCM: a stream's samples then start
    2 bytes off a 16-byte boundary; what lies between the regions stays untouched), and a stream in calls of 2 + 14 + 20
    frames through the state -- call boundaries fall on 16-byte boundaries of the frames for these sizes."""
    ch = 2 if mode else 1
    n_frames = 36
    fb = M.frame_bytes(blocks, ch, bitpool)
    assert (2 * fb) % 16 == 0
    lines = batch_pcm(5 * ch, n_frames * blocks * 8, seed=bitpool).reshape(5, ch, -1)
    planar = lines.reshape(5, ch, n_frames, blocks * 8).transpose(0, 2, 1, 3).reshape(5, -1)
    inter = lines.transpose(0, 2, 1).reshape(5, -1)
    opt = dict(blocks=blocks, mode=mode, bitpool=bitpool, allocation=mode)
    want, _, want_state, _ = M.encode(exe, planar, **opt)
    dec = efx.Decoder(5, 1, 2)
    for pcm, layout in ((planar, efx.PCM_FRAME_PLANAR), (inter, efx.PCM_INTERLEAVED)):
        for calls in (None, [2, 14, 20]):
            got, state, _ = device_encode(efx, dec, pcm, calls=calls, pcm_pad=7, frame_pad=3, pcm_layout=layout, **opt)
            assert np.array_equal(got, want), (layout, calls)
            assert np.array_equal(state, want_state), (layout, calls)
    dec.close()


def test_device_decoder_takes_the_frames_pointer(efx, exe):
    """Item 8: efx_sbc_decode of the device's frames, the frames pointer and stride handed over unchanged, equals
    oracle.sbc_decode of them; and the PCM that comes back is the PCM that went in, 73 samples late, at unity gain."""
    for mode, blocks, bitpool in ((0, 16, 28), (1, 16, 53), (0, 8, 40), (1, 4, 60)):
        ch = 2 if mode else 1
        n, n_frames, per = 4, 48, blocks * 8 * ch
        fb = efx.sbc_frame_bytes(blocks, ch, bitpool)
        pcm = batch_pcm(n, n_frames * per, seed=5)
        dec = efx.Decoder(n, 1, 2)
        stride = (n_frames * fb + 15) // 16 * 16 + 32
        d_pcm, d_st, d_fr = dec.alloc(pcm.nbytes), dec.alloc(n * efx.sbc_enc_state_bytes()), dec.alloc(n * stride)
        d_dst, d_out, d_cnt = dec.alloc(n * efx.sbc_state_bytes()), dec.alloc(pcm.nbytes), dec.alloc(4 * n)
        d_pcm.upload(pcm)
        d_st.upload(np.zeros(n * efx.sbc_enc_state_bytes(), dtype=np.uint8))
        d_dst.upload(np.zeros(n * efx.sbc_state_bytes(), dtype=np.uint8))
        dec.sbc_encode_to(d_pcm, d_st, d_fr, n_streams=n, n_frames=n_frames, blocks=blocks, mode=mode, bitpool=bitpool, frame_stride=stride)
        dec.sbc_decode(n, d_fr, stride, fb, n_frames, d_dst, d_out, n_frames * per, None, d_cnt)   # (nothing synchronised in between)
        dec.sync()
        frames = d_fr.download(np.uint8, n * stride).reshape(n, stride)[:, :n_frames * fb]
        out = d_out.download(np.int16, n * n_frames * per).reshape(n, -1)
        assert (d_cnt.download(np.uint32, n) == n_frames * per).all()
        for i in range(n):
            want, rets = oracle.sbc_decode(frames[i], fb)
            assert rets == [(fb, per * 2)] * n_frames
            assert np.array_equal(out[i], want), (mode, blocks, i)
        if mode == 0 and bitpool == 28:
            g, snr = M.fit(pcm[0], out[0])
            assert abs(g - 1) < 0.005 and M.best_delay(pcm[0], out[0]) == M.DELAY, (g, snr)
        dec.close()


def test_invalid_arguments(efx):
    """Item 9: EFX_ERR_ARG for a field out of range, mode 2 or 3, a NULL or misaligned pointer, a stride too small or a frame
    stride that is no multiple of 16."""
    dec = efx.Decoder(2, 1, 2)
    d_pcm, d_st, d_fr = dec.alloc(2 * 4 * 256 * 2), dec.alloc(2 * efx.sbc_enc_state_bytes()), dec.alloc(2 * 4 * 528)
    good = dict(n_streams=2, n_frames=4, blocks=16, mode=0, allocation=0, bitpool=28, frequency=3)
    dec.sbc_encode_to(d_pcm, d_st, d_fr, **good)
    dec.sync()
    bad = [dict(n_streams=0), dict(n_streams=3), dict(n_frames=0), dict(n_frames=1 << 24), dict(frequency=4), dict(frequency=-1),
           dict(blocks=5), dict(blocks=20), dict(blocks=0), dict(mode=2), dict(mode=3), dict(mode=-1), dict(allocation=2),
           dict(bitpool=1), dict(bitpool=129), dict(pcm_layout=2), dict(pcm_stride=4 * 128 - 1), dict(frame_stride=4 * 64 - 16),
           dict(frame_stride=4 * 64 + 8)]
    for change in bad:
        with pytest.raises(efx.EfxError) as e:
            dec.sbc_encode_to(d_pcm, d_st, d_fr, **dict(good, **change))
        assert e.value.status == -1, change
    for ptrs in ((0, d_st.ptr, d_fr.ptr), (d_pcm.ptr, 0, d_fr.ptr), (d_pcm.ptr, d_st.ptr, 0), (d_pcm.ptr + 2, d_st.ptr, d_fr.ptr),
                 (d_pcm.ptr, d_st.ptr + 8, d_fr.ptr), (d_pcm.ptr, d_st.ptr, d_fr.ptr + 4)):
        with pytest.raises(efx.EfxError) as e:
            dec.sbc_encode_to(ptrs[0] or None, ptrs[1] or None, ptrs[2] or None, **good)
        assert e.value.status == -1, ptrs
    assert efx.sbc_frame_bytes(16, 1, 28) == 64 and efx.sbc_frame_bytes(16, 2, 128) == 524
    assert efx.sbc_frame_bytes(5, 1, 28) == 0 and efx.sbc_frame_bytes(16, 3, 28) == 0 and efx.sbc_frame_bytes(16, 1, 129) == 0
    assert efx.sbc_enc_state_bytes() == M.STATE_BYTES
    dec.close()


def test_isolation_from_the_decoders(efx, exe):
    """Item 9: an encode between two efx_decode calls and between two efx_sbc_decode calls changes neither's results."""
    import common
    from espflix_amd import gen
    streams = gen.Batch(3, 4, 6, 12, 0, threads=4).all_es()
    fb = common.sbc_frame_bytes(16, 1, 28)
    sbc = [common.sbc_frames(70 + i, 40, freq=3, blocks=16, mode=0, alloc=0, bitpool=28) for i in range(4)]

    def run(encode):
        dec = efx.Decoder(4, 6, ring_depth=7, max_stream_bytes=sum(len(s) for s in streams) + 4096)
        d_fr, d_st = dec.alloc(4 * 40 * fb), dec.alloc(4 * efx.sbc_state_bytes())
        d_out, d_cnt = dec.alloc(4 * 40 * 256), dec.alloc(16)
        d_fr.upload(np.concatenate(sbc))
        d_st.upload(np.zeros(4 * efx.sbc_state_bytes(), dtype=np.uint8))
        res = []
        for half in range(2):
            dec.upload(streams, efx.FORMAT_ES)
            dec.decode()
            dec.sbc_decode(4, d_fr.ptr + half * 20 * fb, 40 * fb, fb, 20, d_st, d_out, 20 * 128, None, d_cnt)
            dec.sync()
            res.append((dec.frame_hashes().tolist(), [dec.stream_state(i) for i in range(4)],
                        d_out.download(np.int16, 4 * 20 * 128).tolist(), d_st.download(np.uint8, 4 * efx.sbc_state_bytes()).tolist()))
            if encode and half == 0:
                got, _, _ = device_encode(efx, dec, batch_pcm(4, 30 * 128))
                assert np.array_equal(got, M.encode(exe, batch_pcm(4, 30 * 128))[0])
        dec.close()
        return res

    assert run(True) == run(False)


TORCH_CHILD = textwrap.dedent("""
    import sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import sbc_encode_model as M

    dec = efx.Decoder(3, 1, 2, device=torch.cuda.current_device())
    pcm = np.stack([M.signal("chord"), M.signal("lowpass"), M.signal("square")])
    want = M.encode(M.model_exe(), pcm)[0]
    whole = dec.sbc_encode(torch.from_numpy(pcm).cuda())
    assert whole.dtype == torch.uint8 and tuple(whole.shape) == (3, 60, 64) and whole.is_cuda
    assert np.array_equal(whole.cpu().numpy(), want)
    a = dec.sbc_encode(pcm[:, :8 * 128])                 # NumPy in, a fresh encoder
    b = dec.sbc_encode(pcm[:, 8 * 128:], cont=True)      # ... continued through the state the object keeps
    assert np.array_equal(np.concatenate([a.cpu().numpy(), b.cpu().numpy()], axis=1), want)
    print("torch sbc encode ok")
""")


def test_python_interface_with_tensors(efx, tmp_path):
    script = tmp_path / "torch_sbc_encode.py"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch sbc encode ok" in r.stdout


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import espflix_amd as efx
efx.load_library()
# buffers that end with their last valid byte: the PCM of 3 x 10 frames, the states, frames of 9 / 64 / 524 bytes
for blocks, mode, bitpool in ((16, 0, 28), (4, 0, 2), (16, 1, 128), (12, 1, 19)):
    ch = 2 if mode else 1
    n, frames, per = 3, 10, blocks * 8 * ch
    fb = efx.sbc_frame_bytes(blocks, ch, bitpool)
    stride = (frames * fb + 15) // 16 * 16
    dec = efx.Decoder(n, 1, 2)
    d_pcm, d_st = dec.alloc(n * frames * per * 2), dec.alloc(n * efx.sbc_enc_state_bytes())
    d_fr = dec.alloc((n - 1) * stride + frames * fb)
    rng = np.random.default_rng(blocks)
    d_pcm.upload(rng.integers(-32768, 32768, n * frames * per).astype(np.int16))
    d_st.upload(np.zeros(n * efx.sbc_enc_state_bytes(), dtype=np.uint8))
    for layout in (0, 1):
        dec.sbc_encode_to(d_pcm, d_st, d_fr, n_streams=n, n_frames=frames, blocks=blocks, mode=mode, bitpool=bitpool,
                          pcm_layout=layout, frame_stride=stride)
        dec.sync()
    dec.close()
print("GUARD_OK")
"""


@pytest.mark.parametrize("guard", ["1", "2"])
def test_every_buffer_of_a_call_under_the_guard_page_allocator(guard):
    """Item 12.  EFX_GUARD: every device buffer is its own mapping that ends (1) or starts (2) on an unmapped page, so a kernel
    that reads or writes one element past a buffer faults.  The PCM, state and frame buffers end with their last valid byte:
    the staging reads whole aligned 16 bytes around a stream's samples, the store writes whole aligned 16 bytes only inside a
    frame."""
    env = dict(os.environ, EFX_GUARD=guard)
    r = subprocess.run([sys.executable, "-c", _GUARD_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GUARD_OK" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-1500:])
