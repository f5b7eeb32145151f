"""The directed SBC streams of tests/sbc_streams.py through efx_sbc_decode: every call by the default (frame-parallel) kernels
and by the one-wave kernel (OPT_SBC_SERIAL) -- PCM and return values of every stream against the oracle, the call's hashes
against tests/golden/sbc_directed.json (made from the reference), the decoder states of the two paths byte for byte.  What the
streams cover is asserted on the CPU in tests/test_sbc_directed.py."""
import json
import os

import numpy as np
import pytest

import oracle
import sbc_streams as S
from test_gpu_sbc import _decode_batch, unpack_ret

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sbc_directed.json")) as _f:
    GOLDEN = json.load(_f)

SB_SAMPLE = slice(1152, 2176)   # SbcState::sb_sample[16][2][8] inside a downloaded state


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


def run_call(efx, dec, call):
    """Both kernel paths over a call.  Returns the oracle's (pcm, rets, sb_sample) and the states the default kernels left."""
    data = [s.data for s in call.streams]
    want, wret, wsb = oracle.sbc_decode_call(data, call.fb)
    states = []
    for serial in (False, True):
        got, rets, st = _decode_batch(efx, dec, data, call.fb, call.frames, False, 1, serial)
        rets = np.array(rets, dtype=np.int32).reshape(wret.shape)
        for i, s in enumerate(call.streams):
            assert np.array_equal(rets[i], wret[i]), (s.name, serial)
            assert np.array_equal(got[i], want[i]), (s.name, serial)
        assert oracle.sbc_call_hashes(got, rets) == GOLDEN[call.name], (call.name, serial)
        states.append(st)
    for i, s in enumerate(call.streams):
        assert np.array_equal(states[0][i], states[1][i]), s.name
    return want, wret, wsb, states[0]


BITPOOL_RUNS = [range(0, 24), range(24, 56), range(56, 84), range(84, 104), range(104, 118), range(118, 129)]   # (a call's cost grows with its bitpool)


@pytest.mark.parametrize("bitpools", BITPOOL_RUNS, ids=[f"bp{r[0]}-{r[-1]}" for r in BITPOOL_RUNS])
@pytest.mark.parametrize("geometry", list(S.GEOMETRIES))
def test_alloc(efx, geometry, bitpools):
    """bit_allocation() at every frequency x allocation x bitpool 0..128: rows 0 and 1 of offset8 and the slice counter's
    edges, which only these streams reach.  The sample bits are random, so a wrong width shows in every later sample."""
    assert sorted(bp for r in BITPOOL_RUNS for bp in r) == list(S.BITPOOLS)
    dec = efx.Decoder(1, 1, 2)
    for bp in bitpools:
        run_call(efx, dec, S.alloc_call(geometry, bp))
    dec.close()


@pytest.mark.parametrize("layout", S.DEQUANT_LAYOUTS)
@pytest.mark.parametrize("b", list(S.WIDTHS))
def test_dequant(efx, b, layout):
    """sbc_iquant()'s multiply-and-shift division at every code of width b and every scale factor, observed where it is
    stored: the state's sb_sample after a one-frame stream (k_sbc_par_mono) and after the same frame behind a rejected one
    (k_sbc_gen) is the plain-Python IQUANT of the manifest's codes -- PCM can hide a one-LSB error.  The long layouts run the
    same frames through the steady state of k_sbc_par_mono and k_sbc_par_stereo."""
    dec = efx.Decoder(1, 1, 2)
    call = S.dequant_call(layout, b)
    _, _, wsb, states = run_call(efx, dec, call)
    if layout in ("one", "gen"):
        assert len(call.streams) <= 8192
        got = np.ascontiguousarray(states[:, SB_SAMPLE]).view(np.int32).reshape(-1, 16, 2, 8)
        assert np.array_equal(got, S.dequant_samples(b))
        assert np.array_equal(got, wsb)
    dec.close()


def _decode_shifted(efx, dec, call, offset, serial):
    """A call decoded from a device pointer `offset` bytes into its buffer, streams an odd number of bytes apart, their PCM an
    odd number of samples apart."""
    n, frames, fb = len(call.streams), call.frames, call.fb
    stride = (frames * fb + 16) | 1
    pcm_stride = frames * 256 + 1
    buf = np.zeros(offset + n * stride + 1024, dtype=np.uint8)
    for i, s in enumerate(call.streams):
        buf[offset + i * stride:offset + i * stride + frames * fb] = s.data
    dec.set_option(efx.OPT_SBC_SERIAL, 1 if serial else 0)
    d_fr, d_st = dec.alloc(buf.size), dec.alloc(n * efx.sbc_state_bytes())
    d_pcm, d_ret, d_cnt = dec.alloc(n * pcm_stride * 2), dec.alloc(n * frames * 4), dec.alloc(n * 4)
    d_fr.upload(buf)
    d_st.upload(np.zeros(n * efx.sbc_state_bytes(), dtype=np.uint8))
    d_ret.upload(np.full(n * frames, 0xDEADBEEF, dtype=np.uint32))
    dec.sbc_decode(n, d_fr.ptr + offset, stride, fb, frames, d_st, d_pcm, pcm_stride, d_ret, d_cnt)
    dec.sync()
    cnt = d_cnt.download(np.uint32, n)
    allpcm = d_pcm.download(np.int16, n * pcm_stride).reshape(n, pcm_stride)
    rets = np.array([unpack_ret(x) for x in d_ret.download(np.uint32, n * frames)], dtype=np.int32).reshape(n, frames, 2)
    states = d_st.download(np.uint8, n * efx.sbc_state_bytes()).reshape(n, -1).copy()
    for b in (d_fr, d_st, d_pcm, d_ret, d_cnt):
        b.free()
    dec.set_option(efx.OPT_SBC_SERIAL, 0)
    return [allpcm[i, :cnt[i]].copy() for i in range(n)], rets, states


@pytest.mark.parametrize("layout", S.PHASE_LAYOUTS)
def test_phase(efx, layout):
    """Fields of every width at every bit phase through field_staged, field_global and k_sbc_gen's reader."""
    dec = efx.Decoder(1, 1, 2)
    run_call(efx, dec, S.phase_call(layout))
    dec.close()


@pytest.mark.parametrize("serial", [False, True], ids=["default", "serial"])
@pytest.mark.parametrize("layout", S.PHASE_LAYOUTS)
def test_phase_misaligned(efx, layout, serial):
    """The phase streams from a frame pointer at each of the 16 byte offsets of an aligned buffer, with an odd stream_stride
    and an odd pcm_stride: efx_sbc_decode states no alignment for them and the audio demultiplexer hands over any offset.
    PCM, return values and states are the aligned decode's (the oracle's) at every offset."""
    call = S.phase_call(layout)
    want, wret, _ = oracle.sbc_decode_call([s.data for s in call.streams], call.fb)
    dec = efx.Decoder(1, 1, 2)
    _, _, states = _decode_batch(efx, dec, [s.data for s in call.streams], call.fb, call.frames, False, 1, serial)
    for offset in range(16):
        got, rets, st = _decode_shifted(efx, dec, call, offset, serial)
        for i, s in enumerate(call.streams):
            assert np.array_equal(rets[i], wret[i]), (s.name, offset)
            assert np.array_equal(got[i], want[i]), (s.name, offset)
            assert np.array_equal(st[i], states[i]), (s.name, offset)
    dec.close()


@pytest.mark.parametrize("width,mode", S.RANGE_CALLS)
def test_range(efx, width, mode):
    """Full-scale streams: the 24-bit multiplies of the frame-parallel kernels where both filter stages wrap 32 bits, and the
    clip to +-0x7FFF with the last unclipped values next to it."""
    dec = efx.Decoder(1, 1, 2)
    want, _, _, _ = run_call(efx, dec, S.range_call(width, mode))
    allpcm = np.concatenate(want)
    assert (allpcm == 0x7FFF).any() and allpcm.min() == -0x7FFF
    dec.close()
