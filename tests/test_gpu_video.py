"""Composite-video field and PDM kernels against the reference-derived goldens and the oracle.
The bar for the composite line is +-1 LSB of the DAC byte; the path is all-integer so the tests
demand exact equality."""
import numpy as np
import pytest

import common
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


def gpu_fields(efx, dec, frames2, ntsc, nfields):
    """Fields for frame_counter 0..nfields-1 of the front frame (Frame[0])."""
    dec.upload_frame(0, 0, frames2[:efx.FRAME_BYTES])
    vp = efx.video_params(ntsc)
    n = vp["line_width"] * vp["line_count"]
    dst = dec.alloc(n * 2)
    out = []
    for fc in range(nfields):
        dec.composite_fields(dst, 0, 1, 0, ntsc, fc)
        dec.sync()
        out.append(dst.download(np.uint16, n).reshape(vp["line_count"], vp["line_width"]))
    dst.free()
    return np.stack(out)


def test_composite_vs_reference_golden(efx, golden):
    from espflix_amd import gen
    _, _, _, frames = oracle.decode(gen.Batch(0, 1, 12, 12, 0).es(0), 0, want_frames=True)
    inputs = {"lcg": common.lcg_frames(), "random": common.random_frames(7),
              "decoded": np.concatenate([frames[10], frames[11]])}
    dec = efx.Decoder(1, 1, 2)
    for name, fr in inputs.items():
        for ntsc in (True, False):
            f = gpu_fields(efx, dec, fr, ntsc, 3)
            got = [f"{common.fnv_bytes(f[i]):016x}" for i in range(3)]
            assert got == golden["composite"][f"{name}:{'ntsc' if ntsc else 'pal'}"]
            want = oracle.video_field(fr, ntsc, 0, 3)
            # stated tolerance: +-1 LSB on the DAC (high) byte; observed: identical words
            assert np.abs((f >> 8).astype(int) - (want >> 8).astype(int)).max() <= 1
            assert np.array_equal(f, want)
    dec.close()


def test_composite_batch_of_decoded_streams(efx):
    """config 4: fields of the last decoded picture of a batch of streams, both dither phases."""
    from espflix_amd import gen
    b = gen.Batch(0, 32, 12, 12, 0)
    dec = efx.Decoder(32, 12, 2)
    dec.upload(b.all_es(), efx.FORMAT_ES)
    dec.decode()
    slot = dec.picture_slot(11)
    for ntsc in (True, False):
        vp = efx.video_params(ntsc)
        n = vp["line_width"] * vp["line_count"]
        dst = dec.alloc(32 * n * 2)
        for fc in (0, 1):
            dec.composite_fields(dst, 0, 32, slot, ntsc, fc)
            dec.sync()
            got = dst.download(np.uint16, 32 * n).reshape(32, -1)
            for k in (0, 13, 31):
                fr = dec.download_frame(k, slot)
                want = oracle.video_field(np.concatenate([fr, fr]), ntsc, fc, 1).reshape(-1)
                assert np.array_equal(got[k], want)
        dst.free()
    dec.close()


def test_pdm_vs_reference_golden_and_oracle(efx, golden):
    dec = efx.Decoder(1, 1, 2)
    S, calls = 64, 40
    pcm = np.stack([common.pdm_pcm(k, calls) for k in range(S)])
    n = pcm.shape[1]
    d_pcm, d_state, d_out = dec.alloc(pcm.nbytes), dec.alloc(S * 12), dec.alloc(S * n * 4)
    d_pcm.upload(pcm)
    d_state.upload(np.zeros(S * 3, dtype=np.int32))
    dec.pdm(S, d_pcm, n, d_state, d_out)
    dec.sync()
    got = d_out.download(np.uint16, S * 2 * n).reshape(S, 2 * n)
    assert f"{common.fnv_bytes(got[0]):016x}" == golden["pdm"]["sine220"]
    states = d_state.download(np.int32, S * 3).reshape(S, 3)
    for k in range(S):
        st = np.zeros(3, dtype=np.int32)
        assert np.array_equal(got[k], oracle.pdm(st, pcm[k]))
        assert np.array_equal(states[k], st)
    # state persists across calls (static _i0,_i1,_i2 in the sketch): 128-sample calls chained
    d_state.upload(np.zeros(S * 3, dtype=np.int32))
    d_small = dec.alloc(S * 128 * 2)
    d_o2 = dec.alloc(S * 128 * 4)
    for c in range(3):
        d_small.upload(np.ascontiguousarray(pcm[:, c * 128:(c + 1) * 128]))
        dec.pdm(S, d_small, 128, d_state, d_o2)
        dec.sync()
        part = d_o2.download(np.uint16, S * 256).reshape(S, 256)
        assert np.array_equal(part, got[:, c * 256:(c + 1) * 256])
    dec.close()


def test_display_state_hscroll_and_overlay(efx, golden):
    """the two-frame slide (_hscroll, video.cpp:1146-1154) and the overlay / progress
    bar (composite(), video.cpp:845-887) in k_composite: every field bit-exact against the
    reference goldens and the oracle; the caller decrements the blend per field as the ISR does."""
    disp = np.minimum(common.random_frames(77), 248)
    dec = efx.Decoder(1, 1, 2)
    dec.upload_frame(0, 0, disp[:efx.FRAME_BYTES])
    dec.upload_frame(0, 1, disp[efx.FRAME_BYTES:])
    d_ov = dec.alloc(1280)
    for name, front, hs, ov_seed, blend0, progress in common.DISPLAY_CASES:
        n = len(hs) if hs is not None else 6
        ov = common.overlay_bytes(ov_seed) if ov_seed is not None else None
        d_ov.upload(ov if ov is not None else np.zeros(1280, np.uint8))
        for ntsc in (True, False):
            vp = efx.video_params(ntsc)
            cnt = vp["line_width"] * vp["line_count"]
            dst = dec.alloc(cnt * 2)
            want = oracle.video_field_ex(disp, ntsc, 0, n, front, hs, ov, blend0, progress)
            blend = blend0
            got = []
            for fld in range(n):
                dec.composite_fields_ex(dst, 0, 1, front, ntsc, fld, other_slot=front ^ 1, hscroll=hs[fld] if hs else 0,
                                        overlay=d_ov if ov is not None else None, overlay_blend=blend, overlay_progress=progress)
                dec.sync()
                f = dst.download(np.uint16, cnt).reshape(vp["line_count"], vp["line_width"])
                assert np.array_equal(f, want[fld]), (name, ntsc, fld)
                got.append(f"{common.fnv_bytes(f):016x}")
                if blend > 0:
                    blend -= 1
            assert got == golden["display"][f"{name}:{'ntsc' if ntsc else 'pal'}"], name
            dst.free()
    dec.close()


def test_display_state_batch_and_arguments(efx):
    """Per-stream overlays (stride) and a shared overlay give each stream its own field; bad
    scroll values are rejected."""
    from espflix_amd import gen
    b = gen.Batch(0, 4, 2, 12, 0)
    dec = efx.Decoder(4, 2, 3)
    dec.upload(b.all_es())
    dec.decode()
    frames = [[dec.download_frame(i, s) for s in range(3)] for i in range(4)]
    ovs = np.stack([common.overlay_bytes(20 + i) for i in range(4)])
    d_ov = dec.alloc(ovs.size)
    d_ov.upload(ovs)
    vp = efx.video_params(True)
    cnt = vp["line_width"] * vp["line_count"]
    dst = dec.alloc(4 * cnt * 2)
    s1, s2 = dec.picture_slot(0), dec.picture_slot(1)
    dec.composite_fields_ex(dst, 0, 4, s2, True, 3, other_slot=s1, hscroll=-104, overlay=d_ov, overlay_stride=1280,
                            overlay_blend=17, overlay_progress=77)
    dec.sync()
    got = dst.download(np.uint16, 4 * cnt).reshape(4, vp["line_count"], vp["line_width"])
    for i in range(4):
        pair = np.concatenate([frames[i][s2], frames[i][s1]])  # oracle frame 0 = displayed, 1 = other
        want = oracle.video_field_ex(pair, True, 3, 1, 0, [-104], ovs[i], 17, 77)[0]
        assert np.array_equal(got[i], want), i
    for bad in (4, 352, -352, 1000):
        with pytest.raises(efx.EfxError):
            dec.composite_fields_ex(dst, 0, 4, s2, True, 0, other_slot=s1, hscroll=bad)
    dec.close()


def pdm_edge_pcm(rng, n_streams: int, n_samples: int) -> np.ndarray:
    """Full-scale noise with both extremes and runs of each, a different mix in every stream."""
    pcm = rng.integers(-32768, 32768, (n_streams, n_samples)).astype(np.int16)
    for s in range(n_streams):
        k = s % 4
        if k == 0:
            pcm[s, ::3] = -32768
            pcm[s, 1::3] = 32767
        elif k == 1:
            pcm[s, :max(1, n_samples // 2)] = 32767     # a run of the upper extreme, then noise
        elif k == 2:
            pcm[s, n_samples // 3:] = -32768            # noise, then a run of the lower extreme
    return pcm


def pdm_edge_states(n_streams: int) -> np.ndarray:
    """Hand-made start states: large i1 / i2 of both signs (the integrators wrap like int32), a few small ones."""
    hand = np.array([[30000, 0x7FFFFF00, -0x7FFFFF00], [-30000, -0x70000000, 0x7FFFFFFF], [-65536, 123456789, -987654321],
                     [1, -1, 0], [0, 0x40000000, 0x40000000]], dtype=np.int64)
    st = hand[np.arange(n_streams) % len(hand)].copy()
    st[:, 0] += np.arange(n_streams) * 7
    return st.astype(np.int32)


GUARD = 64  # bytes behind every output of the PDM edge tests, which no call may touch


def run_pdm(dec, pcm: np.ndarray, state: np.ndarray, pcm_skew: int = 0, dst_skew: int = 0):
    """One efx_pdm call on fresh buffers; pcm_skew / dst_skew move the pointers by that many bytes inside the buffers.
    Returns (words (S, 2n), end states (S, 3)) after checking the bytes around the outputs."""
    S, n = pcm.shape
    d_pcm, d_state, d_out = dec.alloc(pcm_skew + pcm.nbytes), dec.alloc(S * 12 + GUARD), dec.alloc(dst_skew + S * n * 4 + GUARD)
    d_pcm.upload(np.concatenate([np.zeros(pcm_skew, np.uint8), pcm.reshape(-1).view(np.uint8)]))
    d_state.upload(np.concatenate([state.reshape(-1).view(np.uint8), np.full(GUARD, 0xA5, np.uint8)]))
    d_out.upload(np.full(dst_skew + S * n * 4 + GUARD, 0xA5, np.uint8))
    dec.pdm(S, d_pcm.ptr + pcm_skew, n, d_state, d_out.ptr + dst_skew)
    dec.sync()
    out = d_out.download(np.uint8, dst_skew + S * n * 4 + GUARD)
    st = d_state.download(np.uint8, S * 12 + GUARD)
    for b in (d_pcm, d_state, d_out):
        b.free()
    assert (out[:dst_skew] == 0xA5).all() and (out[dst_skew + S * n * 4:] == 0xA5).all() and (st[S * 12:] == 0xA5).all()
    return out[dst_skew:dst_skew + S * n * 4].view(np.uint16).reshape(S, 2 * n), st[:S * 12].view(np.int32).reshape(S, 3)


def check_pdm(words, states, pcm, start, tag):
    for s in range(pcm.shape[0]):
        st = start[s].copy()
        want = oracle.pdm(st, pcm[s])
        assert np.array_equal(words[s], want), (tag, s)
        assert np.array_equal(states[s], st), (tag, s)


def test_pdm_tails_short_calls_unaligned_streams_partial_blocks(efx):
    """k_pdm beyond the service's shapes: the scalar tail (n_samples % 8), calls shorter than one group of eight, streams
    whose PCM is not 16-byte aligned (any odd n_samples puts stream 1 there), workgroups of 64 only partly filled; from
    hand-made start states with large integrators and from the end states of the call before."""
    dec = efx.Decoder(1, 1, 2)
    rng = np.random.default_rng(2024)
    for S in (1, 3, 65, 130):
        for n in (1, 7, 8, 9, 15, 127, 136):
            start = pdm_edge_states(S)
            pcm = pdm_edge_pcm(rng, S, n)
            words, states = run_pdm(dec, pcm, start)
            check_pdm(words, states, pcm, start, (S, n, "hand-made"))
            pcm2 = pdm_edge_pcm(rng, S, n)[::-1].copy()
            words2, states2 = run_pdm(dec, pcm2, states)
            check_pdm(words2, states2, pcm2, states, (S, n, "carried"))
            assert pcm.min() == -32768 and pcm.max() == 32767 or S * n < 3
    dec.close()


def test_pdm_chained_calls_and_skewed_pointers(efx):
    """Calls of 127, 9 and 136 samples give the words and the end state of one call of 272; with the PCM pointer advanced
    by one sample and dst by four bytes every stream goes sample by sample and gives the same words; a dst or state
    pointer that is not 4-byte aligned is refused before anything is launched."""
    dec = efx.Decoder(1, 1, 2)
    S = 65
    rng = np.random.default_rng(77)
    pcm = pdm_edge_pcm(rng, S, 272)
    start = pdm_edge_states(S)
    whole, end = run_pdm(dec, pcm, start)
    check_pdm(whole, end, pcm, start, "one call")
    st, pos, parts = start, 0, []
    for n in (127, 9, 136):
        w, st = run_pdm(dec, np.ascontiguousarray(pcm[:, pos:pos + n]), st)
        parts.append(w)
        pos += n
    assert np.array_equal(np.concatenate(parts, axis=1), whole) and np.array_equal(st, end)
    skew, end2 = run_pdm(dec, pcm, start, pcm_skew=2, dst_skew=4)
    assert np.array_equal(skew, whole) and np.array_equal(end2, end)
    d_pcm, d_state, d_out = dec.alloc(64), dec.alloc(64), dec.alloc(128)
    d_state.upload(np.zeros(16, dtype=np.int32))
    d_pcm.upload(np.zeros(32, dtype=np.int16))
    for state_ptr, dst_ptr in ((d_state.ptr, d_out.ptr + 2), (d_state.ptr, d_out.ptr + 1), (d_state.ptr + 2, d_out.ptr)):
        with pytest.raises(efx.EfxError) as err:
            dec.pdm(1, d_pcm, 8, state_ptr, dst_ptr)
        assert err.value.status == -1   # EFX_ERR_ARG
    dec.pdm(1, d_pcm.ptr + 2, 8, d_state.ptr + 4, d_out.ptr + 4)   # what the contract allows
    dec.sync()
    dec.close()


def test_composite_sub_ranges_of_a_batch(efx):
    """first_stream > 0, a ring deeper than 2 and a slot above 1: k_composite's stream addressing
    frames + (first_stream + s) * ring_depth * frame bytes, the output offset of a sub-range (field k of the output is
    stream first_stream + k) and per-stream overlays (output stream k reads overlay k of the call)."""
    dec = efx.Decoder(5, 2, 3)
    frames = [[np.minimum(common.random_frames(300 + 3 * i + j)[:efx.FRAME_BYTES], 248) for j in range(3)] for i in range(5)]
    for i in range(5):
        for j in range(3):
            dec.upload_frame(i, j, frames[i][j])
    ovs = np.stack([common.overlay_bytes(40 + k) for k in range(2)])
    d_ov = dec.alloc(ovs.size)
    d_ov.upload(ovs)
    for ntsc in (True, False):
        vp = efx.video_params(ntsc)
        cnt = vp["line_width"] * vp["line_count"]
        dst = dec.alloc(4 * cnt * 2)
        for fc in (0, 1):
            dst.upload(np.full(4 * cnt, 0xABCD, dtype=np.uint16))
            dec.composite_fields(dst, 2, 3, 2, ntsc, fc)
            dec.sync()
            got = dst.download(np.uint16, 4 * cnt).reshape(4, -1)
            for k in range(3):
                f = frames[2 + k][2]
                assert np.array_equal(got[k], oracle.video_field(np.concatenate([f, f]), ntsc, fc, 1).reshape(-1)), (ntsc, fc, k)
            assert (got[3] == 0xABCD).all() and len({got[k].tobytes() for k in range(3)}) == 3
            dst.upload(np.full(4 * cnt, 0xABCD, dtype=np.uint16))
            dec.composite_fields_ex(dst, 3, 2, 1, ntsc, fc, other_slot=2, hscroll=-104, overlay=d_ov, overlay_stride=1280,
                                    overlay_blend=17, overlay_progress=77)
            dec.sync()
            got = dst.download(np.uint16, 4 * cnt).reshape(4, -1)
            for k in range(2):
                pair = np.concatenate([frames[3 + k][1], frames[3 + k][2]])  # oracle frame 0 = displayed, 1 = other
                want = oracle.video_field_ex(pair, ntsc, fc, 1, 0, [-104], ovs[k], 17, 77)[0].reshape(-1)
                assert np.array_equal(got[k], want), (ntsc, fc, k)
            assert (got[2:] == 0xABCD).all() and got[0].tobytes() != got[1].tobytes()
        for first, n in ((3, 3), (5, 1), (0, 6)):
            with pytest.raises(efx.EfxError):
                dec.composite_fields(dst, first, n, 2, ntsc, 0)
            with pytest.raises(efx.EfxError):
                dec.composite_fields_ex(dst, first, n, 1, ntsc, 0, other_slot=2, hscroll=-104)
        dst.free()
    dec.close()
