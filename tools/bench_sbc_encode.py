"""Measure efx_sbc_encode (k_sbc_enc) and efx_mux_av (k_mux): 1024 streams x 1 s of mono 48 kHz at bitpool 28 (375 frames of
64 bytes each), and 1024 twelve-picture transport streams multiplexed with the audio that lasts as long.  Prints one JSON
line: ms per call from HIP events recorded on the library's own stream around one call (the best of --steps timed calls
after --warmup, and their mean), stream-seconds per second, the bytes the algorithms move over the time as a share of the
HBM peak, and -- for context only -- efx_sbc_decode of the same frames, measured the same way in the same process."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import espflix_amd as efx  # noqa: E402
import encode_model as E  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second (MI355X data sheet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=375)
    ap.add_argument("--pictures", type=int, default=12)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    N, F, P, FB = args.streams, args.frames, args.pictures, 64
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    dec = efx.Decoder(N, 1, hip_stream=stream.value)  # the library runs on this stream: the events below bracket its launches
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(ev0))
    hip.hipEventCreate(C.byref(ev1))

    def timed(call):
        for _ in range(args.warmup):
            call()
        dec.sync()
        ms = []
        for _ in range(args.steps):
            hip.hipEventRecord(ev0, stream)
            call()
            hip.hipEventRecord(ev1, stream)
            hip.hipEventSynchronize(ev1)
            t = C.c_float()
            hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
            ms.append(t.value)
        dec.sync()
        return min(ms), float(np.mean(ms))

    out = {"streams": N, "frames": F, "timing": "HIP events on the library's stream around one call; best and mean of the timed calls",
           "hbm_peak_bytes_per_s": HBM_PEAK}
    # -- efx_sbc_encode: a tone and noise of its own per stream ---------------------------------------------------------
    rng = np.random.default_rng(1)
    t = np.arange(F * 128)
    pcm = np.stack([np.clip(np.round(6000 * np.sin(2 * np.pi * (150 + 13 * (i % 97)) * t / 48000) + rng.normal(0, 300, t.size)),
                            -32768, 32767).astype(np.int16) for i in range(N)])
    stride = (F * FB + 15) // 16 * 16
    d_pcm, d_st, d_fr = dec.alloc(pcm.nbytes), dec.alloc(N * efx.sbc_enc_state_bytes()), dec.alloc(N * stride)
    d_pcm.upload(pcm)
    d_st.upload(np.zeros(N * efx.sbc_enc_state_bytes(), dtype=np.uint8))
    best, mean = timed(lambda: dec.sbc_encode_to(d_pcm, d_st, d_fr, n_streams=N, n_frames=F, frame_stride=stride))
    moved = N * F * (128 * 2 + FB)
    seconds = F * 128 / 48000
    out["sbc_encode"] = {"ms_per_call": best, "ms_mean": mean, "stream_seconds_per_s": N * seconds / (best / 1e3),
                         "bytes_moved": moved, "share_of_hbm_peak": moved / (best / 1e3) / HBM_PEAK}
    # -- context: efx_sbc_decode of those frames ----------------------------------------------------------------------------
    d_dst, d_out, d_cnt = dec.alloc(N * efx.sbc_state_bytes()), dec.alloc(pcm.nbytes), dec.alloc(4 * N)
    d_dst.upload(np.zeros(N * efx.sbc_state_bytes(), dtype=np.uint8))
    best, mean = timed(lambda: dec.sbc_decode(N, d_fr, stride, FB, F, d_dst, d_out, F * 128, None, d_cnt))
    out["sbc_decode_context"] = {"ms_per_call": best, "ms_mean": mean, "stream_seconds_per_s": N * seconds / (best / 1e3)}
    # -- efx_mux_av: twelve-picture streams with the audio that lasts as long --------------------------------------------------
    base = E.moving(P, seed=3)
    src = np.stack([np.roll(base, k * 97, axis=1) ^ np.uint8(k & 0x3F) for k in range(N)])
    v_stride = P * 128 * 1024
    n_audio = -(-P * 3003 * 48000 // (90000 * 128))
    assert n_audio <= F
    st_off = (4 * N + 15) // 16 * 16
    d_src, d_v, d_meta = dec.alloc(src.size), dec.alloc(N * v_stride), dec.alloc(4 * st_off)
    d_src.upload(src)
    dec.encode_to(d_src, d_v, d_meta.ptr, d_meta.ptr + st_off, n_streams=N, n_pictures=P, qscale=8, gop=12, search=7, fmt=efx.FORMAT_TS,
                  dst_stride=v_stride)
    dec.sync()
    vlen = d_meta.download(np.uint32, N)
    m_stride = efx.mux_bound(int(vlen.max()), n_audio, FB, 8)
    d_dst2 = dec.alloc(N * m_stride)
    best, mean = timed(lambda: dec.mux_to(d_v, d_meta.ptr, d_fr, d_dst2, d_meta.ptr + 2 * st_off, d_meta.ptr + 3 * st_off, n_streams=N,
                                          frame_bytes=FB, n_frames=n_audio, video_stride=v_stride, audio_stride=stride, dst_stride=m_stride,
                                          audio_first_pts=0))
    status = np.empty(N, dtype=np.uint32)
    assert dec._lib.efx_memcpy_d2h(dec._ctx, status.ctypes.data, d_meta.ptr + 3 * st_off, 4 * N) == 0
    assert (status == 0).all()
    mlen = np.empty(N, dtype=np.uint32)
    assert dec._lib.efx_memcpy_d2h(dec._ctx, mlen.ctypes.data, d_meta.ptr + 2 * st_off, 4 * N) == 0
    moved = int(vlen.sum()) + N * n_audio * FB + int(mlen.sum())
    out["mux"] = {"pictures": P, "audio_frames": n_audio, "ms_per_call": best, "ms_mean": mean, "video_bytes_per_stream": float(vlen.mean()),
                  "title_bytes_per_stream": float(mlen.mean()), "bytes_moved": moved, "share_of_hbm_peak": moved / (best / 1e3) / HBM_PEAK}
    print(json.dumps(out))
    dec.close()


if __name__ == "__main__":
    main()
