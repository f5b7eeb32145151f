"""Measure efx_encode (k_encode): 1024 streams x 12 pictures, GOP 12, qscale 8, TS, at search 7 and 15, and -- to split
the time -- at search 0 and intra only (GOP 1), then efx_encode_rc at search 7: 1500 kbit/s under a 250 000-bit buffer, qmin 3 (the
reference indexer's profile; 1 + 3 x pictures launches, the activity measure included).  The source is distinct per stream (a moving texture, rotated and xor-ed per
stream).  Prints one JSON line: encoded pictures per second from HIP events recorded on the library's own stream around one
efx_encode call (the best of --steps timed calls after --warmup, and their mean), bytes per picture and the mean luma PSNR
of the reconstruction against the source (every 64th stream).

--aq S[,S...]: adaptive quantisation strengths (efx_encode_set_adaptive_quant; 0 = off, the default).  Every leg runs at
every strength, the timed calls alternating between them; a leg at strength S > 0 is reported as <leg>_aq<S> (one more
launch per picture: k_enc_aq)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pictures", type=int, default=12)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--searches", default="7,15")
    ap.add_argument("--aq", default="0", help="comma-separated adaptive quantisation strengths 0 .. 256, e.g. 0,256")
    ap.add_argument("--legs", default="", help="comma-separated leg names to run (default: all), e.g. rate_1500k for a profile")
    args = ap.parse_args()
    N, P = args.streams, args.pictures
    base = E.moving(P, seed=3)
    src = np.stack([np.roll(base, k * 97, axis=1) ^ np.uint8(k & 0x3F) for k in range(N)])
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    dec = efx.Decoder(N, 1, hip_stream=stream.value)  # the library runs on this stream: the events below bracket its launches
    stride = P * 128 * 1024  # well above what qscale 8 writes here, intra pictures included (checked: no EFX_ENCODE_FULL)
    st_off = (4 * N + 15) // 16 * 16
    d_src, d_dst, d_meta = dec.alloc(src.size), dec.alloc(N * stride), dec.alloc(2 * st_off)
    d_rec = dec.alloc(N * P * efx.FRAME_BYTES)
    d_src.upload(src)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(ev0))
    hip.hipEventCreate(C.byref(ev1))
    out = {"streams": N, "pictures": P, "qscale": 8, "format": "ts", "timing": "HIP events on the library's stream around "
           "one efx_encode call (its 1 + 2 x pictures launches); best and mean of the timed calls"}
    # the issue's two radii, then the parts: search 0 (no search, every P tool else) and GOP 1 (intra only: no search, no
    # prediction) -- the differences split the time between the search and the rest
    legs = [(f"search{r}", r, 12, {}) for r in (int(x) for x in args.searches.split(","))]
    legs += [("search0", 0, 12, {}), ("intra_only", 0, 1, {})]
    legs += [("rate_1500k", 7, 12, dict(bitrate=1_500_000, vbv_bits=250_000, qmin=3, qmax=31))]
    legs = [leg for leg in legs if not args.legs or leg[0] in args.legs.split(",")]
    strengths = [int(x) for x in args.aq.split(",")]
    for leg, R, gop, rate in legs:
        kw = dict(n_streams=N, n_pictures=P, qscale=8, gop=gop, search=R, fmt=efx.FORMAT_TS, dst_stride=stride, **rate)
        for _ in range(args.warmup):
            for aq in strengths:
                dec.encode_to(d_src, d_dst, d_meta.ptr, d_meta.ptr + st_off, recon=d_rec, aq=aq, **kw)
        dec.sync()
        times = {aq: [] for aq in strengths}
        for _ in range(args.steps):
            for aq in strengths:
                hip.hipEventRecord(ev0, stream)
                dec.encode_to(d_src, d_dst, d_meta.ptr, d_meta.ptr + st_off, recon=d_rec, aq=aq, **kw)
                hip.hipEventRecord(ev1, stream)
                hip.hipEventSynchronize(ev1)
                t = C.c_float()
                hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
                times[aq].append(t.value)
        dec.sync()
        for aq in strengths:
            name, ms = (f"{leg}_aq{aq}" if aq else leg), times[aq]
            if len(strengths) > 1:  # the figures below are those of the call's own output
                dec.encode_to(d_src, d_dst, d_meta.ptr, d_meta.ptr + st_off, recon=d_rec, aq=aq, **kw)
                dec.sync()
            lens = d_meta.download(np.uint32, N)
            status = np.empty(N, dtype=np.uint32)
            assert dec._lib.efx_memcpy_d2h(dec._ctx, status.ctypes.data, d_meta.ptr + st_off, 4 * N) == 0
            assert (status & efx.ENCODE_FULL == 0).all(), "a stream filled its output region"
            assert rate or (status == 0).all()
            rec = d_rec.download(np.uint8, N * P * efx.FRAME_BYTES).reshape(N, P, -1)
            psnr = float(np.mean([E.luma_psnr(src[i], rec[i]) for i in range(0, N, 64)]))
            best = min(ms)
            out[name] = {"gop": gop, "search": R, "pictures_per_s": N * P / (best / 1e3), "pictures_per_s_mean": N * P / (np.mean(ms) / 1e3),
                         "ms_per_call": best, "ms_mean": float(np.mean(ms)), "bytes_per_picture": float(lens.sum()) / (N * P),
                         "luma_psnr_db": round(psnr, 2)}
            if rate:  # (this source is noise-like: far more than 1500 kbit/s even at qscale 31, so its streams run into debt)
                out[name].update(rate, streams_in_debt=int((status & efx.ENCODE_VBV != 0).sum()))
    print(json.dumps(out))
    dec.close()


if __name__ == "__main__":
    main()
