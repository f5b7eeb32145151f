"""Measure what scene-cut detection costs the encoder (efx_encode_set_scene_cut: k_enc_cut, one more launch per picture):
1024 streams x 12 pictures, GOP 12, min_gop 6, qscale 8, search 7, TS, with the option off and on, for efx_encode and for
efx_encode_rc (1500 kbit/s under a 250 000-bit buffer, qmin 3).  The source is a texture panning by 4 pels a picture
(tests/encode_cut_model.py: motion the measure follows), rotated and xor-ed per stream as in bench_encode.py; every second
stream cuts to another texture at picture 6, so half the streams code a cut I picture there while the others code a P
picture in the same launches.  The leg `on_256` runs the measure at threshold 256, which no picture can exceed: the
bytes are those of `off`, so its time against `off` is the option's own cost, free of what an I picture in place of a P
picture changes.  Prints one JSON line: per leg the milliseconds
one picture of all streams takes (HIP events recorded on the library's own stream around one encode call, over its
pictures; best and mean of --steps timed calls after --warmup), pictures per second, bytes per picture and the I pictures
the cut rule placed.  The legs run --rounds times, off and on alternating, so the spread between equal runs shows next to
the difference.  `--legs rc_on --rounds 1` runs one leg alone for a `rocprofv3 --kernel-trace --stats` run, which gives
k_enc_cut's time next to k_enc_act's and k_enc_rows'."""
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
import encode_cut_model as CM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pictures", type=int, default=12)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=efx.SCENE_CUT_DEFAULT)
    ap.add_argument("--legs", default="", help="comma-separated leg names to run (default: all): off, on, on_256, rc_off, rc_on")
    args = ap.parse_args()
    N, P = args.streams, args.pictures
    base, cuts = CM.pan(P, cut_at=P), CM.pan(P, cut_at=P // 2)
    src = np.stack([np.roll(cuts if k & 1 else base, k * 97, axis=1) ^ np.uint8(k & 0x3F) for k in range(N)])
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    dec = efx.Decoder(N, 1, hip_stream=stream.value)  # the library runs on this stream: the events below bracket its launches
    stride = P * 128 * 1024  # well above what qscale 8 writes here, intra pictures included (checked: no EFX_ENCODE_FULL)
    st_off = (4 * N + 15) // 16 * 16
    d_src, d_dst, d_meta = dec.alloc(src.size), dec.alloc(N * stride), dec.alloc(2 * st_off)
    d_src.upload(src)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(ev0))
    hip.hipEventCreate(C.byref(ev1))
    rate = dict(bitrate=1_500_000, vbv_bits=250_000, qmin=3, qmax=31)
    cut = dict(scene_cut=args.threshold, min_gop=6)
    legs = [("off", {}), ("on", cut), ("on_256", {**cut, "scene_cut": 256}), ("rc_off", rate), ("rc_on", {**rate, **cut})]
    legs = [leg for leg in legs if not args.legs or leg[0] in args.legs.split(",")]
    out = {"streams": N, "pictures": P, "qscale": 8, "gop": 12, "search": 7, "format": "ts", "threshold": args.threshold, "min_gop": 6,
           "timing": "HIP events on the library's stream around one encode call, divided by its pictures; best and mean of the "
                     "timed calls; one entry per round", "legs": {name: [] for name, _ in legs}}
    for _ in range(args.rounds):
        for name, opts in legs:
            kw = dict(n_streams=N, n_pictures=P, qscale=8, gop=12, search=7, fmt=efx.FORMAT_TS, dst_stride=stride, **opts)
            for _ in range(args.warmup):
                dec.encode_to(d_src, d_dst, d_meta.ptr, d_meta.ptr + st_off, **kw)
            dec.sync()
            ms = []
            for _ in range(args.steps):
                hip.hipEventRecord(ev0, stream)
                dec.encode_to(d_src, d_dst, d_meta.ptr, d_meta.ptr + st_off, **kw)
                hip.hipEventRecord(ev1, stream)
                hip.hipEventSynchronize(ev1)
                t = C.c_float()
                hip.hipEventElapsedTime(C.byref(t), ev0, ev1)
                ms.append(t.value)
            dec.sync()
            lens = d_meta.download(np.uint32, N)
            status = np.empty(N, dtype=np.uint32)
            assert dec._lib.efx_memcpy_d2h(dec._ctx, status.ctypes.data, d_meta.ptr + st_off, 4 * N) == 0
            assert (status & efx.ENCODE_FULL == 0).all(), "a stream filled its output region"
            types = dec.encode_picture_info(N)["type"]
            out["legs"][name].append({"ms_per_picture": min(ms) / P, "ms_per_picture_mean": float(np.mean(ms)) / P,
                                      "pictures_per_s": N * P / (min(ms) / 1e3), "bytes_per_picture": float(lens.sum()) / (N * P),
                                      "cut_i_pictures": int((types == efx.PICTURE_CUT_I).sum()),
                                      "i_pictures": int((types == efx.PICTURE_I).sum())})
    print(json.dumps(out))
    dec.close()


if __name__ == "__main__":
    main()
