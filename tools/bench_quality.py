#!/usr/bin/env python3
"""Throughput of k_quality (efx_compare_pictures): PSNR and SSIM of a batch of pictures against a reference batch.

Cases: 1024 x 12 and 16 x 12 pictures (the encode benchmark's batch, and one of a low count).  The pictures are made on
the device with torch: noise, and the same noise disturbed by up to +-6.  Each case is first checked bit for bit against
the NumPy model (tests/quality_model.py: the records and maps of the first and the last image).  Then per call, after
warm-up calls, HIP events on the library's stream (a torch stream) around every single call: best and mean ms, images/s,
GB/s over the algorithmic bytes (2 x 101376 per image; the records are negligible) and the fraction of the 8 TB/s HBM
spec bench.py uses.  Next to it a plain device copy of the same bytes (torch's copy_ of both batches, which reads and
writes them), and the host path this call replaces: downloading the pictures under test in full and NumPy's
encode_model.luma_psnr against the source -- on every picture of the small case, on every 64th stream of the large one
(what tools/bench_encode.py does), with the time for all streams extrapolated.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import espflix_amd as efx  # noqa: E402
import encode_model  # noqa: E402
import quality_model  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (bench.py's figure)
PIC = efx.FRAME_BYTES


def timed_calls(stream, run, warmup, reps):
    """ms of every one of reps calls, each between two events on the stream."""
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            run()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, nargs="+", default=[1024, 16])
    ap.add_argument("--pictures", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-max", type=int, default=248)
    ap.add_argument("--no-host", action="store_true", help="skip the host path")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    out = {"timing": "HIP events on the library's stream around each call", "ref_max": args.ref_max, "hbm_peak_gbs": HBM_PEAK_GBS}
    for N in args.streams:
        P = args.pictures
        n = N * P
        gen = torch.Generator(device="cuda").manual_seed(n)
        ref = torch.randint(0, 256, (n, PIC), dtype=torch.uint8, device="cuda", generator=gen)
        test = (ref.to(torch.int16) + torch.randint(-6, 7, (n, PIC), dtype=torch.int16, device="cuda", generator=gen)).clamp_(0, 255).to(torch.uint8)
        recs = torch.empty((n, 6), dtype=torch.int64, device="cuda")
        maps = torch.empty((n, 264), dtype=torch.int32, device="cuda")
        stream.synchronize()
        dec.compare_to(ref.data_ptr(), test.data_ptr(), recs.data_ptr(), n_images=n, ref_max=args.ref_max, mb_sse=maps.data_ptr())
        dec.sync()
        check = [0, n - 1]
        sse, ssim, mb = quality_model.compare_batch(ref[check].cpu().numpy(), test[check].cpu().numpy(), args.ref_max)
        got = recs[check].cpu().numpy()
        assert np.array_equal(got[:, :3].view(np.uint64), sse) and np.array_equal(got[:, 3:], ssim), "records differ from the model"
        assert np.array_equal(maps[check].cpu().numpy().view(np.uint32), mb), "macroblock maps differ from the model"
        read = 2 * n * PIC
        case = {"streams": N, "pictures": P, "images": n, "bytes_read": read}
        for name, mb_ptr in (("records", None), ("records_and_maps", maps.data_ptr())):
            run = lambda: dec.compare_to(ref.data_ptr(), test.data_ptr(), recs.data_ptr(), n_images=n, ref_max=args.ref_max, mb_sse=mb_ptr)
            ms = timed_calls(stream, run, args.warmup, args.reps)
            best, mean = min(ms), float(np.mean(ms))
            case[name] = {"ms_best": round(best, 4), "ms_mean": round(mean, 4), "images_per_s": round(n / best * 1e3),
                          "gbps": round(read / best / 1e6, 1), "hbm_frac": round(read / best / 1e6 / HBM_PEAK_GBS, 4)}
        run = lambda: dec.compare_to(ref.data_ptr(), test.data_ptr(), recs.data_ptr(), n_images=n, ref_max=0)
        ms = timed_calls(stream, run, args.warmup, args.reps)
        case["records_no_clamp"] = {"ms_best": round(min(ms), 4), "ms_mean": round(float(np.mean(ms)), 4),
                                    "gbps": round(read / min(ms) / 1e6, 1), "hbm_frac": round(read / min(ms) / 1e6 / HBM_PEAK_GBS, 4)}
        # a plain copy of the same bytes: reads them once and writes them once
        dst = torch.empty_like(ref)
        def copy():
            dst.copy_(ref)
            dst.copy_(test)
        ms = timed_calls(stream, copy, args.warmup, args.reps)
        case["device_copy_of_the_same_bytes"] = {"ms_best": round(min(ms), 4), "ms_mean": round(float(np.mean(ms)), 4),
                                                 "read_gbps": round(read / min(ms) / 1e6, 1)}
        del dst
        if not args.no_host:
            step = 64 if N >= 128 else 1
            t0 = time.perf_counter()
            rec_host = test.cpu().numpy().reshape(N, P, PIC)
            t1 = time.perf_counter()
            src_host = ref.cpu().numpy().reshape(N, P, PIC)   # (the source is the caller's: not timed)
            t2 = time.perf_counter()
            psnr = float(np.mean([encode_model.luma_psnr(src_host[i], rec_host[i]) for i in range(0, N, step)]))
            t3 = time.perf_counter()
            measured = len(range(0, N, step))
            if args.ref_max == 248:  # (luma_psnr's convention: the device's numbers give the same mean)
                dec.compare_to(ref.data_ptr(), test.data_ptr(), recs.data_ptr(), n_images=n, ref_max=248)
                dec.sync()
                luma_sse = recs[:, 0].cpu().numpy().view(np.uint64).reshape(N, P)[::step]
                dev = float(np.mean([efx.compare_psnr(int(v)) for v in luma_sse.reshape(-1)]))
                assert abs(dev - psnr) < 1e-9, (dev, psnr)
            case["host_path"] = {"what": "download of the pictures under test + NumPy luma PSNR (no SSIM)", "download_ms": round((t1 - t0) * 1e3, 2),
                                 "numpy_streams_measured": measured, "numpy_ms": round((t3 - t2) * 1e3, 2),
                                 "total_ms_as_measured": round((t1 - t0 + t3 - t2) * 1e3, 2),
                                 "total_ms_all_streams": round((t1 - t0 + (t3 - t2) * N / measured) * 1e3, 2), "luma_psnr_db": round(psnr, 4)}
            del rec_host, src_host
        out[f"{N}x{P}"] = case
        del ref, test, recs, maps
        torch.cuda.empty_cache()
    print(json.dumps(out))
    dec.close()


if __name__ == "__main__":
    main()
