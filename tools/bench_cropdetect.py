#!/usr/bin/env python3
"""Throughput of k_cropdetect (efx_detect_crop): the black borders of source pictures, one rectangle per stream.

Cases: 1920 x 1080 RGB24 and 1280 x 720 I420, each at 64 and 1024 images (streams of 16 images).  Sources are generated
on the device with torch: noise inside a window, black bars around it.  Each case is first checked bit for bit against
the NumPy model (tests/crop_model.py: every record, and the sums of the first and the last image).  Then per call -- 10
back to back after 2 of warm-up, HIP events on the library's stream (a torch stream): ms, images/s, GB/s over the
algorithmic bytes (I420: W x H, RGB: 3 W x H; the records are negligible) and the fraction of the 8 TB/s HBM spec
bench.py uses.  Next to each case: the torch formulation of the same job on the same device -- an integer matrix for
luma, sum(dim), comparisons, argmax -- timed the same way and checked against the same records.  Prints one JSON line
per case and implementation, and whether the kernel is at least as fast as torch on that row."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import espflix_amd as efx  # noqa: E402
import crop_model  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (bench.py's figure)
CASES = [("rgb24", 1920, 1080), ("i420", 1280, 720)]
PER_STREAM = 16
LIMIT, ROUND = 24, 16


def make_sources(fmt, w, h, n, gen):
    """(n, image bytes) uint8 on the device: noise in a window that differs from stream to stream, black outside."""
    image = efx.import_src_bytes(fmt, w, h)
    src = torch.randint(60, 256, (n, image), dtype=torch.uint8, device="cuda", generator=gen)
    view = src.view(n, h, w, 3) if fmt == "rgb24" else src[:, :w * h].view(n, h, w)
    black = 0 if fmt == "rgb24" else 16
    for s in range(0, n, PER_STREAM):
        k = s // PER_STREAM
        top, left = 40 + 2 * (k % 50), 8 * (k % 20)
        view[s:s + PER_STREAM, :top] = black
        view[s:s + PER_STREAM, h - top - 3:] = black
        view[s:s + PER_STREAM, :, :left] = black
        view[s:s + PER_STREAM, :, w - left - 5:] = black
    return src


def torch_detect(src, fmt, w, h, weights):
    """The same job in torch ops: (n_streams, 8) int32 records.  Integer throughout, so it is exact too."""
    n = src.shape[0]
    if fmt == "rgb24":
        rgb = src.view(n, h, w, 3).to(torch.int32)
        luma = (((rgb * weights).sum(dim=3) + 128) >> 8) + 16   # (no clamp needed: 16 .. 235)
    else:
        luma = src[:, :w * h].view(n, h, w).to(torch.int32)
    rows = luma.sum(dim=2) > LIMIT * w
    cols = luma.sum(dim=1) > LIMIT * h
    contributes = rows.any(dim=1) & cols.any(dim=1)

    def first_last(mask, size):
        first = mask.to(torch.int32).argmax(dim=1)
        last = size - 1 - mask.flip(1).to(torch.int32).argmax(dim=1)
        first = torch.where(contributes, first, torch.full_like(first, size))
        last = torch.where(contributes, last, torch.full_like(last, -1))
        return first.view(-1, PER_STREAM).amin(dim=1), last.view(-1, PER_STREAM).amax(dim=1)

    def axis(a, b, size):
        a1 = a + (a & 1)
        avail = b + 1 - a1
        length = torch.where(avail >= ROUND, avail - avail % ROUND, avail & ~1)
        pos = a1 + (((avail - length) >> 1) & ~1)
        return pos, length, avail >= 2

    y1, y2 = first_last(rows, h)
    x1, x2 = first_last(cols, w)
    px, lw, okx = axis(x1, x2, w)
    py, lh, oky = axis(y1, y2, h)
    ok = okx & oky & (x2 >= 0)
    zero = torch.zeros_like(px)
    rec = torch.stack([torch.where(ok, px, zero), torch.where(ok, py, zero), torch.where(ok, lw, zero + w),
                       torch.where(ok, lh, zero + h), x1, y1, x2, y2], dim=1)
    return rec.to(torch.int32)


def timed(stream, run, warmup, reps):
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            run()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    weights = torch.tensor([66, 129, 25], dtype=torch.int32, device="cuda")
    slower = 0
    for fmt, w, h in CASES:
        image = efx.import_src_bytes(fmt, w, h)
        assert image % 16 == 0
        for n in args.images:
            assert n % PER_STREAM == 0
            n_streams = n // PER_STREAM
            src = make_sources(fmt, w, h, n, torch.Generator(device="cuda").manual_seed(n + w))
            rects = torch.empty((n_streams, 8), dtype=torch.int32, device="cuda")
            sums = torch.empty((n, (h + w + 3) // 4 * 4), dtype=torch.int32, device="cuda")
            run = lambda: dec.detect_crop_to(src.data_ptr(), rects.data_ptr(), n_streams=n_streams, images_per_stream=PER_STREAM,
                                             fmt=fmt, width=w, height=h, limit=LIMIT, round=ROUND, sums=sums.data_ptr())
            stream.synchronize()
            run()
            dec.sync()
            check = [0, n - 1]
            want_sums = np.stack([crop_model.sums(s, fmt, w, h) for s in src[check].cpu().numpy()])
            assert np.array_equal(sums[check, :h + w].cpu().numpy().view(np.uint32), want_sums), f"{fmt} {w}x{h}: sums differ from the model"
            # (the model's records from the device's sums of every image, which the torch formulation confirms below)
            all_sums = sums[:, :h + w].cpu().numpy().view(np.uint32)
            want = np.stack([crop_model.record(all_sums[i:i + PER_STREAM], w, h, LIMIT, ROUND) for i in range(0, n, PER_STREAM)])
            got = rects.cpu().numpy()
            assert np.array_equal(got, want), f"{fmt} {w}x{h}: records differ from the model"
            assert (got[:, 2] < w).all() and (got[:, 3] < h).all()
            # timed without the sums output: the library's scratch, as import_pictures(crop="auto") calls it
            run = lambda: dec.detect_crop_to(src.data_ptr(), rects.data_ptr(), n_streams=n_streams, images_per_stream=PER_STREAM,
                                             fmt=fmt, width=w, height=h, limit=LIMIT, round=ROUND)
            run()
            dec.sync()
            read = n * (w * h if fmt == "i420" else 3 * w * h)
            base = {"format": fmt, "width": w, "height": h, "images": n, "streams": n_streams, "bytes_read": read,
                    "timing": "HIP events on the library's stream, mean over back-to-back calls"}
            ms = timed(stream, run, args.warmup, args.reps)
            gbps = read / ms / 1e6
            print(json.dumps({"impl": "k_cropdetect", **base, "ms": round(ms, 4), "images_per_s": round(n / ms * 1e3),
                              "gbps": round(gbps, 1), "hbm_frac": round(gbps / HBM_PEAK_GBS, 4)}), flush=True)
            if not args.no_torch:
                try:
                    # (chunks of 64 images: the int32 planes of 1024 full-HD pictures would not fit beside the source)
                    run_t = lambda: torch.cat([torch_detect(src[i:i + 64], fmt, w, h, weights) for i in range(0, n, 64)])
                    same = bool(np.array_equal(run_t().cpu().numpy(), want))
                    ms_t = timed(stream, run_t, 1, max(1, args.reps // 3))
                    slower += ms > ms_t
                    print(json.dumps({"impl": "torch int matrix + sum + compare + argmax", **base, "ms": round(ms_t, 4),
                                      "images_per_s": round(n / ms_t * 1e3), "records_equal": same,
                                      "kernel_at_least_as_fast": bool(ms <= ms_t)}), flush=True)
                except Exception as e:  # the comparison must not take the measurement down
                    print(json.dumps({"impl": "torch int matrix + sum + compare + argmax", **base, "error": repr(e)[:300]}), flush=True)
            del src, rects, sums
            torch.cuda.empty_cache()
    dec.close()
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
