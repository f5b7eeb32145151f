#!/usr/bin/env python3
"""Throughput of k_trick (efx_trick_pick): the pictures of a title that make its fast-forward and rewind streams.

Cases: 64 streams x 360 pictures and 8 streams x 90 pictures at speed 15, fwd + rwd in one call, from I420 pictures in
device memory and from the frame rings (synthetic streams of 5-slice pictures, decoded once; a decode holds at most 255
pictures, so the ring source offers min(pictures, 255): 64 x 255 for the large case).  Each case is first checked bit for bit: the I420 source against the torch formulation, the ring source against
one efx_export_frames call per picked picture.  Then per call -- 20 back to back after 3 of warm-up, HIP events on the
library's stream (a torch stream): ms, GB/s over the algorithmic bytes (every picked picture read once and written twice)
and the fraction of the 6.3 TB/s an element-wise kernel reaches on this part.  Next to each case, timed the same way, the
ways the parent commit offers: p[:, ::15].contiguous() and .flip(1) for the I420 source, two efx_export_frames calls per
picked picture (its fwd and its rwd place) for the ring source.  Last: titles per second of Decoder.make_title (a host
clock around the call, which synchronises).  Prints one JSON line per case and implementation."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import espflix_amd as efx  # noqa: E402
from espflix_amd import gen  # noqa: E402

ELEMENTWISE_GBS = 6300.0  # the element-wise ceiling of the part (about 6.3 TB/s), the yardstick of hbm_frac
PIC = efx.FRAME_BYTES
SPEED = 15


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


def report(impl, base, ms, moved, **more):
    gbps = moved / ms / 1e6
    print(json.dumps({"impl": impl, **base, "ms": round(ms, 4), "gbps": round(gbps, 1),
                      "elementwise_frac": round(gbps / ELEMENTWISE_GBS, 4), **more}), flush=True)


def bench_i420(dec, stream, n, P, args):
    K = efx.trick_count(0, P, SPEED)
    src = torch.randint(0, 256, (n, P, PIC), dtype=torch.uint8, device="cuda")
    fwd = torch.zeros((n, K, PIC), dtype=torch.uint8, device="cuda")
    rwd = torch.zeros((n, K, PIC), dtype=torch.uint8, device="cuda")
    run = lambda: dec.trick_pick_to(src.data_ptr(), fwd.data_ptr(), rwd.data_ptr(), n_streams=n, n_pictures=P, speed=SPEED,
                                    total_pictures=P)
    torch_run = lambda: (src[:, ::SPEED].contiguous(), src[:, ::SPEED].flip(1))
    stream.synchronize()
    run()
    dec.sync()
    want_f, want_r = torch_run()
    assert torch.equal(fwd, want_f) and torch.equal(rwd, want_r), "k_trick differs from the torch formulation"
    moved = 3 * n * K * PIC
    base = {"source": "i420", "streams": n, "pictures": P, "speed": SPEED, "picks": K, "bytes_moved": moved,
            "timing": "HIP events on the library's stream, mean over back-to-back calls"}
    ms = timed(stream, run, args.warmup, args.reps)
    report("k_trick", base, ms, moved)
    ms_t = timed(stream, torch_run, args.warmup, args.reps)
    report("torch p[:, ::15].contiguous() + .flip(1)", base, ms_t, moved, kernel_at_least_as_fast=bool(ms <= ms_t))
    # (the torch formulation reads every pick twice: 4 x the picked bytes cross the memory system)
    del src, fwd, rwd
    torch.cuda.empty_cache()


def bench_ring(stream, n, P, args):
    P = min(P, 255)  # max_pictures of a context: the most one decode, and so one ring pick, holds
    K = efx.trick_count(0, P, SPEED)
    batch = gen.Batch(900, n, P, 12, gen.FLAG_WIDE_SLICES, threads=min(16, os.cpu_count() or 1))
    ts = [batch.ts(i) for i in range(n)]
    dec = efx.Decoder(n, P, P + 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream,
                      max_stream_bytes=sum(len(t) for t in ts) + 4096 * n)
    dec.upload(ts, efx.FORMAT_TS)
    dec.decode()
    assert all(dec.stream_status(i) == 0 and dec.picture_count(i) == P for i in range(n)), "the synthetic streams must decode"
    fwd = torch.zeros((n, K, PIC), dtype=torch.uint8, device="cuda")
    rwd = torch.zeros((n, K, PIC), dtype=torch.uint8, device="cuda")
    fwd_e, rwd_e = torch.zeros_like(fwd), torch.zeros_like(rwd)
    run = lambda: dec.trick_pick_to(None, fwd.data_ptr(), rwd.data_ptr(), n_streams=n, n_pictures=P, speed=SPEED,
                                    total_pictures=P, source=efx.TRICK_FROM_RING)

    def export_run():
        for k in range(K):
            dec.export_to(fwd_e.data_ptr() + k * PIC, "i420", n_streams=n, picture=k * SPEED, dst_stride=K * PIC)
            dec.export_to(rwd_e.data_ptr() + (K - 1 - k) * PIC, "i420", n_streams=n, picture=k * SPEED, dst_stride=K * PIC)

    stream.synchronize()
    run()
    export_run()
    dec.sync()
    assert torch.equal(fwd, fwd_e) and torch.equal(rwd, rwd_e), "k_trick differs from efx_export_frames"
    assert torch.equal(rwd, fwd.flip(1)) and int(fwd.max()) > 0
    moved = 3 * n * K * PIC
    base = {"source": "ring", "streams": n, "pictures": P, "speed": SPEED, "picks": K, "bytes_moved": moved,
            "timing": "HIP events on the library's stream, mean over back-to-back calls"}
    ms = timed(stream, run, args.warmup, args.reps)
    report("k_trick", base, ms, moved)
    ms_e = timed(stream, export_run, args.warmup, args.reps)
    report("2 efx_export_frames calls per picked picture", base, ms_e, moved, launches=2 * K, kernel_at_least_as_fast=bool(ms <= ms_e))
    dec.close()
    del fwd, rwd, fwd_e, rwd_e
    torch.cuda.empty_cache()


def bench_make_title(stream, n, P, args):
    """Titles per second of make_title: smooth synthetic pictures (a drifting gradient with noise), P / 30 s of a tone."""
    g = torch.Generator(device="cuda").manual_seed(5)
    y, x = torch.meshgrid(torch.arange(192, device="cuda"), torch.arange(352, device="cuda"), indexing="ij")
    pics = torch.empty((n, P, PIC), dtype=torch.uint8, device="cuda")
    for p in range(P):
        luma = ((x + 2 * p) % 256 + (y + p) % 64).clamp(16, 235).to(torch.uint8)
        pics[:, p, :352 * 192] = luma.reshape(-1)
        pics[:, p, 352 * 192:] = 128
    pics[:, :, :352 * 192:7] += torch.randint(0, 8, pics[:, :, :352 * 192:7].shape, dtype=torch.uint8, device="cuda", generator=g)
    samples = (P * 1600 + 127) // 128 * 128  # 48 kHz at 30 pictures per second, whole SBC frames
    t = torch.arange(samples, device="cuda")
    pcm = (6000 * torch.sin(2 * np.pi * 440 * t / 48000)).round().to(torch.int16).repeat(n, 1)
    dec = efx.Decoder(n, 1, 2, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream, max_stream_bytes=64 << 20)
    opts = dict(speed=SPEED, bitrate=1_500_000, qscale=8, gop=12, search=7)
    stream.synchronize()
    titles, st = dec.make_title(pics[:, :min(P, 24)], pcm[:, :3200 * 12], **opts)  # warm-up: code objects, allocations
    best = None
    for _ in range(args.title_reps):
        t0 = time.perf_counter()
        titles, st = dec.make_title(pics, pcm, **opts)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    sizes = {k: int(np.mean([len(t[k]) for t in titles])) for k in titles[0]}
    print(json.dumps({"impl": "make_title", "streams": n, "pictures": P, "speed": SPEED, "seconds": round(best, 3),
                      "titles_per_s": round(n / best, 2), "pictures_per_s": round(n * P / best), "status_or": int(np.bitwise_or.reduce(st, axis=None)),
                      "mean_bytes": sizes, "timing": "host clock around the call (it synchronises), best of %d" % args.title_reps}),
          flush=True)
    dec.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", type=int, nargs="+", default=[64, 360, 8, 90], help="streams pictures [streams pictures ...]")
    ap.add_argument("--title-shape", type=int, nargs=2, default=[64, 240], help="streams pictures of make_title (<= 255 pictures)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--title-reps", type=int, default=2)
    ap.add_argument("--no-ring", action="store_true")
    ap.add_argument("--no-title", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    for n, P in zip(args.shapes[0::2], args.shapes[1::2]):
        bench_i420(dec, stream, n, P, args)
    dec.close()
    if not args.no_ring:
        for n, P in zip(args.shapes[0::2], args.shapes[1::2]):
            bench_ring(stream, n, P, args)
    if not args.no_title:
        bench_make_title(stream, args.title_shape[0], args.title_shape[1], args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
