#!/usr/bin/env python3
"""Throughput of k_scan (efx_detect_scan): progressive, interlaced or telecined, per frame and per stream.

The case (the defaults; --width, --height, --streams, --frames change it): 720 x 480 NV12, 64 streams of 30 frames each,
synthetic 2-3 pulldown of a moving texture made on the host from a seed (tools/bench_detelecine.py's), top field first.
The call is first checked bit for bit, frame records and stream records, against the NumPy model (tests/scan_model.py) on
its first stream, whose verdict must be "telecined, top".  Then, after warm-up calls, HIP events on the library's stream
(a torch stream) around every single call: best and mean ms of the two launches together, frames/s.  Next to it the
yardstick, timed the same way in the same run: a plain device-to-device copy (torch's copy_) of the bytes the measuring
launch must move at the least -- each frame's luma twice (once as the frame, once as its successor's predecessor: 2 w h
per frame, nothing written); a copy of B bytes moves B / 2 in and B / 2 out.  Also timed: efx_detelecine's call on the
same frames, whose measuring launch reads the same rows and forms two combs and one difference where this one forms
three and two.

Each launch's own time comes from a run of its own: unless --no-profile is given the tool starts itself again under
`rocprofv3 --kernel-trace --stats` (the timed loops only) and reads the kernels' average and minimum durations out of the
kernel statistics.  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np
import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import espflix_amd as efx  # noqa: E402
import scan_model  # noqa: E402
import surface_model  # noqa: E402
import bench_detelecine as BD  # noqa: E402

KIND = "nv12"
KERNELS = ("k_scan_measure", "k_scan_count", "k_telecine_measure")


def kernel_stats(out_dir):
    """{kernel: (calls, average us, minimum us)} out of rocprofv3's kernel statistics under out_dir."""
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"no kernel statistics under {out_dir}")
    stats = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Name"].split("(")[0].split("::")[-1].replace(".kd", "")
        if name in KERNELS:
            stats[name] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3)
    if sorted(stats) != sorted(KERNELS):
        raise RuntimeError(f"kernels missing from {files[0]}: {sorted(stats)}")
    return stats


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-dir", default=os.path.join(ROOT, "bench_runs", "scan_profile"))
    ap.add_argument("--no-profile", action="store_true", help="leave the per-launch times out (no rocprofv3 run)")
    ap.add_argument("--inner", action="store_true", help="the timed loops alone, for the profiler")
    args = ap.parse_args()
    n_streams, n, w, h = args.streams, args.frames, args.width, args.height
    BD.W, BD.H = w, h   # (pulldown_stream makes frames of bench_detelecine's size)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    surf, model = efx.surface_layout(KIND, w, h), surface_model.layout(KIND, w, h)
    image = w * h * 3 // 2
    assert surf.bytes == image and image % 16 == 0
    # a few different streams, repeated: the host makes the pulldown, the device only has to hold it
    few = np.stack([BD.pulldown_stream(n, 100 + k) for k in range(min(4, n_streams))])
    host = np.concatenate([few[k % len(few)] for k in range(n_streams)])
    src = torch.from_numpy(host).cuda()
    frames = torch.full((n_streams * n, 48), 0xA5, dtype=torch.uint8, device="cuda")
    recs = torch.full((n_streams, 64), 0xA5, dtype=torch.uint8, device="cuda")
    run = lambda: dec.detect_scan_to(src.data_ptr(), frames.data_ptr(), recs.data_ptr(), surface=surf, n_streams=n_streams, n_frames=n)
    n_out = efx.detelecine_count(n)
    dst = torch.empty((n_streams * n_out, image), dtype=torch.uint8, device="cuda")
    info = torch.empty((n_streams * n, 32), dtype=torch.uint8, device="cuda")
    detelecine = lambda: dec.detelecine_to(src.data_ptr(), dst.data_ptr(), info.data_ptr(), surface=surf, n_streams=n_streams, n_frames=n)
    stream.synchronize()
    assert run() == n
    dec.sync()
    if args.inner:
        BD.timed_calls(stream, run, args.warmup, args.reps)
        BD.timed_calls(stream, detelecine, args.warmup, args.reps)
        dec.close()
        return
    want_f, want_r = scan_model.scan(few[0], model, 1)
    got_f = frames.cpu().numpy().reshape(-1).view(scan_model.FRAME).reshape(n_streams, n)
    got_r = recs.cpu().numpy().reshape(-1).view(scan_model.REC)
    assert np.array_equal(got_f[0], want_f[0]) and got_r[0].tobytes() == want_r[0].tobytes(), "differs from the model"
    verdict = efx.scan_verdict(got_r[0])
    assert (verdict.kind, verdict.first_field) == ("telecined", "top"), verdict
    ms = BD.timed_calls(stream, run, args.warmup, args.reps)
    total = n_streams * n
    moved = 2 * w * h * total
    a, c = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    cms = BD.timed_calls(stream, lambda: c.copy_(a), args.warmup, args.reps)
    del a, c
    tms = BD.timed_calls(stream, detelecine, args.warmup, args.reps)
    out = {"case": f"{KIND} {w}x{h}, {n_streams} streams x {n} frames, synthetic 2-3 pulldown, default options",
           "timing": "HIP events on the library's stream around each call; per launch: rocprofv3 kernel statistics of a run of its own",
           "labels": {name: int((got_f["label"] == v).sum()) for name, v in (("none", 0), ("still", 1), ("progressive", 2), ("tff", 3), ("bff", 4),
                                                                              ("undetermined", 5))},
           "call": {"ms_best": round(min(ms), 4), "ms_mean": round(float(np.mean(ms)), 4), "frames_per_s": round(total / min(ms) * 1e3)},
           "luma_bytes_moved_at_least": moved,
           "copy_of_those_bytes": {"ms_best": round(min(cms), 4), "ms_mean": round(float(np.mean(cms)), 4), "gbps": round(moved / min(cms) / 1e6, 1)},
           "call_fraction_of_the_copys_rate": round(min(cms) / min(ms), 3),
           "efx_detelecine_call_same_frames": {"ms_best": round(min(tms), 4), "ms_mean": round(float(np.mean(tms)), 4)}}
    dec.close()
    if not args.no_profile:
        os.makedirs(args.profile_dir, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.profile_dir, "-o", "scan", "--", sys.executable,
               os.path.abspath(__file__), "--inner", "--no-profile", "--width", str(w), "--height", str(h), "--streams", str(n_streams),
               "--frames", str(n), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode:
            raise RuntimeError("the profiled run failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
        stats = kernel_stats(args.profile_dir)
        for name, (calls, avg_us, min_us) in stats.items():
            out[name] = {"calls": calls, "us_mean": round(avg_us, 2), "us_best": round(min_us, 2)}
            if name != "k_scan_count":
                out[name]["gbps"] = round(moved / avg_us / 1e3, 1)
                out[name]["fraction_of_the_copys_rate"] = round(min(cms) * 1e3 / avg_us, 3)
        out["k_scan_measure_over_k_telecine_measure"] = round(stats["k_scan_measure"][1] / stats["k_telecine_measure"][1], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
