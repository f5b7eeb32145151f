#!/usr/bin/env python3
"""Throughput of k_telecine (efx_detelecine): telecined frames back to film frames at the source's size.

The case: 720 x 480 NV12, 64 streams of 30 frames each, synthetic 2-3 pulldown of a moving texture made on the host from
a seed (so that matches of both kinds and real drops occur), top field first.  The call is first checked byte for byte,
outputs and records, against the NumPy model (tests/telecine_model.py) on its first stream.  Then, after warm-up calls,
HIP events on the library's stream (a torch stream) around every single call: best and mean ms of the three launches
together, frames/s.  Next to it the yardstick, timed the same way in the same run: plain device-to-device copies (torch's
copy_) of the bytes each launch must move at the least -- the measure reads each frame's luma twice (once as the frame,
once as its successor's predecessor: 2 w h per frame, nothing written), the weave reads and writes 0.8 x 1.5 w h per
frame (four of five frames have an output); a copy of B bytes moves B / 2 in and B / 2 out.  Also timed, for comparison:
efx_deinterlace at the frame rate on the same frames.

Each launch's own time comes from a run of its own: unless --no-profile is given the tool starts itself again under
`rocprofv3 --kernel-trace --stats` (the timed loop only) and reads the three kernels' average and minimum durations out
of the kernel statistics.  Prints one JSON line."""
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
import espflix_amd as efx  # noqa: E402
import surface_model  # noqa: E402
import telecine_model  # noqa: E402

W, H, KIND = 720, 480, "nv12"
KERNELS = ("k_telecine_measure", "k_telecine_decide", "k_telecine_weave")


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


def pulldown_stream(n, seed):
    """n telecined NV12 frames of a texture that moves 3 samples right and 1 line down per film frame, with +-1 noise."""
    rng = np.random.default_rng(seed)
    film = []
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for k in range(n):
        xs, ys = x - 3 * k, y - k
        v = 128 + 50 * np.sin(2 * np.pi * xs / 41) + 30 * np.cos(2 * np.pi * (xs + 2 * ys) / 67) + 20 * np.sin(2 * np.pi * ys / 29)
        c = 128 + 40 * np.sin(2 * np.pi * (xs[::2, ::2] + ys[::2, ::2]) / 53)
        film.append(np.concatenate([np.rint(v).reshape(-1), np.rint(c).reshape(-1), np.rint(255 - c).reshape(-1)]).astype(np.uint8))
    video, _ = telecine_model.telecine(np.stack(film), W, H, telecine_model.TOP, int(rng.integers(0, 4)), int(rng.integers(0, 5)))
    video = video[:n]
    video = np.clip(video.astype(np.int16) + rng.integers(-1, 2, video.shape), 0, 255).astype(np.uint8)
    # packed I420 to NV12: the chroma planes interleaved
    ysz, csz = W * H, W * H // 4
    pairs = np.stack([video[:, ysz:ysz + csz], video[:, ysz + csz:]], axis=2).reshape(n, 2 * csz)
    return np.concatenate([video[:, :ysz], pairs], axis=1)


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
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-dir", default=os.path.join(ROOT, "bench_runs", "detelecine_profile"))
    ap.add_argument("--no-profile", action="store_true", help="leave the per-launch times out (no rocprofv3 run)")
    ap.add_argument("--inner", action="store_true", help="the timed loop alone, for the profiler")
    args = ap.parse_args()
    n_streams, n = args.streams, args.frames
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    surf, model = efx.surface_layout(KIND, W, H), surface_model.layout(KIND, W, H)
    image = W * H * 3 // 2
    assert surf.bytes == image and image % 16 == 0
    # eight different streams, repeated: the host makes the pulldown, the device only has to hold it
    few = np.stack([pulldown_stream(n, 100 + k) for k in range(min(8, n_streams))])
    host = np.concatenate([few[k % len(few)] for k in range(n_streams)])
    src = torch.from_numpy(host).cuda()
    n_out = efx.detelecine_count(n)
    dst = torch.empty((n_streams * n_out, image), dtype=torch.uint8, device="cuda")
    info = torch.full((n_streams * n, 32), 0xA5, dtype=torch.uint8, device="cuda")
    run = lambda: dec.detelecine_to(src.data_ptr(), dst.data_ptr(), info.data_ptr(), surface=surf, n_streams=n_streams, n_frames=n)
    stream.synchronize()
    assert run() == n_out
    dec.sync()
    if args.inner:
        timed_calls(stream, run, args.warmup, args.reps)
        dec.close()
        return
    want, recs = telecine_model.detelecine(few[0], model, 1)
    assert np.array_equal(dst[:n_out].cpu().numpy(), want[0]), "differs from the model"
    records = info.cpu().numpy().reshape(-1).view(telecine_model.INFO).reshape(n_streams, n)
    assert np.array_equal(records[0], recs[0]), "records differ from the model"
    ms = timed_calls(stream, run, args.warmup, args.reps)
    frames = n_streams * n
    moved = {"k_telecine_measure": 2 * W * H * frames, "k_telecine_weave": int(2 * 0.8 * 1.5 * W * H * frames)}
    out = {"case": f"{KIND} {W}x{H}, {n_streams} streams x {n} frames, top field first, synthetic 2-3 pulldown",
           "timing": "HIP events on the library's stream around each call; per launch: rocprofv3 kernel statistics of a run of its own",
           "frames_dropped": int((records["out"] < 0).sum()), "frames_matched_p": int((records["match"] == 1).sum()),
           "call": {"ms_best": round(min(ms), 4), "ms_mean": round(float(np.mean(ms)), 4), "frames_per_s": round(frames / min(ms) * 1e3)}}
    copies = {}
    for name, b in moved.items():
        a, c = torch.empty(b // 2, dtype=torch.uint8, device="cuda"), torch.empty(b // 2, dtype=torch.uint8, device="cuda")
        cms = timed_calls(stream, lambda: c.copy_(a), args.warmup, args.reps)
        del a, c
        copies[name] = min(cms)
        out[name] = {"bytes_moved_at_least": b, "copy_of_those_bytes": {"ms_best": round(min(cms), 4), "ms_mean": round(float(np.mean(cms)), 4),
                                                                      "gbps": round(b / min(cms) / 1e6, 1)}}
    # k_deint at the frame rate on the same frames: one launch that reads three frames and writes one per frame
    full = torch.empty((frames, image), dtype=torch.uint8, device="cuda")
    dms = timed_calls(stream, lambda: dec.deinterlace_to(src.data_ptr(), full.data_ptr(), surface=surf, n_streams=n_streams, n_frames=n,
                                                         rate="frame"), args.warmup, args.reps)
    del full
    out["k_deint_frame_rate_same_frames"] = {"ms_best": round(min(dms), 4), "ms_mean": round(float(np.mean(dms)), 4)}
    out["call"]["copy_of_both"] = round(sum(copies.values()), 4)
    out["call"]["call_over_copies"] = round(min(ms) / sum(copies.values()), 2)
    dec.close()
    if not args.no_profile:
        os.makedirs(args.profile_dir, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.profile_dir, "-o", "detelecine", "--", sys.executable, os.path.abspath(__file__),
               "--inner", "--no-profile", "--streams", str(n_streams), "--frames", str(n), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode:
            raise RuntimeError("the profiled run failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
        for name, (calls, avg_us, min_us) in kernel_stats(args.profile_dir).items():
            leg = out.setdefault(name, {})
            leg.update({"calls": calls, "us_mean": round(avg_us, 2), "us_best": round(min_us, 2)})
            if name in moved:
                leg["gbps"] = round(moved[name] / avg_us / 1e3, 1)
                leg["fraction_of_the_copys_rate"] = round(copies[name] * 1e3 / avg_us, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
