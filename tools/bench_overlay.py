#!/usr/bin/env python3
"""Throughput of k_overlay (efx_overlay) against a copy of the pictures it works on.

1024 streams x 12 pictures of 352 x 192 I420 (1.25 GB) on the device, blended in place:
  subtitle  a 320 x 32 alpha mask (EFX_OVL_A8) at (16, 152), shown on every second picture: six events of one picture each
            that share the bitmap, every stream.
  logo      a 48 x 24 RGBA bitmap at (296, 8) on every picture: one event.
  scan      the subtitle's list on pictures 1000 .. 1011 of the title, where none of it is shown: what the launch and the
            walk over the list cost before anything is blended.
  copy      the yardstick: a plain device-to-device copy (torch's copy_) of the same picture bytes.
Each step runs in a process of its own under a time limit of its own, one after the other, and the run ends at the first
that fails.  A step checks its first stream byte for byte against the NumPy model (tests/overlay_model.py), then, after
warm-up calls, puts HIP events on the library's stream (a torch stream) around every single call -- the call is one
launch: best and mean ms.  Blending in place again and again changes the bytes, not the work: the same chunks are read
and written every time.

Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("subtitle", "logo", "scan", "copy")
PICTURE = 101376


def timed_calls(torch, stream, run, warmup, reps):
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


def step(name, args):
    import numpy as np
    import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import espflix_amd as efx
    import overlay_model as M

    n, P = args.streams, args.pictures
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    g = torch.Generator(device="cuda").manual_seed(7)
    pics = torch.randint(0, 256, (n, P, PICTURE), dtype=torch.uint8, device="cuda", generator=g)
    stream.synchronize()
    total = n * P * PICTURE
    if name == "copy":
        other = torch.empty_like(pics)
        ms = timed_calls(torch, stream, lambda: other.copy_(pics), args.warmup, args.reps)
        return {"step": name, "bytes_copied": total, "ms_best": round(min(ms), 4), "ms_mean": round(float(np.mean(ms)), 4),
                "gbps_read_plus_written": round(2 * total / min(ms) / 1e6, 1)}
    rng = np.random.default_rng(8)
    first = 1000 if name == "scan" else 0
    if name in ("subtitle", "scan"):
        mask = rng.integers(0, 256, (32, 320), dtype=np.uint8)
        mask[rng.random(mask.shape) < 0.5] = 0  # (text: half of the box is empty)
        ovs = [efx.Overlay(mask, p, p, 16, 152) for p in range(0, P, 2)]
        touched = 0 if first else len(ovs) * n * (32 * 320 + 2 * 16 * 176)  # (16-byte chunks: every chroma chunk of the 16 rows)
    else:
        logo = rng.integers(0, 256, (24, 48, 4), dtype=np.uint8)
        ovs = [efx.Overlay(logo, 0, P - 1, 296, 8, opacity=200)]
        touched = P * n * (24 * 64 + 2 * 12 * 32)  # (16-byte chunks: columns 288 .. 351)
    events, atlas = efx.overlay_pack(ovs)
    assert efx.overlay_check(events, atlas.size) == -1
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    ev, at, st = dec.alloc(events.nbytes), dec.alloc(atlas.size), dec.alloc(4 * n)
    ev.upload(events)
    at.upload(atlas)
    st.upload(np.zeros(n, dtype=np.uint32))
    before = pics[:1].cpu().numpy()
    run = lambda: dec.overlay_to(pics.data_ptr(), ev, at, n_streams=n, n_pictures=P, n_events=len(events), atlas_bytes=atlas.size, status=st,
                                 first_picture=first)
    run()
    dec.sync()
    assert np.array_equal(pics[:1].cpu().numpy(), M.overlay(before, events, atlas, first_picture=first)), "differs from the model"
    assert first or not np.array_equal(pics[:1].cpu().numpy(), before)
    assert not st.download(np.uint32, n).any()
    ms = timed_calls(torch, stream, run, args.warmup, args.reps)
    dec.close()
    return {"step": name, "events": len(events), "pictures": n * P, "picture_bytes": total, "bytes_read_and_written_at_least": 2 * touched,
            "ms_best": round(min(ms), 4), "ms_mean": round(float(np.mean(ms)), 4), "gbps_of_touched_bytes": round(2 * touched / min(ms) / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pictures", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--step", choices=STEPS, help="run this step alone, in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args.step, args)))
        return 0
    out = {"timing": "HIP events on the library's stream around each call (one launch); the copy timed the same way; a process per step",
           "load": f"{args.streams} streams x {args.pictures} pictures of 352 x 192 I420", "steps": {}}
    for name in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [f"--{k}={getattr(args, k)}" for k in ("streams", "pictures", "reps", "warmup")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out["failed"] = f"{name}: no result within {args.limit} s"
            break
        if r.returncode != 0:
            out["failed"] = f"{name}: exit status {r.returncode}: {r.stderr[-1000:]}"
            break
        out["steps"][name] = json.loads(r.stdout.strip().split("\n")[-1])
    s = out["steps"]
    if all(k in s for k in STEPS):
        out["subtitle_over_copy"] = round(s["subtitle"]["ms_best"] / s["copy"]["ms_best"], 3)
        out["logo_over_copy"] = round(s["logo"]["ms_best"] / s["copy"]["ms_best"], 3)
        out["scan_over_copy"] = round(s["scan"]["ms_best"] / s["copy"]["ms_best"], 3)
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
