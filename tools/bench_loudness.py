#!/usr/bin/env python3
"""Time of the three loudness kernels' calls: efx_loudness_steps, efx_loudness_gate and efx_pcm_gain.

The shape: 1024 streams x 10 s of 48 kHz mono int16 (100 steps per stream), one call each.  Every call is timed in a
process of its own, started from here under a time limit (--limit seconds; the first one that fails or runs out ends the
run): HIP events on the library's stream (a torch stream) around back-to-back calls after a warm-up, the mean per call.
Before timing, the first and the last stream are checked against the NumPy model (tests/loudness_model.py).  Per call:
ms, ms per 1024 stream-seconds (the unit of the README's audio table), algorithmic bytes (samples read, records and
states read and written), GB/s and the fraction of the 8 TB/s HBM spec bench.py uses.  Prints one JSON line per call."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (bench.py's figure)
RATE = 48000
STEPS = ("steps", "gate", "gain")


def child(args):
    import numpy as np
    import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import espflix_amd as efx
    import loudness_model as M

    n, samples = args.streams, args.seconds * RATE
    n_steps = efx.loudness_step_count(RATE, 0, samples)
    stride = (samples + 7) // 8 * 8
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(n, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(n)
    # noise of about -20 dBFS, every fourth stream 20 dB quieter
    pcm = (torch.randn((n, stride), device="cuda", generator=gen) * 3276.8)
    pcm[::4] *= 0.1
    pcm = pcm.round().clamp(-32768, 32767).to(torch.int16)
    state = torch.zeros((n, efx.loudness_state_bytes(RATE)), dtype=torch.uint8, device="cuda")
    steps = torch.zeros((n, n_steps, 16), dtype=torch.uint8, device="cuda")
    recs = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(pcm)
    thr = efx.loudness_thresholds(RATE)
    stream.synchronize()

    def run_steps():
        state.zero_()  # (a fresh stream every call: the records stay those of the check)
        dec.loudness_steps_to(pcm.data_ptr(), state.data_ptr(), steps.data_ptr(), n_streams=n, n_samples=samples, rate=RATE,
                              pcm_stride=stride, steps_stride=n_steps)

    run_gate = lambda: dec.loudness_gate_to(steps.data_ptr(), state.data_ptr(), recs.data_ptr(), n_streams=n, n_steps=n_steps, rate=RATE,
                                            thresholds=thr, steps_stride=n_steps)
    run_gain = lambda: dec.pcm_gain_to(pcm.data_ptr(), recs.data_ptr(), out.data_ptr(), n_streams=n, n_samples=samples,
                                       src_stride=stride, dst_stride=stride)
    with torch.cuda.stream(stream):
        run_steps()
        run_gate()
        run_gain()
    dec.sync()
    for i in (0, n - 1):
        x = pcm[i, :samples].cpu().numpy()
        want = M.step_records(x, RATE)[0]
        got = steps[i].cpu().numpy().reshape(-1).view(M.STEP_DTYPE)
        assert np.array_equal(got, want), f"stream {i}: the step records differ from the model"
        rec = M.gate(want, RATE, thr, M.state(x, RATE)[0])
        assert recs[i].cpu().numpy().view(M.REC_DTYPE)[0] == rec, f"stream {i}: the record differs from the model"
        assert np.array_equal(out[i, :samples].cpu().numpy(), M.apply_gain(x, int(rec["gain_q12"]))), f"stream {i}: the scaled samples differ"
    state_bytes = efx.loudness_state_bytes(RATE)
    run, nbytes = {"steps": (run_steps, n * (2 * samples + 16 * n_steps + 2 * state_bytes)),
                   "gate": (run_gate, n * (16 * n_steps + state_bytes + 32)),
                   "gain": (run_gain, n * (4 * samples + 32))}[args.step]
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            run()
        e1.record(stream)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.reps
    gbps = nbytes / ms / 1e6
    note = "HIP events on the library's stream, mean over back-to-back calls"
    if args.step == "steps":
        note += "; each call includes k_loud_state and the memset that makes the streams fresh"
    print(json.dumps({"call": {"steps": "efx_loudness_steps", "gate": "efx_loudness_gate", "gain": "efx_pcm_gain"}[args.step],
                      "rate": RATE, "streams": n, "seconds_per_stream": args.seconds, "steps_per_stream": n_steps, "ms": round(ms, 4),
                      "ms_per_1024_stream_seconds": round(ms * 1024 / (n * args.seconds), 4), "bytes": nbytes, "gbps": round(gbps, 1),
                      "hbm_frac": round(gbps / HBM_PEAK_GBS, 4), "hbm_floor_ms": round(nbytes / HBM_PEAK_GBS / 1e6, 4), "timing": note}),
          flush=True)
    dec.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a timed call's process may take")
    ap.add_argument("--step", choices=STEPS, help="(the child processes' argument)")
    args = ap.parse_args()
    if args.step:
        return child(args)
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--streams", str(args.streams),
               "--seconds", str(args.seconds), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd)
        if r.returncode != 0:
            sys.exit(f"{step}: exit status {r.returncode}; nothing more is started")


if __name__ == "__main__":
    main()
