#!/usr/bin/env python3
"""Time of the peak limiter's two calls, efx_limit_peaks and efx_pcm_limit, with efx_pcm_gain beside them as the yardstick.

The shape of profiles/loudness.md: 1024 streams x 10 s of 48 kHz mono int16, one call each.  Noise of about -20 dBFS, every
fourth stream 20 dB quieter and with a 2 ms burst near full scale each second, so that its peak caps efx_pcm_gain's gain and the limiter
acts on it.  The streams are measured once (efx_loudness_steps, efx_loudness_gate); then the three calls are timed in ONE
process on the same buffers, alternated round by round: HIP events on the library's stream (a torch stream) around every
single call after a warm-up; the median, the smallest and the largest over the rounds.  The process runs under a time limit
(--limit seconds).  Before timing, the first stream (bursts) and the last (none) are checked against the NumPy model
(tests/limit_model.py, tests/loudness_model.py) bit for bit.  Per call: ms, algorithmic bytes (peaks: samples read and
peaks written; limit: samples read and written, the peaks and the records read; gain: samples read and written, the
records), GB/s, the fraction of the 8 TB/s HBM spec bench.py uses, and the ratio to efx_pcm_gain.  Prints one JSON line per
call."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (bench.py's figure)
RATE = 48000


def child(args):
    import numpy as np
    import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import espflix_amd as efx
    import limit_model as M
    import loudness_model as L

    n, samples, H = args.streams, args.seconds * RATE, args.half_window
    bk = efx.limit_block(RATE)
    nb = -(-samples // bk)
    n_steps = efx.loudness_step_count(RATE, 0, samples)
    stride = (samples + 7) // 8 * 8
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(n, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(n)
    pcm = torch.randn((n, stride), device="cuda", generator=gen) * 3276.8
    pcm[::4] *= 0.1  # (20 dB quieter: a gain of some 20 dB, which the bursts' peak would cap at -1 dB)
    t = torch.arange(96, device="cuda") / RATE
    burst = 31000.0 * torch.sin(2 * torch.pi * 1000.0 * t)
    for s in range(args.seconds):
        at = s * RATE + RATE // 3
        pcm[::4, at:at + 96] += burst
    pcm = pcm.round().clamp(-32768, 32767).to(torch.int16)
    state = torch.zeros((n, efx.loudness_state_bytes(RATE)), dtype=torch.uint8, device="cuda")
    steps = torch.zeros((n, n_steps, 16), dtype=torch.uint8, device="cuda")
    recs = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    peaks = torch.zeros((n, nb), dtype=torch.int16, device="cuda")
    out = torch.zeros_like(pcm)
    out_gain = torch.zeros_like(pcm)
    thr = efx.loudness_thresholds(RATE)
    stream.synchronize()

    run_peaks = lambda: dec.limit_peaks_to(pcm.data_ptr(), peaks.data_ptr(), n_streams=n, n_samples=samples, rate=RATE, pcm_stride=stride,
                                           peaks_stride=nb)
    run_limit = lambda: dec.pcm_limit_to(pcm.data_ptr(), peaks.data_ptr(), recs.data_ptr(), out.data_ptr(), n_streams=n, n_samples=samples,
                                         rate=RATE, n_peaks=nb, half_window=H, thresholds=thr, src_stride=stride, dst_stride=stride,
                                         peaks_stride=nb)
    run_gain = lambda: dec.pcm_gain_to(pcm.data_ptr(), recs.data_ptr(), out_gain.data_ptr(), n_streams=n, n_samples=samples,
                                       src_stride=stride, dst_stride=stride)
    with torch.cuda.stream(stream):
        dec.loudness_steps_to(pcm.data_ptr(), state.data_ptr(), steps.data_ptr(), n_streams=n, n_samples=samples, rate=RATE,
                              pcm_stride=stride, steps_stride=n_steps)
        dec.loudness_gate_to(steps.data_ptr(), state.data_ptr(), recs.data_ptr(), n_streams=n, n_steps=n_steps, rate=RATE, thresholds=thr,
                             steps_stride=n_steps)
        run_peaks()
        run_limit()
        run_gain()
    dec.sync()
    touched = []
    for i in (0, n - 1):
        x = pcm[i, :samples].cpu().numpy()
        rec = recs[i].cpu().numpy().view(L.REC_DTYPE)[0]
        assert rec == L.gate(L.step_records(x, RATE)[0], RATE, thr, L.state(x, RATE)[0]), f"stream {i}: the record differs from the model"
        G = M.stream_gain(int(rec["gated_mean"]), int(rec["n_gated"]), thr[1], L.step_of(RATE))
        assert efx.limit_gain(int(rec["gated_mean"]), int(rec["n_gated"]), thr[1], RATE) == G
        assert np.array_equal(peaks[i].cpu().numpy().view(np.uint16), M.peaks(x, RATE)), f"stream {i}: the peaks differ from the model"
        want, g = M.limit(x, RATE, G, thr[2], H, want_gains=True)
        assert np.array_equal(out[i, :samples].cpu().numpy(), want), f"stream {i}: the limited samples differ from the model"
        assert np.array_equal(out_gain[i, :samples].cpu().numpy(), L.apply_gain(x, int(rec["gain_q12"]))), f"stream {i}: the scaled samples differ"
        touched.append(round(float((g < G).mean()), 4))
        assert (G > int(rec["gain_q12"])) == (i == 0), "the first stream's cap binds, the last one's does not"

    calls = {"efx_limit_peaks": (run_peaks, n * (2 * samples + 2 * nb)), "efx_pcm_limit": (run_limit, n * (4 * samples + 2 * nb + 32)),
             "efx_pcm_gain": (run_gain, n * (4 * samples + 32))}
    events = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.reps):
            for name, (run, _) in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
                if r >= args.warmup:
                    events[name].append((e0, e1))
    stream.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in events.items()}
    gain_med = statistics.median(ms["efx_pcm_gain"])
    for name, (_, nbytes) in calls.items():
        med = statistics.median(ms[name])
        gbps = nbytes / med / 1e6
        print(json.dumps({"call": name, "rate": RATE, "streams": n, "seconds_per_stream": args.seconds, "half_window": H, "rounds": args.reps,
                          "ms": round(med, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                          "ms_per_1024_stream_seconds": round(med * 1024 / (n * args.seconds), 4), "bytes": nbytes, "gbps": round(gbps, 1),
                          "hbm_frac": round(gbps / HBM_PEAK_GBS, 4), "hbm_floor_ms": round(nbytes / HBM_PEAK_GBS / 1e6, 4),
                          "ratio_to_pcm_gain": round(med / gain_med, 3), "touched_first_last": touched,
                          "timing": "HIP events around every single call, the three calls alternated on the same buffers; median over the rounds"}),
              flush=True)
    dec.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--half-window", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds the timing process may take")
    ap.add_argument("--child", action="store_true", help="(the timing process's argument)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--streams", str(args.streams),
           "--seconds", str(args.seconds), "--half-window", str(args.half_window), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        sys.exit(f"exit status {r.returncode}")


if __name__ == "__main__":
    main()
