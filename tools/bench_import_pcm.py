#!/usr/bin/env python3
"""Throughput of k_import_pcm (efx_import_pcm): PCM downmixed to mono and resampled to 48 kHz on the device.

Cases: 1 s of 44.1 kHz stereo and 1 s of 96 kHz mono per stream, at 64 and 1024 streams, one call each.  Per call (both
launches): HIP events on the library's stream (a torch stream), stream-seconds per second, algorithmic bytes = the source
elements read + the samples written + the 256-byte states read and written, GB/s and the fraction of the 8 TB/s HBM spec
bench.py uses.  Before timing, the first and the last stream are checked against the NumPy model
(tests/import_pcm_model.py).  Next to each case, unless --no-host: the same arithmetic (csrc/import_pcm.h with the
kernel's addressing, tests/import_pcm_model_main.cpp built with g++ -O2) on one core of the host.  Prints one JSON line
per case and implementation."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import espflix_amd as efx  # noqa: E402
import import_pcm_model as M  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (bench.py's figure)
CASES = [(44100, 48000, 2), (96000, 48000, 1)]
SECONDS = 1


def host_seconds(tmp, r, o, ch, n_in, reps):
    """Seconds per call of one stream on one core, or None without a compiler."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        return None
    exe, table = os.path.join(tmp, "drv"), os.path.join(tmp, "table.bin")
    if not os.path.exists(exe):
        subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "espflix_amd", "csrc"),
                        os.path.join(ROOT, "tests", "import_pcm_model_main.cpp"), "-o", exe], check=True)
        efx.import_pcm_filter().tofile(table)
    out = subprocess.run([exe, "time", table, str(r), str(o), str(ch), str(n_in), str(reps)], capture_output=True, text=True,
                         check=True)
    return float(out.stdout.split()[0]) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host build on one core")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(max(args.streams), 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    with tempfile.TemporaryDirectory() as tmp:
        for r, o, ch in CASES:
            n_in = SECONDS * r
            n_out = efx.import_pcm_out_samples(r, o, 0, n_in)
            ss, ds = (n_in * ch + 7) // 8 * 8, (n_out + 7) // 8 * 8
            for n in args.streams:
                gen = torch.Generator(device="cuda").manual_seed(n + r)
                src = torch.randint(-32768, 32768, (n, ss), dtype=torch.int32, device="cuda", generator=gen).to(torch.int16)
                state = torch.zeros((n, efx.import_pcm_state_bytes()), dtype=torch.uint8, device="cuda")
                out = torch.zeros((n, ds), dtype=torch.int16, device="cuda")
                stream.synchronize()
                run = lambda: dec.import_pcm_to(src.data_ptr(), state.data_ptr(), out.data_ptr(), n_streams=n, n_in=n_in, in_rate=r,
                                                out_rate=o, channels=ch, src_stride=ss, dst_stride=ds)
                run()
                dec.sync()
                check = [0, n - 1]
                want, _ = M.import_pcm(src[check, :n_in * ch].cpu().numpy(), r, o, ch)
                assert np.array_equal(out[check, :n_out].cpu().numpy(), want), f"{r} -> {o}: output differs from the model"
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
                nbytes = n * (2 * n_in * ch + 2 * n_out + 2 * efx.import_pcm_state_bytes())
                gbps = nbytes / ms / 1e6
                base = {"in_rate": r, "out_rate": o, "channels": ch, "streams": n, "seconds_per_stream": SECONDS, "bytes": nbytes}
                print(json.dumps({"impl": "k_import_pcm", **base, "ms": round(ms, 4),
                                  "stream_seconds_per_s": round(n * SECONDS / ms * 1e3), "gbps": round(gbps, 1),
                                  "hbm_frac": round(gbps / HBM_PEAK_GBS, 4), "hbm_floor_ms": round(nbytes / HBM_PEAK_GBS / 1e6, 4),
                                  "timing": "HIP events on the library's stream, mean over back-to-back calls"}), flush=True)
                del src, out, state
                torch.cuda.empty_cache()
            if not args.no_host:
                s = host_seconds(tmp, r, o, ch, n_in, 5)
                if s is not None:
                    print(json.dumps({"impl": "import_pcm.h, g++ -O2, one core", "in_rate": r, "out_rate": o, "channels": ch,
                                      "streams": 1, "seconds_per_stream": SECONDS, "ms": round(s * 1e3, 3),
                                      "stream_seconds_per_s": round(SECONDS / s, 1)}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
