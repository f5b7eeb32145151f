#!/usr/bin/env python3
"""Throughput of k_conform (efx_conform_rate): pictures at one constant rate conformed to a rate MPEG-1 codes.

Cases: 1024 streams x 24 source pictures, 25 -> 24 Hz (23 outputs: one picture dropped) and 50 -> 25 Hz (12 outputs: every
second picture).  Each case is first checked bit for bit against the torch formulation src[:, idx], idx from
efx_conform_source.  Then per call -- 20 back to back after 3 of warm-up, HIP events on the library's stream (a torch
stream): ms, GB/s over the algorithmic bytes (every output picture read once and written once) and the fraction of the
6.3 TB/s an element-wise kernel reaches on this part.  Next to each case, timed the same way in the same process, k_trick
(efx_trick_pick, fwd only) moving the same number of bytes with the same access pattern: speed 1 over 23 pictures, speed 2
over 24.  The two kernels alternate, `--rounds` times.  Prints one JSON line per case, implementation and round."""
import argparse
import json
import os
import sys
from fractions import Fraction

import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import espflix_amd as efx  # noqa: E402

ELEMENTWISE_GBS = 6300.0  # the element-wise ceiling of the part (about 6.3 TB/s), the yardstick of elementwise_frac
PIC = efx.FRAME_BYTES
CASES = [("25 -> 24", Fraction(25), Fraction(24), 1), ("50 -> 25", Fraction(50), Fraction(25), 2)]  # (..., k_trick's speed)


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


def bench(dec, stream, n, P, what, fps_in, fps_out, speed, args):
    lib = efx.load_library()
    code = efx.picture_rate_code(fps_out)
    K = efx.conform_count(fps_in, fps_out, 0, P)
    idx = [int(lib.efx_conform_source(fps_in.numerator, fps_in.denominator, code, k)) for k in range(K)]
    trick_P = K * speed if speed > 1 else K
    assert efx.trick_count(0, trick_P, speed) == K and trick_P <= P
    src = torch.randint(0, 256, (n, P, PIC), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((n, K, PIC), dtype=torch.uint8, device="cuda")
    fwd = torch.zeros((n, K, PIC), dtype=torch.uint8, device="cuda")
    run = lambda: dec.conform_to(src.data_ptr(), dst.data_ptr(), n_streams=n, n_pictures=P, fps_in=fps_in, fps_out=fps_out)
    trick = lambda: dec.trick_pick_to(src.data_ptr(), fwd.data_ptr(), None, n_streams=n, n_pictures=trick_P, speed=speed,
                                      src_stride=P * PIC)
    stream.synchronize()
    run()
    trick()
    dec.sync()
    assert torch.equal(dst, src[:, idx]), "k_conform differs from the torch formulation"
    assert torch.equal(fwd, src[:, :trick_P:speed])
    moved = 2 * n * K * PIC
    base = {"case": what, "streams": n, "pictures": P, "outputs": K, "bytes_moved": moved,
            "timing": "HIP events on the library's stream, mean over back-to-back calls"}
    for rnd in range(args.rounds):
        for impl, fn in (("k_conform", run), (f"k_trick speed {speed}, fwd only", trick)):
            ms = timed(stream, fn, args.warmup, args.reps)
            gbps = moved / ms / 1e6
            print(json.dumps({"impl": impl, "round": rnd, **base, "ms": round(ms, 4), "gbps": round(gbps, 1),
                              "elementwise_frac": round(gbps / ELEMENTWISE_GBS, 4)}), flush=True)
    del src, dst, fwd
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--pictures", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    for what, fps_in, fps_out, speed in CASES:
        bench(dec, stream, args.streams, args.pictures, what, fps_in, fps_out, speed, args)
    dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
