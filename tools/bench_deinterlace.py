#!/usr/bin/env python3
"""Throughput of k_deint (efx_deinterlace): interlaced frames to progressive pictures at the source's size.

Cases: 1920 x 1080 NV12, 720 x 576 and 720 x 480 I420, each at the frame rate (one picture per frame) and at the field
rate (two), as one stream of 8 and of 64 frames.  The frames are noise made on the device with torch.  Each case is first
checked byte for byte against the NumPy model (tests/deint_model.py: the first and the last picture of the call).  Then,
after warm-up calls, HIP events on the library's stream (a torch stream) around every single call: best and mean ms,
frames/s, and GB/s over the bytes the kernel moves -- per frame it reads the frame and its two neighbours (at the frame
rate only the half of the next frame that the missing lines use) and writes one or two pictures: 5 images at the field
rate, 3.5 at the frame rate, the fetches of the halo lanes and of the two rows above and below a band not counted.
Next to it the yardstick: a plain device-to-device copy (torch's copy_) that moves the same number of bytes, half of them
read and half written, timed the same way in the same run.  Prints one JSON line."""
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
import deint_model  # noqa: E402
import surface_model  # noqa: E402

CASES = [("nv12", 1920, 1080), ("i420", 720, 576), ("i420", 720, 480)]


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
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    out = {"timing": "HIP events on the library's stream around each call", "first_field": "top"}
    for kind, w, h in CASES:
        surf, model = efx.surface_layout(kind, w, h), surface_model.layout(kind, w, h)
        image = w * h * 3 // 2
        assert surf.bytes == image and image % 16 == 0
        for n in args.frames:
            gen = torch.Generator(device="cuda").manual_seed(w + n)
            src = torch.randint(0, 256, (n, image), dtype=torch.uint8, device="cuda", generator=gen)
            dst = torch.empty((2 * n, image), dtype=torch.uint8, device="cuda")
            for rate, per_frame, images_moved in (("frame", 1, 3.5), ("field", 2, 5.0)):
                run = lambda: dec.deinterlace_to(src.data_ptr(), dst.data_ptr(), surface=surf, n_frames=n, rate=rate)
                stream.synchronize()
                n_out = run()
                dec.sync()
                assert n_out == per_frame * n
                first, last = src[:2].cpu().numpy(), src[n - 2:].cpu().numpy()
                mode = deint_model.FIELD if rate == "field" else deint_model.FRAME
                assert np.array_equal(dst[0].cpu().numpy(), deint_model.deinterlace(first, model, 1, mode=mode, tail=1)[0, 0]), "differs from the model"
                assert np.array_equal(dst[n_out - 1].cpu().numpy(), deint_model.deinterlace(last, model, 1, mode=mode, lead=1)[0, -1]), "differs from the model"
                ms = timed_calls(stream, run, args.warmup, args.reps)
                moved = int(images_moved * image * n)
                a, b = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
                cms = timed_calls(stream, lambda: b.copy_(a), args.warmup, args.reps)
                del a, b
                best, cbest = min(ms), min(cms)
                out[f"{kind}_{w}x{h}_{n}_frames_{rate}_rate"] = {
                    "pictures_out": n_out, "bytes_moved": moved, "ms_best": round(best, 4), "ms_mean": round(float(np.mean(ms)), 4),
                    "frames_per_s": round(n / best * 1e3), "gbps": round(moved / best / 1e6, 1),
                    "copy_of_the_same_bytes": {"ms_best": round(cbest, 4), "ms_mean": round(float(np.mean(cms)), 4), "gbps": round(moved / cbest / 1e6, 1)},
                    "kernel_over_copy": round(best / cbest, 2)}
            del src, dst
            torch.cuda.empty_cache()
    print(json.dumps(out))
    dec.close()


if __name__ == "__main__":
    main()
