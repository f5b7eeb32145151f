#!/usr/bin/env python3
"""Throughput of k_export (efx_export_frames): decoded pictures of a batch of streams out as I420 / RGB24 / RGBP.

The ring is filled by decoding a synthetic batch (gen.Batch, 2 pictures per stream, ring_depth 2), then one picture of
every stream is exported in picture mode, back to back.  Per launch: HIP events on the library's stream (a torch stream),
algorithmic bytes = the frames read (101 376 B per stream) + the images written, GB/s and the fraction of the 8 TB/s HBM
spec bench.py uses.  At the default 4096 streams the frames alone are 415 MB, past the 256 MiB Infinity Cache.  Before
timing, the output of two streams is checked against the NumPy model (tests/export_model.py).
Prints one JSON line per format x chroma mode."""
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
import export_model  # noqa: E402
from espflix_amd import gen  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (bench.py's figure)
CASES = [("i420", "nearest"), ("rgb24", "nearest"), ("rgb24", "bilinear"), ("rgbp", "nearest"), ("rgbp", "bilinear")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full-range", action="store_true")
    args = ap.parse_args()
    S = args.streams
    stream = torch.cuda.Stream()
    dec = efx.Decoder(S, 2, 2, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    b = gen.Batch(0, S, 2, 12, 0, threads=16)
    dec.upload(b.all_es(), efx.FORMAT_ES)
    b.close()
    dec.decode()
    picture = 1
    out = torch.empty(S * efx.export_bytes("rgb24"), dtype=torch.uint8, device="cuda")
    check = [0, S - 1]
    frames = np.stack([dec.download_frame(s, dec.picture_slot(picture, s)) for s in check])
    for fmt, chroma in CASES:
        image = efx.export_bytes(fmt)
        dst = out[:S * image]
        run = lambda: dec.export(fmt, picture=picture, chroma=chroma, full_range=args.full_range, out=dst, sync=False)
        run()
        dec.sync()
        got = dst.view(S, image)[check].cpu().numpy()
        want = export_model.export(frames, fmt, chroma, args.full_range).reshape(len(check), image)
        assert np.array_equal(got, want), f"{fmt} {chroma}: output differs from the model"
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
        read, written = S * efx.FRAME_BYTES, S * image
        gbps = (read + written) / ms / 1e6
        print(json.dumps({"kernel": "k_export", "format": fmt, "chroma": chroma if fmt != "i420" else None,
                          "full_range": args.full_range, "streams": S, "ms": round(ms, 4), "bytes_read": read,
                          "bytes_written": written, "gbps": round(gbps, 1), "hbm_frac": round(gbps / HBM_PEAK_GBS, 3),
                          "timing": "HIP events on the library's stream, mean over back-to-back launches"}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
