#!/usr/bin/env python3
"""Throughput of k_denoise (efx_denoise), and what the step is worth to the encoder.

Throughput.  NV12 sources of 720 x 480 at 1, 8 and 64 streams and of 1920 x 1080 at 1 and 8 streams, 30 frames each: a
moving texture with Gaussian noise of sigma = 6 made on the device from a seed, filtered at denoise_thresholds(6).  The
720 x 480 calls are first checked byte for byte against the NumPy model (tests/denoise_model.py) on their first stream.
Then, after warm-up calls, HIP events on the library's stream (a torch stream) around every single call -- the call is
one launch: best and mean ms, frames/s, and the bytes it must move at the least (every source byte in once, every output
byte out once).  Next to it the yardstick, timed the same way in the same run: a plain device-to-device copy (torch's
copy_) that moves the same bytes.

Encoder.  With --encoder: the noisy moving scene of tests/test_denoise_model.py, 16 frames enlarged to 704 x 384 I420 with
noise of sigma = 6 on all three planes, imported to 352 x 192 and encoded at a fixed quantiser, with and without
efx_denoise in front of the import: the stream's bytes, and the PSNR of the decoder's reconstruction against the imported
CLEAN scene (efx_compare_pictures).

Prints one JSON line."""
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
import denoise_model  # noqa: E402
import surface_model  # noqa: E402
import test_denoise_model  # noqa: E402

KIND, SIGMA = "nv12", 6
CASES = [(720, 480, 1), (720, 480, 8), (720, 480, 64), (1920, 1080, 1), (1920, 1080, 8)]
NAMES = ("luma_spatial", "chroma_spatial", "luma_temporal", "chroma_temporal")


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


def noisy_frames(w, h, n_streams, n, seed):
    """(n_streams * n, w * h * 3 / 2) NV12 frames on the device: a texture that moves 3 samples a frame, another phase per
    stream, with noise of sigma = 6 on luma and chroma."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    out = torch.empty((n_streams * n, w * h * 3 // 2), dtype=torch.uint8, device="cuda")
    for i in range(n_streams):
        for t in range(n):
            xs = x - 3 * t - 17 * i
            luma = 128 + 50 * torch.sin(2 * np.pi * xs / 41) + 30 * torch.cos(2 * np.pi * (xs + 2 * y) / 67) + 70 * (((xs // 96) + (y // 64)) % 2)
            pair = 128 + 40 * torch.sin(2 * np.pi * (xs[::2] + y[::2]) / 53)  # (h / 2, w): Cb, Cr interleaved
            img = torch.cat([luma.reshape(-1), pair.reshape(-1)])
            img = img + SIGMA * torch.randn(img.shape, device="cuda", generator=g)
            out[i * n + t] = img.round().clamp(0, 255).to(torch.uint8)
    return out


def throughput(dec, stream, w, h, n_streams, n, args):
    surf, model = efx.surface_layout(KIND, w, h), surface_model.layout(KIND, w, h)
    image = w * h * 3 // 2
    assert surf.bytes == image and image % 16 == 0
    thr = dict(zip(NAMES, efx.denoise_thresholds(SIGMA)))
    src = noisy_frames(w, h, n_streams, n, 1000 + w + n_streams)
    dst = torch.empty_like(src)
    run = lambda: dec.denoise_to(src.data_ptr(), dst.data_ptr(), surface=surf, n_streams=n_streams, n_frames=n, **thr)
    stream.synchronize()
    run()
    dec.sync()
    if w <= 720:
        k = min(n, 6)  # (the recursion from the stream's start: the first frames of the first stream)
        want = denoise_model.denoise(src[:k].cpu().numpy(), model, 1, **thr)
        assert np.array_equal(dst[:k].cpu().numpy(), want), "differs from the model"
    ms = timed_calls(stream, run, args.warmup, args.reps)
    frames = n_streams * n
    moved = 2 * image * frames
    a, c = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    cms = timed_calls(stream, lambda: c.copy_(a), args.warmup, args.reps)
    del a, c, src, dst
    return {"case": f"{KIND} {w}x{h}, {n_streams} streams x {n} frames", "ms_best": round(min(ms), 4), "ms_mean": round(float(np.mean(ms)), 4),
            "frames_per_s": round(frames / min(ms) * 1e3), "bytes_moved_at_least": moved, "gbps": round(moved / min(ms) / 1e6, 1),
            "copy_of_those_bytes": {"ms_best": round(min(cms), 4), "ms_mean": round(float(np.mean(cms)), 4), "gbps": round(moved / min(cms) / 1e6, 1)},
            "call_over_copy": round(min(ms) / min(cms), 2)}


def encoder_benefit(dec, qscale):
    """The test scene, enlarged 11 x 8 to 704 x 384 with flat chroma, clean and with sigma = 6 noise on all planes."""
    T = test_denoise_model
    w, h = 11 * T.W, 8 * T.H
    clean_y = np.kron(T.scene(), np.ones((1, 8, 11), dtype=np.int64))
    clean = np.concatenate([clean_y.reshape(T.N, -1), np.full((T.N, w * h // 2), 128, dtype=np.int64)], axis=1)
    noise = np.rint(np.random.default_rng(1).normal(0, SIGMA, clean.shape)).astype(np.int64)
    noisy = np.clip(clean + noise, 0, 255).astype(np.uint8)
    thr = dict(zip(NAMES, efx.denoise_thresholds(SIGMA)))
    ref = dec.import_pictures(clean.astype(np.uint8), fmt="i420", width=w, height=h)
    out = {"source": f"{T.N} frames of {w} x {h} I420, sigma = {SIGMA}, imported to 352 x 192; qscale {qscale}, gop 12", "thresholds": thr}
    for name, pics in (("without", noisy), ("with_denoise", dec.denoise(noisy, fmt="i420", width=w, height=h, **thr))):
        small = dec.import_pictures(pics, fmt="i420", width=w, height=h)
        enc = dec.encode(small[None], qscale=qscale, gop=12, recon=True)
        assert int(enc.status[0]) == 0
        q = dec.compare(ref[None], np.asarray(enc.recon), ref_max=248)
        src_q = dec.compare(ref, small)
        out[name] = {"stream_bytes": len(enc.streams[0]), "psnr_y_recon_vs_clean": round(float(q.psnr[0, :, 0].mean()), 2),
                     "psnr_y_encoder_input_vs_clean": round(float(src_q.psnr[:, 0].mean()), 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--encoder", action="store_true", help="also measure the encoder's bytes and PSNR with and without the step")
    ap.add_argument("--qscale", type=int, default=8)
    ap.add_argument("--no-throughput", action="store_true", help="leave the timed cases out")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 16, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    out = {"timing": "HIP events on the library's stream around each call (one launch); the copy timed the same way in the same process",
           "cases": [] if args.no_throughput else [throughput(dec, stream, w, h, k, args.frames, args) for w, h, k in CASES]}
    if args.encoder:
        out["encoder"] = encoder_benefit(dec, args.qscale)
    dec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
