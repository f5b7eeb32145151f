#!/usr/bin/env python3
"""Throughput of k_import (efx_import_frames): pictures of any size cropped, scaled and converted to 352 x 192 I420.

Cases: 1920 x 1080 RGB24, 1920 x 1080 and 1280 x 720 I420 and 352 x 192 I420 (the copy case), and the surface legs
(efx_import_surfaces): 1920 x 1080 NV12 with a pitch of 2048 bytes and P010 with a pitch of 4096 bytes, 1088 plane rows
each -- every case at 64 and 1024 images.  Per launch: HIP events on the library's stream (a torch stream), algorithmic
bytes = the source samples read (pitch padding and unused plane rows do not count) + the 101 376-byte pictures written,
images/s, GB/s and the fraction of the 8 TB/s HBM spec bench.py uses.  Before timing, the first and the last image are
checked bit for bit against the NumPy model (tests/import_model.py, tests/surface_model.py).  Next to each case: what a user would otherwise
write with torch on the same device -- F.interpolate(..., mode="bilinear", antialias=True) on float planes plus the
BT.601 matrix as a matrix multiply and 4:2:0 chroma by a second interpolation; for a surface the strided plane views, the
de-interleave of the pair plane and the cast of the 16-bit samples in front of it -- timed the same way (it is not
bit-identical to the import, it does the same job).  --matrix CODE --src-range R: the YCbCr cases run with the colour
conversion (efx_import_set_colour: an H.273 matrix_coefficients code, "studio" or "full") and are checked against
tests/colour_model.py on top of the import's model; the RGB case and the torch comparison are then left out.  --hdr PEAK:
the YCbCr cases run as HDR10 sources (efx_import_set_hdr: PQ, BT.2020 primaries and matrix, the peak in nits; --src-range
applies) and are checked against tests/hdr_model.py.  --uhd adds 3840 x 2160 P010, the surface of HDR10 material.  Prints
one JSON line per case and implementation."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # (first: the process's HIP runtime is torch's, the library runs on a torch stream)
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import colour_model  # noqa: E402
import espflix_amd as efx  # noqa: E402
import hdr_model  # noqa: E402
import import_model  # noqa: E402
import surface_model  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (bench.py's figure)
# format or surface kind, width, height, pitch in bytes, plane rows (0, 0: a packed efx_pixel_format picture)
CASES = [("rgb24", 1920, 1080, 0, 0), ("i420", 1920, 1080, 0, 0), ("i420", 1280, 720, 0, 0), ("i420", 352, 192, 0, 0),
         ("nv12", 1920, 1080, 2048, 1088), ("p010", 1920, 1080, 4096, 1088)]
W, H = efx.FRAME_WIDTH, efx.FRAME_HEIGHT


def torch_import(src, fmt, w, h, matrix):
    """The same job in torch ops: (n, 101376) uint8."""
    n = src.shape[0]
    if fmt == "rgb24":
        rgb = src.view(n, h, w, 3).float()
        yuv = (rgb @ matrix[:, :3].T + matrix[:, 3]).permute(0, 3, 1, 2)
        y = F.interpolate(yuv[:, :1], size=(H, W), mode="bilinear", antialias=True)
        c = F.interpolate(yuv[:, 1:], size=(H // 2, W // 2), mode="bilinear", antialias=True)
    else:
        y = F.interpolate(src[:, :w * h].view(n, 1, h, w).float(), size=(H, W), mode="bilinear", antialias=True)
        c = F.interpolate(src[:, w * h:].view(n, 2, h // 2, w // 2).float(), size=(H // 2, W // 2), mode="bilinear", antialias=True)
    return torch.cat([y.reshape(n, -1), c.reshape(n, -1)], dim=1).round_().clamp_(0, 255).to(torch.uint8)


def torch_import_surface(src, s, w, h):
    """The same job for a semi-planar surface s (tests/surface_model.py) in torch ops: (n, 101376) uint8."""
    n = src.shape[0]
    if s.words:  # uint16 samples through int16 views: the value modulo 2^16, in 8-bit steps
        el, P = src.view(torch.int16), s.pitch[0] // 2
        cast = lambda t: torch.remainder(t.float(), 65536.0) / (1 << s.shift)
    else:
        el, P = src, s.pitch[0]
        cast = lambda t: t.float()
    o1 = s.offset[1] // (2 if s.words else 1)
    y = cast(el[:, :P * h].view(n, 1, h, P)[..., :w])
    uv = cast(el[:, o1:o1 + P * (h // 2)].view(n, h // 2, P)[..., :w].reshape(n, h // 2, w // 2, 2).permute(0, 3, 1, 2))
    y = F.interpolate(y, size=(H, W), mode="bilinear", antialias=True)
    c = F.interpolate(uv, size=(H // 2, W // 2), mode="bilinear", antialias=True)
    return torch.cat([y.reshape(n, -1), c.reshape(n, -1)], dim=1).round_().clamp_(0, 255).to(torch.uint8)


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
    ap.add_argument("--formats", nargs="+", default=None, help="only these cases: rgb24, i420, nv12, p010")
    ap.add_argument("--matrix", type=int, default=None, help="H.273 matrix_coefficients of the YCbCr sources (1 = BT.709 ...): convert to BT.601")
    ap.add_argument("--src-range", choices=["studio", "full"], default=None, help="range of the YCbCr sources")
    ap.add_argument("--hdr", type=int, nargs="?", const=1000, default=None, metavar="PEAK",
                    help="the YCbCr sources are HDR10 (PQ, BT.2020) of this peak in nits: tone-map to BT.601 SDR")
    ap.add_argument("--uhd", action="store_true", help="add the case 3840 x 2160 P010")
    args = ap.parse_args()
    if args.hdr is not None and args.matrix is not None:
        ap.error("--hdr runs with the BT.2020 matrix: leave --matrix out")
    colour = args.matrix is not None or args.src_range is not None or args.hdr is not None
    ckw = dict(matrix=args.matrix, src_range=args.src_range) if colour else {}
    hdr = None
    if args.hdr is not None:
        ckw = dict(transfer="pq", primaries="bt2020", peak_nits=args.hdr, src_range=args.src_range)
        t = efx.hdr_tables(args.hdr, src_range=args.src_range or "studio")
        hdr = hdr_model.Setting(args.hdr, int(args.src_range == "full"), 9, 9, pq=t["pq"], gam=t["gamma"])
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    dec = efx.Decoder(1, 1, device=torch.cuda.current_device(), hip_stream=stream.cuda_stream)
    matrix = torch.tensor([[66, 129, 25, 16 * 256], [-38, -74, 112, 128 * 256], [112, -94, -18, 128 * 256]],
                          dtype=torch.float32, device="cuda") / 256
    for fmt, w, h, pitch, rows in CASES + ([("p010", 3840, 2160, 7680, 2160)] if args.uhd else []):
        if (args.formats and fmt not in args.formats) or (colour and fmt == "rgb24"):
            continue
        surf = surface_model.layout(fmt, w, h, pitch, rows) if pitch else None
        image = surf.bytes if surf else efx.import_src_bytes(fmt, w, h)
        samples = w * h * 3 // 2 * (2 if surf.words else 1) if surf else image
        assert image % 16 == 0
        for n in args.images:
            gen = torch.Generator(device="cuda").manual_seed(n + w)
            src = torch.randint(0, 256, (n, image), dtype=torch.uint8, device="cuda", generator=gen)
            out = torch.empty((n, efx.FRAME_BYTES), dtype=torch.uint8, device="cuda")
            shaped = src.view(n, h, w, 3) if fmt == "rgb24" else src
            run = lambda: dec.import_pictures(shaped, fmt=fmt, width=w, height=h, pitch=pitch, plane_rows=rows, out=out, sync=False, **ckw)
            run()
            dec.sync()
            check = [0, n - 1]
            host = src[check].cpu().numpy()
            want = surface_model.import_images(host, surf) if surf else import_model.import_images(host, fmt, w, h)
            if hdr is not None:
                want = hdr_model.import_images(hdr, surface_model.canonicals(host, surf) if surf else host, w, h)
            elif colour:
                coefs = colour_model.coefs(6 if args.matrix is None else args.matrix, args.src_range == "full", h)
                want = colour_model.convert(want, None, *coefs) if coefs else want
            assert np.array_equal(out[check].cpu().numpy(), want), f"{fmt} {w}x{h}: output differs from the model"
            read, written = n * samples, n * efx.FRAME_BYTES
            base = {"format": fmt, "width": w, "height": h, "pitch": pitch, "plane_rows": rows, "images": n, "bytes_read": read,
                    "bytes_written": written, "matrix": args.matrix, "src_range": args.src_range, "hdr_peak_nits": args.hdr, "timing": "HIP events on the library's stream, mean over back-to-back calls"}
            ms = timed(stream, run, args.warmup, args.reps)
            gbps = (read + written) / ms / 1e6
            print(json.dumps({"impl": "k_import", **base, "ms": round(ms, 4), "images_per_s": round(n / ms * 1e3),
                              "gbps": round(gbps, 1), "hbm_frac": round(gbps / HBM_PEAK_GBS, 4)}), flush=True)
            if not args.no_torch and not colour:
                try:
                    # (chunks of 64 images: the float planes of 1024 full-HD pictures would not fit beside the source)
                    one = (lambda part: torch_import_surface(part, surf, w, h)) if surf else (lambda part: torch_import(part, fmt, w, h, matrix))
                    run_t = lambda: [one(src[i:i + 64]) for i in range(0, n, 64)]
                    got = run_t()[0][0].cpu().numpy().astype(int)
                    worst = int(np.abs(got - want[0].astype(int)).max())
                    ms_t = timed(stream, run_t, 1, max(1, args.reps // 3))
                    print(json.dumps({"impl": "torch interpolate(antialias)" + ("" if surf else " + matmul"), **base, "ms": round(ms_t, 4),
                                      "images_per_s": round(n / ms_t * 1e3), "worst_abs_difference_to_import": worst}), flush=True)
                except Exception as e:  # the comparison must not take the measurement down
                    print(json.dumps({"impl": "torch interpolate(antialias)" + ("" if surf else " + matmul"), **base, "error": repr(e)[:300]}), flush=True)
            del src, out
            torch.cuda.empty_cache()
    dec.close()


if __name__ == "__main__":
    main()
