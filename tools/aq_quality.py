"""What adaptive quantisation does to the golden clips, on the host model (no GPU): tests/enc_aq_model_main.cpp encodes
every picture of both clips at strength 0, 64, 128 and 256 -- at fixed qscale 8, and at the reference indexer's profile
(1.5 Mbit/s into 250 000 bits, qmin 3, scene cuts off) -- and tests/quality_model.py compares each reconstruction with
its source (ref_max 248).  Prints the table of profiles/adaptive_quant.md: bytes, luma PSNR, luma SSIM, and the summed
mb_sse of the macroblocks below the picture's average activity (a < avg, "smooth") and of the others ("textured")."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import encode_aq_model as A  # noqa: E402
import export_model as M  # noqa: E402
import oracle  # noqa: E402
import quality_model as Q  # noqa: E402

STRENGTHS = (0, 64, 128, 256)
MODES = (("q 8", dict(qscale=8)), ("1.5 Mbit/s", dict(bitrate=1_500_000, vbv_bits=250_000, qmin=3, qmax=31, qscale=8)))


def main():
    g = os.path.join(ROOT, "tests", "golden")
    with tempfile.TemporaryDirectory() as td:
        exe = A.build(td)
        print("| clip | mode | strength | bytes | luma PSNR dB | luma SSIM | SSE smooth | SSE textured | smooth MBs | mean q | mq range |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        for name in ("splash", "vmedia"):
            clip = np.fromfile(os.path.join(g, name + ".ts"), dtype=np.uint8)
            n, _, _, frames = oracle.decode(clip, 1, flush_last=True, want_frames=True)
            pics = M.strip_to_i420(frames[:n]).reshape(n, -1)
            act = np.stack([A.activities(p) for p in pics]).reshape(n, 264)
            smooth = act < ((act.sum(axis=1) + 132) // 264)[:, None]
            for mode, kw in MODES:
                for s in STRENGTHS:
                    r = A.encode(exe, pics, aq=s, fmt=1, **kw)
                    sse, ssim, mb = Q.compare_batch(pics, r.recon, ref_max=248)
                    psnr = Q.psnr(int(sse[:, 0].sum()), n * 352 * 192)   # of the clip's summed error: black pictures have none
                    ss = np.mean([Q.mean_ssim(int(v), 0) for v in ssim[:, 0]])
                    mb = mb.astype(np.int64)
                    print(f"| {name} ({n}) | {mode} | {s} | {len(r.stream)} | {psnr:.2f} | {ss:.4f} | {int(mb[smooth].sum())} | "
                          f"{int(mb[~smooth].sum())} | {int(smooth.sum())} of {smooth.size} | {r.qscales.mean():.2f} | "
                          f"{int(r.maps.min())} .. {int(r.maps.max())} |", flush=True)


if __name__ == "__main__":
    main()
