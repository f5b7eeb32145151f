#!/usr/bin/env python3
"""Generates tests/golden/encode_psnr.json: the float64 yardstick encoder's (tests/encode_float.py) mean luma PSNR of the I
pictures and of the P pictures for every case of the encoder's quality checks (tests/test_encode_yardstick.py,
tests/test_gpu_encode.py), the same at the neighbouring qscale (q + 1, or 30 for 31), and the margin: a quarter of the
absolute difference of the two, per case and per picture type.  Nothing of the encoder under test enters.

    python tests/golden/make_encode_psnr.py
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import encode_float as F  # noqa: E402
import encode_model as E  # noqa: E402
import export_model as M  # noqa: E402
import oracle  # noqa: E402


def sources():
    clip = {}
    for name in ("splash", "vmedia"):
        ts = np.fromfile(os.path.join(HERE, name + ".ts"), dtype=np.uint8)
        n, _, _, frames = oracle.decode(ts, 1, flush_last=True, want_frames=True)
        clip[name] = M.strip_to_i420(frames[:n])
    return E.quality_sources(clip)


def yardstick(job):
    name, q = job
    pics = sources()[name]
    return name, q, F.psnr_by_type(pics, F.encode(pics, E.QUALITY_GOP, q, E.QUALITY_SEARCH), E.QUALITY_GOP)


def main():
    qs = sorted(set(E.QUALITY_Q) | {E.neighbour_q(q) for q in E.QUALITY_Q})
    jobs = [(name, q) for name in ("splash", "vmedia", "moving") for q in qs]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        psnr = {(name, q): p for name, q, p in pool.map(yardstick, jobs)}
    cases = {}
    for name in ("splash", "vmedia", "moving"):
        for q in E.QUALITY_Q:
            nq = E.neighbour_q(q)
            rec = {"neighbour": nq}
            for k, t in enumerate("IP"):
                rec[t] = round(psnr[name, q][k], 4)
                rec[t + "_neighbour"] = round(psnr[name, nq][k], 4)
                rec[t + "_margin"] = round(abs(rec[t] - rec[t + "_neighbour"]) / 4, 4)
            cases[f"{name}_q{q}"] = rec
            print(f"{name}_q{q}", rec)
    with open(E.PSNR_JSON, "w") as f:
        json.dump({"gop": E.QUALITY_GOP, "search": E.QUALITY_SEARCH, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
