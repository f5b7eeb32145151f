"""Regenerates tests/golden/syntax.json from the UNMODIFIED reference (oracle/_ref, `make ref`): per-picture frame hashes and
PTS of the directed streams of tests/syntax_streams.py whose decoding the reference defines (families codes, vectors,
windows, coefs), each wrapped into a transport stream with one PES per picture, and the FNV of the elementary stream the hashes
belong to -- the layout of golden.json["handmade"].  tests/golden/golden.json is made by make_golden.py and is not touched."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import common
import oracle
import syntax_streams

assert oracle.have_ref(), "build oracle/_ref first (make ref)"
out = {}
for s in syntax_streams.all_streams(("codes", "vectors", "windows", "coefs")):
    h, pts, _ = oracle.ref_decode(np.frombuffer(common.one_pes_per_picture(s.es), dtype=np.uint8), flush_last=True)
    assert len(h) == len(s.pictures), s.name
    out[s.name] = {"hashes": [f"{int(x):016x}" for x in h], "pts": [int(x) for x in pts], "es_fnv": f"{common.fnv_bytes(s.array()):016x}"}

with open(os.path.join(HERE, "syntax.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote syntax.json:", len(out), "streams")
