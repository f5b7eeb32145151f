"""Regenerates tests/golden/index_edges.json from the UNMODIFIED reference indexer (oracle/_ref, `make ref`): for every
directed stream of common.index_edge_streams() that the indexer accepts, the FNV-1a-64 of the video.idx it writes (tail
padding of the three records masked) for the title (stream, small, small) with small = common.index_small_ts().  Streams
with two consecutive sequence starts less than 90 ticks apart are left out: indexer.cpp:136 divides by their distance in
milliseconds (common.INDEX_EDGE_NOT_FOR_REFERENCE)."""
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

assert oracle.have_ref(), "build oracle/_ref first (make ref)"
small = np.frombuffer(common.index_small_ts(), dtype=np.uint8)
out = {}
for name, ts in common.index_edge_streams():
    if name in common.INDEX_EDGE_NOT_FOR_REFERENCE:
        continue
    idx = oracle.ref_make_idx([np.frombuffer(ts, dtype=np.uint8), small, small])
    out[name] = f"{oracle.fnv1a64(oracle.idx_masked(idx)):016x}"

with open(os.path.join(HERE, "index_edges.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote index_edges.json:", len(out), "streams")
