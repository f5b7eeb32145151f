"""Regenerates tests/golden/sbc_directed.json from the UNMODIFIED reference (oracle/_ref/efx_ref_sbc, `make ref`): for every
directed call of tests/sbc_streams.py the FNV of the PCM the reference decoder makes of its streams (each from a fresh
sbc_init(): one run of the harness per stream; all of them back to back) and of its return values and decoded byte counts.
One entry per call, not per stream; some 40 000 short runs, a few minutes.  tests/golden/golden.json is made by
make_golden.py and is not touched."""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle
import sbc_streams

assert oracle.have_ref_sbc(), "build oracle/_ref first (make ref)"
out = {}
with ThreadPoolExecutor(8) as pool:
    for key in sbc_streams.call_names():
        call = sbc_streams.make_call(key)
        done = list(pool.map(lambda s: oracle.ref_sbc_decode(s.data, call.fb), call.streams))
        out[call.name] = oracle.sbc_call_hashes([d[0] for d in done], np.array([d[1] for d in done], dtype=np.int32))

with open(os.path.join(HERE, "sbc_directed.json"), "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote sbc_directed.json:", len(out), "calls")
