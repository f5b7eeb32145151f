"""The directed streams of tests/syntax_streams.py through the HIP decoder (espflix_amd.Decoder): every VLC code, f_code
1 ... 7 with and without full_pel, every window alignment and edge of k_recon's fetch, every scan position, matrix entry and
rounding class of the dequantiser, waves of full blocks -- against tests/golden/syntax.json (what the unmodified reference
decoded) and the oracle, bit-exact; vectors that leave the picture, saturated blocks at the extremes of the IDCT's range
and intra DC predictors far outside 0 ... 255 against the oracle alone.  What the streams cover is asserted on the CPU side,
tests/test_syntax_streams.py."""
import json
import os

import numpy as np
import pytest

import common
import oracle
import syntax_streams as ss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFINED = ("codes", "vectors", "windows", "coefs")


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def syntax_golden():
    with open(os.path.join(ROOT, "tests", "golden", "syntax.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def expected():
    """name -> (n, hashes) of the oracle on the elementary stream; computed once."""
    out = {}
    for s in ss.all_streams():
        n, h, _, _ = oracle.decode(s.array(), 0)
        out[s.name] = (n, [int(x) for x in h])
    return out


def decode(efx, streams, fmt, ring_depth=None, max_pictures=8):
    dec = efx.Decoder(max_streams=len(streams), max_pictures=max_pictures, ring_depth=ring_depth or max_pictures + 1,
                      max_stream_bytes=sum(len(s) for s in streams) + 4096)
    dec.upload(streams, fmt)
    dec.decode()
    return dec


def results(dec, n_streams):
    hashes = dec.frame_hashes()
    res = []
    for i in range(n_streams):
        n = dec.picture_count(i)
        res.append(dict(n=n, status=dec.stream_status(i), pts=[dec.picture_pts(i, p) for p in range(n)],
                        hashes=[int(hashes[i, dec.picture_slot(p, i)]) for p in range(n)]))
    return res


def first_difference(s, k, got, want):
    """Names the first macroblock, plane and block in which picture k of stream s differs, with the manifest's entry for the
    macroblock and the block's list of (scan position, level)."""
    g, w = ss.planes(got), ss.planes(want)
    for addr in range(ss.MBW * ss.MBH):
        for plane, (a, b) in enumerate(zip(ss.mb_pixels(g, addr), ss.mb_pixels(w, addr))):
            if not np.array_equal(a, b):
                m = s.pictures[k]["mbs"][addr] if s.pictures[k] else None
                text = f"{s.name} picture {k}: macroblock {addr} (column {addr % ss.MBW}, row {addr // ss.MBW}) plane {'Y Cr Cb'.split()[plane]} differs"
                if m:
                    d = a != b
                    blk = 4 + plane - 1 if plane else next(i for i in range(4) if d[8 * (i >> 1):8 * (i >> 1) + 8, 8 * (i & 1):8 * (i & 1) + 8].any())
                    coded = [i for i in range(6) if m["cbp"] & (0x20 >> i)]
                    entries = m["blocks"][coded.index(blk)] if blk in coded else "not coded"
                    y, x = (int(v[0]) for v in np.nonzero(d))
                    text += (f"; f_code {s.pictures[k]['f_code']} full_pel {s.pictures[k]['full_pel']}; manifest "
                             f"{ {key: v for key, v in m.items() if key != 'blocks'} }; block {blk} (scan position, level) {entries}; "
                             f"first differing pixel ({y}, {x}) of the plane's part: {int(a[y, x])}, expected {int(b[y, x])}")
                    if m["type"] != ss.T_SKIPPED and m["type"] & ss.T_FORWARD:
                        text += f"; windows (blk, px0, py0, hx, hy, pw, ph) {ss.block_windows(addr, m['mv'])}"
                return text
    return None


def test_defined_streams_in_one_batch_es(efx, syntax_golden, expected):
    """codes, vectors and windows side by side: neighbouring streams carry different r_size / full_pel into the same parse
    waves.  Against the reference's golden hashes and the oracle."""
    streams = ss.all_streams(DEFINED)
    dec = decode(efx, [s.array() for s in streams], efx.FORMAT_ES)
    res = results(dec, len(streams))
    dec.close()
    for s, r in zip(streams, res):
        assert r["status"] == 0 and r["n"] == len(s.pictures) == expected[s.name][0], (s.name, r["status"], r["n"])
        hexes = [f"{h:016x}" for h in r["hashes"]]
        bad = [k for k in range(r["n"]) if hexes[k] != syntax_golden[s.name]["hashes"][k]]
        assert not bad, f"{s.name}: pictures {bad} differ from the reference's golden"
        assert r["hashes"] == expected[s.name][1], s.name


def test_defined_streams_in_one_batch_ts(efx, syntax_golden):
    streams = ss.all_streams(DEFINED)
    dec = decode(efx, [np.frombuffer(common.one_pes_per_picture(s.es), dtype=np.uint8) for s in streams], efx.FORMAT_TS)
    res = results(dec, len(streams))
    dec.close()
    for s, r in zip(streams, res):
        g = syntax_golden[s.name]
        assert r["status"] == 0 and r["n"] == len(g["hashes"]), (s.name, r["status"], r["n"])
        assert [f"{h:016x}" for h in r["hashes"]] == g["hashes"] and r["pts"] == g["pts"], s.name


def test_interleaved_with_generator_streams_double_buffer(efx, expected):
    """The same batch interleaved with generator streams, ring_depth = 2 (the reference's two frame buffers): the last two
    pictures of every stream against the oracle."""
    from espflix_amd import gen
    directed = ss.all_streams(DEFINED)
    b = gen.Batch(0, len(directed), 8, 12, 0)
    streams, names = [], []
    for i, s in enumerate(directed):
        streams += [s.array(), b.es(i)]
        names += [s.name, None]
    dec = decode(efx, streams, efx.FORMAT_ES, ring_depth=2)
    hashes = dec.frame_hashes()
    for i, name in enumerate(names):
        if name:
            n, want = expected[name]
        else:
            n, h, _, _ = oracle.decode(streams[i], 0)
            want = [int(x) for x in h]
        assert dec.stream_status(i) == 0 and dec.picture_count(i) == n, (i, name)
        for p in (n - 2, n - 1):
            assert int(hashes[i, dec.picture_slot(p, i)]) == want[p], (i, name, p)
    dec.close()


def test_outside_equals_oracle(efx, expected):
    """Vectors that leave the picture (undefined in the reference; the oracle clamps the coordinates): one half-pel beyond,
    far beyond (f_code 7 with full_pel), beyond the corners, and waves of the clamped path that hold mostly inside windows.
    No status bit concerns vectors."""
    streams = ss.family("outside")
    dec = decode(efx, [s.array() for s in streams], efx.FORMAT_ES)
    res = results(dec, len(streams))
    dec.close()
    for s, r in zip(streams, res):
        assert r["status"] == 0 and r["n"] == expected[s.name][0], (s.name, r["status"], r["n"])
        bad = [k for k in range(r["n"]) if r["hashes"][k] != expected[s.name][1][k]]
        assert not bad, f"{s.name}: pictures {bad} differ from the oracle"


def test_range_equals_oracle(efx, expected):
    """Outside the reference's clamp table (the oracle clamps plainly to 0 ... 248): blocks whose 63 AC coefficients are all
    saturated, in the sign patterns that drive each multiplied operand of the IDCT and the residual to their extremes, and
    intra DC predictors walked to +-40 000 and back, in DC-only blocks (replicated unmasked) and in blocks that run the IDCT.
    What the streams hold is asserted in tests/test_syntax_streams.py."""
    streams = ss.family("range")
    dec = decode(efx, [s.array() for s in streams], efx.FORMAT_ES)
    res = results(dec, len(streams))
    dec.close()
    for s, r in zip(streams, res):
        assert r["status"] == 0 and r["n"] == expected[s.name][0], (s.name, r["status"], r["n"])
        bad = [k for k in range(r["n"]) if r["hashes"][k] != expected[s.name][1][k]]
        assert not bad, f"{s.name}: pictures {bad} differ from the oracle"


def test_whole_frames_name_the_macroblock(efx):
    """One stream per family, whole frames: a mismatch names the first differing macroblock and plane and the manifest's
    entry for it (vector, window alignment), so a failure points at a path rather than at a 64-bit number."""
    streams = [ss.family("codes")[-1], ss.family("vectors")[1], ss.family("windows")[1], ss.family("outside")[0],
               ss.family("coefs")[0], ss.family("range")[1]]
    dec = decode(efx, [s.array() for s in streams], efx.FORMAT_ES)
    for i, s in enumerate(streams):
        n, _, _, frames = oracle.decode(s.array(), 0, want_frames=True)
        assert dec.picture_count(i) == n
        for k in range(n):
            got = dec.download_frame(i, dec.picture_slot(k, i))
            if not np.array_equal(got, frames[k]):
                pytest.fail(first_difference(s, k, got, frames[k]) or f"{s.name} picture {k}: bytes outside the planes differ")
    dec.close()
