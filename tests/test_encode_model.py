"""The encoder's arithmetic (espflix_amd/csrc/enc_core.h) built for the host: what it writes decodes with the test oracle
to exactly the reconstruction it reports, on clip pictures and at the domain edges.  No GPU."""
import numpy as np
import pytest

import common
import encode_model as E
import export_model as M
import oracle


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return E.build(str(tmp_path_factory.mktemp("enc_model")))


@pytest.fixture(scope="module")
def splash_i420(clips):
    n, _, _, frames = oracle.decode(clips["splash"], 1, flush_last=True, want_frames=True)
    return M.strip_to_i420(frames[:n])


def round_trip(stream: bytes, fmt: int, recon, first_pts=0):
    n, hashes, pts, frames = oracle.decode(np.frombuffer(stream, dtype=np.uint8), fmt, flush_last=True, want_frames=True)
    assert n == len(recon), (n, len(recon))
    assert np.array_equal(frames, M.i420_to_strip(recon)), "the oracle's pictures differ from the encoder's reconstruction"
    if fmt == 1:
        assert list(pts) == [first_pts + 3003 * k for k in range(n)]


@pytest.mark.parametrize("fmt,qscale,search", [(0, 2, 7), (1, 8, 15), (1, 31, 7), (0, 8, 0)])
def test_clip_round_trip(enc, splash_i420, fmt, qscale, search):
    pics = splash_i420[:26]
    stream, recon = E.encode(enc, pics, gop=12, qscale=qscale, search=search, fmt=fmt, first_pts=129003)
    round_trip(stream, fmt, recon, 129003)
    assert E.luma_psnr(pics, recon) > {2: 38, 8: 30, 31: 22}[qscale]


@pytest.mark.parametrize("name", ["checker_q1", "noise", "flat0", "flat255"])
def test_domain_edges(enc, name):
    pics = {"checker_q1": E.checkerboard(3), "noise": common.random_frames(5).reshape(2, -1)[:, :E.PIC],
            "flat0": E.flat(3, 0), "flat255": E.flat(3, 255)}[name]
    for gop, search in ((12, 15), (1, 0), (2, 7)):
        stream, recon = E.encode(enc, pics, gop=gop, qscale=1 if name == "checker_q1" else 3, search=search, fmt=1)
        round_trip(stream, 1, recon)


def test_search_finds_motion(enc):
    pics = E.moving(8)
    with_search, rec7 = E.encode(enc, pics, gop=8, qscale=8, search=7, fmt=0)
    without, rec0 = E.encode(enc, pics, gop=8, qscale=8, search=0, fmt=0)
    round_trip(with_search, 0, rec7)
    round_trip(without, 0, rec0)
    assert 2 * len(with_search) <= len(without), (len(with_search), len(without))


def test_search_radius_bounds_the_vectors(enc):
    """search 0 codes the zero vector only (no half-pel step either); search R keeps |vector| within R full pels plus the
    half-pel step, and finds the motion of the moving source (half-pel positions included)."""
    pics = E.moving(8)
    for R in (0, 3, 7, 15):
        stream, recon = E.encode(enc, pics, gop=8, qscale=8, search=R, fmt=0)
        round_trip(stream, 0, recon)
        mbs = E.p_vectors(stream, 0)
        assert len(mbs) == 7 * 264
        vec = [(h, v) for _, _, intra, _, h, v in mbs if not intra]
        assert vec, R
        lim = 2 * R + 1 if R else 0
        assert all(abs(h) <= lim and abs(v) <= lim for h, v in vec), R
        if R >= 7:
            assert any(h & 1 or v & 1 for h, v in vec) and any(h or v for h, v in vec)
