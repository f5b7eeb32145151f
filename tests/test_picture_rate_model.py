"""The encoder's picture rates on the host: efx_picture_pts_offset and efx_picture_rate_code of the built library against
fractions.Fraction, and the host build of the encoder at a code (tests/enc_picture_rate_model_main.cpp) against the
existing host models at 30000/1001 Hz and against a rewrite of their streams for the other codes.  No GPU."""
from fractions import Fraction
from math import floor

import numpy as np
import pytest

import conform_model as C
import encode_model as E
import encode_rate_model as R
import picture_rate_model as P

KS = [0, 1, 2, 3, 4, 5, 1 << 32]


@pytest.fixture(scope="module")
def lib():
    import espflix_amd
    return espflix_amd.load_library()


def test_pts_offset_is_floor_of_k_periods(lib):
    for code, rate in C.RATES.items():
        for k in KS + [1001, 24000, (1 << 32) - 1]:
            assert lib.efx_picture_pts_offset(code, k) == floor(k * Fraction(90000) / rate), (code, k)
    assert [lib.efx_picture_pts_offset(1, k + 1) - lib.efx_picture_pts_offset(1, k) for k in range(8)] == [3753, 3754, 3754, 3754] * 2
    assert [lib.efx_picture_pts_offset(7, k + 1) - lib.efx_picture_pts_offset(7, k) for k in range(4)] == [1501, 1502] * 2
    for code, k in ((0, 1), (9, 1), (-1, 0), (4, -1), (4, (1 << 32) + 1)):
        assert lib.efx_picture_pts_offset(code, k) == -1, (code, k)


def test_rate_code_is_exact(lib):
    for code, rate in C.RATES.items():
        for m in (1, 2, 7, 1000):
            assert lib.efx_picture_rate_code(rate.numerator * m, rate.denominator * m) == code
    inexact = [(23976, 1000), (2997, 100), (5994, 100), (15, 1), (25, 2), (48, 1), (120, 1), (1000000, 41667), (24001, 1001),
               (24000, 1002), (0, 1), (24, 0), (-24, 1), (24, -1), (1 << 40, 1)]
    for num, den in inexact:
        assert lib.efx_picture_rate_code(num, den) == 0, (num, den)


def test_python_fps_forms():
    import espflix_amd as efx
    assert [efx.picture_rate_code(v) for v in (23.976, 29.97, 59.94, 24, "24000/1001", Fraction(50), 25.0, "60")] == [1, 4, 7, 2, 1, 6, 3, 8]
    assert [efx.picture_rate_code(v) for v in (15, 12.5, "1000000/41667", 23.98)] == [0] * 4
    assert efx.picture_pts_offset(24, 7) == 7 * 3750 and efx.picture_pts_offset("24000/1001", 3) == 11261
    for bad in (15, "12.5", 0, -24):
        with pytest.raises(ValueError):
            efx.picture_pts_offset(bad, 1)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("picture_rate_model"))
    return P.build(d), E.build(d), R.build(d)


def test_code_4_is_the_existing_models(exes):
    """At code 4 the new host build gives the bytes, reconstruction and quantisers of the existing host builds, which were
    compiled from the same headers with the default arguments."""
    pr, enc, rate = exes
    pics = E.moving(5)
    for fmt in (0, 1):
        want, rec = E.encode(enc, pics, gop=3, qscale=6, search=3, fmt=fmt, first_pts=777)
        got = P.encode(pr, pics, code=4, gop=3, qscale=6, search=3, fmt=fmt, first_pts=777)
        assert got.stream == want and np.array_equal(got.recon, rec)
        kw = dict(bitrate=300_000, vbv_bits=60_000, qmin=2, qmax=31, gop=3, qscale=6, search=3, fmt=fmt, first_pts=777)
        want = R.encode(rate, pics, **kw)
        got = P.encode(pr, pics, code=4, **kw)
        assert got.stream == want.stream and np.array_equal(got.qscales, want.qscales) and got.status == want.status


@pytest.mark.parametrize("code", range(1, 9))
def test_other_codes_change_headers_and_pts_only(exes, code):
    pr, enc, _ = exes
    pics = E.moving(5)
    es4, rec4 = E.encode(enc, pics, gop=3, qscale=6, search=3, fmt=0)
    got = P.encode(pr, pics, code=code, gop=3, qscale=6, search=3, fmt=0)
    assert got.stream == P.rewrite_es(es4, code) and np.array_equal(got.recon, rec4)
    assert P.sequence_codes(got.stream) == [code, code]
    first = (1 << 33) - 2 * 3753
    ts = P.encode(pr, pics, code=code, gop=3, qscale=6, search=3, fmt=1, first_pts=first)
    assert P.ts_pts(ts.stream) == [(first + C.pts_offset(code, k)) % (1 << 33) for k in range(5)]
    assert R.ts_payload(ts.stream)[14:14 + 12] == got.stream[:12]  # the first PES carries the sequence header


def test_time_code_counts_at_the_nominal_rate():
    assert P.time_code(0, 24) == 1 << 12
    assert P.time_code(24 * 3661 + 5, 24) == 1 << 19 | 1 << 13 | 1 << 12 | 1 << 6 | 5
    assert P.time_code(60 * 60, 60) == 1 << 13 | 1 << 12
