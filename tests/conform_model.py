"""NumPy / fractions model of efx_conform_rate as include/efx.h defines it: which source picture every output picture
shows when a constant picture rate is conformed to one of the eight rates MPEG-1 codes, and the outputs a call holds."""
from fractions import Fraction
from math import floor

import numpy as np

RATES = {1: Fraction(24000, 1001), 2: Fraction(24), 3: Fraction(25), 4: Fraction(30000, 1001), 5: Fraction(30), 6: Fraction(50),
         7: Fraction(60000, 1001), 8: Fraction(60)}
NOMINAL = {1: 24, 2: 24, 3: 25, 4: 30, 5: 30, 6: 50, 7: 60, 8: 60}
# the source rates of the tests: what MPEG-1 cannot code, a container rate, and the eight coded rates
SOURCES = [Fraction(15), Fraction(25, 2), Fraction(48), Fraction(120), Fraction(1000000, 41667)] + [RATES[c] for c in range(1, 9)]
MAX_INDEX = (1 << 31) - 1


def pts_offset(code: int, k: int) -> int:
    """90 kHz ticks from picture 0 to picture k at the code's rate: floor(k x 90000 / rate)."""
    return floor(k * 90000 / RATES[code])


def ratio(r: Fraction, code: int):
    """A : B = in_num x out_den : 2 x out_num x in_den, reduced."""
    f = Fraction(r) / (2 * RATES[code])
    return f.numerator, f.denominator


def accepted(r: Fraction, code: int) -> bool:
    r = Fraction(r)
    if not 1 <= code <= 8 or r <= 0:
        return False
    A, B = ratio(r, code)
    return A < 1 << 31 and B < 1 << 31 and r <= 64 * RATES[code] and RATES[code] <= 64 * r


def slot(i: int, r: Fraction, code: int) -> int:
    """The output slot of source picture i, shown at time i / r."""
    return floor(i * RATES[code] / Fraction(r) + Fraction(1, 2))


def source(n: int, r: Fraction, code: int) -> int:
    A, B = ratio(r, code)
    return ((2 * n + 1) * A - 1) // B


def outputs(N: int, r: Fraction, code: int) -> int:
    """Outputs the stream holds after its first N source pictures."""
    A, B = ratio(r, code)
    return max(0, -(-(N * B + 1 - A) // (2 * A)))


def count(first: int, n: int, r: Fraction, code: int) -> int:
    if not accepted(r, code) or first < 0 or n < 0 or first + n > MAX_INDEX or outputs(first + n, r, code) - 1 > MAX_INDEX:
        return -1
    return outputs(first + n, r, code) - outputs(first, r, code)


def brute_sources(N: int, r: Fraction, code: int):
    """By the slot rule alone: the source of every output whose source is among the first N source pictures."""
    slots = [slot(i, r, code) for i in range(N + 1)]  # (one more: the picture that ends the last one's slots)
    out, n = [], 0
    while True:
        last = max(i for i in range(N + 1) if slots[i] <= n) if slots[0] <= n else None
        if last is None or last >= N:
            # (slot(0) = 0, so every output has a source; an output whose last source is picture N or later is not held)
            return out
        out.append(last)
        n += 1


def conform(pictures: np.ndarray, first: int, r: Fraction, code: int) -> np.ndarray:
    """One call: pictures (streams, n, bytes) are the title's pictures first .. first + n - 1; returns (streams, outputs,
    bytes), output outputs(first) + m at image m."""
    n = pictures.shape[1]
    n0, n1 = outputs(first, r, code), outputs(first + n, r, code)
    idx = [source(k, r, code) - first for k in range(n0, n1)]
    assert all(0 <= j < n for j in idx)
    return pictures[:, idx] if idx else pictures[:, :0]
