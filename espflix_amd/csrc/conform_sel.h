// conform_sel.h -- the rule of efx_conform_rate (k_conform.hip): which source picture every output picture shows when a
// stream of pictures at one constant rate is conformed to one of the eight rates MPEG-1 codes, and the outputs a call holds.
//
// Host + device: the kernel and the host entry points run exactly these functions, and tests/test_conform_model.py builds
// this header with a plain C++ compiler (tests/conform_model_main.cpp) and checks it against the NumPy model
// (tests/conform_model.py).  Plain integer functions, no HIP (the definition: include/efx.h).
//
// Source picture i, shown at time i / r, belongs to output slot floor(i o / r + 1/2) (r, o: source and output rate); output n
// shows the last source picture whose slot is <= n.  With A : B = in_num x out_den : 2 x out_num x in_den, reduced:
//   src(n)  = floor(((2 n + 1) A - 1) / B)
//   Nout(N) = max(0, ceil((N B + 1 - A) / (2 A)))      outputs whose source is among the first N source pictures
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EFX_CSEL_HD __host__ __device__
#else
#define EFX_CSEL_HD
#endif

namespace efx {
namespace csel {

constexpr int64_t kMaxIndex = INT32_MAX;  // source pictures offered so far, and the largest output index
constexpr int64_t kMaxTerm = ((int64_t)1 << 31) - 1;  // A and B: (2 n + 1) A and N B stay inside 63 bits
constexpr int kMaxRatio = 64;             // source rate : output rate, either way

struct Ratio {
    int64_t A, B;
};

// picture_rate code 1 .. 8 as a fraction of Hz
EFX_CSEL_HD inline bool code_rate(int code, int64_t* num, int64_t* den)
{
    const int32_t n[9] = {0, 24000, 24, 25, 30000, 30, 50, 60000, 60};
    if (code < 1 || code > 8)
        return false;
    *num = n[code];
    *den = n[code] >= 1000 ? 1001 : 1;
    return true;
}

// the code whose rate is num / den exactly, or 0
EFX_CSEL_HD inline int rate_code(int64_t num, int64_t den)
{
    if (num < 1 || den < 1 || num > INT32_MAX || den > INT32_MAX)
        return 0;
    for (int c = 1; c <= 8; c++) {
        int64_t cn, cd;
        code_rate(c, &cn, &cd);
        if (num * cd == cn * den)
            return c;
    }
    return 0;
}

EFX_CSEL_HD inline int64_t gcd(int64_t a, int64_t b)
{
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// A : B of a source rate and an output code; false where the call rejects them (a rate out of range, a reduced term of
// 2^31 or more, a ratio above kMaxRatio either way)
EFX_CSEL_HD inline bool ratio(int64_t in_num, int64_t in_den, int out_code, Ratio* r)
{
    int64_t on, od;
    if (in_num < 1 || in_num > INT32_MAX || in_den < 1 || in_den > INT32_MAX || !code_rate(out_code, &on, &od))
        return false;
    int64_t a = in_num * od, b = 2 * on * in_den;  // < 2^41, < 2^48
    const int64_t g = gcd(a, b);
    a /= g;
    b /= g;
    if (a > kMaxTerm || b > kMaxTerm)
        return false;
    // r / o = 2 A / B
    if (2 * a > kMaxRatio * b || b > 2 * kMaxRatio * a)
        return false;
    r->A = a;
    r->B = b;
    return true;
}

// the source picture of output n (0 <= n <= kMaxIndex)
EFX_CSEL_HD inline int64_t source(const Ratio& r, int64_t n) { return ((2 * n + 1) * r.A - 1) / r.B; }

// outputs whose source is among the first N source pictures (0 <= N <= kMaxIndex)
EFX_CSEL_HD inline int64_t outputs(const Ratio& r, int64_t N)
{
    const int64_t t = N * r.B + 1 - r.A;
    return t <= 0 ? 0 : (t + 2 * r.A - 1) / (2 * r.A);
}

// A call's pictures first_picture .. first_picture + n_pictures - 1 and its outputs outputs(first_picture) ..
// outputs(first_picture + n_pictures) - 1 stay inside the bounds
EFX_CSEL_HD inline bool span_ok(const Ratio& r, int64_t first_picture, int64_t n_pictures)
{
    if (first_picture < 0 || n_pictures < 0 || first_picture > kMaxIndex || n_pictures > kMaxIndex ||
        first_picture + n_pictures > kMaxIndex)
        return false;
    return outputs(r, first_picture + n_pictures) - 1 <= kMaxIndex;
}

// outputs of a call (may be 0); -1 for arguments the call rejects
EFX_CSEL_HD inline int64_t count(int64_t in_num, int64_t in_den, int out_code, int64_t first_picture, int64_t n_pictures)
{
    Ratio r;
    if (!ratio(in_num, in_den, out_code, &r) || !span_ok(r, first_picture, n_pictures))
        return -1;
    return outputs(r, first_picture + n_pictures) - outputs(r, first_picture);
}

// title index of the source picture of output n; -1 for arguments the call rejects
EFX_CSEL_HD inline int64_t source_of(int64_t in_num, int64_t in_den, int out_code, int64_t n)
{
    Ratio r;
    if (!ratio(in_num, in_den, out_code, &r) || n < 0 || n > kMaxIndex)
        return -1;
    return source(r, n);
}

}  // namespace csel
}  // namespace efx
