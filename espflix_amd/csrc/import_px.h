// import_px.h -- arithmetic of k_import (k_import.hip): the RGB -> YCbCr matrix, the resampling taps of one axis and the
// two rounding steps of the separable filter.
//
// Host + device: the kernels run exactly these functions, tests/test_import_model.py builds this header with a plain C++
// compiler and checks it against the NumPy model (tests/import_model.py), and tests/import_model_main.cpp performs a
// whole import with them on the host.  Everything is an integer function of the source bytes, so the import is bit-exact
// by construction (the formulas: include/efx.h).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EFX_IPX_HD __host__ __device__
#else
#define EFX_IPX_HD
#endif

namespace efx {
namespace ipx {

constexpr int kCoefOne = 16384;  // the coefficients of one window sum to this
constexpr int kMaxRatio = 32;    // crop extent <= kMaxRatio x extent of the destination rectangle, which bounds a window
                                 // (<= 2 S / D + 1 taps): 65 taps for luma and the chroma of an I420 source, 129 for the
                                 // chroma of an RGB source, which goes from the full crop to half the rectangle
constexpr int kMaxTaps = 130;

EFX_IPX_HD inline int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// 8-bit fixed-point BT.601 matrix: Y = ((yr R + yg G + yb B + 128) >> 8) + y0, Cb = ((ur R + ug G + ub B + 128) >> 8) + 128,
// Cr likewise (>> of a negative int is an arithmetic shift in every compiler this builds with, C++20 by rule)
struct Matrix {
    int yr, yg, yb, y0;
    int ur, ug, ub;
    int vr, vg, vb;
};

EFX_IPX_HD inline Matrix matrix(int full_range)
{
    // studio swing (what MPEG-1 carries: Y 16..235, Cb / Cr 16..240) or full range (JFIF)
    return full_range ? Matrix{77, 150, 29, 0, -43, -85, 128, 128, -107, -21}
                      : Matrix{66, 129, 25, 16, -38, -74, 112, 112, -94, -18};
}

// One pixel: Y | Cb << 8 | Cr << 16
EFX_IPX_HD inline uint32_t ycbcr(const Matrix& m, int r, int g, int b)
{
    const int y = clamp_u8(((m.yr * r + m.yg * g + m.yb * b + 128) >> 8) + m.y0);
    const int u = clamp_u8(((m.ur * r + m.ug * g + m.ub * b + 128) >> 8) + 128);
    const int v = clamp_u8(((m.vr * r + m.vg * g + m.vb * b + 128) >> 8) + 128);
    return (uint32_t)y | ((uint32_t)u << 8) | ((uint32_t)v << 16);
}

// The taps of one axis, source extent S -> destination extent D (S <= kMaxRatio D), M = max(S, D): a triangle filter
// widened by the down-scaling ratio, centre-aligned.  Source index s weighs u(s) = max(0, 2M - |(2s + 1) D - (2d + 1) S|)
// for destination index d.
EFX_IPX_HD inline int64_t floor_div(int64_t a, int64_t b)  // b > 0
{
    const int64_t q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

EFX_IPX_HD inline int64_t raw_weight(int S, int D, int d, int s)
{
    const int64_t M = S > D ? S : D;
    int64_t v = (int64_t)(2 * s + 1) * D - (int64_t)(2 * d + 1) * S;
    if (v < 0)
        v = -v;
    return v < 2 * M ? 2 * M - v : 0;
}

// The window of d: every s in [0, S) with u(s) > 0 -- contiguous, never empty (s = floor((2d + 1) S / 2D) is inside), cut
// at the edges of the source.  Returns the first index, *count = the number of taps (<= kMaxTaps).
EFX_IPX_HD inline int window(int S, int D, int d, int* count)
{
    const int64_t M = S > D ? S : D, c = (int64_t)(2 * d + 1) * S;
    // (2s + 1) D > c - 2M  <=>  s >= floor((c - 2M - D) / 2D) + 1;   (2s + 1) D < c + 2M  <=>  s <= floor((c + 2M - D - 1) / 2D)
    int64_t lo = floor_div(c - 2 * M - D, 2 * (int64_t)D) + 1;
    int64_t hi = floor_div(c + 2 * M - D - 1, 2 * (int64_t)D);
    if (lo < 0)
        lo = 0;
    if (hi > S - 1)
        hi = S - 1;
    *count = (int)(hi - lo + 1);
    return (int)lo;
}

// The coefficients of d's window: k(s) = floor(u(s) 16384 / U), U = sum of u; what is missing to 16384 goes to the tap
// with the largest u, the first such tap on a tie.  k has room for kMaxTaps entries.  Returns the window's first index.
EFX_IPX_HD inline int taps(int S, int D, int d, int* count, uint16_t* k)
{
    int n;
    const int start = window(S, D, d, &n);
    int64_t U = 0, best = -1;
    int best_i = 0;
    for (int i = 0; i < n; i++) {
        const int64_t u = raw_weight(S, D, d, start + i);
        U += u;
        if (u > best) {
            best = u;
            best_i = i;
        }
    }
    int sum = 0;
    for (int i = 0; i < n; i++) {
        const int c = (int)(raw_weight(S, D, d, start + i) * kCoefOne / U);
        k[i] = (uint16_t)c;
        sum += c;
    }
    k[best_i] = (uint16_t)(k[best_i] + (kCoefOne - sum));
    *count = n;
    return start;
}

// Where the kernel finds a row segment: bytes [off, off + len) counted from the image's 16-byte aligned start are fetched
// as the 16-byte pieces [a0, a0 + 16 pieces) with a0 = off rounded down to 16, the segment begins `shift` bytes into them.
// The last piece ends at most at the image's size rounded up to 16.
struct Span {
    size_t a0;
    int pieces, shift;
};

EFX_IPX_HD inline Span span(size_t off, int len)
{
    const size_t a0 = off & ~(size_t)15;
    return Span{a0, (int)((off + (size_t)len - a0 + 15) >> 4), (int)(off - a0)};
}

// Byte offset of the crop's row r (of its chroma row r for planes 1, 2) in an I420 image: plane 0 = Y, 1 = Cb, 2 = Cr
EFX_IPX_HD inline size_t i420_row(int plane, int width, int height, int crop_x, int crop_y, int r)
{
    const size_t y_bytes = (size_t)width * height;
    if (plane == 0)
        return (size_t)(crop_y + r) * width + crop_x;
    return y_bytes + (plane == 2 ? y_bytes / 4 : 0) + (size_t)(crop_y / 2 + r) * (width / 2) + crop_x / 2;
}
// ... in an RGB24 image (3 crop_w bytes, R G B interleaved) and in plane c of an RGBP image (crop_w bytes)
EFX_IPX_HD inline size_t rgb24_row(int width, int crop_x, int crop_y, int r) { return ((size_t)(crop_y + r) * width + crop_x) * 3; }
EFX_IPX_HD inline size_t rgbp_row(int c, int width, int height, int crop_x, int crop_y, int r)
{
    return (size_t)c * width * height + (size_t)(crop_y + r) * width + crop_x;
}

// Horizontal pass: sum = sum of k_x * p over the window (<= 16384 x 255); the result fits 16 bits (<= 65280)
EFX_IPX_HD inline int hround(int sum) { return (sum + 32) >> 6; }
// Vertical pass: sum = sum of k_y * h (< 2^31)
EFX_IPX_HD inline int vround(int sum) { return clamp_u8((int)(((uint32_t)sum + (1u << 21)) >> 22)); }

}  // namespace ipx
}  // namespace efx
