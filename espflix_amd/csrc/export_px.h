// export_px.h -- per-pixel arithmetic of k_export (k_export.hip): chroma upsampling taps and the YCbCr -> RGB matrix.
//
// Host + device: the kernel runs exactly these functions, and tests/test_export_model.py builds this header with a plain
// C++ compiler and checks it against the NumPy model (tests/export_model.py) over every (Y, U, V) triple.  Everything is
// an integer function of the frame bytes, so the export is bit-exact by construction (the formulas: include/efx.h).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EFX_PX_HD __host__ __device__
#else
#define EFX_PX_HD
#endif

namespace efx {
namespace px {

// 8-bit fixed-point matrix: R = (t + rv v) >> 8, G = (t + gu u + gv v) >> 8, B = (t + bu u) >> 8, t = cy (Y - y0) + 128
struct Matrix {
    int cy, y0, rv, gu, gv, bu;
};

EFX_PX_HD inline Matrix matrix(int full_range)
{
    // BT.601: studio swing (what MPEG-1 carries: Y 16..235, Cb / Cr 16..240) or full range (JFIF)
    return full_range ? Matrix{256, 0, 359, -88, -183, 454} : Matrix{298, 16, 409, -100, -208, 516};
}

EFX_PX_HD inline int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One pixel: 0x00BBGGRR.  (>> of a negative int is an arithmetic shift in every compiler this builds with, C++20 by rule)
EFX_PX_HD inline uint32_t rgb(const Matrix& m, int y, int u, int v)
{
    const int t = m.cy * (y - m.y0) + 128;
    u -= 128;
    v -= 128;
    const int r = clamp_u8((t + m.rv * v) >> 8);
    const int g = clamp_u8((t + m.gu * u + m.gv * v) >> 8);
    const int b = clamp_u8((t + m.bu * u) >> 8);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

// MPEG-1 chroma siting: a chroma sample lies centred between its 2 x 2 luma samples, so luma column x (row y) takes
// chroma column x >> 1 with weight 3/4 and its neighbour on the side x lies on with weight 1/4, clamped at the edge.
EFX_PX_HD inline int near_tap(int x, int last)
{
    const int c = (x >> 1) + ((x & 1) ? 1 : -1);
    return c < 0 ? 0 : (c > last ? last : c);
}

// The vertical half of the bilinear filter: 3 C[cy0] + C[cy1] (0 .. 1020)
EFX_PX_HD inline int vtap(int c_near_row, int c_far_row) { return 3 * c_near_row + c_far_row; }
// ... and the horizontal half on two vertical sums: (9 C00 + 3 C01 + 3 C10 + C11 + 8) >> 4 exactly
EFX_PX_HD inline int htap(int v_near_col, int v_far_col) { return (3 * v_near_col + v_far_col + 8) >> 4; }

// The 2 x 2 filter in one call (C[cy0][cx0], C[cy0][cx1], C[cy1][cx0], C[cy1][cx1])
EFX_PX_HD inline int bilinear(int c00, int c01, int c10, int c11) { return htap(vtap(c00, c10), vtap(c01, c11)); }

}  // namespace px
}  // namespace efx
