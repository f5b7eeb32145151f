// quality_px.h -- arithmetic of k_quality (k_quality.hip): the reference clamp on packed bytes, the sums of a 4 x 4 block,
// the 8 x 8 SSIM window made of four blocks, its Q16 quotient, the window and sample counts, and how a band of an image
// is dealt to the threads of a workgroup.
//
// Host + device: the kernel runs exactly these functions, efx_api.hip's host helpers take their counts from here,
// tests/test_quality_model.py builds this header with a plain C++ compiler and checks it against the NumPy model
// (tests/quality_model.py), and tests/quality_model_main.cpp performs whole comparisons with them on the host.
// Everything is an integer function of the two pictures' bytes, so the records are bit-exact by construction (the
// definition: include/efx.h, "picture quality").
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EFX_QPX_HD __host__ __device__
#else
#define EFX_QPX_HD
#endif

namespace efx {
namespace qpx {

constexpr int kImageBytes = 101376;
constexpr int kC1 = 416, kC2 = 235963;  // (0.01 x 255)^2 x 64 and (0.03 x 255)^2 x 64 x 63, rounded: x264's ssim_end1
constexpr int kBands = 12;              // a band: one macroblock row -- 16 luma rows and 8 rows of each chroma plane
constexpr int kThreads = 192;           // of a workgroup: a band has at most 176 block tasks
constexpr int kStageBlocks = 5 * 88 + 2 * 3 * 44;  // the block sums of a band and of the block row below it

// plane 0 = Y, 1 = Cb, 2 = Cr
EFX_QPX_HD inline int plane_width(int p) { return p ? 176 : 352; }
EFX_QPX_HD inline int plane_offset(int p) { return p == 0 ? 0 : (p == 1 ? 67584 : 84480); }
EFX_QPX_HD inline int block_cols(int p) { return p ? 44 : 88; }
EFX_QPX_HD inline int block_rows(int p) { return p ? 24 : 48; }
EFX_QPX_HD inline int band_block_rows(int p) { return p ? 2 : 4; }  // block rows a band owns
EFX_QPX_HD inline int stage_base(int p) { return p == 0 ? 0 : (p == 1 ? 440 : 572); }
EFX_QPX_HD inline int64_t windows(int p) { return p == 0 ? 87 * 47 : ((p == 1 || p == 2) ? 43 * 23 : 0); }
EFX_QPX_HD inline int64_t samples(int p) { return p == 0 ? 67584 : ((p == 1 || p == 2) ? 16896 : 0); }

// min(a, m) on each of the four bytes of a word, 1 <= m <= 255, without a branch: a byte exceeds m exactly when
// a + (255 - m) carries out of the byte; the carry is put together from the low seven bits' sum and the top bits, so no
// add crosses a byte.
EFX_QPX_HD inline uint32_t clamp4(uint32_t a, uint32_t m)
{
    const uint32_t cc = (255u - m) * 0x01010101u, m4 = m * 0x01010101u;
    const uint32_t lo = (a & 0x7F7F7F7Fu) + (cc & 0x7F7F7F7Fu);
    const uint32_t g = ((a & cc) | ((a | cc) & lo)) & 0x80808080u;
    const uint32_t mask = (g - (g >> 7)) | g;
    return (a & ~mask) | (m4 & mask);
}

// The sums of a 4 x 4 block: s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b (a: the clamped reference)
struct Block {
    uint32_t s1, s2, ss, s12;
};

// Four pels of one row, packed, into the block's sums
EFX_QPX_HD inline void add_row(uint32_t a, uint32_t b, Block* k)
{
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    k->s1 = __builtin_amdgcn_sad_u8(a, 0u, k->s1);
    k->s2 = __builtin_amdgcn_sad_u8(b, 0u, k->s2);
    k->ss = __builtin_amdgcn_udot4(a, a, k->ss, false);
    k->ss = __builtin_amdgcn_udot4(b, b, k->ss, false);
    k->s12 = __builtin_amdgcn_udot4(a, b, k->s12, false);
#else
    for (int i = 0; i < 4; i++) {
        const uint32_t x = (a >> (8 * i)) & 0xFF, y = (b >> (8 * i)) & 0xFF;
        k->s1 += x, k->s2 += y, k->ss += x * x + y * y, k->s12 += x * y;
    }
#endif
}

// sum (a - b)^2 of a block (ss >= 2 s12)
EFX_QPX_HD inline uint32_t block_sse(const Block& k) { return k.ss - 2u * k.s12; }

// floor(|num| x 65536 / den) with num's sign, |num| <= den, 0 < den < 2^62.  |num| x 65536 does not fit 64 bits, so the
// quotient is not made by one division: a single-precision estimate of the ratio (relative error below 2^-21, so at most
// one off) is corrected with the remainder |num| x 65536 - q x den, which is below 2 den in magnitude and therefore exact
// in wrapping 64-bit arithmetic.  The result does not depend on how the estimate was rounded: the host divides, the
// device multiplies by v_rcp_f32.
EFX_QPX_HD inline int32_t q16(int64_t num, int64_t den)
{
    const uint64_t r = num < 0 ? (uint64_t)(-num) : (uint64_t)num, d = (uint64_t)den;
    uint32_t q = 65536;
    if (r < d) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
        const float e = (float)r * __builtin_amdgcn_rcpf((float)d);
#else
        const float e = (float)r / (float)d;
#endif
        q = (uint32_t)(e * 65536.0f);
        uint64_t rem = (r << 16) - (uint64_t)q * d;  // (both terms wrap; their difference does not)
        while ((int64_t)rem < 0)
            q--, rem += d;
        while (rem >= d)
            q++, rem -= d;
    }
    return num < 0 ? -(int32_t)q : (int32_t)q;
}

// num and den of a window from the sums of its four blocks.  S1, S2 <= 16320, SS <= 8 323 200, S12 <= 4 161 600: every
// factor fits 32 bits (64 SS, S1^2 + S2^2 <= 532 684 800; |2 covar| <= vars), the two products 64.
EFX_QPX_HD inline void window(uint32_t S1, uint32_t S2, uint32_t SS, uint32_t S12, int64_t* num, int64_t* den)
{
    const uint32_t sq = S1 * S1 + S2 * S2, p = S1 * S2;
    const int32_t vars = (int32_t)(64u * SS - sq);
    const int32_t covar = (int32_t)(64u * S12) - (int32_t)p;
    *num = (int64_t)(int32_t)(2u * p + kC1) * (int64_t)(2 * covar + kC2);
    *den = (int64_t)(sq + kC1) * (int64_t)(vars + kC2);
}

EFX_QPX_HD inline int32_t window_q16(const Block& a, const Block& b, const Block& c, const Block& d)
{
    int64_t num, den;
    window(a.s1 + b.s1 + c.s1 + d.s1, a.s2 + b.s2 + c.s2 + d.s2, a.ss + b.ss + c.ss + d.ss, a.s12 + b.s12 + c.s12 + d.s12, &num, &den);
    return q16(num, den);
}

// How a band is dealt out.  Band b owns luma block rows 4b .. 4b + 3 and block rows 2b, 2b + 1 of each chroma plane,
// and the windows whose upper blocks lie in them; those of its last row reach into the next band's first block row
// (the halo), whose sums the band computes as well, for its windows only.
//
// A block task: four blocks side by side (16 pels x 4 rows: four 16-byte pieces of each picture) -- in luma the four
// blocks of one macroblock's block row.  row: block row within the band (halo: row == band_block_rows(plane)).
struct BlockTask {
    int plane, row, quad;
    bool valid, halo;
};

EFX_QPX_HD inline BlockTask block_task(int band, int t)
{
    const int nl = band < kBands - 1 ? 5 : 4, nc = band < kBands - 1 ? 3 : 2;
    BlockTask k{0, 0, 0, true, false};
    if (t < 22 * nl) {
        k.row = t / 22, k.quad = t - 22 * k.row;
    } else {
        t -= 22 * nl;
        k.plane = 1;
        if (t >= 11 * nc)
            t -= 11 * nc, k.plane = 2;
        k.row = t / 11, k.quad = t - 11 * k.row;
        k.valid = t < 11 * nc;
    }
    k.halo = k.row >= band_block_rows(k.plane);
    return k;
}

// Byte offset in the image of pel row r (0 .. 3) of a task's 16 pels; where its first block's sums go in the stage
EFX_QPX_HD inline int task_offset(int band, const BlockTask& k, int r)
{
    return plane_offset(k.plane) + ((band * band_block_rows(k.plane) + k.row) * 4 + r) * plane_width(k.plane) + 16 * k.quad;
}
EFX_QPX_HD inline int task_stage(const BlockTask& k) { return stage_base(k.plane) + k.row * block_cols(k.plane) + 4 * k.quad; }

// A window task: the window whose upper left block is (row, col) of the band's blocks of a plane
struct WindowTask {
    int plane, row, col;
};

EFX_QPX_HD inline int band_windows(int band) { return band < kBands - 1 ? 4 * 87 + 2 * 2 * 43 : 3 * 87 + 2 * 43; }

EFX_QPX_HD inline WindowTask window_task(int band, int w)  // w < band_windows(band)
{
    const int wl = (band < kBands - 1 ? 4 : 3) * 87, wc = (band < kBands - 1 ? 2 : 1) * 43;
    WindowTask k{0, 0, 0};
    if (w < wl) {
        k.row = w / 87, k.col = w - 87 * k.row;
    } else {
        w -= wl;
        k.plane = 1;
        if (w >= wc)
            w -= wc, k.plane = 2;
        k.row = w / 43, k.col = w - 43 * k.row;
    }
    return k;
}

// The stage index of a window's upper left block; the others are at + 1, + block_cols(plane), + block_cols(plane) + 1
EFX_QPX_HD inline int window_stage(const WindowTask& k) { return stage_base(k.plane) + k.row * block_cols(k.plane) + k.col; }

}  // namespace qpx
}  // namespace efx
