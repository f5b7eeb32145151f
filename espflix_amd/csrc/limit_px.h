// limit_px.h -- arithmetic of k_limit_peaks and k_pcm_limit (k_limit.hip): the look-ahead peak limiter of include/efx.h,
// "peak limiter".  Block peaks, the gain each block requires under the ceiling, the sliding minimum and the box average
// over the block borders (nodes), the gain of a sample between two nodes and its application.
//
// Host + device: the kernels run exactly these functions, tests/test_limit_model.py builds this header with a plain C++
// compiler and checks it against the NumPy model (tests/limit_model.py), and tests/limit_model_main.cpp performs whole
// calls with them on the host.  Everything is an integer function of the samples, of the stream gain and of the ceiling:
// no floating point.  The two quotients per block (4096 C / p and sum / W) are unsigned 32-bit divisions; the quotient per
// sample (/ Bk) is a multiply and a shift whose exactness over every numerator the test checks.
#pragma once
#include <stdint.h>

#include "loudness_px.h"

namespace efx {
namespace limit {

constexpr int kMaxHalf = 64;       // H, blocks
constexpr int kDefaultHalf = 32;
constexpr int kTile = 256;         // blocks of a workgroup's tile, in both kernels
constexpr int kThreads = 256;
constexpr int kHalo = 2 * kMaxHalf + 1;           // blocks either side of a tile whose peaks its samples depend on, at most
constexpr int kMaxNodes = kTile + 4 * kMaxHalf + 2;  // peaks a tile reads with the largest window: 514
constexpr int64_t kMaxFirstSample = (int64_t)1 << 40;

// Bk: about 1 ms, a whole number of 32-byte pieces; 0 for a rate that is not one of the four
EFX_LOUD_HD inline int block_of(int rate)
{
    return rate == 16000 ? 16 : rate == 32000 ? 32 : (rate == 44100 || rate == 48000) ? 48 : 0;
}

// floor(n / Bk) = (n M) >> S for every n the interpolation can make (n <= 32767 Bk < 2^21): M and S of a block length
struct DivBk {
    uint32_t mul;
    int shift;
};
EFX_LOUD_HD inline DivBk div_of(int bk)
{
    // 16, 32: a shift written as a multiply, so that the three lengths share the code; 48: M = ceil(2^37 / 48), 48 M - 2^37 = 16,
    // exact while 16 n < 2^37
    return bk == 16 ? DivBk{0x80000000u, 35} : bk == 32 ? DivBk{0x80000000u, 36} : DivBk{2863311531u, 37};
}
EFX_LOUD_HD inline uint32_t div_bk(uint32_t n, DivBk d) { return (uint32_t)(((uint64_t)n * d.mul) >> d.shift); }

// r: the gain a block of peak p (0 .. 32768) may have: G where it is silent, else min(G, floor(4096 C / p)); may be 0
EFX_LOUD_HD inline uint32_t required(uint32_t p, uint32_t G, uint32_t C)
{
    if (p == 0)
        return G;
    const uint32_t cap = (4096u * C) / p;
    return cap < G ? cap : G;
}

// a: floor(sum / W), sum of W = 2H + 1 minima (sum <= 129 x 32767)
EFX_LOUD_HD inline uint32_t average(uint32_t sum, uint32_t W) { return sum / W; }

// the numerator of sample t's gain (t = 0 .. Bk - 1) between the nodes' a0 (the block's front border) and a1 (its rear)
EFX_LOUD_HD inline uint32_t lerp_num(uint32_t a0, uint32_t a1, int bk, int t) { return a0 * (uint32_t)(bk - t) + a1 * (uint32_t)t; }

// y = clamp16((x g + 2048) >> 12): loudness_px.h's apply_gain

// The largest |x| of eight samples held as four dwords: the maximum and the minimum taken separately and the minimum
// negated in 32 bits, so that -32768 counts as 32768
EFX_LOUD_HD inline uint32_t peak_of(int mx, int mn) { return (uint32_t)(mx > -mn ? mx : -mn); }

// ---- a whole stream on the host: what the two kernels compute, written serially (the test's and the model program's) ----
#if !defined(__HIP_DEVICE_COMPILE__)
// p[b] of the n samples x, b = 0 .. ceil(n / Bk) - 1
inline void host_peaks(const int16_t* x, int64_t n, int bk, uint16_t* p)
{
    for (int64_t b = 0; b * bk < n; b++) {
        int mx = 0, mn = 0;
        for (int64_t i = b * bk; i < n && i < (b + 1) * bk; i++) {
            mx = x[i] > mx ? x[i] : mx;
            mn = x[i] < mn ? x[i] : mn;
        }
        p[b] = (uint16_t)peak_of(mx, mn);
    }
}

// the peak of stream block b as a call sees it: entry b - peaks_first of a row of n_peaks, 0 outside
inline uint32_t peak_at(const uint16_t* peaks, int64_t peaks_first, int n_peaks, int64_t b)
{
    const int64_t e = b - peaks_first;
    return e >= 0 && e < n_peaks ? peaks[e] : 0;
}

// a[b] for one node, straight from the rule (W^2 work: the host's yardstick, not the kernel's method)
inline uint32_t host_node(const uint16_t* peaks, int64_t peaks_first, int n_peaks, int64_t b, int H, uint32_t G, uint32_t C)
{
    uint32_t sum = 0;
    for (int64_t j = b - H; j <= b + H; j++) {
        uint32_t m = G;
        for (int64_t k = j - H; k <= j + H; k++) {
            const uint32_t r0 = required(peak_at(peaks, peaks_first, n_peaks, k - 1), G, C);
            const uint32_t r1 = required(peak_at(peaks, peaks_first, n_peaks, k), G, C);
            const uint32_t q = r0 < r1 ? r0 : r1;
            m = q < m ? q : m;
        }
        sum += m;
    }
    return average(sum, (uint32_t)(2 * H + 1));
}

// efx_pcm_limit for one stream's piece: n samples from stream sample first (a multiple of Bk)
inline void host_limit(const int16_t* x, int64_t n, int64_t first, int bk, const uint16_t* peaks, int64_t peaks_first, int n_peaks,
                       int H, uint32_t G, uint32_t C, int16_t* y, uint16_t* gains = nullptr)
{
    const DivBk d = div_of(bk);
    for (int64_t b0 = 0; b0 * bk < n; b0++) {
        const int64_t b = first / bk + b0;
        const uint32_t a0 = host_node(peaks, peaks_first, n_peaks, b, H, G, C);
        const uint32_t a1 = host_node(peaks, peaks_first, n_peaks, b + 1, H, G, C);
        for (int t = 0; t < bk && b0 * bk + t < n; t++) {
            const uint32_t g = div_bk(lerp_num(a0, a1, bk, t), d);
            y[b0 * bk + t] = (int16_t)loud::apply_gain(x[b0 * bk + t], (int)g);
            if (gains)
                gains[b0 * bk + t] = (uint16_t)g;
        }
    }
}
#endif

}  // namespace limit
}  // namespace efx
