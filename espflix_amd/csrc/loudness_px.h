// loudness_px.h -- arithmetic of k_loud_steps, k_loud_gate and k_pcm_gain (k_loudness.hip): the K-weighting recurrence in
// fixed point, the energy and the peak of a 100 ms step, the two gates of ITU-R BS.1770-4 on integer block energies, the
// gain that takes a stream to a target under a peak ceiling, and its application; and the plan of an efx_loudness_steps
// call (the constants the host works out once and hands the kernels by value).
//
// Host + device: the kernels run exactly these functions, tests/test_loudness_model.py builds this header with a plain
// C++ compiler and checks it against the NumPy model (tests/loudness_model.py), and tests/loudness_model_main.cpp performs
// whole calls with them on the host, with the kernels' own addressing.  Everything is an integer function of the samples
// and of the integer coefficients and thresholds the host passes in (the formulas: include/efx.h): no floating point and
// no `/` on the device (the two quotients of the gain are long divisions written out here).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EFX_LOUD_HD __host__ __device__
#else
#define EFX_LOUD_HD
#endif

namespace efx {
namespace loud {

typedef unsigned __int128 u128;

constexpr int kF = 12;                    // fraction bits of the filter's input, of both stages' outputs
constexpr int kCoefBits = 28;             // fraction bits of the coefficients
constexpr int kEnergyShift = kF - 4;      // the squared value keeps four fraction bits
constexpr int kUnity = 4096;              // gain_q12 of 0 dB
constexpr int kMaxGain = 32767;
constexpr int kMaxHist = 7200;            // samples of a state at 48 kHz, the largest
constexpr int kMaxSteps = 1 << 24;        // steps of one efx_loudness_gate call: the split sums below stay inside 64 bits
constexpr int64_t kMaxFirstSample = (int64_t)1 << 40;
constexpr uint64_t kMaxTarget = (uint64_t)1 << 40;  // target_ms below it: 2^24 T 4 step < 2^79

constexpr int kLanes = 64;                // steps of a k_loud_steps wave, one lane each
constexpr int kChunk = 64;                // samples of a row staged per trip: 128 bytes
constexpr int kRowPitch16 = 9;            // 16-byte slots between staged rows: 36 dwords, so that the 16 lanes that read
                                          // together (9 r mod 16 takes every value) fall on 16 different slots of the bank row

inline bool rate_ok(int rate) { return rate == 16000 || rate == 32000 || rate == 44100 || rate == 48000; }
EFX_LOUD_HD inline int step_of(int rate) { return rate / 10; }
EFX_LOUD_HD inline int runin_of(int rate) { return rate / 20; }
// samples a stream's state holds: the newest W + step, rounded up to whole 16-byte pieces (6616 at 44.1 kHz)
EFX_LOUD_HD inline int hist_of(int rate) { return (step_of(rate) + runin_of(rate) + 7) & ~7; }

struct Coefs {
    int32_t c[10];  // b0 b1 b2 a1 a2 of the shelf, then of the high pass; round(2^28 x)
};

// 16 bytes, written with one store
struct StepRec {
    uint64_t energy;
    uint32_t peak;
    uint32_t zero;
};

// efx_loudness_rec
struct GateRec {
    uint64_t gated_mean, max_block;
    uint32_t n_gated, n_blocks, n_abs;
    uint16_t peak, gain_q12;
};

struct Filter {
    int32_t x1, x2, y1, y2, z1, z2;  // the input's, the shelf's and the high pass's last two values
};

// One sample through both stages, direct form I.  |x| <= 2^15: |x0| <= 2^27; |y|, |z| <= 3.4 x 2^27 < 2^29 (the L1 norms
// of the impulse responses: tests/test_loudness_model.py); |coefficient| < 2^29.1: a sum of five products stays below
// 5 x 2^58.1 < 2^61.  >> of a negative value is an arithmetic shift in every compiler this builds with.
EFX_LOUD_HD inline int32_t kweight(const Coefs& k, Filter& f, int x)
{
    const int32_t x0 = x * (1 << kF);
    const int64_t half = (int64_t)1 << (kCoefBits - 1);
    const int64_t a = (int64_t)k.c[0] * x0 + (int64_t)k.c[1] * f.x1 + (int64_t)k.c[2] * f.x2 - (int64_t)k.c[3] * f.y1 -
                      (int64_t)k.c[4] * f.y2;
    const int32_t y = (int32_t)((a + half) >> kCoefBits);
    const int64_t b = (int64_t)k.c[5] * y + (int64_t)k.c[6] * f.y1 + (int64_t)k.c[7] * f.y2 - (int64_t)k.c[8] * f.z1 -
                      (int64_t)k.c[9] * f.z2;
    const int32_t z = (int32_t)((b + half) >> kCoefBits);
    f.x2 = f.x1, f.x1 = x0;
    f.y2 = f.y1, f.y1 = y;
    f.z2 = f.z1, f.z1 = z;
    return z;
}

// s^2 with s = (z + 2^(F - 5)) >> (F - 4); |s| < 2^21
EFX_LOUD_HD inline uint64_t energy_of(int32_t z)
{
    const int64_t s = (z + (1 << (kEnergyShift - 1))) >> kEnergyShift;
    return (uint64_t)(s * s);
}

EFX_LOUD_HD inline uint32_t abs16(int x) { return (uint32_t)(x < 0 ? -x : x); }  // 32768 for -32768

// One lane of k_loud_steps: a step and the run-in in front of it
struct Lane {
    Filter f;
    uint64_t energy;
    uint32_t peak;
};

// `inside`: the sample belongs to the lane's W + step (else the filter is fed a zero, which leaves a filter at rest at
// rest and is never measured); `measured`: it belongs to the step itself
EFX_LOUD_HD inline void feed(const Coefs& k, Lane& l, int x, bool inside, bool measured)
{
    x = inside ? x : 0;
    const int32_t z = kweight(k, l.f, x);
    l.energy += measured ? energy_of(z) : 0;
    const uint32_t ax = measured ? abs16(x) : 0;
    l.peak = ax > l.peak ? ax : l.peak;
}

// The constants of an efx_loudness_steps call
struct Plan {
    int rate, step, runin, hist;
    int n_samples;
    int n_new;    // steps that become whole in this call
    int row0;     // where the first of them begins its run-in, counted from the call's first sample: -(pending + W)
    Coefs k;
};

inline int64_t step_count(int rate, int64_t first_sample, int64_t n_samples)
{
    const int step = step_of(rate);
    return (first_sample + n_samples) / step - first_sample / step;
}

// (arguments checked by the caller: efx_loudness_steps)
inline Plan plan(int rate, const Coefs& k, int64_t first_sample, int n_samples)
{
    Plan p{};
    p.rate = rate, p.step = step_of(rate), p.runin = runin_of(rate), p.hist = hist_of(rate);
    p.n_samples = n_samples;
    p.n_new = (int)step_count(rate, first_sample, n_samples);
    p.row0 = -(int)(first_sample % p.step) - p.runin;
    p.k = k;
    return p;
}

// ---- gating ---------------------------------------------------------------------------------------------------------------
// A sum of up to 2^24 block energies (each below 2^56) as the sums of their halves: integer adds in any order
struct Acc {
    uint64_t lo, hi;
    uint32_t n;
};

EFX_LOUD_HD inline void acc_add(Acc& a, uint64_t b)
{
    a.lo += b & 0xFFFFFFFFu;
    a.hi += b >> 32;
    a.n++;
}

EFX_LOUD_HD inline u128 acc_sum(uint64_t lo, uint64_t hi) { return ((u128)hi << 32) + lo; }

// 10 B n_abs > S_abs: the block is above a tenth of the mean of the blocks that passed the absolute gate (-10 LU)
EFX_LOUD_HD inline bool rel_pass(uint64_t B, uint32_t n_abs, u128 S_abs) { return (u128)B * (10ull * n_abs) > S_abs; }

// floor(n / d), d >= 1, 2^64 - 1 where the quotient does not fit: shift and subtract, 64 rounds
EFX_LOUD_HD inline uint64_t udiv128(u128 n, uint64_t d)
{
    uint64_t r = (uint64_t)(n >> 64);
    const uint64_t lo = (uint64_t)n;
    if (r >= d)
        return ~(uint64_t)0;
    uint64_t q = 0;
    for (int i = 63; i >= 0; i--) {
        const bool carry = (r >> 63) != 0;
        r = (r << 1) | ((lo >> i) & 1);
        q <<= 1;
        if (carry || r >= d) {
            r -= d;
            q |= 1;
        }
    }
    return q;
}

// floor(sqrt(x)), x < 2^62
EFX_LOUD_HD inline uint32_t isqrt(uint64_t x)
{
    uint64_t r = 0;
    for (uint64_t b = (uint64_t)1 << 60; b; b >>= 2) {
        if (x >= r + b) {
            x -= r + b;
            r = (r >> 1) + b;
        } else {
            r >>= 1;
        }
    }
    return (uint32_t)r;
}

// The gain that takes a stream to the target with no regard to its peak (include/efx.h): T = target_ms < 2^40; 1 .. 32767.
// What gain_q12 caps and what the limiter (limit_px.h) aims at.
EFX_LOUD_HD inline int stream_gain_q12(uint64_t gated_mean, uint32_t n_gated, uint64_t T, int step)
{
    if (n_gated == 0)
        return kUnity;
    uint64_t q = udiv128(((u128)T << 24) * (uint64_t)(4 * step), gated_mean ? gated_mean : 1);
    if (q > ((uint64_t)1 << 32))
        q = (uint64_t)1 << 32;  // (the clamp below is at 32767)
    const uint64_t g = isqrt(q);
    return g < 1 ? 1 : (g > (uint64_t)kMaxGain ? kMaxGain : (int)g);
}

// gain_q12 of a stream (include/efx.h): T = target_ms < 2^40, C = ceiling 1 .. 32767
EFX_LOUD_HD inline int gain_q12(uint64_t gated_mean, uint32_t n_gated, uint32_t peak, uint64_t T, uint32_t C, int step)
{
    if (n_gated == 0 || peak == 0)
        return kUnity;
    // (clamping the uncapped gain to 1 .. 32767 before the cap gives what clamping after it gave: min and clamp commute)
    uint64_t g = (uint64_t)stream_gain_q12(gated_mean, n_gated, T, step);
    const uint64_t cap = udiv128((u128)(4096ull * C), peak);
    g = g < cap ? g : cap;
    return g < 1 ? 1 : (int)g;
}

EFX_LOUD_HD inline int apply_gain(int x, int g)
{
    const int v = (x * g + 2048) >> 12;  // |x g| < 2^30
    return v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
}

}  // namespace loud
}  // namespace efx
