// import_pcm.h -- arithmetic of k_import_pcm (k_import_pcm.hip): the downmix, the polyphase coefficient read from the
// prototype table with linear interpolation, the 64-bit accumulation, the scaling of a down-sampling filter and the final
// rounding; and the plan of a call (the constants that the host works out once and hands the kernels by value).
//
// Host + device: the kernels run exactly these functions, tests/test_import_pcm_model.py builds this header with a plain
// C++ compiler and checks it against the NumPy model (tests/import_pcm_model.py), and tests/import_pcm_model_main.cpp
// performs whole calls with them on the host, with the kernels' own addressing.  Everything is an integer function of the
// source bytes (the formulas: include/efx.h).
//
// No division on the device: every quotient the kernels need has a divisor that is fixed for the call (the output rate,
// max(rates), the input rate, the channel count), so the host leaves the round-up reciprocal m = floor(2^64 / d) + 1 in
// the plan and the quotient is the high half of one 64 x 64 bit product -- exact while dividend x divisor < 2^64, which
// the comments at the call sites show.  (A `/` in device code expands to a sequence seeded by a floating-point
// reciprocal; this header keeps the device free of floating point altogether.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EFX_IPCM_HD __host__ __device__
#else
#define EFX_IPCM_HD
#endif

namespace efx {
namespace ipcm {

constexpr int kP = 512;                     // table entries per unit of the prototype's argument
constexpr int kQ = 22;                      // coefficient scale: T[i] = round(2^22 p(i / 512))
constexpr int kHalf = 16;                   // the prototype is zero from |u| = 16 on
constexpr int kTableLen = kHalf * kP + 1;   // T[0 .. 16 P]; T[16 P] = 0
constexpr int kFracBits = 12;               // interpolation between two entries in 1/4096
constexpr int kMaxW = 64;                   // W = ceil(16 max(r, o) / o) <= 64 because r <= 4 o
constexpr int kHist = 2 * kMaxW - 1;        // mixed samples a stream carries from call to call: 127
constexpr int kStateBytes = 256;            // 128 int16: hist[k] = m[first_in - 127 + k], hist[127] = 0
constexpr int kMaxChannels = 8;
constexpr int kMaxRatio = 4;                // in_rate <= 4 out_rate
constexpr int kMinRate = 8000, kMaxRate = 192000;
constexpr int64_t kMaxFirstIn = (int64_t)1 << 40;
constexpr int kLayoutInterleaved = 1, kLayoutPlanar = 2;  // EFX_PCM_INTERLEAVED, EFX_PCM_PLANAR

constexpr int kTile = 1024;                 // outputs of a workgroup's tile
// input frames a tile can need: (kTile - 1) r / o + 1 for the positions, 2 W - 1 behind the first
constexpr int kSpanMax = (kTile - 1) * kMaxRatio + 1 + 2 * kMaxW;

EFX_IPCM_HD inline int clamp16(int64_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : (int)v); }

// m[j] = clamp16((sum_c w[c] x[j][c] + 16384) >> 15); |sum| <= 32768 x 32768 because sum |w| <= 32768
EFX_IPCM_HD inline int mix_round(int32_t sum) { return clamp16((sum + 16384) >> 15); }

EFX_IPCM_HD inline uint64_t mulhi64(uint64_t a, uint64_t b)
{
    return (uint64_t)(((unsigned __int128)a * b) >> 64);  // (on the device: 32-bit multiplies, no call)
}

// m = floor(2^64 / d) + 1 (d a power of two: 2^64 / d, exact); floor(x / d) = mulhi64(x, m) whenever x d < 2^64:
// m = (2^64 + k) / d with 0 <= k <= d, so x m / 2^64 = x / d + x k / (d 2^64) and the excess stays below 1 / d.
inline uint64_t magic(uint64_t d) { return ~(uint64_t)0 / d + 1; }  // d >= 2
EFX_IPCM_HD inline uint64_t udiv(uint64_t x, uint64_t m) { return mulhi64(x, m); }

// The constants of a call
struct Plan {
    int r, o, M, W;        // rates, max(r, o), the delay ceil(16 M / o)
    int equal;             // r == o: y[n] = m[n]
    int channels, layout, n_in;
    int n_out;             // ceil((first_in + n_in) o / r) - ceil(first_in o / r)
    int base_rel;          // floor(n0 r / o) - first_in for the call's first output n0 = ceil(first_in o / r): 0 .. 4
    int rem0;              // (n0 r) mod o
    uint32_t dQ, dG;       // (o P 4096) div M and mod M: what a tap's table position grows by from tap to tap
    int w[kMaxChannels];   // downmix weights, defaults filled in
    uint64_t magic_o, magic_M, magic_r, magic_c;
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }  // a >= 0, b > 0

inline int delay(int r, int o)
{
    const int64_t M = r > o ? r : o;
    return r == o ? 0 : (int)ceil_div(16 * M, o);
}

// outputs of a call; first_in < 2^40 and o < 2^16, so the products stay below 2^57
inline int64_t out_samples(int r, int o, int64_t first_in, int64_t n_in)
{
    return ceil_div((first_in + n_in) * o, r) - ceil_div(first_in * o, r);
}

// (arguments checked by the caller: efx_import_pcm)
inline Plan plan(int r, int o, int channels, int layout, const int* mix_q15, int64_t first_in, int n_in)
{
    Plan p{};
    p.r = r, p.o = o, p.M = r > o ? r : o;
    p.equal = r == o;
    p.W = p.equal ? 0 : delay(r, o);
    p.channels = channels, p.layout = layout, p.n_in = n_in;
    p.n_out = (int)out_samples(r, o, first_in, n_in);
    const int64_t n0 = ceil_div(first_in * o, r);
    p.base_rel = (int)(n0 * r / o - first_in);
    p.rem0 = (int)(n0 * r % o);
    const uint64_t step = (uint64_t)o * kP << kFracBits;
    p.dQ = (uint32_t)(step / (uint64_t)p.M), p.dG = (uint32_t)(step % (uint64_t)p.M);
    bool all_zero = true;
    for (int c = 0; c < kMaxChannels; c++)
        all_zero = all_zero && mix_q15[c] == 0;
    for (int c = 0; c < channels; c++)
        p.w[c] = all_zero ? 32768 / channels : mix_q15[c];
    p.magic_o = magic((uint64_t)o), p.magic_M = magic((uint64_t)p.M), p.magic_r = magic((uint64_t)r);
    p.magic_c = magic((uint64_t)channels);
    return p;
}

// Output t of the call (t = 0 .. n_out - 1, global index n0 + t): a = (n0 + t) r = fl0 o + rem0 + t r, so with
// A = rem0 + t r: fl = fl0 + A div o and the phase a - fl o = A mod o.  A < o + n_out r <= n_in o + 2 r + o < 2^47 and
// o < 2^16: A o < 2^63.  Returns fl - first_in, the newest tap's frame counted from the call's first input frame.
EFX_IPCM_HD inline int position(const Plan& p, int t, int* phase)
{
    const uint64_t A = (uint64_t)p.rem0 + (uint64_t)t * (uint64_t)p.r;
    const uint64_t dq = udiv(A, p.magic_o);
    *phase = (int)(A - dq * (uint64_t)p.o);
    return p.base_rel + (int)dq;
}

// floor(acc o / r) of a down-sampling filter.  |acc| < 2^41 (sum |k| <= 2.28 x 2^22 x r / o, |m| <= 2^15) and o < 2^16:
// x = |acc| o < 2^57 goes through two exact steps, x = x1 2^28 + x0: x1 < 2^29, and (x1 mod r) 2^28 + x0 < r 2^28 < 2^46,
// both times r < 2^18 below 2^64.
EFX_IPCM_HD inline int64_t scale_down(const Plan& p, int64_t acc)
{
    const bool neg = acc < 0;
    uint64_t x = (uint64_t)(neg ? -acc : acc) * (uint64_t)p.o;
    if (neg)
        x += (uint64_t)p.r - 1;  // floor(-y / r) = -ceil(y / r)
    const uint64_t x1 = x >> 28, x0 = x & ((1u << 28) - 1);
    const uint64_t q1 = udiv(x1, p.magic_r), r1 = x1 - q1 * (uint64_t)p.r;
    const uint64_t q0 = udiv((r1 << 28) | x0, p.magic_r);
    const int64_t q = (int64_t)((q1 << 28) + q0);
    return neg ? -q : q;
}

// k of a tap at table position qf = (e P 4096) div M = q 4096 + f
template <class TP>
EFX_IPCM_HD inline int coef(TP T, uint32_t qf)
{
    const uint32_t q = qf >> kFracBits;
    if (q >= (uint32_t)(kHalf * kP))
        return 0;
    const int t0 = T[q], t1 = T[q + 1];
    // |t1 - t0| < 2^14 (the prototype's slope is below 1.4 per unit), so the product stays inside 32 bits; >> of a
    // negative int is an arithmetic shift in every compiler this builds with
    return t0 + (((t1 - t0) * (int)(qf & ((1u << kFracBits) - 1))) >> kFracBits);
}

// One run of W taps whose distances e = e0, e0 + o, e0 + 2 o, ... grow by o: sample i of the run is m[i * dir].
// (e0 P 4096 <= o 2^21 < 2^37 and M < 2^18.)  The table position steps with a carry, no division per tap.
template <class TP, class MP>
EFX_IPCM_HD inline int64_t run(const Plan& p, TP T, MP m, int dir, int e0)
{
    const uint64_t E = ((uint64_t)e0 * kP) << kFracBits;
    uint32_t qf = (uint32_t)udiv(E, p.magic_M);
    uint32_t g = (uint32_t)(E - (uint64_t)qf * (uint64_t)p.M);
    int64_t acc = 0;
    for (int i = 0; i < p.W; i++) {
        acc += (int64_t)coef(T, qf) * (int64_t)m[i * dir];
        qf += p.dQ;
        g += p.dG;
        if (g >= (uint32_t)p.M) {
            g -= (uint32_t)p.M;
            qf++;
        }
    }
    return acc;
}

// y[n] from the 2 W taps j = fl - 2 W + 1 .. fl; newest = &m[fl], phase = a - fl o in [0, o).  With tap j = fl - W + 1 + i
// the distance j o - a + W o is (i + 1) o - phase > 0 for i = 0 .. W - 1, and with j = fl - W - i it is -(phase + i o).
template <class TP, class MP>
EFX_IPCM_HD inline int output(const Plan& p, TP T, MP newest, int phase)
{
    int64_t acc = run(p, T, newest - p.W, -1, phase) + run(p, T, newest - p.W + 1, 1, p.o - phase);
    if (p.r > p.o)
        acc = scale_down(p, acc);
    return clamp16((acc + ((int64_t)1 << (kQ - 1))) >> kQ);
}

// Frame and channel of element e of an interleaved stream (e < 2^31, channels <= 8)
EFX_IPCM_HD inline int frame_of(const Plan& p, int e)
{
    return p.channels == 1 ? e : (int)udiv((uint64_t)e, p.magic_c);  // (2^64 / 1 has no 64-bit reciprocal)
}

}  // namespace ipcm
}  // namespace efx
