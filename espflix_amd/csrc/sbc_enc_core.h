// sbc_enc_core.h -- the arithmetic of the SBC encoder (k_sbc_enc.hip): analysis, scale factors, bit allocation,
// quantiser, header and CRC.
//
// Host + device: the kernel runs exactly these functions, and tests/sbc_encode_model.py builds this header with a plain
// C++ compiler (tests/sbc_enc_model_main.cpp), so the host model writes the bytes the device writes.  All integer.
//
// What binds it is the decoder (reference src/sbc_decoder.cpp): 8 subbands, mono or dual channel (291-292), its bit
// allocation (142-233) and its amplitude convention -- a subband sample comes back as
// ((2q + 1) << scale) / (2^bits - 1) - (1 << scale), inside (-2^scale, 2^scale) (257-264, 330-334).  PCM encoded here and
// decoded there returns at unity gain, 73 samples late: the analysis below is Appendix B's with its subband samples
// HALVED (S = S_standard / 2), which is what that convention amounts to.
//
// Analysis of one block (8 new samples), per channel, X[n] = the sample n places back from the block's newest:
//   Z[n] = C[n] X[n],  Y[i] = Z[i] + Z[i+16] + Z[i+32] + Z[i+48] + Z[i+64]   (i = 0..15; C = Proto_8_80, sbc_proto.h)
//   S[sb] = sum_i cos((sb + 1/2)(i - 4) pi / 8) Y[i]
// The cosine is even about i = 4 and odd about i = 12, so the sixteen Y fold into eight terms
//   T[0] = Y[4], T[k] = Y[4+k] + Y[4-k] (k = 1..4), T[k] = Y[4+k] - Y[20-k] (k = 5..7)     (Y[12] meets a zero)
//   S[sb] = sum_k cos((sb + 1/2) k pi / 8) T[k]
//
// Fixed-point formats:
//   X      int16 PCM                                                    Q0
//   W[n]   round(C[n] 2^16), |W| <= 9631                                Q16
//   T[k]   sum of ten (k = 0: five) W X                                 Q16, |T| <= 32768 sum|W| <= kMaxT < 2^31
//   M      round(cos 2^30), |M| <= 2^30                                 Q30
//   S      sum_k mulhi32(M, T[k]) = the standard's S x 2^14             Q15 of the halved S, |S| <= kMaxS < 2^31
//   u      S clamped to +-2^(scale+15), + 2^(scale+15)                  uint32 < 2^(scale+16) <= 2^31
//   q      umulhi32(u << (15 - scale), (2^bits - 1) << 1)               = floor(u (2^bits - 1) / 2^(scale+16))
// mulhi32 is the high word of the 32 x 32-bit product (v_mul_hi_i32 / v_mul_hi_u32 on the device): no value that is kept,
// added to or shifted is wider than 32 bits.  The bounds are static_asserts below; tests/test_sbc_encode_model.py
// runs the worst-case inputs (every tap at +-32768 with the sign of its coefficient) against a 64-bit evaluation.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sbc_proto.h"

#if defined(__HIPCC__)
#define EFX_SBC_HD __host__ __device__
#define EFX_SBC_HOST __host__
#define EFX_SBC_UNROLL _Pragma("unroll")
#else
#define EFX_SBC_UNROLL
#define EFX_SBC_HD
#define EFX_SBC_HOST
#endif

namespace efx {
namespace sbcenc {

constexpr int kHist = 72;          // samples of the past a block's 80 taps reach behind its own 8
constexpr int kMaxBlocks = 16, kSubbands = 8;
constexpr int kStateBytes = 2 * kHist * 2;  // per stream: the last 72 samples of each channel, oldest first (int16)
constexpr int kFracS = 15;         // S as kept: the halved S x 2^15

constexpr int32_t win_q16(int n)
{
    const double x = sbc_proto_tap(n) * 65536.0;
    return (int32_t)(x < 0 ? x - 0.5 : x + 0.5);
}

// The folded window: term j = 0..4 of T[k] is w[k][j] X[tap[k][j]], term 5 + j is w[k][5 + j] X[tap[k][5 + j]]
constexpr int fold_first(int k) { return 4 + k; }
constexpr int fold_second(int k) { return k == 0 ? -1 : (k <= 4 ? 4 - k : 20 - k); }
constexpr int fold_sign(int k) { return k <= 4 ? 1 : -1; }

struct Tables {
    int32_t w[8][10];    // Q16, the second five negated for k >= 5, zero for k = 0
    int32_t tap[8][10];  // n of X[n]
    int32_t m[8][8];     // m[sb][k] = round(2^30 cos((sb + 1/2) k pi / 8))
};

constexpr int64_t abs64(int64_t v) { return v < 0 ? -v : v; }
constexpr int64_t fold_abs_sum(int k)
{
    int64_t a = 0;
    for (int j = 0; j < 5; j++) {
        a += abs64(win_q16(fold_first(k) + 16 * j));
        if (fold_second(k) >= 0)
            a += abs64(win_q16(fold_second(k) + 16 * j));
    }
    return a;
}
constexpr int64_t max_t()
{
    int64_t m = 0;
    for (int k = 0; k < 8; k++)
        if (fold_abs_sum(k) * 32768 > m)
            m = fold_abs_sum(k) * 32768;
    return m;
}
constexpr int64_t max_s()
{
    // |mulhi32(M, T)| <= |T| / 4 + 1 for |M| <= 2^30
    int64_t s = 0;
    for (int k = 0; k < 8; k++)
        s += fold_abs_sum(k) * 32768 / 4 + 1;
    return s;
}
constexpr int64_t kMaxT = max_t(), kMaxS = max_s();
static_assert(kMaxT < (1ll << 31), "a folded window sum overflows 32 bits for some int16 input");
static_assert(kMaxS < (1ll << 31), "a subband sample overflows 32 bits for some int16 input");

EFX_SBC_HOST inline void build_tables(Tables* t)
{
    for (int k = 0; k < 8; k++)
        for (int j = 0; j < 5; j++) {
            t->tap[k][j] = fold_first(k) + 16 * j;
            t->w[k][j] = win_q16(t->tap[k][j]);
            const int second = fold_second(k);
            t->tap[k][5 + j] = second < 0 ? 0 : second + 16 * j;
            t->w[k][5 + j] = second < 0 ? 0 : fold_sign(k) * win_q16(second + 16 * j);
        }
    for (int sb = 0; sb < 8; sb++)
        for (int k = 0; k < 8; k++) {
            const double x = cos((sb + 0.5) * k * M_PI / 8) * 1073741824.0;
            t->m[sb][k] = (int32_t)floor(x + 0.5);
        }
}

EFX_SBC_HD inline int32_t mulhi32(int32_t a, int32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mulhi(a, b);
#else
    return (int32_t)(((int64_t)a * b) >> 32);
#endif
}
EFX_SBC_HD inline uint32_t umulhi32(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// T[k] of the block whose newest sample is *newest (X[n] = newest[-n], n = 0..79)
EFX_SBC_HD inline int32_t window_term(const int16_t* newest, int k, const Tables& t)
{
    int32_t acc = 0;
    EFX_SBC_UNROLL
    for (int j = 0; j < 10; j++)
        acc += t.w[k][j] * (int32_t)newest[-t.tap[k][j]];
    return acc;
}

// S[sb] (Q15 of the halved subband sample) from the block's eight T
EFX_SBC_HD inline int32_t matrix_term(const int32_t* T, int sb, const Tables& t)
{
    int32_t acc = 0;
    EFX_SBC_UNROLL
    for (int k = 0; k < 8; k++)
        acc += mulhi32(t.m[sb][k], T[k]);
    return acc;
}

EFX_SBC_HD inline uint32_t abs_s(int32_t s) { return s < 0 ? 0u - (uint32_t)s : (uint32_t)s; }

// The smallest scale factor with max |S| < 2^scale over the frame's blocks (max_abs in Q15); 15 when none fits
EFX_SBC_HD inline int scale_factor(uint32_t max_abs)
{
    int len = 0;  // bits of max_abs
    while (len < 32 && (max_abs >> len))
        len++;
    const int s = len - kFracS;
    return s < 0 ? 0 : (s > 15 ? 15 : s);
}

// Appendix B 12.6.3 as the decoder writes it (sbc_decoder.cpp:142-233), one channel, 8 subbands
EFX_SBC_HD inline void bit_allocation(int frequency, int allocation, int bitpool, const uint8_t* scale, int* bits)
{
    const int8_t offset8[4][8] = {{-2, 0, 0, 0, 0, 0, 0, 1}, {-3, 0, 0, 0, 0, 0, 1, 2}, {-4, 0, 0, 0, 0, 0, 1, 2}, {-4, 0, 0, 0, 0, 0, 1, 2}};
    int bitneed[8], max_bitneed = 0;
    for (int sb = 0; sb < 8; sb++) {
        const int s = scale[sb];
        int need;
        if (allocation)
            need = s;
        else if (s == 0)
            need = -5;
        else {
            need = s - offset8[frequency][sb];
            if (need > 0)
                need /= 2;
        }
        bitneed[sb] = need;
        if (need > max_bitneed)
            max_bitneed = need;
    }
    int bitcount = 0, slicecount = 0, bitslice = max_bitneed + 1;
    do {
        bitslice--;
        bitcount += slicecount;
        slicecount = 0;
        for (int sb = 0; sb < 8; sb++) {
            if (bitneed[sb] > bitslice + 1 && bitneed[sb] < bitslice + 16)
                slicecount++;
            else if (bitneed[sb] == bitslice + 1)
                slicecount += 2;
        }
    } while (bitcount + slicecount < bitpool);
    if (bitcount + slicecount == bitpool) {
        bitcount += slicecount;
        bitslice--;
    }
    for (int sb = 0; sb < 8; sb++) {
        int b = 0;
        if (bitneed[sb] >= bitslice + 2) {
            b = bitneed[sb] - bitslice;
            if (b > 16)
                b = 16;
        }
        bits[sb] = b;
    }
    for (int sb = 0; bitcount < bitpool && sb < 8; sb++) {
        if (bits[sb] >= 2 && bits[sb] < 16) {
            bits[sb]++;
            bitcount++;
        } else if (bitneed[sb] == bitslice + 1 && bitpool > bitcount + 1) {
            bits[sb] = 2;
            bitcount += 2;
        }
    }
    for (int sb = 0; bitcount < bitpool && sb < 8; sb++)
        if (bits[sb] < 16) {
            bits[sb]++;
            bitcount++;
        }
}

// q = floor((S + 2^scale)(2^bits - 1) / 2^(scale+1)) for the halved S, clamped to 0 .. 2^bits - 2; bits = 1..16
EFX_SBC_HD inline uint32_t quantise(int32_t s_q15, int scale, int bits)
{
    const int32_t lim = (int32_t)1 << (scale + kFracS);
    const int32_t c = s_q15 < -lim ? -lim : (s_q15 > lim - 1 ? lim - 1 : s_q15);
    const uint32_t u = (uint32_t)(c + lim);  // < 2^(scale + 16)
    const uint32_t levels = (1u << bits) - 1;
    const uint32_t q = umulhi32(u << (15 - scale), levels << 1);
    return q > levels - 1 ? levels - 1 : q;
}

// The standard's CRC-8 (x^8 + x^4 + x^3 + x^2 + 1, initial value 0x0F), a byte at a time
EFX_SBC_HD inline uint32_t crc8_byte(uint32_t crc, uint32_t byte)
{
    crc ^= byte;
    for (int i = 0; i < 8; i++)
        crc = (crc & 0x80) ? ((crc << 1) ^ 0x1D) & 0xFF : (crc << 1) & 0xFF;
    return crc;
}

EFX_SBC_HD inline uint32_t header_byte1(int frequency, int blocks, int mode, int allocation)
{
    return (uint32_t)(frequency << 6 | (blocks / 4 - 1) << 4 | mode << 2 | allocation << 1 | 1);
}

// The frame's first 4 + 4 channels bytes: 9C, the geometry, the bitpool, the CRC over bytes 1, 2 and the scale factors,
// then the scale factors, four bits each
EFX_SBC_HD inline void write_header(uint8_t* out, int frequency, int blocks, int mode, int allocation, int bitpool,
                                    const uint8_t (*scale)[8])
{
    const int channels = mode ? 2 : 1;
    out[0] = 0x9C;
    out[1] = (uint8_t)header_byte1(frequency, blocks, mode, allocation);
    out[2] = (uint8_t)bitpool;
    uint32_t crc = crc8_byte(crc8_byte(0x0F, out[1]), out[2]);
    for (int c = 0; c < channels; c++)
        for (int p = 0; p < 4; p++) {
            const uint8_t b = (uint8_t)(scale[c][2 * p] << 4 | scale[c][2 * p + 1]);
            out[4 + c * 4 + p] = b;
            crc = crc8_byte(crc, b);
        }
    out[3] = (uint8_t)crc;
}

EFX_SBC_HD inline uint32_t frame_bytes(int blocks, int channels, int bitpool)
{
    return (uint32_t)(4 + 4 * channels + (blocks * channels * bitpool + 7) / 8);
}

// Where sample n of channel c of a frame lies among the frame's samples_per_frame x channels PCM values
EFX_SBC_HD inline int pcm_index(int layout_interleaved, int channels, int samples_per_frame, int c, int n)
{
    return layout_interleaved ? n * channels + c : c * samples_per_frame + n;
}

}  // namespace sbcenc
}  // namespace efx
