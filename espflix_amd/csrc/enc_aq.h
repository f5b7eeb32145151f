// enc_aq.h -- adaptive quantisation of the MPEG-1 encoder (efx_encode_set_adaptive_quant): the spatial activity of one
// macroblock of the source picture, the picture's average, and the rule that turns the picture's quantiser and those two
// into the macroblock's own quantiser_scale.  Test Model 5's spatial activity and normalisation, stated in integers.
//
// Host + device, like enc_core.h, enc_rate.h and enc_cut.h: k_encode.hip (k_enc_aq, k_enc_rows) runs exactly these
// functions and tests/enc_aq_model_main.cpp builds them with a plain C++ compiler.  Integer arithmetic only, and the
// picture's sum is a sum of per-macroblock values, so the order of any reduction does not show in the result.
// include/efx.h ("adaptive quantisation") defines the rule; DESIGN.md gives the reasoning behind it.
#pragma once
#include <stdint.h>

#ifndef EFX_ENC_HD
#if defined(__HIPCC__)
#define EFX_ENC_HD __host__ __device__
#else
#define EFX_ENC_HD
#endif
#endif

namespace efx {
namespace enc {

constexpr int kAqMbs = 22 * 12;      // macroblocks of a picture
constexpr int kAqMaxStrength = 256;  // TM5's factor (2 a + avg) / (a + 2 avg)

// What a call fixes for every stream (efx_adaptive_quant, checked): strength 0 = off
struct AqParams {
    int strength;  // 0, or 1 .. 256
};

// One 8 x 8 luma block: the deviation of its pels from their rounded mean, 0 .. 8160
EFX_ENC_HD inline uint32_t aq_block_dev(const uint8_t* p, int pitch)
{
    int sum = 0;
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++)
            sum += p[y * pitch + x];
    const int m = (sum + 32) >> 6;
    uint32_t d = 0;
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++) {
            const int e = (int)p[y * pitch + x] - m;
            d += (uint32_t)(e < 0 ? -e : e);
        }
    return d;
}

// One macroblock (host form; k_enc_aq computes the same sums with v_sad_u8 on packed words): 1 + the smallest deviation
// of its four luma blocks, 1 .. 8161
EFX_ENC_HD inline uint32_t aq_mb_activity(const uint8_t* luma, int pitch)
{
    uint32_t best = 0xFFFFFFFFu;
    for (int b = 0; b < 4; b++) {
        const uint32_t d = aq_block_dev(luma + (b >> 1) * 8 * pitch + (b & 1) * 8, pitch);
        best = d < best ? d : best;
    }
    return 1 + best;
}

// The picture's average of its 264 activities, rounded
EFX_ENC_HD inline uint32_t aq_average(uint32_t sum) { return (sum + kAqMbs / 2) / kAqMbs; }

// The macroblock's quantiser: the picture's q scaled by ((256 + s) a + 256 avg) / (256 a + (256 + s) avg), rounded, kept
// in lo .. hi.  q num < 2^31: q <= 31, num <= 768 x 8161.  a == avg gives q.
EFX_ENC_HD inline int aq_mb_quant(int q, int strength, uint32_t a, uint32_t avg, int lo, int hi)
{
    const uint32_t num = (256u + (uint32_t)strength) * a + 256u * avg;
    const uint32_t den = 256u * a + (256u + (uint32_t)strength) * avg;
    const int mq = (int)(((uint32_t)q * num + (den >> 1)) / den);
    return mq < lo ? lo : (mq > hi ? hi : mq);
}

}  // namespace enc
}  // namespace efx
