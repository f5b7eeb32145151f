// enc_rate.h -- per-picture rate control of the MPEG-1 encoder (efx_encode_rc): the buffer model of include/efx.h, the
// activity measure of one macroblock row and the controller that turns buffer state, history and activity into one
// quantiser_scale per picture.
//
// Host + device, like enc_core.h: k_encode.hip runs exactly these functions and tests/enc_rate_model_main.cpp builds them
// with a plain C++ compiler.  Integer arithmetic only (64-bit where bits x 90000 needs it), so both make the same
// decisions bit for bit.  DESIGN.md ("Rate control") gives the reasoning behind the formula and its constants.
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

constexpr int64_t kRcTick = 3003;          // one picture period in 90 kHz ticks at the default picture rate (30000/1001 Hz)
constexpr int64_t kRcByte = 8 * 90000;     // one byte in buffer units (1 / 90000 bit)
constexpr int kRcActBias = 16384;          // activity that stands for what a picture costs before any coefficient
constexpr int kRcHorizonMax = 48;          // pictures the controller looks ahead, at most
constexpr int kRcFloorDiv = 8;             // the look-ahead keeps the predicted level above capacity / 8 ...
constexpr int kRcSlackNum = 9, kRcSlackDen = 8;  // ... with every predicted cost taken 9/8 of its estimate
constexpr int64_t kRcCpaMax = 0xFFFFF;     // bound of the history figure: keeps 48 predicted costs far inside 64 bits

// What a call fixes for every stream (efx_encode_rate, checked)
struct RateParams {
    int64_t cap;   // C = vbv_bits x 90000
    int64_t gain;  // G = bitrate x the ticks the picture lasts (enc_core.h: rate_pts_step; 3003 at the default rate)
    int qmin, qmax, q0;  // q0 = clamp(opts->qscale, qmin, qmax): the first picture of a fresh stream
};

// Per stream, carried across cont = 1 calls
struct RateState {
    int64_t level;     // F
    uint32_t cpa[2];   // bytes x qscale x 256 per unit of (activity + kRcActBias) of the last I ([0]) and P ([1]) picture
    uint32_t seen[2];  // ... whether there has been one
};

EFX_ENC_HD inline void rate_reset(RateState* r, const RateParams& p)
{
    r->level = p.cap;
    r->cpa[0] = r->cpa[1] = 0;
    r->seen[0] = r->seen[1] = 0;
}

// Activity of one macroblock from its 16 x 16 luma: the absolute deviation from its own mean (k_enc_rows' `dev`), and the
// SAD against the pels at the same place of the previous reconstruction (host form; k_enc_act computes the same sums
// with v_sad_u8 on packed words).
EFX_ENC_HD inline void mb_activity(const uint8_t* cur, const uint8_t* ref, int pitch, int* dev_out, int* sad_out)
{
    int sum = 0, dev = 0, sad = 0;
    for (int y = 0; y < 16; y++)
        for (int x = 0; x < 16; x++)
            sum += cur[y * pitch + x];
    const int mean = (sum + 128) >> 8;
    for (int y = 0; y < 16; y++)
        for (int x = 0; x < 16; x++) {
            const int d = (int)cur[y * pitch + x] - mean;
            dev += d < 0 ? -d : d;
            if (ref) {
                const int e = (int)cur[y * pitch + x] - (int)ref[y * pitch + x];
                sad += e < 0 ? -e : e;
            }
        }
    *dev_out = dev;
    *sad_out = sad;
}

// Predicted bytes x qscale of a picture of activity `act` and type index t (0 = I, 1 = P)
EFX_ENC_HD inline int64_t rate_complexity(const RateState& r, int t, uint32_t act)
{
    // a stream's first P picture has no P history: it is taken to cost what intra coding of its activity costs
    const uint32_t cpa = r.seen[t] ? r.cpa[t] : r.cpa[0];
    return ((int64_t)cpa * ((int64_t)act + kRcActBias)) >> 8;
}

// Does the predicted buffer level stay above the floor over the horizon when every picture is coded at q?
EFX_ENC_HD inline bool rate_fits(const RateParams& p, int64_t level, int q, int64_t x_now, int64_t x_i, int64_t x_p, int phase,
                                 int gop, int horizon)
{
    const int64_t floor_u = p.cap / kRcFloorDiv;
    const int64_t ci = (x_i / q + 188) * kRcByte / kRcSlackDen * kRcSlackNum;
    const int64_t cp = (x_p / q + 188) * kRcByte / kRcSlackDen * kRcSlackNum;
    const int64_t c0 = (x_now / q + 188) * kRcByte / kRcSlackDen * kRcSlackNum;
    int ph = phase;
    for (int k = 0; k < horizon; k++) {
        level -= k == 0 ? c0 : (ph == 0 ? ci : cp);
        if (level < floor_u)
            return false;
        level += p.gain;
        level = level > p.cap ? p.cap : level;
        ph = ph + 1 == gop ? 0 : ph + 1;
    }
    return true;
}

// The quantiser_scale of the picture about to be coded.  pictures = pictures of the stream so far, phase = pictures % gop
// (0: an I picture), act_i = the picture's summed `dev`, act_p = its summed min(dev, zero-vector SAD) (pictures > 0).
EFX_ENC_HD inline int rate_decide(const RateState& r, const RateParams& p, uint32_t pictures, int phase, int gop, uint32_t act_i,
                                  uint32_t act_p)
{
    if (p.qmin == p.qmax)
        return p.qmin;
    if (pictures == 0)
        return p.q0;
    if (r.level <= 0)
        return p.qmax;
    // the content the look-ahead assumes for the pictures to come is the content of this picture
    const int64_t x_i = rate_complexity(r, 0, act_i), x_p = rate_complexity(r, 1, act_p);
    const int64_t x_now = phase == 0 ? x_i : x_p;
    int horizon = 2 * gop + 1;
    horizon = horizon > kRcHorizonMax ? kRcHorizonMax : horizon;
    // the smallest q that fits: rate_fits is monotone in q (a larger q lowers every cost, min(C, .) keeps the order)
    int lo = p.qmin, hi = p.qmax;
    if (!rate_fits(p, r.level, hi, x_now, x_i, x_p, phase, gop, horizon))
        return hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rate_fits(p, r.level, mid, x_now, x_i, x_p, phase, gop, horizon))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// After a picture of `bytes` bytes was written at q: the buffer model of efx.h and the controller's history.  Returns
// whether the level went below zero (EFX_ENCODE_VBV).
EFX_ENC_HD inline bool rate_update(RateState* r, const RateParams& p, int phase, int q, uint32_t bytes, uint32_t act_i, uint32_t act_p)
{
    r->level -= kRcByte * (int64_t)bytes;
    const bool under = r->level < 0;
    r->level += p.gain;
    r->level = r->level > p.cap ? p.cap : r->level;
    const int t = phase == 0 ? 0 : 1;
    const int64_t act = (int64_t)(t == 0 ? act_i : act_p) + kRcActBias;
    int64_t cpa = ((int64_t)bytes * q * 256) / act;
    cpa = cpa > kRcCpaMax ? kRcCpaMax : cpa;
    // P pictures: the mean of the old and the new figure; an I picture replaces the last one (they are a GOP apart)
    r->cpa[t] = t == 1 && r->seen[1] ? (uint32_t)(((int64_t)r->cpa[1] + cpa + 1) >> 1) : (uint32_t)cpa;
    r->seen[t] = 1;
    return under;
}

}  // namespace enc
}  // namespace efx
