// enc_core.h -- the per-macroblock and per-slice arithmetic of the MPEG-1 encoder (k_encode.hip).
//
// Host + device: the kernels run exactly these functions, and tests/test_encode_model.py builds this header with a plain
// C++ compiler, encodes pictures on the host and decodes them with the test oracle.  Everything is integer arithmetic
// (the forward DCT too), so the host build and the kernels produce the same levels, the same bits and the same
// reconstruction.  The reconstruction is the decoder's (reference player.cpp:922-1236, restated by gen/efx_gen.cpp's
// reconstruct()): dequantisation, the one-coefficient shortcut with its unclamped intra DC, the integer IDCT and the
// clamp to 0..248.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mpeg1_codebook.h"

#if defined(__HIPCC__)
#define EFX_ENC_HD __host__ __device__
#else
#define EFX_ENC_HD
#endif

namespace efx {
namespace enc {

constexpr int kW = 352, kH = 192, kCW = 176, kCH = 96, kMbCols = 22, kMbRows = 12;
constexpr int kYBytes = kW * kH, kCBytes = kCW * kCH;  // I420: Y, then Cb, then Cr
constexpr int kPicBytes = kYBytes + 2 * kCBytes;       // 101 376
// Bits of one macroblock at most: address increment 11, type 6, two motion codes of 11 + 1, pattern 9, and six blocks
// of 64 escaped coefficients (28 bits each) and end_of_block.
// Adaptive quantisation (write_slice's mq) keeps inside this: the quant variants of the inter types cost 5 + 5 bits, 4
// over the 6, but the budget is only reached with all six blocks coded, where the pattern 63 is a 6-bit code against
// the 9, and an address increment inside a slice of 22 is at most 21, a 10-bit code against the 11.  Intra + quant is
// 6 + 5 bits, 5 over, and an intra macroblock's DC sizes and differentials take up to 4 x 15 + 2 x 16 = 92 bits, but it
// spends none of the 24 motion and 9 pattern bits and codes 63 AC coefficients per block, not 64: 6 x 28 bits to spare.
// tests/test_encode_aq_model.py derives both sums from the code book's lengths.
constexpr int kMbMaxBits = 11 + 6 + 24 + 9 + 6 * (64 * 28 + 2);
// Bytes of one slice at most: start code, quantiser_scale + extra_bit_slice, 22 macroblocks; rounded to 16
constexpr int kSliceCap = ((4 + (6 + kMbCols * kMbMaxBits + 7) / 8) + 15) / 16 * 16;
constexpr int kHdrCap = 32;     // sequence (12) + GOP (8) + picture header (5)
constexpr int kPesHdrBytes = 14;  // 00 00 01 E0, length 0, 80 80 05, PTS
constexpr int kMaxSearch = 15;
// Luma search window of one macroblock in LDS: 16 + 2 R + 2 rows / columns (the +1 a half-pel neighbour fetches on
// either side), row stride padded so that a 4-byte read at any column stays inside the row's two aligned words
constexpr int kWin = 16 + 2 * kMaxSearch + 2, kWinStride = 56;

// Code books in encoder form (built once per context from mpeg1_codebook.h) and the integer forward DCT basis
struct Tables {
    uint16_t dct_code[32][41];
    uint8_t dct_len[32][41];  // 0 = needs escape
    uint16_t mba_code[36];
    uint8_t mba_len[36];
    uint16_t cbp_code[64];
    uint8_t cbp_len[64];
    uint16_t mv_code[33];  // index = motion_code + 16
    uint8_t mv_len[33];
    uint16_t type_p_code[32];
    uint8_t type_p_len[32];
    uint8_t zz[64];       // scan position -> raster index
    uint8_t intra_q[64];  // default intra matrix, raster order
    uint8_t premul[64];   // the decoder's IDCT pre-multipliers (efx_gen.cpp Books::premul)
    int16_t cosv[8][8];   // round(4096 c(u) cos((2x + 1) u pi / 16)), c(0) = 1 / (2 sqrt 2), c(u) = 1 / 2
};

// One macroblock as the slice coder needs it (LDS / host)
struct Mb {
    int16_t lev[6][64];  // levels in scan order; intra: lev[b][0] = DC value 0..255
    int8_t h, v;         // half-pel forward vector (inter)
    uint8_t intra, cbp;
};

// ---------------------------------------------------------------------------------------
// picture geometry

// A half-pel luma vector (h, v) for macroblock (mbx, mby) keeps every fetch inside the picture: the 16 x 16 luma block
// (17 wide / high at a half-pel position) and the two 8 x 8 chroma blocks under the decoder's chroma rule (chroma
// position = luma half-pel position >> 1, gen/efx_gen.cpp predict_mb).
EFX_ENC_HD inline bool axis_ok(int mb, int d, int size, int csize)
{
    const int p = (mb << 5) + d;  // luma half-pels
    if (p < 0 || (p >> 1) + 16 + (p & 1) > size)
        return false;
    const int c = p >> 1;  // chroma half-pels
    return (c >> 1) + 8 + (c & 1) <= csize;
}
EFX_ENC_HD inline bool mv_ok(int mbx, int mby, int h, int v) { return axis_ok(mbx, h, kW, kCW) && axis_ok(mby, v, kH, kCH); }

// The decoder's half-pel prediction of one pixel (four cases)
EFX_ENC_HD inline int interp(const uint8_t* s, int pitch, int hx, int hy)
{
    if (!hx && !hy)
        return s[0];
    if (hx && !hy)
        return (s[0] + s[1] + 1) >> 1;
    if (!hx)
        return (s[0] + s[pitch] + 1) >> 1;
    return (s[0] + s[1] + s[pitch] + s[pitch + 1] + 2) >> 2;
}

// Plane, pitch and top-left of block b (0-3 luma, 4 Cb, 5 Cr) of macroblock (mbx, mby) in an I420 picture
EFX_ENC_HD inline const uint8_t* block_ptr(const uint8_t* pic, int b, int mbx, int mby, int* pitch)
{
    if (b < 4) {
        *pitch = kW;
        return pic + (mby * 16 + (b >> 1) * 8) * kW + mbx * 16 + (b & 1) * 8;
    }
    *pitch = kCW;
    return pic + kYBytes + (b - 4) * kCBytes + mby * 8 * kCW + mbx * 8;
}

// Prediction of block b from the reference picture for half-pel luma vector (h, v)
EFX_ENC_HD inline void predict_block(const uint8_t* ref, int b, int mbx, int mby, int h, int v, uint8_t* out)
{
    int px, py, pitch;
    const uint8_t* plane;
    if (b < 4) {
        px = (mbx << 5) + h + (b & 1) * 16;
        py = (mby << 5) + v + (b >> 1) * 16;
        plane = ref;
        pitch = kW;
    } else {
        px = ((mbx << 5) + h) >> 1;
        py = ((mby << 5) + v) >> 1;
        plane = ref + kYBytes + (b - 4) * kCBytes;
        pitch = kCW;
    }
    const uint8_t* s = plane + (py >> 1) * pitch + (px >> 1);
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++)
            out[y * 8 + x] = (uint8_t)interp(s + y * pitch + x, pitch, px & 1, py & 1);
}

// ---------------------------------------------------------------------------------------
// transform, quantisation, reconstruction

EFX_ENC_HD inline void idct_pass(int* b, int st, bool final)
{
    int i0 = b[0], i1 = b[st], i2 = b[2 * st], i3 = b[3 * st], i4 = b[4 * st], i5 = b[5 * st], i6 = b[6 * st], i7 = b[7 * st];
    int b3 = i2 + i6, b4 = i5 - i3, t1 = i1 + i7, t2 = i3 + i5, b6 = i1 - i7, b7 = t1 + t2;
    int x4 = ((b6 * 473 - b4 * 196 + 128) >> 8) - b7;
    int x0 = x4 - (((t1 - t2) * 362 + 128) >> 8);
    int x1 = i0 - i4;
    int x2 = (((i2 - i6) * 362 + 128) >> 8) - b3;
    int x3 = i0 + i4;
    int y3 = x1 + x2, y4 = x3 + b3, y5 = x1 - x2, y6 = x3 - b3;
    int y7 = -x0 - ((b4 * 473 + b6 * 196 + 128) >> 8);
    int o[8] = {b7 + y4, x4 + y3, y5 - x0, y6 - y7, y6 + y7, x0 + y5, y3 - x4, y4 - b7};
    for (int k = 0; k < 8; k++)
        b[k * st] = final ? (o[k] + 128) >> 8 : o[k];
}

EFX_ENC_HD inline int clamp248(int v) { return v < 0 ? 0 : (v > 248 ? 248 : v); }

// The decoder's reconstruction of one block from levels in scan order.  blk holds the prediction (inter) on entry and the
// reconstruction on return (when `commit`).  Returns false when a value handed to the decoder's clamp leaves -256..511.
EFX_ENC_HD inline bool reconstruct(const int* lev, bool intra, int q, const Tables& T, uint8_t* blk, bool commit)
{
    int coef[64];
    for (int i = 0; i < 64; i++)
        coef[i] = 0;
    int last = -1;
    if (intra) {
        coef[0] = lev[0] << 8;
        last = 0;
    }
    for (int n = intra ? 1 : 0; n < 64; n++) {
        int v = lev[n];
        if (!v)
            continue;
        const int zz = T.zz[n];
        v <<= 1;
        if (!intra)
            v += v < 0 ? -1 : 1;
        v = (v * q * (intra ? T.intra_q[zz] : 16)) / 16;
        if ((v & 1) == 0)
            v -= v > 0 ? 1 : -1;
        v = v > 2047 ? 2047 : (v < -2048 ? -2048 : v);
        coef[zz] = v * T.premul[zz];
        last = n;
    }
    if (last < 0)
        return true;
    if (last == 0) {  // the decoder's shortcut: exactly one coefficient, at scan position 0
        const int dc = coef[0] >> 8;
        if (commit)
            for (int i = 0; i < 64; i++)
                blk[i] = intra ? (uint8_t)dc : (uint8_t)clamp248(dc + blk[i]);
        return true;
    }
    for (int c = 0; c < 8; c++)
        idct_pass(coef + c, 8, false);
    for (int r = 0; r < 8; r++)
        idct_pass(coef + r * 8, 1, true);
    bool in_range = true;
    for (int i = 0; i < 64; i++) {
        const int v = coef[i] + (intra ? 0 : blk[i]);
        in_range &= v >= -256 && v <= 511;
        if (commit)
            blk[i] = (uint8_t)clamp248(v);
    }
    return in_range;
}

// Integer forward DCT: out = round(8 x orthonormal 2-D DCT of in), raster order
EFX_ENC_HD inline void fdct8(const int* in, int* out, const Tables& T)
{
    int tmp[64];
    for (int y = 0; y < 8; y++)
        for (int u = 0; u < 8; u++) {
            int s = 0;
            for (int x = 0; x < 8; x++)
                s += in[y * 8 + x] * T.cosv[u][x];
            tmp[y * 8 + u] = (s + 256) >> 9;  // 8 x the row transform
        }
    for (int v = 0; v < 8; v++)
        for (int u = 0; u < 8; u++) {
            int s = 0;
            for (int y = 0; y < 8; y++)
                s += tmp[y * 8 + u] * T.cosv[v][y];
            out[v * 8 + u] = (s + 2048) >> 12;
        }
}

// Quantise the coefficients F (raster order, fdct8's units) into levels in scan order: intra DC the rounded mean 0..255,
// intra AC rounded, non-intra truncated (a dead zone), |level| <= 255.  Returns whether a level other than the intra DC
// is non-zero.
EFX_ENC_HD inline bool quantise(const int* F, bool intra, int q, const Tables& T, int* lev)
{
    bool any = false;
    for (int n = 0; n < 64; n++) {
        const int zz = T.zz[n];
        int l;
        if (intra && n == 0) {
            l = (F[0] + 32) >> 6;  // the mean, 0 .. 255
            l = l < 0 ? 0 : (l > 255 ? 255 : l);
        } else {
            const int d = q * (intra ? T.intra_q[zz] : 16);
            const int a = F[zz] < 0 ? -F[zz] : F[zz];
            const int m = intra ? (a + (d >> 1)) / d : a / d;
            l = F[zz] < 0 ? -m : m;
            l = l > 255 ? 255 : (l < -255 ? -255 : l);
        }
        lev[n] = l;
        any |= l != 0 && !(intra && n == 0);
    }
    return any;
}

// Code one block: the source block (8 x 8) minus the prediction in blk (inter), transformed and quantised, then the
// levels halved until the decoder's clamp stays inside its domain; blk gets the reconstruction and lev_out the levels.
// Returns 1 when the block has a level to code (intra: 1).
EFX_ENC_HD inline int code_block(const uint8_t* src, int pitch, bool intra, int q, const Tables& T, uint8_t* blk, int16_t* lev_out)
{
    int pix[64], F[64], lev[64];
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++)
            pix[y * 8 + x] = (int)src[y * pitch + x] - (intra ? 0 : (int)blk[y * 8 + x]);
    fdct8(pix, F, T);
    bool any = quantise(F, intra, q, T, lev);
    while (!reconstruct(lev, intra, q, T, blk, false)) {
        any = false;
        for (int n = intra ? 1 : 0; n < 64; n++) {
            lev[n] /= 2;
            any |= lev[n] != 0;
        }
    }
    if (!intra && !any)
        for (int n = 0; n < 64; n++)
            lev[n] = 0;
    reconstruct(lev, intra, q, T, blk, true);
    for (int n = 0; n < 64; n++)
        lev_out[n] = (int16_t)lev[n];
    return intra || any;
}

// Mode decision of a P macroblock: intra when the luma's deviation from its own mean undercuts the best inter SAD by
// more than 512 (H.263 TMN's rule with its 500 rounded up)
EFX_ENC_HD inline bool choose_intra(int intra_cost, int inter_sad) { return intra_cost + 512 < inter_sad; }
// Search cost of an integer candidate: its SAD, the zero vector's less 128 (skipped macroblocks are cheap)
EFX_ENC_HD inline int search_cost(int sad, int dx, int dy) { return (dx | dy) ? sad : (sad > 128 ? sad - 128 : 0); }
// Ordering key of an integer candidate: cost, then |dx| + |dy|, then raster index in the window -- unique per candidate
EFX_ENC_HD inline uint32_t search_key(int cost, int dx, int dy, int idx)
{
    const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    return ((uint32_t)cost << 15) | ((uint32_t)dist << 10) | (uint32_t)idx;
}

// ---------------------------------------------------------------------------------------
// bits

struct Bits {
    uint8_t* out;
    uint32_t n;  // bytes written
    int nb;      // bits waiting in acc
    uint64_t acc;
    EFX_ENC_HD void put(uint32_t v, int len)
    {
        acc = (acc << len) | (v & (uint32_t)((1ull << len) - 1));
        nb += len;
        while (nb >= 8) {
            nb -= 8;
            out[n++] = (uint8_t)(acc >> nb);
        }
    }
    EFX_ENC_HD void align()
    {
        if (nb)
            put(0, 8 - nb);
    }
    EFX_ENC_HD void start_code(int code)
    {
        align();
        put(0, 16);
        put(1, 8);
        put((uint32_t)code, 8);
    }
};

// The eight picture rates MPEG-1 codes (picture_rate 1 .. 8): one picture period is kRateTickNum / 2^kRateTickShift ticks
// of 90 kHz (24000/1001 Hz: 15015/4; 60000/1001 Hz: 3003/2), and the GOP time code counts kRateNominal pictures a second
constexpr int kRateDefault = 4;  // 30000/1001 Hz
EFX_ENC_HD inline bool rate_code_ok(int code) { return code >= 1 && code <= 8; }
EFX_ENC_HD inline int64_t rate_tick_num(int code)
{
    const int16_t num[9] = {0, 15015, 3750, 3600, 3003, 3000, 1800, 3003, 1500};
    return num[code];
}
EFX_ENC_HD inline int rate_tick_shift(int code) { return code == 1 ? 2 : (code == 7 ? 1 : 0); }
EFX_ENC_HD inline uint32_t rate_nominal(int code)
{
    const uint8_t f[9] = {0, 24, 24, 25, 30, 30, 50, 60, 60};
    return f[code];
}
// 90 kHz ticks from picture 0 to picture k: floor(k x period), no accumulated rounding (k <= 2^32)
EFX_ENC_HD inline int64_t rate_pts_offset(int code, int64_t k) { return (k * rate_tick_num(code)) >> rate_tick_shift(code); }
// ... and from picture k to picture k + 1: the period, or one of the two steps around it (codes 1 and 7)
EFX_ENC_HD inline int64_t rate_pts_step(int code, int64_t k) { return rate_pts_offset(code, k + 1) - rate_pts_offset(code, k); }

// Sequence header (352 x 192, square pels, picture_rate `rate_code`, default matrices) + GOP header (closed, time code of
// picture_number at the code's nominal rate, drop_frame 0) when `seq`, then the picture header: temporal_reference, type
// (1 = I, 2 = P), vbv_delay 0xFFFF, full_pel_forward_vector 0 and forward_f_code for P.  Returns the bytes written (at
// most kHdrCap).
EFX_ENC_HD inline uint32_t write_headers(uint8_t* out, bool seq, uint32_t picture_number, int tref, int type, int f_code,
                                         int rate_code = kRateDefault)
{
    Bits bw{out, 0, 0, 0};
    if (seq) {
        const uint32_t F = rate_nominal(rate_code);
        bw.start_code(0xB3);
        bw.put(kW, 12);
        bw.put(kH, 12);
        bw.put(1, 4);
        bw.put((uint32_t)rate_code, 4);
        bw.put(3750, 18);
        bw.put(1, 1);
        bw.put(20, 10);
        bw.put(0, 1);
        bw.put(0, 1);
        bw.put(0, 1);
        bw.start_code(0xB8);
        const uint32_t pictures = picture_number % F, seconds = (picture_number / F) % 60, minutes = (picture_number / (60 * F)) % 60,
                       hours = (picture_number / (3600 * F)) % 24;
        bw.put((hours << 19) | (minutes << 13) | (1u << 12) | (seconds << 6) | pictures, 25);
        bw.put(1, 1);  // closed_gop
        bw.put(0, 1);  // broken_link
        bw.put(0, 5);
    }
    bw.start_code(0x00);
    bw.put((uint32_t)tref & 1023, 10);
    bw.put((uint32_t)type, 3);
    bw.put(0xFFFF, 16);
    if (type == 2) {
        bw.put(0, 1);
        bw.put((uint32_t)f_code, 3);
    }
    bw.put(0, 1);  // extra_bit_picture
    bw.align();
    return bw.n;
}

EFX_ENC_HD inline void put_dc(Bits& bw, int diff, bool luma)
{
    int a = diff < 0 ? -diff : diff, size = 0;
    while (a >> size)
        size++;
    const uint8_t ycode[9] = {4, 0, 1, 5, 6, 14, 30, 62, 126}, ylen[9] = {3, 2, 2, 3, 3, 4, 5, 6, 7};
    const uint8_t ccode[9] = {0, 1, 2, 6, 14, 30, 62, 126, 254}, clen[9] = {2, 2, 2, 3, 4, 5, 6, 7, 8};
    if (luma)
        bw.put(ycode[size], ylen[size]);
    else
        bw.put(ccode[size], clen[size]);
    if (size)
        bw.put((uint32_t)(diff > 0 ? diff : diff + (1 << size) - 1), size);
}

EFX_ENC_HD inline void put_coefs(Bits& bw, const int16_t* lev, bool intra, const Tables& T)
{
    int run = 0;
    bool first = !intra;
    for (int n = intra ? 1 : 0; n < 64; n++) {
        const int v = lev[n];
        if (!v) {
            run++;
            continue;
        }
        const int a = v < 0 ? -v : v;
        if (run == 0 && a == 1) {
            if (first)
                bw.put(2 | (v < 0), 2);  // "1s"
            else
                bw.put(6 | (v < 0), 3);  // "11s"
        } else if (a <= 40 && run < 32 && T.dct_len[run][a]) {
            bw.put(T.dct_code[run][a], T.dct_len[run][a]);
            bw.put(v < 0, 1);
        } else {  // escape: 6-bit run, 8-bit level for -127..127, else 00 xx / 80 xx
            bw.put(1, 6);
            bw.put((uint32_t)run, 6);
            if (a < 128)
                bw.put((uint32_t)v & 0xFF, 8);
            else if (v > 0) {
                bw.put(0, 8);
                bw.put((uint32_t)v, 8);
            } else {
                bw.put(128, 8);
                bw.put((uint32_t)(v + 256), 8);
            }
        }
        first = false;
        run = 0;
    }
    bw.put(2, 2);  // end_of_block
}

EFX_ENC_HD inline void put_motion(Bits& bw, int delta, int f_code, const Tables& T)  // delta wrapped into the f_code range
{
    const int r = f_code - 1;
    if (delta == 0 || r == 0) {
        bw.put(T.mv_code[delta + 16], T.mv_len[delta + 16]);
        return;
    }
    const int a = (delta < 0 ? -delta : delta) - 1;
    int code = (a >> r) + 1;
    if (delta < 0)
        code = -code;
    bw.put(T.mv_code[code + 16], T.mv_len[code + 16]);
    bw.put((uint32_t)(a & ((1 << r) - 1)), r);
}

// One slice = one macroblock row: start code row + 1, quantiser_scale q, then the 22 macroblocks.  A P macroblock with
// vector (0, 0) and no coded block is skipped unless it is the first or last of the slice; the DC and vector predictors
// reset as the decoder resets them.  Returns the bytes written (byte-aligned, at most kSliceCap).
//
// mq (adaptive quantisation, enc_aq.h; nullptr: every macroblock at q): the quantiser of each of the 22 macroblocks.  The
// slice header carries mq[0]; a coded macroblock (intra, or with a pattern) whose quantiser is not the current one is
// written with the quant variant of its type and five bits of its quantiser, which becomes the current one.  A
// macroblock without coded blocks never changes it.  (kMq = whether mq is given: the coder without it is a function of
// its own, the one it was before there was an mq.)
template <bool kMq>
EFX_ENC_HD inline uint32_t write_slice_t(uint8_t* out, int row, int q, int type, int f_code, const Mb* mbs, const Tables& T,
                                         const uint8_t* mq)
{
    Bits bw{out, 0, 0, 0};
    bw.start_code(row + 1);
    int cur_q = kMq ? mq[0] : q;
    bw.put((uint32_t)cur_q, 5);
    bw.put(0, 1);  // extra_bit_slice
    int dc_pred[3] = {128, 128, 128};
    int pmv_h = 0, pmv_v = 0;
    int pending_skip = 0;
    const int range = 16 << (f_code - 1);
    for (int mbx = 0; mbx < kMbCols; mbx++) {
        const Mb& m = mbs[mbx];
        const bool inter = type == 2 && !m.intra;
        if (inter && m.h == 0 && m.v == 0 && m.cbp == 0 && mbx > 0 && mbx < kMbCols - 1) {
            pending_skip++;
            continue;
        }
        const int inc = pending_skip + 1;
        if (pending_skip) {
            dc_pred[0] = dc_pred[1] = dc_pred[2] = 128;
            pmv_h = pmv_v = 0;
            pending_skip = 0;
        }
        bw.put(T.mba_code[inc], T.mba_len[inc]);
        const bool quant = kMq && (!inter || m.cbp) && mq[mbx] != cur_q;
        if (quant)
            cur_q = mq[mbx];
        if (!inter) {
            if (type == 1)
                bw.put(1, quant ? 2 : 1);
            else
                bw.put(T.type_p_code[quant ? 17 : 1], T.type_p_len[quant ? 17 : 1]);
            if (quant)
                bw.put((uint32_t)cur_q, 5);
            pmv_h = pmv_v = 0;
            for (int b = 0; b < 6; b++) {
                const int comp = b < 4 ? 0 : b - 3;
                put_dc(bw, m.lev[b][0] - dc_pred[comp], b < 4);
                dc_pred[comp] = m.lev[b][0];
                put_coefs(bw, m.lev[b], true, T);
            }
            continue;
        }
        dc_pred[0] = dc_pred[1] = dc_pred[2] = 128;
        const bool has_mv = m.h != 0 || m.v != 0 || m.cbp == 0;  // "no motion compensation, not coded" does not exist
        const int t = (m.cbp ? 2 : 0) | (has_mv ? 8 : 0) | (quant ? 16 : 0);
        bw.put(T.type_p_code[t], T.type_p_len[t]);
        if (quant)
            bw.put((uint32_t)cur_q, 5);
        if (has_mv) {
            int dh = m.h - pmv_h, dv = m.v - pmv_v;
            dh = dh < -range ? dh + 2 * range : (dh > range - 1 ? dh - 2 * range : dh);
            dv = dv < -range ? dv + 2 * range : (dv > range - 1 ? dv - 2 * range : dv);
            put_motion(bw, dh, f_code, T);
            put_motion(bw, dv, f_code, T);
            pmv_h = m.h;
            pmv_v = m.v;
        } else
            pmv_h = pmv_v = 0;
        if (m.cbp) {
            bw.put(T.cbp_code[m.cbp], T.cbp_len[m.cbp]);
            for (int b = 0; b < 6; b++)
                if (m.cbp & (0x20 >> b))
                    put_coefs(bw, m.lev[b], false, T);
        }
    }
    bw.align();
    return bw.n;
}
EFX_ENC_HD inline uint32_t write_slice(uint8_t* out, int row, int q, int type, int f_code, const Mb* mbs, const Tables& T,
                                       const uint8_t* mq = nullptr)
{
    return mq ? write_slice_t<true>(out, row, q, type, f_code, mbs, T, mq) : write_slice_t<false>(out, row, q, type, f_code, mbs, T, nullptr);
}

// ---------------------------------------------------------------------------------------
// transport stream: PID 0x100, one PES (stream id E0, PTS only) per picture, 188-byte packets, the last packet of a
// PES padded with adaptation-field stuffing (gen/efx_gen.cpp ts_wrap)

EFX_ENC_HD inline uint32_t ts_packets(uint32_t pes_len) { return (pes_len + 183) / 184; }

EFX_ENC_HD inline uint8_t pes_header_byte(int i, int64_t pts)
{
    switch (i) {
    case 0: case 1: case 4: case 5: return 0;
    case 2: return 1;
    case 3: return 0xE0;
    case 6: case 7: return 0x80;
    case 8: return 5;
    case 9: return (uint8_t)(0x21 | ((pts >> 29) & 0x0E));
    case 10: return (uint8_t)(pts >> 22);
    case 11: return (uint8_t)(0x01 | ((pts >> 14) & 0xFE));
    case 12: return (uint8_t)(pts >> 7);
    default: return (uint8_t)(0x01 | ((pts << 1) & 0xFE));
    }
}

// Byte o of the packets that carry one PES of pes_len bytes, the first packet with continuity counter cc0: either a
// packet header / stuffing byte (returned, *pes_pos = -1) or PES byte *pes_pos.
EFX_ENC_HD inline uint8_t ts_byte(uint32_t o, uint32_t pes_len, uint32_t cc0, int64_t* pes_pos)
{
    const uint32_t pkt = o / 188, j = o % 188, npk = ts_packets(pes_len);
    const uint32_t left = pes_len - pkt * 184;
    const bool last_short = pkt == npk - 1 && left < 184;
    *pes_pos = -1;
    if (j == 0)
        return 0x47;
    if (j == 1)
        return (uint8_t)((pkt == 0 ? 0x40 : 0) | 0x01);
    if (j == 2)
        return 0x00;
    if (j == 3)
        return (uint8_t)((last_short ? 0x30 : 0x10) | ((cc0 + pkt) & 15));
    uint32_t k = j - 4;
    if (last_short) {
        const uint32_t stuff = 184 - left;  // adaptation_field_length byte + flags + 0xFF fill
        if (k == 0)
            return (uint8_t)(stuff - 1);
        if (k == 1 && stuff > 1)
            return 0x00;
        if (k < stuff)
            return 0xFF;
        k -= stuff;
    }
    *pes_pos = (int64_t)pkt * 184 + k;
    return 0;
}

#if defined(__HIPCC__)
#define EFX_ENC_HOST __host__
#else
#define EFX_ENC_HOST
#endif
// The tables above from the code books of mpeg1_codebook.h (host; once per context, and by the host build of the tests)
EFX_ENC_HOST inline void build_tables(Tables* t)
{
    *t = Tables{};
    for (auto& c : kMbaCodes) {
        t->mba_code[c.value] = c.code;
        t->mba_len[c.value] = c.len;
    }
    for (auto& c : kCbpCodes) {
        t->cbp_code[c.value] = c.code;
        t->cbp_len[c.value] = c.len;
    }
    for (auto& c : kMotionCodes) {
        t->mv_code[c.value + 16] = c.code;
        t->mv_len[c.value + 16] = c.len;
    }
    for (auto& c : kTypePCodes) {
        t->type_p_code[c.value] = c.code;
        t->type_p_len[c.value] = c.len;
    }
    for (auto& c : kDctCodes) {
        t->dct_code[c.run][c.level] = c.code;
        t->dct_len[c.run][c.level] = c.len;
    }
    double s[8];
    s[0] = 1.0;
    for (int k = 1; k < 8; k++)
        s[k] = sqrt(2.0) * cos(k * M_PI / 16);
    for (int i = 0; i < 64; i++) {
        t->zz[i] = kZigZag[i];
        t->intra_q[i] = kDefaultIntraQ[i];
        t->premul[i] = (uint8_t)floor(32.0 * s[i >> 3] * s[i & 7] + 0.5);
    }
    for (int u = 0; u < 8; u++)
        for (int x = 0; x < 8; x++)
            t->cosv[u][x] = (int16_t)lround(4096.0 * cos((2 * x + 1) * u * M_PI / 16) * (u ? 0.5 : 0.5 / sqrt(2.0)));
}

}  // namespace enc
}  // namespace efx
