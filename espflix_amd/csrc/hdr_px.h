// hdr_px.h -- arithmetic of the import's HDR stage (k_import.hip, the _h kernels): an HDR10 source (PQ transfer, BT.2020
// or BT.709 primaries, any matrix colour_px.h knows) tone-mapped to the BT.601 studio swing SDR picture MPEG-1 carries.
// The stage reads the import at 10 bits (vround10: the vertical accumulators rounded to 0 .. 1020 instead of 0 .. 255; the
// 10-bit video scale: studio luma 64 .. 940, chroma 512 +- 448, full range 0 .. 1020 around 512) and rounds to 8 bits once,
// after the tone map.
//
// An item is a chroma site and its 2 x 2 luma samples; all four pixels use the site's Cb10, Cr10 (nearest siting, as
// colour::convert_block).  Per pixel:
//   1. matrix     (Y10, Cb10, Cr10) -> non-linear R', G', B' in steps of 2^-24, clamped to [0, 1]: Q14 coefficients that
//                 carry the scale 2^24 / 876 (896, 1020), from rational arithmetic (kTable; tests/hdr_model.py recomputes
//                 it); 64-bit sums.  (One step of PQ code is 11 steps of relative light, and the gamut matrix takes the
//                 difference of channels: beside a channel at 1, a channel near 0 needs its neighbours' light to 3 x 10^-6,
//                 or the 2.4 gamma shows it.  Steps of 2^-15, which 32-bit sums allow, are 50 times too coarse)
//   2. first table, per channel: PQ code -> display light relative to 100 nits in steps of 2^-24 -- the ST 2084 EOTF behind
//                 the BT.2390 EETF for the setting's peak, kPqEntries entries at E' = i / (kPqEntries - 1), read with the
//                 bits below the index as a linear interpolation
//   3. gamut      the linear BT.2020 -> BT.709 matrix of BT.2087 (identity for BT.709 primaries) in steps of 2^-28, every row
//                 summing to exactly 2^28 so that grey stays grey; 64-bit products; clamped to [0, 1].  (Q14 coefficients
//                 are too coarse here: beside a channel at 1 their rounding moves a channel near 0 by 2 x 10^-5 of linear
//                 light, which the 2.4 gamma turns into three output codes)
//   4. second table: inverse BT.1886, E' = L^(1 / 2.4) in steps of 2^-15, addressed by the position of the leading bit and
//                 the next 6 bits (values below 128 address themselves), the bits below interpolate linearly
//   5. luma       BT.601 studio Y' of the SDR R', G', B', rounded once
// and Cb', Cr' from the sums of the four pixels' R', G', B' (the box is MPEG-1's centred chroma site), rounded once.
// The tables depend on the peak; the host builds them in double (efx_tables.cpp: build_import_hdr_tables) and the device
// reads them: there is no pow() here.
//
// Host + device, exact integers: the kernels run exactly these functions, tests/test_hdr_model.py builds this header with a
// plain C++ compiler and checks it against the NumPy model (tests/hdr_model.py) and a float64 yardstick, and
// tests/hdr_model_main.cpp performs whole HDR imports with them on the host.
#pragma once
#include <stdint.h>

#include "colour_px.h"
#include "import_px.h"

namespace efx {
namespace hdr {

constexpr int kTransferPq = 16;                    // H.273 transfer_characteristics: SMPTE ST 2084
constexpr int kPeakMin = 200, kPeakMax = 10000, kPeakDefault = 1000;
constexpr int kPosBits = 24, kPosOne = 1 << kPosBits;  // the source's non-linear R', G', B': steps of 2^-24
constexpr int kEBits = 15, kEOne = 1 << kEBits;    // the SDR non-linear R', G', B': steps of 2^-15
constexpr int kLinBits = 24, kLinOne = 1 << kLinBits;  // linear light: steps of 2^-24 (near black one step of a 16-bit scale
                                                       // is almost 3 output codes through the 2.4 gamma)
constexpr int kPqBits = 11;                        // the first table's index
constexpr int kPqFrac = kPosBits - kPqBits;        // bits of R' below it
constexpr int kPqEntries = (1 << kPqBits) + 1;
constexpr int kGamMant = 6;                        // bits behind the leading bit that address the second table
constexpr int kGamEntries = (kLinBits - kGamMant) * (1 << kGamMant) + (1 << kGamMant) + 1;  // 1217: the last is L = 1
constexpr int kPqSlots = kPqEntries + 3, kGamSlots = 1224;  // the arrays padded to multiples of 16 bytes

// Q14 coefficients of the matrix: R' = qy (Y10 - y0) + qrv (Cr10 - 512), G' = qy (Y10 - y0) + qgu (Cb10 - 512) + qgv (Cr10
// - 512), B' = qy (Y10 - y0) + qbu (Cb10 - 512), each q = round(2^14 x 2^24 x exact): 1 / 876 and 2 (1 - Kr) / 896 ...
// (studio), 1 / 1020 and 2 (1 - Kr) / 1020 ... (full)
struct Entry {
    int code;         // H.273 matrix_coefficients
    int32_t q[2][5];  // [range][qy, qrv, qgu, qgv, qbu]
};
constexpr Entry kTable[] = {
    {1, {{313787565, 483122464, -57467973, -143612746, 569267237}, {269488144, 424389929, -50481671, -126153942, 500062200}}},
    {4, {{313787565, 429496730, -101810484, -218388168, 546074413}, {269488144, 377283402, -89433523, -191839018, 479688896}}},
    {5, {{313787565, 430110296, -105575292, -219085142, 543620146}, {269488144, 377822378, -92740649, -192451262, 477532991}}},
    {6, {{313787565, 430110296, -105575292, -219085142, 543620146}, {269488144, 377822378, -92740649, -192451262, 477532991}}},
    {7, {{313787565, 483490604, -69523853, -146219698, 560186449}, {269488144, 424713315, -61071934, -128443970, 492085351}}},
    {9, {{313787565, 452382770, -50482164, -175281642, 577182248}, {269488144, 397387217, -44345117, -153972894, 507014994}}},
};
// gamut matrices in steps of 2^-28, row major: inverse(RGB -> XYZ of BT.709) x (RGB -> XYZ of the source's primaries), white
// D65, from rational arithmetic; what a row's rounded entries miss of 2^28 is added to its diagonal entry
constexpr int kGamutBits = 28;
constexpr int32_t kGamutOne = 1 << kGamutBits;
constexpr int32_t kGamut2020[9] = {445734659, -157743717, -19555486, -33433763, 304110500, -2241281, -4872308, -26998942, 300306706};
constexpr int32_t kGamut709[9] = {kGamutOne, 0, 0, 0, kGamutOne, 0, 0, 0, kGamutOne};
// BT.601 studio swing from R', G', B': 219 x (0.299, 0.587, 0.114) in steps of 2^-8, 224 x the Cb and Cr rows in steps of
// 2^-7
constexpr int32_t kLuma[3] = {16763, 32910, 6391};
constexpr int32_t kCb[3] = {-4838, -9498, 14336}, kCr[3] = {14336, -12005, -2331};

constexpr int64_t cabs64(int64_t v) { return v < 0 ? -v : v; }
constexpr bool rows_sum_to_one(const int32_t g[9])
{
    return g[0] + g[1] + g[2] == kGamutOne && g[3] + g[4] + g[5] == kGamutOne && g[6] + g[7] + g[8] == kGamutOne;
}
// the matrix sum of the widest samples (|Y10 - y0| <= 1020, |C10 - 512| <= 512) stays below 2^41 for every entry: 64-bit
// sums of 32-bit factors
constexpr bool matrix_fits()
{
    for (const Entry& e : kTable)
        for (int r = 0; r < 2; r++) {
            const int64_t y = cabs64(e.q[r][0]) * 1020 + 8192, top = (int64_t)1 << 41;
            if (y + cabs64(e.q[r][1]) * 512 >= top || y + (cabs64(e.q[r][2]) + cabs64(e.q[r][3])) * 512 >= top || y + cabs64(e.q[r][4]) * 512 >= top)
                return false;
        }
    return true;
}
static_assert(matrix_fits(), "the matrix stage is 64-bit arithmetic with room");
// first table: consecutive entries differ by less than 2^18 (d ln L / d E' < 14 for the PQ EOTF, so a step is below
// 14 / 2^kPqBits x 2^24; build_import_hdr_tables checks it, and that the table never falls)
constexpr uint32_t kPqMaxStep = 1u << 18;
static_assert((14u << kLinBits >> kPqBits) < kPqMaxStep, "the bound of a step of the first table");
static_assert((uint64_t)kPqMaxStep * ((1u << kPqFrac) - 1) + (1u << (kPqFrac - 1)) < ((uint64_t)1 << 32),
              "the first table's interpolation is unsigned 32-bit arithmetic");
static_assert(rows_sum_to_one(kGamut2020) && rows_sum_to_one(kGamut709), "grey stays grey");
static_assert(kGamEntries == 1217 && kPqSlots >= kPqEntries && kPqSlots % 4 == 0 && kGamSlots >= kGamEntries && kGamSlots % 8 == 0, "table sizes");
static_assert(((int64_t)445734659 + 157743717 + 19555486) * kLinOne + (kGamutOne >> 1) < ((int64_t)1 << 54), "the gamut sum is 64-bit arithmetic with room");
static_assert((int64_t)(kLuma[0] + kLuma[1] + kLuma[2]) * kEOne + (1 << 22) < INT32_MAX && kLuma[0] + kLuma[1] + kLuma[2] == 219 * 256,
              "luma is 32-bit arithmetic, white is 235");
static_assert((int64_t)14336 * 4 * kEOne + (1 << 23) < INT32_MAX && kCb[0] + kCb[1] + kCb[2] == 0 && kCr[0] + kCr[1] + kCr[2] == 0 &&
                  -(kCb[0] + kCb[1]) == kCb[2] && -(kCr[1] + kCr[2]) == kCr[0],
              "chroma is 32-bit arithmetic (the positive and the negative coefficients each sum to 112 x 128), grey is 128");
// second table: consecutive entries differ by at most 2^9 (the curve is concave: the largest step is the first one of an
// octave, E ((65 / 64)^(1 / 2.4) - 1) < 2^15 / 150, and 0 -> 1 is 32; build_import_hdr_tables checks it), the fraction has at
// most 18 bits
constexpr int kGamMaxStep = 1 << 9;
static_assert((int64_t)kGamMaxStep * ((1 << (kLinBits - kGamMant)) - 1) + (1 << (kLinBits - kGamMant - 1)) < INT32_MAX,
              "the second table's interpolation is 32-bit arithmetic");

// What a kernel reads through one pointer (efx_import_hdr_tables hands out exactly these bytes)
struct Coefs {
    int32_t qy, qrv, qgu, qgv, qbu, y0;  // the matrix; y0 = 64 (studio) or 0 (full)
    int32_t g[9];                        // the gamut matrix
    int32_t peak_nits;                   // the peak the tables were built for
};
struct Tables {
    Coefs k;
    uint32_t pq[kPqSlots];    // [i] = round(2^24 L(i / 2^kPqBits)), L <= 1; the slots behind kPqEntries are zero
    uint16_t gam[kGamSlots];  // [idx] = round(2^15 (x / 2^24)^(1 / 2.4)), x = gam_x(idx); the slots behind kGamEntries are zero
};
static_assert(sizeof(Coefs) == 64 && sizeof(Tables) % 16 == 0 && sizeof(Tables) == 64 + 4 * kPqSlots + 2 * kGamSlots, "staged as 16-byte pieces");

// A setting as efx_import_set_hdr takes it (host)
inline bool valid(int transfer, int primaries, int matrix, int full_range, int peak_nits)
{
    return transfer == kTransferPq && (primaries == 9 || primaries == 1) && colour::valid(matrix, full_range) &&
           (peak_nits == 0 || (peak_nits >= kPeakMin && peak_nits <= kPeakMax));
}

// The coefficients of a valid setting for a picture of `height` lines (matrix code 2 resolves by it, as colour::coefs)
inline bool coefs(int primaries, int matrix, int full_range, int peak_nits, int height, Coefs* k)
{
    if (matrix == colour::kUnspecified)
        matrix = height > colour::kAutoHdAbove ? 1 : 6;
    for (const Entry& e : kTable) {
        if (e.code != matrix)
            continue;
        const int32_t* q = e.q[full_range ? 1 : 0];
        k->qy = q[0], k->qrv = q[1], k->qgu = q[2], k->qgv = q[3], k->qbu = q[4];
        k->y0 = full_range ? 0 : 64;
        for (int i = 0; i < 9; i++)
            k->g[i] = primaries == 9 ? kGamut2020[i] : kGamut709[i];
        k->peak_nits = peak_nits ? peak_nits : kPeakDefault;
        return true;
    }
    return false;
}

// The import's vertical pass at 10 bits: sum = sum of k_y * h (< 2^31), 0 .. 1020
EFX_IPX_HD inline int vround10(int sum) { return (int)(((uint32_t)sum + (1u << 19)) >> 20); }

// The linear value (steps of 2^-24) of entry idx of the second table, and the entry a value starts from
EFX_IPX_HD inline uint32_t gam_x(int idx)
{
    const int s = idx < 128 ? 0 : idx / 64 - 1;
    return (uint32_t)(idx - 64 * s) << s;
}

// step 1's end: the 64-bit sum to R' (0 .. 2^24)
EFX_IPX_HD inline int clamp_pos(int64_t sum)
{
    const int64_t v = sum >> 14;
    return v < 0 ? 0 : (v > kPosOne ? kPosOne : (int)v);
}

// step 2: R' (0 .. 2^24) -> linear light (0 .. 2^24); the table never falls
EFX_IPX_HD inline int32_t linear(const uint32_t* pq, int e)
{
    const int i = e >> kPqFrac;
    const uint32_t f = (uint32_t)e & ((1u << kPqFrac) - 1);
    const uint32_t a = pq[i], b = pq[i + 1 < kPqEntries ? i + 1 : kPqEntries - 1];
    return (int32_t)(a + (((b - a) * f + (1u << (kPqFrac - 1))) >> kPqFrac));
}

// step 3: one row of the gamut matrix
EFX_IPX_HD inline int32_t gamut_row(const int32_t* g, int32_t r, int32_t gg, int32_t b)
{
    const int64_t v = ((int64_t)g[0] * r + (int64_t)g[1] * gg + (int64_t)g[2] * b + (kGamutOne >> 1)) >> kGamutBits;
    return v < 0 ? 0 : (v > kLinOne ? kLinOne : (int32_t)v);
}

// step 4: linear light (0 .. 2^24) -> E' (0 .. 2^15)
EFX_IPX_HD inline int inv1886(const uint16_t* gam, int32_t x)
{
    const int top = x ? 31 - __builtin_clz((unsigned)x) : 0;
    const int s = top > kGamMant ? top - kGamMant : 0;
    const int idx = 64 * s + (x >> s), f = x & ((1 << s) - 1);
    const int a = gam[idx], b = gam[idx + 1 < kGamEntries ? idx + 1 : kGamEntries - 1];
    return a + (((b - a) * f + ((1 << s) >> 1)) >> s);
}

// steps 1 .. 4 of one pixel: y = Y10 - y0, and the chroma terms of its site
struct Site {
    int64_t r, g, b;  // qrv v + 8192, qgu u + qgv v + 8192, qbu u + 8192
};
EFX_IPX_HD inline Site site(const Coefs& k, int cb10, int cr10)
{
    const int u = cb10 - 512, v = cr10 - 512;
    return Site{(int64_t)k.qrv * v + 8192, (int64_t)k.qgu * u + (int64_t)k.qgv * v + 8192, (int64_t)k.qbu * u + 8192};
}
EFX_IPX_HD inline void sdr_rgb(const Coefs& k, const uint32_t* pq, const uint16_t* gam, const Site& c, int y10, int rgb[3])
{
    const int64_t y = (int64_t)k.qy * (y10 - k.y0);
    const int32_t lr = linear(pq, clamp_pos(y + c.r)), lg = linear(pq, clamp_pos(y + c.g)), lb = linear(pq, clamp_pos(y + c.b));
    rgb[0] = inv1886(gam, gamut_row(k.g, lr, lg, lb));
    rgb[1] = inv1886(gam, gamut_row(k.g + 3, lr, lg, lb));
    rgb[2] = inv1886(gam, gamut_row(k.g + 6, lr, lg, lb));
}
// step 5, and the chroma of the sums of four pixels
EFX_IPX_HD inline int luma(const int rgb[3])
{
    return ipx::clamp_u8(16 + ((kLuma[0] * rgb[0] + kLuma[1] * rgb[1] + kLuma[2] * rgb[2] + (1 << 22)) >> 23));
}
EFX_IPX_HD inline int chroma_b(const int sum[3]) { return ipx::clamp_u8(128 + ((kCb[0] * sum[0] + kCb[1] * sum[1] + kCb[2] * sum[2] + (1 << 23)) >> 24)); }
EFX_IPX_HD inline int chroma_r(const int sum[3]) { return ipx::clamp_u8(128 + ((kCr[0] * sum[0] + kCr[1] * sum[1] + kCr[2] * sum[2] + (1 << 23)) >> 24)); }

// One work item: y10 points at the block's top left 10-bit luma sample, y at where its 8-bit result goes; both bands have
// rows y_pitch samples apart
EFX_IPX_HD inline void tonemap_block(const Coefs& k, const uint32_t* pq, const uint16_t* gam, const uint16_t* y10, int cb10, int cr10,
                                     int y_pitch, uint8_t* y, uint8_t* cb, uint8_t* cr)
{
    const Site c = site(k, cb10, cr10);
    int sum[3] = {0, 0, 0};
    for (int i = 0; i < 4; i++) {
        const int o = (i >> 1) * y_pitch + (i & 1);
        int rgb[3];
        sdr_rgb(k, pq, gam, c, y10[o], rgb);
        y[o] = (uint8_t)luma(rgb);
        sum[0] += rgb[0], sum[1] += rgb[1], sum[2] += rgb[2];
    }
    *cb = (uint8_t)chroma_b(sum);
    *cr = (uint8_t)chroma_r(sum);
}

// Item (r, c) of a band's part (colour::band_part): band10 holds the band at 10 bits, band the 8-bit band, both laid out as
// `width` luma samples per row, then the Cb rows and the Cr rows of width / 2 samples
EFX_IPX_HD inline void tonemap_item(const Coefs& k, const uint32_t* pq, const uint16_t* gam, const colour::BandPart& p, int r, int c, int width,
                                    int band_rows, const uint16_t* band10, uint8_t* band)
{
    const int band_y = band_rows * width, band_c = band_y / 4;
    const int ci = (p.row0 + r) * (width / 2) + p.col0 + c;
    const int yi = 2 * (p.row0 + r) * width + 2 * (p.col0 + c);
    tonemap_block(k, pq, gam, band10 + yi, band10[band_y + ci], band10[band_y + band_c + ci], width, band + yi, band + band_y + ci,
                  band + band_y + band_c + ci);
}

}  // namespace hdr
}  // namespace efx
