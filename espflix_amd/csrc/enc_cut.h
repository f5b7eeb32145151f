// enc_cut.h -- scene-cut detection of the MPEG-1 encoder (efx_encode_set_scene_cut): the measure of one macroblock on the
// decimated luma, and the rule that turns a stream's state and the picture's two sums into its picture type.
//
// Host + device, like enc_core.h and enc_rate.h: k_encode.hip (k_enc_cut, k_enc_rows, k_enc_pack) runs exactly these
// functions and tests/enc_cut_model_main.cpp builds them with a plain C++ compiler.  Integer arithmetic only, and the
// picture's sums are sums of per-macroblock minima, so the order of any reduction does not show in the result.
// include/efx.h ("scene cuts") defines the rule; DESIGN.md gives the reasoning behind it and its constants.
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

constexpr int kCutW = 88, kCutH = 48;        // the decimated luma: one byte per 4 x 4 pels of 352 x 192
constexpr int kCutBytes = kCutW * kCutH;     // 4224
constexpr int kCutRange = 4;                 // full-pel search range on the decimated picture (16 luma pels)
constexpr int kCutSide = 2 * kCutRange + 1;  // 9 x 9 = 81 candidates per macroblock
constexpr uint32_t kCutFloor = 8192;         // a cut needs cut_p above this: fades from and to black score 256/256 on tiny sums
constexpr int kTypeI = 1, kTypeP = 2, kTypeCutI = 5;  // efx_enc_picture_info.type: 5 = I placed by the cut rule alone

// What a call fixes for every stream (efx_scene_cut, checked): threshold 0 = off
struct CutParams {
    int threshold;  // 0, or 1 .. 256: a cut needs 256 cut_p > threshold cut_i
    int min_gop;    // 1 .. 255: ... and at least min_gop pictures since the last I picture, counting it
};

// D[y][x] = (sum of the 4 x 4 luma pels at (4 y, 4 x) + 8) >> 4 of a 352-wide luma plane, for `rows` decimated rows
EFX_ENC_HD inline void cut_decimate(const uint8_t* luma, int rows, uint8_t* d)
{
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < kCutW; x++) {
            int sum = 0;
            for (int j = 0; j < 4; j++)
                for (int i = 0; i < 4; i++)
                    sum += luma[(4 * y + j) * (4 * kCutW) + 4 * x + i];
            d[y * kCutW + x] = (uint8_t)((sum + 8) >> 4);
        }
}

// May the 4 x 4 block of macroblock (r, c) be compared at (dx, dy)?  Only where it lies wholly inside the picture.
EFX_ENC_HD inline bool cut_vector_ok(int r, int c, int dx, int dy)
{
    const int x = 4 * c + dx, y = 4 * r + dy;
    return x >= 0 && x + 4 <= kCutW && y >= 0 && y + 4 <= kCutH;
}

// One macroblock (host form; k_enc_cut computes the same sums with v_sad_u8 on packed words): dev = the deviation of its
// 4 x 4 block of `cur` from the block's own mean, best = the smallest SAD against `prev` over the allowed vectors
// (prev == nullptr: best = dev, a fresh stream's picture 0).
EFX_ENC_HD inline void cut_mb(const uint8_t* cur, const uint8_t* prev, int r, int c, uint32_t* dev_out, uint32_t* best_out)
{
    const uint8_t* b = cur + 4 * r * kCutW + 4 * c;
    int sum = 0;
    for (int j = 0; j < 4; j++)
        for (int i = 0; i < 4; i++)
            sum += b[j * kCutW + i];
    const int mean = (sum + 8) >> 4;
    uint32_t dev = 0;
    for (int j = 0; j < 4; j++)
        for (int i = 0; i < 4; i++) {
            const int d = (int)b[j * kCutW + i] - mean;
            dev += (uint32_t)(d < 0 ? -d : d);
        }
    uint32_t best = dev;
    if (prev) {
        best = 0xFFFFFFFFu;
        for (int dy = -kCutRange; dy <= kCutRange; dy++)
            for (int dx = -kCutRange; dx <= kCutRange; dx++) {
                if (!cut_vector_ok(r, c, dx, dy))
                    continue;
                const uint8_t* p = prev + (4 * r + dy) * kCutW + 4 * c + dx;
                uint32_t sad = 0;
                for (int j = 0; j < 4; j++)
                    for (int i = 0; i < 4; i++) {
                        const int d = (int)b[j * kCutW + i] - (int)p[j * kCutW + i];
                        sad += (uint32_t)(d < 0 ? -d : d);
                    }
                best = sad < best ? sad : best;
            }
    }
    *dev_out = dev;
    *best_out = best;
}

// The picture's type: pictures = pictures of the stream so far, g = pictures since the stream's last I picture, counting
// it (0 on a fresh stream), cut_i / cut_p = the picture's sums (anything when threshold is 0).  kTypeI: the first picture
// and every gop-th since the last I picture; kTypeCutI: the cut rule alone; else kTypeP.
EFX_ENC_HD inline int cut_picture_type(uint32_t pictures, uint32_t g, int gop, const CutParams& p, uint32_t cut_i, uint32_t cut_p)
{
    if (pictures == 0 || g == (uint32_t)gop)
        return kTypeI;
    // 256 cut_p < 2^32: cut_p <= 264 x 16 x 255; threshold cut_i likewise
    if (p.threshold > 0 && g >= (uint32_t)p.min_gop && cut_p > kCutFloor && 256u * cut_p > (uint32_t)p.threshold * cut_i)
        return kTypeCutI;
    return kTypeP;
}

// ... and what follows from it: the GOP phase the headers and the rate controller see (0 for an I picture, else g, which
// is the picture's temporal_reference), and g after the picture
EFX_ENC_HD inline int cut_phase(int type, uint32_t g) { return type == kTypeP ? (int)g : 0; }
EFX_ENC_HD inline uint32_t cut_next_g(int type, uint32_t g) { return type == kTypeP ? g + 1 : 1; }

}  // namespace enc
}  // namespace efx
