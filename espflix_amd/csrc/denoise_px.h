// denoise_px.h -- arithmetic of k_denoise (k_denoise.hip, efx_denoise): the thresholded 3 x 3 binomial filter and the
// recursive temporal blend, two samples at a time in the 16-bit halves of a word, the checks of a call, and how a call is
// cut into items.  Words, the column clamp, the 16-byte fetch that stays inside an image and the store of a chunk are
// deint_px.h's.
//
// Host + device: the kernel runs exactly these functions, and tests/denoise_model_main.cpp performs whole calls with them
// on the host.  Everything is an integer function of the source bytes (the definition: include/efx.h, "noisy sources").
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "efx.h"
#include "deint_px.h"
#include "surface_px.h"

namespace efx {
namespace npx {

constexpr int kChunk = dpx::kChunk;                // samples of a row a lane owns: one 16-byte access
constexpr int kTileChunks = dpx::kTileChunks;      // chunks a wave writes per row: lanes 1 .. 62; lanes 0 and 63 fetch the halo
constexpr int kTileCols = 992;                     // kTileChunks * kChunk: the column tile
constexpr int kBandRows = 4;                       // rows of a plane a wave keeps from frame to frame: 16 registers a lane
constexpr int kWaves = 4;                          // items a workgroup takes at a time, one per wave
constexpr int kMaxThreshold = 64;
constexpr uint32_t kBlendOne = 192u * 65536u;      // 12582912: Q = kBlendOne / (Tt * Tt)
static_assert(kTileCols == kTileChunks * kChunk, "the tile is whole chunks");

// ---- the call ------------------------------------------------------------------------------------------------------------------
// Surfaces the stage reads: the byte layouts, any even size
EFX_IPX_HD inline bool surface_ok(const efx_surface& s)
{
    return spx::check(s) == spx::kOk && (s.layout == EFX_SURF_PLANAR8 || s.layout == EFX_SURF_SEMI8);
}
EFX_IPX_HD inline bool threshold_ok(int t) { return t >= 0 && t <= kMaxThreshold; }
// Q of the temporal step (0 where Tt = 0: every sample then takes the new value whole and Q is never used)
EFX_IPX_HD inline uint32_t blend_q(int tt) { return tt > 0 ? kBlendOne / (uint32_t)(tt * tt) : 0u; }

EFX_IPX_HD inline int bands(int ph) { return (ph + kBandRows - 1) / kBandRows; }
// items of one stream: a band of a column tile of a plane; luma first, then Cb and Cr -- side by side in one wave where
// they fit its halves (dpx::shared_chroma), tile by tile otherwise
EFX_IPX_HD inline int stream_items(int w, int h)
{
    return dpx::tiles(w) * bands(h) + (dpx::shared_chroma(w) ? 1 : 2) * dpx::tiles(w / 2) * bands(h / 2);
}
EFX_IPX_HD inline dpx::Item item(int w, int h, int k)
{
    const int luma = dpx::tiles(w) * bands(h);
    dpx::Item it;
    it.shared = false;
    if (k < luma) {
        it.plane = 0, it.tile = k % dpx::tiles(w), it.band = k / dpx::tiles(w);
    } else if (dpx::shared_chroma(w)) {
        it.plane = 1, it.tile = 0, it.band = k - luma, it.shared = true;
    } else {
        k -= luma;
        it.plane = 1 + (k & 1);
        k >>= 1;
        it.tile = k % dpx::tiles(w / 2), it.band = k / dpx::tiles(w / 2);
    }
    return it;
}
// The index rule for rows: clamped to the plane
EFX_IPX_HD inline int clamp_row(int r, int h) { return r < 0 ? 0 : (r >= h ? h - 1 : r); }

// The thresholds of one plane as the arithmetic takes them
struct Plane {
    uint32_t ts2;  // Ts in both halves
    int tt;
    uint32_t q;    // blend_q(tt)
};
EFX_IPX_HD inline Plane plane_of(int ts, int tt)
{
    Plane p;
    p.ts2 = (uint32_t)ts * 0x00010001u, p.tt = tt, p.q = blend_q(tt);
    return p;
}

// ---- words ----------------------------------------------------------------------------------------------------------------------
// both halves shifted right arithmetically by n
#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline uint32_t sra2(uint32_t a, int n) { return dpx::un(dpx::pk(a) >> dpx::s16x2{(short)n, (short)n}); }
#else
inline uint32_t sra2(uint32_t a, int n) { return dpx::each2(a, 0, [n](int x, int) { return x >> n; }); }
#endif

// Bytes P, P + 1 of the 24 bytes of a row's six words (columns X - 4 .. X + 19) in the two 16-bit halves: one v_perm_b32
template <int P>
EFX_IPX_HD inline uint32_t pair_at(const uint32_t* e)
{
    static_assert(P >= 3 && P <= 19, "the pair lies inside the six words");
    constexpr int k = P >> 2, b = P & 3;
    constexpr uint32_t sel = 0x0c000c00u | ((uint32_t)(b + 1) << 16) | (uint32_t)b;
    return dpx::perm(e[k < 5 ? k + 1 : 5], e[k], sel);
}

// v - c where |v - c| <= Ts, else 0, in both halves: what a neighbour adds to the weighted sum beyond the centre
EFX_IPX_HD inline uint32_t near2(uint32_t v, uint32_t c, uint32_t ts2)
{
    const uint32_t d = dpx::sub2(v, c);
    const uint32_t a = dpx::max2(d, dpx::sub2(c, v));
    const uint32_t far = sra2(dpx::sub2(ts2, a), 15);  // all ones where |v - c| > Ts
    return d & ~far;
}

// The spatial step for samples 2 H, 2 H + 1 of word I of a chunk.  Every v(i, j) is c + near2, so the weighted sum is
// 16 c + the weighted sum of the near2 terms, and s = c + ((that + 8) >> 4): the shift is arithmetic and 16 c a multiple
// of 16, so the result is the definition's.
template <int I, int H>
EFX_IPX_HD inline uint32_t spatial2(const dpx::Ext& up, const dpx::Ext& mid, const dpx::Ext& dn, uint32_t ts2)
{
    constexpr int p = 4 * (1 + I) + 2 * H;
    const uint32_t c = pair_at<p>(mid.e);
    const uint32_t corners = dpx::add2(dpx::add2(near2(pair_at<p - 1>(up.e), c, ts2), near2(pair_at<p + 1>(up.e), c, ts2)),
                                       dpx::add2(near2(pair_at<p - 1>(dn.e), c, ts2), near2(pair_at<p + 1>(dn.e), c, ts2)));
    const uint32_t edges = dpx::add2(dpx::add2(near2(pair_at<p>(up.e), c, ts2), near2(pair_at<p>(dn.e), c, ts2)),
                                     dpx::add2(near2(pair_at<p - 1>(mid.e), c, ts2), near2(pair_at<p + 1>(mid.e), c, ts2)));
    const uint32_t sum = dpx::add2(dpx::add2(corners, 0x00080008u), dpx::add2(edges, edges));
    return dpx::add2(c, sra2(sum, 4));
}

// (a k + 128) >> 8 of the temporal step for one |d| = a (0 .. 255): how far the output moves from P towards s.  Both
// products fit 24 x 24 bits (a a < 2^16, Q < 2^24); where a >= Tt the first one is not used.
EFX_IPX_HD inline uint32_t blend_step(uint32_t a, int tt, uint32_t q)
{
    a &= 0xFFu;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t far = __umul24(__umul24(a, a), q) >> 16;  // (v_mul_u32_u24: the low 32 bits of a 24 x 24 bit product)
#else
    const uint32_t far = ((a * a) * (q & 0xFFFFFFu)) >> 16;
#endif
    const uint32_t k = (int)a >= tt ? 256u : 64u + far;
    return (a * k + 128u) >> 8;
}

// The temporal step in both halves: out = P + sgn(d) ((a k + 128) >> 8)
EFX_IPX_HD inline uint32_t temporal2(uint32_t s, uint32_t p, int tt, uint32_t q)
{
    const uint32_t d = dpx::sub2(s, p);
    const uint32_t a = dpx::max2(d, dpx::sub2(p, s));
    const uint32_t m = blend_step(a & 0xFFFFu, tt, q) | (blend_step(a >> 16, tt, q) << 16);
    const uint32_t neg = sra2(d, 15);  // all ones where d < 0
    return dpx::add2(p, dpx::sub2(m ^ neg, neg));
}

// the row's words one place down: word 1 of the chunk becomes word 0
EFX_IPX_HD inline void next_word(dpx::Ext* x)
{
    x->e[0] = x->e[1], x->e[1] = x->e[2], x->e[2] = x->e[3], x->e[3] = x->e[4], x->e[4] = x->e[5];
}

// One output row of a chunk: up, mid, dn = rows y - 1, y, y + 1 of the frame (clamped) with their halo words; prev = the
// chunk at the same place of the stream's previous output.  Without one (has_prev = false: the stream's first picture)
// the same arithmetic runs with Tt = 0, under which every sample takes the new value whole whatever prev holds: out = s.
// The four words go through one body, each moved into word 0's place in turn: a quarter of the code of four bodies, which
// keeps the kernel's walk over a band inside the instruction cache, for 19 moves a word.
EFX_IPX_HD inline dpx::Chunk row_out(dpx::Ext up, dpx::Ext mid, dpx::Ext dn, dpx::Chunk prev, bool has_prev, const Plane& t)
{
    const int tt = has_prev ? t.tt : 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int i = 0; i < 4; i++) {
        const uint32_t lo = temporal2(spatial2<0, 0>(up, mid, dn, t.ts2), dpx::widen(prev.d[0], 0), tt, t.q);
        const uint32_t hi = temporal2(spatial2<0, 1>(up, mid, dn, t.ts2), dpx::widen(prev.d[0], 1), tt, t.q);
        next_word(&up), next_word(&mid), next_word(&dn);
        prev.d[0] = prev.d[1], prev.d[1] = prev.d[2], prev.d[2] = prev.d[3];
        prev.d[3] = dpx::perm(hi, lo, dpx::kNarrow);
    }
    return prev;
}

// A fetched row with the neighbouring lanes' words either side, clamped at the picture's edges
EFX_IPX_HD inline dpx::Ext widen_row(const dpx::Chunk& c, uint32_t left, uint32_t right, bool active, int X, int n)
{
    dpx::Ext x;
    x.e[0] = left, x.e[5] = right;
    x.e[1] = c.d[0], x.e[2] = c.d[1], x.e[3] = c.d[2], x.e[4] = c.d[3];
    if (active)
        dpx::clamp_cols(&x, X, n);
    return x;
}

// A row of byte samples (every plane but a semi-planar surface's pair plane) in two steps, so that the kernel can ask for
// the next frame's row long before it reads it, without a branch between the load and the register it lands in:
// load_plain makes the one 16-byte access -- at the samples, or at end - 16 where that would cross end (dpx::fetch16's
// rule) -- and settle_plain, when the row is taken, shifts down what such a moved access brought.  X = the chunk's first
// column; a lane with nothing to fetch passes 0 and its chunk is never looked at.
EFX_IPX_HD inline size_t plain_at(const dpx::PlaneAt& p, int r, int X) { return p.first + (size_t)r * p.pitch + (size_t)X; }
EFX_IPX_HD inline dpx::Chunk load_plain(const dpx::PlaneAt& p, const uint8_t* img, size_t end, int r, int X)
{
    const size_t at = plain_at(p, r, X);
    dpx::Chunk c;
    memcpy(c.d, img + (at + 16 <= end ? at : end - 16), 16);
    return c;
}
EFX_IPX_HD inline dpx::Chunk settle_plain(dpx::Chunk c, const dpx::PlaneAt& p, size_t end, int r, int X)
{
    const size_t at = plain_at(p, r, X);
    if (at + 16 > end) {
        const int k = (int)(at - (end - 16));  // 1 .. 15
        uint64_t lo = ((uint64_t)c.d[1] << 32) | c.d[0], hi = ((uint64_t)c.d[3] << 32) | c.d[2];
        if (k >= 8) {
            lo = hi >> (8 * (k - 8));
            hi = 0;
        } else {
            lo = (lo >> (8 * k)) | (hi << (64 - 8 * k));
            hi >>= 8 * k;
        }
        c.d[0] = (uint32_t)lo, c.d[1] = (uint32_t)(lo >> 32), c.d[2] = (uint32_t)hi, c.d[3] = (uint32_t)(hi >> 32);
    }
    return c;
}

// Samples X .. X + 15 of row y of a plane of a packed I420 picture (a previous output) whose readable bytes end at end
EFX_IPX_HD inline dpx::Chunk fetch_prev(const uint8_t* pic, size_t end, size_t plane_first, int pw, int y, int X)
{
    return dpx::fetch16(pic + plane_first + (size_t)y * pw + X, pic + end, false);
}

}  // namespace npx
}  // namespace efx
