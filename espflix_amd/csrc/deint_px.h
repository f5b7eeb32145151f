// deint_px.h -- arithmetic of k_deint (k_deint.hip, efx_deinterlace): the rule for one missing sample, four samples at a
// time on packed words, the picture-edge clamp on fetched words, the 16-byte fetch that stays inside an image, the store of
// a chunk, and how a call is cut into items.
//
// Host + device: the kernel runs exactly these functions, and tests/deint_model_main.cpp performs whole calls with them on
// the host.  Everything is an integer function of the source bytes (the definition: include/efx.h, "interlaced sources").
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "efx.h"
#include "surface_px.h"

namespace efx {
namespace dpx {

constexpr int kChunk = 16;                         // samples of a row a lane owns: one 16-byte access
constexpr int kTileChunks = 62;                    // chunks a wave writes per row: lanes 1 .. 62; lanes 0 and 63 fetch the halo
constexpr int kTileCols = kTileChunks * kChunk;    // 992: the column tile
constexpr int kHalfChunks = 30;                    // ... per chroma plane where Cb and Cr share a wave: lanes 1 .. 30 and 33 .. 62
constexpr int kBandRows = 16;                      // rows a wave walks down; even
constexpr int kWaves = 4;                          // items a workgroup takes at a time, one per wave

// ---- the call ------------------------------------------------------------------------------------------------------------------
// efx_deinterlace_count
EFX_IPX_HD inline int count(int n_frames, int lead, int tail, int mode)
{
    if (n_frames < 1 || (lead != 0 && lead != 1) || (tail != 0 && tail != 1) || lead + tail >= n_frames)
        return -1;
    if (mode != EFX_DEINT_FRAME && mode != EFX_DEINT_FIELD)
        return -1;
    const int64_t n = (int64_t)(n_frames - lead - tail) * (mode == EFX_DEINT_FIELD ? 2 : 1);
    return n > INT32_MAX ? -1 : (int)n;
}

// Surfaces the stage reads: the byte layouts, height a multiple of 4 from 8
EFX_IPX_HD inline bool surface_ok(const efx_surface& s)
{
    return spx::check(s) == spx::kOk && (s.layout == EFX_SURF_PLANAR8 || s.layout == EFX_SURF_SEMI8) && s.height >= 8 && (s.height & 3) == 0;
}

EFX_IPX_HD inline int plane_w(int w, int plane) { return plane ? w / 2 : w; }
EFX_IPX_HD inline int plane_h(int h, int plane) { return plane ? h / 2 : h; }
// where a plane begins in a packed I420 output picture
EFX_IPX_HD inline size_t out_plane(int w, int h, int plane)
{
    return plane == 0 ? 0 : (size_t)w * h + (plane == 2 ? (size_t)(w / 2) * (h / 2) : 0);
}
EFX_IPX_HD inline int tiles(int pw) { return ((pw + kChunk - 1) / kChunk + kTileChunks - 1) / kTileChunks; }
EFX_IPX_HD inline int bands(int ph) { return (ph + kBandRows - 1) / kBandRows; }
// Chroma planes of at most 480 samples a row (SD sources) fit half a wave: Cb takes lanes 0 .. 31 and Cr lanes 32 .. 63 of
// the same item, instead of two items that leave most of their lanes idle
EFX_IPX_HD inline bool shared_chroma(int w) { return (w / 2 + kChunk - 1) / kChunk <= kHalfChunks; }
// items of one frame: a band of a column tile of a plane; luma first, then Cb and Cr tile by tile side by side
EFX_IPX_HD inline int frame_items(int w, int h) { return tiles(w) * bands(h) + (shared_chroma(w) ? 1 : 2) * tiles(w / 2) * bands(h / 2); }

struct Item {
    int plane, tile, band;
    bool shared;  // plane 1 in lanes 0 .. 31 and plane 2 in lanes 32 .. 63
};
EFX_IPX_HD inline Item item(int w, int h, int k)
{
    const int luma = tiles(w) * bands(h);
    Item it;
    it.shared = false;
    if (k < luma) {
        it.plane = 0, it.tile = k % tiles(w), it.band = k / tiles(w);
    } else if (shared_chroma(w)) {
        it.plane = 1, it.tile = 0, it.band = k - luma, it.shared = true;
    } else {
        k -= luma;
        it.plane = 1 + (k & 1);
        k >>= 1;
        it.tile = k % tiles(w / 2), it.band = k / tiles(w / 2);
    }
    return it;
}

// A lane's place in an item: its plane, the first column of its chunk (below 0 or beyond the row: nothing to fetch), and
// whether it only fetches the halo for its neighbour
struct Place {
    int plane, X;
    bool halo;
};
EFX_IPX_HD inline Place place(const Item& it, int lane)
{
    Place p;
    if (it.shared) {
        const int l = lane & 31;
        p.plane = 1 + (lane >> 5), p.X = (l - 1) * kChunk, p.halo = l == 0 || l == 31;
    } else {
        p.plane = it.plane, p.X = (it.tile * kTileChunks - 1 + lane) * kChunk, p.halo = lane == 0 || lane == 63;
    }
    return p;
}

// The index rule for rows: only -2 .. h + 1 occur
EFX_IPX_HD inline int reflect(int r, int h) { return r < 0 ? r + 2 : (r >= h ? r - 2 : r); }

// Which output of a frame (0 = its first field completed, 1 = its second) keeps the rows of parity q, -1 = none;
// n_out_i = outputs per frame (1 or 2).  The other parity's rows are the missing ones of that output.
EFX_IPX_HD inline int keeper(int first_field, int n_out_i, int q)
{
    const int i = first_field == EFX_FIELD_TOP ? q : 1 - q;
    return i < n_out_i ? i : -1;
}

// ---- words ----------------------------------------------------------------------------------------------------------------------
struct Chunk {
    uint32_t d[4];  // 16 samples, sample 0 in the low byte of d[0]
};
struct Ext {
    uint32_t e[6];  // columns X - 4 .. X + 19 of a row: the left neighbour's last word, the chunk, the right neighbour's first
};

// v_perm_b32: result byte i is byte sel_i of the eight bytes hi : lo (0 .. 3 lie in lo), or 0x00 for the selector 0x0c
EFX_IPX_HD inline uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 0xFF;
        if (s < 8)
            r |= (uint32_t)((both >> (8 * s)) & 0xFF) << (8 * i);
    }
    return r;
#endif
}

// v_sad_u8 against an accumulator of 0: the sum of the four bytes' absolute differences
EFX_IPX_HD inline uint32_t sad4(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, 0u);
#else
    uint32_t s = 0;
    for (int i = 0; i < 4; i++) {
        const int x = (int)((a >> (8 * i)) & 0xFF) - (int)((b >> (8 * i)) & 0xFF);
        s += (uint32_t)(x < 0 ? -x : x);
    }
    return s;
#endif
}

// Two signed 16-bit values in the halves of a dword: the v_pk_*_i16 instructions on the device
#if defined(__HIP_DEVICE_COMPILE__)
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ inline s16x2 pk(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
__device__ inline uint32_t un(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ inline uint32_t add2(uint32_t a, uint32_t b) { return un(pk(a) + pk(b)); }
__device__ inline uint32_t sub2(uint32_t a, uint32_t b) { return un(pk(a) - pk(b)); }
__device__ inline uint32_t half2(uint32_t a) { return un(pk(a) >> s16x2{1, 1}); }
__device__ inline uint32_t min2(uint32_t a, uint32_t b) { return un(__builtin_elementwise_min(pk(a), pk(b))); }
__device__ inline uint32_t max2(uint32_t a, uint32_t b) { return un(__builtin_elementwise_max(pk(a), pk(b))); }
#else
template <class F>
inline uint32_t each2(uint32_t a, uint32_t b, F f)
{
    const int lo = f((int)(int16_t)(a & 0xFFFF), (int)(int16_t)(b & 0xFFFF));
    const int hi = f((int)(int16_t)(a >> 16), (int)(int16_t)(b >> 16));
    return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
}
inline uint32_t add2(uint32_t a, uint32_t b) { return each2(a, b, [](int x, int y) { return x + y; }); }
inline uint32_t sub2(uint32_t a, uint32_t b) { return each2(a, b, [](int x, int y) { return x - y; }); }
inline uint32_t half2(uint32_t a) { return each2(a, 0, [](int x, int) { return x >> 1; }); }
inline uint32_t min2(uint32_t a, uint32_t b) { return each2(a, b, [](int x, int y) { return x < y ? x : y; }); }
inline uint32_t max2(uint32_t a, uint32_t b) { return each2(a, b, [](int x, int y) { return x > y ? x : y; }); }
#endif
EFX_IPX_HD inline uint32_t absdiff2(uint32_t a, uint32_t b) { return max2(sub2(a, b), sub2(b, a)); }

constexpr uint32_t kNarrow = 0x06040200u;  // the low bytes of four halves back into a word
// bytes 0, 1 (half 0) or 2, 3 (half 1) of a word into the two 16-bit halves
EFX_IPX_HD inline uint32_t widen(uint32_t v, int half) { return perm(0u, v, half ? 0x0c030c02u : 0x0c010c00u); }

// Three bytes from byte U (1 .. 8) of the twelve bytes of w[0 .. 2], the fourth byte 0: one v_perm_b32
template <int U>
EFX_IPX_HD inline uint32_t win3(const uint32_t* w)
{
    static_assert(U >= 0 && U <= 9, "the window lies inside the three words");
    constexpr int b = U <= 5 ? U : U - 4;
    constexpr uint32_t sel = 0x0c000000u | ((uint32_t)(b + 2) << 16) | ((uint32_t)(b + 1) << 8) | (uint32_t)b;
    return U <= 5 ? perm(w[1], w[0], sel) : perm(w[2], w[1], sel);
}
template <int I>
EFX_IPX_HD inline int byte_at(const uint32_t* w) { return (int)((w[I >> 2] >> (8 * (I & 3))) & 0xFF); }

// score(J) and pred(J) of sample S (0 .. 3) of the middle word; up = cur[y - 1], dn = cur[y + 1], three words each
template <int S, int J>
EFX_IPX_HD inline int score(const uint32_t* up, const uint32_t* dn) { return (int)sad4(win3<3 + S + J>(up), win3<3 + S - J>(dn)); }
template <int S, int J>
EFX_IPX_HD inline int pred(const uint32_t* up, const uint32_t* dn) { return (byte_at<4 + S + J>(up) + byte_at<4 + S - J>(dn)) >> 1; }

// The spatial prediction of sample S: the edge-directed search of the definition.  All five scores are made and the
// choices are selects: a lane that skipped score(2s) would wait for its neighbours that did not.
template <int S>
EFX_IPX_HD inline int spatial(const uint32_t* up, const uint32_t* dn)
{
    int best = score<S, 0>(up, dn) - 1, sp = pred<S, 0>(up, dn);
    const int m1 = score<S, -1>(up, dn), m2 = score<S, -2>(up, dn), p1 = score<S, 1>(up, dn), p2 = score<S, 2>(up, dn);
    const bool a1 = m1 < best;
    best = a1 ? m1 : best, sp = a1 ? pred<S, -1>(up, dn) : sp;
    const bool a2 = a1 && m2 < best;
    best = a2 ? m2 : best, sp = a2 ? pred<S, -2>(up, dn) : sp;
    const bool b1 = p1 < best;
    best = b1 ? p1 : best, sp = b1 ? pred<S, 1>(up, dn) : sp;
    const bool b2 = b1 && p2 < best;
    return b2 ? pred<S, 2>(up, dn) : sp;
}

// The rows one missing row is made from, one word (four samples) of each; cur rows with the words either side
struct Rows {
    uint32_t up[3];      // cur[y - 1]: three words, the middle one the samples' own
    uint32_t dn[3];      // cur[y + 1]
    uint32_t pu, pd;     // prev[y - 1], prev[y + 1]
    uint32_t nu, nd;     // next[y - 1], next[y + 1]
    uint32_t bm, b0, bp; // B[y - 2], B[y], B[y + 2]
    uint32_t am, a0, ap; // A
};

// Four missing samples: the temporal part two samples at a time in 16-bit halves, the spatial search per sample
EFX_IPX_HD inline uint32_t missing4(const Rows& r)
{
    const int sp[4] = {spatial<0>(r.up, r.dn), spatial<1>(r.up, r.dn), spatial<2>(r.up, r.dn), spatial<3>(r.up, r.dn)};
    uint32_t out[2];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int h = 0; h < 2; h++) {
        const uint32_t c = widen(r.up[1], h), e = widen(r.dn[1], h);
        const uint32_t b0 = widen(r.b0, h), a0 = widen(r.a0, h);
        const uint32_t d = half2(add2(b0, a0));
        const uint32_t t0 = half2(absdiff2(b0, a0));
        const uint32_t t1 = half2(add2(absdiff2(widen(r.pu, h), c), absdiff2(widen(r.pd, h), e)));
        const uint32_t t2 = half2(add2(absdiff2(widen(r.nu, h), c), absdiff2(widen(r.nd, h), e)));
        uint32_t diff = max2(max2(t0, t1), t2);
        const uint32_t b = half2(add2(widen(r.bm, h), widen(r.am, h)));
        const uint32_t f = half2(add2(widen(r.bp, h), widen(r.ap, h)));
        const uint32_t de = sub2(d, e), dc = sub2(d, c), bc = sub2(b, c), fe = sub2(f, e);
        const uint32_t mx = max2(max2(de, dc), min2(bc, fe));
        const uint32_t mn = min2(min2(de, dc), max2(bc, fe));
        diff = max2(max2(diff, mn), sub2(0u, mx));
        const uint32_t s2 = (uint32_t)sp[2 * h] | ((uint32_t)sp[2 * h + 1] << 16);
        out[h] = min2(max2(s2, sub2(d, diff)), add2(d, diff));
    }
    return perm(out[1], out[0], kNarrow);
}

// The column clamp on the fetched words of a cur row: X = the chunk's first column, n = pw - X >= 1 the columns that
// exist from X on.  Columns below 0 take column 0's sample, columns from pw on column pw - 1's.
EFX_IPX_HD inline void clamp_cols(Ext* x, int X, int n)
{
    if (X == 0)
        x->e[0] = perm(0u, x->e[1], 0u);
    if (n < kChunk + 4) {
        const int last = n - 1;  // 0 .. 18
        uint32_t word = 0;  // the word that holds column pw - 1 (kept in registers: OR of masked words, no indexed access)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 1; j < 6; j++)
            word |= (last >> 2) == j - 1 ? x->e[j] : 0u;
        const uint32_t e4 = ((word >> (8 * (last & 3))) & 0xFF) * 0x01010101u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 1; j < 6; j++) {
            const int k = n - 4 * (j - 1);  // columns of this word that exist
            if (k < 4) {
                const uint32_t mask = k <= 0 ? 0u : (1u << (8 * k)) - 1u;
                x->e[j] = (x->e[j] & mask) | (e4 & ~mask);
            }
        }
    }
}

// ---- memory ---------------------------------------------------------------------------------------------------------------------
// 16 bytes from a (any alignment), never touching a byte at or beyond end (end - 16 is readable): where the access would
// cross end it is made at end - 16 and shifted down; the bytes beyond end come out as 0.  safe = the caller knows that it
// cannot cross (the same for every lane of a wave, so that the test costs the wave a scalar branch).
EFX_IPX_HD inline Chunk fetch16(const uint8_t* a, const uint8_t* end, bool safe)
{
    uint64_t v[2];
    uint64_t lo, hi;
    if (safe || a + 16 <= end) {
        memcpy(v, a, 16);
        lo = v[0], hi = v[1];
    } else {
        const int k = (int)(a - (end - 16));  // 1 .. 15
        memcpy(v, end - 16, 16);
        lo = v[0], hi = v[1];
        if (k >= 8) {
            lo = hi >> (8 * (k - 8));
            hi = 0;
        } else {
            lo = (lo >> (8 * k)) | (hi << (64 - 8 * k));
            hi >>= 8 * k;
        }
    }
    Chunk c;
    c.d[0] = (uint32_t)lo, c.d[1] = (uint32_t)(lo >> 32), c.d[2] = (uint32_t)hi, c.d[3] = (uint32_t)(hi >> 32);
    return c;
}

// Where the rows of a plane of the canonical image lie in a source image
struct PlaneAt {
    size_t first, pitch;  // bytes to row 0, and from a row to the next
    size_t row_bytes;     // bytes of a row that hold samples
    bool pairs;           // a chroma plane of a semi-planar surface: its samples are every other byte of the pair rows
    bool odd;             // ... the odd ones
};
EFX_IPX_HD inline PlaneAt plane_at(const efx_surface& s, int plane)
{
    PlaneAt p;
    p.pairs = plane != 0 && s.layout == EFX_SURF_SEMI8;
    const int k = p.pairs ? 1 : plane;
    // (selects, not an index: the plane may differ from lane to lane, and the surface lies in scalar registers)
    p.first = k == 0 ? s.offset[0] : (k == 1 ? s.offset[1] : s.offset[2]);
    p.pitch = k == 0 ? s.pitch[0] : (k == 1 ? s.pitch[1] : s.pitch[2]);
    p.row_bytes = (size_t)(plane == 0 || p.pairs ? s.width : s.width / 2);
    p.odd = p.pairs && ((plane == 2) != (s.swap_uv != 0));
    return p;
}

// Samples X .. X + 15 of row r of a plane of the image at img (n = pw - X >= 1 of them exist; the rest is whatever lies
// there); end = the image's bytes rounded up to 16.  Everything but X and n is the same for the lanes of a wave.
EFX_IPX_HD inline Chunk fetch_row(const PlaneAt& p, const uint8_t* img, size_t end, int r, int X, int n)
{
    const size_t row = p.first + (size_t)r * p.pitch;
    const bool safe = row + ((p.row_bytes + 15) & ~(size_t)15) <= end;  // no 16 bytes that begin in this row cross the end
    const uint8_t* at = img + row;
    if (!p.pairs)
        return fetch16(at + X, img + end, safe);
    // the pair plane: 32 bytes, the even or the odd ones
    const uint8_t* a = at + 2 * (size_t)X;
    const Chunk p0 = fetch16(a, img + end, safe);
    Chunk p1 = {};
    if (n > 8)
        p1 = fetch16(a + 16, img + end, safe);
    const uint32_t sel = p.odd ? spx::kPickOdd : spx::kPickEven;
    Chunk c;
    c.d[0] = perm(p0.d[1], p0.d[0], sel), c.d[1] = perm(p0.d[3], p0.d[2], sel);
    c.d[2] = perm(p1.d[1], p1.d[0], sel), c.d[3] = perm(p1.d[3], p1.d[2], sel);
    return c;
}

// The first n (1 .. 16) bytes of a chunk to p (any alignment): one 16-byte store, or the binary pieces of a row's tail
EFX_IPX_HD inline void store_chunk(uint8_t* p, const Chunk& c, int n)
{
    if (n >= kChunk) {
        memcpy(p, c.d, 16);
        return;
    }
    uint32_t w0 = c.d[0], w1 = c.d[1];
    if (n & 8) {
        const uint64_t v = ((uint64_t)w1 << 32) | w0;
        memcpy(p, &v, 8);
        p += 8, w0 = c.d[2], w1 = c.d[3];
    }
    if (n & 4) {
        memcpy(p, &w0, 4);
        p += 4, w0 = w1;
    }
    if (n & 2) {
        const uint16_t v = (uint16_t)w0;
        memcpy(p, &v, 2);
        p += 2, w0 >>= 16;
    }
    if (n & 1)
        *p = (uint8_t)w0;
}

}  // namespace dpx
}  // namespace efx
