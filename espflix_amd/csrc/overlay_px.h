// overlay_px.h -- arithmetic of k_overlay (k_overlay.hip, efx_overlay): the validity rule of an event, its gain at a
// picture, the two rounded divisions without a division, the blend of four columns of two rows and their two chroma
// sites, the 16-byte window of a bitmap row that stays inside the atlas, and how a picture is cut into the units a lane
// owns.  Words, v_perm_b32, the packed 16-bit halves and the bounded 16-byte fetch are deint_px.h's; the colour matrix is
// import_px.h's.
//
// Host + device: the kernel runs exactly these functions, and tests/overlay_model_main.cpp performs whole calls with them
// on the host.  Everything is an integer function of the bytes (the definition: include/efx.h, "subtitles and logos").
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "efx.h"
#include "import_px.h"
#include "deint_px.h"

namespace efx {
namespace ovx {

constexpr int kScanStep = 256;                     // events a workgroup tests per step of the list's scan: one per lane
constexpr int kWaves = 4;                          // waves of a workgroup: kScanStep / 64
constexpr int kWidth = 352, kHeight = 192;         // the picture
constexpr size_t kPicture = 101376;                // its bytes; Cb begins at kCb, Cr at kCr
constexpr size_t kCb = (size_t)kWidth * kHeight, kCr = kCb + kCb / 4;
constexpr int kUnitCols = 32, kUnitRows = 2;       // luma samples a lane owns: four 16-byte chunks, and one chunk of Cb and of Cr
constexpr int kUnitsX = kWidth / kUnitCols;        // 11
constexpr int kUnits = kUnitsX * (kHeight / kUnitRows);  // 1056, row by row
constexpr int kTiles = (kUnits + 63) / 64;         // 17: a wave's tile is 64 consecutive units
constexpr int64_t kMaxIndex = (int64_t)1 << 40;
static_assert(kScanStep == 64 * kWaves, "one event per lane");
static_assert(kPicture == kCr + kCb / 4 && kCb % 16 == 0 && kCr % 16 == 0 && kWidth % kUnitCols == 0, "chunks are aligned");

// ---- the rule ------------------------------------------------------------------------------------------------------------------
EFX_IPX_HD inline int bpp(const efx_overlay_event& e) { return e.kind == EFX_OVL_RGBA ? 4 : 1; }

// The one predicate: efx_overlay_check and the kernel
EFX_IPX_HD inline bool valid(const efx_overlay_event& e, uint64_t atlas_bytes)
{
    if (e.kind != EFX_OVL_A8 && e.kind != EFX_OVL_RGBA)
        return false;
    if (e.first < 0 || e.first > e.last || e.last >= kMaxIndex || e.stream < -1)
        return false;
    if (e.x < -4096 || e.x > 4095 || e.y < -4096 || e.y > 4095 || e.w < 1 || e.w > 4096 || e.h < 1 || e.h > 4096)
        return false;
    if (e.opacity > 256 || e.fade_in > 32767 || e.fade_out > 32767 || e.reserved0 != 0 || e.reserved != 0)
        return false;
    const uint32_t row = (uint32_t)e.w * (uint32_t)bpp(e);
    if (e.pitch < row)
        return false;
    if (e.kind == EFX_OVL_RGBA ? ((e.offset | e.pitch) & 3) != 0 || e.colour != 0 : e.colour >= (1u << 24))
        return false;
    // (h - 1) pitch + w bpp < 2^44: the sum wraps only with an offset that is itself beyond any atlas
    const uint64_t span = (uint64_t)(e.h - 1) * e.pitch + row;
    return e.offset <= atlas_bytes && span <= atlas_bytes - e.offset;
}

EFX_IPX_HD inline bool active(const efx_overlay_event& e, uint64_t atlas_bytes, int stream, int64_t p)
{
    return valid(e, atlas_bytes) && (e.stream == -1 || e.stream == stream) && e.first <= p && p <= e.last;
}

// one side of a fade: k pictures from the end the fade begins at
EFX_IPX_HD inline int fade(int64_t k, int len) { return len == 0 || k >= len ? 256 : (int)(256 * (k + 1)) / (len + 1); }
EFX_IPX_HD inline int gain(const efx_overlay_event& e, int64_t p)
{
    const int fi = fade(p - e.first, e.fade_in), fo = fade(e.last - p, e.fade_out);
    return (e.opacity * (fi < fo ? fi : fo) + 128) >> 8;
}

// t / 255 rounded half up, t in 0 .. 65025, and n / 1020, n in 0 .. 260610 (tests/test_overlay_model.py: the whole ranges)
EFX_IPX_HD inline uint32_t div255(uint32_t t) { return (t + 128 + ((t + 128) >> 8)) >> 8; }
EFX_IPX_HD inline uint32_t div1020(uint32_t n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(n, 4210753u);
#else
    return (uint32_t)(((uint64_t)n * 4210753u) >> 32);
#endif
}

// ---- words ----------------------------------------------------------------------------------------------------------------------
// unsigned sums, differences, products and shifts in both halves (the sums reach 65407, beyond a signed half)
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ inline u16x2 upk(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ inline uint32_t uun(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ inline uint32_t mul2(uint32_t a, uint32_t b) { return uun(upk(a) * upk(b)); }
__device__ inline uint32_t shr8_2(uint32_t a) { return uun(upk(a) >> u16x2{8, 8}); }
__device__ inline uint32_t add2(uint32_t a, uint32_t b) { return uun(upk(a) + upk(b)); }
__device__ inline uint32_t sub2(uint32_t a, uint32_t b) { return uun(upk(a) - upk(b)); }
#else
inline uint32_t add2(uint32_t a, uint32_t b) { return dpx::add2(a, b); }
inline uint32_t sub2(uint32_t a, uint32_t b) { return dpx::sub2(a, b); }
inline uint32_t mul2(uint32_t a, uint32_t b) { return (((a & 0xFFFFu) * (b & 0xFFFFu)) & 0xFFFFu) | (((a >> 16) * (b >> 16)) << 16); }
inline uint32_t shr8_2(uint32_t a) { return (a >> 8) & 0x00FF00FFu; }
#endif
EFX_IPX_HD inline int byte_of(uint32_t w, int i) { return (int)((w >> (8 * i)) & 0xFF); }

// a = (A g + 128) >> 8 for the four alpha bytes of a word (A g + 128 <= 65408: it fits a half)
EFX_IPX_HD inline uint32_t gain4(uint32_t A, int g)
{
    const uint32_t g2 = (uint32_t)g * 0x00010001u;
    const uint32_t lo = shr8_2(add2(mul2(dpx::widen(A, 0), g2), 0x00800080u));
    const uint32_t hi = shr8_2(add2(mul2(dpx::widen(A, 1), g2), 0x00800080u));
    return dpx::perm(hi, lo, dpx::kNarrow);
}

// Luma of two samples in the halves: y, a, c (the colour's luma) -> round(y (255 - a) + c a) / 255); every step fits 16 bits
EFX_IPX_HD inline uint32_t luma2(uint32_t y, uint32_t a, uint32_t c)
{
    const uint32_t t = add2(add2(mul2(y, sub2(0x00FF00FFu, a)), mul2(c, a)), 0x00800080u);
    return shr8_2(add2(t, shr8_2(t)));
}

// The colours of four columns of one row: luma in halves (columns 0, 1 and 2, 3), Cb and Cr as bytes of a word
struct Colour4 {
    uint32_t y01, y23, cb, cr;
};
EFX_IPX_HD inline Colour4 uniform4(uint32_t ycc)
{
    Colour4 c;
    c.y01 = c.y23 = (ycc & 0xFFu) * 0x00010001u;
    c.cb = ((ycc >> 8) & 0xFFu) * 0x01010101u, c.cr = ((ycc >> 16) & 0xFFu) * 0x01010101u;
    return c;
}
// ... of four RGBA pixels (R, G, B, A in a word's bytes from the low one), and their alpha bytes in *A
EFX_IPX_HD inline Colour4 rgba4(const uint32_t* px, uint32_t* A)
{
    const ipx::Matrix m = ipx::matrix(0);
    uint32_t v[4];
    for (int i = 0; i < 4; i++)
        v[i] = ipx::ycbcr(m, byte_of(px[i], 0), byte_of(px[i], 1), byte_of(px[i], 2));
    Colour4 c;
    c.y01 = (v[0] & 0xFFu) | ((v[1] & 0xFFu) << 16), c.y23 = (v[2] & 0xFFu) | ((v[3] & 0xFFu) << 16);
    c.cb = byte_of(v[0], 1) | (byte_of(v[1], 1) << 8) | (byte_of(v[2], 1) << 16) | ((uint32_t)byte_of(v[3], 1) << 24);
    c.cr = byte_of(v[0], 2) | (byte_of(v[1], 2) << 8) | (byte_of(v[2], 2) << 16) | ((uint32_t)byte_of(v[3], 2) << 24);
    *A = (px[0] >> 24) | ((px[1] >> 24) << 8) | ((px[2] >> 24) << 16) | ((px[3] >> 24) << 24);
    return c;
}

// Four luma samples of a row: y = the picture's word, a = the alphas (0 where absent)
EFX_IPX_HD inline uint32_t luma4(uint32_t y, uint32_t a, const Colour4& c)
{
    return dpx::perm(luma2(dpx::widen(y, 1), dpx::widen(a, 1), c.y23), luma2(dpx::widen(y, 0), dpx::widen(a, 0), c.y01), dpx::kNarrow);
}

// One chroma site: C = the picture's sample; columns i, i + 1 of rows 0 and 1 with alphas a0, a1 and chroma c0, c1 (words)
EFX_IPX_HD inline uint32_t site(uint32_t C, int i, uint32_t a0, uint32_t a1, uint32_t c0, uint32_t c1)
{
    const uint32_t p = byte_of(a0, i), q = byte_of(a0, i + 1), r = byte_of(a1, i), s = byte_of(a1, i + 1);
    const uint32_t S = p + q + r + s;
    const uint32_t N = p * byte_of(c0, i) + q * byte_of(c0, i + 1) + r * byte_of(c1, i) + s * byte_of(c1, i + 1);
    return div1020(C * (1020u - S) + N + 510u);
}
// The two sites of four columns: bytes 2 k, 2 k + 1 (k = 0, 1) of the chroma word
EFX_IPX_HD inline uint32_t sites2(uint32_t cw, int k, uint32_t a0, uint32_t a1, uint32_t c0, uint32_t c1)
{
    const uint32_t lo = site((cw >> (16 * k)) & 0xFFu, 0, a0, a1, c0, c1), hi = site((cw >> (16 * k + 8)) & 0xFFu, 2, a0, a1, c0, c1);
    return (cw & ~(0xFFFFu << (16 * k))) | ((lo | (hi << 8)) << (16 * k));
}

// ---- memory ---------------------------------------------------------------------------------------------------------------------
// Bytes pos .. pos + 15 of a bitmap row of `limit` bytes (pos may be negative: 0 comes out below the row's first byte and
// from limit on), never touching a byte in front of the row or at or beyond end (the atlas rounded up to 16).  The
// window must meet the row: pos < limit and pos + 16 > 0.
EFX_IPX_HD inline dpx::Chunk window16(const uint8_t* row, int pos, int limit, const uint8_t* end)
{
    const int skip = pos < 0 ? -pos : 0;  // 0 .. 15 bytes in front of the row
    const dpx::Chunk c = dpx::fetch16(row + (pos + skip), end, false);
    uint64_t lo = ((uint64_t)c.d[1] << 32) | c.d[0], hi = ((uint64_t)c.d[3] << 32) | c.d[2];
    if (skip >= 8) {
        hi = skip == 8 ? lo : lo << (8 * (skip - 8));
        lo = 0;
    } else if (skip > 0) {
        hi = (hi << (8 * skip)) | (lo >> (64 - 8 * skip));
        lo <<= 8 * skip;
    }
    const int n = limit - pos;  // bytes of the window that belong to the row
    if (n < 16) {
        if (n <= 8) {
            hi = 0;
            lo = n == 8 ? lo : lo & (((uint64_t)1 << (8 * n)) - 1);
        } else {
            hi &= ((uint64_t)1 << (8 * (n - 8))) - 1;
        }
    }
    dpx::Chunk out;
    out.d[0] = (uint32_t)lo, out.d[1] = (uint32_t)(lo >> 32), out.d[2] = (uint32_t)hi, out.d[3] = (uint32_t)(hi >> 32);
    return out;
}

// ---- one event at one picture ---------------------------------------------------------------------------------------------------
// What the lanes of a wave share about an active event: its clipped rectangle, gain and (A8) colour
struct Draw {
    const uint8_t* bitmap;   // atlas + offset
    int x, y, w;
    int x0, x1, y0, y1;      // the rectangle inside the picture: columns x0 .. x1 - 1, rows y0 .. y1 - 1
    uint32_t pitch;
    int g;
    bool rgba;
    uint32_t ycc;            // A8: ipx::ycbcr of the colour
};
// Whether any sample of the bitmap lies inside the picture
EFX_IPX_HD inline bool reaches(const efx_overlay_event& e)
{
    return e.x < kWidth && e.x + e.w > 0 && e.y < kHeight && e.y + e.h > 0;
}
// An event that reaches the picture, at the gain g (> 0) it has there
EFX_IPX_HD inline Draw draw_of(const efx_overlay_event& e, const uint8_t* atlas, int g)
{
    Draw d;
    d.bitmap = atlas + e.offset;
    d.x = e.x, d.y = e.y, d.w = e.w, d.pitch = e.pitch;
    d.x0 = e.x < 0 ? 0 : e.x, d.x1 = e.x + e.w < kWidth ? e.x + e.w : kWidth;
    d.y0 = e.y < 0 ? 0 : e.y, d.y1 = e.y + e.h < kHeight ? e.y + e.h : kHeight;
    d.g = g;
    d.rgba = e.kind == EFX_OVL_RGBA;
    d.ycc = ipx::ycbcr(ipx::matrix(0), (int)((e.colour >> 16) & 0xFF), (int)((e.colour >> 8) & 0xFF), (int)(e.colour & 0xFF));
    return d;
}
// the units (row by row) its rectangle lies between: a wave whose tile lies outside skips the event
EFX_IPX_HD inline int first_unit(const Draw& d) { return (d.y0 / kUnitRows) * kUnitsX + d.x0 / kUnitCols; }
EFX_IPX_HD inline int last_unit(const Draw& d) { return ((d.y1 - 1) / kUnitRows) * kUnitsX + (d.x1 - 1) / kUnitCols; }

// A lane's unit of a picture: 32 columns of two luma rows and the 16 sites of Cb and Cr below them, each chunk fetched
// when the first event touches it and stored, if it was fetched, when all events are done
struct Unit {
    dpx::Chunk y[2][2];  // [row][half]
    dpx::Chunk cb, cr;
    uint32_t have;       // bit 2 row + half: a luma chunk; bit 4: cb and cr
};
EFX_IPX_HD inline size_t luma_at(int X, int Y) { return (size_t)Y * kWidth + (size_t)X; }
EFX_IPX_HD inline size_t chroma_at(int X, int Y) { return (size_t)(Y / 2) * (kWidth / 2) + (size_t)(X / 2); }

EFX_IPX_HD inline void need(Unit* u, const uint8_t* pic, int X, int Y, int r, int h)
{
    const uint32_t bit = 1u << (2 * r + h);
    if (!(u->have & bit)) {
        memcpy(u->y[r][h].d, pic + luma_at(X + 16 * h, Y + r), 16);
        u->have |= bit;
    }
    if (!(u->have & 16u)) {
        memcpy(u->cb.d, pic + kCb + chroma_at(X, Y), 16);
        memcpy(u->cr.d, pic + kCr + chroma_at(X, Y), 16);
        u->have |= 16u;
    }
}
EFX_IPX_HD inline void store(const Unit& u, uint8_t* pic, int X, int Y)
{
    for (int r = 0; r < 2; r++)
        for (int h = 0; h < 2; h++)
            if (u.have & (1u << (2 * r + h)))
                memcpy(pic + luma_at(X + 16 * h, Y + r), u.y[r][h].d, 16);
    if (u.have & 16u) {
        memcpy(pic + kCb + chroma_at(X, Y), u.cb.d, 16);
        memcpy(pic + kCr + chroma_at(X, Y), u.cr.d, 16);
    }
}

// four columns of both rows and their two sites: word j of half h
EFX_IPX_HD inline void blend4(Unit* u, int h, int j, uint32_t a0, uint32_t a1, const Colour4& c0, const Colour4& c1)
{
    u->y[0][h].d[j] = luma4(u->y[0][h].d[j], a0, c0);
    u->y[1][h].d[j] = luma4(u->y[1][h].d[j], a1, c1);
    const int cw = 2 * h + (j >> 1), k = j & 1;
    u->cb.d[cw] = sites2(u->cb.d[cw], k, a0, a1, c0.cb, c1.cb);
    u->cr.d[cw] = sites2(u->cr.d[cw], k, a0, a1, c0.cr, c1.cr);
}

// One event on the unit whose first luma sample is (X, Y) of the picture at pic; end = the atlas rounded up to 16
EFX_IPX_HD inline void apply(Unit* u, const Draw& d, const uint8_t* pic, int X, int Y, const uint8_t* end)
{
    const bool in0 = Y >= d.y0 && Y < d.y1, in1 = Y + 1 >= d.y0 && Y + 1 < d.y1;
    if (!in0 && !in1)
        return;
    const uint8_t* row0 = d.bitmap + (size_t)(in0 ? Y - d.y : 0) * d.pitch;
    const uint8_t* row1 = d.bitmap + (size_t)(in1 ? Y + 1 - d.y : 0) * d.pitch;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int h = 0; h < 2; h++) {
        const int Xh = X + 16 * h;
        if (Xh >= d.x1 || Xh + 16 <= d.x0)
            continue;
        if (in0)
            need(u, pic, X, Y, 0, h);
        if (in1)
            need(u, pic, X, Y, 1, h);
        if (!d.rgba) {
            dpx::Chunk A0 = {}, A1 = {};
            if (in0)
                A0 = window16(row0, Xh - d.x, d.w, end);
            if (in1)
                A1 = window16(row1, Xh - d.x, d.w, end);
            const Colour4 c = uniform4(d.ycc);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int j = 0; j < 4; j++)
                blend4(u, h, j, gain4(A0.d[j], d.g), gain4(A1.d[j], d.g), c, c);
        } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int j = 0; j < 4; j++) {
                const int Xj = Xh + 4 * j;
                if (Xj >= d.x1 || Xj + 4 <= d.x0)
                    continue;
                dpx::Chunk P0 = {}, P1 = {};
                if (in0)
                    P0 = window16(row0, 4 * (Xj - d.x), 4 * d.w, end);
                if (in1)
                    P1 = window16(row1, 4 * (Xj - d.x), 4 * d.w, end);
                uint32_t A0, A1;
                const Colour4 c0 = rgba4(P0.d, &A0), c1 = rgba4(P1.d, &A1);
                blend4(u, h, j, gain4(A0, d.g), gain4(A1, d.g), c0, c1);
            }
        }
    }
}

}  // namespace ovx
}  // namespace efx
