// telecine_px.h -- arithmetic of k_telecine (k_telecine.hip, efx_detelecine): the comb score of a woven luma row on packed
// 16-bit halves, what one lane adds to a frame's three sums for its strip of a band, the decision of a cycle of five
// frames, the rows one lane copies into an output picture, and how a call is cut into items.
//
// Host + device: the kernels run exactly these functions -- a lane's whole share of an item is one call, because no lane
// needs a neighbour's samples -- and tests/telecine_model_main.cpp performs whole calls with them on the host.  Everything
// is an integer function of the source bytes (the definition: include/efx.h, "telecined sources").
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "efx.h"
#include "deint_px.h"

namespace efx {
namespace tpx {

constexpr int kChunk = dpx::kChunk;                // samples of a row a lane owns: one 16-byte access
constexpr int kBandRows = 32;                      // rows a lane walks down; even
constexpr int kWaveStrips = 64;                    // strips (a chunk's columns down a band) a measuring wave takes: one per lane
constexpr int kCycle = 5;                          // frames of a decimation cycle
constexpr int kMeasureWaves = 4;                   // waves of a measuring workgroup: one frame's items go round them
constexpr int kWeaveWaves = 4;                     // items a weaving workgroup takes at a time, one per wave
constexpr uint64_t kNoDiff = ~(uint64_t)0;         // D of a frame with no predecessor

static_assert(sizeof(efx_telecine_info) == 32, "the record is 32 bytes");

// ---- the call ------------------------------------------------------------------------------------------------------------------
// frames of a call that are processed, -1 for rejected arguments
EFX_IPX_HD inline int processed(int n_frames, int lead)
{
    return n_frames < 1 || (lead != 0 && lead != 1) || lead >= n_frames ? -1 : n_frames - lead;
}
// efx_detelecine_count
EFX_IPX_HD inline int count(int n_frames, int lead)
{
    const int n = processed(n_frames, lead);
    return n < 0 ? -1 : n - n / kCycle;
}

EFX_IPX_HD inline int chunks(int pw) { return (pw + kChunk - 1) / kChunk; }
EFX_IPX_HD inline int bands(int ph) { return (ph + kBandRows - 1) / kBandRows; }
// items of one frame's luma for the measure: 64 strips, counted chunk by chunk along a band and then band by band.  The
// comb is vertical, so a lane needs no neighbour and the lanes of a wave may walk different bands: a picture whose rows are
// no multiple of 64 chunks (720 samples: 45) still fills its waves
EFX_IPX_HD inline int measure_items(int w, int h) { return (chunks(w) * bands(h) + kWaveStrips - 1) / kWaveStrips; }
// items of one output picture for the weave: bands of the luma plane, then of the chroma planes.  Of a semi-planar surface
// one item makes a band of Cb and of Cr from one fetch of the pair rows; of a planar one Cb's and Cr's bands are items of
// their own, side by side.
EFX_IPX_HD inline int weave_items(const efx_surface& s)
{
    return bands(s.height) + (s.layout == EFX_SURF_SEMI8 ? 1 : 2) * bands(s.height / 2);
}

// ---- the comb score --------------------------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// a * k in each half (v_pk_mul_lo_u16, or folded into v_pk_mad_i16 with the add that follows)
__device__ inline uint32_t mul2(uint32_t a, int k) { return dpx::un(dpx::pk(a) * dpx::s16x2{(short)k, (short)k}); }
// max(0, a - b) in each half, a and b not negative: v_pk_sub_u16 with clamp
__device__ inline uint32_t subsat2(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
#else
inline uint32_t mul2(uint32_t a, int k) { return dpx::each2(a, 0, [k](int x, int) { return x * k; }); }
inline uint32_t subsat2(uint32_t a, uint32_t b) { return dpx::each2(a, b, [](int x, int y) { return x > y ? x - y : 0; }); }
#endif

// 16 samples of a row in 16-bit halves
struct Wide {
    uint32_t h[8];
};
EFX_IPX_HD inline Wide widen(const dpx::Chunk& c)
{
    Wide w;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++)
        w.h[2 * i] = dpx::widen(c.d[i], 0), w.h[2 * i + 1] = dpx::widen(c.d[i], 1);
    return w;
}

// 6 * nt in both halves
EFX_IPX_HD inline uint32_t threshold2(int nt) { return (uint32_t)(6 * nt) * 0x00010001u; }

// The sum of max(0, v - 6 nt) over the 16 samples of row y of a woven plane, from its rows y - 2 .. y + 2.  v is at most
// 1530 and the sum of eight of them fits a half.
EFX_IPX_HD inline uint32_t comb_row(const Wide& m2, const Wide& m1, const Wide& c0, const Wide& p1, const Wide& p2, uint32_t thr2)
{
    uint32_t s = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) {
        const uint32_t a = dpx::add2(dpx::add2(m2.h[i], p2.h[i]), mul2(c0.h[i], 4));
        const uint32_t b = mul2(dpx::add2(m1.h[i], p1.h[i]), 3);
        const uint32_t d = dpx::sub2(a, b);
        s = dpx::add2(s, subsat2(dpx::max2(d, dpx::sub2(0u, d)), thr2));
    }
    return (s & 0xFFFFu) + (s >> 16);
}

// The score of a whole plane held in memory (the definition, through comb_row): rows of w bytes, pitch apart
EFX_IPX_HD inline uint64_t score_plane(const uint8_t* y, size_t pitch, int w, int h, int nt)
{
    uint64_t sum = 0;
    const uint32_t thr2 = threshold2(nt);
    for (int r = 2; r <= h - 3; r++)
        for (int x = 0; x < w; x += kChunk) {
            Wide rows[5];
            for (int k = 0; k < 5; k++) {
                uint8_t b[kChunk] = {};
                memcpy(b, y + (size_t)(r - 2 + k) * pitch + x, (size_t)(w - x < kChunk ? w - x : kChunk));
                dpx::Chunk c;
                memcpy(c.d, b, kChunk);
                rows[k] = widen(c);
            }
            sum += comb_row(rows[0], rows[1], rows[2], rows[3], rows[4], thr2);
        }
    return sum;
}

// ---- measure ---------------------------------------------------------------------------------------------------------------------
struct Sums {
    uint64_t cc, cp, d;
};

// What the lanes of an item share
struct Measure {
    const uint8_t *cur, *prev;  // F[t] and F[t - 1] (prev is never read when has_prev is false)
    bool has_prev;
    size_t end;                 // bytes of an image that may be read: the surface's, rounded up to 16
    dpx::PlaneAt at;            // the luma plane
    int w, h;
    uint32_t thr2;
};

// samples X .. X + 15 of luma row r, the samples from column w on as 0 (so that they add nothing to any sum)
EFX_IPX_HD inline dpx::Chunk luma_row(const Measure& m, const uint8_t* img, int r, int X, int n)
{
    dpx::Chunk c = dpx::fetch_row(m.at, img, m.end, r, X, n);
    if (n < kChunk) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 4; i++) {
            const int k = n - 4 * i;
            c.d[i] &= k >= 4 ? ~0u : (k <= 0 ? 0u : (1u << (8 * k)) - 1u);
        }
    }
    return c;
}

// One row entering the window.  EARLY: the row belongs to the earlier field E (parity p): both candidates take it from
// F[t], and where the row lies in the band itself (counted) its difference from F[t - 1]'s goes into D.  Otherwise it
// belongs to L: the second candidate takes it from F[t - 1].
struct Raw {
    dpx::Chunk c, p;
};
template <bool EARLY>
EFX_IPX_HD inline Raw fetch_rows(const Measure& m, int r, bool counted, int X, int n)
{
    Raw v = {};
    if (r < 0 || r >= m.h)
        return v;
    v.c = luma_row(m, m.cur, r, X, n);
    if (m.has_prev && (!EARLY || counted))
        v.p = luma_row(m, m.prev, r, X, n);
    return v;
}
template <bool EARLY>
EFX_IPX_HD inline void enter(const Raw& v, bool counted, Wide* c, Wide* l, uint32_t* d)
{
    *c = widen(v.c);
    if (EARLY) {
        if (counted) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int i = 0; i < 4; i++)
                *d += dpx::sad4(v.c.d[i], v.p.d[i]);
        }
    } else {
        *l = widen(v.p);
    }
}

// Slot I of the second candidate's window, weave(E[t], L[t - 1]): F[t]'s row where the slot's parity is P, else F[t - 1]'s
template <int P, int I>
EFX_IPX_HD inline const Wide& woven(const Wide (&C)[6], const Wide (&L)[3]) { return (I & 1) == P ? C[I] : L[I >> 1]; }

// What lane `lane` of the wave that takes item `item` adds to the frame's sums: one strip.  P = the parity of
// the earlier field.  A window of six rows of F[t] (C) and of the three L rows of F[t - 1] among them (L) slides down the
// band two rows at a time; the two rows the next step adds are asked for before this step's arithmetic begins.  Rows
// y - 2 .. y + 2 of the image serve row y; rows 0, 1, h - 2 and h - 1 have no score.  For a row of either parity the two
// candidates share the partial sum of the rows that both take from F[t].
template <int P>
EFX_IPX_HD inline void measure_lane(const Measure& m, int item, int lane, Sums* sums)
{
    const int strip = item * kWaveStrips + lane, across = chunks(m.w);
    if (strip >= across * bands(m.h))
        return;
    const int X = strip % across * kChunk, n = m.w - X;
    const int y0 = strip / across * kBandRows;
    const int y1 = y0 + kBandRows < m.h ? y0 + kBandRows : m.h;  // even: h is; at least y0 + 4
    constexpr bool kEven = P == 0, kOdd = P == 1;                // whether the even / the odd rows are E's
    Wide C[6], L[3], none;
    uint32_t cc = 0, cp = 0, d = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 3; i++) {
        const int r = y0 - 2 + 2 * i;
        const bool in = i > 0;  // rows y0 .. y0 + 3 lie in the band, rows y0 - 2 and y0 - 1 above it
        enter<kEven>(fetch_rows<kEven>(m, r, in, X, n), in, &C[2 * i], kEven ? &none : &L[i], &d);
        enter<kOdd>(fetch_rows<kOdd>(m, r + 1, in, X, n), in, &C[2 * i + 1], kOdd ? &none : &L[i], &d);
    }
    for (int y = y0; y < y1; y += 2) {
        // (slots 0 .. 5 hold rows y - 2 .. y + 3)
        const bool more = y + 2 < y1, in = y + 4 < y1;
        Raw v4 = {}, v5 = {};
        if (more)
            v4 = fetch_rows<kEven>(m, y + 4, in, X, n), v5 = fetch_rows<kOdd>(m, y + 5, in, X, n);
        if (y >= 2 && y <= m.h - 3) {
            cc += comb_row(C[0], C[1], C[2], C[3], C[4], m.thr2);
            cp += comb_row(woven<P, 0>(C, L), woven<P, 1>(C, L), woven<P, 2>(C, L), woven<P, 3>(C, L), woven<P, 4>(C, L), m.thr2);
        }
        if (y >= 2 && y + 1 <= m.h - 3) {
            cc += comb_row(C[1], C[2], C[3], C[4], C[5], m.thr2);
            cp += comb_row(woven<P, 1>(C, L), woven<P, 2>(C, L), woven<P, 3>(C, L), woven<P, 4>(C, L), woven<P, 5>(C, L), m.thr2);
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 4; i++)
            C[i] = C[i + 2];
        L[0] = L[1], L[1] = L[2];
        enter<kEven>(v4, in, &C[4], kEven ? &none : &L[2], &d);
        enter<kOdd>(v5, in, &C[5], kOdd ? &none : &L[2], &d);
    }
    sums->cc += cc, sums->cp += cp, sums->d += d;
}

// The record of a measured frame before the decision
EFX_IPX_HD inline efx_telecine_info measured(const Sums& s, bool has_prev)
{
    efx_telecine_info r;
    r.comb_c = s.cc, r.comb_p = has_prev ? s.cp : 0, r.diff = has_prev ? s.d : kNoDiff;
    r.match = 0, r.out = -1;
    return r;
}

// ---- decide ----------------------------------------------------------------------------------------------------------------------
// The records r[0 .. n - 1] of one cycle (n = 5, or fewer in a last partial cycle) whose first kept frame is output
// first_out: match and out
EFX_IPX_HD inline void decide_cycle(efx_telecine_info* r, int n, int first_out)
{
    int drop = -1;
    if (n == kCycle) {
        drop = 0;
        for (int k = 1; k < kCycle; k++)
            if (r[k].diff < r[drop].diff)
                drop = k;
    }
    for (int k = 0; k < n; k++) {
        r[k].match = r[k].diff != kNoDiff && 4 * r[k].comb_p < 3 * r[k].comb_c ? 1 : 0;
        r[k].out = k == drop ? -1 : first_out++;
    }
}

// ---- weave -----------------------------------------------------------------------------------------------------------------------
constexpr int kWeaveDepth = 4;  // chunks a lane has in flight

// What the lanes of an item share
struct Weave {
    const uint8_t* even;        // the image that supplies the even rows: F[t] or F[t - match] by the parity
    ptrdiff_t odd;              // ... and from there to the image that supplies the odd rows (0, or one source stride either way)
    size_t end;
    dpx::PlaneAt at;            // the plane the item reads (for `both`: the pair plane, not de-interleaved by the fetch)
    bool both;                  // a semi-planar surface's chroma: Cb and Cr from one fetch
    bool swap;                  // ... whose pairs are (Cr, Cb)
    uint8_t *to, *to2;          // row 0 of the plane in the output picture (to2: Cr's for `both`)
    int pw, chunks;             // samples and chunks of a row
    int y0, total;              // the band's first row and its chunks
};
EFX_IPX_HD inline Weave weave_of(const efx_surface& s, const uint8_t* cur, const uint8_t* other, size_t end, uint8_t* out, int parity, int k)
{
    Weave w;
    const int lb = bands(s.height);
    int plane = 0, band = k;
    w.both = false;
    if (k >= lb && s.layout == EFX_SURF_SEMI8)
        plane = 1, band = k - lb, w.both = true;
    else if (k >= lb)
        plane = 1 + ((k - lb) & 1), band = (k - lb) >> 1;
    const int ph = dpx::plane_h(s.height, plane);
    w.pw = dpx::plane_w(s.width, plane), w.chunks = chunks(w.pw);
    w.even = parity == 0 ? cur : other, w.odd = parity == 0 ? other - cur : cur - other;
    w.end = end;
    w.at = dpx::plane_at(s, plane);
    w.swap = s.swap_uv != 0;
    w.to = out + dpx::out_plane(s.width, s.height, plane), w.to2 = out + dpx::out_plane(s.width, s.height, 2);
    w.y0 = band * kBandRows;
    const int y1 = w.y0 + kBandRows < ph ? w.y0 + kBandRows : ph;
    w.total = (y1 - w.y0) * w.chunks;
    return w;
}

// Chunk i of the band, counted row by row: fetched, then stored.  A lane's chunks lie in different rows, so a wave wastes
// no lane on a narrow plane.
struct Piece {
    dpx::Chunk a, b;
};
EFX_IPX_HD inline Piece weave_fetch(const Weave& w, int i)
{
    Piece p = {};
    if (i >= w.total)
        return p;
    const int y = w.y0 + i / w.chunks, X = (i % w.chunks) * kChunk, n = w.pw - X;
    const uint8_t* img = w.even + (y & 1 ? w.odd : 0);
    if (!w.both) {
        p.a = dpx::fetch_row(w.at, img, w.end, y, X, n);
        return p;
    }
    // 16 pairs: 32 bytes, the even ones one plane's samples and the odd ones the other's
    const size_t row = w.at.first + (size_t)y * w.at.pitch;
    const bool safe = row + ((w.at.row_bytes + 15) & ~(size_t)15) <= w.end;
    const uint8_t* at = img + row + 2 * (size_t)X;
    const dpx::Chunk p0 = dpx::fetch16(at, img + w.end, safe);
    dpx::Chunk p1 = {};
    if (n > 8)
        p1 = dpx::fetch16(at + 16, img + w.end, safe);
    const uint32_t first = w.swap ? spx::kPickOdd : spx::kPickEven, second = w.swap ? spx::kPickEven : spx::kPickOdd;
    p.a.d[0] = dpx::perm(p0.d[1], p0.d[0], first), p.a.d[1] = dpx::perm(p0.d[3], p0.d[2], first);
    p.a.d[2] = dpx::perm(p1.d[1], p1.d[0], first), p.a.d[3] = dpx::perm(p1.d[3], p1.d[2], first);
    p.b.d[0] = dpx::perm(p0.d[1], p0.d[0], second), p.b.d[1] = dpx::perm(p0.d[3], p0.d[2], second);
    p.b.d[2] = dpx::perm(p1.d[1], p1.d[0], second), p.b.d[3] = dpx::perm(p1.d[3], p1.d[2], second);
    return p;
}
EFX_IPX_HD inline void weave_store(const Weave& w, int i, const Piece& p)
{
    if (i >= w.total)
        return;
    const int y = w.y0 + i / w.chunks, X = (i % w.chunks) * kChunk, n = w.pw - X;
    const size_t at = (size_t)y * w.pw + X;
    dpx::store_chunk(w.to + at, p.a, n);
    if (w.both)
        dpx::store_chunk(w.to2 + at, p.b, n);
}

// What lane `lane` copies for item k of an output picture: the rows of parity p of each plane from F[t] (cur), the others
// from F[t - match] (other); every row of a plane is fetched once and stored once.  out = the output picture.
EFX_IPX_HD inline void weave_lane(const efx_surface& s, const uint8_t* cur, const uint8_t* other, size_t end, uint8_t* out, int parity, int k,
                                  int lane)
{
    const Weave w = weave_of(s, cur, other, end, out, parity, k);
    for (int i = lane; i < w.total; i += 64 * kWeaveDepth) {
        const Piece p0 = weave_fetch(w, i), p1 = weave_fetch(w, i + 64), p2 = weave_fetch(w, i + 128), p3 = weave_fetch(w, i + 192);
        weave_store(w, i, p0);
        weave_store(w, i + 64, p1);
        weave_store(w, i + 128, p2);
        weave_store(w, i + 192, p3);
    }
}
static_assert(kWeaveDepth == 4, "weave_lane is written out for four");

}  // namespace tpx
}  // namespace efx
