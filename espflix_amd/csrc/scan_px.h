// scan_px.h -- arithmetic of k_scan (k_scan.hip, efx_detect_scan): what one lane adds to a frame's five sums for its strip
// of a band -- the three comb scores from one pass over the rows of a frame and of its predecessor, and the two field
// differences --, the label and the repeat of a frame from its sums, where a frame record counts in a stream's record,
// the verdict of a stream's record, and how a call is cut into items.
//
// Host + device: the kernels run exactly these functions -- a lane's whole share of an item is one call, because no lane
// needs a neighbour's samples -- and tests/scan_model_main.cpp performs whole calls with them on the host.  Everything is
// an integer function of the source bytes (the definition: include/efx.h, "scan type").  The comb score's packed halves,
// the 16-byte fetch and the masked luma row are telecine_px.h's and deint_px.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "efx.h"
#include "deint_px.h"
#include "telecine_px.h"

namespace efx {
namespace scpx {

constexpr int kChunk = tpx::kChunk;                // samples of a row a lane owns: one 16-byte access
constexpr int kBandRows = 32;                      // rows a lane walks down; even
constexpr int kWaveStrips = 64;                    // strips (a chunk's columns down a band) a measuring wave takes: one per lane
constexpr int kMeasureWaves = 4;                   // waves of a measuring workgroup: one frame's items go round them
constexpr int kCountWaves = 4;                     // streams a counting workgroup takes at a time, one per wave
constexpr int kCycle = 5;                          // phases of the repeat counters
constexpr int kSlots = 15;                         // counters of a record: five labels, then rep_top[5], then rep_bottom[5]

static_assert(sizeof(efx_scan_frame) == 48, "the frame record is 48 bytes");
static_assert(sizeof(efx_scan_rec) == 64, "the stream record is 64 bytes");
static_assert(sizeof(efx_scan_opts) == 56, "the options are a packed record");

// ---- the call ------------------------------------------------------------------------------------------------------------------
EFX_IPX_HD inline bool options_ok(const efx_scan_opts& o)
{
    return o.nt >= 0 && o.nt <= 255 && o.still >= 0 && o.still <= 4080 && o.prog >= 256 && o.prog <= 65535 && o.intl >= 256 && o.intl <= 65535 &&
           o.rep >= 256 && o.rep <= 65535 && (o.accumulate == 0 || o.accumulate == 1);
}
EFX_IPX_HD inline int chunks(int pw) { return (pw + kChunk - 1) / kChunk; }
EFX_IPX_HD inline int bands(int ph) { return (ph + kBandRows - 1) / kBandRows; }
// items of one frame's luma: 64 strips, counted chunk by chunk along a band and then band by band (as k_telecine_measure's)
EFX_IPX_HD inline int measure_items(int w, int h) { return (chunks(w) * bands(h) + kWaveStrips - 1) / kWaveStrips; }

// ---- label and repeat ------------------------------------------------------------------------------------------------------------
struct Sums {
    uint64_t cc, ctb, cbt, dt, db;
};
// The options of the label as the tests use them: still w h, and the three Q8 ratios
struct Rule {
    uint64_t still_wh;
    uint32_t prog, intl, rep;
};
EFX_IPX_HD inline Rule rule_of(const efx_scan_opts& o, int w, int h)
{
    Rule r;
    r.still_wh = (uint64_t)o.still * (uint64_t)w * (uint64_t)h;
    r.prog = (uint32_t)o.prog, r.intl = (uint32_t)o.intl, r.rep = (uint32_t)o.rep;
    return r;
}
// The label and the repeat of a frame that has a predecessor.  cc, ctb, cbt < 2^35, dt + db < 2^33, the ratios < 2^16: no
// product leaves 64 bits.
EFX_IPX_HD inline void label(const Sums& s, const Rule& r, int32_t* lab, int32_t* repeat)
{
    *repeat = EFX_SCAN_REPEAT_NONE;
    if (16 * (s.dt + s.db) < r.still_wh) {
        *lab = EFX_SCAN_STILL;
        return;
    }
    const uint64_t least = s.ctb < s.cbt ? s.ctb : s.cbt;
    if (256 * least > r.prog * s.cc)
        *lab = EFX_SCAN_PROGRESSIVE;
    else if (256 * s.cbt > r.intl * s.ctb)
        *lab = EFX_SCAN_TFF;
    else if (256 * s.ctb > r.intl * s.cbt)
        *lab = EFX_SCAN_BFF;
    else
        *lab = EFX_SCAN_UNDETERMINED;
    if (r.rep * s.dt < 256 * s.db)
        *repeat = EFX_SCAN_REPEAT_TOP;
    else if (r.rep * s.db < 256 * s.dt)
        *repeat = EFX_SCAN_REPEAT_BOTTOM;
}
// The record of a measured frame
EFX_IPX_HD inline efx_scan_frame measured(const Sums& s, bool has_prev, const Rule& r)
{
    efx_scan_frame f;
    f.comb = f.comb_tb = f.comb_bt = f.diff_top = f.diff_bottom = 0;
    f.label = EFX_SCAN_NONE, f.repeat = EFX_SCAN_REPEAT_NONE;
    if (has_prev) {
        f.comb = s.cc, f.comb_tb = s.ctb, f.comb_bt = s.cbt, f.diff_top = s.dt, f.diff_bottom = s.db;
        label(s, r, &f.label, &f.repeat);
    }
    return f;
}

// ---- count -----------------------------------------------------------------------------------------------------------------------
// A stream's record as its 16 words: the counter a frame's label adds to, and the one its repeat adds to, -1 = none
EFX_IPX_HD inline int phase_of(uint64_t first_frame, int index) { return (int)((first_frame % kCycle + (uint64_t)index) % kCycle); }
EFX_IPX_HD inline int label_slot(const efx_scan_frame& f) { return f.label >= EFX_SCAN_STILL && f.label <= EFX_SCAN_UNDETERMINED ? f.label - 1 : -1; }
EFX_IPX_HD inline int repeat_slot(const efx_scan_frame& f, int phase)
{
    return f.repeat == EFX_SCAN_REPEAT_TOP ? 5 + phase : (f.repeat == EFX_SCAN_REPEAT_BOTTOM ? 10 + phase : -1);
}
static_assert(offsetof(efx_scan_rec, rep_top) == 20 && offsetof(efx_scan_rec, rep_bottom) == 40 && offsetof(efx_scan_rec, reserved) == 60,
              "the counters are the record's first 15 words");

// ---- verdict ---------------------------------------------------------------------------------------------------------------------
// efx_scan_verdict
inline int verdict(const efx_scan_rec& r, int* first_field)
{
    const uint64_t n_moving = (uint64_t)r.n_prog + r.n_tff + r.n_bff + r.n_undet;
    int pt = 0, pb = 0;
    uint64_t tot = 0;
    for (int k = 0; k < kCycle; k++) {
        if (r.rep_top[k] > r.rep_top[pt])
            pt = k;
        if (r.rep_bottom[k] > r.rep_bottom[pb])
            pb = k;
        tot += (uint64_t)r.rep_top[k] + r.rep_bottom[k];
    }
    const uint64_t m = (uint64_t)r.rep_top[pt] + r.rep_bottom[pb];
    const int gap = (pb - pt + kCycle) % kCycle;
    if (r.rep_top[pt] >= 1 && r.rep_bottom[pb] >= 1 && m >= 4 && 4 * m >= 3 * tot && 5 * m >= n_moving && (gap == 2 || gap == 3)) {
        if (first_field)
            *first_field = gap == 2 ? EFX_FIELD_TOP : EFX_FIELD_BOTTOM;
        return EFX_SCAN_IS_TELECINED;
    }
    const uint64_t ordered = (uint64_t)r.n_tff + r.n_bff;
    const uint64_t lo = r.n_tff < r.n_bff ? r.n_tff : r.n_bff, hi = r.n_tff < r.n_bff ? r.n_bff : r.n_tff;
    if (ordered > r.n_prog && 4 * lo <= hi) {
        if (first_field)
            *first_field = r.n_tff > r.n_bff ? EFX_FIELD_TOP : EFX_FIELD_BOTTOM;
        return EFX_SCAN_IS_INTERLACED;
    }
    if (r.n_prog >= 1 && r.n_prog >= ordered)
        return EFX_SCAN_IS_PROGRESSIVE;
    return EFX_SCAN_IS_UNKNOWN;
}

// ---- measure ---------------------------------------------------------------------------------------------------------------------
// What the lanes of an item share: tpx::Measure with has_prev true (a frame with no predecessor is not walked)
typedef tpx::Measure Measure;
typedef tpx::Wide Wide;

// Rows r of F[t] and of F[t - 1], 16 samples each; a row outside the picture is 0 (and enters no sum)
struct Raw {
    dpx::Chunk c, p;
};
EFX_IPX_HD inline Raw fetch_rows(const Measure& m, int r, int X, int n)
{
    Raw v = {};
    if (r < 0 || r >= m.h)
        return v;
    v.c = tpx::luma_row(m, m.cur, r, X, n);
    v.p = tpx::luma_row(m, m.prev, r, X, n);
    return v;
}
// One row entering the window: widened once, and where the row lies in the band itself (counted) its difference from
// the predecessor's goes into d (v_sad_u8 on the loaded words)
EFX_IPX_HD inline void enter(const Raw& v, bool counted, Wide* c, Wide* p, uint32_t* d)
{
    *c = tpx::widen(v.c), *p = tpx::widen(v.p);
    if (counted) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 4; i++)
            *d += dpx::sad4(v.c.d[i], v.p.d[i]);
    }
}

// max(0, |a - b| - 6 nt) in each half; a, b in 0 .. 1530
EFX_IPX_HD inline uint32_t over2(uint32_t a, uint32_t b, uint32_t thr2)
{
    const uint32_t d = dpx::sub2(a, b);
    return tpx::subsat2(dpx::max2(d, dpx::sub2(0u, d)), thr2);
}
EFX_IPX_HD inline uint32_t fold2(uint32_t s) { return (s & 0xFFFFu) + (s >> 16); }

// The three scores' terms of the 16 samples of row y from rows y - 2 .. y + 2 of F[t] (c) and of F[t - 1] (p): with
//   S_X = X[y-2] + 4 X[y] + X[y+2]   and   A_X = 3 (X[y-1] + X[y+1])      (both at most 1530)
// cc takes |S_c - A_c|, u1 |S_c - A_p| (the row and its field from F[t], the other field from F[t - 1]) and u2 |S_p - A_c|:
// four partial sums and three differences for three scores.  A sum of eight terms fits a half.
EFX_IPX_HD inline void comb_rows(const Wide& cm2, const Wide& cm1, const Wide& c0, const Wide& cp1, const Wide& cp2, const Wide& pm2,
                                 const Wide& pm1, const Wide& p0, const Wide& pp1, const Wide& pp2, uint32_t thr2, uint32_t* cc, uint32_t* u1,
                                 uint32_t* u2)
{
    uint32_t s0 = 0, s1 = 0, s2 = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) {
        const uint32_t sc = dpx::add2(dpx::add2(cm2.h[i], cp2.h[i]), tpx::mul2(c0.h[i], 4));
        const uint32_t ac = tpx::mul2(dpx::add2(cm1.h[i], cp1.h[i]), 3);
        const uint32_t sp = dpx::add2(dpx::add2(pm2.h[i], pp2.h[i]), tpx::mul2(p0.h[i], 4));
        const uint32_t ap = tpx::mul2(dpx::add2(pm1.h[i], pp1.h[i]), 3);
        s0 = dpx::add2(s0, over2(sc, ac, thr2));
        s1 = dpx::add2(s1, over2(sc, ap, thr2));
        s2 = dpx::add2(s2, over2(sp, ac, thr2));
    }
    *cc += fold2(s0), *u1 += fold2(s1), *u2 += fold2(s2);
}

// Five 32-bit sums of a lane over a band
struct Band {
    uint32_t cc, ctb, cbt, dt, db;
};

// One step of a lane's walk: rows y and y + 1 of the band, from windows of six rows of F[t] (C) and of F[t - 1] (P) that
// hold rows y - 2 .. y + 3.  The windows are rings: row y - 2 + s lies in slot (s + 2 K) mod 6, K = the step's number mod
// 3, so that a step moves no row -- the two rows it adds take the slots of the two that leave.  The four rows the next
// step needs are asked for before this step's arithmetic begins.  Rows y - 2 .. y + 2 serve row y; rows 0, 1, h - 2 and
// h - 1 have no score.  On an even row u1 belongs to ctb and u2 to cbt, on an odd row the other way round; an even row's
// difference goes to dt, an odd row's to db.
template <int K>
EFX_IPX_HD inline void step(const Measure& m, int y, int y1, int X, int n, Wide (&C)[6], Wide (&P)[6], Band* b)
{
    constexpr int s0 = (2 * K) % 6, s1 = (2 * K + 1) % 6, s2 = (2 * K + 2) % 6, s3 = (2 * K + 3) % 6, s4 = (2 * K + 4) % 6, s5 = (2 * K + 5) % 6;
    const bool more = y + 2 < y1, in = y + 4 < y1;
    Raw v4 = {}, v5 = {};
    if (more)
        v4 = fetch_rows(m, y + 4, X, n), v5 = fetch_rows(m, y + 5, X, n);
    if (y >= 2 && y <= m.h - 3)
        comb_rows(C[s0], C[s1], C[s2], C[s3], C[s4], P[s0], P[s1], P[s2], P[s3], P[s4], m.thr2, &b->cc, &b->ctb, &b->cbt);
    if (y >= 2 && y + 1 <= m.h - 3)
        comb_rows(C[s1], C[s2], C[s3], C[s4], C[s5], P[s1], P[s2], P[s3], P[s4], P[s5], m.thr2, &b->cc, &b->cbt, &b->ctb);
    enter(v4, in, &C[s0], &P[s0], &b->dt);
    enter(v5, in, &C[s1], &P[s1], &b->db);
}

// What lane `lane` of the wave that takes item `item` adds to the frame's sums: one strip, three steps to a turn of the
// rings.
EFX_IPX_HD inline void measure_lane(const Measure& m, int item, int lane, Sums* sums)
{
    const int strip = item * kWaveStrips + lane, across = chunks(m.w);
    if (strip >= across * bands(m.h))
        return;
    const int X = strip % across * kChunk, n = m.w - X;
    const int y0 = strip / across * kBandRows;
    const int y1 = y0 + kBandRows < m.h ? y0 + kBandRows : m.h;  // even: h is; at least y0 + 4
    Wide C[6], P[6];
    Band b = {0, 0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 3; i++) {
        const int r = y0 - 2 + 2 * i;
        const bool in = i > 0;  // rows y0 .. y0 + 3 lie in the band, rows y0 - 2 and y0 - 1 above it
        enter(fetch_rows(m, r, X, n), in, &C[2 * i], &P[2 * i], &b.dt);
        enter(fetch_rows(m, r + 1, X, n), in, &C[2 * i + 1], &P[2 * i + 1], &b.db);
    }
    for (int y = y0; y < y1; y += 6) {
        step<0>(m, y, y1, X, n, C, P, &b);
        if (y + 2 >= y1)
            break;
        step<1>(m, y + 2, y1, X, n, C, P, &b);
        if (y + 4 >= y1)
            break;
        step<2>(m, y + 4, y1, X, n, C, P, &b);
    }
    sums->cc += b.cc, sums->ctb += b.ctb, sums->cbt += b.cbt, sums->dt += b.dt, sums->db += b.db;
}

}  // namespace scpx
}  // namespace efx
