// k_deint.hip -- interlaced sources to progressive pictures (efx_deinterlace): every line a field lacks is made from the
// lines above and below it and from the neighbouring fields, by the rule of include/efx.h, "interlaced sources".  The
// arithmetic is deint_px.h's: an integer function of the source bytes, the same functions on the host and here.
//
// k_deint   one launch per call.  An item is a band of 16 rows of a column tile of 992 samples of one plane of one source
//           frame, and a wave takes an item: four items per workgroup, no LDS, no barrier.  In field mode the wave makes
//           that band of both outputs of the frame, so the three frames it needs are read once, not twice.
//           Columns.  A lane owns 16 samples of a row: one 16-byte load (two for a row of NV12 pairs, de-interleaved with
//           v_perm_b32), at whatever alignment the plane's offset and pitch give, and one 16-byte store per output row;
//           only a row's last, partial chunk leaves in smaller pieces.  The rule looks 3 samples to either side: the word
//           before and the word after a lane's own four come from the neighbouring lanes (two lane shuffles per cur
//           row), and the first and last lane of the wave only fetch -- the tile is 62 chunks wide, the wave reads 64.
//           Chroma planes of up to 480 samples a row (SD) share a wave, Cb in lanes 0 .. 31 and Cr in lanes 32 .. 63, each
//           half with its own two halo lanes: two items of 25 busy lanes become one of 50.
//           The picture-edge clamp is done on those words (dpx::clamp_cols), once per cur row.
//           Rows.  A register window of six rows of prev, cur and next slides down the band two rows at a time: every cur
//           row serves the missing rows above and below it, every B / A row three of them.  The two rows the next step
//           adds are asked for before this step's arithmetic begins.  Registers, not LDS: the only sharing between lanes
//           is the two halo words, and a window in LDS would be written and read back by the lane that owns it.
//           Arithmetic.  A word holds four samples.  score(j) is v_sad_u8 of two 3-byte windows, each cut out of a pair
//           of words and zero-extended by one v_perm_b32; the search is per sample; the temporal part runs two samples at
//           a time in 16-bit halves (v_pk_*_i16).
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "deint_px.h"

namespace efx {

namespace {

struct Wave {
    const uint8_t *prev, *cur, *next;  // the three source images
    size_t end;                        // bytes of an image that may be read: the surface's, rounded up to 16
    dpx::PlaneAt at;                   // where the plane's rows lie in an image
    uint8_t *out0, *out1;              // the lane's chunk in row 0 of the plane, in each output of the frame
    // per row parity (even, odd), picked with selects so that nothing here is indexed at run time:
    int keep0, keep1;                  // the output that keeps such rows, -1 = none; the other parity's keeper lacks them
    bool prev0, prev1, next0, next1;   // whether any missing row reads such rows of prev / next
    int pw, ph;
    int X, n;                          // the lane's first column, and the columns from there on
    bool active, writes;
};

struct Raw {
    dpx::Chunk c, p, n;
};

__device__ inline Raw fetch(const Wave& w, int r)
{
    Raw v = {};
    const int rr = dpx::reflect(r, w.ph);
    if (w.active) {
        v.c = dpx::fetch_row(w.at, w.cur, w.end, rr, w.X, w.n);
        if (rr & 1 ? w.prev1 : w.prev0)
            v.p = dpx::fetch_row(w.at, w.prev, w.end, rr, w.X, w.n);
        if (rr & 1 ? w.next1 : w.next0)
            v.n = dpx::fetch_row(w.at, w.next, w.end, rr, w.X, w.n);
    }
    return v;
}

// A cur row with its halo words, clamped at the picture's edges (every lane of the wave comes here: the shuffles)
__device__ inline dpx::Ext widen_row(const Wave& w, const dpx::Chunk& c)
{
    dpx::Ext x;
    x.e[0] = __shfl_up(c.d[3], 1);
    x.e[5] = __shfl_down(c.d[0], 1);
#pragma unroll
    for (int i = 0; i < 4; i++)
        x.e[1 + i] = c.d[i];
    if (w.active)
        dpx::clamp_cols(&x, w.X, w.n);
    return x;
}

// Row y, the window's slot K: copied to the output that keeps its parity, made for the output that lacks it
template <int K>
__device__ inline void make_row(const Wave& w, int y, const dpx::Ext (&C)[6], const dpx::Chunk (&P)[6], const dpx::Chunk (&N)[6])
{
    if (!w.writes)
        return;
    const int q = y & 1;
    const size_t row = (size_t)y * w.pw;
    const int kp = q ? w.keep1 : w.keep0, ms = q ? w.keep0 : w.keep1;
    if (kp >= 0) {
        dpx::Chunk c;
#pragma unroll
        for (int i = 0; i < 4; i++)
            c.d[i] = C[K].e[1 + i];
        dpx::store_chunk((kp ? w.out1 : w.out0) + row, c, w.n);
    }
    if (ms >= 0) {
        const bool first = ms == 0;  // B = prev, A = cur; else B = cur, A = next
        dpx::Chunk o;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            dpx::Rows r;
#pragma unroll
            for (int j = 0; j < 3; j++)
                r.up[j] = C[K - 1].e[i + j], r.dn[j] = C[K + 1].e[i + j];
            r.pu = P[K - 1].d[i], r.pd = P[K + 1].d[i];
            r.nu = N[K - 1].d[i], r.nd = N[K + 1].d[i];
            r.bm = first ? P[K - 2].d[i] : C[K - 2].e[1 + i];
            r.b0 = first ? P[K].d[i] : C[K].e[1 + i];
            r.bp = first ? P[K + 2].d[i] : C[K + 2].e[1 + i];
            r.am = first ? C[K - 2].e[1 + i] : N[K - 2].d[i];
            r.a0 = first ? C[K].e[1 + i] : N[K].d[i];
            r.ap = first ? C[K + 2].e[1 + i] : N[K + 2].d[i];
            o.d[i] = dpx::missing4(r);
        }
        dpx::store_chunk((ms ? w.out1 : w.out0) + row, o, w.n);
    }
}

// SHARED: Cb and Cr in the two halves of the wave (the plane, and with it where rows lie, then differs from lane to lane;
// everywhere else it is the same for the wave and its arithmetic is scalar)
template <bool SHARED>
__device__ __forceinline__ void deint_item(const DeintArgs& a, size_t frame, dpx::Item it)
{
    const int lane = threadIdx.x & 63;
    const efx_surface& s = a.s;
    it.shared = SHARED;
    const dpx::Place at = dpx::place(it, lane);
    Wave w;
    w.at = dpx::plane_at(s, at.plane);
    w.pw = dpx::plane_w(s.width, it.plane), w.ph = dpx::plane_h(s.height, it.plane);
    w.X = at.X;
    w.n = w.pw - w.X;
    w.active = w.X >= 0 && w.n > 0;
    w.writes = w.active && !at.halo;

    const size_t stream = frame / (size_t)a.frames_out;
    const int jo = (int)(frame - stream * (size_t)a.frames_out), j = a.lead + jo;
    const uint8_t* first = a.src + stream * (size_t)a.n_frames * a.src_stride;
    w.cur = first + (size_t)j * a.src_stride;
    w.prev = first + (size_t)(j > 0 ? j - 1 : j) * a.src_stride;
    w.next = first + (size_t)(j + 1 < a.n_frames ? j + 1 : j) * a.src_stride;
    w.end = (s.bytes + 15) / 16 * 16;
    const size_t n_out = (size_t)a.frames_out * a.per_frame;
    uint8_t* o0 = a.dst + (stream * n_out + (size_t)jo * a.per_frame) * a.dst_stride + dpx::out_plane(s.width, s.height, at.plane) + w.X;
    w.out0 = o0, w.out1 = o0 + a.dst_stride;
    w.keep0 = dpx::keeper(a.first_field, a.per_frame, 0), w.keep1 = dpx::keeper(a.first_field, a.per_frame, 1);
    // (rows of parity q are read by the missing rows of the other parity -- t1, t2 -- and, as B = prev of output 0 or
    // A = next of output 1, by the missing rows of their own)
    w.prev0 = w.keep0 >= 0 || w.keep1 == 0, w.prev1 = w.keep1 >= 0 || w.keep0 == 0;
    w.next0 = w.keep0 >= 0 || w.keep1 == 1, w.next1 = w.keep1 >= 0 || w.keep0 == 1;

    const int y0 = it.band * dpx::kBandRows;
    const int y1 = y0 + dpx::kBandRows < w.ph ? y0 + dpx::kBandRows : w.ph;  // even: ph is
    dpx::Ext C[6];
    dpx::Chunk P[6], N[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const Raw v = fetch(w, y0 - 2 + i);
        C[i] = widen_row(w, v.c), P[i] = v.p, N[i] = v.n;
    }
    for (int y = y0; y < y1; y += 2) {
        // (slots 0 .. 5 hold rows y - 2 .. y + 3; the rows of the next step are asked for now)
        const bool more = y + 2 < y1;
        Raw v4 = {}, v5 = {};
        if (more)
            v4 = fetch(w, y + 4), v5 = fetch(w, y + 5);
        make_row<2>(w, y, C, P, N);
        make_row<3>(w, y + 1, C, P, N);
#pragma unroll
        for (int i = 0; i < 4; i++)
            C[i] = C[i + 2], P[i] = P[i + 2], N[i] = N[i + 2];
        C[4] = widen_row(w, v4.c), P[4] = v4.p, N[4] = v4.n;
        C[5] = widen_row(w, v5.c), P[5] = v5.p, N[5] = v5.n;
    }
}

}  // namespace

__global__ __launch_bounds__(64 * dpx::kWaves) void k_deint(DeintArgs a)
{
    const size_t total = (size_t)a.n_streams * a.frames_out * a.frame_items;
    const int wave = threadIdx.x >> 6;
    for (size_t item = (size_t)blockIdx.x * dpx::kWaves + wave; item < total; item += (size_t)gridDim.x * dpx::kWaves) {
        const size_t frame = item / (size_t)a.frame_items;
        const dpx::Item it = dpx::item(a.s.width, a.s.height, (int)(item - frame * (size_t)a.frame_items));
        if (it.shared)
            deint_item<true>(a, frame, it);
        else
            deint_item<false>(a, frame, it);
    }
}

}  // namespace efx
