// k_denoise.hip -- spatial and temporal noise reduction of source pictures (efx_denoise): a thresholded 3 x 3 binomial
// filter, then a recursive blend with the stream's previous output, by the rule of include/efx.h, "noisy sources".  The
// arithmetic is denoise_px.h's: an integer function of the source bytes, the same functions on the host and here.
//
// k_denoise one launch per call.  The serial axis is time: an item is a band of 4 rows of a column tile of 992 samples of
//           one plane of one STREAM, and the wave that owns it walks the stream's frames in order; four items per
//           workgroup, no LDS, no barrier.
//           What lives in registers.  The previous output P of the band, 4 rows x 4 words a lane, from one frame to the
//           next: it is read from memory only for the first frame of a call that has a `prev`, and never read back from
//           dst.  A window of 6 source rows (the band and a row either side), 4 words each: a slot is free as soon as
//           its row has been widened with the halo words, and the same row of frame t + 1 is asked for at that moment,
//           before the arithmetic of frame t's row begins -- the source does not depend on the recursion, so only the
//           blend is on the serial chain, and one window serves both frames.
//           Columns are k_deint's.  A lane owns 16 samples of a row: one 16-byte load (two for a row of NV12 pairs,
//           de-interleaved with v_perm_b32) at whatever alignment the plane gives, one 16-byte store per output row; the
//           word before and the word after come from the neighbouring lanes (two lane shuffles per row), lanes 0 and 63
//           only fetch; chroma planes of up to 480 samples a row share a wave, Cb in lanes 0 .. 31, Cr in 32 .. 63; the
//           picture-edge clamp is done on the fetched words, once per row.  Rows are clamped by index: the band's halo
//           rows are its neighbours' own rows, fetched a second time (from L2).
//           Arithmetic.  Two samples per instruction in 16-bit halves (v_pk_*_i16): a neighbour is cut out of a pair of
//           words and zero-extended by one v_perm_b32, and what it adds to the sum is its difference from the centre
//           where that lies within the threshold, else 0 (a sign mask, no compare).  The blend's k needs 24-bit
//           products and runs per sample; Q comes with the arguments, nothing is divided here.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "denoise_px.h"

namespace efx {

namespace {

constexpr int kRows = npx::kBandRows + 2;  // source rows of a frame a wave holds: the band and a row either side

struct Wave {
    const uint8_t* src;  // the stream's frame 0
    size_t src_stride;
    size_t end;          // bytes of an image that may be read: the surface's, rounded up to 16
    dpx::PlaneAt at;     // where the plane's rows lie in an image
    bool pairs;          // ... as every other byte of pair rows (the same for the lanes of a wave)
    int ph, y0, nr;      // the plane's rows; the band's first row and its rows (1 .. 4)
    int X, n;            // the lane's first column, and the columns from there on
    bool active;
};

// Slot i of the window: row y0 - 1 + i (clamped) of the image at img.  A row of byte samples is one load and nothing
// else (npx::load_plain: no branch stands between the load and the slot's registers, so the wave does not wait for it
// here); a row of pairs is fetched and de-interleaved at once.
__device__ inline dpx::Chunk fetch_slot(const Wave& w, const uint8_t* img, int i)
{
    const int r = npx::clamp_row(w.y0 - 1 + i, w.ph);
    if (!w.pairs)
        return npx::load_plain(w.at, img, w.end, r, w.active ? w.X : 0);
    dpx::Chunk c = {};
    if (w.active)
        c = dpx::fetch_row(w.at, img, w.end, r, w.X, w.n);
    return c;
}

// A slot with its halo words (every lane of the wave comes here: the shuffles); the slot is free from then on and the same
// row of the next frame, if there is one, is asked for at once
__device__ inline dpx::Ext take_slot(const Wave& w, dpx::Chunk* slot, const uint8_t* next, int i)
{
    dpx::Chunk c = *slot;
    if (!w.pairs)
        c = npx::settle_plain(c, w.at, w.end, npx::clamp_row(w.y0 - 1 + i, w.ph), w.active ? w.X : 0);
    const dpx::Ext x = npx::widen_row(c, __shfl_up(c.d[3], 1), __shfl_down(c.d[0], 1), w.active, w.X, w.n);
    if (next)
        *slot = fetch_slot(w, next, i);
    return x;
}

// SHARED: Cb and Cr in the two halves of the wave (the plane, and with it where rows lie, then differs from lane to lane)
template <bool SHARED>
__device__ __forceinline__ void denoise_item(const DenoiseArgs& a, size_t stream, dpx::Item it)
{
    const int lane = threadIdx.x & 63;
    const efx_surface& s = a.s;
    it.shared = SHARED;
    const dpx::Place at = dpx::place(it, lane);
    const int pw = dpx::plane_w(s.width, it.plane);
    Wave w;
    w.at = dpx::plane_at(s, at.plane);
    w.pairs = it.plane != 0 && s.layout == EFX_SURF_SEMI8;
    w.ph = dpx::plane_h(s.height, it.plane);
    w.y0 = it.band * npx::kBandRows;
    w.nr = w.ph - w.y0 < npx::kBandRows ? w.ph - w.y0 : npx::kBandRows;
    w.X = at.X;
    w.n = pw - w.X;
    w.active = w.X >= 0 && w.n > 0;
    const bool writes = w.active && !at.halo;
    w.src = a.src + stream * (size_t)a.n_frames * a.src_stride;
    w.src_stride = a.src_stride;
    w.end = (s.bytes + 15) / 16 * 16;
    npx::Plane thr;  // (Q was divided on the host)
    thr.ts2 = (uint32_t)(it.plane ? a.ts[1] : a.ts[0]) * 0x00010001u;
    thr.tt = it.plane ? a.tt[1] : a.tt[0], thr.q = it.plane ? a.q[1] : a.q[0];
    // the lane's chunk in row y0 of its plane, in a packed I420 picture
    const size_t image = (size_t)s.width * s.height * 3 / 2;
    const size_t plane_first = dpx::out_plane(s.width, s.height, at.plane);
    uint8_t* out = a.dst + stream * (size_t)a.n_frames * a.dst_stride + plane_first + (size_t)w.y0 * pw + w.X;

    dpx::Chunk P[npx::kBandRows] = {};
    bool has_prev = a.prev != nullptr;
    if (has_prev && writes) {
        const uint8_t* pic = a.prev + stream * a.prev_stride;
#pragma unroll
        for (int r = 0; r < npx::kBandRows; r++)
            if (r < w.nr)
                P[r] = npx::fetch_prev(pic, (image + 15) / 16 * 16, plane_first, pw, w.y0 + r, w.X);
    }
    dpx::Chunk row[kRows] = {};
#pragma unroll
    for (int i = 0; i < kRows; i++)
        if (i < w.nr + 2)
            row[i] = fetch_slot(w, w.src, i);
    for (int t = 0; t < a.n_frames; t++) {
        // (what a lane derives from its column is made again for every frame: with this barrier the compiler keeps less
        // across the loop, the kernel fits 256 registers -- two waves per SIMD -- and the scheduler, no longer pressed for
        // registers, interleaves the neighbours' chains instead of filling their gaps with s_nop)
        asm volatile("" : "+v"(w.X), "+v"(w.n));
        const uint8_t* next = t + 1 < a.n_frames ? w.src + (size_t)(t + 1) * a.src_stride : nullptr;
        dpx::Ext up = take_slot(w, &row[0], next, 0), mid = take_slot(w, &row[1], next, 1);
#pragma unroll
        for (int r = 0; r < npx::kBandRows; r++) {
            if (r < w.nr) {
                const dpx::Ext dn = take_slot(w, &row[r + 2], next, r + 2);
                if (writes) {
                    P[r] = npx::row_out(up, mid, dn, P[r], has_prev, thr);
                    dpx::store_chunk(out + (size_t)r * pw, P[r], w.n);
                }
                up = mid, mid = dn;
            }
        }
        has_prev = true;
        out += a.dst_stride;
    }
}

}  // namespace

__global__ __launch_bounds__(64 * npx::kWaves) void k_denoise(DenoiseArgs a)
{
    const size_t total = (size_t)a.n_streams * a.stream_items;
    const int wave = threadIdx.x >> 6;
    for (size_t item = (size_t)blockIdx.x * npx::kWaves + wave; item < total; item += (size_t)gridDim.x * npx::kWaves) {
        const size_t stream = item / (size_t)a.stream_items;
        const dpx::Item it = npx::item(a.s.width, a.s.height, (int)(item - stream * (size_t)a.stream_items));
        if (it.shared)
            denoise_item<true>(a, stream, it);
        else
            denoise_item<false>(a, stream, it);
    }
}

}  // namespace efx
