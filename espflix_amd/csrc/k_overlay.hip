// k_overlay.hip -- subtitles and logos burnt into 352 x 192 I420 pictures in place (efx_overlay): a list of events, alpha
// masks with a colour or RGBA bitmaps shown over a span of pictures, by the rule of include/efx.h, "subtitles and logos".
// The arithmetic is overlay_px.h's: an integer function of the bytes, the same functions on the host and here.
//
// k_overlay one launch per call, a workgroup of four waves per (stream, picture).
//           Scan.  The workgroup walks the event list once, 256 events a step, a lane an event: the validity rule, the
//           stream, the span, the gain at this picture and whether the bitmap reaches the picture at all.  What is left
//           is compacted in list order into LDS -- a ballot per wave, the waves' counts through LDS, one barrier a step
//           (the counts alternate between two slots) -- as index | gain << 16.  An empty list ends the workgroup: a
//           picture nothing is shown on is never touched.  Picture 0's workgroup of a stream reports an invalid event.
//           Draw.  A picture is 1056 units of 32 x 2 luma samples and the 16 sites of Cb and Cr below them, row by row:
//           four 16-byte luma chunks and two of chroma, all aligned, so every byte has one owner for the whole call and
//           a chroma site's four alphas are its owner's.  A tile is 64 consecutive units, a lane each; the four waves
//           take the 17 tiles in turn.  A wave walks the active list in order with the unit in registers: an event
//           whose rectangle lies before or behind the tile is skipped by the whole wave, a chunk is fetched when the
//           first event touches it and stored once at the end, so in-place blending needs no order between waves and
//           a picture's bytes move once however many events overlap.
//           Bitmap.  16 alpha bytes (A8), or four RGBA pixels, per 16-byte access at whatever alignment the atlas
//           gives, moved inside the row where it would begin in front of it and inside the atlas where it would cross
//           its end (ovx::window16).  Luma runs two samples per instruction in 16-bit halves (v_pk_mul_lo_u16,
//           v_pk_add_u16), the chroma sites per sample with v_mul_hi_u32 for the division by 1020.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "overlay_px.h"

namespace efx {

__global__ __launch_bounds__(ovx::kScanStep) void k_overlay(OverlayArgs a)
{
    __shared__ uint32_t sh_active[EFX_OVERLAY_MAX_EVENTS];  // index | gain << 16, in list order
    __shared__ uint32_t sh_count[2][ovx::kWaves];           // a step's active events per wave | an invalid one << 16
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t items = (size_t)a.n_streams * (size_t)a.n_pictures;
    const uint8_t* end = a.atlas + (a.atlas_bytes + 15) / 16 * 16;
    int step = 0;  // (it alternates from picture to picture as well: a wave may begin the next scan while others end this one)
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int stream = (int)(item / (size_t)a.n_pictures), j = (int)(item - (size_t)stream * a.n_pictures);
        const int64_t p = a.first_picture + j;
        int total = 0;
        bool bad = false;
        for (int base = 0; base < a.n_events; base += ovx::kScanStep, step ^= 1) {
            const int i = base + (int)threadIdx.x;
            bool act = false, inv = false;
            int g = 0;
            if (i < a.n_events) {
                const efx_overlay_event e = a.events[i];
                inv = !ovx::valid(e, a.atlas_bytes);
                if (!inv && (e.stream == -1 || e.stream == stream) && e.first <= p && p <= e.last && ovx::reaches(e)) {
                    g = ovx::gain(e, p);
                    act = g > 0;
                }
            }
            const uint64_t m = __ballot(act);
            const bool any_inv = __ballot(inv) != 0;
            if (lane == 0)
                sh_count[step][wave] = (uint32_t)__popcll(m) | (any_inv ? 1u << 16 : 0u);
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < ovx::kWaves; w++) {
                const uint32_t c = sh_count[step][w];
                all += (int)(c & 0xFFFFu), before += w < wave ? (int)(c & 0xFFFFu) : 0;
                bad |= (c >> 16) != 0;
            }
            if (act)
                sh_active[total + before + __popcll(m & (((uint64_t)1 << lane) - 1))] = (uint32_t)i | ((uint32_t)g << 16);
            total += all;
        }
        if (bad && a.status && j == 0 && threadIdx.x == 0)
            atomicOr(a.status + stream, EFX_OVERLAY_BAD_EVENT);
        if (total == 0)
            continue;  // (the same for every lane of the workgroup)
        __syncthreads();
        uint8_t* pic = a.pictures + (size_t)stream * a.stride + (size_t)j * ovx::kPicture;
        for (int tile = wave; tile < ovx::kTiles; tile += ovx::kWaves) {
            const int unit = tile * 64 + lane;
            const bool mine = unit < ovx::kUnits;
            const int X = (unit % ovx::kUnitsX) * ovx::kUnitCols, Y = (unit / ovx::kUnitsX) * ovx::kUnitRows;
            ovx::Unit u = {};
            for (int k = 0; k < total; k++) {
                const uint32_t rec = __builtin_amdgcn_readfirstlane(sh_active[k]);
                const efx_overlay_event e = a.events[rec & 0xFFFFu];
                const ovx::Draw d = ovx::draw_of(e, a.atlas, (int)(rec >> 16));
                if (ovx::last_unit(d) < tile * 64 || ovx::first_unit(d) >= tile * 64 + 64)
                    continue;
                if (mine)
                    ovx::apply(&u, d, pic, X, Y, end);
            }
            if (mine)
                ovx::store(u, pic, X, Y);
        }
        __syncthreads();  // the list is the next picture's from here on
    }
}

}  // namespace efx
