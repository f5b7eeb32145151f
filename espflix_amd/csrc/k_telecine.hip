// k_telecine.hip -- telecined sources back to film frames (efx_detelecine): for every frame the comb scores of the frame as
// it is and of its earlier field woven with the previous frame's later field, the difference of the earlier fields, the
// match and the frame to drop in every cycle of five, and the woven outputs, by the rule of include/efx.h, "telecined
// sources".  The arithmetic is telecine_px.h's: an integer function of the source bytes, the same functions on the host
// and here.  Three launches per call, in stream order; the records in info_device are the only state between them.
//
// k_telecine_measure  the hot path.  A workgroup of four waves takes a processed frame.  A lane walks a strip -- the 16
//           columns of a chunk down a band of 32 rows -- with one 16-byte load per row at whatever alignment the plane
//           gives (NV12's luma plane is read like a planar one); the comb is vertical, so no lane needs a neighbour's
//           samples: no halo, no shuffle, no LDS in the walk, and the lanes of a wave need not share a band.  An item is
//           64 strips counted along a band and then band by band, one per lane, so that a row of 45 chunks (720 samples)
//           fills its waves as well as one of 64; the frame's items go round the four waves.  A register window of six rows of F[t] and the three later-field rows of F[t - 1] among them slides
//           down the band two rows at a time, rows widened once to 16-bit halves (v_perm_b32); v runs two samples per
//           instruction (v_pk_*_i16, the threshold one v_pk_sub_u16 with clamp), D is v_sad_u8 on the loaded words.  The
//           two candidates of a row share the partial sum of the rows both take from F[t].  F[t] is read once as a
//           frame and once as the next frame's predecessor (of which the earlier field's rows only inside the band);
//           chroma is never read.
//           Sums.  Per-item partials kept on chip, not atomics: a lane sums in 32 bits over a band, in 64 bits over its
//           items; the wave adds its lanes with shuffles, the four waves meet in 96 bytes of LDS, and one thread stores
//           the record.  Nothing has to be zeroed first (the records' earlier content does not matter and a fourth
//           launch is not needed), and the sum does not depend on any order.
// k_telecine_decide   one thread per stream and cycle: tpx::decide_cycle on the cycle's records.
// k_telecine_weave    an item is a band of 32 rows of a plane of a processed frame, one per wave.  The frame's record says
//           whether it has an output, which one, and which frame supplies the later field; a dropped frame's items end
//           at once.  The band's chunks are counted row by row and dealt to the lanes (a narrow plane wastes no lanes),
//           four in flight per lane.  Every output row is one source row: a 16-byte load and a 16-byte store; of a
//           semi-planar surface one item makes Cb's and Cr's band from one fetch of the pair rows (32 bytes,
//           de-interleaved with v_perm_b32).
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "telecine_px.h"

namespace efx {

namespace {

__device__ inline uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1)
        v += __shfl_down((unsigned long long)v, k);
    return v;  // (lane 0's is the wave's)
}

}  // namespace

__global__ __launch_bounds__(64 * tpx::kMeasureWaves) void k_telecine_measure(TelecineArgs a)
{
    __shared__ uint64_t part[tpx::kMeasureWaves][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t total = (size_t)a.n_streams * a.n;
    tpx::Measure m;
    m.end = (a.s.bytes + 15) / 16 * 16;
    m.at = dpx::plane_at(a.s, 0);
    m.w = a.s.width, m.h = a.s.height;
    m.thr2 = tpx::threshold2(a.nt);
    for (size_t frame = blockIdx.x; frame < total; frame += gridDim.x) {
        const size_t stream = frame / (size_t)a.n;
        const int t = a.lead + (int)(frame - stream * (size_t)a.n);
        m.cur = a.src + (stream * (size_t)a.n_frames + (size_t)t) * a.src_stride;
        m.has_prev = t > 0;
        m.prev = m.has_prev ? m.cur - a.src_stride : m.cur;
        tpx::Sums s = {0, 0, 0};
        for (int k = wave; k < a.measure_items; k += tpx::kMeasureWaves) {
            if (a.first_field == EFX_FIELD_TOP)
                tpx::measure_lane<0>(m, k, lane, &s);
            else
                tpx::measure_lane<1>(m, k, lane, &s);
        }
        s.cc = wave_sum(s.cc), s.cp = wave_sum(s.cp), s.d = wave_sum(s.d);
        if (lane == 0)
            part[wave][0] = s.cc, part[wave][1] = s.cp, part[wave][2] = s.d;
        __syncthreads();
        if (threadIdx.x == 0) {
            tpx::Sums all = {0, 0, 0};
            for (int i = 0; i < tpx::kMeasureWaves; i++)
                all.cc += part[i][0], all.cp += part[i][1], all.d += part[i][2];
            a.info[frame] = tpx::measured(all, m.has_prev);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_telecine_decide(TelecineArgs a)
{
    const int cycles = (a.n + tpx::kCycle - 1) / tpx::kCycle;
    const size_t total = (size_t)a.n_streams * cycles;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t stream = i / (size_t)cycles;
        const int c = (int)(i - stream * (size_t)cycles);
        const int left = a.n - c * tpx::kCycle;
        tpx::decide_cycle(a.info + stream * (size_t)a.n + (size_t)c * tpx::kCycle, left < tpx::kCycle ? left : tpx::kCycle, c * (tpx::kCycle - 1));
    }
}

__global__ __launch_bounds__(64 * tpx::kWeaveWaves) void k_telecine_weave(TelecineArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t total = (size_t)a.n_streams * a.n * a.weave_items;
    const size_t end = (a.s.bytes + 15) / 16 * 16;
    for (size_t item = (size_t)blockIdx.x * tpx::kWeaveWaves + wave; item < total; item += (size_t)gridDim.x * tpx::kWeaveWaves) {
        const size_t frame = item / (size_t)a.weave_items;
        const int k = (int)(item - frame * (size_t)a.weave_items);
        const efx_telecine_info r = a.info[frame];
        if (r.out < 0 || r.out >= a.n_out)  // dropped (the second test never holds: k_telecine_decide wrote the record)
            continue;
        const size_t stream = frame / (size_t)a.n;
        const int t = a.lead + (int)(frame - stream * (size_t)a.n);
        const uint8_t* cur = a.src + (stream * (size_t)a.n_frames + (size_t)t) * a.src_stride;
        const uint8_t* other = r.match && t > 0 ? cur - a.src_stride : cur;
        uint8_t* out = a.dst + (stream * (size_t)a.n_out + (size_t)r.out) * a.dst_stride;
        tpx::weave_lane(a.s, cur, other, end, out, a.first_field == EFX_FIELD_TOP ? 0 : 1, k, lane);
    }
}

}  // namespace efx
