// k_scan.hip -- progressive, interlaced or telecined (efx_detect_scan): for every frame the comb scores of the frame as it
// is and of its two weaves with the previous frame, the differences of the top and of the bottom fields, its label and
// its repeat, and for every stream the counts of these, by the rule of include/efx.h, "scan type".  The arithmetic is
// scan_px.h's: an integer function of the source bytes, the same functions on the host and here.  Two launches per call,
// in stream order; the frame records in frames_device are the only state between them.
//
// k_scan_measure  the hot path, laid out as k_telecine_measure.  A workgroup of four waves takes a processed frame.  A lane
//           walks a strip -- the 16 columns of a chunk down a band of 32 rows -- with one 16-byte load per row of F[t] and
//           of F[t - 1] at whatever alignment the plane gives; the comb is vertical, so no lane needs a neighbour's
//           samples: no halo, no shuffle, no LDS in the walk.  An item is 64 strips counted along a band and then band by
//           band, one per lane; the frame's items go round the four waves.  Register windows of six rows of both frames
//           go down the band two rows at a time, rows widened once to 16-bit halves (v_perm_b32); the windows are rings,
//           three steps to a turn (scpx::step<K>), so that a step moves no row.  All three combs come
//           from one pass: per row the partial sums S and A of both frames and three absolute differences, two samples
//           per instruction (v_pk_*_i16, the threshold one v_pk_sub_u16 with clamp); the field differences are v_sad_u8
//           on the loaded words.  Chroma is never read.  A frame with no predecessor is not walked.
//           Sums.  Per-item partials kept on chip, not atomics: a lane sums in 32 bits over a band, in 64 bits over its
//           items; the wave adds its lanes with shuffles, the four waves meet in 160 bytes of LDS, and one thread stores
//           the frame's record with its label and repeat.  Nothing has to be zeroed first.
// k_scan_count    one wave per stream.  Lanes take the stream's frame records 64 at a time; each of a record's 15 counters
//           grows by the population count of a ballot.  Lane 0 writes the 64-byte record, or adds to it.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "scan_px.h"

namespace efx {

namespace {

__device__ inline uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1)
        v += __shfl_down((unsigned long long)v, k);
    return v;  // (lane 0's is the wave's)
}

__device__ inline scpx::Rule rule_of(const ScanArgs& a)
{
    scpx::Rule r;
    r.still_wh = a.still_wh, r.prog = a.prog, r.intl = a.intl, r.rep = a.rep;
    return r;
}

}  // namespace

__global__ __launch_bounds__(64 * scpx::kMeasureWaves) void k_scan_measure(ScanArgs a)
{
    __shared__ uint64_t part[scpx::kMeasureWaves][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t total = (size_t)a.n_streams * a.n;
    scpx::Measure m;
    m.end = (a.s.bytes + 15) / 16 * 16;
    m.at = dpx::plane_at(a.s, 0);
    m.w = a.s.width, m.h = a.s.height;
    m.thr2 = tpx::threshold2(a.nt);
    m.has_prev = true;
    for (size_t frame = blockIdx.x; frame < total; frame += gridDim.x) {
        const size_t stream = frame / (size_t)a.n;
        const int t = a.lead + (int)(frame - stream * (size_t)a.n);
        const bool has_prev = t > 0;
        m.cur = a.src + (stream * (size_t)a.n_frames + (size_t)t) * a.src_stride;
        m.prev = has_prev ? m.cur - a.src_stride : m.cur;
        scpx::Sums s = {0, 0, 0, 0, 0};
        if (has_prev)
            for (int k = wave; k < a.measure_items; k += scpx::kMeasureWaves)
                scpx::measure_lane(m, k, lane, &s);
        s.cc = wave_sum(s.cc), s.ctb = wave_sum(s.ctb), s.cbt = wave_sum(s.cbt), s.dt = wave_sum(s.dt), s.db = wave_sum(s.db);
        if (lane == 0)
            part[wave][0] = s.cc, part[wave][1] = s.ctb, part[wave][2] = s.cbt, part[wave][3] = s.dt, part[wave][4] = s.db;
        __syncthreads();
        if (threadIdx.x == 0) {
            scpx::Sums all = {0, 0, 0, 0, 0};
            for (int i = 0; i < scpx::kMeasureWaves; i++)
                all.cc += part[i][0], all.ctb += part[i][1], all.cbt += part[i][2], all.dt += part[i][3], all.db += part[i][4];
            a.frames[frame] = scpx::measured(all, has_prev, rule_of(a));
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64 * scpx::kCountWaves) void k_scan_count(ScanArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t stream = (size_t)blockIdx.x * scpx::kCountWaves + wave; stream < (size_t)a.n_streams; stream += (size_t)gridDim.x * scpx::kCountWaves) {
        const efx_scan_frame* f = a.frames + stream * (size_t)a.n;
        uint32_t count[scpx::kSlots] = {};
        for (int j0 = 0; j0 < a.n; j0 += 64) {
            const int j = j0 + lane;
            int ls = -1, rs = -1;
            if (j < a.n) {
                const efx_scan_frame r = f[j];
                ls = scpx::label_slot(r), rs = scpx::repeat_slot(r, scpx::phase_of(a.first_frame, a.lead + j));
            }
#pragma unroll
            for (int k = 0; k < scpx::kSlots; k++)
                count[k] += (uint32_t)__popcll(__ballot(ls == k || rs == k));
        }
        if (lane == 0) {
            uint32_t* rec = reinterpret_cast<uint32_t*>(a.recs + stream);
#pragma unroll
            for (int k = 0; k < scpx::kSlots; k++)
                rec[k] = (a.accumulate ? rec[k] : 0u) + count[k];
            rec[scpx::kSlots] = 0;
        }
    }
}

}  // namespace efx
