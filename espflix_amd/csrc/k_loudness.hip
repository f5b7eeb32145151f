// k_loudness.hip -- programme loudness by ITU-R BS.1770-4 / EBU R 128 of mono int16 PCM at the four SBC rates, for a batch
// of streams, and the gain that levels a stream.  The arithmetic is loudness_px.h's: an integer function of the samples
// (the formulas: include/efx.h), the same functions on the host and here.  No floating point, no division, no scratch.
//
// k_loud_steps  one lane per (stream, 100 ms step), a wave per 64 consecutive steps of one stream.  A lane starts the
//               K-weighting filter at rest W = step / 2 samples in front of its step and runs it over W + step samples, so
//               steps do not depend on each other (include/efx.h).  Adjacent lanes' rows lie 2 x step bytes apart
//               (3200 .. 9600), so the samples come through LDS: per trip the wave fetches 128 bytes of each of its 64
//               rows with 16-byte loads, eight lanes to a row, and every lane reads its own row back, 16 bytes at a
//               time, rows 144 bytes apart.  Rows begin at any sample: a row is fetched from its 16-byte piece aligned
//               down, and the d = 0 .. 7 samples in front of it are fed to the filter as zeros, which a filter at rest
//               does not notice.  Samples in front of the call's first come from the stream's state.
// k_loud_state  one workgroup per stream: the newest W + step samples (rounded up to whole pieces) become the stream's
//               state.  A launch of its own: k_loud_steps' waves read the old state.
// k_loud_gate   one workgroup per stream: blocks of four steps, the absolute gate, the relative gate, the largest block,
//               the peak; integer sums, so their order does not show; then one lane works out the gain.
// k_pcm_gain    16 bytes per lane: y = clamp16((x g + 2048) >> 12), g from the stream's record on the device.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "loudness_px.h"

namespace efx {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ inline int lo16(uint32_t w) { return (int16_t)(w & 0xFFFF); }
__device__ inline int hi16(uint32_t w) { return (int16_t)(w >> 16); }

// the 16-byte piece of samples v8 .. v8 + 7 (v8 a multiple of 8, -hist <= v8 < n_samples), counted from the call's first
__device__ inline u32x4 piece(const loud::Plan& p, const int16_t* __restrict__ src, const int16_t* __restrict__ hist, int v8)
{
    if (v8 < 0)
        return *reinterpret_cast<const u32x4*>(hist + p.hist + v8);
    if (v8 + 8 <= p.n_samples)
        return *reinterpret_cast<const u32x4*>(src + v8);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (v8 + i < p.n_samples)
            w[i >> 1] |= (uint32_t)(uint16_t)src[v8 + i] << (16 * (i & 1));
    return u32x4{w[0], w[1], w[2], w[3]};
}

}  // namespace

__global__ __launch_bounds__(64) void k_loud_steps(LoudStepsArgs a)
{
    __shared__ u32x4 s_rows[loud::kLanes * loud::kRowPitch16];

    const loud::Plan& p = a.plan;
    const int lane = threadIdx.x;
    // (the stream in grid.x, which has no 65535 limit)
    const int16_t* src = a.pcm + (size_t)blockIdx.x * a.pcm_stride;
    const int16_t* hist = a.state + (size_t)blockIdx.x * p.hist;
    const int t0 = blockIdx.y * loud::kLanes;
    const int len = p.runin + p.step;

    const int t = t0 + lane;
    const bool live = t < p.n_new;
    // the lane's first sample (>= -hist), counted from the call's first; lanes past the call's steps take the last step's,
    // so that no product leaves int where n_samples is next to 2^31
    const int start = p.row0 + min(t, p.n_new - 1) * p.step;
    const int d = start & 7;                // samples between the piece aligned down and the row
    loud::Lane L{};

    const int sub = lane >> 3, col = lane & 7;
    const int n_trips = (len + 7 + loud::kChunk - 1) / loud::kChunk;
    for (int c = 0; c < n_trips; c++) {
        __syncthreads();  // the previous trip's readers are done
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int r = 8 * k + sub;
            const int rs = p.row0 + min(t0 + r, p.n_new - 1) * p.step;  // (rows past the call's steps: not fetched)
            const int v8 = (rs & ~7) + loud::kChunk * c + 8 * col;
            u32x4 v = {0, 0, 0, 0};
            if (t0 + r < p.n_new && v8 < rs + len)  // (rs + len <= n_samples: the step is whole)
                v = piece(p, src, hist, v8);
            s_rows[r * loud::kRowPitch16 + col] = v;
        }
        __syncthreads();
        if (live) {
#pragma unroll 2
            for (int q = 0; q < 8; q++) {
                const u32x4 v = s_rows[lane * loud::kRowPitch16 + q];
                const int i0 = loud::kChunk * c + 8 * q - d;  // the row's index of the piece's first sample
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int i = i0 + 2 * j;
                    loud::feed(p.k, L, lo16(v[j]), i >= 0 && i < len, i >= p.runin && i < len);
                    loud::feed(p.k, L, hi16(v[j]), i + 1 >= 0 && i + 1 < len, i + 1 >= p.runin && i + 1 < len);
                }
            }
        }
    }
    if (live) {
        u32x4* out = reinterpret_cast<u32x4*>(a.steps + (size_t)blockIdx.x * a.steps_stride + a.first_step + t);
        *out = u32x4{(uint32_t)L.energy, (uint32_t)(L.energy >> 32), L.peak, 0};
    }
}

__global__ __launch_bounds__(256) void k_loud_state(LoudStepsArgs a)
{
    const loud::Plan& p = a.plan;
    const int16_t* src = a.pcm + (size_t)blockIdx.x * a.pcm_stride;
    int16_t* hist = a.state + (size_t)blockIdx.x * p.hist;
    constexpr int kPer = (loud::kMaxHist / 8 + 255) / 256;  // pieces of a lane: 4
    u32x4 keep[kPer];
#pragma unroll
    for (int m = 0; m < kPer; m++) {
        const int k8 = 8 * ((int)threadIdx.x + 256 * m);
        uint32_t w[4] = {0, 0, 0, 0};
        if (k8 < p.hist) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int j = p.n_samples - p.hist + k8 + i;  // the sample that lands in hist[k8 + i], counted from the call's first
                const int16_t x = j < 0 ? hist[k8 + i + p.n_samples] : src[j];
                w[i >> 1] |= (uint32_t)(uint16_t)x << (16 * (i & 1));
            }
        }
        keep[m] = u32x4{w[0], w[1], w[2], w[3]};
    }
    __syncthreads();  // every old sample is read
#pragma unroll
    for (int m = 0; m < kPer; m++) {
        const int k8 = 8 * ((int)threadIdx.x + 256 * m);
        if (k8 < p.hist)
            *reinterpret_cast<u32x4*>(hist + k8) = keep[m];
    }
}

__global__ __launch_bounds__(256) void k_loud_gate(LoudGateArgs a)
{
    // [0] lo, [1] hi of the absolute gate's sum, [2] lo, [3] hi of the relative gate's, [4] the largest block
    __shared__ unsigned long long s_sum[5];
    __shared__ unsigned int s_cnt[3];  // blocks above the absolute gate, blocks above both, the peak

    const int tid = threadIdx.x;
    const u32x4* steps = reinterpret_cast<const u32x4*>(a.steps + (size_t)blockIdx.x * a.steps_stride);
    const int n_blocks = a.n_steps >= 4 ? a.n_steps - 3 : 0;
    if (tid < 5)
        s_sum[tid] = 0;
    if (tid < 3)
        s_cnt[tid] = 0;
    __syncthreads();

    auto block = [&](int j) {
        uint64_t b = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const u32x4 r = steps[j + i];
            b += (uint64_t)r[0] | ((uint64_t)r[1] << 32);
        }
        return b;
    };

    // the peak: every step's, and the samples of the state when there is one
    uint32_t peak = 0;
    for (int j = tid; j < a.n_steps; j += 256)
        peak = max(peak, steps[j][2]);
    if (a.state) {
        const u32x4* h = reinterpret_cast<const u32x4*>(a.state + (size_t)blockIdx.x * a.hist);
        for (int k = tid; k < a.hist / 8; k += 256) {
            const u32x4 v = h[k];
#pragma unroll
            for (int i = 0; i < 4; i++)
                peak = max(peak, max(loud::abs16(lo16(v[i])), loud::abs16(hi16(v[i]))));
        }
    }
    atomicMax(&s_cnt[2], peak);

    // the absolute gate and the largest block
    loud::Acc acc{};
    uint64_t largest = 0;
    for (int j = tid; j < n_blocks; j += 256) {
        const uint64_t b = block(j);
        largest = b > largest ? b : largest;
        if (b > a.abs_thr)
            loud::acc_add(acc, b);
    }
    if (acc.n) {
        atomicAdd(&s_sum[0], (unsigned long long)acc.lo);
        atomicAdd(&s_sum[1], (unsigned long long)acc.hi);
        atomicAdd(&s_cnt[0], acc.n);
    }
    atomicMax(&s_sum[4], (unsigned long long)largest);
    __syncthreads();

    // the relative gate
    const uint32_t n_abs = s_cnt[0];
    const loud::u128 S_abs = loud::acc_sum(s_sum[0], s_sum[1]);
    acc = loud::Acc{};
    if (n_abs)
        for (int j = tid; j < n_blocks; j += 256) {
            const uint64_t b = block(j);
            if (b > a.abs_thr && loud::rel_pass(b, n_abs, S_abs))
                loud::acc_add(acc, b);
        }
    if (acc.n) {
        atomicAdd(&s_sum[2], (unsigned long long)acc.lo);
        atomicAdd(&s_sum[3], (unsigned long long)acc.hi);
        atomicAdd(&s_cnt[1], acc.n);
    }
    __syncthreads();

    if (tid == 0) {
        const uint32_t n_gated = s_cnt[1], pk = s_cnt[2];
        const uint64_t mean = n_gated ? loud::udiv128(loud::acc_sum(s_sum[2], s_sum[3]), n_gated) : 0;
        const uint32_t g = (uint32_t)loud::gain_q12(mean, n_gated, pk, a.target_ms, a.ceiling, a.step);
        const uint64_t largest_block = s_sum[4];
        u32x4* out = reinterpret_cast<u32x4*>(a.recs + blockIdx.x);
        out[0] = u32x4{(uint32_t)mean, (uint32_t)(mean >> 32), (uint32_t)largest_block, (uint32_t)(largest_block >> 32)};
        out[1] = u32x4{n_gated, (uint32_t)n_blocks, n_abs, pk | (g << 16)};
    }
}

__global__ __launch_bounds__(256) void k_pcm_gain(PcmGainArgs a)
{
    const int16_t* src = a.src + (size_t)blockIdx.x * a.src_stride;
    int16_t* dst = a.dst + (size_t)blockIdx.x * a.dst_stride;
    const int g = a.recs ? (int)a.recs[blockIdx.x].gain_q12 : a.fixed_gain;
    const int n_pieces = (a.n_samples + 7) / 8;
    for (int k = blockIdx.y * 256 + threadIdx.x; k < n_pieces; k += gridDim.y * 256) {
        const int base = 8 * k;
        if (base + 8 <= a.n_samples) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(src + base);
            u32x4 y;
#pragma unroll
            for (int i = 0; i < 4; i++)
                y[i] = (uint32_t)(uint16_t)loud::apply_gain(lo16(v[i]), g) | ((uint32_t)(uint16_t)loud::apply_gain(hi16(v[i]), g) << 16);
            *reinterpret_cast<u32x4*>(dst + base) = y;
        } else {
            for (int i = base; i < a.n_samples; i++)
                dst[i] = (int16_t)loud::apply_gain(src[i], g);
        }
    }
}

}  // namespace efx
