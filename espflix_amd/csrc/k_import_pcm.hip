// k_import_pcm.hip -- sound in: int16 PCM of any rate (8 .. 192 kHz) and 1 .. 8 channels downmixed to mono and resampled to
// one of the four SBC rates, the layout efx_sbc_encode reads.  The arithmetic is import_pcm.h's: an integer function of
// the source bytes (the formulas: include/efx.h), the same functions on the host and here.  No floating point, no
// division, no scratch.
//
// k_import_pcm        one workgroup per (stream, set of tiles of 1024 outputs): grid.y workgroups share a stream's tiles
//                     round robin, so the prototype table (32 KB, copied into LDS once per workgroup) serves many tiles.
//                     Per tile the input span -- the frames under the tile's taps, at most 4 x 1023 + 129 -- is staged in
//                     LDS as mixed samples: the source is fetched as 16-byte pieces aligned down inside the stream's
//                     n_in x channels elements (a piece that would end behind them is fetched element by element), every
//                     element adds w[c] x into its frame's 32-bit sum with an LDS atomic (integer sums do not depend on
//                     their order), frames in front of the call come from the stream's history.  Then one output per
//                     lane and step: two runs of W taps, coefficient = table entry + interpolated difference, 64-bit
//                     accumulate.
// k_import_pcm_state  one workgroup per stream: the newest 127 mixed samples -- from the old history where the call was
//                     shorter than that, else from the source -- become the stream's history.  A launch of its own: the
//                     main kernel's workgroups read the old history.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "import_pcm.h"

namespace efx {

namespace {

constexpr int kThreads = 256;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// elements [ea, eb) of the stream (0 <= ea <= eb <= total = n_in x channels) as 16-byte pieces; `plane` < 0: interleaved,
// else the elements are frames ea - plane_base .. of channel `plane`.  Frame f adds into acc[f - s_lo].
__device__ inline void gather(const ipcm::Plan& p, const int16_t* __restrict__ src, int ea, int eb, int total, int plane, int plane_base,
                              const int* s_w, int* acc, int s_lo)
{
    if (ea >= eb)
        return;
    const int k0 = ea >> 3, k1 = (eb - 1) >> 3;
    for (int k = k0 + (int)threadIdx.x; k <= k1; k += kThreads) {
        const int base = 8 * k;
        int16_t x[8];
        if (base + 8 <= total) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(src + base);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                x[2 * i] = (int16_t)(v[i] & 0xFFFF);
                x[2 * i + 1] = (int16_t)(v[i] >> 16);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++)
                x[i] = base + i < total ? src[base + i] : (int16_t)0;
        }
        int f, c;
        if (plane < 0) {
            f = ipcm::frame_of(p, base);
            c = base - f * p.channels;
        } else {
            f = base - plane_base;
            c = plane;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int e = base + i;
            if (e >= ea && e < eb)
                atomicAdd(&acc[f - s_lo], s_w[c] * (int)x[i]);
            if (plane < 0) {
                if (++c == p.channels)
                    c = 0, f++;
            } else {
                f++;
            }
        }
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_import_pcm(ImportPcmArgs a)
{
    __shared__ int32_t s_T[ipcm::kTableLen + 3];
    __shared__ int32_t s_acc[ipcm::kSpanMax];
    __shared__ int16_t s_mix[ipcm::kSpanMax + 1];
    __shared__ int s_w[ipcm::kMaxChannels];

    const ipcm::Plan& p = a.plan;
    const int tid = threadIdx.x;
    // (the stream in grid.x, which has no 65535 limit)
    const int16_t* src = a.src + (size_t)blockIdx.x * a.src_stride;
    const int16_t* hist = a.state ? a.state + (size_t)blockIdx.x * (ipcm::kStateBytes / 2) : nullptr;
    int16_t* dst = a.dst + (size_t)blockIdx.x * a.dst_stride;

    if (!p.equal)
        for (int i = tid; i < ipcm::kTableLen; i += kThreads)
            s_T[i] = a.table[i];
#pragma unroll
    for (int c = 0; c < ipcm::kMaxChannels; c++)
        if (tid == c)
            s_w[c] = p.w[c];

    const int total = p.n_in * p.channels;
    const int n_tiles = (p.n_out + ipcm::kTile - 1) / ipcm::kTile;
    for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const int t_a = tile * ipcm::kTile, t_b = min(t_a + ipcm::kTile, p.n_out) - 1;  // the tile's first and last output
        // the span: frames s_lo .. s_hi counted from the call's first input frame (negative: history)
        int s_lo, s_hi, ph;
        if (p.equal) {
            s_lo = t_a, s_hi = t_b;
        } else {
            s_lo = ipcm::position(p, t_a, &ph) - 2 * p.W + 1;
            s_hi = ipcm::position(p, t_b, &ph);
        }
        const int len = s_hi - s_lo + 1;  // <= kSpanMax
        __syncthreads();                  // the previous tile's readers are done
        for (int i = tid; i < len; i += kThreads)
            s_acc[i] = 0;
        __syncthreads();
        const int fa = max(s_lo, 0), fb = s_hi + 1;  // frames from the source (s_hi < n_in)
        if (p.layout == ipcm::kLayoutInterleaved || p.channels == 1) {
            gather(p, src, fa * p.channels, fb * p.channels, total, -1, 0, s_w, s_acc, s_lo);
        } else {
            for (int c = 0; c < p.channels; c++)
                gather(p, src, c * p.n_in + fa, c * p.n_in + fb, total, c, c * p.n_in, s_w, s_acc, s_lo);
        }
        __syncthreads();
        for (int i = tid; i < len; i += kThreads) {
            const int j = s_lo + i;
            // hist[k] = m[first_in - 127 + k]; j >= -(2 W - 1) >= -127
            s_mix[i] = j < 0 ? hist[ipcm::kHist + j] : (int16_t)ipcm::mix_round(s_acc[i]);
        }
        __syncthreads();
        for (int t = t_a + tid; t <= t_b; t += kThreads) {
            int y;
            if (p.equal) {
                y = s_mix[t - s_lo];
            } else {
                const int newest = ipcm::position(p, t, &ph);
                y = ipcm::output(p, s_T, s_mix + (newest - s_lo), ph);
            }
            dst[t] = (int16_t)y;
        }
    }
}

__global__ __launch_bounds__(128) void k_import_pcm_state(ImportPcmArgs a)
{
    const ipcm::Plan& p = a.plan;
    const int k = threadIdx.x;
    const int16_t* src = a.src + (size_t)blockIdx.x * a.src_stride;
    int16_t* hist = a.state + (size_t)blockIdx.x * (ipcm::kStateBytes / 2);
    int v = 0;
    if (k < ipcm::kHist) {
        const int j = p.n_in - ipcm::kHist + k;  // the frame that lands in hist[k], counted from the call's first
        if (j < 0) {
            v = hist[k + p.n_in];  // old hist[127 + j]
        } else {
            int32_t sum = 0;
            const bool inter = p.layout == ipcm::kLayoutInterleaved;
#pragma unroll
            for (int c = 0; c < ipcm::kMaxChannels; c++)
                if (c < p.channels)
                    sum += p.w[c] * (int)src[inter ? (size_t)j * p.channels + c : (size_t)c * p.n_in + j];
            v = ipcm::mix_round(sum);
        }
    }
    __syncthreads();  // every old sample is read
    hist[k] = (int16_t)v;
}

}  // namespace efx
