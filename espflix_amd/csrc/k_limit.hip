// k_limit.hip -- the look-ahead peak limiter of mono int16 PCM at the four SBC rates, for a batch of streams.  The rule is
// include/efx.h's ("peak limiter"), the arithmetic limit_px.h's: the same functions on the host and here.  No floating point,
// no scratch, no recurrence along a stream: every tile of blocks is independent work.
//
// k_limit_peaks  a workgroup per tile of 256 blocks of one stream.  Lane t loads the 16-byte pieces t, t + 256, .. of the
//                tile (2, 4 or 6 rounds: Bk / 8), takes their packed 16-bit maximum and minimum, and leaves max(mx, -mn),
//                negated in 32 bits, in LDS; lane t then joins the 2 / 4 / 6 pieces of block t and stores its peak.
// k_pcm_limit    a workgroup per tile of 256 blocks of one stream.  The peaks of the tile and of 2H + 1 blocks either side
//                (514 at most) come into LDS as required gains r; where none is below the stream gain G (most tiles of
//                most titles) the tile is k_pcm_gain's work with gain G.  Else: q over the nodes, the sliding minimum by
//                doubling (log2 W rounds and one that joins two spans into a window of W), the box sum by doubling over
//                the bits of W, both ping-pong between two LDS rows with one barrier per round, one division per node.
//                Then the tile's samples stream through: 16-byte load, eight gains along the line between the block's two
//                nodes (an add, a multiply-high and a shift each), 16-byte store.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "limit_px.h"

namespace efx {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ inline int lo16(uint32_t w) { return (int16_t)(w & 0xFFFF); }
__device__ inline int hi16(uint32_t w) { return (int16_t)(w >> 16); }
__device__ inline s16x2 pair(uint32_t w) { return __builtin_bit_cast(s16x2, w); }

constexpr int kT = limit::kThreads;
constexpr int kRow = (limit::kMaxNodes + 7) & ~7;  // 520

}  // namespace

__global__ __launch_bounds__(256) void k_limit_peaks(LimitPeaksArgs a)
{
    __shared__ uint32_t s_pk[6 * kT];  // the peaks of the tile's pieces

    const int tid = threadIdx.x;
    const int16_t* src = a.pcm + (size_t)blockIdx.x * a.pcm_stride;
    uint16_t* out = a.peaks + (size_t)blockIdx.x * a.peaks_stride + a.entry0;
    const int pb = a.bk >> 3;  // pieces of a block
    const int64_t n = a.n_samples;
    const int64_t n_blocks = (n + a.bk - 1) / a.bk;
    const int64_t n_tiles = (n_blocks + limit::kTile - 1) / limit::kTile;
    for (int64_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const int64_t piece0 = tile * limit::kTile * pb;
        for (int j = 0; j < pb; j++) {
            const int64_t base = 8 * (piece0 + j * kT + tid);
            uint32_t pk = 0;
            if (base + 8 <= n) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(src + base);
                const s16x2 mx = __builtin_elementwise_max(__builtin_elementwise_max(pair(v[0]), pair(v[1])),
                                                           __builtin_elementwise_max(pair(v[2]), pair(v[3])));
                const s16x2 mn = __builtin_elementwise_min(__builtin_elementwise_min(pair(v[0]), pair(v[1])),
                                                           __builtin_elementwise_min(pair(v[2]), pair(v[3])));
                pk = limit::peak_of(max((int)mx[0], (int)mx[1]), min((int)mn[0], (int)mn[1]));
            } else {
                int mx = 0, mn = 0;
                for (int64_t i = base; i < n; i++) {
                    mx = max(mx, (int)src[i]);
                    mn = min(mn, (int)src[i]);
                }
                pk = limit::peak_of(mx, mn);
            }
            s_pk[j * kT + tid] = pk;
        }
        __syncthreads();
        const int64_t b = tile * limit::kTile + tid;
        if (b < n_blocks) {
            uint32_t m = 0;
            for (int i = 0; i < pb; i++)
                m = max(m, s_pk[tid * pb + i]);
            out[b] = (uint16_t)m;
        }
        __syncthreads();  // the next tile's writers wait for these readers
    }
}

__global__ __launch_bounds__(256) void k_pcm_limit(PcmLimitArgs a)
{
    __shared__ uint32_t s_row[2][kRow];
    __shared__ uint32_t s_node[limit::kTile + 8];  // a of the tile's nodes: nb + 1

    const int tid = threadIdx.x;
    const int16_t* src = a.src + (size_t)blockIdx.x * a.src_stride;
    int16_t* dst = a.dst + (size_t)blockIdx.x * a.dst_stride;
    const uint16_t* row = a.peaks + (size_t)blockIdx.x * a.peaks_stride;
    uint32_t G = (uint32_t)a.fixed_gain;
    if (a.recs) {
        const loud::GateRec& rec = a.recs[blockIdx.x];
        G = (uint32_t)loud::stream_gain_q12(rec.gated_mean, rec.n_gated, a.target_ms, a.step);
    }
    const uint32_t C = (uint32_t)a.ceiling;
    const int H = a.half, W = 2 * H + 1;
    const int pb = a.bk >> 3;
    const int64_t n = a.n_samples;
    const int64_t n_blocks = (n + a.bk - 1) / a.bk;
    const int64_t n_tiles = (n_blocks + limit::kTile - 1) / limit::kTile;

    for (int64_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const int nb = (int)min((int64_t)limit::kTile, n_blocks - tile * limit::kTile);  // blocks of this tile
        const int64_t B0 = a.first_block + tile * limit::kTile;                          // its first, as a block of the stream
        const int Np = nb + 4 * H + 2;  // peaks: blocks B0 - 2H - 1 .. B0 + nb + 2H
        bool below = false;
        for (int i = tid; i < Np; i += kT) {
            const int64_t e = B0 - 2 * H - 1 + i - a.peaks_first;
            const uint32_t p = e >= 0 && e < a.n_peaks ? row[e] : 0;
            const uint32_t r = limit::required(p, G, C);
            s_row[0][i] = r;
            below |= r < G;
        }
        const bool limited = __syncthreads_or(below) != 0;  // (also: every r is written)

        if (limited) {
            uint32_t* cur = s_row[1];
            uint32_t* nxt = s_row[0];
            // q of nodes B0 - 2H .. B0 + nb + 2H
            int N = Np - 1;
            for (int i = tid; i < N; i += kT)
                cur[i] = min(nxt[i], nxt[i + 1]);
            __syncthreads();
            // cur[i] = min q[i .. i + span - 1], until span <= W < 2 span
            int span = 1;
            for (; 2 * span <= W; span *= 2) {
                for (int i = tid; i < N; i += kT)
                    nxt[i] = i + span < N ? min(cur[i], cur[i + span]) : cur[i];
                __syncthreads();
                uint32_t* t = cur;
                cur = nxt, nxt = t;
            }
            // M of nodes B0 - H .. B0 + nb + H: two spans cover a window
            const int Nm = nb + 2 * H + 1;
            for (int i = tid; i < Nm; i += kT)
                nxt[i] = min(cur[i], cur[i + W - span]);
            __syncthreads();
            {
                uint32_t* t = cur;
                cur = nxt, nxt = t;
            }
            // the sum of W consecutive M: cur[i] = sum M[i .. i + span - 1]; a node adds the spans of the bits of W
            uint32_t acc[2] = {0, 0};
            int off = 0;
            for (span = 1; span <= W; span *= 2) {
                if (W & span) {
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        const int m = tid + kT * e;
                        if (m <= nb)
                            acc[e] += cur[m + off];
                    }
                    off += span;
                }
                if (2 * span <= W) {
                    for (int i = tid; i < Nm; i += kT)
                        nxt[i] = cur[i] + (i + span < Nm ? cur[i + span] : 0);
                    __syncthreads();
                    uint32_t* t = cur;
                    cur = nxt, nxt = t;
                }
            }
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int m = tid + kT * e;
                if (m <= nb)
                    s_node[m] = limit::average(acc[e], (uint32_t)W);
            }
            __syncthreads();
        }

        const int64_t s0 = tile * limit::kTile * a.bk;  // the tile's first sample, counted from the call's first
        for (int k = tid; k < nb * pb; k += kT) {
            const int64_t base = s0 + 8 * k;
            if (base >= n)
                break;
            uint32_t num = 0, d = 0;
            if (limited) {
                const int bl = (int)limit::div_bk((uint32_t)(8 * k), a.div);
                const uint32_t a0 = s_node[bl], a1 = s_node[bl + 1];
                num = limit::lerp_num(a0, a1, a.bk, 8 * k - bl * a.bk);
                d = a1 - a0;  // (modulo 2^32: num + i d is the numerator of sample i)
            }
            if (base + 8 <= n) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(src + base);
                u32x4 y;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int g0 = limited ? (int)limit::div_bk(num + (2 * i) * d, a.div) : (int)G;
                    const int g1 = limited ? (int)limit::div_bk(num + (2 * i + 1) * d, a.div) : (int)G;
                    y[i] = (uint32_t)(uint16_t)loud::apply_gain(lo16(v[i]), g0) | ((uint32_t)(uint16_t)loud::apply_gain(hi16(v[i]), g1) << 16);
                }
                *reinterpret_cast<u32x4*>(dst + base) = y;
            } else {
                for (int64_t i = base; i < n; i++) {
                    const int g = limited ? (int)limit::div_bk(num + (uint32_t)(i - base) * d, a.div) : (int)G;
                    dst[i] = (int16_t)loud::apply_gain(src[i], g);
                }
            }
        }
        __syncthreads();  // the next tile's writers wait for the readers of s_row and s_node
    }
}

}  // namespace efx
