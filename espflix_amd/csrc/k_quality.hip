// k_quality.hip -- how close one batch of pictures is to another (efx_compare_pictures): per image and plane the sum of
// squared errors and the sum of the Q16 SSIM of x264's 8 x 8 windows on the 4-pel grid, and per macroblock the luma SSE.
// The arithmetic is quality_px.h's: an integer function of the two pictures' bytes (the definition: include/efx.h), the
// same functions on the host and here.
//
// k_quality_zero   the records of every image to 0 (the bands of an image add into them).
// k_quality / k_quality_clamp  (without and with the reference clamp, so that ref_max 0 / 255 does not pay for it)
//                  one workgroup of 192 threads per image and band; a band is a macroblock row: 16 luma rows and 8 rows
//                  of each chroma plane, 8448 bytes of each picture.  A thread takes 16 pels x 4 rows of a plane -- four
//                  4 x 4 blocks side by side, in luma a macroblock's block row -- as four 16-byte loads from each
//                  picture, all eight in flight at once, and makes the four blocks' sums from the packed words: v_sad_u8
//                  against 0 for s1 and s2, v_dot4_u32_u8 for ss and s12.  The SSE is ss - 2 s12, so it costs no further
//                  pass over the pels; a macroblock's SSE is that of its four tasks, added in LDS.  The block sums go to
//                  LDS (11 KB), and after one barrier a thread takes windows: four 16-byte LDS reads, two 32 x 32 -> 64
//                  bit products each for num and den, and the quotient from a v_rcp_f32 estimate corrected exactly with
//                  the 64-bit remainder.  The windows' q are summed across a wave with lane shuffles.
//                  The windows of a band's last block row need the first block row of the next band.  That row's sums
//                  are recomputed from its pels (a fifth luma block row and a third chroma one: 25 % more bytes asked
//                  for, which the neighbouring band's workgroup, dispatched next to this one, asks for at the same time
//                  -- they meet in L2), not handed over: a hand-over between workgroups would need a flag, a fence and a
//                  wait per band, for 2112 bytes.
//                  A band's six sums fit 32 bits; they meet in LDS and leave as six 8-byte integer atomic adds per
//                  workgroup.  Integer sums: the order of the adds does not show.  The macroblock map is written with
//                  plain stores, 22 words per band.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "quality_px.h"

namespace efx {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(qpx::Block) == 16 && sizeof(efx_compare_rec) == 48, "a block's sums are one 16-byte LDS access; the record is six 8-byte words");
static_assert(qpx::kThreads >= 22 * 5 + 2 * 11 * 3 && qpx::kThreads >= 64 + 22, "every block task of a band has a thread; the map's 22 words leave from the second wave");

constexpr int kOutSse = 0, kOutSsim = 3, kOutMb = 6, kOutWords = 6 + 22;

__device__ inline int32_t wave_sum(int32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_xor(v, d);
    return v;
}

template <bool CLAMP>
__device__ void compare_band(const QualityArgs& a, size_t image, int band, qpx::Block* s_blk, uint32_t* s_out)
{
    const int tid = threadIdx.x;
    const uint8_t* ref = a.ref + image * a.ref_stride;
    const uint8_t* test = a.test + image * a.test_stride;
    if (tid < kOutWords)
        s_out[tid] = 0;

    const qpx::BlockTask t = qpx::block_task(band, tid);
    uint32_t sse = 0;
    if (t.valid) {
        const int width = qpx::plane_width(t.plane);
        const int off = qpx::task_offset(band, t, 0);
        u32x4 va[4], vb[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            va[r] = *reinterpret_cast<const u32x4*>(ref + off + r * width);
            vb[r] = *reinterpret_cast<const u32x4*>(test + off + r * width);
        }
        u32x4* dst = reinterpret_cast<u32x4*>(s_blk + qpx::task_stage(t));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            qpx::Block k{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; r++)
                qpx::add_row(CLAMP ? qpx::clamp4(va[r][j], (uint32_t)a.ref_max) : va[r][j], vb[r][j], &k);
            u32x4 v;
            v[0] = k.s1, v[1] = k.s2, v[2] = k.ss, v[3] = k.s12;
            dst[j] = v;
            sse += qpx::block_sse(k);
        }
    }
    __syncthreads();  // (the block sums are in LDS, the band's sums are 0)
    // (luma: a macroblock's four tasks meet in its word, the band's SSE is the 22 words' sum)
    if (t.valid && !t.halo)
        atomicAdd(&s_out[t.plane == 0 ? kOutMb + t.quad : kOutSse + t.plane], sse);

    int32_t q0 = 0, q1 = 0, q2 = 0;
    const int total = qpx::band_windows(band);
    for (int w = tid; w < total; w += qpx::kThreads) {
        const qpx::WindowTask wt = qpx::window_task(band, w);
        const qpx::Block* b = s_blk + qpx::window_stage(wt);
        const int down = qpx::block_cols(wt.plane);
        const int32_t q = qpx::window_q16(b[0], b[1], b[down], b[down + 1]);
        if (wt.plane == 0)
            q0 += q;
        else if (wt.plane == 1)
            q1 += q;
        else
            q2 += q;
    }
    q0 = wave_sum(q0), q1 = wave_sum(q1), q2 = wave_sum(q2);
    if ((tid & 63) == 0) {
        atomicAdd(&s_out[kOutSsim + 0], (uint32_t)q0);
        atomicAdd(&s_out[kOutSsim + 1], (uint32_t)q1);
        atomicAdd(&s_out[kOutSsim + 2], (uint32_t)q2);
    }
    __syncthreads();

    // (a band's SSE is at most 5632 x 65025, its SSIM sum at most 348 x 65536 in magnitude: 32 bits each)
    unsigned long long* rec = reinterpret_cast<unsigned long long*>(a.recs + 6 * image);
    if (tid == 0) {
        uint32_t luma = 0;
        for (int c = 0; c < 22; c++)
            luma += s_out[kOutMb + c];
        atomicAdd(&rec[0], (unsigned long long)luma);
    } else if (tid < 3)
        atomicAdd(&rec[tid], (unsigned long long)s_out[kOutSse + tid]);
    else if (tid < 6)
        atomicAdd(&rec[tid], (unsigned long long)(long long)(int32_t)s_out[tid]);
    if (a.mb_sse && tid >= 64 && tid < 64 + 22)
        a.mb_sse[image * a.mb_stride + 22 * band + (tid - 64)] = s_out[kOutMb + tid - 64];
    __syncthreads();  // (the workgroup's next band uses the same LDS)
}

template <bool CLAMP>
__device__ inline void compare_items(const QualityArgs& a, qpx::Block* s_blk, uint32_t* s_out)
{
    const size_t total = (size_t)a.n_images * qpx::kBands;
    for (size_t item = blockIdx.x; item < total; item += gridDim.x) {
        const size_t image = item / qpx::kBands;
        compare_band<CLAMP>(a, image, (int)(item - image * qpx::kBands), s_blk, s_out);
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_quality_zero(QualityArgs a)
{
    const size_t total = (size_t)a.n_images * 3;  // 16-byte pieces
    ulonglong2* out = reinterpret_cast<ulonglong2*>(a.recs);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        out[i] = make_ulonglong2(0, 0);
}

__global__ __launch_bounds__(qpx::kThreads) void k_quality(QualityArgs a)
{
    __shared__ __attribute__((aligned(16))) qpx::Block s_blk[qpx::kStageBlocks];
    __shared__ uint32_t s_out[kOutWords];
    compare_items<false>(a, s_blk, s_out);
}

__global__ __launch_bounds__(qpx::kThreads) void k_quality_clamp(QualityArgs a)
{
    __shared__ __attribute__((aligned(16))) qpx::Block s_blk[qpx::kStageBlocks];
    __shared__ uint32_t s_out[kOutWords];
    compare_items<true>(a, s_blk, s_out);
}

}  // namespace efx
