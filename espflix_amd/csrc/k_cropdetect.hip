// k_cropdetect.hip -- the black borders of source pictures (efx_detect_crop): row and column sums of the luma of every
// image, and from them one crop rectangle per stream.  The arithmetic is crop_px.h's: an integer function of the source
// bytes (the definition: include/efx.h), the same functions on the host and here.
//
// k_crop_zero   the column sums of every image to 0 (the bands of an image add into them).
// k_crop_sums_i420 / _rgb24 / _rgbp  (one kernel per source format, each with its own register count)
//               one workgroup per image and band of 64 rows; it reads the band's luma bytes (RGB: all three components)
//               once.  Rows are staged a few at a time in LDS with 16-byte loads from the 16-byte piece their first byte
//               lies in (rows start anywhere; the pieces stay inside the image rounded up to 16 bytes).  A wave owns whole
//               rows, a lane 4 adjacent columns of every 256: it reads them as aligned words, converts RGB to luma, keeps
//               the column sums of its band in registers (two 16-bit sums to a register) and its share of the row sum,
//               which the wave reduces with lane shuffles and stores.  At the end of the band the four waves' column sums
//               meet in LDS and leave as one 4-byte integer atomic add per column: 4 / (64 x bytes per pixel) of the
//               source bytes, 2 % for RGB and 6 % for I420, in wave instructions of 256 contiguous bytes.  Integer sums:
//               the order of the adds does not show.
// k_crop_sums_surf8 / _surf16  the same for the luma plane of an efx_surface of bytes or of 16-bit words (surface_px.h):
//               rows lie a pitch apart behind the plane's offset, a word is reduced to a byte as it is read, two samples
//               to a dword.  The chroma planes are never read.
// k_crop_rects  one workgroup per stream.  A wave takes an image: it classifies the image's rows and columns, finds the
//               first and last picture row and column by min / max across its lanes, and folds a contributing image into
//               the wave's bounds; the four waves' bounds meet in LDS, lane 0 rounds them and writes the record.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "crop_px.h"
#include "surface_px.h"

namespace efx {

namespace {

constexpr int kThreads = 64 * cpx::kWaves;
static_assert(cpx::kStageBytes % 16 == 0 && cpx::kStageBytes >= 4 * (kImportMaxWidth + 4), "the stage holds the column sums of a band");
static_assert(cpx::kStageBytes >= 3 * (((kImportMaxWidth + 30) >> 4) * 16 + 16) && cpx::kStageBytes >= ((3 * kImportMaxWidth + 30) >> 4) * 16 + 16,
              "the stage holds a row of every format");
static_assert(cpx::kStageBytes >= ((2 * kImportMaxWidth + 30) >> 4) * 16 + 16, "the stage holds a luma row of 16-bit words");
static_assert(cpx::kLaneCols * 64 * cpx::kColGroups >= kImportMaxWidth && cpx::kBandRows * 255 < 65536, "a lane's 16-bit column sums");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ inline uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ inline int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ inline int wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v = max(v, __shfl_xor(v, d));
    return v;
}

// sum_band's source: FORMAT is an efx_pixel_format and ARGS CropArgs, or FORMAT says whether the luma plane of a surface
// holds bytes or words and ARGS is CropSurfArgs, which says where the plane lies
constexpr int kSurf8 = 100, kSurf16 = 101;
__device__ inline const CropArgs& crop_args(const CropArgs& a) { return a; }
__device__ inline const CropArgs& crop_args(const CropSurfArgs& a) { return a.c; }
template <int FORMAT>
__device__ inline cpx::Layout band_layout(int W)
{
    if (FORMAT == kSurf8 || FORMAT == kSurf16)
        return spx::crop_layout(W, FORMAT == kSurf16 ? 2 : 1);
    return cpx::layout(FORMAT, W);
}
template <int FORMAT>
__device__ inline size_t band_seg_offset(const CropArgs&, int s, int W, int H, int y)
{
    return cpx::seg_offset(FORMAT, s, W, H, y);
}
template <int FORMAT>
__device__ inline size_t band_seg_offset(const CropSurfArgs& a, int, int, int, int y)
{
    return a.y_offset + (size_t)y * a.y_pitch;
}
template <int FORMAT>
__device__ inline uint32_t band_luma4(const CropArgs&, const ipx::Matrix& m, const uint32_t* seg, int seg_cap, const int shift[3], int x, int W)
{
    return cpx::luma4<FORMAT>(m, seg, seg_cap, shift, x, W);
}
template <int FORMAT>
__device__ inline uint32_t band_luma4(const CropSurfArgs& a, const ipx::Matrix&, const uint32_t* seg, int, const int shift[3], int x, int W)
{
    return spx::luma4<FORMAT == kSurf16>(seg, shift[0], x, W, a.shift);
}

// One band of one image: R[y] of its rows stored, its share of C[x] added.  s_stage: kStageBytes of LDS.
template <int FORMAT, class ARGS>
__device__ void sum_band(const ARGS& args, const uint8_t* __restrict__ img, uint32_t* __restrict__ sums, int band, uint32_t* s_stage)
{
    const CropArgs& a = crop_args(args);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.width, H = a.height;
    const cpx::Layout L = band_layout<FORMAT>(W);
    const ipx::Matrix m = ipx::matrix(a.full_range);
    const int y0 = band * cpx::kBandRows, y1 = min(y0 + cpx::kBandRows, H);
    const int slots = L.seg_cap >> 4;  // 16-byte places of a segment's slot
    uint32_t even[cpx::kColGroups] = {}, odd[cpx::kColGroups] = {};

    for (int g0 = y0; g0 < y1; g0 += L.group_rows) {
        const int g = min(L.group_rows, y1 - g0);
        // the group's rows into LDS, two pieces per lane in flight
        const int total = g * L.nseg * slots;
        for (int p = tid; p < total; p += 2 * kThreads) {
            u32x4 v[2];
            int at[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int q = p + k * kThreads;
                const int slot = q / slots, i = q - slot * slots;
                const int row = slot / L.nseg, s = slot - row * L.nseg;
                at[k] = -1;
                if (q < total) {
                    const ipx::Span sp = ipx::span(band_seg_offset<FORMAT>(args, s, W, H, g0 + row), L.seg_len);
                    if (i < sp.pieces) {
                        v[k] = *reinterpret_cast<const u32x4*>(img + sp.a0 + 16 * (size_t)i);
                        at[k] = slot * L.seg_cap + 16 * i;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 2; k++)
                if (at[k] >= 0)
                    *reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(s_stage) + at[k]) = v[k];
        }
        __syncthreads();
        for (int r = wave; r < g; r += cpx::kWaves) {
            int shift[3] = {0, 0, 0};
            for (int s = 0; s < L.nseg; s++)
                shift[s] = ipx::span(band_seg_offset<FORMAT>(args, s, W, H, g0 + r), L.seg_len).shift;
            const uint32_t* seg = s_stage + ((r * L.nseg * L.seg_cap) >> 2);
            uint32_t rs = 0;
#pragma unroll
            for (int j = 0; j < cpx::kColGroups; j++) {
                if (256 * j < W) {
                    const int x = 256 * j + cpx::kLaneCols * lane;
                    if (x < W)
                        rs += cpx::add4(band_luma4<FORMAT>(args, m, seg, L.seg_cap, shift, x, W), &even[j], &odd[j]);
                }
            }
            rs = wave_sum(rs);
            if (lane == 0)
                sums[g0 + r] = rs;
        }
        __syncthreads();  // (the next group's fetch overwrites the rows)
    }

    // the waves' column sums meet in LDS (columns at or beyond the width hold 0 and land behind the sums that leave)
    for (int x = tid; x < W + 4; x += kThreads)
        s_stage[x] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < cpx::kColGroups; j++) {
        if (256 * j < W) {
            const int x = 256 * j + cpx::kLaneCols * lane;
            if (x < W) {
                atomicAdd(&s_stage[x], even[j] & 0xFFFF);
                atomicAdd(&s_stage[x + 1], odd[j] & 0xFFFF);
                atomicAdd(&s_stage[x + 2], even[j] >> 16);
                atomicAdd(&s_stage[x + 3], odd[j] >> 16);
            }
        }
    }
    __syncthreads();
    for (int x = tid; x < W; x += kThreads)
        atomicAdd(&sums[H + x], s_stage[x]);
    __syncthreads();  // (the workgroup's next band stages into the same LDS)
}

}  // namespace

__global__ __launch_bounds__(256) void k_crop_zero(CropArgs a)
{
    const size_t total = (size_t)a.n_images * a.width;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t k = i / a.width;
        a.sums[k * a.sums_stride + a.height + (i - k * a.width)] = 0;
    }
}

// (a kernel per format: each is compiled to its own register count)
template <int FORMAT, class ARGS>
__device__ inline void sum_items(const ARGS& args, uint32_t* s_stage)
{
    const CropArgs& a = crop_args(args);
    const int bands = (a.height + cpx::kBandRows - 1) / cpx::kBandRows;
    const size_t total = (size_t)a.n_images * bands;
    for (size_t item = blockIdx.x; item < total; item += gridDim.x) {
        const size_t image = item / bands;
        sum_band<FORMAT>(args, a.src + image * a.src_stride, a.sums + image * a.sums_stride, (int)(item - image * bands), s_stage);
    }
}

__global__ __launch_bounds__(256) void k_crop_sums_i420(CropArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[cpx::kStageBytes / 4];
    sum_items<EFX_PIX_I420>(a, s_stage);
}

__global__ __launch_bounds__(256) void k_crop_sums_rgb24(CropArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[cpx::kStageBytes / 4];
    sum_items<EFX_PIX_RGB24>(a, s_stage);
}

__global__ __launch_bounds__(256) void k_crop_sums_rgbp(CropArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[cpx::kStageBytes / 4];
    sum_items<EFX_PIX_RGBP>(a, s_stage);
}

__global__ __launch_bounds__(256) void k_crop_sums_surf8(CropSurfArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[cpx::kStageBytes / 4];
    sum_items<kSurf8>(a, s_stage);
}

__global__ __launch_bounds__(256) void k_crop_sums_surf16(CropSurfArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[cpx::kStageBytes / 4];
    sum_items<kSurf16>(a, s_stage);
}

__global__ __launch_bounds__(256) void k_crop_rects(CropArgs a)
{
    __shared__ int s_bounds[cpx::kWaves][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.width, H = a.height;
    for (size_t stream = blockIdx.x; stream < (size_t)a.n_streams; stream += gridDim.x) {
        int x1 = W, y1 = H, x2 = -1, y2 = -1;
        for (int i = wave; i < a.images_per_stream; i += cpx::kWaves) {
            const uint32_t* sums = a.sums + (stream * a.images_per_stream + i) * a.sums_stride;
            int top = H, bottom = -1, left = W, right = -1;
            for (int y = lane; y < H; y += 64)
                if (cpx::is_picture(sums[y], a.limit, W))
                    top = min(top, y), bottom = max(bottom, y);
            for (int x = lane; x < W; x += 64)
                if (cpx::is_picture(sums[H + x], a.limit, H))
                    left = min(left, x), right = max(right, x);
            top = wave_min(top), bottom = wave_max(bottom), left = wave_min(left), right = wave_max(right);
            if (bottom >= 0 && right >= 0)  // a picture row and a picture column: the image contributes
                x1 = min(x1, left), y1 = min(y1, top), x2 = max(x2, right), y2 = max(y2, bottom);
        }
        if (lane == 0)
            s_bounds[wave][0] = x1, s_bounds[wave][1] = y1, s_bounds[wave][2] = x2, s_bounds[wave][3] = y2;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < cpx::kWaves; w++)
                x1 = min(x1, s_bounds[w][0]), y1 = min(y1, s_bounds[w][1]), x2 = max(x2, s_bounds[w][2]), y2 = max(y2, s_bounds[w][3]);
            int32_t rec[8];
            cpx::record(W, H, a.round, x1, y1, x2, y2, rec);
            int4* out = reinterpret_cast<int4*>(a.rects + stream * 8);
            out[0] = make_int4(rec[0], rec[1], rec[2], rec[3]);
            out[1] = make_int4(rec[4], rec[5], rec[6], rec[7]);
        }
        __syncthreads();
    }
}

}  // namespace efx
