// k_export.hip -- ring frames out as standard pictures: planar YUV 4:2:0 (I420) or RGB (interleaved HWC / planar CHW).
//
// The ring holds pictures in the reference's strip layout (12 strips x 16 rows x 528 bytes; a row is 352 luma bytes and
// 176 bytes of ONE chroma plane: strip rows 0-7 carry Cb, 8-15 Cr -- reference src/player.cpp:20-46 names them the other
// way round, see include/efx.h).  k_export un-shuffles it and, for RGB, upsamples the chroma and applies the BT.601
// matrix of export_px.h, in one pass over every selected stream.
//
// Work decomposition: an item is 16 luma columns x 2 rows (2y, 2y + 1) of one picture -- the two rows share chroma row
// y -- and a workgroup converts kExportItemsPerBlock consecutive items (the items of consecutive streams follow one
// another, as k_composite's 8-sample groups do).  Every global access is 16 bytes: two luma loads, per chroma plane one
// load per chroma row (the 16 bytes that hold the chroma of this item and of its even / odd partner; the partner loads the
// same line), stores of 16 (I420 / planar) or 3 x 16 (RGB24) bytes per row.  Bilinear chroma needs the rows y - 1 and
// y + 1 as well (MPEG-1 siting: luma row 2y takes 3/4 of chroma row y and 1/4 of row y - 1, row 2y + 1 1/4 of y + 1) and
// one chroma column on each side of the item: one of them lies inside the 16 loaded bytes, the other in the neighbouring
// lane's (ds_bpermute), or -- for the first and last lane of a wave -- in one extra 4-byte load.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "export_px.h"
#include "ring_px.h"

namespace efx {

namespace {

constexpr int kYBytes = EFX_FRAME_WIDTH * EFX_FRAME_HEIGHT;  // I420 / RGBP plane offsets
constexpr int kCBytes = kYBytes / 4;

using ring::chroma_row_off;  // (ring_px.h: shared with k_trick.hip)
using ring::luma_row_off;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ inline u32x4 load16(const uint8_t* p) { return *reinterpret_cast<const u32x4*>(p); }
// Plain stores: the L2 assembles whole lines from the lanes' 16-byte pieces before they go out.  Non-temporal stores
// (k_composite's choice) measured 2-15 % slower here and wrote 1.27-1.40 x the RGB24 bytes (profiles/export.md).
__device__ inline void store16(uint8_t* p, u32x4 v) { *reinterpret_cast<u32x4*>(p) = v; }

__device__ inline int byte_of(uint32_t w, int k) { return (int)((w >> (8 * k)) & 0xFF); }

// The ten chroma samples of one chroma row an item's bilinear taps reach: columns 8g - 1 ... 8g + 8 (clamped at the edges
// of the picture).  `line` = the 16 loaded bytes (columns 16 (g >> 1) ...), `outer` = the dword from the neighbour that
// holds the column outside them (even g: column 8g - 1 in its top byte; odd g: column 8g + 8 in its low byte).
__device__ inline void chroma_span(u32x4 line, uint32_t outer, int g, int c[10])
{
    const bool odd = g & 1;
    const uint32_t w0 = odd ? line.z : line.x, w1 = odd ? line.w : line.y;  // this item's eight columns
#pragma unroll
    for (int k = 0; k < 4; k++) {
        c[1 + k] = byte_of(w0, k);
        c[5 + k] = byte_of(w1, k);
    }
    // even g: the left column lies outside the line, the right one is the first of the odd half; odd g: mirror image
    c[0] = odd ? byte_of(line.y, 3) : (g == 0 ? c[1] : byte_of(outer, 3));
    c[9] = odd ? (g == EFX_FRAME_WIDTH / 16 - 1 ? c[8] : byte_of(outer, 0)) : byte_of(line.z, 0);
}

// The dword a lane hands its neighbour (see chroma_span): the odd lane of a pair gives its line's last dword to the even
// lane on its right, the even lane its first dword to the odd lane on its left.
__device__ inline uint32_t neighbour_dword(u32x4 line, int g, int lane, const uint8_t* row_base)
{
    const bool odd = g & 1;
    const uint32_t give = odd ? line.w : line.x;
    const int src = odd ? lane + 1 : lane - 1;  // (item parity = lane parity: items per picture and per block are even)
    uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute((src & 63) << 2, (int)give);
    // the first / last lane of a wave: the neighbour belongs to another wave -- one 4-byte load (inside the same chroma row)
    if ((lane == 0 && !odd && g != 0) || (lane == 63 && odd && g != EFX_FRAME_WIDTH / 16 - 1))
        got = *reinterpret_cast<const uint32_t*>(row_base + (odd ? 8 * g + 8 : 8 * g - 4));
    return got;
}

// 16 pixels of one luma row (four dwords) with their chroma -> 16 packed 0x00BBGGRR values
template <int CHROMA>
__device__ inline void convert_row(const px::Matrix& m, u32x4 luma, const int* u_near, const int* u_far, const int* v_near,
                                   const int* v_far, uint32_t out[16])
{
    const uint32_t yw[4] = {luma.x, luma.y, luma.z, luma.w};
    int vu[10], vv[10];
    if (CHROMA == EFX_CHROMA_BILINEAR) {
#pragma unroll
        for (int k = 0; k < 10; k++) {
            vu[k] = px::vtap(u_near[k], u_far[k]);
            vv[k] = px::vtap(v_near[k], v_far[k]);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int y = byte_of(yw[i >> 2], i & 3);
        const int j = 1 + (i >> 1);                   // chroma column x >> 1 in the span
        const int jn = (i & 1) ? j + 1 : j - 1;       // its neighbour on the side of x
        int u, v;
        if (CHROMA == EFX_CHROMA_BILINEAR) {
            u = px::htap(vu[j], vu[jn]);
            v = px::htap(vv[j], vv[jn]);
        } else {
            u = u_near[j];
            v = v_near[j];
        }
        out[i] = px::rgb(m, y, u, v);
    }
}

}  // namespace

template <int FMT, int CHROMA>
__global__ __launch_bounds__(256) void k_export(const uint8_t* __restrict__ frames, int n_streams, ExportArgs a)
{
    const uint32_t total = (uint32_t)n_streams * kExportItemsPerPicture;  // < 2^32: 2^32 / 2112 ring frames exceed any HBM
    const int lane = threadIdx.x & 63;
    const px::Matrix m = px::matrix(a.full_range);
    for (int k = threadIdx.x; k < kExportItemsPerBlock; k += blockDim.x) {
        const uint32_t item0 = blockIdx.x * (uint32_t)kExportItemsPerBlock + (uint32_t)k;
        if (item0 - lane >= total)
            break;  // (wave-uniform: every lane of a wave that has work stays for the lane exchange)
        const bool live = item0 < total;
        const uint32_t item = live ? item0 : total - 1;  // lanes past the end re-read the last item and store nothing
        const int s = (int)(item / kExportItemsPerPicture);
        const int r = (int)(item - (uint32_t)s * kExportItemsPerPicture);
        const int cy = r / (EFX_FRAME_WIDTH / 16), g = r - cy * (EFX_FRAME_WIDTH / 16);
        const int stream = a.first_stream + s;

        int slot = a.slot;
        if (slot < 0)
            // picture mode: the ring position k_advance recorded for this stream's group (efx_stream_picture_slot)
            slot = ring::picture_slot(a, stream, a.picture);
        const uint8_t* fr = frames + ((size_t)stream * a.ring_depth + slot) * kFrameBytes;
        uint8_t* dst = a.dst + (size_t)s * a.dst_stride;
        const int y0 = 2 * cy;
        const u32x4 l0 = load16(fr + luma_row_off(y0) + 16 * g);
        const u32x4 l1 = load16(fr + luma_row_off(y0 + 1) + 16 * g);
        const int cline = 16 * (g >> 1);  // the chroma bytes of this item and its partner

        if (FMT == EFX_PIX_I420) {
            // planes as they are: the even lane of a pair moves the pair's 16 Cb bytes, the odd lane the 16 Cr bytes
            const int plane = (g & 1) ? 2 : 1;
            const u32x4 c = load16(fr + chroma_row_off(plane, cy) + cline);
            if (live) {
                store16(dst + y0 * EFX_FRAME_WIDTH + 16 * g, l0);
                store16(dst + (y0 + 1) * EFX_FRAME_WIDTH + 16 * g, l1);
                store16(dst + kYBytes + (plane == 2 ? kCBytes : 0) + cy * (EFX_FRAME_WIDTH / 2) + cline, c);
            }
            continue;
        }

        // chroma rows: cy, and for bilinear cy - 1 (for luma row 2 cy) and cy + 1 (for 2 cy + 1), clamped
        int un[10], vn[10], ua[10], va[10], ub[10], vb[10];
        {
            const uint8_t* ur = fr + chroma_row_off(1, cy);
            const uint8_t* vr = fr + chroma_row_off(2, cy);
            const u32x4 uc = load16(ur + cline), vc = load16(vr + cline);
            if (CHROMA == EFX_CHROMA_BILINEAR) {
                const int ya = cy > 0 ? cy - 1 : 0, yb = cy < EFX_FRAME_HEIGHT / 2 - 1 ? cy + 1 : cy;
                const uint8_t* uar = fr + chroma_row_off(1, ya);
                const uint8_t* var = fr + chroma_row_off(2, ya);
                const uint8_t* ubr = fr + chroma_row_off(1, yb);
                const uint8_t* vbr = fr + chroma_row_off(2, yb);
                const u32x4 uac = load16(uar + cline), vac = load16(var + cline);
                const u32x4 ubc = load16(ubr + cline), vbc = load16(vbr + cline);
                chroma_span(uc, neighbour_dword(uc, g, lane, ur), g, un);
                chroma_span(vc, neighbour_dword(vc, g, lane, vr), g, vn);
                chroma_span(uac, neighbour_dword(uac, g, lane, uar), g, ua);
                chroma_span(vac, neighbour_dword(vac, g, lane, var), g, va);
                chroma_span(ubc, neighbour_dword(ubc, g, lane, ubr), g, ub);
                chroma_span(vbc, neighbour_dword(vbc, g, lane, vbr), g, vb);
            } else {
                chroma_span(uc, 0, g, un);  // (nearest: columns 1 ... 8 of the span only)
                chroma_span(vc, 0, g, vn);
            }
        }

#pragma unroll
        for (int row = 0; row < 2; row++) {
            uint32_t p[16];
            convert_row<CHROMA>(m, row ? l1 : l0, un, row ? ub : ua, vn, row ? vb : va, p);
            const int y = y0 + row;
            if (!live)
                continue;
            if (FMT == EFX_PIX_RGB24) {
                // 16 x 3 bytes = three dwordx4: four pixels make three dwords
                uint32_t w[12];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t a0 = p[4 * q], a1 = p[4 * q + 1], a2 = p[4 * q + 2], a3 = p[4 * q + 3];
                    w[3 * q] = a0 | (a1 << 24);
                    w[3 * q + 1] = (a1 >> 8) | (a2 << 16);
                    w[3 * q + 2] = (a2 >> 16) | (a3 << 8);
                }
                uint8_t* o = dst + (size_t)y * (3 * EFX_FRAME_WIDTH) + 48 * g;
                store16(o, u32x4{w[0], w[1], w[2], w[3]});
                store16(o + 16, u32x4{w[4], w[5], w[6], w[7]});
                store16(o + 32, u32x4{w[8], w[9], w[10], w[11]});
            } else {
                // planar R, G, B: byte c of every pixel
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    uint32_t w[4];
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        w[q] = ((p[4 * q] >> (8 * c)) & 0xFF) | (((p[4 * q + 1] >> (8 * c)) & 0xFF) << 8) |
                               (((p[4 * q + 2] >> (8 * c)) & 0xFF) << 16) | (((p[4 * q + 3] >> (8 * c)) & 0xFF) << 24);
                    store16(dst + c * kYBytes + y * EFX_FRAME_WIDTH + 16 * g, u32x4{w[0], w[1], w[2], w[3]});
                }
            }
        }
    }
}

template __global__ void k_export<EFX_PIX_I420, EFX_CHROMA_NEAREST>(const uint8_t*, int, ExportArgs);
template __global__ void k_export<EFX_PIX_RGB24, EFX_CHROMA_NEAREST>(const uint8_t*, int, ExportArgs);
template __global__ void k_export<EFX_PIX_RGB24, EFX_CHROMA_BILINEAR>(const uint8_t*, int, ExportArgs);
template __global__ void k_export<EFX_PIX_RGBP, EFX_CHROMA_NEAREST>(const uint8_t*, int, ExportArgs);
template __global__ void k_export<EFX_PIX_RGBP, EFX_CHROMA_BILINEAR>(const uint8_t*, int, ExportArgs);

}  // namespace efx
