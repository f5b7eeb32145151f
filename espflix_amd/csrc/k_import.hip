// k_import.hip -- pictures in: I420 / RGB24 / RGBP pictures of any size cropped, scaled and converted to the 352 x 192
// I420 layout efx_encode reads (the inverse of k_export).  The arithmetic is import_px.h's: an integer function of the
// source bytes (the formulas: include/efx.h), the same functions on the host and here.
//
// k_import_taps  one lane per axis (luma columns / rows, chroma columns / rows) and destination index: the window and its
//                u16 coefficients into the context's table.  It runs in stream order in front of k_import, so queued calls
//                with different geometry never share a table's content.
// k_import       one workgroup per image and band of 8 luma rows (4 rows of each chroma plane).  It walks the source rows
//                of the band's vertical support: a row is fetched into LDS with 16-byte loads from the 16-byte piece its
//                first byte lies in (rows start anywhere; the pieces stay inside the image rounded up to 16 bytes), an RGB
//                row is converted there into three byte rows, so one read of the source makes all three planes.  A lane
//                owns destination columns (2 luma columns, 2 chroma columns): it forms the 16-bit horizontal sum of the
//                row and adds k_y * h into one register per destination row.  The band is assembled in LDS on the border
//                colour and leaves as 16-byte stores: the whole 101376 bytes of an image are written, nothing else.
// k_import_surf8p / 8s / 16p / 16s  the same band walk for the four layouts of an efx_surface (surface_px.h): a luma or
//                planar chroma row is staged from its plane's offset and pitch, a pair row is staged once and
//                de-interleaved into the Cb and Cr byte rows, and 16-bit rows are reduced to bytes on the way from the
//                raw row to the byte rows, two samples to a dword.  A kernel per layout: k_import runs what it ran.
// k_import_surf8p_c / 8s_c / 16p_c / 16s_c  the surface kernels with the colour stage (colour_px.h; COLOUR = true): between
//                the lanes' columns into the band and the band's stores, the samples inside the destination rectangle are
//                converted from the source's matrix and range to BT.601 studio swing, in place in LDS.  An item is a
//                chroma site and its 2 x 2 luma samples, luma first (it reads the unconverted chroma); no two items share
//                a sample.  The coefficients come by value.  A packed I420 source with a conversion runs k_import_surf8p_c
//                (it is a planar surface of pitch = width), so k_import itself and the kernels without the stage are,
//                instruction for instruction, the code they were.
// k_import_surf8p_h / 8s_h / 16p_h / 16s_h  the surface kernels with the HDR stage (hdr_px.h; HDR = true): the lanes' columns
//                leave the accumulators at 10 bits (vround10) into a 16-bit band of their own, and between that and the
//                band's stores one item per lane and step -- a chroma site and its 2 x 2 luma samples inside the destination
//                rectangle -- goes through matrix, PQ EOTF and tone curve, gamut matrix, inverse BT.1886 and the BT.601
//                matrix into the 8-bit band, which leaves as before.  The two tables (10.7 KB for one peak) are staged into
//                LDS once per workgroup: lanes gather different entries.  Both the 16-bit band and the tables live in the
//                row loaders' LDS, which is free once the band walk is over, so the kernels' LDS is the _c kernels'.  The
//                setting's coefficients and tables come through one pointer (the context keeps a device copy per
//                setting).  A kernel per layout again, so every kernel above is the code it was.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "efx.h"
#include "efx_internal.h"
#include "colour_px.h"
#include "hdr_px.h"
#include "import_px.h"
#include "surface_px.h"

namespace efx {

static_assert(kImportTapSlots >= ipx::kMaxTaps && kImportTapSlots % 4 == 0 && sizeof(ImportTap) % 16 == 0 && offsetof(ImportTap, k) == 8,
              "a tap record holds every window, its coefficients readable in 8-byte groups");

namespace {

constexpr int kW = EFX_FRAME_WIDTH, kH = EFX_FRAME_HEIGHT;
constexpr int kYBytes = kW * kH, kCBytes = kYBytes / 4;
constexpr int kRows = kImportBandRows, kCRows = kImportBandRows / 2;
constexpr int kRowBuf = kImportMaxWidth + 32;      // a byte row behind its alignment shift (<= 15), read four taps at a time
constexpr int kRawBuf = 3 * kRowBuf + 16;          // an RGB24 row (3 x 4096 + 15) or three RGBP rows, read 4 pixels at a time
constexpr int kBandY = kRows * kW, kBandC = kCRows * (kW / 2), kBandBytes = kBandY + 2 * kBandC;
constexpr int kRawHalf = (kRawBuf / 2) & ~15;      // where the second chroma row of a planar 16-bit surface is staged
constexpr int kThreads = 256;
// the widest surface rows: 4096 words of luma or 2048 word pairs (8192 bytes), or two rows of 2048 words side by side,
// each behind its alignment shift (<= 15) and read as aligned dwords, one beyond the last sample's
static_assert(kRawBuf >= 2 * kImportMaxWidth + 15 + 16 + 8 && kRawHalf >= kImportMaxWidth + 15 + 16 + 8,
              "s_raw holds the widest 16-bit luma row, pair row and pair of planar chroma rows");
static_assert(2 * kThreads >= kW, "a lane owns two luma columns and two chroma columns");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// bytes [off, off + len) of the image into buf (16-byte aligned LDS) as whole 16-byte pieces; the segment starts at
// buf + the returned shift
__device__ inline int stage(const uint8_t* __restrict__ img, size_t off, int len, uint8_t* buf)
{
    const ipx::Span sp = ipx::span(off, len);
    for (int i = threadIdx.x; i < sp.pieces; i += kThreads)
        *reinterpret_cast<u32x4*>(buf + 16 * i) = *reinterpret_cast<const u32x4*>(img + sp.a0 + 16 * (size_t)i);
    return sp.shift;
}

// The vertical coefficient of source row s for each of the band's destination rows (wave-uniform)
template <int R>
__device__ inline void vcoefs(const ImportTap* __restrict__ ty, int n, int s, int ky[R])
{
#pragma unroll
    for (int r = 0; r < R; r++) {
        ky[r] = 0;
        if (r < n) {
            const unsigned i = (unsigned)(s - ty[r].start);
            if (i < (unsigned)ty[r].count)
                ky[r] = ty[r].k[i];
        }
    }
}

// One destination column's share of a source row: the horizontal sum, rounded to 16 bits, into the rows' accumulators
template <int R>
__device__ inline void accumulate(const uint8_t* row, const ImportTap* __restrict__ tx, const int ky[R], int acc[R])
{
    // four taps per step, their coefficients in one 8-byte load: k_import_taps leaves zeros behind a window, and the up
    // to three bytes read behind it lie inside the row buffer (start + count <= 4096, shift <= 15)
    const int n = tx->count;
    const uint8_t* p = row + tx->start;
    const uint2* k4 = reinterpret_cast<const uint2*>(tx->k);
    int sum = 0;
    for (int i = 0; i < n; i += 4) {
        const uint2 w = k4[i >> 2];
        sum += (int)(w.x & 0xFFFF) * (int)p[i] + (int)(w.x >> 16) * (int)p[i + 1] + (int)(w.y & 0xFFFF) * (int)p[i + 2] +
               (int)(w.y >> 16) * (int)p[i + 3];
    }
    const int h = ipx::hround(sum);
#pragma unroll
    for (int r = 0; r < R; r++)
        acc[r] += ky[r] * h;
}

// The colour stage: the band's samples inside the destination rectangle, in place (s_out: the band's luma rows, then its Cb
// and its Cr rows).  One item per lane and step; a row of the rectangle has at most 176 items.
__device__ inline void convert_band(const ImportArgs& a, const colour::Coefs& k, int y0, uint8_t* s_out)
{
    const colour::BandPart p = colour::band_part(a.dst_x, a.dst_y, a.dst_w, a.dst_h, y0, kRows);
    for (int r = 0; r < p.rows; r++)
        for (int c = threadIdx.x; c < p.cols; c += kThreads)
            colour::convert_item(k, p, r, c, kW, s_out, s_out + kBandY, s_out + kBandY + kBandC);
    __syncthreads();
}

// The HDR stage: the band's items inside the destination rectangle from the 10-bit band (s_b10, laid out as s_out) into
// s_out.  tab: the setting's coefficients and first table in LDS, gam: its second table.
__device__ inline void tonemap_band(const ImportArgs& a, const hdr::Tables* tab, const uint16_t* gam, int y0, const uint16_t* s_b10,
                                    uint8_t* s_out)
{
    const colour::BandPart p = colour::band_part(a.dst_x, a.dst_y, a.dst_w, a.dst_h, y0, kRows);
    const hdr::Coefs k = tab->k;
    for (int r = 0; r < p.rows; r++)
        for (int c = threadIdx.x; c < p.cols; c += kThreads)
            hdr::tonemap_item(k, tab->pq, gam, p, r, c, kW, kRows, s_b10, s_out);
    __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(256) void k_import_taps(ImportTap* __restrict__ table, ImportArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kImportTapRows)
        return;
    // chroma: an I420 source brings half the crop, an RGB source is converted at full resolution
    const int half = a.format == EFX_PIX_I420 ? 2 : 1;
    int d, S, D;
    if (i < kImportTapLY) {
        d = i - kImportTapLX, S = a.crop_w, D = a.dst_w;
    } else if (i < kImportTapCX) {
        d = i - kImportTapLY, S = a.crop_h, D = a.dst_h;
    } else if (i < kImportTapCY) {
        d = i - kImportTapCX, S = a.crop_w / half, D = a.dst_w / 2;
    } else {
        d = i - kImportTapCY, S = a.crop_h / half, D = a.dst_h / 2;
    }
    if (d >= D)
        return;
    int n;
    table[i].start = ipx::taps(S, D, d, &n, table[i].k);
    table[i].count = n;
    for (int j = n; j < kImportTapSlots; j++)
        table[i].k[j] = 0;  // (k_import reads the coefficients four at a time)
}

__global__ __launch_bounds__(256) void k_import(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                const ImportTap* __restrict__ taps, ImportArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[kRawBuf];
    __shared__ __attribute__((aligned(16))) uint8_t s_row[3][kRowBuf];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kBandBytes];

    const int tid = threadIdx.x;
    const int band = (int)(blockIdx.x % kImportBands);
    const size_t image = blockIdx.x / kImportBands;
    const uint8_t* img = src + image * a.src_stride;
    uint8_t* out = dst + image * a.dst_stride;
    const bool rgb = a.format != EFX_PIX_I420;

    // the band on the border colour
    {
        const uint32_t black = (rgb && a.full_range) ? 0u : 0x10101010u;
        for (int i = tid; i < kBandBytes / 4; i += kThreads)
            reinterpret_cast<uint32_t*>(s_out)[i] = i < kBandY / 4 ? black : 0x80808080u;
    }

    // the band's rows inside the destination rectangle, as indices into the rectangle: luma [l0, l0 + nl), chroma
    // [c0, c0 + nc) (every coordinate of the rectangle is even, so the two agree)
    const int y0 = band * kRows, cy0 = band * kCRows;
    const int l0 = max(y0, a.dst_y) - a.dst_y, nl = min(y0 + kRows, a.dst_y + a.dst_h) - a.dst_y - l0;
    const int c0 = max(cy0, a.dst_y / 2) - a.dst_y / 2, nc = min(cy0 + kCRows, (a.dst_y + a.dst_h) / 2) - a.dst_y / 2 - c0;
    const ImportTap* tly = taps + kImportTapLY + l0;
    const ImportTap* tcy = taps + kImportTapCY + c0;

    // this lane's columns: luma tid and tid + 256; chroma items tid and tid + 256 of [Cb columns | Cr columns]
    const int cw2 = a.dst_w / 2;
    bool lv[2], cv[2];
    int cplane[2], ccol[2];
    const ImportTap* tlx[2];
    const ImportTap* tcx[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int col = tid + kThreads * j;
        lv[j] = col < a.dst_w;
        tlx[j] = taps + kImportTapLX + (lv[j] ? col : 0);
        cv[j] = col < a.dst_w;
        cplane[j] = col >= cw2 ? 1 : 0;
        ccol[j] = cv[j] ? col - cplane[j] * cw2 : 0;
        tcx[j] = taps + kImportTapCX + ccol[j];
    }
    int accl[2][kRows] = {}, accc[2][kCRows] = {};

    if (nl > 0) {  // (nl > 0 exactly when nc > 0)
        const int ls0 = tly[0].start, ls1 = tly[nl - 1].start + tly[nl - 1].count;  // source rows of the supports
        const int cs0 = tcy[0].start, cs1 = tcy[nc - 1].start + tcy[nc - 1].count;
        if (rgb) {
            const ipx::Matrix m = ipx::matrix(a.full_range);
            for (int s = min(ls0, cs0); s < max(ls1, cs1); s++) {
                int sh[3];
                if (a.format == EFX_PIX_RGB24) {
                    sh[0] = stage(img, ipx::rgb24_row(a.width, a.crop_x, a.crop_y, s), 3 * a.crop_w, s_raw);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        sh[c] = stage(img, ipx::rgbp_row(c, a.width, a.height, a.crop_x, a.crop_y, s), a.crop_w, s_raw + c * kRowBuf) +
                                c * kRowBuf;
                }
                __syncthreads();
                // four pixels per lane and step (the last step may convert up to three stale pixels nobody reads)
                for (int x = 4 * tid; x < a.crop_w; x += 4 * kThreads) {
                    uint32_t wy = 0, wu = 0, wv = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        int r, g, b;
                        if (a.format == EFX_PIX_RGB24) {
                            const uint8_t* p = s_raw + sh[0] + 3 * (x + q);
                            r = p[0], g = p[1], b = p[2];
                        } else {
                            r = s_raw[sh[0] + x + q], g = s_raw[sh[1] + x + q], b = s_raw[sh[2] + x + q];
                        }
                        const uint32_t yuv = ipx::ycbcr(m, r, g, b);
                        wy |= (yuv & 0xFF) << (8 * q);
                        wu |= ((yuv >> 8) & 0xFF) << (8 * q);
                        wv |= (yuv >> 16) << (8 * q);
                    }
                    *reinterpret_cast<uint32_t*>(&s_row[0][x]) = wy;
                    *reinterpret_cast<uint32_t*>(&s_row[1][x]) = wu;
                    *reinterpret_cast<uint32_t*>(&s_row[2][x]) = wv;
                }
                __syncthreads();
                if (s >= ls0 && s < ls1) {
                    int ky[kRows];
                    vcoefs<kRows>(tly, nl, s, ky);
#pragma unroll
                    for (int j = 0; j < 2; j++)
                        if (lv[j])
                            accumulate<kRows>(s_row[0], tlx[j], ky, accl[j]);
                }
                if (s >= cs0 && s < cs1) {
                    int ky[kCRows];
                    vcoefs<kCRows>(tcy, nc, s, ky);
#pragma unroll
                    for (int j = 0; j < 2; j++)
                        if (cv[j])
                            accumulate<kCRows>(s_row[1 + cplane[j]], tcx[j], ky, accc[j]);
                }
                // (the next row's fetch writes s_raw, which nobody reads any more; its conversion waits at the barrier)
            }
        } else {
            for (int s = ls0; s < ls1; s++) {
                const int sh = stage(img, ipx::i420_row(0, a.width, a.height, a.crop_x, a.crop_y, s), a.crop_w, s_row[0]);
                __syncthreads();
                int ky[kRows];
                vcoefs<kRows>(tly, nl, s, ky);
#pragma unroll
                for (int j = 0; j < 2; j++)
                    if (lv[j])
                        accumulate<kRows>(s_row[0] + sh, tlx[j], ky, accl[j]);
                __syncthreads();
            }
            for (int s = cs0; s < cs1; s++) {
                int sh[2];
#pragma unroll
                for (int c = 0; c < 2; c++)
                    sh[c] = stage(img, ipx::i420_row(1 + c, a.width, a.height, a.crop_x, a.crop_y, s), a.crop_w / 2, s_row[1 + c]);
                __syncthreads();
                int ky[kCRows];
                vcoefs<kCRows>(tcy, nc, s, ky);
#pragma unroll
                for (int j = 0; j < 2; j++)
                    if (cv[j])
                        accumulate<kCRows>(s_row[1 + cplane[j]] + sh[cplane[j]], tcx[j], ky, accc[j]);
                __syncthreads();
            }
        }
    }
    __syncthreads();  // the border is laid out

    // the lanes' columns into the band
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int col = tid + kThreads * j;
#pragma unroll
        for (int r = 0; r < kRows; r++)
            if (lv[j] && r < nl)
                s_out[(a.dst_y + l0 + r - y0) * kW + a.dst_x + col] = (uint8_t)ipx::vround(accl[j][r]);
#pragma unroll
        for (int r = 0; r < kCRows; r++)
            if (cv[j] && r < nc)
                s_out[kBandY + cplane[j] * kBandC + (a.dst_y / 2 + c0 + r - cy0) * (kW / 2) + a.dst_x / 2 + ccol[j]] =
                    (uint8_t)ipx::vround(accc[j][r]);
    }
    __syncthreads();

    // a band is contiguous in each plane: 176 + 44 + 44 pieces of 16 bytes
    for (int i = tid; i < kBandBytes / 16; i += kThreads) {
        uint8_t* o;
        if (i < kBandY / 16)
            o = out + y0 * kW + 16 * i;
        else if (i < (kBandY + kBandC) / 16)
            o = out + kYBytes + cy0 * (kW / 2) + 16 * (i - kBandY / 16);
        else
            o = out + kYBytes + kCBytes + cy0 * (kW / 2) + 16 * (i - (kBandY + kBandC) / 16);
        *reinterpret_cast<u32x4*>(o) = *reinterpret_cast<const u32x4*>(s_out + 16 * i);
    }
}

namespace {

// Four word samples per lane and step from a staged raw row (it begins `sh` bytes into raw) into a byte row (the last
// step may reduce up to three stale samples nobody reads)
__device__ inline void reduce_row(const uint8_t* raw, int sh, int n, int shift, uint8_t* row)
{
    for (int x = 4 * threadIdx.x; x < n; x += 4 * kThreads) {
        uint32_t w[2];
        spx::dwords_at<2>(raw, sh + 2 * x, w);
        *reinterpret_cast<uint32_t*>(row + x) = spx::reduce4(w[0], w[1], shift);
    }
}

// Four chroma pairs per lane and step from a staged pair row into the two byte rows: `first` takes elements 2x, `second`
// elements 2x + 1
template <bool WORDS>
__device__ inline void split_row(const uint8_t* raw, int sh, int n, int shift, uint8_t* first, uint8_t* second)
{
    for (int x = 4 * threadIdx.x; x < n; x += 4 * kThreads) {
        uint32_t a4, b4;
        if (WORDS) {
            uint32_t p[4];
            spx::dwords_at<4>(raw, sh + 4 * x, p);
            spx::split_pairs16(p, shift, &a4, &b4);
        } else {
            uint32_t p[2];
            spx::dwords_at<2>(raw, sh + 2 * x, p);
            spx::split_pairs8(p[0], p[1], &a4, &b4);
        }
        *reinterpret_cast<uint32_t*>(first + x) = a4;
        *reinterpret_cast<uint32_t*>(second + x) = b4;
    }
}

// k_import's band for a surface of layout SRC (EFX_SURF_*): a describes the canonical I420 image, sf where its samples lie.
// The band walk, the accumulators and the way out are k_import's, which stays as it is; only the row loaders differ.
template <int SRC, bool COLOUR, bool HDR = false>
__device__ inline void import_surface_band(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const ImportTap* __restrict__ taps,
                                           const ImportArgs& a, const efx_surface& sf, const colour::Coefs& k,
                                           const hdr::Tables* __restrict__ ht = nullptr)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[kRawBuf];
    __shared__ __attribute__((aligned(16))) uint8_t s_row[3][kRowBuf];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kBandBytes];
    // the HDR stage's own, in what the row loaders no longer need once the band walk is over: the band at 10 bits and the
    // second table in s_raw, the coefficients and the first table in s_row.  The tables are fetched into registers now and
    // put down behind the walk.
    constexpr int kTabA = (int)offsetof(hdr::Tables, gam), kTabB = (int)sizeof(hdr::Tables) - kTabA;  // bytes in s_row, in s_raw
    static_assert(kTabA % 16 == 0 && kTabB % 16 == 0 && sizeof(s_row) >= (size_t)kTabA && sizeof(s_raw) >= (size_t)(2 * kBandBytes + kTabB),
                  "the HDR stage's LDS is the row loaders'");
    uint16_t* const s_b10 = reinterpret_cast<uint16_t*>(s_raw);
    uint8_t* const s_tab_b = s_raw + 2 * kBandBytes;
    uint8_t* const s_tab_a = &s_row[0][0];
    constexpr int kTabPieces = (int)((sizeof(hdr::Tables) / 16 + kThreads - 1) / kThreads);

    const int tid = threadIdx.x;
    u32x4 tab[kTabPieces];
    if (HDR) {
#pragma unroll
        for (int i = 0; i < kTabPieces; i++)
            if (tid + kThreads * i < (int)(sizeof(hdr::Tables) / 16))
                tab[i] = reinterpret_cast<const u32x4*>(ht)[tid + kThreads * i];
    }
    const int band = (int)(blockIdx.x % kImportBands);
    const size_t image = blockIdx.x / kImportBands;
    const uint8_t* img = src + image * a.src_stride;
    uint8_t* out = dst + image * a.dst_stride;

    // the band on the border colour
    {
        const uint32_t black = 0x10101010u;
        for (int i = tid; i < kBandBytes / 4; i += kThreads)
            reinterpret_cast<uint32_t*>(s_out)[i] = i < kBandY / 4 ? black : 0x80808080u;
    }

    // the band's rows inside the destination rectangle, as indices into the rectangle: luma [l0, l0 + nl), chroma
    // [c0, c0 + nc) (every coordinate of the rectangle is even, so the two agree)
    const int y0 = band * kRows, cy0 = band * kCRows;
    const int l0 = max(y0, a.dst_y) - a.dst_y, nl = min(y0 + kRows, a.dst_y + a.dst_h) - a.dst_y - l0;
    const int c0 = max(cy0, a.dst_y / 2) - a.dst_y / 2, nc = min(cy0 + kCRows, (a.dst_y + a.dst_h) / 2) - a.dst_y / 2 - c0;
    const ImportTap* tly = taps + kImportTapLY + l0;
    const ImportTap* tcy = taps + kImportTapCY + c0;

    // this lane's columns: luma tid and tid + 256; chroma items tid and tid + 256 of [Cb columns | Cr columns]
    const int cw2 = a.dst_w / 2;
    bool lv[2], cv[2];
    int cplane[2], ccol[2];
    const ImportTap* tlx[2];
    const ImportTap* tcx[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int col = tid + kThreads * j;
        lv[j] = col < a.dst_w;
        tlx[j] = taps + kImportTapLX + (lv[j] ? col : 0);
        cv[j] = col < a.dst_w;
        cplane[j] = col >= cw2 ? 1 : 0;
        ccol[j] = cv[j] ? col - cplane[j] * cw2 : 0;
        tcx[j] = taps + kImportTapCX + ccol[j];
    }
    int accl[2][kRows] = {}, accc[2][kCRows] = {};

    if (nl > 0) {  // (nl > 0 exactly when nc > 0)
        const int ls0 = tly[0].start, ls1 = tly[nl - 1].start + tly[nl - 1].count;  // source rows of the supports
        const int cs0 = tcy[0].start, cs1 = tcy[nc - 1].start + tcy[nc - 1].count;
        constexpr bool words = SRC == EFX_SURF_PLANAR16 || SRC == EFX_SURF_SEMI16;
        constexpr bool semi = SRC == EFX_SURF_SEMI8 || SRC == EFX_SURF_SEMI16;
        constexpr int B = words ? 2 : 1;
        for (int s = ls0; s < ls1; s++) {
            // byte samples go straight to the byte row; word samples pass through s_raw and are reduced
            const int sh = stage(img, spx::crop_row(sf, 0, a.crop_x, a.crop_y, s), B * a.crop_w, words ? s_raw : s_row[0]);
            __syncthreads();
            if (words) {
                reduce_row(s_raw, sh, a.crop_w, sf.shift, s_row[0]);
                __syncthreads();
            }
            int ky[kRows];
            vcoefs<kRows>(tly, nl, s, ky);
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (lv[j])
                    accumulate<kRows>(s_row[0] + (words ? 0 : sh), tlx[j], ky, accl[j]);
            if (!words)
                __syncthreads();  // (a word row's next fetch writes s_raw, which nobody reads any more)
        }
        const int cw = a.crop_w / 2;
        for (int s = cs0; s < cs1; s++) {
            int sh[2] = {0, 0};
            if (semi) {
                // the pair row once, for both planes
                const int shp = stage(img, spx::crop_row(sf, 1, a.crop_x, a.crop_y, s), B * a.crop_w, s_raw);
                __syncthreads();
                split_row<words>(s_raw, shp, cw, sf.shift, s_row[1 + sf.swap_uv], s_row[2 - sf.swap_uv]);
            } else {
#pragma unroll
                for (int c = 0; c < 2; c++)
                    sh[c] = stage(img, spx::crop_row(sf, 1 + c, a.crop_x, a.crop_y, s), B * cw,
                                  words ? s_raw + c * kRawHalf : s_row[1 + c]);
                if (words) {
                    __syncthreads();
#pragma unroll
                    for (int c = 0; c < 2; c++)
                        reduce_row(s_raw + c * kRawHalf, sh[c], cw, sf.shift, s_row[1 + c]);
                    sh[0] = sh[1] = 0;
                }
            }
            __syncthreads();
            int ky[kCRows];
            vcoefs<kCRows>(tcy, nc, s, ky);
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (cv[j])
                    accumulate<kCRows>(s_row[1 + cplane[j]] + sh[cplane[j]], tcx[j], ky, accc[j]);
            if (!words && !semi)
                __syncthreads();
        }
    }
    __syncthreads();  // the border is laid out

    // the lanes' columns into the band
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int col = tid + kThreads * j;
        if (HDR) {
            // ... at 10 bits into the band the HDR stage reads
#pragma unroll
            for (int r = 0; r < kRows; r++)
                if (lv[j] && r < nl)
                    s_b10[(a.dst_y + l0 + r - y0) * kW + a.dst_x + col] = (uint16_t)hdr::vround10(accl[j][r]);
#pragma unroll
            for (int r = 0; r < kCRows; r++)
                if (cv[j] && r < nc)
                    s_b10[kBandY + cplane[j] * kBandC + (a.dst_y / 2 + c0 + r - cy0) * (kW / 2) + a.dst_x / 2 + ccol[j]] =
                        (uint16_t)hdr::vround10(accc[j][r]);
            continue;
        }
#pragma unroll
        for (int r = 0; r < kRows; r++)
            if (lv[j] && r < nl)
                s_out[(a.dst_y + l0 + r - y0) * kW + a.dst_x + col] = (uint8_t)ipx::vround(accl[j][r]);
#pragma unroll
        for (int r = 0; r < kCRows; r++)
            if (cv[j] && r < nc)
                s_out[kBandY + cplane[j] * kBandC + (a.dst_y / 2 + c0 + r - cy0) * (kW / 2) + a.dst_x / 2 + ccol[j]] =
                    (uint8_t)ipx::vround(accc[j][r]);
    }
    if (HDR) {
#pragma unroll
        for (int i = 0; i < kTabPieces; i++)
            if (tid + kThreads * i < (int)(sizeof(hdr::Tables) / 16))
                *reinterpret_cast<u32x4*>(tid + kThreads * i < kTabA / 16 ? s_tab_a + 16 * (tid + kThreads * i)
                                                                          : s_tab_b + 16 * (tid + kThreads * i) - kTabA) = tab[i];
    }
    __syncthreads();
    if (COLOUR)
        convert_band(a, k, y0, s_out);
    if (HDR)
        tonemap_band(a, reinterpret_cast<const hdr::Tables*>(s_tab_a), reinterpret_cast<const uint16_t*>(s_tab_b), y0, s_b10, s_out);

    // a band is contiguous in each plane: 176 + 44 + 44 pieces of 16 bytes
    for (int i = tid; i < kBandBytes / 16; i += kThreads) {
        uint8_t* o;
        if (i < kBandY / 16)
            o = out + y0 * kW + 16 * i;
        else if (i < (kBandY + kBandC) / 16)
            o = out + kYBytes + cy0 * (kW / 2) + 16 * (i - kBandY / 16);
        else
            o = out + kYBytes + kCBytes + cy0 * (kW / 2) + 16 * (i - (kBandY + kBandC) / 16);
        *reinterpret_cast<u32x4*>(o) = *reinterpret_cast<const u32x4*>(s_out + 16 * i);
    }
}

}  // namespace

// (a kernel per surface layout, like k_cropdetect's kernel per format: each is compiled to its own register count)
__global__ __launch_bounds__(256) void k_import_surf8p(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const ImportTap* __restrict__ taps, ImportSurfArgs a)
{
    import_surface_band<EFX_SURF_PLANAR8, false>(src, dst, taps, a.a, a.s, colour::Coefs{});
}

__global__ __launch_bounds__(256) void k_import_surf8s(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const ImportTap* __restrict__ taps, ImportSurfArgs a)
{
    import_surface_band<EFX_SURF_SEMI8, false>(src, dst, taps, a.a, a.s, colour::Coefs{});
}

__global__ __launch_bounds__(256) void k_import_surf16p(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        const ImportTap* __restrict__ taps, ImportSurfArgs a)
{
    import_surface_band<EFX_SURF_PLANAR16, false>(src, dst, taps, a.a, a.s, colour::Coefs{});
}

__global__ __launch_bounds__(256) void k_import_surf16s(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        const ImportTap* __restrict__ taps, ImportSurfArgs a)
{
    import_surface_band<EFX_SURF_SEMI16, false>(src, dst, taps, a.a, a.s, colour::Coefs{});
}

// ... and with the colour stage
__global__ __launch_bounds__(256) void k_import_surf8p_c(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const ImportTap* __restrict__ taps, ImportSurfArgs a, colour::Coefs k)
{
    import_surface_band<EFX_SURF_PLANAR8, true>(src, dst, taps, a.a, a.s, k);
}

__global__ __launch_bounds__(256) void k_import_surf8s_c(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const ImportTap* __restrict__ taps, ImportSurfArgs a, colour::Coefs k)
{
    import_surface_band<EFX_SURF_SEMI8, true>(src, dst, taps, a.a, a.s, k);
}

__global__ __launch_bounds__(256) void k_import_surf16p_c(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const ImportTap* __restrict__ taps, ImportSurfArgs a, colour::Coefs k)
{
    import_surface_band<EFX_SURF_PLANAR16, true>(src, dst, taps, a.a, a.s, k);
}

__global__ __launch_bounds__(256) void k_import_surf16s_c(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const ImportTap* __restrict__ taps, ImportSurfArgs a, colour::Coefs k)
{
    import_surface_band<EFX_SURF_SEMI16, true>(src, dst, taps, a.a, a.s, k);
}

// ... and with the HDR stage
__global__ __launch_bounds__(256) void k_import_surf8p_h(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const ImportTap* __restrict__ taps, ImportSurfArgs a,
                                                         const hdr::Tables* __restrict__ ht)
{
    import_surface_band<EFX_SURF_PLANAR8, false, true>(src, dst, taps, a.a, a.s, colour::Coefs{}, ht);
}

__global__ __launch_bounds__(256) void k_import_surf8s_h(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const ImportTap* __restrict__ taps, ImportSurfArgs a,
                                                         const hdr::Tables* __restrict__ ht)
{
    import_surface_band<EFX_SURF_SEMI8, false, true>(src, dst, taps, a.a, a.s, colour::Coefs{}, ht);
}

__global__ __launch_bounds__(256) void k_import_surf16p_h(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const ImportTap* __restrict__ taps, ImportSurfArgs a,
                                                          const hdr::Tables* __restrict__ ht)
{
    import_surface_band<EFX_SURF_PLANAR16, false, true>(src, dst, taps, a.a, a.s, colour::Coefs{}, ht);
}

__global__ __launch_bounds__(256) void k_import_surf16s_h(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const ImportTap* __restrict__ taps, ImportSurfArgs a,
                                                          const hdr::Tables* __restrict__ ht)
{
    import_surface_band<EFX_SURF_SEMI16, false, true>(src, dst, taps, a.a, a.s, colour::Coefs{}, ht);
}

}  // namespace efx
