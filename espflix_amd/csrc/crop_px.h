// crop_px.h -- arithmetic of k_cropdetect (k_cropdetect.hip): the luma byte of a source pixel, the picture / black test of
// a row or column sum, the rounding of a detected axis, the record of a stream, and where the sums kernel finds and keeps
// the rows of its band.
//
// Host + device: the kernels run exactly these functions, tests/test_crop_model.py builds this header with a plain C++
// compiler and checks it against the NumPy model (tests/crop_model.py), and tests/crop_model_main.cpp performs a whole
// detection with them on the host.  Everything is an integer function of the source bytes, so the detection is
// bit-exact by construction (the definition: include/efx.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "efx.h"
#include "import_px.h"

namespace efx {
namespace cpx {

constexpr int kBandRows = 64;      // rows of an image one workgroup sums: a column costs one 4-byte atomic add per band
constexpr int kWaves = 4;          // a wave owns whole rows: row r of a group goes to wave r % kWaves
constexpr int kLaneCols = 4;       // a lane owns 4 adjacent columns of every 256: columns 256 j + 4 lane + 0 .. 3
constexpr int kColGroups = 16;     // j = 0 .. 15 (4096 columns)
constexpr int kMaxGroupRows = 8;   // rows staged per barrier pair, at most
constexpr int kStageBytes = 24672; // the staged rows: two RGB rows of 4096 pixels; at least 4096 column sums (16384 bytes)

// The luma byte of an RGB pixel: Y of ipx::ycbcr (its low byte), which is what efx_import_frames would write
EFX_IPX_HD inline int luma(const ipx::Matrix& m, int r, int g, int b)
{
    return ipx::clamp_u8(((m.yr * r + m.yg * g + m.yb * b + 128) >> 8) + m.y0);
}

// A row (n = width) or column (n = height) is picture when its sum exceeds limit x n; equality is black.  No division.
EFX_IPX_HD inline bool is_picture(uint32_t sum, int limit, int n) { return sum > (uint32_t)limit * (uint32_t)n; }

// One axis: bounds a .. b inclusive (0 <= a <= b) to an even position and an even length that is a multiple of r where
// the axis has room for one, inside the bounds and centred to within one even step.  false: fewer than 2 usable lines.
EFX_IPX_HD inline bool round_axis(int a, int b, int r, int* pos, int* len)
{
    const int a1 = a + (a & 1);
    const int avail = b + 1 - a1;
    if (avail < 2)
        return false;
    const int l = avail >= r ? avail - avail % r : (avail & ~1);
    *pos = a1 + (((avail - l) >> 1) & ~1);
    *len = l;
    return true;
}

// The record of a stream from the union of its contributing images (x1 = W, y1 = H, x2 = y2 = -1: none contributed)
EFX_IPX_HD inline void record(int width, int height, int round, int x1, int y1, int x2, int y2, int32_t out[8])
{
    int x = 0, y = 0, w = width, h = height;
    int px, pw, py, ph;
    if (x2 >= x1 && y2 >= y1 && round_axis(x1, x2, round, &px, &pw) && round_axis(y1, y2, round, &py, &ph))
        x = px, y = py, w = pw, h = ph;
    out[0] = x, out[1] = y, out[2] = w, out[3] = h;
    out[4] = x1, out[5] = y1, out[6] = x2, out[7] = y2;
}

// How the sums kernel stages rows.  A row of the image is 1 segment (I420: its Y row; RGB24: its 3 W bytes) or 3 (RGBP:
// the row of each plane).  A segment is fetched as 16-byte pieces aligned down inside the image (ipx::span) into a slot
// of seg_cap bytes: the pieces (<= len + 30 bytes) and 16 more, since columns are read as aligned 4-byte words, two per
// access, up to 12 bytes past a segment's last byte.  group_rows rows are staged at once.
struct Layout {
    int nseg, seg_len, seg_cap, group_rows;
};

EFX_IPX_HD inline Layout layout(int format, int width)
{
    Layout l;
    l.nseg = format == EFX_PIX_RGBP ? 3 : 1;
    l.seg_len = format == EFX_PIX_RGB24 ? 3 * width : width;
    l.seg_cap = ((l.seg_len + 30) >> 4) * 16 + 16;
    int g = kStageBytes / (l.nseg * l.seg_cap);
    if (g > kMaxGroupRows)
        g = kMaxGroupRows;
    if (g > kWaves)
        g -= g % kWaves;  // (whole turns of the waves)
    l.group_rows = g;
    return l;
}

// Byte offset of segment s of row y in the image
EFX_IPX_HD inline size_t seg_offset(int format, int s, int width, int height, int y)
{
    if (format == EFX_PIX_RGB24)
        return ipx::rgb24_row(width, 0, 0, y);
    if (format == EFX_PIX_RGBP)
        return ipx::rgbp_row(s, width, height, 0, 0, y);
    return ipx::i420_row(0, width, height, 0, 0, y);
}

// Bytes [off, off + 4) of a word array (4-byte aligned; off >= 0), little endian
EFX_IPX_HD inline uint32_t word_at(const uint32_t* words, int off)
{
    const uint32_t lo = words[off >> 2], hi = words[(off >> 2) + 1];
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (off & 3)));
}

// The luma bytes of columns x .. x + 3 of a staged row, column x in the low byte.  seg: the row's first slot, shift[s]:
// where segment s begins in its slot.  Columns at or beyond the width come out as 0.
template <int FORMAT>
EFX_IPX_HD inline uint32_t luma4(const ipx::Matrix& m, const uint32_t* seg, int seg_cap, const int shift[3], int x, int width)
{
    uint32_t y4;
    if (FORMAT == EFX_PIX_I420) {
        y4 = word_at(seg, shift[0] + x);
    } else {
        uint32_t r4, g4, b4;
        if (FORMAT == EFX_PIX_RGB24) {
            const uint32_t w0 = word_at(seg, shift[0] + 3 * x), w1 = word_at(seg, shift[0] + 3 * x + 4),
                           w2 = word_at(seg, shift[0] + 3 * x + 8);
            // R G B R | G B R G | B R G B
            r4 = (w0 & 0xFF) | ((w0 >> 24) << 8) | (((w1 >> 16) & 0xFF) << 16) | (((w2 >> 8) & 0xFF) << 24);
            g4 = ((w0 >> 8) & 0xFF) | ((w1 & 0xFF) << 8) | ((w1 >> 24) << 16) | (((w2 >> 16) & 0xFF) << 24);
            b4 = ((w0 >> 16) & 0xFF) | (((w1 >> 8) & 0xFF) << 8) | ((w2 & 0xFF) << 16) | ((w2 >> 24) << 24);
        } else {
            r4 = word_at(seg, shift[0] + x);
            g4 = word_at(seg + (seg_cap >> 2), shift[1] + x);
            b4 = word_at(seg + 2 * (seg_cap >> 2), shift[2] + x);
        }
        y4 = 0;
        for (int q = 0; q < 4; q++)
            y4 |= (uint32_t)luma(m, (r4 >> (8 * q)) & 0xFF, (g4 >> (8 * q)) & 0xFF, (b4 >> (8 * q)) & 0xFF) << (8 * q);
    }
    const int n = width - x;
    return n >= 4 ? y4 : (y4 & ((1u << (8 * n)) - 1u));  // (1 <= n: the caller's lanes stay inside the row)
}

// Column sums of a lane, two columns to a register (a wave adds at most kBandRows x 255 = 16320 to a column): even holds
// columns +0 (low half) and +2, odd columns +1 and +3.  Returns the sum of the four bytes for the row sum.
EFX_IPX_HD inline uint32_t add4(uint32_t y4, uint32_t* even, uint32_t* odd)
{
    const uint32_t e = y4 & 0x00FF00FFu, o = (y4 >> 8) & 0x00FF00FFu;
    *even += e;
    *odd += o;
    const uint32_t t = e + o;
    return (t & 0xFFFF) + (t >> 16);
}

}  // namespace cpx
}  // namespace efx
