// colour_px.h -- arithmetic of the import's colour conversion (k_import.hip): a YCbCr source of another matrix or range
// (BT.709, full range ...) to the BT.601 studio swing MPEG-1 carries.  The source matrix is named by its H.273
// matrix_coefficients code, the range is 0 = studio (Y 16 .. 235, C 16 .. 240) or 1 = full (Y 0 .. 255, C centred on 128
// over 255).  Code 9 (BT.2020 non-constant luminance) converts the matrix only: transfer and gamut mapping are hdr_px.h's.
//
// Host + device: the kernels run exactly these functions, tests/test_colour_model.py builds this header with a plain C++
// compiler and checks it against the NumPy model (tests/colour_model.py), and tests/colour_model_main.cpp converts whole
// pictures with them on the host.  Everything is an integer function of the imported bytes (the definition:
// include/efx.h, "source colour").
#pragma once
#include <stdint.h>

#include "import_px.h"

namespace efx {
namespace colour {

constexpr int kUnspecified = 2;     // resolves by the picture's height
constexpr int kAutoHdAbove = 576;   // ... to BT.709 above this many lines, to BT.601 otherwise

// What a kernel gets by value.  The matrix takes (Y - y0, Cb - 128, Cr - 128) to (Y' - 16, Cb' - 128, Cr' - 128) in steps
// of 2^-14; its first column is (q00, 0, 0): converted chroma never depends on luma.
struct Coefs {
    int32_t q00, q01, q02;
    int32_t q11, q12;
    int32_t q21, q22;
    int32_t y0;
};

// q = round(2^14 x exact value), the exact value formed in rational arithmetic (tests/colour_model.py recomputes every
// entry): R, G, B from the source's normalised (y, pb, pr) with its (Kr, Kb), the BT.601 (y', pb', pr') of that R, G, B,
// scaled by the 8-bit ranges 219 / 224 of the target over 219 / 224 or 255 / 255 of the source.
struct Entry {
    int code;         // H.273 matrix_coefficients
    int32_t q[2][9];  // [range][row major]
};
constexpr Entry kTable[] = {
    // BT.709: Kr 0.2126, Kb 0.0722
    {1, {{16384, 1627, 3141, 0, 16218, -1813, 0, -1187, 16112}, {14071, 1429, 2759, 0, 14246, -1593, 0, -1043, 14153}}},
    // FCC: Kr 0.30, Kb 0.11
    {4, {{16384, 130, 12, 0, 16383, -7, 0, -95, 16352}, {14071, 114, 10, 0, 14391, -6, 0, -83, 14364}}},
    // BT.601 (625 and 525 lines): Kr 0.299, Kb 0.114 -- studio range is the target itself
    {5, {{16384, 0, 0, 0, 16384, 0, 0, 0, 16384}, {14071, 0, 0, 0, 14392, 0, 0, 0, 14392}}},
    {6, {{16384, 0, 0, 0, 16384, 0, 0, 0, 16384}, {14071, 0, 0, 0, 14392, 0, 0, 0, 14392}}},
    // SMPTE 240M: Kr 0.212, Kb 0.087
    {7, {{16384, 1204, 3067, 0, 16189, -1770, 0, -878, 16180}, {14071, 1057, 2694, 0, 14221, -1555, 0, -771, 14213}}},
    // BT.2020 non-constant luminance: Kr 0.2627, Kb 0.0593
    {9, {{16384, 1888, 1690, 0, 16306, -976, 0, -1378, 15999}, {14071, 1659, 1485, 0, 14323, -857, 0, -1210, 14054}}},
};

// A setting as efx_import_set_colour takes it: a known code (2 included) and a range of 0 or 1.  (Host: the kernels get
// their coefficients by value.)
inline bool valid(int matrix, int full_range)
{
    if (full_range != 0 && full_range != 1)
        return false;
    if (matrix == kUnspecified)
        return true;
    for (const Entry& e : kTable)
        if (e.code == matrix)
            return true;
    return false;
}

// The coefficients of a setting for a picture of `height` lines: 0 = "off" (the source is BT.601 studio swing: q is the
// identity), 1 = a conversion, -1 = an invalid setting (q and y0 untouched)
inline int coefs(int matrix, int full_range, int height, int32_t q[9], int* y0)
{
    if (!valid(matrix, full_range))
        return -1;
    if (matrix == kUnspecified)
        matrix = height > kAutoHdAbove ? 1 : 6;
    for (const Entry& e : kTable) {
        if (e.code != matrix)
            continue;
        for (int i = 0; i < 9; i++)
            q[i] = e.q[full_range][i];
        *y0 = full_range ? 0 : 16;
        return ((matrix == 5 || matrix == 6) && !full_range) ? 0 : 1;
    }
    return -1;
}

EFX_IPX_HD inline Coefs pack(const int32_t q[9], int y0) { return Coefs{q[0], q[1], q[2], q[4], q[5], q[7], q[8], y0}; }

// One pixel (>> of a negative int is an arithmetic shift, as in import_px.h).  u = Cb - 128, v = Cr - 128.  Every product
// is below 2^15 x 2^8 and every sum below 2^25.
EFX_IPX_HD inline int luma_chroma_term(const Coefs& k, int u, int v) { return k.q01 * u + k.q02 * v + 8192; }
EFX_IPX_HD inline int luma(const Coefs& k, int y, int term) { return ipx::clamp_u8(16 + ((k.q00 * (y - k.y0) + term) >> 14)); }
EFX_IPX_HD inline int chroma_b(const Coefs& k, int u, int v) { return ipx::clamp_u8(128 + ((k.q11 * u + k.q12 * v + 8192) >> 14)); }
EFX_IPX_HD inline int chroma_r(const Coefs& k, int u, int v) { return ipx::clamp_u8(128 + ((k.q21 * u + k.q22 * v + 8192) >> 14)); }

// Y | Cb << 8 | Cr << 16 of one source triple
EFX_IPX_HD inline uint32_t pixel(const Coefs& k, int y, int cb, int cr)
{
    const int u = cb - 128, v = cr - 128;
    return (uint32_t)luma(k, y, luma_chroma_term(k, u, v)) | ((uint32_t)chroma_b(k, u, v) << 8) | ((uint32_t)chroma_r(k, u, v) << 16);
}

// One work item: a chroma site and the 2 x 2 luma samples around it, in place.  y points at the block's top left luma
// sample, its rows are y_pitch apart.  Luma is converted first, with the unconverted chroma (nearest siting); nobody else
// reads or writes these six samples, so items need no order among themselves.
EFX_IPX_HD inline void convert_block(const Coefs& k, uint8_t* y, int y_pitch, uint8_t* cb, uint8_t* cr)
{
    const int u = *cb - 128, v = *cr - 128;
    const int term = luma_chroma_term(k, u, v);
    y[0] = (uint8_t)luma(k, y[0], term);
    y[1] = (uint8_t)luma(k, y[1], term);
    y[y_pitch] = (uint8_t)luma(k, y[y_pitch], term);
    y[y_pitch + 1] = (uint8_t)luma(k, y[y_pitch + 1], term);
    *cb = (uint8_t)chroma_b(k, u, v);
    *cr = (uint8_t)chroma_r(k, u, v);
}

// The part of the destination rectangle (dst_x, dst_y, dst_w, dst_h: all even) inside the band of `band_rows` luma rows
// that begins at luma row y0, in chroma units: rows [row0, row0 + rows) of the band, columns [col0, col0 + cols) of the
// frame.  rows <= 0: the band lies outside the rectangle.
struct BandPart {
    int row0, rows, col0, cols;
};

EFX_IPX_HD inline BandPart band_part(int dst_x, int dst_y, int dst_w, int dst_h, int y0, int band_rows)
{
    const int top = (dst_y > y0 ? dst_y : y0) / 2;
    const int end = (dst_y + dst_h < y0 + band_rows ? dst_y + dst_h : y0 + band_rows) / 2;
    return BandPart{top - y0 / 2, end - top, dst_x / 2, dst_w / 2};
}

// Item (r, c) of a band's part: chroma row r < rows, chroma column c < cols.  band_y: the band's luma rows, `width` bytes
// each; band_cb, band_cr: its chroma rows, width / 2 bytes each.
EFX_IPX_HD inline void convert_item(const Coefs& k, const BandPart& p, int r, int c, int width, uint8_t* band_y, uint8_t* band_cb,
                                    uint8_t* band_cr)
{
    const int ci = (p.row0 + r) * (width / 2) + p.col0 + c;
    convert_block(k, band_y + 2 * (p.row0 + r) * width + 2 * (p.col0 + c), width, band_cb + ci, band_cr + ci);
}

}  // namespace colour
}  // namespace efx
