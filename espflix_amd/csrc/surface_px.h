// surface_px.h -- arithmetic of the surface loaders of k_import (k_import.hip) and k_cropdetect (k_cropdetect.hip): the
// reduction of a 16-bit sample to a byte, where a plane's row lies, the checks of an efx_surface, the conventional layout
// of a decoder's surface, and how the sums kernel stages a luma row.
//
// Host + device: the kernels run exactly these functions, tests/test_surface_model.py builds this header with a plain C++
// compiler and checks it against the NumPy model (tests/surface_model.py), and tests/surface_model_main.cpp performs whole
// imports and detections with them on the host.  Everything is an integer function of the source bytes (the definition:
// include/efx.h, "surfaces").
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "efx.h"
#include "crop_px.h"
#include "import_px.h"

namespace efx {
namespace spx {

constexpr int kMaxSize = 4096;                     // width and height (kImportMaxWidth)
constexpr size_t kMaxPitch = (size_t)1 << 20;      // bytes between rows
constexpr size_t kMaxBytes = (size_t)1 << 40;      // extent of an image, exclusive

EFX_IPX_HD inline bool is_words(int layout) { return layout == EFX_SURF_PLANAR16 || layout == EFX_SURF_SEMI16; }
EFX_IPX_HD inline bool is_semi(int layout) { return layout == EFX_SURF_SEMI8 || layout == EFX_SURF_SEMI16; }

// One sample: min(255, (w + half a step) >> shift), shift 1 .. 8
EFX_IPX_HD inline uint32_t reduce(uint32_t w, int shift)
{
    const uint32_t v = (w + (1u << (shift - 1))) >> shift;
    return v > 255u ? 255u : v;
}

// Two samples in the halves of a dword, the results in the low byte of each half: an add that saturates at 65535 (which
// still reduces to 255 for every shift up to 8, where a wrapping add would give 0), a shift and a minimum, all packed.
EFX_IPX_HD inline uint32_t reduce2(uint32_t w2, int shift)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
    const uint16_t half = (uint16_t)(1u << (shift - 1)), sh = (uint16_t)shift;
    u16x2 v = __builtin_elementwise_add_sat(__builtin_bit_cast(u16x2, w2), u16x2{half, half});  // v_pk_add_u16 clamp
    v = v >> u16x2{sh, sh};                                                                   // v_pk_lshrrev_b16
    v = __builtin_elementwise_min(v, u16x2{255, 255});                                        // v_pk_min_u16
    return __builtin_bit_cast(uint32_t, v);
#else
    return reduce(w2 & 0xFFFF, shift) | (reduce(w2 >> 16, shift) << 16);
#endif
}

// Bytes of two dwords picked by a selector, v_perm_b32's: result byte i is byte sel_i of the eight bytes hi : lo (0 .. 3
// lie in lo, 4 .. 7 in hi)
EFX_IPX_HD inline uint32_t pick(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++)
        r |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7))) & 0xFF) << (8 * i);
    return r;
#endif
}

constexpr uint32_t kPickEven = 0x06040200u;  // bytes 0, 2 of lo, then of hi: the low bytes of four 16-bit halves
constexpr uint32_t kPickOdd = 0x07050301u;   // bytes 1, 3
constexpr uint32_t kPickPairs = 0x06020400u; // lo.0, hi.0, lo.2, hi.2: (a0, a1, b0, b1) of two reduced (a, b) pairs
constexpr uint32_t kPickLow = 0x05040100u;   // the low halves of lo and hi
constexpr uint32_t kPickHigh = 0x07060302u;  // the high halves

// Four word samples (w01 = samples 0, 1; w23 = samples 2, 3) as four bytes, sample 0 in the low byte
EFX_IPX_HD inline uint32_t reduce4(uint32_t w01, uint32_t w23, int shift)
{
    return pick(reduce2(w23, shift), reduce2(w01, shift), kPickEven);
}

// Four (a, b) byte pairs (eight bytes, p01 first) as a0 a1 a2 a3 and b0 b1 b2 b3
EFX_IPX_HD inline void split_pairs8(uint32_t p01, uint32_t p23, uint32_t* a4, uint32_t* b4)
{
    *a4 = pick(p23, p01, kPickEven);
    *b4 = pick(p23, p01, kPickOdd);
}

// Four (a, b) word pairs (one dword each) reduced, as a0 a1 a2 a3 and b0 b1 b2 b3
EFX_IPX_HD inline void split_pairs16(const uint32_t p[4], int shift, uint32_t* a4, uint32_t* b4)
{
    const uint32_t t01 = pick(reduce2(p[1], shift), reduce2(p[0], shift), kPickPairs);
    const uint32_t t23 = pick(reduce2(p[3], shift), reduce2(p[2], shift), kPickPairs);
    *a4 = pick(t23, t01, kPickLow);
    *b4 = pick(t23, t01, kPickHigh);
}

// Bytes [off, off + 4 N) of a staged row (buf: 4-byte aligned; off >= 0) as N dwords, little endian: N + 1 aligned reads
template <int N>
EFX_IPX_HD inline void dwords_at(const uint8_t* buf, int off, uint32_t out[N])
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(buf) + (off >> 2);
    const int bits = 8 * (off & 3);
    uint32_t lo = w[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < N; i++) {
        const uint32_t hi = w[i + 1];
        out[i] = (uint32_t)((((uint64_t)hi << 32) | lo) >> bits);
        lo = hi;
    }
}

// Byte offset of row r of a plane (0 = Y, 1 = Cb or the pair plane, 2 = Cr) in the image, in 64 bits
EFX_IPX_HD inline size_t plane_row(const efx_surface& s, int plane, int r) { return s.offset[plane] + (size_t)r * s.pitch[plane]; }

// ... of the crop's row r: its first byte and its length.  Luma and a pair row bring crop_w samples, a planar chroma row
// crop_w / 2; B = bytes per sample.
EFX_IPX_HD inline size_t crop_row(const efx_surface& s, int plane, int crop_x, int crop_y, int r)
{
    const int B = is_words(s.layout) ? 2 : 1;
    if (plane == 0)
        return plane_row(s, 0, crop_y + r) + (size_t)crop_x * B;
    return plane_row(s, plane, crop_y / 2 + r) + (size_t)(is_semi(s.layout) ? crop_x : crop_x / 2) * B;
}

// The checks of efx_import_surfaces / efx_detect_crop_surfaces: 0 = a surface the kernels can read, else what is wrong
enum Fault { kOk = 0, kBadLayout, kBadShift, kBadSwap, kBadSize, kOddWords, kBadPitch, kBadBytes, kRowBeyondBytes };

EFX_IPX_HD inline int check(const efx_surface& s)
{
    if (s.layout < EFX_SURF_PLANAR8 || s.layout > EFX_SURF_SEMI16)
        return kBadLayout;
    const bool words = is_words(s.layout), semi = is_semi(s.layout);
    if (words ? (s.shift < 1 || s.shift > 8) : s.shift != 0)
        return kBadShift;
    if (semi ? (s.swap_uv != 0 && s.swap_uv != 1) : s.swap_uv != 0)
        return kBadSwap;
    if (s.width < 2 || s.width > kMaxSize || s.height < 2 || s.height > kMaxSize || ((s.width | s.height) & 1))
        return kBadSize;
    if (s.bytes >= kMaxBytes)
        return kBadBytes;
    const size_t B = words ? 2 : 1;
    const int planes = semi ? 2 : 3;
    for (int p = 0; p < planes; p++) {
        const size_t row = (p == 0 || semi ? (size_t)s.width : (size_t)s.width / 2) * B;
        const size_t rows = p == 0 ? (size_t)s.height : (size_t)s.height / 2;
        if (words && ((s.offset[p] | s.pitch[p]) & 1))
            return kOddWords;
        if (s.pitch[p] < row || s.pitch[p] > kMaxPitch)
            return kBadPitch;
        // (offset <= bytes < 2^40 and (rows - 1) x pitch < 2^32: the sum cannot wrap)
        if (s.offset[p] > s.bytes || s.offset[p] + (rows - 1) * s.pitch[p] + row > s.bytes)
            return kRowBeyondBytes;
    }
    return kOk;
}

// efx_surface_layout: the conventional layout of a kind (efx_surface_kind); returns bytes, 0 for arguments check() or
// the rule itself rejects
EFX_IPX_HD inline size_t layout(int kind, int width, int height, size_t pitch, int plane_rows, efx_surface* out)
{
    efx_surface s = {};
    switch (kind) {
    case EFX_KIND_I420: case EFX_KIND_YV12: s.layout = EFX_SURF_PLANAR8; break;
    case EFX_KIND_NV12: case EFX_KIND_NV21: s.layout = EFX_SURF_SEMI8; break;
    case EFX_KIND_P010: case EFX_KIND_P012: case EFX_KIND_P016: s.layout = EFX_SURF_SEMI16, s.shift = 8; break;
    case EFX_KIND_I010: s.layout = EFX_SURF_PLANAR16, s.shift = 2; break;
    case EFX_KIND_I012: s.layout = EFX_SURF_PLANAR16, s.shift = 4; break;
    case EFX_KIND_I016: s.layout = EFX_SURF_PLANAR16, s.shift = 8; break;
    default: return 0;
    }
    if (width < 2 || width > kMaxSize || height < 2 || height > kMaxSize || ((width | height) & 1))
        return 0;
    const size_t B = is_words(s.layout) ? 2 : 1;
    const size_t P = pitch ? pitch : (size_t)width * B;
    const int R = plane_rows ? plane_rows : height;
    if (P > kMaxPitch || R < height || (R & 1) || (!is_semi(s.layout) && P % (2 * B)))
        return 0;
    s.swap_uv = kind == EFX_KIND_NV21 ? 1 : 0;
    s.width = width, s.height = height;
    s.pitch[0] = P;
    s.offset[1] = P * (size_t)R;
    if (is_semi(s.layout)) {
        s.pitch[1] = P;
    } else {
        s.pitch[1] = s.pitch[2] = P / 2;
        s.offset[2] = s.offset[1] + (P / 2) * (size_t)(R / 2);
        if (kind == EFX_KIND_YV12) {
            const size_t t = s.offset[1];
            s.offset[1] = s.offset[2], s.offset[2] = t;
        }
    }
    s.bytes = P * (size_t)R * 3 / 2;
    if (check(s) != kOk)
        return 0;
    *out = s;
    return s.bytes;
}

// How the sums kernel stages the luma rows of a surface: one segment of width x B bytes per row (cpx::layout's rule)
EFX_IPX_HD inline cpx::Layout crop_layout(int width, int B)
{
    cpx::Layout l;
    l.nseg = 1;
    l.seg_len = width * B;
    l.seg_cap = ((l.seg_len + 30) >> 4) * 16 + 16;
    int g = cpx::kStageBytes / l.seg_cap;
    if (g > cpx::kMaxGroupRows)
        g = cpx::kMaxGroupRows;
    if (g > cpx::kWaves)
        g -= g % cpx::kWaves;
    l.group_rows = g;
    return l;
}

// The luma bytes of columns x .. x + 3 of a staged luma row that begins `shift0` bytes into seg, column x in the low
// byte; columns at or beyond the width come out as 0 (cpx::luma4's rule)
template <bool WORDS>
EFX_IPX_HD inline uint32_t luma4(const uint32_t* seg, int shift0, int x, int width, int shift)
{
    uint32_t y4;
    if (WORDS) {
        uint32_t w[2];
        dwords_at<2>(reinterpret_cast<const uint8_t*>(seg), shift0 + 2 * x, w);
        y4 = reduce4(w[0], w[1], shift);
    } else {
        y4 = cpx::word_at(seg, shift0 + x);
    }
    const int n = width - x;
    return n >= 4 ? y4 : (y4 & ((1u << (8 * n)) - 1u));
}

}  // namespace spx
}  // namespace efx
