// TEST: a whole efx_import_frames on the host, with import_px.h's functions and k_import's own index arithmetic: the tap
// table of k_import_taps, the bands of 8 luma rows, the source rows of a band's vertical support, every row fetched as
// 16-byte pieces aligned down inside the image (ipx::span) into buffers of the kernel's sizes.  The source lives in a heap
// block of exactly its size rounded up to 16 and the output in one of exactly 101376 bytes, so a sanitizer build
// (-fsanitize=address,undefined: tests/test_import_model.py) sees every byte the kernel's addressing would touch.
//
//   import_model_main FORMAT WIDTH HEIGHT CROP_X CROP_Y CROP_W CROP_H DST_X DST_Y DST_W DST_H FULL_RANGE SRC_FILE DST_FILE
//   import_model_main taps S D                (start, count, coefficients of every destination index: int32 each, to stdout)
//   import_model_main matrix FULL_RANGE       (Y | Cb << 8 | Cr << 16 of every (R, G, B), R major, B minor: uint32, to stdout)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "efx.h"
#include "efx_internal.h"
#include "import_px.h"

using namespace efx;

namespace {

constexpr int kW = EFX_FRAME_WIDTH, kH = EFX_FRAME_HEIGHT, kYBytes = kW * kH, kCBytes = kYBytes / 4;
constexpr int kRows = kImportBandRows, kCRows = kRows / 2;
constexpr int kRowBuf = kImportMaxWidth + 32, kRawBuf = 3 * kRowBuf + 16;

// k_import's stage(): whole 16-byte pieces
int stage(const uint8_t* img, size_t off, int len, uint8_t* buf)
{
    const ipx::Span sp = ipx::span(off, len);
    for (int i = 0; i < sp.pieces; i++)
        memcpy(buf + 16 * i, img + sp.a0 + 16 * (size_t)i, 16);
    return sp.shift;
}

int vcoef(const ImportTap& t, int s)
{
    const unsigned i = (unsigned)(s - t.start);
    return i < (unsigned)t.count ? t.k[i] : 0;
}

int hsum(const uint8_t* row, const ImportTap& t)
{
    // four taps per step, as k_import's accumulate() reads them: zeros follow the window's coefficients
    int sum = 0;
    for (int i = 0; i < t.count; i += 4)
        for (int j = i; j < i + 4; j++)
            sum += (int)t.k[j] * (int)row[t.start + j];
    return ipx::hround(sum);
}

void import_image(const ImportArgs& a, const ImportTap* taps, const uint8_t* img, uint8_t* out)
{
    const bool rgb = a.format != EFX_PIX_I420;
    // (zeroed: the kernel's last conversion step and its four-tap steps read a few stale bytes, which weigh nothing)
    std::unique_ptr<uint8_t[]> raw(new uint8_t[kRawBuf]()), row0(new uint8_t[kRowBuf]()), row1(new uint8_t[kRowBuf]()),
        row2(new uint8_t[kRowBuf]());
    uint8_t* row[3] = {row0.get(), row1.get(), row2.get()};
    const ipx::Matrix m = ipx::matrix(a.full_range);
    for (int band = 0; band < kImportBands; band++) {
        const int y0 = band * kRows, cy0 = band * kCRows;
        memset(out + y0 * kW, (rgb && a.full_range) ? 0 : 16, kRows * kW);
        memset(out + kYBytes + cy0 * (kW / 2), 128, kCRows * (kW / 2));
        memset(out + kYBytes + kCBytes + cy0 * (kW / 2), 128, kCRows * (kW / 2));
        const int l0 = std::max(y0, a.dst_y) - a.dst_y, nl = std::min(y0 + kRows, a.dst_y + a.dst_h) - a.dst_y - l0;
        const int c0 = std::max(cy0, a.dst_y / 2) - a.dst_y / 2, nc = std::min(cy0 + kCRows, (a.dst_y + a.dst_h) / 2) - a.dst_y / 2 - c0;
        if (nl <= 0)
            continue;
        const ImportTap* tly = taps + kImportTapLY + l0;
        const ImportTap* tcy = taps + kImportTapCY + c0;
        const int ls0 = tly[0].start, ls1 = tly[nl - 1].start + tly[nl - 1].count;
        const int cs0 = tcy[0].start, cs1 = tcy[nc - 1].start + tcy[nc - 1].count;
        std::vector<int> accl((size_t)kRows * a.dst_w, 0), accc((size_t)kCRows * a.dst_w, 0);
        auto luma = [&](const uint8_t* r, int s) {
            for (int x = 0; x < a.dst_w; x++) {
                const int h = hsum(r, taps[kImportTapLX + x]);
                for (int k = 0; k < nl; k++)
                    accl[(size_t)k * a.dst_w + x] += vcoef(tly[k], s) * h;
            }
        };
        auto chroma = [&](const uint8_t* ru, const uint8_t* rv, int s) {
            for (int x = 0; x < a.dst_w; x++) {
                const int plane = x >= a.dst_w / 2, col = x - plane * (a.dst_w / 2);
                const int h = hsum(plane ? rv : ru, taps[kImportTapCX + col]);
                for (int k = 0; k < nc; k++)
                    accc[(size_t)k * a.dst_w + x] += vcoef(tcy[k], s) * h;
            }
        };
        if (rgb) {
            for (int s = std::min(ls0, cs0); s < std::max(ls1, cs1); s++) {
                int sh[3] = {0, 0, 0};
                if (a.format == EFX_PIX_RGB24)
                    sh[0] = stage(img, ipx::rgb24_row(a.width, a.crop_x, a.crop_y, s), 3 * a.crop_w, raw.get());
                else
                    for (int c = 0; c < 3; c++)
                        sh[c] = stage(img, ipx::rgbp_row(c, a.width, a.height, a.crop_x, a.crop_y, s), a.crop_w, raw.get() + c * kRowBuf) +
                                c * kRowBuf;
                for (int x = 0; x < (a.crop_w + 3) / 4 * 4; x++) {
                    int r, g, b;
                    if (a.format == EFX_PIX_RGB24) {
                        const uint8_t* p = raw.get() + sh[0] + 3 * x;
                        r = p[0], g = p[1], b = p[2];
                    } else {
                        r = raw[sh[0] + x], g = raw[sh[1] + x], b = raw[sh[2] + x];
                    }
                    const uint32_t yuv = ipx::ycbcr(m, r, g, b);
                    row[0][x] = (uint8_t)yuv, row[1][x] = (uint8_t)(yuv >> 8), row[2][x] = (uint8_t)(yuv >> 16);
                }
                if (s >= ls0 && s < ls1)
                    luma(row[0], s);
                if (s >= cs0 && s < cs1)
                    chroma(row[1], row[2], s);
            }
        } else {
            for (int s = ls0; s < ls1; s++)
                luma(row[0] + stage(img, ipx::i420_row(0, a.width, a.height, a.crop_x, a.crop_y, s), a.crop_w, row[0]), s);
            for (int s = cs0; s < cs1; s++) {
                const int su = stage(img, ipx::i420_row(1, a.width, a.height, a.crop_x, a.crop_y, s), a.crop_w / 2, row[1]);
                const int sv = stage(img, ipx::i420_row(2, a.width, a.height, a.crop_x, a.crop_y, s), a.crop_w / 2, row[2]);
                chroma(row[1] + su, row[2] + sv, s);
            }
        }
        for (int k = 0; k < nl; k++)
            for (int x = 0; x < a.dst_w; x++)
                out[(a.dst_y + l0 + k) * kW + a.dst_x + x] = (uint8_t)ipx::vround(accl[(size_t)k * a.dst_w + x]);
        for (int k = 0; k < nc; k++)
            for (int x = 0; x < a.dst_w; x++) {
                const int plane = x >= a.dst_w / 2, col = x - plane * (a.dst_w / 2);
                out[kYBytes + plane * kCBytes + (a.dst_y / 2 + c0 + k) * (kW / 2) + a.dst_x / 2 + col] =
                    (uint8_t)ipx::vround(accc[(size_t)k * a.dst_w + x]);
            }
    }
}

// k_import_taps, lane by lane
void fill_taps(const ImportArgs& a, ImportTap* table)
{
    const int half = a.format == EFX_PIX_I420 ? 2 : 1;
    for (int i = 0; i < kImportTapRows; i++) {
        int d, S, D;
        if (i < kImportTapLY)
            d = i - kImportTapLX, S = a.crop_w, D = a.dst_w;
        else if (i < kImportTapCX)
            d = i - kImportTapLY, S = a.crop_h, D = a.dst_h;
        else if (i < kImportTapCY)
            d = i - kImportTapCX, S = a.crop_w / half, D = a.dst_w / 2;
        else
            d = i - kImportTapCY, S = a.crop_h / half, D = a.dst_h / 2;
        if (d >= D)
            continue;
        int n;
        table[i].start = ipx::taps(S, D, d, &n, table[i].k);
        table[i].count = n;
        for (int j = n; j < kImportTapSlots; j++)
            table[i].k[j] = 0;
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "taps")) {
        const int S = atoi(argv[2]), D = atoi(argv[3]);
        std::vector<int32_t> rec(2 + ipx::kMaxTaps);
        for (int d = 0; d < D; d++) {
            std::unique_ptr<uint16_t[]> k(new uint16_t[ipx::kMaxTaps]);
            std::fill(rec.begin(), rec.end(), 0);
            int n;
            rec[0] = ipx::taps(S, D, d, &n, k.get());
            rec[1] = n;
            for (int i = 0; i < n; i++)
                rec[2 + i] = k[i];
            fwrite(rec.data(), 4, rec.size(), stdout);
        }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "matrix")) {
        const ipx::Matrix m = ipx::matrix(atoi(argv[2]));
        std::vector<uint32_t> out(1 << 16);
        for (int r = 0; r < 256; r++) {
            for (int g = 0; g < 256; g++)
                for (int b = 0; b < 256; b++)
                    out[g * 256 + b] = ipx::ycbcr(m, r, g, b);
            fwrite(out.data(), 4, out.size(), stdout);
        }
        return 0;
    }
    if (argc != 15) {
        fprintf(stderr, "usage: see the head of tests/import_model_main.cpp\n");
        return 2;
    }
    ImportArgs a{};
    int* f[] = {&a.format, &a.width, &a.height, &a.crop_x, &a.crop_y, &a.crop_w, &a.crop_h, &a.dst_x, &a.dst_y, &a.dst_w, &a.dst_h,
                &a.full_range};
    for (int i = 0; i < 12; i++)
        *f[i] = atoi(argv[1 + i]);
    const size_t bytes = (size_t)a.width * a.height * (a.format == EFX_PIX_I420 ? 3 : 6) / 2, padded = (bytes + 15) / 16 * 16;
    // operator new[] hands out 16-byte aligned blocks, like the device pointers of the contract
    std::unique_ptr<uint8_t[]> src(new uint8_t[padded]), dst(new uint8_t[kFrameBytes]);
    std::unique_ptr<ImportTap[]> table(new ImportTap[kImportTapRows]);
    memset(src.get(), 0, padded);
    FILE* in = fopen(argv[13], "rb");
    if (!in || fread(src.get(), 1, bytes, in) != bytes) {
        fprintf(stderr, "cannot read %zu bytes from %s\n", bytes, argv[13]);
        return 1;
    }
    fclose(in);
    fill_taps(a, table.get());
    import_image(a, table.get(), src.get(), dst.get());
    FILE* o = fopen(argv[14], "wb");
    if (!o || fwrite(dst.get(), 1, kFrameBytes, o) != (size_t)kFrameBytes) {
        fprintf(stderr, "cannot write %s\n", argv[14]);
        return 1;
    }
    fclose(o);
    return 0;
}
