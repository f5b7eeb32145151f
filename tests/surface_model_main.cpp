// TEST: efx_import_surfaces and efx_detect_crop_surfaces on the host, with surface_px.h's functions and the kernels' own
// index arithmetic: the tap table of k_import_taps, the bands and their vertical supports, every row fetched as 16-byte
// pieces aligned down inside the image (ipx::span) into buffers of the kernels' sizes, pair rows de-interleaved and word
// rows reduced four samples at a time as the kernels do it.  The source lives in a heap block of exactly src_stride x
// (n - 1) + bytes rounded up to 16 and every output in a block of exactly its size, so a sanitizer build
// (-fsanitize=address,undefined: tests/test_surface_model.py) sees every byte the kernels' addressing would touch.
//
//   surface_model_main reduce SHIFT           (reduce() of every word, then reduce4() of every word: 2 x 65536 bytes, to stdout)
//   surface_model_main layout KIND WIDTH HEIGHT PITCH PLANE_ROWS     (bytes, then the surface's twelve fields, as text)
//   surface_model_main check SURFACE          (spx::check's verdict as text)
//   surface_model_main import SURFACE N SRC_STRIDE CROP_X CROP_Y CROP_W CROP_H DST_X DST_Y DST_W DST_H SRC_FILE DST_FILE
//   surface_model_main crop SURFACE N_STREAMS PER_STREAM SRC_STRIDE LIMIT ROUND SRC_FILE OUT_FILE
//                                             (OUT_FILE: per image height + width uint32 sums, then per stream 8 int32)
//   SURFACE = LAYOUT SHIFT SWAP_UV WIDTH HEIGHT OFFSET0 OFFSET1 OFFSET2 PITCH0 PITCH1 PITCH2 BYTES
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "efx.h"
#include "efx_internal.h"
#include "surface_px.h"

using namespace efx;

namespace {

constexpr int kW = EFX_FRAME_WIDTH, kH = EFX_FRAME_HEIGHT, kYBytes = kW * kH, kCBytes = kYBytes / 4;
constexpr int kRows = kImportBandRows, kCRows = kRows / 2;
constexpr int kRowBuf = kImportMaxWidth + 32, kRawBuf = 3 * kRowBuf + 16, kRawHalf = (kRawBuf / 2) & ~15;

efx_surface parse_surface(char** v)
{
    efx_surface s = {};
    s.layout = atoi(v[0]), s.shift = atoi(v[1]), s.swap_uv = atoi(v[2]), s.width = atoi(v[3]), s.height = atoi(v[4]);
    for (int i = 0; i < 3; i++)
        s.offset[i] = strtoull(v[5 + i], nullptr, 10), s.pitch[i] = strtoull(v[8 + i], nullptr, 10);
    s.bytes = strtoull(v[11], nullptr, 10);
    return s;
}

// the source of n images: a heap block of exactly the contract's size (operator new[] hands out 16-byte aligned blocks)
std::unique_ptr<uint8_t[]> read_source(const char* path, const efx_surface& s, size_t n, size_t stride)
{
    const size_t last = (s.bytes + 15) / 16 * 16, total = stride * (n - 1) + last;
    std::unique_ptr<uint8_t[]> src(new uint8_t[total]());
    FILE* in = fopen(path, "rb");
    for (size_t k = 0; in && k < n; k++)
        if (fread(src.get() + k * stride, 1, s.bytes, in) != s.bytes) {
            fclose(in);
            in = nullptr;
        }
    if (!in) {
        fprintf(stderr, "cannot read %zu images of %zu bytes from %s\n", n, s.bytes, path);
        exit(1);
    }
    fclose(in);
    return src;
}

void write_file(const char* path, const void* p, size_t bytes)
{
    FILE* o = fopen(path, "wb");
    if (!o || fwrite(p, 1, bytes, o) != bytes) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(1);
    }
    fclose(o);
}

// k_import's stage(): whole 16-byte pieces
int stage(const uint8_t* img, size_t off, int len, uint8_t* buf)
{
    const ipx::Span sp = ipx::span(off, len);
    for (int i = 0; i < sp.pieces; i++)
        memcpy(buf + 16 * i, img + sp.a0 + 16 * (size_t)i, 16);
    return sp.shift;
}

// k_import's reduce_row() and split_row(), every lane's steps in turn
void reduce_row(const uint8_t* raw, int sh, int n, int shift, uint8_t* row)
{
    for (int x = 0; x < n; x += 4) {
        uint32_t w[2];
        spx::dwords_at<2>(raw, sh + 2 * x, w);
        const uint32_t y4 = spx::reduce4(w[0], w[1], shift);
        memcpy(row + x, &y4, 4);
    }
}

void split_row(bool words, const uint8_t* raw, int sh, int n, int shift, uint8_t* first, uint8_t* second)
{
    for (int x = 0; x < n; x += 4) {
        uint32_t a4, b4;
        if (words) {
            uint32_t p[4];
            spx::dwords_at<4>(raw, sh + 4 * x, p);
            spx::split_pairs16(p, shift, &a4, &b4);
        } else {
            uint32_t p[2];
            spx::dwords_at<2>(raw, sh + 2 * x, p);
            spx::split_pairs8(p[0], p[1], &a4, &b4);
        }
        memcpy(first + x, &a4, 4);
        memcpy(second + x, &b4, 4);
    }
}

int vcoef(const ImportTap& t, int s)
{
    const unsigned i = (unsigned)(s - t.start);
    return i < (unsigned)t.count ? t.k[i] : 0;
}

int hsum(const uint8_t* row, const ImportTap& t)
{
    int sum = 0;
    for (int i = 0; i < t.count; i += 4)
        for (int j = i; j < i + 4; j++)
            sum += (int)t.k[j] * (int)row[t.start + j];
    return ipx::hround(sum);
}

// k_import_taps, lane by lane (the canonical image is I420)
void fill_taps(const ImportArgs& a, ImportTap* table)
{
    for (int i = 0; i < kImportTapRows; i++) {
        int d, S, D;
        if (i < kImportTapLY)
            d = i - kImportTapLX, S = a.crop_w, D = a.dst_w;
        else if (i < kImportTapCX)
            d = i - kImportTapLY, S = a.crop_h, D = a.dst_h;
        else if (i < kImportTapCY)
            d = i - kImportTapCX, S = a.crop_w / 2, D = a.dst_w / 2;
        else
            d = i - kImportTapCY, S = a.crop_h / 2, D = a.dst_h / 2;
        if (d >= D)
            continue;
        int n;
        table[i].start = ipx::taps(S, D, d, &n, table[i].k);
        table[i].count = n;
        for (int j = n; j < kImportTapSlots; j++)
            table[i].k[j] = 0;
    }
}

// import_band<an EFX_SURF_* layout> of k_import.hip for every band of one image
void import_image(const ImportArgs& a, const efx_surface& sf, const ImportTap* taps, const uint8_t* img, uint8_t* out)
{
    const bool words = spx::is_words(sf.layout), semi = spx::is_semi(sf.layout);
    const int B = words ? 2 : 1;
    std::unique_ptr<uint8_t[]> raw(new uint8_t[kRawBuf]()), row0(new uint8_t[kRowBuf]()), row1(new uint8_t[kRowBuf]()),
        row2(new uint8_t[kRowBuf]());
    uint8_t* row[3] = {row0.get(), row1.get(), row2.get()};
    for (int band = 0; band < kImportBands; band++) {
        const int y0 = band * kRows, cy0 = band * kCRows;
        memset(out + y0 * kW, 16, kRows * kW);
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
        for (int s = ls0; s < ls1; s++) {
            const int sh = stage(img, spx::crop_row(sf, 0, a.crop_x, a.crop_y, s), B * a.crop_w, words ? raw.get() : row[0]);
            if (words)
                reduce_row(raw.get(), sh, a.crop_w, sf.shift, row[0]);
            const uint8_t* r = row[0] + (words ? 0 : sh);
            for (int x = 0; x < a.dst_w; x++) {
                const int h = hsum(r, taps[kImportTapLX + x]);
                for (int k = 0; k < nl; k++)
                    accl[(size_t)k * a.dst_w + x] += vcoef(tly[k], s) * h;
            }
        }
        const int cw = a.crop_w / 2;
        for (int s = cs0; s < cs1; s++) {
            int sh[2] = {0, 0};
            if (semi) {
                const int shp = stage(img, spx::crop_row(sf, 1, a.crop_x, a.crop_y, s), B * a.crop_w, raw.get());
                split_row(words, raw.get(), shp, cw, sf.shift, row[1 + sf.swap_uv], row[2 - sf.swap_uv]);
            } else {
                for (int c = 0; c < 2; c++)
                    sh[c] = stage(img, spx::crop_row(sf, 1 + c, a.crop_x, a.crop_y, s), B * cw, words ? raw.get() + c * kRawHalf : row[1 + c]);
                if (words) {
                    for (int c = 0; c < 2; c++)
                        reduce_row(raw.get() + c * kRawHalf, sh[c], cw, sf.shift, row[1 + c]);
                    sh[0] = sh[1] = 0;
                }
            }
            for (int x = 0; x < a.dst_w; x++) {
                const int plane = x >= a.dst_w / 2, col = x - plane * (a.dst_w / 2);
                const int h = hsum(row[1 + plane] + sh[plane], taps[kImportTapCX + col]);
                for (int k = 0; k < nc; k++)
                    accc[(size_t)k * a.dst_w + x] += vcoef(tcy[k], s) * h;
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

// k_crop_sums_surf8 / _surf16 for one image: every luma row staged into a slot of the layout's size, read four columns at
// a time; R[0 .. H) then C[0 .. W)
void sum_image(const efx_surface& sf, const uint8_t* img, uint32_t* sums)
{
    const bool words = spx::is_words(sf.layout);
    const int W = sf.width, H = sf.height;
    const cpx::Layout L = spx::crop_layout(W, words ? 2 : 1);
    std::unique_ptr<uint32_t[]> slot(new uint32_t[L.seg_cap / 4]());
    std::fill(sums, sums + H + W, 0u);
    for (int y = 0; y < H; y++) {
        const ipx::Span sp = ipx::span(sf.offset[0] + (size_t)y * sf.pitch[0], L.seg_len);
        if (16 * sp.pieces > L.seg_cap - 16) {
            fprintf(stderr, "row %d: %d pieces do not fit the slot\n", y, sp.pieces);
            exit(1);
        }
        for (int i = 0; i < sp.pieces; i++)
            memcpy(reinterpret_cast<uint8_t*>(slot.get()) + 16 * i, img + sp.a0 + 16 * (size_t)i, 16);
        for (int x = 0; x < W; x += cpx::kLaneCols) {
            const uint32_t y4 = words ? spx::luma4<true>(slot.get(), sp.shift, x, W, sf.shift) : spx::luma4<false>(slot.get(), sp.shift, x, W, sf.shift);
            for (int q = 0; q < 4 && x + q < W; q++) {
                sums[y] += (y4 >> (8 * q)) & 0xFF;
                sums[H + x + q] += (y4 >> (8 * q)) & 0xFF;
            }
        }
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "reduce")) {
        const int shift = atoi(argv[2]);
        std::vector<uint8_t> out(2 << 16);
        for (uint32_t w = 0; w < 65536; w++) {
            out[w] = (uint8_t)spx::reduce(w, shift);
            // the packed path, the word in each of the four places in turn beside the word that wraps
            const uint32_t other = 0xFFFFu, place = w & 3;
            const uint32_t w01 = place == 0 ? (w | other << 16) : place == 1 ? (other | w << 16) : other | other << 16;
            const uint32_t w23 = place == 2 ? (w | other << 16) : place == 3 ? (other | w << 16) : other | other << 16;
            const uint32_t y4 = spx::reduce4(w01, w23, shift);
            out[65536 + w] = (uint8_t)(y4 >> (8 * place));
            for (uint32_t q = 0; q < 4; q++)
                if (q != place && ((y4 >> (8 * q)) & 0xFF) != 255)
                    return 3;
        }
        fwrite(out.data(), 1, out.size(), stdout);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "layout")) {
        efx_surface s = {};
        const size_t bytes = spx::layout(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), strtoull(argv[5], nullptr, 10), atoi(argv[6]), &s);
        printf("%zu %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu\n", bytes, s.layout, s.shift, s.swap_uv, s.width, s.height, s.offset[0],
               s.offset[1], s.offset[2], s.pitch[0], s.pitch[1], s.pitch[2], s.bytes);
        return 0;
    }
    if (argc == 14 && !strcmp(argv[1], "check")) {
        printf("%d\n", spx::check(parse_surface(argv + 2)));
        return 0;
    }
    if (argc == 26 && !strcmp(argv[1], "import")) {
        const efx_surface sf = parse_surface(argv + 2);
        if (spx::check(sf) != spx::kOk)
            return 2;
        const size_t n = strtoull(argv[14], nullptr, 10), stride = strtoull(argv[15], nullptr, 10);
        ImportArgs a{};
        a.format = EFX_PIX_I420, a.width = sf.width, a.height = sf.height;
        int* f[] = {&a.crop_x, &a.crop_y, &a.crop_w, &a.crop_h, &a.dst_x, &a.dst_y, &a.dst_w, &a.dst_h};
        for (int i = 0; i < 8; i++)
            *f[i] = atoi(argv[16 + i]);
        const std::unique_ptr<uint8_t[]> src = read_source(argv[24], sf, n, stride);
        std::unique_ptr<uint8_t[]> dst(new uint8_t[n * kFrameBytes]);
        std::unique_ptr<ImportTap[]> table(new ImportTap[kImportTapRows]);
        fill_taps(a, table.get());
        for (size_t k = 0; k < n; k++)
            import_image(a, sf, table.get(), src.get() + k * stride, dst.get() + k * kFrameBytes);
        write_file(argv[25], dst.get(), n * kFrameBytes);
        return 0;
    }
    if (argc == 21 && !strcmp(argv[1], "crop")) {
        const efx_surface sf = parse_surface(argv + 2);
        if (spx::check(sf) != spx::kOk)
            return 2;
        const int n_streams = atoi(argv[14]), per = atoi(argv[15]), limit = atoi(argv[17]), round = atoi(argv[18]);
        const size_t stride = strtoull(argv[16], nullptr, 10), n = (size_t)n_streams * per;
        const int W = sf.width, H = sf.height;
        const std::unique_ptr<uint8_t[]> src = read_source(argv[19], sf, n, stride);
        std::vector<uint32_t> out(n * (H + W) + (size_t)n_streams * 8);
        for (size_t k = 0; k < n; k++)
            sum_image(sf, src.get() + k * stride, out.data() + k * (H + W));
        // k_crop_rects
        for (int st = 0; st < n_streams; st++) {
            int x1 = W, y1 = H, x2 = -1, y2 = -1;
            for (int i = 0; i < per; i++) {
                const uint32_t* sums = out.data() + ((size_t)st * per + i) * (H + W);
                int top = H, bottom = -1, left = W, right = -1;
                for (int y = 0; y < H; y++)
                    if (cpx::is_picture(sums[y], limit, W))
                        top = std::min(top, y), bottom = std::max(bottom, y);
                for (int x = 0; x < W; x++)
                    if (cpx::is_picture(sums[H + x], limit, H))
                        left = std::min(left, x), right = std::max(right, x);
                if (bottom >= 0 && right >= 0)
                    x1 = std::min(x1, left), y1 = std::min(y1, top), x2 = std::max(x2, right), y2 = std::max(y2, bottom);
            }
            int32_t rec[8];
            cpx::record(W, H, round, x1, y1, x2, y2, rec);
            memcpy(out.data() + n * (H + W) + (size_t)st * 8, rec, sizeof rec);
        }
        write_file(argv[20], out.data(), out.size() * 4);
        return 0;
    }
    fprintf(stderr, "usage: see the head of tests/surface_model_main.cpp\n");
    return 2;
}
