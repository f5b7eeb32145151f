// TEST: the import's HDR stage on the host, with hdr_px.h's functions and the kernels' own index arithmetic.  The tables
// come from a file (the 6624 bytes efx_import_hdr_tables hands out), so the program has no pow() of its own.  `import`
// performs whole HDR imports as k_import_surf*_h do: the tap table of k_import_taps, the bands and their vertical
// supports, every row fetched as 16-byte pieces aligned down inside the image (ipx::span) into buffers of the kernels'
// sizes, the lanes' columns at 10 bits into a band of 16-bit samples, then the HDR stage item by item -- the part of the
// destination rectangle inside the band -- from that band into the 8-bit band.  The source lives in a heap block of
// exactly src_stride x (n - 1) + bytes rounded up to 16, the tables, both bands and every output in blocks of exactly
// their sizes, so a sanitizer build (-fsanitize=address,undefined: tests/test_hdr_model.py) sees every byte the kernels'
// addressing would touch.
//
//   hdr_model_main coefs PRIMARIES MATRIX RANGE PEAK HEIGHT   (hdr::valid for transfer 16, then the 16 ints of hdr::Coefs, as text)
//   hdr_model_main lattice TABLES OUT_FILE   (every Y10 0 .. 1020 x Cb10, Cr10 = 0, 4 .. 1020, the item's four luma samples
//                                             equal: 1021 x 256 x 256 bytes of Y', then as many of Cb', then of Cr')
//   hdr_model_main blocks TABLES N IN_FILE OUT_FILE           (IN: N x (Y10 x 4, Cb10, Cr10) uint16; OUT: N x (Y' x 4, Cb', Cr') bytes)
//   hdr_model_main import TABLES SURFACE N SRC_STRIDE CROP_X CROP_Y CROP_W CROP_H DST_X DST_Y DST_W DST_H SRC_FILE DST_FILE DST10_FILE
//                                            (DST10: per image 101376 uint16, import10 inside the rectangle, zero outside)
//   SURFACE = LAYOUT SHIFT SWAP_UV WIDTH HEIGHT OFFSET0 OFFSET1 OFFSET2 PITCH0 PITCH1 PITCH2 BYTES
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "efx.h"
#include "efx_internal.h"
#include "hdr_px.h"
#include "surface_px.h"

using namespace efx;

namespace {

constexpr int kW = EFX_FRAME_WIDTH, kH = EFX_FRAME_HEIGHT, kYBytes = kW * kH, kCBytes = kYBytes / 4;
constexpr int kRows = kImportBandRows, kCRows = kRows / 2;
constexpr int kBandY = kRows * kW, kBandC = kCRows * (kW / 2), kBandBytes = kBandY + 2 * kBandC;
constexpr int kRowBuf = kImportMaxWidth + 32, kRawBuf = 3 * kRowBuf + 16, kRawHalf = (kRawBuf / 2) & ~15;
constexpr int kThreads = 256;

efx_surface parse_surface(char** v)
{
    efx_surface s = {};
    s.layout = atoi(v[0]), s.shift = atoi(v[1]), s.swap_uv = atoi(v[2]), s.width = atoi(v[3]), s.height = atoi(v[4]);
    for (int i = 0; i < 3; i++)
        s.offset[i] = strtoull(v[5 + i], nullptr, 10), s.pitch[i] = strtoull(v[8 + i], nullptr, 10);
    s.bytes = strtoull(v[11], nullptr, 10);
    return s;
}

// the setting's tables in a heap block of exactly their size
std::unique_ptr<hdr::Tables> read_tables(const char* path)
{
    std::unique_ptr<hdr::Tables> t(new hdr::Tables);
    FILE* in = fopen(path, "rb");
    if (!in || fread(t.get(), 1, sizeof(hdr::Tables), in) != sizeof(hdr::Tables)) {
        fprintf(stderr, "cannot read %zu bytes of tables from %s\n", sizeof(hdr::Tables), path);
        exit(1);
    }
    fclose(in);
    return t;
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

// the kernels' tonemap_band(), lane by lane
void tonemap_band(const ImportArgs& a, const hdr::Tables* tab, int y0, const uint16_t* b10, uint8_t* band)
{
    const colour::BandPart p = colour::band_part(a.dst_x, a.dst_y, a.dst_w, a.dst_h, y0, kRows);
    const hdr::Coefs k = tab->k;
    for (int tid = 0; tid < kThreads; tid++)
        for (int r = 0; r < p.rows; r++)
            for (int c = tid; c < p.cols; c += kThreads)
                hdr::tonemap_item(k, tab->pq, tab->gam, p, r, c, kW, kRows, b10, band);
}

// import_surface_band<an EFX_SURF_* layout, false, true> of k_import.hip for every band of one image; out10 receives the
// 10-bit bands
void import_image(const ImportArgs& a, const efx_surface& sf, const ImportTap* taps, const hdr::Tables* tab, const uint8_t* img, uint8_t* out,
                  uint16_t* out10)
{
    const bool words = spx::is_words(sf.layout), semi = spx::is_semi(sf.layout);
    const int B = words ? 2 : 1;
    std::unique_ptr<uint8_t[]> raw(new uint8_t[kRawBuf]()), row0(new uint8_t[kRowBuf]()), row1(new uint8_t[kRowBuf]()),
        row2(new uint8_t[kRowBuf]());
    uint8_t* row[3] = {row0.get(), row1.get(), row2.get()};
    for (int band = 0; band < kImportBands; band++) {
        const int y0 = band * kRows, cy0 = band * kCRows;
        std::unique_ptr<uint8_t[]> s_out(new uint8_t[kBandBytes]);     // the kernels' 8-bit band: Y, Cb, Cr, on the border colour
        std::unique_ptr<uint16_t[]> s_b10(new uint16_t[kBandBytes]);   // ... and the 10-bit band: only what the lanes write is read
        memset(s_out.get(), 16, kBandY);
        memset(s_out.get() + kBandY, 128, 2 * kBandC);
        const int l0 = std::max(y0, a.dst_y) - a.dst_y, nl = std::min(y0 + kRows, a.dst_y + a.dst_h) - a.dst_y - l0;
        const int c0 = std::max(cy0, a.dst_y / 2) - a.dst_y / 2, nc = std::min(cy0 + kCRows, (a.dst_y + a.dst_h) / 2) - a.dst_y / 2 - c0;
        if (nl > 0) {
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
            // the lanes' columns into the 10-bit band
            for (int k = 0; k < nl; k++)
                for (int x = 0; x < a.dst_w; x++)
                    s_b10[(a.dst_y + l0 + k - y0) * kW + a.dst_x + x] = (uint16_t)hdr::vround10(accl[(size_t)k * a.dst_w + x]);
            for (int k = 0; k < nc; k++)
                for (int x = 0; x < a.dst_w; x++) {
                    const int plane = x >= a.dst_w / 2, col = x - plane * (a.dst_w / 2);
                    s_b10[kBandY + plane * kBandC + (a.dst_y / 2 + c0 + k - cy0) * (kW / 2) + a.dst_x / 2 + col] =
                        (uint16_t)hdr::vround10(accc[(size_t)k * a.dst_w + x]);
                }
            tonemap_band(a, tab, y0, s_b10.get(), s_out.get());
            // (the record of import10: what the lanes wrote)
            for (int k = 0; k < nl; k++)
                for (int x = 0; x < a.dst_w; x++)
                    out10[(a.dst_y + l0 + k) * kW + a.dst_x + x] = s_b10[(a.dst_y + l0 + k - y0) * kW + a.dst_x + x];
            for (int k = 0; k < nc; k++)
                for (int x = 0; x < a.dst_w; x++) {
                    const int plane = x >= a.dst_w / 2, col = x - plane * (a.dst_w / 2);
                    out10[kYBytes + plane * kCBytes + (a.dst_y / 2 + c0 + k) * (kW / 2) + a.dst_x / 2 + col] =
                        s_b10[kBandY + plane * kBandC + (a.dst_y / 2 + c0 + k - cy0) * (kW / 2) + a.dst_x / 2 + col];
                }
        }
        memcpy(out + y0 * kW, s_out.get(), kBandY);
        memcpy(out + kYBytes + cy0 * (kW / 2), s_out.get() + kBandY, kBandC);
        memcpy(out + kYBytes + kCBytes + cy0 * (kW / 2), s_out.get() + kBandY + kBandC, kBandC);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 7 && !strcmp(argv[1], "coefs")) {
        const int primaries = atoi(argv[2]), matrix = atoi(argv[3]), full = atoi(argv[4]), peak = atoi(argv[5]);
        hdr::Coefs k{};
        const bool ok = hdr::valid(hdr::kTransferPq, primaries, matrix, full, peak) && hdr::coefs(primaries, matrix, full, peak, atoi(argv[6]), &k);
        printf("%d", ok ? 1 : 0);
        const int32_t* v = &k.qy;
        for (int i = 0; i < 16; i++)
            printf(" %d", (int)v[i]);
        printf("\n");
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "lattice")) {
        const std::unique_ptr<hdr::Tables> t = read_tables(argv[2]);
        const size_t plane = (size_t)1021 * 256 * 256;
        std::vector<uint8_t> out(3 * plane);
        for (int y = 0; y <= 1020; y++)
            for (int cb = 0; cb < 256; cb++)
                for (int cr = 0; cr < 256; cr++) {
                    const uint16_t y4[4] = {(uint16_t)y, (uint16_t)y, (uint16_t)y, (uint16_t)y};
                    uint8_t o[4], ob, orr;
                    hdr::tonemap_block(t->k, t->pq, t->gam, y4, 4 * cb, 4 * cr, 2, o, &ob, &orr);
                    const size_t i = ((size_t)y * 256 + cb) * 256 + cr;
                    out[i] = o[3], out[plane + i] = ob, out[2 * plane + i] = orr;
                }
        write_file(argv[3], out.data(), out.size());
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "blocks")) {
        const std::unique_ptr<hdr::Tables> t = read_tables(argv[2]);
        const size_t n = strtoull(argv[3], nullptr, 10);
        std::vector<uint16_t> in(6 * n);
        std::vector<uint8_t> out(6 * n);
        FILE* f = fopen(argv[4], "rb");
        if (!f || fread(in.data(), 2, 6 * n, f) != 6 * n) {
            fprintf(stderr, "cannot read %zu blocks from %s\n", n, argv[4]);
            return 1;
        }
        fclose(f);
        for (size_t i = 0; i < n; i++) {
            const uint16_t* b = in.data() + 6 * i;
            hdr::tonemap_block(t->k, t->pq, t->gam, b, b[4], b[5], 2, out.data() + 6 * i, out.data() + 6 * i + 4, out.data() + 6 * i + 5);
        }
        write_file(argv[5], out.data(), out.size());
        return 0;
    }
    if (argc == 28 && !strcmp(argv[1], "import")) {
        const std::unique_ptr<hdr::Tables> t = read_tables(argv[2]);
        const efx_surface sf = parse_surface(argv + 3);
        if (spx::check(sf) != spx::kOk)
            return 2;
        const size_t n = strtoull(argv[15], nullptr, 10), stride = strtoull(argv[16], nullptr, 10);
        ImportArgs a{};
        a.format = EFX_PIX_I420, a.width = sf.width, a.height = sf.height;
        int* f[] = {&a.crop_x, &a.crop_y, &a.crop_w, &a.crop_h, &a.dst_x, &a.dst_y, &a.dst_w, &a.dst_h};
        for (int i = 0; i < 8; i++)
            *f[i] = atoi(argv[17 + i]);
        const std::unique_ptr<uint8_t[]> src = read_source(argv[25], sf, n, stride);
        std::unique_ptr<uint8_t[]> dst(new uint8_t[n * kFrameBytes]);
        std::unique_ptr<uint16_t[]> dst10(new uint16_t[n * kFrameBytes]());
        std::unique_ptr<ImportTap[]> table(new ImportTap[kImportTapRows]);
        fill_taps(a, table.get());
        for (size_t k = 0; k < n; k++)
            import_image(a, sf, table.get(), t.get(), src.get() + k * stride, dst.get() + k * kFrameBytes, dst10.get() + k * kFrameBytes);
        write_file(argv[26], dst.get(), n * kFrameBytes);
        write_file(argv[27], dst10.get(), n * kFrameBytes * 2);
        return 0;
    }
    fprintf(stderr, "usage: see the head of tests/hdr_model_main.cpp\n");
    return 2;
}
