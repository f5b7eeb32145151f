// TEST: a whole efx_detect_crop on the host, with crop_px.h's functions and k_cropdetect's own index arithmetic: the
// bands of 64 rows, the groups of rows staged as 16-byte pieces aligned down inside the image (ipx::span) into a block of
// the kernel's LDS size, wave r % 4 taking row r, a lane's 4 columns of every 256 read as aligned words, the packed
// 16-bit column sums, and the rectangle pass wave by wave.  Every source image lives in a heap block of exactly the bytes
// the contract lets the kernels read (its size rounded up to 16; I420: width x height rounded up to 16), every image's
// sums in a block of exactly height + width elements and the records in one of exactly 8 n_streams, so a sanitizer
// build (-fsanitize=address,undefined: tests/test_crop_model.py) sees every byte the kernels' addressing would touch.
//
//   crop_model_main detect FORMAT WIDTH HEIGHT FULL_RANGE LIMIT ROUND N_STREAMS IMAGES_PER_STREAM SRC_FILE SUMS_FILE RECS_FILE
//                          (SRC_FILE: the images packed; SUMS_FILE: height + width uint32 per image; RECS_FILE: 8 int32 per stream)
//   crop_model_main luma FULL_RANGE     (the luma byte of every (R, G, B), R major, B minor, to stdout; exit 1 if one is
//                                        not the low byte of ipx::ycbcr)
//   crop_model_main round R             (ok, pos, len as int32 for every 0 <= a <= b < 70, a major, to stdout)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "crop_px.h"
#include "efx.h"
#include "import_px.h"

using namespace efx;

namespace {

struct Args {
    int format, width, height, full_range, limit, round, n_streams, images_per_stream;
};

// k_crop_sums: one band of one image
template <int FORMAT>
void sum_band(const Args& a, const uint8_t* img, uint32_t* sums, int band, uint32_t* stage)
{
    const int W = a.width, H = a.height;
    const cpx::Layout L = cpx::layout(FORMAT, W);
    const ipx::Matrix m = ipx::matrix(a.full_range);
    const int y0 = band * cpx::kBandRows, y1 = std::min(y0 + cpx::kBandRows, H);
    const int slots = L.seg_cap >> 4;
    std::vector<uint32_t> even((size_t)cpx::kWaves * 64 * cpx::kColGroups, 0), odd(even);
    for (int g0 = y0; g0 < y1; g0 += L.group_rows) {
        const int g = std::min(L.group_rows, y1 - g0);
        const int total = g * L.nseg * slots;
        for (int q = 0; q < total; q++) {
            const int slot = q / slots, i = q - slot * slots;
            const int row = slot / L.nseg, s = slot - row * L.nseg;
            const ipx::Span sp = ipx::span(cpx::seg_offset(FORMAT, s, W, H, g0 + row), L.seg_len);
            if (i < sp.pieces)
                memcpy(reinterpret_cast<uint8_t*>(stage) + slot * L.seg_cap + 16 * i, img + sp.a0 + 16 * (size_t)i, 16);
        }
        for (int r = 0; r < g; r++) {
            const int wave = r % cpx::kWaves;
            int shift[3] = {0, 0, 0};
            for (int s = 0; s < L.nseg; s++)
                shift[s] = ipx::span(cpx::seg_offset(FORMAT, s, W, H, g0 + r), L.seg_len).shift;
            const uint32_t* seg = stage + ((r * L.nseg * L.seg_cap) >> 2);
            uint32_t rs = 0;
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < cpx::kColGroups; j++) {
                    const int x = 256 * j + cpx::kLaneCols * lane;
                    if (256 * j < W && x < W) {
                        const size_t k = ((size_t)wave * 64 + lane) * cpx::kColGroups + j;
                        rs += cpx::add4(cpx::luma4<FORMAT>(m, seg, L.seg_cap, shift, x, W), &even[k], &odd[k]);
                    }
                }
            sums[g0 + r] = rs;
        }
    }
    // the column sums meet in the stage, then leave
    for (int x = 0; x < W + 4; x++)
        stage[x] = 0;
    for (int wave = 0; wave < cpx::kWaves; wave++)
        for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < cpx::kColGroups; j++) {
                const int x = 256 * j + cpx::kLaneCols * lane;
                if (256 * j < W && x < W) {
                    const size_t k = ((size_t)wave * 64 + lane) * cpx::kColGroups + j;
                    stage[x] += even[k] & 0xFFFF;
                    stage[x + 1] += odd[k] & 0xFFFF;
                    stage[x + 2] += even[k] >> 16;
                    stage[x + 3] += odd[k] >> 16;
                }
            }
    for (int x = 0; x < W; x++)
        sums[H + x] += stage[x];
}

// k_crop_rects: one stream
void rect_of_stream(const Args& a, uint32_t* const* sums_of, int stream, int32_t* rec)
{
    const int W = a.width, H = a.height;
    int bounds[cpx::kWaves][4];
    for (int wave = 0; wave < cpx::kWaves; wave++) {
        int x1 = W, y1 = H, x2 = -1, y2 = -1;
        for (int i = wave; i < a.images_per_stream; i += cpx::kWaves) {
            const uint32_t* sums = sums_of[(size_t)stream * a.images_per_stream + i];
            int top = H, bottom = -1, left = W, right = -1;
            for (int y = 0; y < H; y++)
                if (cpx::is_picture(sums[y], a.limit, W))
                    top = std::min(top, y), bottom = std::max(bottom, y);
            for (int x = 0; x < W; x++)
                if (cpx::is_picture(sums[H + x], a.limit, H))
                    left = std::min(left, x), right = std::max(right, x);
            if (bottom >= 0 && right >= 0)
                x1 = std::min(x1, left), y1 = std::min(y1, top), x2 = std::max(x2, right), y2 = std::max(y2, bottom);
        }
        bounds[wave][0] = x1, bounds[wave][1] = y1, bounds[wave][2] = x2, bounds[wave][3] = y2;
    }
    int x1 = bounds[0][0], y1 = bounds[0][1], x2 = bounds[0][2], y2 = bounds[0][3];
    for (int w = 1; w < cpx::kWaves; w++)
        x1 = std::min(x1, bounds[w][0]), y1 = std::min(y1, bounds[w][1]), x2 = std::max(x2, bounds[w][2]), y2 = std::max(y2, bounds[w][3]);
    cpx::record(W, H, a.round, x1, y1, x2, y2, rec);
}

int detect(char** argv)
{
    Args a{};
    int* f[] = {&a.format, &a.width, &a.height, &a.full_range, &a.limit, &a.round, &a.n_streams, &a.images_per_stream};
    for (int i = 0; i < 8; i++)
        *f[i] = atoi(argv[2 + i]);
    const bool i420 = a.format == EFX_PIX_I420;
    const size_t image = (size_t)a.width * a.height * (i420 ? 3 : 6) / 2;
    const size_t readable = ((i420 ? (size_t)a.width * a.height : image) + 15) / 16 * 16;
    const size_t n = (size_t)a.n_streams * a.images_per_stream;
    // operator new[] hands out 16-byte aligned blocks, like the device pointers of the contract
    std::vector<std::unique_ptr<uint8_t[]>> src(n);
    std::vector<std::unique_ptr<uint32_t[]>> sums(n);
    std::vector<uint32_t*> sums_of(n);
    FILE* in = fopen(argv[10], "rb");
    std::vector<uint8_t> whole(image);
    for (size_t k = 0; k < n; k++) {
        src[k].reset(new uint8_t[readable]());
        sums[k].reset(new uint32_t[(size_t)a.height + a.width]);
        sums_of[k] = sums[k].get();
        if (!in || fread(whole.data(), 1, image, in) != image) {
            fprintf(stderr, "cannot read %zu images of %zu bytes from %s\n", n, image, argv[10]);
            return 1;
        }
        memcpy(src[k].get(), whole.data(), std::min(image, readable));
    }
    fclose(in);
    std::unique_ptr<uint32_t[]> stage(new uint32_t[cpx::kStageBytes / 4]());
    std::unique_ptr<int32_t[]> recs(new int32_t[(size_t)a.n_streams * 8]);
    const int bands = (a.height + cpx::kBandRows - 1) / cpx::kBandRows;
    for (size_t k = 0; k < n; k++) {
        for (int x = 0; x < a.width; x++)  // k_crop_zero
            sums_of[k][a.height + x] = 0;
        for (int band = 0; band < bands; band++) {
            if (a.format == EFX_PIX_I420)
                sum_band<EFX_PIX_I420>(a, src[k].get(), sums_of[k], band, stage.get());
            else if (a.format == EFX_PIX_RGB24)
                sum_band<EFX_PIX_RGB24>(a, src[k].get(), sums_of[k], band, stage.get());
            else
                sum_band<EFX_PIX_RGBP>(a, src[k].get(), sums_of[k], band, stage.get());
        }
    }
    for (int s = 0; s < a.n_streams; s++)
        rect_of_stream(a, sums_of.data(), s, recs.get() + 8 * (size_t)s);
    FILE* o = fopen(argv[11], "wb");
    for (size_t k = 0; o && k < n; k++)
        if (fwrite(sums_of[k], 4, (size_t)a.height + a.width, o) != (size_t)a.height + a.width)
            return 1;
    if (!o || fclose(o))
        return 1;
    o = fopen(argv[12], "wb");
    if (!o || fwrite(recs.get(), 4, (size_t)a.n_streams * 8, o) != (size_t)a.n_streams * 8 || fclose(o))
        return 1;
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "luma")) {
        const ipx::Matrix m = ipx::matrix(atoi(argv[2]));
        std::vector<uint8_t> out(1 << 16);
        int differs = 0;
        for (int r = 0; r < 256; r++) {
            for (int g = 0; g < 256; g++)
                for (int b = 0; b < 256; b++) {
                    const int y = cpx::luma(m, r, g, b);
                    differs |= y != (int)(ipx::ycbcr(m, r, g, b) & 0xFF);
                    out[g * 256 + b] = (uint8_t)y;
                }
            fwrite(out.data(), 1, out.size(), stdout);
        }
        return differs;
    }
    if (argc == 3 && !strcmp(argv[1], "round")) {
        const int r = atoi(argv[2]);
        for (int a = 0; a < 70; a++)
            for (int b = a; b < 70; b++) {
                int32_t rec[3] = {0, -1, -1};
                int pos, len;
                if (cpx::round_axis(a, b, r, &pos, &len))
                    rec[0] = 1, rec[1] = pos, rec[2] = len;
                fwrite(rec, 4, 3, stdout);
            }
        return 0;
    }
    if (argc == 13 && !strcmp(argv[1], "detect"))
        return detect(argv);
    fprintf(stderr, "usage: see the head of tests/crop_model_main.cpp\n");
    return 2;
}
