// TEST: the import's colour conversion on the host, with colour_px.h's functions and the kernels' own index arithmetic: a
// 352 x 192 picture is taken band by band (8 luma rows, 4 rows of each chroma plane) into a heap block of exactly the
// band's size, laid out as the kernels' LDS band, and converted item by item -- the part of the destination rectangle
// inside the band, a chroma site and its 2 x 2 luma samples per item, luma before chroma.  A sanitizer build
// (-fsanitize=address,undefined: tests/test_colour_model.py) sees every byte that addressing would touch.
//
//   colour_model_main coefs MATRIX RANGE HEIGHT       (efx_import_colour_coefs' result, the nine q and y0, as text)
//   colour_model_main pixels MATRIX RANGE Y CB CR ... (the converted triples, one per line)
//   colour_model_main precision MATRIX RANGE          (every (Y, Cb, Cr): the largest difference between the integer result
//                                                      and the rounded float64 value of the exact affine map, clamped;
//                                                      the number of triples with a difference; 2^24)
//   colour_model_main picture MATRIX RANGE HEIGHT DST_X DST_Y DST_W DST_H SRC_FILE DST_FILE
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "efx.h"
#include "efx_internal.h"
#include "colour_px.h"

using namespace efx;

namespace {

constexpr int kW = EFX_FRAME_WIDTH, kH = EFX_FRAME_HEIGHT, kYBytes = kW * kH, kCBytes = kYBytes / 4;
constexpr int kRows = kImportBandRows, kCRows = kRows / 2;
constexpr int kBandY = kRows * kW, kBandC = kCRows * (kW / 2), kBandBytes = kBandY + 2 * kBandC;
constexpr int kThreads = 256;

// The exact affine map in float64, from (Kr, Kb) -- not from the header's table
struct Exact {
    double m[3][3];
    int y0;
};

bool exact_map(int matrix, int full_range, Exact* e)
{
    double kr, kb;
    switch (matrix) {
    case 1: kr = 0.2126, kb = 0.0722; break;
    case 4: kr = 0.30, kb = 0.11; break;
    case 5: case 6: kr = 0.299, kb = 0.114; break;
    case 7: kr = 0.212, kb = 0.087; break;
    case 9: kr = 0.2627, kb = 0.0593; break;
    default: return false;
    }
    const double kg = 1 - kr - kb, tr = 0.299, tb = 0.114, tg = 1 - tr - tb;
    const double rgb[3][3] = {{1, 0, 2 * (1 - kr)}, {1, -2 * (1 - kb) * kb / kg, -2 * (1 - kr) * kr / kg}, {1, 2 * (1 - kb), 0}};
    const double to[3][3] = {{tr, tg, tb},
                             {-tr / (2 * (1 - tb)), -tg / (2 * (1 - tb)), 0.5},
                             {0.5, -tg / (2 * (1 - tr)), -tb / (2 * (1 - tr))}};
    const double in[3] = {full_range ? 255.0 : 219.0, full_range ? 255.0 : 224.0, full_range ? 255.0 : 224.0};
    const double out[3] = {219, 224, 224};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = 0;
            for (int k = 0; k < 3; k++)
                v += to[i][k] * rgb[k][j];
            e->m[i][j] = v * out[i] / in[j];
        }
    e->y0 = full_range ? 0 : 16;
    return true;
}

int round_clamp(double v)
{
    const double r = std::floor(v + 0.5);
    return r < 0 ? 0 : (r > 255 ? 255 : (int)r);
}

// The kernels' convert_band(), lane by lane, on a band of its own
void convert_band(const colour::Coefs& k, int dst_x, int dst_y, int dst_w, int dst_h, int y0, uint8_t* band)
{
    const colour::BandPart p = colour::band_part(dst_x, dst_y, dst_w, dst_h, y0, kRows);
    for (int tid = 0; tid < kThreads; tid++)
        for (int r = 0; r < p.rows; r++)
            for (int c = tid; c < p.cols; c += kThreads)
                colour::convert_item(k, p, r, c, kW, band, band + kBandY, band + kBandY + kBandC);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 4) {
        const int matrix = atoi(argv[2]), full_range = atoi(argv[3]);
        int32_t q[9] = {};
        int y0 = -1;
        if (argc == 5 && !strcmp(argv[1], "coefs")) {
            const int rc = colour::coefs(matrix, full_range, atoi(argv[4]), q, &y0);
            printf("%d", rc);
            for (int i = 0; i < 9; i++)
                printf(" %d", (int)q[i]);
            printf(" %d\n", y0);
            return 0;
        }
        if (!strcmp(argv[1], "pixels") && (argc - 4) % 3 == 0) {
            if (colour::coefs(matrix, full_range, 0, q, &y0) < 0)
                return 1;
            const colour::Coefs k = colour::pack(q, y0);
            for (int i = 4; i < argc; i += 3) {
                const uint32_t w = colour::pixel(k, atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]));
                printf("%u %u %u\n", w & 0xFF, (w >> 8) & 0xFF, w >> 16);
            }
            return 0;
        }
        if (argc == 4 && !strcmp(argv[1], "precision")) {
            Exact e;
            if (colour::coefs(matrix, full_range, 0, q, &y0) < 0 || !exact_map(matrix, full_range, &e))
                return 1;
            const colour::Coefs k = colour::pack(q, y0);
            int worst = 0;
            long differing = 0;
            for (int y = 0; y < 256; y++)
                for (int cb = 0; cb < 256; cb++)
                    for (int cr = 0; cr < 256; cr++) {
                        const uint32_t w = colour::pixel(k, y, cb, cr);
                        const double v[3] = {(double)(y - e.y0), (double)(cb - 128), (double)(cr - 128)};
                        const int got[3] = {(int)(w & 0xFF), (int)((w >> 8) & 0xFF), (int)(w >> 16)};
                        bool differs = false;
                        for (int i = 0; i < 3; i++) {
                            const int want = round_clamp((i ? 128 : 16) + e.m[i][0] * v[0] + e.m[i][1] * v[1] + e.m[i][2] * v[2]);
                            const int d = abs(got[i] - want);
                            worst = d > worst ? d : worst;
                            differs |= d != 0;
                        }
                        differing += differs;
                    }
            printf("%d %ld %d\n", worst, differing, 1 << 24);
            return 0;
        }
        if (argc == 11 && !strcmp(argv[1], "picture")) {
            if (colour::coefs(matrix, full_range, atoi(argv[4]), q, &y0) < 0)
                return 1;
            const colour::Coefs k = colour::pack(q, y0);
            const int dst_x = atoi(argv[5]), dst_y = atoi(argv[6]), dst_w = atoi(argv[7]), dst_h = atoi(argv[8]);
            std::unique_ptr<uint8_t[]> pic(new uint8_t[kFrameBytes]);
            FILE* in = fopen(argv[9], "rb");
            if (!in || fread(pic.get(), 1, kFrameBytes, in) != (size_t)kFrameBytes) {
                fprintf(stderr, "cannot read %d bytes from %s\n", kFrameBytes, argv[9]);
                return 1;
            }
            fclose(in);
            for (int band = 0; band < kImportBands; band++) {
                std::unique_ptr<uint8_t[]> s_out(new uint8_t[kBandBytes]);  // the kernels' LDS band: Y, Cb, Cr
                uint8_t* part[3] = {pic.get() + band * kBandY, pic.get() + kYBytes + band * kBandC, pic.get() + kYBytes + kCBytes + band * kBandC};
                memcpy(s_out.get(), part[0], kBandY);
                memcpy(s_out.get() + kBandY, part[1], kBandC);
                memcpy(s_out.get() + kBandY + kBandC, part[2], kBandC);
                convert_band(k, dst_x, dst_y, dst_w, dst_h, band * kRows, s_out.get());
                memcpy(part[0], s_out.get(), kBandY);
                memcpy(part[1], s_out.get() + kBandY, kBandC);
                memcpy(part[2], s_out.get() + kBandY + kBandC, kBandC);
            }
            FILE* o = fopen(argv[10], "wb");
            if (!o || fwrite(pic.get(), 1, kFrameBytes, o) != (size_t)kFrameBytes) {
                fprintf(stderr, "cannot write %s\n", argv[10]);
                return 1;
            }
            fclose(o);
            return 0;
        }
    }
    fprintf(stderr, "usage: see the head of tests/colour_model_main.cpp\n");
    return 2;
}
