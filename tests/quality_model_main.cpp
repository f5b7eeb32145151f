// TEST: whole efx_compare_pictures calls on the host, with quality_px.h's functions and k_quality's own index arithmetic:
// the twelve bands of an image, a band's block tasks dealt to 192 threads (16 pels x 4 rows each, fetched as 16-byte
// pieces), the block sums staged in a block of the kernel's LDS size, the windows dealt to the threads, the band's six
// sums added into the record.  Every image lives in a heap block of exactly the 101376 bytes the contract lets the kernel
// read, every record in a block of exactly 48 bytes and every macroblock map in one of exactly 264 words, so a sanitizer
// build (-fsanitize=address,undefined: tests/test_quality_model.py) sees every byte the kernel's addressing would touch.
//
//   quality_model_main compare N REF_MAX REF_FILE TEST_FILE RECS_FILE MB_FILE Q_FILE
//        (REF_FILE, TEST_FILE: N images packed; RECS_FILE: 3 uint64 + 3 int64 per image; MB_FILE: 264 uint32 per image;
//         Q_FILE: every window's q as int32, per image 4089 of Y, 989 of Cb, 989 of Cr, row major)
//   quality_model_main window S1 S2 SS S12 [...]   (num, den and q of windows given by their sums, one line each)
//   quality_model_main q16 NUM DEN [...]           (the Q16 quotient, one line each)
//   quality_model_main clamp                       (exit 1 unless clamp4 is min(a, m) on every byte, for every a, m and place)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "quality_px.h"

using namespace efx;

namespace {

// k_quality: one band of one image.  q_out: the image's windows (Y, Cb, Cr), for the test only.
void compare_band(const uint8_t* ref, const uint8_t* test, int ref_max, int band, qpx::Block* stage, uint64_t* sse, int64_t* ssim,
                  uint32_t* mb, int32_t* q_out)
{
    uint32_t out_sse[3] = {0, 0, 0}, out_mb[22] = {};
    int32_t out_ssim[3] = {0, 0, 0};
    for (int tid = 0; tid < qpx::kThreads; tid++) {
        const qpx::BlockTask t = qpx::block_task(band, tid);
        if (!t.valid)
            continue;
        const int width = qpx::plane_width(t.plane);
        const int off = qpx::task_offset(band, t, 0);
        uint32_t va[4][4], vb[4][4];
        for (int r = 0; r < 4; r++) {
            if (qpx::task_offset(band, t, r) != off + r * width)
                abort();
            memcpy(va[r], ref + off + r * width, 16);
            memcpy(vb[r], test + off + r * width, 16);
        }
        uint32_t quad_sse = 0;
        for (int j = 0; j < 4; j++) {
            qpx::Block k{0, 0, 0, 0};
            for (int r = 0; r < 4; r++)
                qpx::add_row(ref_max < 255 ? qpx::clamp4(va[r][j], (uint32_t)ref_max) : va[r][j], vb[r][j], &k);
            stage[qpx::task_stage(t) + j] = k;
            quad_sse += qpx::block_sse(k);
        }
        if (!t.halo) {
            if (t.plane == 0)
                out_mb[t.quad] += quad_sse;
            else
                out_sse[t.plane] += quad_sse;
        }
    }
    const int total = qpx::band_windows(band);
    for (int w = 0; w < total; w++) {
        const qpx::WindowTask wt = qpx::window_task(band, w);
        const qpx::Block* b = stage + qpx::window_stage(wt);
        const int down = qpx::block_cols(wt.plane);
        const int32_t q = qpx::window_q16(b[0], b[1], b[down], b[down + 1]);
        out_ssim[wt.plane] += q;
        const int first = wt.plane == 0 ? 0 : (wt.plane == 1 ? 4089 : 4089 + 989);
        const int row = band * qpx::band_block_rows(wt.plane) + wt.row;
        q_out[first + row * (qpx::block_cols(wt.plane) - 1) + wt.col] = q;
    }
    for (int c = 0; c < 22; c++)
        out_sse[0] += out_mb[c];
    for (int p = 0; p < 3; p++)
        sse[p] += out_sse[p], ssim[p] += out_ssim[p];
    for (int c = 0; c < 22; c++)
        mb[22 * band + c] = out_mb[c];
}

int compare(char** argv)
{
    const int n = atoi(argv[2]);
    const int ref_max = atoi(argv[3]) ? atoi(argv[3]) : 255;
    FILE* fr = fopen(argv[4], "rb");
    FILE* ft = fopen(argv[5], "rb");
    FILE* o_recs = fopen(argv[6], "wb");
    FILE* o_mb = fopen(argv[7], "wb");
    FILE* o_q = fopen(argv[8], "wb");
    if (!fr || !ft || !o_recs || !o_mb || !o_q)
        return 1;
    std::unique_ptr<qpx::Block[]> stage(new qpx::Block[qpx::kStageBlocks]);
    const int nq = 4089 + 2 * 989;
    for (int k = 0; k < n; k++) {
        // operator new[] hands out 16-byte aligned blocks, like the device pointers of the contract
        std::unique_ptr<uint8_t[]> ref(new uint8_t[qpx::kImageBytes]), test(new uint8_t[qpx::kImageBytes]);
        std::unique_ptr<uint64_t[]> rec(new uint64_t[6]);
        std::unique_ptr<uint32_t[]> mb(new uint32_t[264]);
        std::unique_ptr<int32_t[]> q(new int32_t[nq]);
        if (fread(ref.get(), 1, qpx::kImageBytes, fr) != (size_t)qpx::kImageBytes || fread(test.get(), 1, qpx::kImageBytes, ft) != (size_t)qpx::kImageBytes) {
            fprintf(stderr, "cannot read %d images\n", n);
            return 1;
        }
        for (int i = 0; i < nq; i++)
            q[i] = INT32_MIN;  // (every window must be written)
        uint64_t sse[3] = {0, 0, 0};  // k_quality_zero
        int64_t ssim[3] = {0, 0, 0};
        for (int band = 0; band < qpx::kBands; band++)
            compare_band(ref.get(), test.get(), ref_max, band, stage.get(), sse, ssim, mb.get(), q.get());
        for (int p = 0; p < 3; p++)
            rec[p] = sse[p], rec[3 + p] = (uint64_t)ssim[p];
        if (fwrite(rec.get(), 8, 6, o_recs) != 6 || fwrite(mb.get(), 4, 264, o_mb) != 264 || fwrite(q.get(), 4, nq, o_q) != (size_t)nq)
            return 1;
    }
    fclose(fr), fclose(ft);
    return (fclose(o_recs) | fclose(o_mb) | fclose(o_q)) ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 9 && !strcmp(argv[1], "compare"))
        return compare(argv);
    if (argc >= 6 && (argc - 2) % 4 == 0 && !strcmp(argv[1], "window")) {
        for (int i = 2; i < argc; i += 4) {
            int64_t num, den;
            qpx::window((uint32_t)strtoul(argv[i], nullptr, 10), (uint32_t)strtoul(argv[i + 1], nullptr, 10), (uint32_t)strtoul(argv[i + 2], nullptr, 10),
                        (uint32_t)strtoul(argv[i + 3], nullptr, 10), &num, &den);
            printf("%" PRId64 " %" PRId64 " %d\n", num, den, qpx::q16(num, den));
        }
        return 0;
    }
    if (argc >= 4 && (argc - 2) % 2 == 0 && !strcmp(argv[1], "q16")) {
        for (int i = 2; i < argc; i += 2)
            printf("%d\n", qpx::q16(strtoll(argv[i], nullptr, 10), strtoll(argv[i + 1], nullptr, 10)));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "clamp")) {
        for (uint32_t m = 1; m <= 255; m++)
            for (uint32_t a = 0; a <= 255; a++)
                for (int place = 0; place < 4; place++) {
                    uint8_t in[4], want[4];
                    for (int i = 0; i < 4; i++) {
                        in[i] = i == place ? (uint8_t)a : (uint8_t)(a * 7 + 85 * i + 3 * m + 41 * place);
                        want[i] = in[i] < m ? in[i] : (uint8_t)m;
                    }
                    uint32_t word, got;
                    memcpy(&word, in, 4);
                    got = qpx::clamp4(word, m);
                    if (memcmp(&got, want, 4)) {
                        fprintf(stderr, "clamp4(%08x, %u) = %08x\n", word, m, got);
                        return 1;
                    }
                }
        return 0;
    }
    fprintf(stderr, "usage: see the head of tests/quality_model_main.cpp\n");
    return 2;
}
