// TEST: trick_sel.h on the host -- the selection rule of efx_trick_pick as plain numbers for tests/test_trick_model.py, and
// a whole pick with k_trick's own item arithmetic (run_start / locate: runs of 1024 items, 16-byte pieces) on heap blocks
// of exactly the bytes the contract names, so that a sanitizer build (-fsanitize=address,undefined) sees every byte the
// kernel's addressing would touch.
//
//   trick_model_main windows SPEED MAX   for first = 0 .. MAX-1, n = 1 .. MAX-first: int64 count, k0, then per pick of the
//                                        call the call's picture j, its fwd image and its title pick k (all int64, stdout)
//   trick_model_main rwd SPEED MAX       for total = 1 .. MAX: int64 K, then rwd_image(k, K) for k = 0 .. K-1
//   trick_model_main invalid             count() of argument sets that must be refused, one int64 each
//   trick_model_main gather SPEED N_STREAMS TOTAL N [N ...]
//                                        a title of TOTAL pictures per stream offered as calls of N pictures (their sum is
//                                        TOTAL), fwd + rwd, padded strides; compared in the program with a picture-wise
//                                        copy by the placement functions; exit 1 on any difference or a touched pad byte
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "trick_sel.h"

using namespace efx;

namespace {

constexpr size_t kPic = 101376;
constexpr size_t kPad = 48;  // bytes between streams that must keep their fill
constexpr uint8_t kFill = 0xA5;

void put(int64_t v) { fwrite(&v, sizeof v, 1, stdout); }

// one efx_trick_pick call as k_trick performs it: every run, every item of the run
void pick_call(const uint8_t* src, size_t src_stride, uint8_t* fwd, size_t fwd_stride, uint8_t* rwd, size_t rwd_stride, int n_streams,
               int64_t first, int n, int speed, int64_t total)
{
    const int64_t picks = tsel::count(first, n, speed);
    if (picks <= 0)
        return;
    const int64_t k0 = tsel::first_pick(first, speed), K = tsel::total_picks(total, speed);
    const uint64_t pictures = (uint64_t)n_streams * (uint64_t)picks;
    for (uint64_t run = 0; run < tsel::run_count(pictures); run++) {
        const tsel::Run r = tsel::run_start(run, (int)picks);
        for (int local = 0; local < tsel::kRunItems; local++) {
            int s, i, q;
            if (!tsel::locate(r, local, (int)picks, pictures, &s, &i, &q))
                continue;
            const int64_t k = k0 + i, j = tsel::call_picture(k, speed, first);
            uint8_t v[16];
            memcpy(v, src + (size_t)s * src_stride + (size_t)j * kPic + 16 * (size_t)q, 16);
            memcpy(fwd + (size_t)s * fwd_stride + (size_t)tsel::fwd_image(k, k0) * kPic + 16 * (size_t)q, v, 16);
            memcpy(rwd + (size_t)s * rwd_stride + (size_t)tsel::rwd_image(k, K) * kPic + 16 * (size_t)q, v, 16);
        }
    }
}

int gather(int speed, int n_streams, int total, const std::vector<int>& calls)
{
    const int64_t K = tsel::total_picks(total, speed);
    uint32_t lcg = 12345;
    std::vector<uint8_t> title((size_t)n_streams * total * kPic);
    for (auto& b : title)
        b = (uint8_t)((lcg = lcg * 1664525u + 1013904223u) >> 24);
    // the rwd region of the title: exactly n_streams strides less the last pad
    const size_t rwd_stride = (size_t)K * kPic + kPad, rwd_bytes = (size_t)n_streams * rwd_stride - kPad;
    std::unique_ptr<uint8_t[]> rwd(new uint8_t[rwd_bytes]);
    memset(rwd.get(), kFill, rwd_bytes);
    std::vector<uint8_t> fwd_all((size_t)n_streams * K * kPic);  // the calls' fwd picks put together, per stream
    int64_t first = 0, done = 0;
    for (int n : calls) {
        const int64_t picks = tsel::count(first, n, speed);
        // this call's source and fwd region in blocks of exactly their size
        const size_t src_stride = (size_t)n * kPic + kPad, src_bytes = (size_t)n_streams * src_stride - kPad;
        std::unique_ptr<uint8_t[]> src(new uint8_t[src_bytes]);
        memset(src.get(), kFill, src_bytes);
        for (int s = 0; s < n_streams; s++)
            memcpy(src.get() + s * src_stride, title.data() + ((size_t)s * total + first) * kPic, (size_t)n * kPic);
        const size_t fwd_stride = (size_t)picks * kPic + kPad, fwd_bytes = (size_t)n_streams * fwd_stride - kPad;
        std::unique_ptr<uint8_t[]> fwd(new uint8_t[fwd_bytes]);
        memset(fwd.get(), kFill, fwd_bytes);
        pick_call(src.get(), src_stride, fwd.get(), fwd_stride, rwd.get(), rwd_stride, n_streams, first, n, speed, total);
        for (int s = 0; s < n_streams; s++) {
            memcpy(fwd_all.data() + ((size_t)s * K + done) * kPic, fwd.get() + s * fwd_stride, (size_t)picks * kPic);
            if (s + 1 < n_streams)
                for (size_t b = 0; b < kPad; b++)
                    if (fwd[s * fwd_stride + picks * kPic + b] != kFill)
                        return fprintf(stderr, "fwd pad touched\n"), 1;
        }
        first += n;
        done += picks;
    }
    if (first != total || done != K)
        return fprintf(stderr, "calls do not make the title\n"), 1;
    for (int s = 0; s < n_streams; s++)
        for (int64_t k = 0; k < K; k++) {
            const uint8_t* want = title.data() + ((size_t)s * total + (size_t)k * speed) * kPic;
            if (memcmp(fwd_all.data() + ((size_t)s * K + k) * kPic, want, kPic))
                return fprintf(stderr, "fwd stream %d pick %lld differs\n", s, (long long)k), 1;
            if (memcmp(rwd.get() + s * rwd_stride + (size_t)(K - 1 - k) * kPic, want, kPic))
                return fprintf(stderr, "rwd stream %d pick %lld differs\n", s, (long long)k), 1;
        }
    for (int s = 0; s + 1 < n_streams; s++)
        for (size_t b = 0; b < kPad; b++)
            if (rwd[s * rwd_stride + K * kPic + b] != kFill)
                return fprintf(stderr, "rwd pad touched\n"), 1;
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    const std::string mode = argv[1];
    if (mode == "windows" && argc == 4) {
        const int speed = atoi(argv[2]), max = atoi(argv[3]);
        for (int first = 0; first < max; first++)
            for (int n = 1; n <= max - first; n++) {
                const int64_t c = tsel::count(first, n, speed), k0 = tsel::first_pick(first, speed);
                put(c);
                put(k0);
                for (int64_t i = 0; i < c; i++) {
                    put(tsel::call_picture(k0 + i, speed, first));
                    put(tsel::fwd_image(k0 + i, k0));
                    put(k0 + i);
                }
            }
        return 0;
    }
    if (mode == "rwd" && argc == 4) {
        const int speed = atoi(argv[2]), max = atoi(argv[3]);
        for (int total = 1; total <= max; total++) {
            const int64_t K = tsel::total_picks(total, speed);
            put(K);
            for (int64_t k = 0; k < K; k++)
                put(tsel::rwd_image(k, K));
        }
        return 0;
    }
    if (mode == "invalid") {
        put(tsel::count(-1, 5, 15));
        put(tsel::count((int64_t)1 << 40, 5, 15));
        put(tsel::count(0, -1, 15));
        put(tsel::count(0, (int64_t)1 << 31, 15));
        put(tsel::count(0, 5, 0));
        put(tsel::count(0, 5, 256));
        // ... and the largest arguments that are accepted
        put(tsel::count(((int64_t)1 << 40) - 1, INT32_MAX, 1));
        put(tsel::count(((int64_t)1 << 40) - 1, INT32_MAX, 255));
        return 0;
    }
    if (mode == "gather" && argc >= 6) {
        std::vector<int> calls;
        for (int i = 5; i < argc; i++)
            calls.push_back(atoi(argv[i]));
        return gather(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), calls);
    }
    return 2;
}
