// TEST: conform_sel.h on the host -- the rule of efx_conform_rate as plain numbers for tests/test_conform_model.py, and
// whole calls with k_conform's own item arithmetic (trick_sel.h's run_start / locate: runs of 1024 items, 16-byte pieces;
// the two sources of a run found once, before its items) on heap blocks of exactly the bytes the contract names, so that a
// sanitizer build (-fsanitize=address,undefined) sees every byte the kernel's addressing would touch.
//
//   conform_model_main table IN_NUM IN_DEN CODE MAX   int64 to stdout: accepted (1 / 0); when accepted A, B, then
//                                                     outputs(N) for N = 0 .. MAX, then source(n) for n = 0 ..
//                                                     outputs(MAX) - 1
//   conform_model_main args                           count() / source_of() of argument sets at and beyond the bounds,
//                                                     one int64 each (the list: below)
//   conform_model_main gather IN_NUM IN_DEN CODE N_STREAMS FIRST N [N ...]
//                                                     pictures FIRST .. of a title per stream offered as calls of N
//                                                     pictures, padded strides; compared in the program with a
//                                                     picture-wise copy by source(); exit 1 on any difference, a touched
//                                                     pad byte, or pieces that do not concatenate to the whole
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "conform_sel.h"
#include "trick_sel.h"

using namespace efx;

namespace {

constexpr size_t kPic = 101376;
constexpr size_t kPad = 48;  // bytes between streams that must keep their fill
constexpr uint8_t kFill = 0xA5;

void put(int64_t v) { fwrite(&v, sizeof v, 1, stdout); }

// one efx_conform_rate call as k_conform performs it: every run, every item of the run
void conform_call(const uint8_t* src, size_t src_stride, uint8_t* dst, size_t dst_stride, int n_streams, const csel::Ratio& ratio,
                  int64_t first, int64_t n)
{
    const int64_t n0 = csel::outputs(ratio, first), n_out = csel::outputs(ratio, first + n) - n0;
    if (n_out <= 0)
        return;
    const uint64_t pictures = (uint64_t)n_streams * (uint64_t)n_out;
    for (uint64_t run = 0; run < tsel::run_count(pictures); run++) {
        const tsel::Run r = tsel::run_start(run, (int)n_out);
        const int i1 = r.i0 + 1 == n_out ? 0 : r.i0 + 1;
        const int64_t j0 = csel::source(ratio, n0 + r.i0) - first, j1 = csel::source(ratio, n0 + i1) - first;
        for (int local = 0; local < tsel::kRunItems; local++) {
            int s, i, q;
            if (!tsel::locate(r, local, (int)n_out, pictures, &s, &i, &q))
                continue;
            const int64_t j = i == r.i0 && s == r.s0 ? j0 : j1;
            uint8_t v[16];
            memcpy(v, src + (size_t)s * src_stride + (size_t)j * kPic + 16 * (size_t)q, 16);
            memcpy(dst + (size_t)s * dst_stride + (size_t)i * kPic + 16 * (size_t)q, v, 16);
        }
    }
}

// picture t of stream s of the title: its bytes from its numbers, so that a title near 2^31 needs no memory
void fill_picture(uint8_t* p, int s, int64_t t)
{
    uint32_t lcg = (uint32_t)(t * 2654435761u) ^ (uint32_t)(s * 40503u + 1);
    for (size_t b = 0; b < kPic; b += 4) {
        lcg = lcg * 1664525u + 1013904223u;
        memcpy(p + b, &lcg, 4);
    }
}

int gather(const csel::Ratio& ratio, int n_streams, int64_t first0, const std::vector<int>& calls)
{
    std::vector<uint8_t> want(kPic);
    int64_t first = first0, next_out = csel::outputs(ratio, first0);
    for (int n : calls) {
        const int64_t n0 = csel::outputs(ratio, first), n_out = csel::outputs(ratio, first + n) - n0;
        if (n0 != next_out)
            return fprintf(stderr, "pieces do not concatenate\n"), 1;
        // this call's source and destination in blocks of exactly their size
        const size_t src_stride = (size_t)n * kPic + kPad, src_bytes = (size_t)n_streams * src_stride - kPad;
        std::unique_ptr<uint8_t[]> src(new uint8_t[src_bytes]);
        memset(src.get(), kFill, src_bytes);
        for (int s = 0; s < n_streams; s++)
            for (int j = 0; j < n; j++)
                fill_picture(src.get() + s * src_stride + (size_t)j * kPic, s, first + j);
        const size_t dst_stride = (size_t)n_out * kPic + kPad, dst_bytes = (size_t)n_streams * dst_stride - kPad;
        std::unique_ptr<uint8_t[]> dst(new uint8_t[dst_bytes ? dst_bytes : 1]);
        memset(dst.get(), kFill, dst_bytes);
        conform_call(src.get(), src_stride, dst.get(), dst_stride, n_streams, ratio, first, n);
        for (int s = 0; s < n_streams; s++) {
            for (int64_t m = 0; m < n_out; m++) {
                const int64_t t = csel::source(ratio, n0 + m);
                if (t < first || t >= first + n)
                    return fprintf(stderr, "output %lld: source %lld outside the call\n", (long long)(n0 + m), (long long)t), 1;
                fill_picture(want.data(), s, t);
                if (memcmp(dst.get() + s * dst_stride + (size_t)m * kPic, want.data(), kPic))
                    return fprintf(stderr, "stream %d output %lld differs\n", s, (long long)(n0 + m)), 1;
            }
            if (s + 1 < n_streams)
                for (size_t b = 0; b < kPad; b++)
                    if (dst[s * dst_stride + n_out * kPic + b] != kFill)
                        return fprintf(stderr, "pad touched\n"), 1;
        }
        first += n;
        next_out = n0 + n_out;
    }
    if (next_out != csel::outputs(ratio, first))
        return fprintf(stderr, "pieces do not make the whole\n"), 1;
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    const std::string mode = argv[1];
    if (mode == "table" && argc == 6) {
        csel::Ratio r;
        const int64_t max = atoll(argv[5]);
        if (!csel::ratio(atoll(argv[2]), atoll(argv[3]), atoi(argv[4]), &r)) {
            put(0);
            return 0;
        }
        put(1);
        put(r.A);
        put(r.B);
        for (int64_t N = 0; N <= max; N++)
            put(csel::outputs(r, N));
        for (int64_t n = 0; n < csel::outputs(r, max); n++)
            put(csel::source(r, n));
        return 0;
    }
    if (mode == "args") {
        const int64_t top = INT32_MAX;
        // refused: 0 .. 12
        put(csel::count(0, 1, 4, 0, 5));
        put(csel::count(25, 0, 4, 0, 5));
        put(csel::count((int64_t)1 << 31, 1, 4, 0, 5));
        put(csel::count(25, 1, 0, 0, 5));
        put(csel::count(25, 1, 9, 0, 5));
        put(csel::count(25, 1, 4, -1, 5));
        put(csel::count(25, 1, 4, 0, -1));
        put(csel::count(25, 1, 4, top, 1));                    // first_picture + n_pictures above 2^31 - 1
        put(csel::count(25, 1, 8, top - 1, 1));                // ... within, but the last output's index above it
        put(csel::count(2147483647, 17895698, 8, 0, 5));       // B = 2^31 + 112
        put(csel::count(1537, 1, 2, 0, 5));                    // 1537 : 24 is above 64
        put(csel::count(1, 3, 2, 0, 5));                       // 24 : 1/3 = 72
        put(csel::source_of(25, 1, 4, top + 1));
        // accepted: 13 ..
        put(csel::count(1536, 1, 2, 0, 128));                  // exactly 64 : 1 down: 2 outputs
        put(csel::count(3, 8, 2, 0, 2));                       // exactly 1 : 64 up: 128 outputs
        // the largest first_picture with A and B near 2^31: A = 2^31 - 1 (prime), B = 2^31 - 128
        put(csel::count(2147483647, 17895696, 8, top - 3, 3));
        put(csel::source_of(2147483647, 17895696, 8, csel::count(2147483647, 17895696, 8, 0, top) - 1));
        put(csel::count(2147483647, 17895696, 8, 0, top));
        put(csel::source_of(25, 1, 4, top));
        put(csel::source_of(2147483647, 17895696, 8, top));
        return 0;
    }
    if (mode == "gather" && argc >= 8) {
        csel::Ratio r;
        if (!csel::ratio(atoll(argv[2]), atoll(argv[3]), atoi(argv[4]), &r))
            return 2;
        std::vector<int> calls;
        for (int i = 7; i < argc; i++)
            calls.push_back(atoi(argv[i]));
        return gather(r, atoi(argv[5]), atoll(argv[6]), calls);
    }
    return 2;
}
