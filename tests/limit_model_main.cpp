// limit_model_main.cpp -- espflix_amd/csrc/limit_px.h on the host: whole efx_limit_peaks / efx_pcm_limit calls for one stream,
// written serially and straight from the rule (W^2 work per node), and the exhaustive checks of the header's quotients.
// Built and run by tests/test_limit_model.py, which holds the results against the NumPy model (tests/limit_model.py).
//
//   peaks  RATE SRC DST                                      p of every block of the int16 file SRC as uint16
//   limit  RATE H G C FIRST PEAKS_FIRST SRC PEAKS DST GAINS  the piece SRC that begins at stream sample FIRST, with the row
//                                                            PEAKS (uint16; "-": SRC's own peaks, PEAKS_FIRST 0); y and g
//   gain   MEAN N_GATED T STEP                               prints stream_gain_q12
//   capped MEAN N_GATED PEAK T C STEP                        prints gain_q12, the record's capped gain (loudness_px.h)
//   quotients                                                div_bk over every numerator of the three block lengths,
//                                                            required() against 64-bit division, peak_of over all pairs
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "limit_px.h"

using namespace efx;

template <class T>
static std::vector<T> read_file(const char* path)
{
    std::vector<T> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path);
        exit(2);
    }
    T buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(T), 4096, f)) > 0)
        v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

template <class T>
static void write_file(const char* path, const std::vector<T>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(2);
    }
    fclose(f);
}

static int quotients()
{
    for (int bk : {16, 32, 48}) {
        const limit::DivBk d = limit::div_of(bk);
        const uint32_t top = 32767u * (uint32_t)bk;  // a0 (Bk - t) + a1 t <= 32767 Bk
        for (uint32_t n = 0; n <= top + 4096; n++)
            if (limit::div_bk(n, d) != n / (uint32_t)bk) {
                fprintf(stderr, "div_bk(%u, %d)\n", n, bk);
                return 1;
            }
        // the tile's block of a piece: floor(8 k / Bk), k below 256 Bk / 8
        for (uint32_t k = 0; k < 256u * (uint32_t)bk / 8; k++)
            if (limit::div_bk(8 * k, d) != 8 * k / (uint32_t)bk)
                return 1;
        // the numerator of sample t + i from that of sample t by i steps of a1 - a0 modulo 2^32
        for (uint32_t a0 : {0u, 1u, 4096u, 32767u})
            for (uint32_t a1 : {0u, 1u, 4095u, 32767u})
                for (int t = 0; t + 8 <= bk; t += 8)
                    for (int i = 0; i < 8; i++)
                        if (limit::lerp_num(a0, a1, bk, t) + (uint32_t)i * (a1 - a0) != limit::lerp_num(a0, a1, bk, t + i))
                            return 1;
    }
    for (uint32_t C : {1u, 2u, 255u, 4096u, 29204u, 32766u, 32767u})
        for (uint32_t p = 1; p <= 32768; p++)
            for (uint32_t G : {1u, 4096u, 32767u}) {
                const uint64_t cap = (uint64_t)4096 * C / p;
                if (limit::required(p, G, C) != (cap < G ? cap : G) || (uint64_t)limit::required(p, G, C) * p > (uint64_t)4096 * C)
                    return 1;
            }
    for (int W = 3; W <= 129; W += 2)
        for (uint32_t s = 0; s <= (uint32_t)W * 32767u; s += (s < 1000 || s + 1000 > (uint32_t)W * 32767u) ? 1 : 997)
            if (limit::average(s, (uint32_t)W) != (uint32_t)((uint64_t)s / (uint64_t)W))
                return 1;
    for (int mx = -32768; mx <= 32767; mx += 1)
        for (int mn : {-32768, -32767, -1, 0, 1, 32767})
            if (mn <= mx) {
                const uint32_t want = (uint32_t)std::max(std::abs(mx), std::abs(mn));
                if (limit::peak_of(mx, mn) != want)
                    return 1;
            }
    puts("ok");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "quotients"))
        return quotients();
    if (argc == 6 && !strcmp(argv[1], "gain")) {
        printf("%d\n", loud::stream_gain_q12(strtoull(argv[2], 0, 10), (uint32_t)strtoul(argv[3], 0, 10), strtoull(argv[4], 0, 10), atoi(argv[5])));
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "capped")) {
        printf("%d\n", loud::gain_q12(strtoull(argv[2], 0, 10), (uint32_t)strtoul(argv[3], 0, 10), (uint32_t)strtoul(argv[4], 0, 10),
                                      strtoull(argv[5], 0, 10), (uint32_t)strtoul(argv[6], 0, 10), atoi(argv[7])));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "peaks")) {
        const int bk = limit::block_of(atoi(argv[2]));
        const std::vector<int16_t> x = read_file<int16_t>(argv[3]);
        std::vector<uint16_t> p((x.size() + bk - 1) / bk);
        limit::host_peaks(x.data(), (int64_t)x.size(), bk, p.data());
        write_file(argv[4], p);
        return 0;
    }
    if (argc == 12 && !strcmp(argv[1], "limit")) {
        const int bk = limit::block_of(atoi(argv[2])), H = atoi(argv[3]);
        const uint32_t G = (uint32_t)atoi(argv[4]), C = (uint32_t)atoi(argv[5]);
        const int64_t first = atoll(argv[6]);
        int64_t peaks_first = atoll(argv[7]);
        const std::vector<int16_t> x = read_file<int16_t>(argv[8]);
        std::vector<uint16_t> p;
        if (!strcmp(argv[9], "-")) {
            p.resize((x.size() + bk - 1) / bk);
            limit::host_peaks(x.data(), (int64_t)x.size(), bk, p.data());
            peaks_first = 0;
        } else {
            p = read_file<uint16_t>(argv[9]);
        }
        std::vector<int16_t> y(x.size());
        std::vector<uint16_t> g(x.size());
        limit::host_limit(x.data(), (int64_t)x.size(), first, bk, p.data(), peaks_first, (int)p.size(), H, G, C, y.data(), g.data());
        write_file(argv[10], y);
        write_file(argv[11], g);
        return 0;
    }
    fprintf(stderr, "usage: see the head of tests/limit_model_main.cpp\n");
    return 2;
}
