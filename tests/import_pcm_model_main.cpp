// TEST: whole efx_import_pcm calls on the host, with import_pcm.h's functions and k_import_pcm's own addressing: the tiles
// of 1024 outputs, a tile's input span staged as mixed samples from 16-byte pieces aligned down inside the stream's
// n_in x channels elements (a piece that would end behind them element by element), the frames in front of the call from
// the history, k_import_pcm_state's hand-over.  Every call's source lives in a heap block of exactly n_in x channels
// elements, its output in one of exactly the call's output count, the staging buffers have the kernel's sizes, so a
// sanitizer build (-fsanitize=address,undefined: tests/test_import_pcm_model.py) sees every element the kernel's
// addressing would touch.
//
//   import_pcm_model_main run TABLE R O CHANNELS LAYOUT FIRST_IN W0 .. W7 SRC DST STATE N_IN...
//       one stream fed in pieces of N_IN... frames (SRC: the pieces' elements back to back, each piece in LAYOUT; TABLE:
//       16 P + 1 int32); DST receives the output samples of all pieces, STATE the 256 bytes of state after the last
//   import_pcm_model_main counts R O FIRST_IN N_IN      prints "out_samples delay"
//   import_pcm_model_main time TABLE R O CHANNELS N_IN REPS    prints the seconds of REPS calls of one stream on this core
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "import_pcm.h"

using namespace efx;

namespace {

void gather(const ipcm::Plan& p, const int16_t* src, int ea, int eb, int total, int plane, int plane_base, int32_t* acc, int s_lo)
{
    if (ea >= eb)
        return;
    for (int k = ea >> 3; k <= (eb - 1) >> 3; k++) {
        const int base = 8 * k;
        int16_t x[8] = {};
        if (base + 8 <= total)
            memcpy(x, src + base, 16);
        else
            for (int i = 0; base + i < total; i++)
                x[i] = src[base + i];
        int f, c;
        if (plane < 0) {
            f = ipcm::frame_of(p, base);
            c = base - f * p.channels;
        } else {
            f = base - plane_base;
            c = plane;
        }
        for (int i = 0; i < 8; i++) {
            const int e = base + i;
            if (e >= ea && e < eb)
                acc[f - s_lo] += p.w[c] * (int)x[i];
            if (plane < 0) {
                if (++c == p.channels)
                    c = 0, f++;
            } else {
                f++;
            }
        }
    }
}

// k_import_pcm for one stream, then k_import_pcm_state
void call(const ipcm::Plan& p, const int32_t* T, const int16_t* src, int16_t* hist, int16_t* dst)
{
    std::unique_ptr<int32_t[]> s_acc(new int32_t[ipcm::kSpanMax]);
    std::unique_ptr<int16_t[]> s_mix(new int16_t[ipcm::kSpanMax]);
    const int total = p.n_in * p.channels;
    const int n_tiles = (p.n_out + ipcm::kTile - 1) / ipcm::kTile;
    for (int tile = 0; tile < n_tiles; tile++) {
        const int t_a = tile * ipcm::kTile, t_b = (t_a + ipcm::kTile < p.n_out ? t_a + ipcm::kTile : p.n_out) - 1;
        int s_lo, s_hi, ph;
        if (p.equal) {
            s_lo = t_a, s_hi = t_b;
        } else {
            s_lo = ipcm::position(p, t_a, &ph) - 2 * p.W + 1;
            s_hi = ipcm::position(p, t_b, &ph);
        }
        const int len = s_hi - s_lo + 1;
        if (len > ipcm::kSpanMax || s_lo < -ipcm::kHist || s_hi >= p.n_in) {
            fprintf(stderr, "span [%d, %d] outside the kernel's bounds\n", s_lo, s_hi);
            exit(3);
        }
        for (int i = 0; i < len; i++)
            s_acc[i] = 0;
        const int fa = s_lo > 0 ? s_lo : 0, fb = s_hi + 1;
        if (p.layout == ipcm::kLayoutInterleaved || p.channels == 1) {
            gather(p, src, fa * p.channels, fb * p.channels, total, -1, 0, s_acc.get(), s_lo);
        } else {
            for (int c = 0; c < p.channels; c++)
                gather(p, src, c * p.n_in + fa, c * p.n_in + fb, total, c, c * p.n_in, s_acc.get(), s_lo);
        }
        for (int i = 0; i < len; i++) {
            const int j = s_lo + i;
            s_mix[i] = j < 0 ? hist[ipcm::kHist + j] : (int16_t)ipcm::mix_round(s_acc[i]);
        }
        for (int t = t_a; t <= t_b; t++) {
            if (p.equal) {
                dst[t] = s_mix[t - s_lo];
            } else {
                const int newest = ipcm::position(p, t, &ph);
                dst[t] = (int16_t)ipcm::output(p, T, s_mix.get() + (newest - s_lo), ph);
            }
        }
    }
    if (p.equal)
        return;
    int16_t next[ipcm::kStateBytes / 2] = {};
    for (int k = 0; k < ipcm::kHist; k++) {
        const int j = p.n_in - ipcm::kHist + k;
        if (j < 0) {
            next[k] = hist[k + p.n_in];
        } else {
            int32_t sum = 0;
            for (int c = 0; c < p.channels; c++)
                sum += p.w[c] * (int)src[p.layout == ipcm::kLayoutInterleaved ? (size_t)j * p.channels + c : (size_t)c * p.n_in + j];
            next[k] = (int16_t)ipcm::mix_round(sum);
        }
    }
    memcpy(hist, next, sizeof(next));
}

bool read_file(const char* path, void* dst, size_t bytes)
{
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(dst, 1, bytes, f) == bytes;
    if (f)
        fclose(f);
    if (!ok)
        fprintf(stderr, "cannot read %zu bytes from %s\n", bytes, path);
    return ok;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 6 && !strcmp(argv[1], "counts")) {
        const int r = atoi(argv[2]), o = atoi(argv[3]);
        printf("%lld %d\n", (long long)ipcm::out_samples(r, o, atoll(argv[4]), atoll(argv[5])), ipcm::delay(r, o));
        return 0;
    }
    std::unique_ptr<int32_t[]> T(new int32_t[ipcm::kTableLen]);
    if (argc == 8 && !strcmp(argv[1], "time")) {
        if (!read_file(argv[2], T.get(), ipcm::kTableLen * sizeof(int32_t)))
            return 1;
        const int r = atoi(argv[3]), o = atoi(argv[4]), ch = atoi(argv[5]), n_in = atoi(argv[6]), reps = atoi(argv[7]);
        const int mix[8] = {};
        const ipcm::Plan p = ipcm::plan(r, o, ch, ipcm::kLayoutInterleaved, mix, 0, n_in);
        std::vector<int16_t> src((size_t)n_in * ch), dst((size_t)p.n_out + 1);
        uint32_t seed = 1;
        for (auto& v : src)
            v = (int16_t)((seed = seed * 1664525u + 1013904223u) >> 16);
        int16_t hist[ipcm::kStateBytes / 2] = {};
        const auto t0 = std::chrono::steady_clock::now();
        long long check = 0;
        for (int i = 0; i < reps; i++) {
            call(p, T.get(), src.data(), hist, dst.data());
            check += dst[p.n_out / 2];
        }
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%.6f %lld\n", s, check);
        return 0;
    }
    if (argc < 20 || strcmp(argv[1], "run")) {
        fprintf(stderr, "usage: see the head of tests/import_pcm_model_main.cpp\n");
        return 2;
    }
    if (!read_file(argv[2], T.get(), ipcm::kTableLen * sizeof(int32_t)))
        return 1;
    const int r = atoi(argv[3]), o = atoi(argv[4]), ch = atoi(argv[5]), layout = atoi(argv[6]);
    int64_t first_in = atoll(argv[7]);
    int mix[8];
    for (int c = 0; c < 8; c++)
        mix[c] = atoi(argv[8 + c]);
    FILE* in = fopen(argv[16], "rb");
    FILE* out = fopen(argv[17], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open %s / %s\n", argv[16], argv[17]);
        return 1;
    }
    int16_t hist[ipcm::kStateBytes / 2] = {};
    for (int a = 19; a < argc; a++) {
        const int n_in = atoi(argv[a]);
        const ipcm::Plan p = ipcm::plan(r, o, ch, layout, mix, first_in, n_in);
        // operator new[] hands out 16-byte aligned blocks, like the device pointers of the contract
        std::unique_ptr<int16_t[]> src(new int16_t[(size_t)n_in * ch]), dst(new int16_t[(size_t)p.n_out]);
        if (fread(src.get(), 2, (size_t)n_in * ch, in) != (size_t)n_in * ch) {
            fprintf(stderr, "%s is too short\n", argv[16]);
            return 1;
        }
        call(p, T.get(), src.get(), hist, dst.get());
        if (fwrite(dst.get(), 2, (size_t)p.n_out, out) != (size_t)p.n_out)
            return 1;
        first_in += n_in;
    }
    fclose(in);
    fclose(out);
    FILE* st = fopen(argv[18], "wb");
    if (!st || fwrite(hist, 1, sizeof(hist), st) != sizeof(hist))
        return 1;
    fclose(st);
    return 0;
}
