// TEST: whole efx_loudness_steps / efx_loudness_gate / efx_pcm_gain calls on the host, with loudness_px.h's functions and
// the kernels' own addressing: waves of 64 steps, per trip 128 bytes of each row staged from 16-byte pieces aligned down
// (a piece that would end behind the call's samples element by element, samples in front of the call from the state), the
// d samples in front of a row fed as zeros, k_loud_state's hand-over, k_loud_gate's two passes with split sums,
// k_pcm_gain's pieces.  Every call's samples live in a heap block of exactly n_samples elements, the state in one of
// exactly its size, the staging buffer has the kernel's size, so a sanitizer build (-fsanitize=address,undefined:
// tests/test_loudness_model.py) sees every element the kernels' addressing would touch.
//
//   loudness_model_main steps RATE C0 .. C9 PCM STEPS STATE N...
//       one stream fed in pieces of N... samples (PCM: the pieces back to back); STEPS receives the 16-byte records of all
//       pieces, STATE the state after the last
//   loudness_model_main gate RATE STEPS N_STEPS ABS_THR TARGET_MS CEILING STATE|- REC     REC receives the 32-byte record
//   loudness_model_main gain G SRC DST N                                                  N samples through apply_gain
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "loudness_px.h"

using namespace efx;

namespace {

struct Piece {
    uint32_t w[4];
};

Piece piece(const loud::Plan& p, const int16_t* src, const int16_t* hist, int v8)
{
    Piece v{};
    if (v8 < -p.hist || (v8 & 7) || v8 >= p.n_samples) {
        fprintf(stderr, "piece %d outside the kernel's bounds\n", v8);
        exit(3);
    }
    if (v8 < 0) {
        memcpy(v.w, hist + p.hist + v8, 16);
    } else if (v8 + 8 <= p.n_samples) {
        memcpy(v.w, src + v8, 16);
    } else {
        for (int i = 0; v8 + i < p.n_samples; i++)
            v.w[i >> 1] |= (uint32_t)(uint16_t)src[v8 + i] << (16 * (i & 1));
    }
    return v;
}

int lo16(uint32_t w) { return (int16_t)(w & 0xFFFF); }
int hi16(uint32_t w) { return (int16_t)(w >> 16); }

// k_loud_steps for one stream, then k_loud_state
void steps_call(const loud::Plan& p, const int16_t* src, int16_t* hist, loud::StepRec* out)
{
    std::unique_ptr<Piece[]> s_rows(new Piece[loud::kLanes * loud::kRowPitch16]);
    const int len = p.runin + p.step;
    const int n_trips = (len + 7 + loud::kChunk - 1) / loud::kChunk;
    for (int t0 = 0; t0 < p.n_new; t0 += loud::kLanes) {
        loud::Lane L[loud::kLanes] = {};
        for (int c = 0; c < n_trips; c++) {
            for (int lane = 0; lane < loud::kLanes; lane++) {
                const int sub = lane >> 3, col = lane & 7;
                for (int k = 0; k < 8; k++) {
                    const int r = 8 * k + sub;
                    const int rs = p.row0 + (t0 + r < p.n_new ? t0 + r : p.n_new - 1) * p.step;
                    const int v8 = (rs & ~7) + loud::kChunk * c + 8 * col;
                    Piece v{};
                    if (t0 + r < p.n_new && v8 < rs + len)
                        v = piece(p, src, hist, v8);
                    s_rows[r * loud::kRowPitch16 + col] = v;
                }
            }
            for (int lane = 0; lane < loud::kLanes && t0 + lane < p.n_new; lane++) {
                const int d = (p.row0 + (t0 + lane) * p.step) & 7;
                for (int q = 0; q < 8; q++) {
                    const Piece v = s_rows[lane * loud::kRowPitch16 + q];
                    const int i0 = loud::kChunk * c + 8 * q - d;
                    for (int j = 0; j < 4; j++) {
                        const int i = i0 + 2 * j;
                        loud::feed(p.k, L[lane], lo16(v.w[j]), i >= 0 && i < len, i >= p.runin && i < len);
                        loud::feed(p.k, L[lane], hi16(v.w[j]), i + 1 >= 0 && i + 1 < len, i + 1 >= p.runin && i + 1 < len);
                    }
                }
            }
        }
        for (int lane = 0; lane < loud::kLanes && t0 + lane < p.n_new; lane++)
            out[t0 + lane] = loud::StepRec{L[lane].energy, L[lane].peak, 0};
    }
    std::vector<int16_t> next((size_t)p.hist);
    for (int k = 0; k < p.hist; k++) {
        const int j = p.n_samples - p.hist + k;
        next[k] = j < 0 ? hist[k + p.n_samples] : src[j];
    }
    memcpy(hist, next.data(), 2 * (size_t)p.hist);
}

// k_loud_gate for one stream: 256 lanes' partial sums, added up at the end
loud::GateRec gate_call(const loud::StepRec* steps, int n_steps, const int16_t* state, int hist, uint64_t abs_thr, uint64_t T,
                        uint32_t C, int step)
{
    const int n_blocks = n_steps >= 4 ? n_steps - 3 : 0;
    auto block = [&](int j) { return steps[j].energy + steps[j + 1].energy + steps[j + 2].energy + steps[j + 3].energy; };
    uint32_t peak = 0;
    for (int j = 0; j < n_steps; j++)
        peak = steps[j].peak > peak ? steps[j].peak : peak;
    if (state)
        for (int k = 0; k < hist; k++)
            peak = loud::abs16(state[k]) > peak ? loud::abs16(state[k]) : peak;
    uint64_t lo = 0, hi = 0, largest = 0;
    uint32_t n_abs = 0;
    for (int tid = 0; tid < 256; tid++) {
        loud::Acc acc{};
        for (int j = tid; j < n_blocks; j += 256) {
            const uint64_t b = block(j);
            largest = b > largest ? b : largest;
            if (b > abs_thr)
                loud::acc_add(acc, b);
        }
        lo += acc.lo, hi += acc.hi, n_abs += acc.n;
    }
    const loud::u128 S_abs = loud::acc_sum(lo, hi);
    uint64_t glo = 0, ghi = 0;
    uint32_t n_gated = 0;
    for (int tid = 0; tid < 256 && n_abs; tid++) {
        loud::Acc acc{};
        for (int j = tid; j < n_blocks; j += 256) {
            const uint64_t b = block(j);
            if (b > abs_thr && loud::rel_pass(b, n_abs, S_abs))
                loud::acc_add(acc, b);
        }
        glo += acc.lo, ghi += acc.hi, n_gated += acc.n;
    }
    loud::GateRec r{};
    r.gated_mean = n_gated ? loud::udiv128(loud::acc_sum(glo, ghi), n_gated) : 0;
    r.max_block = largest;
    r.n_gated = n_gated, r.n_blocks = (uint32_t)n_blocks, r.n_abs = n_abs;
    r.peak = (uint16_t)peak;
    r.gain_q12 = (uint16_t)loud::gain_q12(r.gated_mean, n_gated, peak, T, C, step);
    return r;
}

template <class T>
std::unique_ptr<T[]> read_exact(const char* path, size_t count)
{
    // operator new[] hands out 16-byte aligned blocks, like the device pointers of the contract
    std::unique_ptr<T[]> buf(new T[count ? count : 1]);
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(buf.get(), sizeof(T), count, f) == count;
    if (f)
        fclose(f);
    if (!ok) {
        fprintf(stderr, "cannot read %zu elements from %s\n", count, path);
        exit(1);
    }
    return buf;
}

bool write_file(const char* path, const void* src, size_t bytes)
{
    FILE* f = fopen(path, "wb");
    const bool ok = f && fwrite(src, 1, bytes, f) == bytes;
    if (f)
        fclose(f);
    return ok;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 17 && !strcmp(argv[1], "steps")) {
        const int rate = atoi(argv[2]);
        if (!loud::rate_ok(rate))
            return 2;
        loud::Coefs k{};
        for (int i = 0; i < 10; i++)
            k.c[i] = (int32_t)atol(argv[3 + i]);
        FILE* in = fopen(argv[13], "rb");
        if (!in)
            return 1;
        std::vector<int16_t> hist((size_t)loud::hist_of(rate), 0);
        std::vector<loud::StepRec> all;
        int64_t first = 0;
        for (int a = 16; a < argc; a++) {
            const int n = atoi(argv[a]);
            const loud::Plan p = loud::plan(rate, k, first, n);
            std::unique_ptr<int16_t[]> src(new int16_t[(size_t)n]);
            if (fread(src.get(), 2, (size_t)n, in) != (size_t)n)
                return 1;
            std::unique_ptr<loud::StepRec[]> out(new loud::StepRec[(size_t)p.n_new ? p.n_new : 1]);
            steps_call(p, src.get(), hist.data(), out.get());
            all.insert(all.end(), out.get(), out.get() + p.n_new);
            first += n;
        }
        fclose(in);
        return write_file(argv[14], all.data(), all.size() * sizeof(loud::StepRec)) && write_file(argv[15], hist.data(), 2 * hist.size()) ? 0 : 1;
    }
    if (argc == 10 && !strcmp(argv[1], "gate")) {
        const int rate = atoi(argv[2]), n_steps = atoi(argv[4]);
        if (!loud::rate_ok(rate))
            return 2;
        auto steps = read_exact<loud::StepRec>(argv[3], (size_t)n_steps);
        std::unique_ptr<int16_t[]> state;
        if (strcmp(argv[8], "-"))
            state = read_exact<int16_t>(argv[8], (size_t)loud::hist_of(rate));
        const loud::GateRec r = gate_call(steps.get(), n_steps, state.get(), loud::hist_of(rate), strtoull(argv[5], nullptr, 10),
                                          strtoull(argv[6], nullptr, 10), (uint32_t)strtoul(argv[7], nullptr, 10), loud::step_of(rate));
        static_assert(sizeof(loud::GateRec) == 32 && sizeof(loud::StepRec) == 16, "the records of include/efx.h");
        return write_file(argv[9], &r, sizeof(r)) ? 0 : 1;
    }
    if (argc == 6 && !strcmp(argv[1], "gain")) {
        const int g = atoi(argv[2]), n = atoi(argv[5]);
        auto src = read_exact<int16_t>(argv[3], (size_t)n);
        std::unique_ptr<int16_t[]> dst(new int16_t[(size_t)n ? n : 1]);
        for (int base = 0; base < n; base += 8)  // k_pcm_gain's pieces
            for (int i = base; i < n && i < base + 8; i++)
                dst[i] = (int16_t)loud::apply_gain(src[i], g);
        return write_file(argv[4], dst.get(), 2 * (size_t)n) ? 0 : 1;
    }
    fprintf(stderr, "usage: see the head of tests/loudness_model_main.cpp\n");
    return 2;
}
