// Host restatement of k_sbc_enc.hip over espflix_amd/csrc/sbc_enc_core.h (tests/sbc_encode_model.py builds it with g++):
// the decisions the kernel makes, frame by frame, so its bytes are the device's.
//
//   sbc_enc_model PCM N_STREAMS N_FRAMES FREQUENCY BLOCKS MODE ALLOCATION BITPOOL LAYOUT STATE_IN STATE_OUT FRAMES MAXABS
//
// PCM: N_STREAMS x N_FRAMES x BLOCKS x 8 x channels int16; STATE_IN ("-" = fresh encoders) / STATE_OUT: N_STREAMS x 288
// bytes; FRAMES: the frames back to back; MAXABS: per (stream, frame, channel, subband) the largest |S| of the integer
// analysis as a uint32 (S as sbc_enc_core.h keeps it: the halved subband sample x 2^15).
// Every folded window sum and every subband sample is evaluated in 64 bits as well: exit status 3 if one differs from
// the 32-bit value (an overflow).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sbc_enc_core.h"

using namespace efx::sbcenc;

static std::vector<uint8_t> read_file(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path);
        exit(2);
    }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0)
        v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static void write_file(const char* path, const void* p, size_t n)
{
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(2);
    }
    fclose(f);
}

int main(int argc, char** argv)
{
    if (argc != 14) {
        fprintf(stderr, "usage: see the head of tests/sbc_enc_model_main.cpp\n");
        return 2;
    }
    const std::vector<uint8_t> pcm_bytes = read_file(argv[1]);
    const int n_streams = atoi(argv[2]), n_frames = atoi(argv[3]), frequency = atoi(argv[4]), blocks = atoi(argv[5]),
              mode = atoi(argv[6]), allocation = atoi(argv[7]), bitpool = atoi(argv[8]), layout = atoi(argv[9]);
    const int channels = mode ? 2 : 1, spf = blocks * 8;
    const size_t per_stream = (size_t)n_frames * spf * channels;
    if (pcm_bytes.size() != per_stream * n_streams * 2) {
        fprintf(stderr, "PCM holds %zu bytes, %zu expected\n", pcm_bytes.size(), per_stream * n_streams * 2);
        return 2;
    }
    const int16_t* pcm = reinterpret_cast<const int16_t*>(pcm_bytes.data());
    std::vector<int16_t> state((size_t)n_streams * 2 * kHist, 0);
    if (strcmp(argv[10], "-") != 0) {
        const std::vector<uint8_t> s = read_file(argv[10]);
        if (s.size() != state.size() * 2) {
            fprintf(stderr, "bad state size\n");
            return 2;
        }
        memcpy(state.data(), s.data(), s.size());
    }
    Tables T;
    build_tables(&T);
    const uint32_t fb = frame_bytes(blocks, channels, bitpool);
    std::vector<uint8_t> frames((size_t)n_streams * n_frames * fb, 0);
    std::vector<uint32_t> maxabs((size_t)n_streams * n_frames * channels * 8, 0);
    bool overflow = false;

    for (int s = 0; s < n_streams; s++) {
        // the channel's timeline: the state's 72 samples, then the call's
        std::vector<int16_t> line[2];
        for (int c = 0; c < channels; c++) {
            line[c].resize(kHist + (size_t)n_frames * spf);
            for (int i = 0; i < kHist; i++)
                line[c][i] = state[((size_t)s * 2 + c) * kHist + i];
            for (int f = 0; f < n_frames; f++)
                for (int n = 0; n < spf; n++)
                    line[c][kHist + (size_t)f * spf + n] =
                        pcm[s * per_stream + (size_t)f * spf * channels + pcm_index(layout, channels, spf, c, n)];
        }
        for (int f = 0; f < n_frames; f++) {
            int32_t S[2][kMaxBlocks][8];
            uint8_t scale[2][8];
            int bits[2][8];
            for (int c = 0; c < channels; c++) {
                uint32_t mx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int blk = 0; blk < blocks; blk++) {
                    const int16_t* newest = &line[c][kHist + (size_t)f * spf + blk * 8 + 7];
                    int32_t t[8];
                    int64_t t64[8];
                    for (int k = 0; k < 8; k++) {
                        t[k] = window_term(newest, k, T);
                        t64[k] = 0;
                        for (int j = 0; j < 10; j++)
                            t64[k] += (int64_t)T.w[k][j] * newest[-T.tap[k][j]];
                        overflow |= t64[k] != t[k];
                    }
                    for (int sb = 0; sb < 8; sb++) {
                        S[c][blk][sb] = matrix_term(t, sb, T);
                        int64_t s64 = 0;
                        for (int k = 0; k < 8; k++)
                            s64 += ((int64_t)T.m[sb][k] * t64[k]) >> 32;
                        overflow |= s64 != S[c][blk][sb];
                        const uint32_t a = abs_s(S[c][blk][sb]);
                        if (a > mx[sb])
                            mx[sb] = a;
                    }
                }
                for (int sb = 0; sb < 8; sb++) {
                    scale[c][sb] = (uint8_t)scale_factor(mx[sb]);
                    maxabs[(((size_t)s * n_frames + f) * channels + c) * 8 + sb] = mx[sb];
                }
                bit_allocation(frequency, allocation, bitpool, scale[c], bits[c]);
            }
            uint8_t* out = &frames[((size_t)s * n_frames + f) * fb];
            write_header(out, frequency, blocks, mode, allocation, bitpool, scale);
            uint32_t pos = (uint32_t)(4 + 4 * channels) * 8;
            for (int blk = 0; blk < blocks; blk++)
                for (int c = 0; c < channels; c++)
                    for (int sb = 0; sb < 8; sb++) {
                        const int b = bits[c][sb];
                        if (!b)
                            continue;
                        const uint32_t q = quantise(S[c][blk][sb], scale[c][sb], b);
                        for (int i = b - 1; i >= 0; i--, pos++)
                            if ((q >> i) & 1)
                                out[pos >> 3] |= (uint8_t)(0x80 >> (pos & 7));
                    }
            if ((pos + 7) / 8 != fb) {
                fprintf(stderr, "frame %d of stream %d ends at bit %u, %u bytes expected\n", f, s, pos, fb);
                return 4;
            }
        }
        for (int c = 0; c < channels; c++)
            for (int i = 0; i < kHist; i++)
                state[((size_t)s * 2 + c) * kHist + i] = line[c][(size_t)n_frames * spf + i];
    }
    write_file(argv[11], state.data(), state.size() * 2);
    write_file(argv[12], frames.data(), frames.size());
    write_file(argv[13], maxabs.data(), maxabs.size() * 4);
    return overflow ? 3 : 0;
}
