// k_sbc_enc.hip -- PCM -> SBC frames for a batch of streams (gfx950): efx_sbc_encode.
//
// The inverse of k_sbc.hip: frames the reference decoder (src/sbc_decoder.cpp) plays -- 8 subbands, mono or dual channel,
// its bit allocation, its amplitude convention.  All arithmetic is sbc_enc_core.h's (host + device, integer), so
// tests/sbc_enc_model_main.cpp writes the same bytes on the host.
//
// FRAME-PARALLEL without a chain: the analysis is an FIR, so frame f needs the PCM of the call up to its last sample and,
// near the start of the call, the 72 samples per channel the state keeps -- every (stream, frame) is independent work.
//   k_sbc_enc        a WAVE per frame, four frames a workgroup:
//                      stage   the frame's samples and the 72 before them, per channel, into LDS (16-byte global loads of
//                              the one contiguous run of PCM that holds them, whatever the layout);
//                      window  a lane owns (block, k): the folded window sum T[k] of the block, ten multiply-adds;
//                      matrix  a lane owns (block, subband): S from the block's eight T, kept in registers;
//                      scale   max |S| over the block axis = xor-shuffles over lane bits 3..5; one lane per subband writes it;
//                      alloc   ONE lane per channel runs the bit allocation, another writes header, scale factors and CRC;
//                      pack    the bit widths are constant inside a frame, so sample (blk, ch, sb) starts at bit
//                              header + blk x sum(bits) + prefix(ch, sb): every lane ORs its quantised samples into the
//                              frame's image in LDS (ds_or, no serial bit writer, no global atomics);
//                      store   the image lies in LDS at the frame's own offset from a 16-byte boundary, so it leaves as
//                              whole aligned 16-byte stores, with byte stores only where a frame starts or ends inside one.
//   k_sbc_enc_state  afterwards, a workgroup per stream: the last 72 samples per channel of (state, call) become the state
//                    -- in a launch of its own, so that no frame of the call can see the new state (k_sbc_finish's reason).
#include <hip/hip_runtime.h>

#include "efx_internal.h"
#include "efx.h"
#include "sbc_enc_core.h"

namespace efx {

namespace {

constexpr int kEncWaves = 4;                                     // frames of a workgroup
constexpr int kEncLine = sbcenc::kHist + sbcenc::kMaxBlocks * 8; // samples of a channel in reach of a frame
constexpr int kEncImageWords = 144;                              // 15 bytes of offset + the largest frame (524), in whole uint4

// x / d for x * d < 65536 (d <= 32, x < 128 here)
__device__ inline uint32_t small_div(uint32_t x, uint32_t inv) { return (x * inv) >> 16; }
__device__ inline uint32_t small_inv(uint32_t d) { return 65536u / d + 1u; }

}  // namespace

// grid = (frame groups, streams), both strided over; block = 256
__global__ __launch_bounds__(256) void k_sbc_enc(SbcEncArgs a)
{
    using namespace sbcenc;
    __shared__ Tables tb;
    __shared__ __attribute__((aligned(16))) int16_t xs_all[kEncWaves][2][kEncLine];
    __shared__ int32_t t_all[kEncWaves][2][kMaxBlocks][8];
    __shared__ __attribute__((aligned(16))) uint32_t image_all[kEncWaves][kEncImageWords];
    __shared__ uint8_t scale_all[kEncWaves][2][8];
    __shared__ uint8_t bits_all[kEncWaves][2][8];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tables);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&tb);
        for (int i = tid; i < (int)(sizeof(Tables) / 4); i += 256)
            dst[i] = src[i];
    }
    int16_t(*xs)[kEncLine] = xs_all[wave];
    int32_t(*tt)[kMaxBlocks][8] = t_all[wave];
    uint32_t* image = image_all[wave];
    uint8_t* image_bytes = reinterpret_cast<uint8_t*>(image);

    const int blocks = a.blocks, channels = a.mode ? 2 : 1, spf = blocks * 8, per_frame = spf * channels;
    const int cells = blocks * 8;                                    // (block, k) and (block, subband) cells of a channel
    const int back = (kHist + spf - 1) / spf;                        // frames before a frame that hold its 72 samples of history
    const uint32_t inv_pf = small_inv((uint32_t)(blocks * channels)), inv_b = small_inv((uint32_t)blocks);
    const uint32_t hdr_bytes = 4 + 4 * (uint32_t)channels;
    const int sb = lane & 7;

    for (int s = blockIdx.y; s < a.n_streams; s += gridDim.y) {
        const int16_t* pcm = a.pcm + (size_t)s * a.pcm_stride;
        const int16_t* state = a.state + (size_t)s * 2 * kHist;
        for (int fg = blockIdx.x; fg < a.n_groups; fg += gridDim.x) {
            const int f = fg * kEncWaves + wave;
            const bool live = f < a.n_frames;  // (a wave without a frame walks the barriers and touches no memory)
            uint8_t* dst = a.frames + (size_t)s * a.frame_stride + (size_t)(live ? f : 0) * a.frame_bytes;
            const uint32_t mis = (uint32_t)((uintptr_t)dst & 15);

            // ---- stage -------------------------------------------------------------------------------------
            for (int i = lane; i < kEncImageWords; i += 64)
                image[i] = 0;
            if (live) {
                const int g0 = max(f - back, 0);
                const int count = (f + 1 - g0) * per_frame;            // PCM values of frames g0 .. f, one contiguous run
                const uintptr_t A = (uintptr_t)(pcm + (size_t)g0 * per_frame);
                const uintptr_t a0 = A & ~(uintptr_t)15;
                const int n_chunks = (int)((A + (uintptr_t)count * 2 - a0 + 15) >> 4);
                for (int ck = lane; ck < n_chunks; ck += 64) {
                    // (an aligned 16 bytes that hold one value of the run lie in that value's page)
                    const uint4 v = *reinterpret_cast<const uint4*>(a0 + (uintptr_t)ck * 16);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    const int first = ((int)(a0 - A) + ck * 16) / 2;    // index in the run of the chunk's first value (exact: both even)
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const int idx = first + e;
                        if (idx < 0 || idx >= count)
                            continue;
                        const uint32_t g = small_div((uint32_t)idx >> 3, inv_pf);     // frame of the run
                        const uint32_t r = (uint32_t)idx - g * (uint32_t)per_frame;  // value of the frame
                        uint32_t c, n;
                        if (a.layout == EFX_PCM_INTERLEAVED) {
                            c = r & (uint32_t)(channels - 1);
                            n = r >> (channels - 1);
                        } else {
                            c = small_div(r >> 3, inv_b);
                            n = r - c * (uint32_t)spf;
                        }
                        const int j = (g0 + (int)g - f) * spf + (int)n;  // place on the frame's own timeline: 0 = its first sample
                        if (j >= -kHist)
                            xs[c][kHist + j] = (int16_t)(w[e >> 1] >> (16 * (e & 1)));
                    }
                }
                // what lies before the call comes from the state: its 72 samples end where the call's first sample begins
                const int before = f * spf;  // samples of the call before the frame (n_frames x samples per frame < 2^31)
                if (before < kHist)
                    for (int i = lane; i < kHist * channels; i += 64) {
                        const int c = i >= kHist ? 1 : 0, p = i - c * kHist;
                        if (before + p - kHist < 0)
                            xs[c][p] = state[c * kHist + before + p];
                    }
            }
            __syncthreads();

            // ---- window: T[k] of every block ---------------------------------------------------------------------
            for (int c = 0; c < channels; c++)
                for (int cell = lane; cell < cells; cell += 64) {
                    const int blk = cell >> 3, k = cell & 7;
                    tt[c][blk][k] = window_term(&xs[c][kHist + blk * 8 + 7], k, tb);
                }
            __syncthreads();

            // ---- matrix, scale factors ---------------------------------------------------------------------------
            int32_t sv[2][2] = {{0, 0}, {0, 0}};
#pragma unroll
            for (int c = 0; c < 2; c++)
                if (c < channels) {
                    uint32_t mx = 0;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const int cell = lane + 64 * h;
                        if (cell < cells) {
                            sv[c][h] = matrix_term(tt[c][cell >> 3], sb, tb);
                            mx = max(mx, abs_s(sv[c][h]));
                        }
                    }
                    mx = max(mx, (uint32_t)__shfl_xor((int)mx, 8));
                    mx = max(mx, (uint32_t)__shfl_xor((int)mx, 16));
                    mx = max(mx, (uint32_t)__shfl_xor((int)mx, 32));
                    if (lane < 8)
                        scale_all[wave][c][lane] = (uint8_t)scale_factor(mx);
                }
            __syncthreads();

            // ---- bit allocation (a lane per channel); header, scale factors and CRC (one lane) --------------------
            if (lane < channels) {
                int b[8];
                bit_allocation(a.frequency, a.allocation, a.bitpool, scale_all[wave][lane], b);
#pragma unroll
                for (int k = 0; k < 8; k++)
                    bits_all[wave][lane][k] = (uint8_t)b[k];
            } else if (lane == 8) {
                // (the image keeps the frame as big-endian words: byte p of the frame is byte 3 - (p & 3) of word p >> 2)
                auto put = [&](uint32_t p, uint32_t v) { image_bytes[((mis + p) & ~3u) | (3u - ((mis + p) & 3u))] = (uint8_t)v; };
                const uint32_t h1 = header_byte1(a.frequency, blocks, a.mode, a.allocation);
                uint32_t crc = crc8_byte(crc8_byte(0x0F, h1), (uint32_t)a.bitpool);
                put(0, 0x9C);
                put(1, h1);
                put(2, (uint32_t)a.bitpool);
                for (int i = 0; i < 4 * channels; i++) {
                    const uint8_t* sc = scale_all[wave][i >> 2];
                    const uint32_t v = (uint32_t)sc[2 * (i & 3)] << 4 | sc[2 * (i & 3) + 1];
                    put(4 + (uint32_t)i, v);
                    crc = crc8_byte(crc, v);
                }
                put(3, crc);
            }
            __syncthreads();

            // ---- quantise and pack -------------------------------------------------------------------------------
            {
                uint32_t per_block = 0, prefix[2] = {0, 0}, my_bits[2] = {0, 0};
#pragma unroll
                for (int c = 0; c < 2; c++)
                    if (c < channels)
#pragma unroll
                        for (int k = 0; k < 8; k++) {
                            const uint32_t b = bits_all[wave][c][k];
                            if (k == sb) {
                                prefix[c] = per_block;
                                my_bits[c] = b;
                            }
                            per_block += b;
                        }
#pragma unroll
                for (int c = 0; c < 2; c++)
                    if (c < channels && my_bits[c]) {
                        const int scale = scale_all[wave][c][sb];
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const int cell = lane + 64 * h;
                            if (cell >= cells)
                                continue;
                            const uint32_t n = my_bits[c], q = quantise(sv[c][h], scale, (int)n);
                            const uint32_t p = (mis + hdr_bytes) * 8 + (uint32_t)(cell >> 3) * per_block + prefix[c];
                            const uint32_t w = p >> 5, end = (p & 31) + n;  // (n <= 16: two words at most)
                            if (end <= 32)
                                atomicOr(&image[w], q << (32 - end));
                            else {
                                atomicOr(&image[w], q >> (end - 32));
                                atomicOr(&image[w + 1], q << (64 - end));
                            }
                        }
                    }
            }
            __syncthreads();

            // ---- store -------------------------------------------------------------------------------------------
            if (live) {
                uint8_t* base = dst - mis;  // 16-byte aligned
                const uint32_t lo = mis, hi = mis + a.frame_bytes;
                for (uint32_t ck = lane; ck * 16 < hi; ck += 64) {
                    const uint4 v = *reinterpret_cast<const uint4*>(image + ck * 4);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    if (ck * 16 >= lo && ck * 16 + 16 <= hi) {
                        *reinterpret_cast<uint4*>(base + ck * 16) = make_uint4(__builtin_bswap32(w[0]), __builtin_bswap32(w[1]),
                                                                               __builtin_bswap32(w[2]), __builtin_bswap32(w[3]));
                    } else {
#pragma unroll
                        for (uint32_t b = 0; b < 16; b++) {
                            const uint32_t p = ck * 16 + b;
                            if (p >= lo && p < hi)
                                base[p] = (uint8_t)(w[b >> 2] >> (24 - 8 * (b & 3)));
                        }
                    }
                }
            }
            __syncthreads();  // (the next frame's staging clears the image and overwrites the samples)
        }
    }
}

// grid = streams (strided over), block = 192: thread (channel, place) moves one sample of the new state
__global__ __launch_bounds__(192) void k_sbc_enc_state(SbcEncArgs a)
{
    using namespace sbcenc;
    const int channels = a.mode ? 2 : 1, spf = a.blocks * 8;
    const int tid = threadIdx.x, c = tid >= kHist ? 1 : 0, p = tid - c * kHist;
    const bool mine = tid < kHist * channels;
    for (int s = blockIdx.x; s < a.n_streams; s += gridDim.x) {
        int16_t* state = const_cast<int16_t*>(a.state) + (size_t)s * 2 * kHist;
        int16_t v = 0;
        if (mine) {
            const long long pos = (long long)a.n_frames * spf - kHist + p;  // on the call's timeline; negative: still the old state's
            if (pos < 0)
                v = state[c * kHist + kHist + (int)pos];
            else {
                const long long g = pos / spf;
                const int n = (int)(pos - g * spf);
                v = a.pcm[(size_t)s * a.pcm_stride + (size_t)g * spf * channels +
                          pcm_index(a.layout == EFX_PCM_INTERLEAVED, channels, spf, c, n)];
            }
        }
        __syncthreads();  // (a call shorter than 72 samples shifts the state in place: every read before any write)
        if (mine)
            state[c * kHist + p] = v;
    }
}

}  // namespace efx
