// k_encode.hip -- batched MPEG-1 I/P encoder (efx_encode): every stream advances one picture per pair of launches.
//
//   k_enc_begin   one lane per stream: fresh streams get their state reset, every stream its per-call output counters
//   k_enc_cut     scene cuts only (efx_encode_set_scene_cut), before everything else of a picture: one wave per (stream,
//                 macroblock row) decimates the row's source luma 4 x 4 into the stream's decimated picture and measures
//                 its 22 macroblocks against the previous decimated source picture (enc_cut.h)
//   k_enc_aq      adaptive quantisation only (efx_encode_set_adaptive_quant), ahead of the others: one wave per (stream,
//                 macroblock row) measures the spatial activity of the row's 22 macroblocks on the source luma (enc_aq.h)
//   k_enc_act     efx_encode_rc only, before every k_enc_rows: one wave per (stream, macroblock row) sums the activity of the
//                 row's 22 macroblocks -- the luma's deviation from its own mean, and the smaller of that and the SAD
//                 against the previous reconstruction at the same place -- with v_sad_u8 on whole 352-byte lines
//   k_enc_rows    (k_enc_rows_t<false>; <true> with adaptive quantisation) one wave per (stream, macroblock row): for
//                 each of the row's 22 macroblocks, full-pel search over the
//                 previous reconstruction staged in LDS (v_sad_u8, one candidate vector per lane), the 8 half-pel
//                 neighbours of the best one, the intra / inter decision, then transform, quantisation and reconstruction
//                 with one lane per block (enc_core.h).  The levels stay in LDS; at the end of the row one lane codes the
//                 slice into the stream's slice scratch.  Rows are independent: reconstruction does not depend on the
//                 coding order (a skipped macroblock reconstructs like "motion compensated, not coded" with vector 0).
//   k_enc_pack    one workgroup per stream: picture headers, then the picture's slices (ES) or its PES in 188-byte
//                 packets (TS) appended to the stream's output region, or EFX_ENCODE_FULL when it does not fit
//
//
// efx_encode_rc: every wave of k_enc_rows adds the twelve row sums of its stream in row order and evaluates
// enc::rate_decide (enc_rate.h), a pure function of the stream's state and those sums, so all twelve arrive at the same
// quantiser; k_enc_pack evaluates it once more, then applies the buffer model to the bytes it wrote.  The model's gain is
// the picture's own: bitrate x the ticks from its PTS to the next picture's (rate_params).
//
// Scene cuts: every wave of k_enc_rows, and k_enc_pack, adds the twelve row sums of k_enc_cut in row order and evaluates
// enc::cut_picture_type (enc_cut.h), a pure function of the stream's state and those sums, so a stream's picture has one
// type in every wave -- and the streams of one launch need not have the same.
//
// Adaptive quantisation: every wave of k_enc_rows adds the twelve row sums of k_enc_aq in row order, forms the picture's
// average activity and gives each of its 22 macroblocks the quantiser of enc::aq_mb_quant (enc_aq.h) around the
// picture's quantiser -- the fixed one, or the controller's, which never sees the macroblocks' own.
//
// Every store is a vector store (global / LDS); the only serial part is the bit writer of a slice.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "enc_core.h"

namespace efx {

__global__ void k_enc_begin(EncArgs a)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_streams)
        return;
    EncState S = a.st[s];
    if (!a.cont) {
        S.pictures = 0;
        S.cc = 0;
        S.cur = 0;
        S.full = 0;
        S.g = 0;
        S.first_pts = a.first_pts;
        enc::rate_reset(&S.rate, a.rate);  // (not read without rate control)
    }
    S.out_len = 0;
    S.status = S.full ? EFX_ENCODE_FULL : 0u;
    a.st[s] = S;
    a.len[s] = 0;
    a.status[s] = S.status;
}

__device__ inline uint32_t wave_min(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1)
        v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
    return v;
}

__device__ inline int wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// 4-lane group sum: lanes 4 m .. 4 m + 3 hold the four words of macroblock m's line
__device__ inline uint32_t quad_sum(uint32_t v)
{
    v += (uint32_t)__shfl_xor((int)v, 1, 64);
    v += (uint32_t)__shfl_xor((int)v, 2, 64);
    return v;
}

// Activity of one macroblock row.  A luma line is 88 words: lane l takes word l of each of the 16 lines, lanes 0 .. 23
// word 64 + l as well, so every line is read whole, in two coalesced loads.  Sums of bytes, deviations and differences are
// v_sad_u8 on the packed words; integer adds only, so the order of the reduction does not show in the result.
__global__ __launch_bounds__(64) void k_enc_act(EncArgs a)
{
    using namespace enc;
    const int row = blockIdx.x % kMbRows, s = blockIdx.x / kMbRows, lane = threadIdx.x;
    const EncState S = a.st[s];
    const bool has_ref = S.pictures != 0, tail = lane < kW / 4 - 64;
    const size_t line0 = (size_t)row * 16 * kW;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.src + (size_t)s * a.src_stride + (size_t)a.picture * kPicBytes + line0);
    const uint32_t* ref = reinterpret_cast<const uint32_t*>(a.pics + ((size_t)s * 2 + S.cur) * kPicBytes + line0);
    uint32_t c0[16], c1[16], sum0 = 0, sum1 = 0;
    for (int y = 0; y < 16; y++) {
        c0[y] = src[y * (kW / 4) + lane];
        c1[y] = tail ? src[y * (kW / 4) + 64 + lane] : 0u;
        sum0 = __builtin_amdgcn_sad_u8(c0[y], 0u, sum0);
        sum1 = __builtin_amdgcn_sad_u8(c1[y], 0u, sum1);
    }
    const uint32_t m0 = ((quad_sum(sum0) + 128) >> 8) * 0x01010101u, m1 = ((quad_sum(sum1) + 128) >> 8) * 0x01010101u;
    uint32_t dev0 = 0, dev1 = 0, sad0 = 0, sad1 = 0;
    for (int y = 0; y < 16; y++) {
        dev0 = __builtin_amdgcn_sad_u8(c0[y], m0, dev0);
        dev1 = __builtin_amdgcn_sad_u8(c1[y], m1, dev1);
        if (has_ref) {
            sad0 = __builtin_amdgcn_sad_u8(c0[y], ref[y * (kW / 4) + lane], sad0);
            if (tail)
                sad1 = __builtin_amdgcn_sad_u8(c1[y], ref[y * (kW / 4) + 64 + lane], sad1);
        }
    }
    dev0 = quad_sum(dev0);
    dev1 = quad_sum(dev1);
    sad0 = quad_sum(sad0);
    sad1 = quad_sum(sad1);
    const bool lead = (lane & 3) == 0;  // one lane per macroblock: 16 in the first set of words, 6 in the second
    const uint32_t i0 = lead ? dev0 : 0u, i1 = lead && tail ? dev1 : 0u;
    const uint32_t p0 = has_ref ? min(i0, sad0) : i0, p1 = has_ref ? min(i1, sad1) : i1;
    const int act_i = wave_sum((int)(i0 + i1)), act_p = wave_sum((int)(p0 + p1));
    if (lane == 0) {
        uint2 w;
        w.x = (uint32_t)act_i;
        w.y = (uint32_t)act_p;
        *reinterpret_cast<uint2*>(a.act + ((size_t)s * kMbRows + row) * 2) = w;
    }
}

// Spatial activity of one macroblock row (enc_aq.h).  The row's 16 luma lines are read as k_enc_act reads them.  An
// 8 x 8 block is two words of eight lines: lines 0 .. 7 and 8 .. 15 are summed separately, the lanes of a pair (2 k,
// 2 k + 1) added for a block's sum and deviation, then the minimum taken over the two halves and across the quad's two
// pairs.  Lane 4 m holds macroblock m's (lanes 0 .. 23 macroblock 16 + m's as well).
__global__ __launch_bounds__(64) void k_enc_aq(EncArgs a)
{
    using namespace enc;
    const int row = blockIdx.x % kMbRows, s = blockIdx.x / kMbRows, lane = threadIdx.x;
    const bool tail = lane < kW / 4 - 64;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.src + (size_t)s * a.src_stride + (size_t)a.picture * kPicBytes +
                                                            (size_t)row * 16 * kW);
    uint32_t c0[16], c1[16];
    for (int y = 0; y < 16; y++) {
        c0[y] = src[y * (kW / 4) + lane];
        c1[y] = tail ? src[y * (kW / 4) + 64 + lane] : 0u;
    }
    uint32_t best0 = 0xFFFFFFFFu, best1 = 0xFFFFFFFFu;
    for (int half = 0; half < 2; half++) {
        uint32_t sum0 = 0, sum1 = 0;
        for (int y = 8 * half; y < 8 * half + 8; y++) {
            sum0 = __builtin_amdgcn_sad_u8(c0[y], 0u, sum0);
            sum1 = __builtin_amdgcn_sad_u8(c1[y], 0u, sum1);
        }
        sum0 += (uint32_t)__shfl_xor((int)sum0, 1, 64);
        sum1 += (uint32_t)__shfl_xor((int)sum1, 1, 64);
        const uint32_t m0 = ((sum0 + 32) >> 6) * 0x01010101u, m1 = ((sum1 + 32) >> 6) * 0x01010101u;
        uint32_t dev0 = 0, dev1 = 0;
        for (int y = 8 * half; y < 8 * half + 8; y++) {
            dev0 = __builtin_amdgcn_sad_u8(c0[y], m0, dev0);
            dev1 = __builtin_amdgcn_sad_u8(c1[y], m1, dev1);
        }
        dev0 += (uint32_t)__shfl_xor((int)dev0, 1, 64);
        dev1 += (uint32_t)__shfl_xor((int)dev1, 1, 64);
        best0 = min(best0, dev0);
        best1 = min(best1, dev1);
    }
    best0 = min(best0, (uint32_t)__shfl_xor((int)best0, 2, 64));
    best1 = min(best1, (uint32_t)__shfl_xor((int)best1, 2, 64));
    const bool lead = (lane & 3) == 0;  // one lane per macroblock: 16 in the first set of words, 6 in the second
    const uint32_t a0 = lead ? 1 + best0 : 0u, a1 = lead && tail ? 1 + best1 : 0u;
    uint16_t* act = a.aq_act + ((size_t)s * kMbRows + row) * kMbCols;
    if (lead) {
        act[lane >> 2] = (uint16_t)a0;
        if (tail)
            act[16 + (lane >> 2)] = (uint16_t)a1;
    }
    const int sum = wave_sum((int)(a0 + a1));
    if (lane == 0)
        a.aq_sums[(size_t)s * kMbRows + row] = (uint32_t)sum;
}

// Scene-cut measure of one macroblock row (enc_cut.h).  The row's 16 luma lines are read as k_enc_act reads them; the sum
// of a word's four bytes over four lines is one decimated pel, so lane l holds column l of the row's four decimated lines
// (lanes 0 .. 23 column 64 + l as well).  They go to LDS and, as words, to the stream's current decimated picture.  The
// previous decimated picture's rows 4 row - 4 .. 4 row + 7 are staged next to them (its writers ran in the launch
// before, or in the call before); a macroblock's block is four words, a candidate four v_sad_u8 on alignbyte-shifted
// words, 22 x 81 candidates across the lanes, the minimum per macroblock kept in LDS.
__global__ __launch_bounds__(64) void k_enc_cut(EncArgs a)
{
    using namespace enc;
    constexpr int kRowW = kCutW / 4, kStride = kRowW + 2;  // words of a decimated line; staged lines carry the word alignbyte reads past the last
    const int row = blockIdx.x % kMbRows, s = blockIdx.x / kMbRows, lane = threadIdx.x;
    const EncState S = a.st[s];
    const bool has_prev = S.pictures != 0, tail = lane < kW / 4 - 64;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.src + (size_t)s * a.src_stride + (size_t)a.picture * kPicBytes +
                                                            (size_t)row * 16 * kW);
    uint8_t* cur = a.cut_pics + ((size_t)s * 2 + (S.pictures & 1)) * kCutBytes;
    const uint8_t* prev = a.cut_pics + ((size_t)s * 2 + ((S.pictures & 1) ^ 1)) * kCutBytes;

    __shared__ uint32_t cur_w[4 * kRowW];        // the row's four decimated lines
    __shared__ uint32_t prev_w[12 * kStride];    // lines 4 row - 4 .. 4 row + 7 of the previous decimated picture
    __shared__ uint32_t best[kMbCols];
    uint8_t* cur_b = reinterpret_cast<uint8_t*>(cur_w);
    for (int j = 0; j < 4; j++) {
        uint32_t sum0 = 0, sum1 = 0;
        for (int y = 4 * j; y < 4 * j + 4; y++) {
            sum0 = __builtin_amdgcn_sad_u8(src[y * (kW / 4) + lane], 0u, sum0);
            if (tail)
                sum1 = __builtin_amdgcn_sad_u8(src[y * (kW / 4) + 64 + lane], 0u, sum1);
        }
        cur_b[j * kCutW + lane] = (uint8_t)((sum0 + 8) >> 4);
        if (tail)
            cur_b[j * kCutW + 64 + lane] = (uint8_t)((sum1 + 8) >> 4);
    }
    if (lane < kMbCols)
        best[lane] = 0xFFFFFFFFu;
    if (has_prev)
        for (int i = lane; i < 12 * kStride; i += 64) {
            const int y = i / kStride, x = i - y * kStride, gy = 4 * row - 4 + y;
            prev_w[i] = (x < kRowW && gy >= 0 && gy < kCutH) ? reinterpret_cast<const uint32_t*>(prev)[gy * kRowW + x] : 0u;
        }
    __syncthreads();
    // the row's 4 x 88 bytes = 88 words of the current decimated picture
    uint32_t* out = reinterpret_cast<uint32_t*>(cur) + 4 * row * kRowW;
    out[lane] = cur_w[lane];
    if (tail)
        out[64 + lane] = cur_w[64 + lane];
    uint32_t dev = 0;
    if (lane < kMbCols) {
        uint32_t sum = 0;
        for (int j = 0; j < 4; j++)
            sum = __builtin_amdgcn_sad_u8(cur_w[j * kRowW + lane], 0u, sum);
        const uint32_t m = ((sum + 8) >> 4) * 0x01010101u;
        for (int j = 0; j < 4; j++)
            dev = __builtin_amdgcn_sad_u8(cur_w[j * kRowW + lane], m, dev);
    }
    if (has_prev) {
        for (int i = lane; i < kMbCols * kCutSide * kCutSide; i += 64) {
            const int c = i / (kCutSide * kCutSide), v = i - c * (kCutSide * kCutSide);
            const int dy = v / kCutSide - kCutRange, dx = v - (v / kCutSide) * kCutSide - kCutRange;
            if (!cut_vector_ok(row, c, dx, dy))
                continue;
            const int x = 4 * c + dx, w0 = x >> 2, sh = x & 3;
            uint32_t sad = 0;
            for (int j = 0; j < 4; j++) {
                const int o = (4 + dy + j) * kStride + w0;
                sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(prev_w[o + 1], prev_w[o], sh), cur_w[j * kRowW + c], sad);
            }
            atomicMin(&best[c], sad);
        }
        __syncthreads();
    }
    const uint32_t p = lane < kMbCols ? (has_prev ? min(dev, best[lane]) : dev) : 0u;
    const int cut_i = wave_sum((int)dev), cut_p = wave_sum((int)p);
    if (lane == 0) {
        uint2 w;
        w.x = (uint32_t)cut_i;
        w.y = (uint32_t)cut_p;
        *reinterpret_cast<uint2*>(a.cut_sums + ((size_t)s * kMbRows + row) * 2) = w;
    }
}

// The call's rate parameters with the gain of the stream's picture about to be coded: G_k = bitrate x (offset(k + 1) -
// offset(k)) of the streams' picture rate, used for every picture of the look-ahead's horizon too
__device__ inline enc::RateParams rate_params(const EncArgs& a, const EncState& S)
{
    enc::RateParams p = a.rate;
    p.gain = a.bitrate * enc::rate_pts_step(a.rate_code, (int64_t)S.pictures);
    return p;
}

// The picture's type (enc::kTypeI / kTypeP / kTypeCutI): with scene cuts, from the stream's row sums added in row order.
// Every wave of a stream (and k_enc_pack) gets the same value.
__device__ inline int picture_type(const EncArgs& a, const EncState& S, int s, uint32_t* cut_i, uint32_t* cut_p)
{
    uint32_t ci = 0, cp = 0;
    if (a.cut.threshold > 0)
        for (int k = 0; k < enc::kMbRows; k++) {
            const uint2 w = *reinterpret_cast<const uint2*>(a.cut_sums + ((size_t)s * enc::kMbRows + k) * 2);
            ci += w.x;
            cp += w.y;
        }
    *cut_i = ci;
    *cut_p = cp;
    return enc::cut_picture_type(S.pictures, S.g, a.gop, a.cut, ci, cp);
}

// The picture's quantiser under rate control: the stream's row sums added in row order, then the controller.  Every wave
// of a stream (and k_enc_pack) gets the same value.
__device__ inline int rate_q(const EncArgs& a, const EncState& S, int s, int phase, uint32_t* act_i, uint32_t* act_p)
{
    uint32_t ai = 0, ap = 0;
    for (int k = 0; k < enc::kMbRows; k++) {
        const uint2 w = *reinterpret_cast<const uint2*>(a.act + ((size_t)s * enc::kMbRows + k) * 2);
        ai += w.x;
        ap += w.y;
    }
    *act_i = ai;
    *act_p = ap;
    return enc::rate_decide(S.rate, rate_params(a, S), S.pictures, phase, a.gop, ai, ap);
}

// The picture's average activity: the stream's row sums of k_enc_aq added in row order.  Every wave of a stream gets the
// same value.
__device__ inline uint32_t aq_avg(const EncArgs& a, int s)
{
    uint32_t sum = 0;
    for (int k = 0; k < enc::kMbRows; k++)
        sum += a.aq_sums[(size_t)s * enc::kMbRows + k];
    return enc::aq_average(sum);
}

// k_enc_rows: k_enc_rows_t<false>, and <true> with adaptive quantisation.  Two kernels, so that the encoder without the
// option runs the code it ran before there was one.
template <bool kAq>
__global__ __launch_bounds__(64) void k_enc_rows_t(EncArgs a)
{
    using namespace enc;
    const int row = blockIdx.x % kMbRows, s = blockIdx.x / kMbRows, lane = threadIdx.x;
    const Tables& T = *a.tab;
    const EncState S = a.st[s];
    uint32_t cut_i, cut_p;
    const int ptype = picture_type(a, S, s, &cut_i, &cut_p);
    const int type = ptype == kTypeP ? 2 : 1;
    int qscale = a.qscale;
    if (a.rc) {
        uint32_t act_i, act_p;
        qscale = rate_q(a, S, s, cut_phase(ptype, S.g), &act_i, &act_p);
    }
    const uint8_t* src = a.src + (size_t)s * a.src_stride + (size_t)a.picture * kPicBytes;
    const uint8_t* ref = a.pics + ((size_t)s * 2 + S.cur) * kPicBytes;
    uint8_t* rec = a.pics + ((size_t)s * 2 + (S.cur ^ 1)) * kPicBytes;
    uint8_t* rec_out = a.recon ? a.recon + ((size_t)s * a.n_pictures + a.picture) * kPicBytes : nullptr;

    __shared__ Mb mbs[kMbCols];
    __shared__ uint32_t cur_w[64];                      // the macroblock's luma, 16 rows x 4 words
    __shared__ uint32_t win_w[kWin * kWinStride / 4 + 4];  // search window
    __shared__ int best_sad;
    __shared__ uint8_t mq[kMbCols];  // kAq: the macroblocks' quantisers
    uint8_t* win = reinterpret_cast<uint8_t*>(win_w);
    const int R = a.search, side = 2 * R + 1, wn = 2 * R + 18;
    if (kAq) {
        const uint32_t avg = aq_avg(a, s);
        if (lane < kMbCols) {
            const uint32_t act = a.aq_act[((size_t)s * kMbRows + row) * kMbCols + lane];
            const int q = aq_mb_quant(qscale, a.aq.strength, act, avg, a.rc ? a.rate.qmin : 1, a.rc ? a.rate.qmax : 31);
            mq[lane] = (uint8_t)q;
            a.aq_map[((size_t)s * kEncInfoCap + a.picture) * kAqMbs + row * kMbCols + lane] = (uint8_t)q;
        }
        __syncthreads();
    }

    for (int mbx = 0; mbx < kMbCols; mbx++) {
        cur_w[lane] = *reinterpret_cast<const uint32_t*>(src + (row * 16 + (lane >> 2)) * kW + mbx * 16 + (lane & 3) * 4);
        int h = 0, v = 0;
        bool intra = type == 1;
        if (type == 2) {
            const int wx0 = mbx * 16 - R - 1, wy0 = row * 16 - R - 1;
            for (int i = lane; i < wn * wn; i += 64) {
                const int wy = i / wn, wx = i - wy * wn, gx = wx0 + wx, gy = wy0 + wy;
                win[wy * kWinStride + wx] = (gx >= 0 && gx < kW && gy >= 0 && gy < kH) ? ref[gy * kW + gx] : 0;
            }
            __syncthreads();
            // full-pel search: one candidate per lane, 16 x 4 byte-quad SADs against the uniform current rows
            uint32_t best = 0xFFFFFFFFu;
            for (int c = lane; c < side * side; c += 64) {
                const int dy = c / side - R, dx = c - (c / side) * side - R;
                if (!mv_ok(mbx, row, 2 * dx, 2 * dy))
                    continue;
                const int base = (dy + R + 1) * kWinStride + dx + R + 1;
                uint32_t sad = 0;
                for (int y = 0; y < 16; y++) {
                    const int o = base + y * kWinStride;
                    const int w0 = o >> 2, sh = o & 3;
                    const uint32_t q0 = win_w[w0], q1 = win_w[w0 + 1], q2 = win_w[w0 + 2], q3 = win_w[w0 + 3], q4 = win_w[w0 + 4];
                    sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(q1, q0, sh), cur_w[y * 4 + 0], sad);
                    sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(q2, q1, sh), cur_w[y * 4 + 1], sad);
                    sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(q3, q2, sh), cur_w[y * 4 + 2], sad);
                    sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(q4, q3, sh), cur_w[y * 4 + 3], sad);
                }
                best = min(best, search_key(search_cost((int)sad, dx, dy), dx, dy, c));
            }
            best = wave_min(best);
            const int bc = (int)(best & 1023), bdy = bc / side - R, bdx = bc - (bc / side) * side - R;
            // the best vector and its 8 half-pel neighbours, with the decoder's interpolation (search 0: the zero vector
            // only, lane 4 alone, for its SAD)
            uint32_t key2 = 0xFFFFFFFFu;
            int sad2 = 0;
            if (lane < 9 && (R > 0 || lane == 4)) {
                const int hh = 2 * bdx + lane % 3 - 1, vv = 2 * bdy + lane / 3 - 1;
                if (mv_ok(mbx, row, hh, vv)) {
                    const int px = (mbx << 5) + hh, py = (row << 5) + vv;
                    const uint8_t* w = win + ((py >> 1) - wy0) * kWinStride + (px >> 1) - wx0;
                    const uint8_t* cur = reinterpret_cast<const uint8_t*>(cur_w);
                    for (int y = 0; y < 16; y++)
                        for (int x = 0; x < 16; x++) {
                            const int p = interp(w + y * kWinStride + x, kWinStride, px & 1, py & 1);
                            const int d = p - cur[y * 16 + x];
                            sad2 += d < 0 ? -d : d;
                        }
                    const int cost = lane == 4 ? search_cost(sad2, bdx, bdy) : sad2;
                    key2 = ((uint32_t)cost << 4) | (lane == 4 ? 0u : (uint32_t)lane + 1);
                }
            }
            const uint32_t win2 = wave_min(key2);
            const int bl = (int)(win2 & 15) == 0 ? 4 : (int)(win2 & 15) - 1;
            if (lane < 9 && key2 == win2)
                best_sad = sad2;
            h = 2 * bdx + bl % 3 - 1;
            v = 2 * bdy + bl / 3 - 1;
            // intra cost: the luma's deviation from its own mean
            const uint32_t wv = cur_w[lane];
            const int sum = wave_sum((int)((wv & 255) + ((wv >> 8) & 255) + ((wv >> 16) & 255) + (wv >> 24)));
            const int mean = (sum + 128) >> 8;
            int dev = 0;
            for (int k = 0; k < 4; k++) {
                const int d = (int)((wv >> (8 * k)) & 255) - mean;
                dev += d < 0 ? -d : d;
            }
            dev = wave_sum(dev);
            __syncthreads();
            intra = choose_intra(dev, best_sad);
            if (intra)
                h = v = 0;
        }
        // one lane per block: prediction, transform, quantisation, reconstruction
        const int mb_q = kAq ? __builtin_amdgcn_readfirstlane((int)mq[mbx]) : qscale;  // (the same in every lane: kept scalar)
        int coded = 0;
        if (lane < 6) {
            uint8_t blk[64];
            if (!intra)
                predict_block(ref, lane, mbx, row, h, v, blk);
            int pitch;
            const uint8_t* sb = block_ptr(src, lane, mbx, row, &pitch);
            coded = code_block(sb, pitch, intra, mb_q, T, blk, mbs[mbx].lev[lane]);
            uint8_t* rb = const_cast<uint8_t*>(block_ptr(rec, lane, mbx, row, &pitch));
            for (int y = 0; y < 8; y++) {
                uint2 w;
                w.x = blk[y * 8] | blk[y * 8 + 1] << 8 | blk[y * 8 + 2] << 16 | (uint32_t)blk[y * 8 + 3] << 24;
                w.y = blk[y * 8 + 4] | blk[y * 8 + 5] << 8 | blk[y * 8 + 6] << 16 | (uint32_t)blk[y * 8 + 7] << 24;
                *reinterpret_cast<uint2*>(rb + y * pitch) = w;
                if (rec_out)
                    *reinterpret_cast<uint2*>(rec_out + (rb - rec) + y * pitch) = w;
            }
        }
        const uint64_t cm = __ballot(lane < 6 && coded);
        if (lane == 0) {
            int cbp = 0;
            for (int b = 0; b < 6; b++)
                if ((cm >> b) & 1)
                    cbp |= 0x20 >> b;
            mbs[mbx].h = (int8_t)h;
            mbs[mbx].v = (int8_t)v;
            mbs[mbx].intra = intra ? 1 : 0;
            mbs[mbx].cbp = (uint8_t)(intra ? 0 : cbp);
        }
        __syncthreads();
    }
    if (lane == 0)
        a.slice_len[(size_t)s * kMbRows + row] =
            write_slice_t<kAq>(a.slices + ((size_t)s * kMbRows + row) * kSliceCap, row, qscale, type, a.f_code, mbs, T, kAq ? mq : nullptr);
}

template __global__ void k_enc_rows_t<false>(EncArgs);
template __global__ void k_enc_rows_t<true>(EncArgs);

__global__ __launch_bounds__(256) void k_enc_pack(EncArgs a)
{
    using namespace enc;
    const int s = blockIdx.x, tid = threadIdx.x;
    __shared__ uint8_t hdr[kHdrCap];
    __shared__ uint32_t seg[kMbRows + 2];  // ES offsets: headers, then slice k at seg[k + 1]
    __shared__ uint32_t sh_bytes, sh_ok;
    EncState S = a.st[s];
    uint32_t cut_i, cut_p;
    const int ptype = picture_type(a, S, s, &cut_i, &cut_p);
    const uint32_t phase = (uint32_t)cut_phase(ptype, S.g);
    const int type = ptype == kTypeP ? 2 : 1;
    const bool ts = a.format == EFX_FORMAT_TS;
    if (tid == 0) {
        seg[0] = 0;
        seg[1] = write_headers(hdr, phase == 0, S.pictures, (int)phase, type, a.f_code, a.rate_code);
        for (int k = 0; k < kMbRows; k++)
            seg[k + 2] = seg[k + 1] + a.slice_len[(size_t)s * kMbRows + k];
        const uint32_t es = seg[kMbRows + 1];
        const uint32_t bytes = ts ? ts_packets(es + kPesHdrBytes) * 188 : es;
        sh_bytes = bytes;
        sh_ok = !S.full && (uint64_t)S.out_len + bytes <= a.dst_stride;
    }
    __syncthreads();
    const uint32_t bytes = sh_bytes, es_len = seg[kMbRows + 1];
    const int64_t pts = (S.first_pts + rate_pts_offset(a.rate_code, (int64_t)S.pictures)) & ((1ll << 33) - 1);
    if (sh_ok) {
        uint8_t* out = a.dst + (size_t)s * a.dst_stride + S.out_len;
        const uint8_t* sl = a.slices + (size_t)s * kMbRows * kSliceCap;
        for (uint32_t o = tid; o < bytes; o += 256) {
            int64_t e = o;
            uint8_t b = 0;
            if (ts) {
                int64_t pp;
                b = ts_byte(o, es_len + kPesHdrBytes, S.cc, &pp);
                e = pp < kPesHdrBytes ? -1 : pp - kPesHdrBytes;
                if (pp >= 0 && pp < kPesHdrBytes)
                    b = pes_header_byte((int)pp, pts);
            }
            if (e >= 0) {
                const uint32_t u = (uint32_t)e;
                if (u < seg[1])
                    b = hdr[u];
                else {
                    int k = 0;
                    while (u >= seg[k + 2])
                        k++;
                    b = sl[(size_t)k * kSliceCap + (u - seg[k + 1])];
                }
            }
            out[o] = b;
        }
    }
    if (a.aq.strength > 0 && !sh_ok && tid < kAqMbs / 4)  // a picture that was not written has no quantisers
        reinterpret_cast<uint32_t*>(a.aq_map + ((size_t)s * kEncInfoCap + a.picture) * kAqMbs)[tid] = 0u;
    __syncthreads();
    if (tid == 0) {
        if (a.rc) {
            // a picture that was not written changes nothing of the buffer or the history
            uint32_t act_i, act_p;
            const int q = rate_q(a, S, s, (int)phase, &act_i, &act_p);
            if (sh_ok && rate_update(&S.rate, rate_params(a, S), (int)phase, q, bytes, act_i, act_p))
                S.status |= EFX_ENCODE_VBV;
            if (a.qscale_out)
                a.qscale_out[(size_t)s * a.n_pictures + a.picture] = (uint8_t)(sh_ok ? q : 0);
        }
        if (sh_ok) {
            S.out_len += bytes;
            if (ts)
                S.cc = (S.cc + ts_packets(es_len + kPesHdrBytes)) & 15;
        } else if (!S.full) {
            S.full = 1;
            S.status |= EFX_ENCODE_FULL;
            *(volatile uint32_t*)a.full_flag = a.generation;
        }
        EncPictureInfo info{};
        info.cut_i = cut_i;
        info.cut_p = cut_p;
        info.type = (uint8_t)(sh_ok ? ptype : 0);
        a.info[(size_t)s * kEncInfoCap + a.picture] = info;
        S.g = cut_next_g(ptype, S.g);
        S.pictures++;
        S.cur ^= 1;
        a.st[s] = S;
        a.len[s] = S.out_len;
        a.status[s] = S.status;
    }
}

}  // namespace efx
