// Host build of the encoder with adaptive quantisation (efx_encode_set_adaptive_quant): enc_core.h's arithmetic as
// tests/enc_rate_model_main.cpp restates k_encode.hip's decisions, with every macroblock's quantiser from enc_aq.h around
// the picture's -- the fixed one (efx_encode), or the one enc_rate.h chooses (efx_encode_rc) -- the decisions k_enc_aq /
// k_enc_act / k_enc_rows / k_enc_pack make, serially, one stream.
//
//   enc_aq_model <in.i420> <n_pictures> <gop> <qscale> <search> <format 0 ES / 1 TS> <first_pts> <bitrate or 0> <vbv_bits>
//                <qmin> <qmax> <out.stream> <out.recon> <out.q> <state.in or -> <state.out or -> <strength> <out.mq>
//                <out.slices>
//   enc_aq_model lengths
//
// bitrate 0: every picture at qscale (efx_encode), vbv_bits / qmin / qmax unused.  strength 0: adaptive quantisation off,
// write_slice is called as the other host models call it.  out.q: one quantiser per picture, then the 4 bytes of the
// status word (EFX_ENCODE_VBV or 0).  out.mq: 264 quantisers per picture, index 22 r + c (strength 0: the picture's
// quantiser throughout).  out.slices: twelve uint32 slice lengths per picture.  A state file carries a stream from one
// run to the next (cont = 1).  `lengths` prints the code lengths the bound of enc_core.h's kMbMaxBits rests on.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "enc_aq.h"
#include "enc_core.h"
#include "enc_rate.h"

using namespace efx::enc;

struct Carry {
    uint32_t pictures, cc;
    long long first_pts;
    RateState rate;
};

// One picture at quantiser q, macroblock (r, c) at mq[22 r + c] when mq is given: reconstruction into rec, the twelve
// slices into slices / slice_len
static void code_picture(const uint8_t* cur, const std::vector<uint8_t>& ref, std::vector<uint8_t>& rec, int type, int q, int R,
                         int f_code, const Tables& T, std::vector<uint8_t>& slices, uint32_t* slice_len, const uint8_t* mq)
{
    static Mb mbs[kMbCols];
    for (int row = 0; row < kMbRows; row++) {
        for (int mbx = 0; mbx < kMbCols; mbx++) {
            int h = 0, v = 0;
            bool intra = type == 1;
            const uint8_t* cy = cur + row * 16 * kW + mbx * 16;
            if (type == 2) {
                const int side = 2 * R + 1;
                uint32_t best = 0xFFFFFFFFu;
                for (int c = 0; c < side * side; c++) {
                    const int dy = c / side - R, dx = c % side - R;
                    if (!mv_ok(mbx, row, 2 * dx, 2 * dy))
                        continue;
                    int sad = 0;
                    const uint8_t* r = ref.data() + (row * 16 + dy) * kW + mbx * 16 + dx;
                    for (int y = 0; y < 16; y++)
                        for (int x = 0; x < 16; x++)
                            sad += abs((int)r[y * kW + x] - (int)cy[y * kW + x]);
                    const uint32_t k = search_key(search_cost(sad, dx, dy), dx, dy, c);
                    best = k < best ? k : best;
                }
                const int bc = (int)(best & 1023), bdy = bc / side - R, bdx = bc % side - R;
                uint32_t win2 = 0xFFFFFFFFu;
                int best_sad = 0;
                for (int j = 0; j < 9; j++) {
                    if (R == 0 && j != 4)  // search 0: the zero vector only
                        continue;
                    const int hh = 2 * bdx + j % 3 - 1, vv = 2 * bdy + j / 3 - 1;
                    if (!mv_ok(mbx, row, hh, vv))
                        continue;
                    const int px = (mbx << 5) + hh, py = (row << 5) + vv;
                    const uint8_t* w = ref.data() + (py >> 1) * kW + (px >> 1);
                    int sad = 0;
                    for (int y = 0; y < 16; y++)
                        for (int x = 0; x < 16; x++)
                            sad += abs(interp(w + y * kW + x, kW, px & 1, py & 1) - (int)cy[y * kW + x]);
                    const int cost = j == 4 ? search_cost(sad, bdx, bdy) : sad;
                    const uint32_t k = ((uint32_t)cost << 4) | (j == 4 ? 0u : (uint32_t)j + 1);
                    if (k < win2) {
                        win2 = k;
                        best_sad = sad;
                    }
                }
                const int bl = (int)(win2 & 15) == 0 ? 4 : (int)(win2 & 15) - 1;
                h = 2 * bdx + bl % 3 - 1;
                v = 2 * bdy + bl / 3 - 1;
                int sum = 0, dev = 0;
                for (int y = 0; y < 16; y++)
                    for (int x = 0; x < 16; x++)
                        sum += cy[y * kW + x];
                const int mean = (sum + 128) >> 8;
                for (int y = 0; y < 16; y++)
                    for (int x = 0; x < 16; x++)
                        dev += abs((int)cy[y * kW + x] - mean);
                intra = choose_intra(dev, best_sad);
                if (intra)
                    h = v = 0;
            }
            int cbp = 0;
            for (int b = 0; b < 6; b++) {
                uint8_t blk[64];
                if (!intra)
                    predict_block(ref.data(), b, mbx, row, h, v, blk);
                int pitch;
                const uint8_t* sb = block_ptr(cur, b, mbx, row, &pitch);
                if (code_block(sb, pitch, intra, mq ? mq[row * kMbCols + mbx] : q, T, blk, mbs[mbx].lev[b]))
                    cbp |= 0x20 >> b;
                uint8_t* rb = const_cast<uint8_t*>(block_ptr(rec.data(), b, mbx, row, &pitch));
                for (int y = 0; y < 8; y++)
                    memcpy(rb + y * pitch, blk + y * 8, 8);
            }
            mbs[mbx].h = (int8_t)h;
            mbs[mbx].v = (int8_t)v;
            mbs[mbx].intra = intra ? 1 : 0;
            mbs[mbx].cbp = (uint8_t)(intra ? 0 : cbp);
        }
        uint8_t* out = slices.data() + (size_t)row * kSliceCap;
        slice_len[row] = mq ? write_slice(out, row, q, type, f_code, mbs, T, mq + row * kMbCols)
                            : write_slice(out, row, q, type, f_code, mbs, T);
    }
}

int main(int argc, char** argv)
{
    static Tables T;
    build_tables(&T);
    if (argc == 2 && !strcmp(argv[1], "lengths")) {
        int mba = 0, cbp = 0, mv = 0;
        for (int i = 1; i <= 21; i++)
            mba = T.mba_len[i] > mba ? T.mba_len[i] : mba;
        for (int i = 1; i < 64; i++)
            cbp = T.cbp_len[i] > cbp ? T.cbp_len[i] : cbp;
        for (int i = 0; i < 33; i++)
            mv = T.mv_len[i] > mv ? T.mv_len[i] : mv;
        printf("mba21 %d cbp63 %d cbp_max %d mv_max %d intra %d intra_q %d pat %d pat_q %d fwd_pat %d fwd_pat_q %d fwd %d "
               "mb_max_bits %d slice_cap %d\n",
               mba, T.cbp_len[63], cbp, mv, T.type_p_len[1], T.type_p_len[17], T.type_p_len[2], T.type_p_len[18], T.type_p_len[10],
               T.type_p_len[26], T.type_p_len[8], kMbMaxBits, kSliceCap);
        return 0;
    }
    if (argc != 20)
        return 2;
    const long long bitrate = atoll(argv[8]);
    const int strength = atoi(argv[17]);
    const int n_pictures = atoi(argv[2]), gop = atoi(argv[3]), q_opt = atoi(argv[4]), R = atoi(argv[5]), format = atoi(argv[6]);
    const int f_code = R <= 7 ? 1 : 2;
    RateParams P;
    P.cap = atoll(argv[9]) * 90000;
    P.gain = atoll(argv[8]) * kRcTick;
    P.qmin = atoi(argv[10]);
    P.qmax = atoi(argv[11]);
    P.q0 = q_opt < P.qmin ? P.qmin : (q_opt > P.qmax ? P.qmax : q_opt);
    std::vector<uint8_t> src((size_t)n_pictures * kPicBytes);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size())
        return 3;
    fclose(f);
    std::vector<uint8_t> ref(kPicBytes), rec(kPicBytes), out, recon, qs, maps;
    std::vector<uint32_t> lens;
    std::vector<uint8_t> slices((size_t)kMbRows * kSliceCap);
    uint32_t slice_len[kMbRows];
    Carry S{};
    S.first_pts = atoll(argv[7]);
    rate_reset(&S.rate, P);
    if (strcmp(argv[15], "-")) {
        FILE* s = fopen(argv[15], "rb");
        if (!s || fread(&S, sizeof(S), 1, s) != 1 || fread(ref.data(), 1, ref.size(), s) != ref.size())
            return 5;
        fclose(s);
    }
    uint32_t status = 0;
    for (int p = 0; p < n_pictures; p++) {
        const uint8_t* cur = src.data() + (size_t)p * kPicBytes;
        const uint32_t phase = S.pictures % (uint32_t)gop;
        const int type = phase == 0 ? 1 : 2;
        // activity: per row, then the rows in order (k_enc_act's sums)
        uint32_t act_i = 0, act_p = 0;
        for (int row = 0; row < kMbRows; row++)
            for (int mbx = 0; mbx < kMbCols; mbx++) {
                int dev, sad;
                const size_t o = (size_t)row * 16 * kW + mbx * 16;
                mb_activity(cur + o, S.pictures ? ref.data() + o : nullptr, kW, &dev, &sad);
                act_i += (uint32_t)dev;
                act_p += (uint32_t)(S.pictures && sad < dev ? sad : dev);
            }
        const int q = bitrate ? rate_decide(S.rate, P, S.pictures, (int)phase, gop, act_i, act_p) : q_opt;
        // adaptive quantisation: the activities (k_enc_aq), their average and the 264 quantisers (k_enc_rows)
        uint8_t mq[kAqMbs];
        if (strength > 0) {
            uint32_t a[kAqMbs], sum = 0;
            for (int row = 0; row < kMbRows; row++)
                for (int mbx = 0; mbx < kMbCols; mbx++)
                    sum += a[row * kMbCols + mbx] = aq_mb_activity(cur + (size_t)row * 16 * kW + mbx * 16, kW);
            const uint32_t avg = aq_average(sum);
            for (int i = 0; i < kAqMbs; i++)
                mq[i] = (uint8_t)aq_mb_quant(q, strength, a[i], avg, bitrate ? P.qmin : 1, bitrate ? P.qmax : 31);
        } else
            memset(mq, q, sizeof(mq));
        code_picture(cur, ref, rec, type, q, R, f_code, T, slices, slice_len, strength > 0 ? mq : nullptr);
        maps.insert(maps.end(), mq, mq + kAqMbs);
        lens.insert(lens.end(), slice_len, slice_len + kMbRows);
        // picture bytes: headers, then the slices; TS: one PES in packets
        uint8_t hdr[kHdrCap];
        const uint32_t hl = write_headers(hdr, phase == 0, S.pictures, (int)phase, type, f_code);
        std::vector<uint8_t> es(hdr, hdr + hl);
        for (int r = 0; r < kMbRows; r++)
            es.insert(es.end(), slices.begin() + (size_t)r * kSliceCap, slices.begin() + (size_t)r * kSliceCap + slice_len[r]);
        uint32_t bytes = (uint32_t)es.size();
        if (format == 0)
            out.insert(out.end(), es.begin(), es.end());
        else {
            const int64_t pts = (S.first_pts + 3003LL * S.pictures) & ((1LL << 33) - 1);
            const uint32_t pes_len = (uint32_t)es.size() + kPesHdrBytes, npk = ts_packets(pes_len);
            for (uint32_t o = 0; o < npk * 188; o++) {
                int64_t pp;
                uint8_t b = ts_byte(o, pes_len, S.cc, &pp);
                if (pp >= 0)
                    b = pp < kPesHdrBytes ? pes_header_byte((int)pp, pts) : es[(size_t)pp - kPesHdrBytes];
                out.push_back(b);
            }
            S.cc = (S.cc + npk) & 15;
            bytes = npk * 188;
        }
        if (bitrate && rate_update(&S.rate, P, (int)phase, q, bytes, act_i, act_p))
            status |= 4096u;  // EFX_ENCODE_VBV
        qs.push_back((uint8_t)q);
        recon.insert(recon.end(), rec.begin(), rec.end());
        std::swap(ref, rec);
        S.pictures++;
    }
    FILE* o = fopen(argv[12], "wb");
    FILE* r = fopen(argv[13], "wb");
    FILE* qf = fopen(argv[14], "wb");
    FILE* mf = fopen(argv[18], "wb");
    FILE* lf = fopen(argv[19], "wb");
    if (!o || !r || !qf || !mf || !lf)
        return 4;
    fwrite(maps.data(), 1, maps.size(), mf);
    fwrite(lens.data(), 4, lens.size(), lf);
    fclose(mf);
    fclose(lf);
    fwrite(out.data(), 1, out.size(), o);
    fwrite(recon.data(), 1, recon.size(), r);
    fwrite(qs.data(), 1, qs.size(), qf);
    fwrite(&status, 4, 1, qf);
    fclose(o);
    fclose(r);
    fclose(qf);
    if (strcmp(argv[16], "-")) {
        FILE* s = fopen(argv[16], "wb");
        if (!s)
            return 4;
        fwrite(&S, sizeof(S), 1, s);
        fwrite(ref.data(), 1, ref.size(), s);
        fclose(s);
    }
    return 0;
}
