// Host build of the encoder with scene cuts (efx_encode_set_scene_cut): tests/enc_picture_rate_model_main.cpp's restatement
// of k_encode.hip's decisions with the picture type decided by enc_cut.h -- the decimated source picture, the two sums of
// k_enc_cut added row by row, cut_picture_type, g -- serially, one stream.  bitrate 0: a fixed quantiser (efx_encode);
// threshold 0: scene cuts off, the bytes of the programs this one restates.
//
//   enc_cut_model <in.i420> <n_pictures> <gop> <qscale> <search> <format 0 ES / 1 TS> <first_pts> <code> <bitrate or 0>
//                 <vbv_bits> <qmin> <qmax> <threshold> <min_gop> <out.stream> <out.recon> <out.q> <out.info>
//                 <state.in or -> <state.out or ->
//
// out.q: one quantiser per picture, then the 4 bytes of the status word (EFX_ENCODE_VBV or 0).  out.info: 12 bytes per
// picture, efx_enc_picture_info (cut_i, cut_p, type, three zeros; the sums are 0 with threshold 0).  A state file carries a
// stream from one run to the next (cont = 1): pictures so far, g, continuity counter, first PTS, the controller's state,
// the last reconstruction and the last decimated source picture.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "enc_core.h"
#include "enc_cut.h"
#include "enc_rate.h"

using namespace efx::enc;

struct Carry {
    uint32_t pictures, cc, g, pad;
    long long first_pts;
    RateState rate;
};

// One picture at quantiser q: reconstruction into rec, the twelve slices into slices / slice_len
static void code_picture(const uint8_t* cur, const std::vector<uint8_t>& ref, std::vector<uint8_t>& rec, int type, int q, int R,
                         int f_code, const Tables& T, std::vector<uint8_t>& slices, uint32_t* slice_len)
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
                if (code_block(sb, pitch, intra, q, T, blk, mbs[mbx].lev[b]))
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
        slice_len[row] = write_slice(slices.data() + (size_t)row * kSliceCap, row, q, type, f_code, mbs, T);
    }
}

int main(int argc, char** argv)
{
    if (argc != 21)
        return 2;
    const int n_pictures = atoi(argv[2]), gop = atoi(argv[3]), q_opt = atoi(argv[4]), R = atoi(argv[5]), format = atoi(argv[6]);
    const int f_code = R <= 7 ? 1 : 2;
    const int code = atoi(argv[8]);
    const long long bitrate = atoll(argv[9]);
    if (!rate_code_ok(code))
        return 2;
    RateParams P;
    P.cap = atoll(argv[10]) * 90000;
    P.gain = bitrate * kRcTick;
    P.qmin = atoi(argv[11]);
    P.qmax = atoi(argv[12]);
    P.q0 = q_opt < P.qmin ? P.qmin : (q_opt > P.qmax ? P.qmax : q_opt);
    std::vector<uint8_t> src((size_t)n_pictures * kPicBytes);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size())
        return 3;
    fclose(f);
    static Tables T;
    build_tables(&T);
    const CutParams cut{atoi(argv[13]), atoi(argv[14])};
    std::vector<uint8_t> ref(kPicBytes), rec(kPicBytes), out, recon, qs, infos;
    std::vector<uint8_t> d_prev(kCutBytes), d_cur(kCutBytes);
    std::vector<uint8_t> slices((size_t)kMbRows * kSliceCap);
    uint32_t slice_len[kMbRows];
    Carry S{};
    S.first_pts = atoll(argv[7]);
    rate_reset(&S.rate, P);
    if (strcmp(argv[19], "-")) {
        FILE* s = fopen(argv[19], "rb");
        if (!s || fread(&S, sizeof(S), 1, s) != 1 || fread(ref.data(), 1, ref.size(), s) != ref.size() ||
            fread(d_prev.data(), 1, d_prev.size(), s) != d_prev.size())
            return 5;
        fclose(s);
    }
    uint32_t status = 0;
    for (int p = 0; p < n_pictures; p++) {
        const uint8_t* cur = src.data() + (size_t)p * kPicBytes;
        // the measure: per row, then the rows in order (k_enc_cut's sums)
        uint32_t cut_i = 0, cut_p = 0;
        if (cut.threshold > 0) {
            cut_decimate(cur, kCutH, d_cur.data());
            for (int row = 0; row < kMbRows; row++)
                for (int mbx = 0; mbx < kMbCols; mbx++) {
                    uint32_t dev, best;
                    cut_mb(d_cur.data(), S.pictures ? d_prev.data() : nullptr, row, mbx, &dev, &best);
                    cut_i += dev;
                    cut_p += best < dev ? best : dev;
                }
        }
        const int ptype = cut_picture_type(S.pictures, S.g, gop, cut, cut_i, cut_p);
        const uint32_t phase = (uint32_t)cut_phase(ptype, S.g);
        const int type = ptype == kTypeP ? 2 : 1;
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
        P.gain = bitrate * rate_pts_step(code, (int64_t)S.pictures);  // this picture's, also over the look-ahead's horizon
        const int q = bitrate ? rate_decide(S.rate, P, S.pictures, (int)phase, gop, act_i, act_p) : q_opt;
        code_picture(cur, ref, rec, type, q, R, f_code, T, slices, slice_len);
        // picture bytes: headers, then the slices; TS: one PES in packets
        uint8_t hdr[kHdrCap];
        const uint32_t hl = write_headers(hdr, phase == 0, S.pictures, (int)phase, type, f_code, code);
        std::vector<uint8_t> es(hdr, hdr + hl);
        for (int r = 0; r < kMbRows; r++)
            es.insert(es.end(), slices.begin() + (size_t)r * kSliceCap, slices.begin() + (size_t)r * kSliceCap + slice_len[r]);
        uint32_t bytes = (uint32_t)es.size();
        if (format == 0)
            out.insert(out.end(), es.begin(), es.end());
        else {
            const int64_t pts = (S.first_pts + rate_pts_offset(code, (int64_t)S.pictures)) & ((1LL << 33) - 1);
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
        const uint32_t sums[2] = {cut_i, cut_p};
        const uint8_t tail[4] = {(uint8_t)ptype, 0, 0, 0};
        infos.insert(infos.end(), (const uint8_t*)sums, (const uint8_t*)sums + 8);
        infos.insert(infos.end(), tail, tail + 4);
        std::swap(d_prev, d_cur);
        S.g = cut_next_g(ptype, S.g);
        recon.insert(recon.end(), rec.begin(), rec.end());
        std::swap(ref, rec);
        S.pictures++;
    }
    FILE* o = fopen(argv[15], "wb");
    FILE* r = fopen(argv[16], "wb");
    FILE* qf = fopen(argv[17], "wb");
    FILE* inf = fopen(argv[18], "wb");
    if (!o || !r || !qf || !inf)
        return 4;
    fwrite(infos.data(), 1, infos.size(), inf);
    fclose(inf);
    fwrite(out.data(), 1, out.size(), o);
    fwrite(recon.data(), 1, recon.size(), r);
    fwrite(qs.data(), 1, qs.size(), qf);
    fwrite(&status, 4, 1, qf);
    fclose(o);
    fclose(r);
    fclose(qf);
    if (strcmp(argv[20], "-")) {
        FILE* s = fopen(argv[20], "wb");
        if (!s)
            return 4;
        fwrite(&S, sizeof(S), 1, s);
        fwrite(ref.data(), 1, ref.size(), s);
        fwrite(d_prev.data(), 1, d_prev.size(), s);
        fclose(s);
    }
    return 0;
}
