// Host build of the encoder's arithmetic (espflix_amd/csrc/enc_core.h), one stream, the decisions of k_encode.hip restated
// serially: the same search keys, half-pel choice, intra decision, block coding, slice, header and packet bytes.
// tests/test_encode_model.py decodes what it writes with the test oracle; tests/test_gpu_encode.py compares the device's
// output with it byte for byte.
//
//   enc_model <in.i420> <n_pictures> <gop> <qscale> <search> <format 0 ES / 1 TS> <first_pts> <out.stream> <out.recon>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "enc_core.h"

using namespace efx::enc;

int main(int argc, char** argv)
{
    if (argc != 10)
        return 2;
    const int n_pictures = atoi(argv[2]), gop = atoi(argv[3]), q = atoi(argv[4]), R = atoi(argv[5]), format = atoi(argv[6]);
    const long long first_pts = atoll(argv[7]);
    const int f_code = R <= 7 ? 1 : 2;
    std::vector<uint8_t> src((size_t)n_pictures * kPicBytes);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size())
        return 3;
    fclose(f);
    static Tables T;
    build_tables(&T);
    std::vector<uint8_t> ref(kPicBytes), rec(kPicBytes), out, recon;
    std::vector<uint8_t> slices((size_t)kMbRows * kSliceCap);
    uint32_t slice_len[kMbRows];
    static Mb mbs[kMbCols];
    uint32_t cc = 0;
    for (int p = 0; p < n_pictures; p++) {
        const uint8_t* cur = src.data() + (size_t)p * kPicBytes;
        const int type = p % gop == 0 ? 1 : 2;
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
        // picture bytes: headers, then the slices; TS: one PES in packets
        uint8_t hdr[kHdrCap];
        const uint32_t phase = (uint32_t)(p % gop);
        const uint32_t hl = write_headers(hdr, phase == 0, (uint32_t)p, (int)phase, type, f_code);
        std::vector<uint8_t> es(hdr, hdr + hl);
        for (int r = 0; r < kMbRows; r++)
            es.insert(es.end(), slices.begin() + (size_t)r * kSliceCap, slices.begin() + (size_t)r * kSliceCap + slice_len[r]);
        if (format == 0)
            out.insert(out.end(), es.begin(), es.end());
        else {
            const int64_t pts = (first_pts + 3003LL * p) & ((1LL << 33) - 1);
            const uint32_t pes_len = (uint32_t)es.size() + kPesHdrBytes, npk = ts_packets(pes_len);
            for (uint32_t o = 0; o < npk * 188; o++) {
                int64_t pp;
                uint8_t b = ts_byte(o, pes_len, cc, &pp);
                if (pp >= 0)
                    b = pp < kPesHdrBytes ? pes_header_byte((int)pp, pts) : es[(size_t)pp - kPesHdrBytes];
                out.push_back(b);
            }
            cc = (cc + npk) & 15;
        }
        recon.insert(recon.end(), rec.begin(), rec.end());
        std::swap(ref, rec);
    }
    FILE* o = fopen(argv[8], "wb");
    FILE* r = fopen(argv[9], "wb");
    if (!o || !r)
        return 4;
    fwrite(out.data(), 1, out.size(), o);
    fwrite(recon.data(), 1, recon.size(), r);
    fclose(o);
    fclose(r);
    return 0;
}
