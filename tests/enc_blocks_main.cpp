// Host build of the encoder's block arithmetic (espflix_amd/csrc/enc_core.h) for single 8 x 8 blocks: the forward DCT and
// code_block, for tests/test_encode_yardstick.py, which compares them with float64.
//
//   enc_blocks fdct <in> <out>   in: int32 [n][64] blocks (raster);  out: int32 [n][64] fdct8 outputs (raster)
//   enc_blocks code <in> <out>   in: [n] records of intra (1 byte), q (1 byte), source block (64 bytes), prediction (64 bytes)
//                                out: int32 [n][129]: fdct8 of the source (intra) or of source - prediction (raster), the
//                                levels code_block returns (scan order), and whether its halving loop ran
#include <cstdio>
#include <cstring>
#include <vector>

#include "enc_core.h"

using namespace efx::enc;

static bool read_all(const char* path, std::vector<uint8_t>* buf)
{
    FILE* f = fopen(path, "rb");
    if (!f)
        return false;
    fseek(f, 0, SEEK_END);
    buf->resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    const bool ok = fread(buf->data(), 1, buf->size(), f) == buf->size();
    fclose(f);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc != 4)
        return 2;
    std::vector<uint8_t> in;
    if (!read_all(argv[2], &in))
        return 3;
    static Tables T;
    build_tables(&T);
    std::vector<int32_t> out;
    if (!strcmp(argv[1], "fdct")) {
        const size_t n = in.size() / (64 * sizeof(int32_t));
        out.resize(n * 64);
        for (size_t i = 0; i < n; i++) {
            int pix[64], F[64];
            for (int k = 0; k < 64; k++) {
                int32_t v;
                memcpy(&v, in.data() + (i * 64 + k) * sizeof v, sizeof v);
                pix[k] = v;
            }
            fdct8(pix, F, T);
            for (int k = 0; k < 64; k++)
                out[i * 64 + k] = F[k];
        }
    } else if (!strcmp(argv[1], "code")) {
        const size_t n = in.size() / 130;
        out.resize(n * 129);
        for (size_t i = 0; i < n; i++) {
            const uint8_t* r = in.data() + i * 130;
            const bool intra = r[0] != 0;
            const int q = r[1];
            int pix[64], F[64], lev[64];
            for (int k = 0; k < 64; k++)
                pix[k] = (int)r[2 + k] - (intra ? 0 : (int)r[66 + k]);
            fdct8(pix, F, T);
            uint8_t blk[64];
            memcpy(blk, r + 66, 64);
            quantise(F, intra, q, T, lev);
            const bool halved = !reconstruct(lev, intra, q, T, blk, false);  // code_block's loop condition on its first levels
            int16_t coded[64];
            code_block(r + 2, 8, intra, q, T, blk, coded);
            for (int k = 0; k < 64; k++) {
                out[i * 129 + k] = F[k];
                out[i * 129 + 64 + k] = coded[k];
            }
            out[i * 129 + 128] = halved;
        }
    } else
        return 2;
    FILE* o = fopen(argv[3], "wb");
    if (!o)
        return 4;
    fwrite(out.data(), sizeof(int32_t), out.size(), o);
    fclose(o);
    return 0;
}
