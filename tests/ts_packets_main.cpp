// enc_core.h's packetiser on the host, for tests/test_mux_model.py:
//   ts_packets_main ts  in out   in: uint32 (PES length, first continuity counter) pairs; out: the packets of each PES back
//                                to back, PES byte k written as (k x 7 + 3) & 0xFF
//   ts_packets_main pes in out   in: int64 PTS values; out: pes_header_byte(0 .. 13) of each
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "enc_core.h"

template <typename T>
static std::vector<T> slurp(const char* path)
{
    std::vector<T> v;
    if (FILE* f = fopen(path, "rb")) {
        T x;
        while (fread(&x, sizeof x, 1, f) == 1)
            v.push_back(x);
        fclose(f);
    }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 4)
        return 2;
    std::vector<uint8_t> out;
    if (!strcmp(argv[1], "ts")) {
        const auto in = slurp<uint32_t>(argv[2]);
        for (size_t k = 0; k + 1 < in.size(); k += 2) {
            const uint32_t len = in[k], cc = in[k + 1], n = efx::enc::ts_packets(len) * 188;
            for (uint32_t o = 0; o < n; o++) {
                int64_t pp;
                const uint8_t b = efx::enc::ts_byte(o, len, cc, &pp);
                out.push_back(pp < 0 ? b : (uint8_t)(pp * 7 + 3));
            }
        }
    } else {
        for (int64_t pts : slurp<int64_t>(argv[2]))
            for (int i = 0; i < 14; i++)
                out.push_back(efx::enc::pes_header_byte(i, pts));
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size())
        return 1;
    fclose(f);
    return 0;
}
