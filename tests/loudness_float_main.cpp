// TEST: the yardstick of tests/loudness_float.py -- ITU-R BS.1770-4 K-weighting of one mono int16 stream, serially, in
// double, with the whole history (one filter from the first sample to the last), and the mean squares of the 400 ms blocks
// every 100 ms.  Shares no code with espflix_amd/csrc/loudness_px.h or tests/loudness_model.py; what is independent is
// the evaluation -- double, transposed direct form II, one serial pass, samples as fractions of full scale.  The
// coefficient design is NOT independent: the same bilinear-transform formulas and prototype constants as include/efx.h,
// typed in again.  Only at 48 kHz are they anchored from outside, to the coefficients BS.1770 prints
// (test_host_functions_of_the_library); at the other three rates the design rests on the tone cases reading within 0.1 LU.
//
//   loudness_float_main RATE PCM BLOCKS      BLOCKS receives one double per block: the mean of z^2 over 4 x RATE / 10 samples
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct Section {
    double b0, b1, b2, a1, a2, s1 = 0, s2 = 0;
    double run(double x)
    {
        const double y = b0 * x + s1;
        s1 = b1 * x - a1 * y + s2;
        s2 = b2 * x - a2 * y;
        return y;
    }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 4)
        return 2;
    const int rate = atoi(argv[1]);
    const double pi = std::acos(-1.0);
    // high shelf: H(s) = (Vh s^2 + Vb s w / Q + w^2) / (s^2 + s w / Q + w^2), s -> (1 - z^-1) / (1 + z^-1), w -> tan(pi f / rate)
    Section shelf{}, hp{};
    {
        const double w = std::tan(pi * 1681.974450955533 / rate), q = 0.7071752369554196;
        const double vh = std::pow(10.0, 3.999843853973347 / 20.0), vb = std::pow(vh, 0.4996667741545416);
        const double den = 1.0 + w / q + w * w;
        shelf.b0 = (vh + vb * w / q + w * w) / den;
        shelf.b1 = 2.0 * (w * w - vh) / den;
        shelf.b2 = (vh - vb * w / q + w * w) / den;
        shelf.a1 = 2.0 * (w * w - 1.0) / den;
        shelf.a2 = (1.0 - w / q + w * w) / den;
    }
    {
        const double w = std::tan(pi * 38.13547087602444 / rate), q = 0.5003270373238773;
        const double den = 1.0 + w / q + w * w;
        hp.b0 = 1.0, hp.b1 = -2.0, hp.b2 = 1.0;  // (BS.1770 leaves the numerator unnormalised)
        hp.a1 = 2.0 * (w * w - 1.0) / den;
        hp.a2 = (1.0 - w / q + w * w) / den;
    }
    FILE* in = fopen(argv[2], "rb");
    if (!in)
        return 1;
    std::vector<int16_t> x;
    int16_t buf[4096];
    for (size_t n; (n = fread(buf, 2, 4096, in)) > 0;)
        x.insert(x.end(), buf, buf + n);
    fclose(in);
    const size_t hop = (size_t)rate / 10;
    std::vector<double> hops;  // sums of z^2 over each whole 100 ms
    double sum = 0;
    for (size_t n = 0; n < x.size(); n++) {
        const double z = hp.run(shelf.run(x[n] / 32768.0));
        sum += z * z;
        if ((n + 1) % hop == 0) {
            hops.push_back(sum);
            sum = 0;
        }
    }
    FILE* out = fopen(argv[3], "wb");
    if (!out)
        return 1;
    for (size_t j = 0; j + 4 <= hops.size(); j++) {
        const double ms = (hops[j] + hops[j + 1] + hops[j + 2] + hops[j + 3]) / (4.0 * hop);
        if (fwrite(&ms, sizeof(ms), 1, out) != 1)
            return 1;
    }
    fclose(out);
    return 0;
}
