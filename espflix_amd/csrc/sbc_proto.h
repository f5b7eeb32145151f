// sbc_proto.h -- the SBC prototype filter Proto_8_80 (A2DP Appendix B), the one copy in the tree.
//
// The filter is symmetric about tap 40 except that taps 48 and 64 are the negatives of taps 32 and 16, so half of it
// is kept.  The decoder's synthesis window (efx_tables.cpp:build_sbc_tables) and the encoder's analysis window
// (sbc_enc_core.h) are both derived from it.
#pragma once

namespace efx {

constexpr double kSbcProtoHalf[41] = {
    0.00000000E+00, 1.56575398E-04, 3.43256425E-04, 5.54620202E-04, 8.23919506E-04, 1.13992507E-03,
    1.47640169E-03, 1.78371725E-03, 2.01182542E-03, 2.10371989E-03, 1.99454554E-03, 1.61656283E-03,
    9.02154502E-04, -1.78805361E-04, -1.64973098E-03, -3.49717454E-03, 5.65949473E-03, 8.02941163E-03,
    1.04584443E-02, 1.27472335E-02, 1.46525263E-02, 1.59045603E-02, 1.62208471E-02, 1.53184106E-02,
    1.29371806E-02, 8.85757540E-03, 2.92408442E-03, -4.91578024E-03, -1.46404076E-02, -2.61098752E-02,
    -3.90751381E-02, -5.31873032E-02, 6.79989431E-02, 8.29847578E-02, 9.75753918E-02, 1.11196689E-01,
    1.23264548E-01, 1.33264415E-01, 1.40753505E-01, 1.45389847E-01, 1.46955068E-01};

// Proto_8_80[n], n = 0 .. 79
constexpr double sbc_proto_tap(int n)
{
    const int h = n <= 40 ? n : 80 - n;
    return (n > 40 && (h == 16 || h == 32)) ? -kSbcProtoHalf[h] : kSbcProtoHalf[h];
}

}  // namespace efx
