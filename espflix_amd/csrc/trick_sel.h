// trick_sel.h -- the selection rule of efx_trick_pick (k_trick.hip): which pictures of a title make its fast-forward and
// rewind streams, and where each of them goes.
//
// Host + device: the kernel and the host entry points run exactly these functions, and tests/test_trick_model.py builds
// this header with a plain C++ compiler (tests/trick_model_main.cpp) and checks it against the NumPy model
// (tests/trick_model.py).  Plain integer functions, no HIP (the definition: include/efx.h).
//
// A title is the pictures t = 0 .. total-1.  Picture t is picked iff t mod speed == 0 and is then pick k = t / speed of
// the K = ceil(total / speed) picks of the title.  A call offers the pictures first_picture .. first_picture + n - 1; its
// picks are k0 .. k0 + count - 1 with k0 = ceil(first_picture / speed).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EFX_TSEL_HD __host__ __device__
#else
#define EFX_TSEL_HD
#endif

namespace efx {
namespace tsel {

constexpr int kMaxSpeed = 255;
constexpr int64_t kMaxFirstPicture = ((int64_t)1 << 40) - 1;
constexpr int kPieceBytes = 16;
constexpr int kPiecesPerPicture = 101376 / kPieceBytes;  // 6336 pieces of 16 bytes: 4224 of luma, 1056 of each chroma plane

EFX_TSEL_HD inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }  // a >= 0, b >= 1

// picks of a whole title of `total` pictures
EFX_TSEL_HD inline int64_t total_picks(int64_t total, int speed) { return ceil_div(total, speed); }

// the first pick at or behind picture first_picture
EFX_TSEL_HD inline int64_t first_pick(int64_t first_picture, int speed) { return ceil_div(first_picture, speed); }

EFX_TSEL_HD inline bool args_ok(int64_t first_picture, int64_t n_pictures, int speed)
{
    return first_picture >= 0 && first_picture <= kMaxFirstPicture && n_pictures >= 0 && n_pictures <= INT32_MAX && speed >= 1 &&
           speed <= kMaxSpeed;
}

// picks among the pictures first_picture .. first_picture + n_pictures - 1 (may be 0); -1 for invalid arguments
EFX_TSEL_HD inline int64_t count(int64_t first_picture, int64_t n_pictures, int speed)
{
    if (!args_ok(first_picture, n_pictures, speed))
        return -1;
    return ceil_div(first_picture + n_pictures, speed) - first_pick(first_picture, speed);
}

// the call's picture (0 .. n_pictures-1) that is pick k of the title
EFX_TSEL_HD inline int64_t call_picture(int64_t k, int speed, int64_t first_picture) { return k * speed - first_picture; }

// fwd placement, call-relative: the image of the call's fwd region that receives pick k
EFX_TSEL_HD inline int64_t fwd_image(int64_t k, int64_t k0) { return k - k0; }

// rwd placement, title-absolute: the image of the rwd region (K images) that receives pick k
EFX_TSEL_HD inline int64_t rwd_image(int64_t k, int64_t K) { return K - 1 - k; }

// The kernel's item arithmetic.  An item is (stream, pick of the call, piece), the piece fastest; a workgroup moves a run of
// kRunItems consecutive items.  run_start() divides the run's first item once (wave-uniform in the kernel); locate() finds
// an item of the run from there, at most one picture further.
constexpr int kRunItems = 1024;

struct Run {
    uint64_t pic0;  // picked picture (stream x n_picks + pick) of the run's first item
    int piece0;     // ... and its piece
    int s0, i0;     // pic0's stream and pick of the call
};

EFX_TSEL_HD inline uint64_t run_count(uint64_t pictures) { return (pictures * kPiecesPerPicture + kRunItems - 1) / kRunItems; }

EFX_TSEL_HD inline Run run_start(uint64_t run, int n_picks)
{
    Run r;
    const uint64_t item0 = run * kRunItems;
    r.pic0 = item0 / kPiecesPerPicture;
    r.piece0 = (int)(item0 - r.pic0 * kPiecesPerPicture);
    r.s0 = (int)(r.pic0 / (uint64_t)n_picks);
    r.i0 = (int)(r.pic0 - (uint64_t)r.s0 * (uint64_t)n_picks);
    return r;
}

// item `local` (0 .. kRunItems-1) of the run: false past the last item of the call (pictures = n_streams x n_picks)
EFX_TSEL_HD inline bool locate(const Run& r, int local, int n_picks, uint64_t pictures, int* s, int* i, int* q)
{
    const int l = r.piece0 + local;  // < 6336 + 1024
    const bool next = l >= kPiecesPerPicture;
    if (r.pic0 + (next ? 1 : 0) >= pictures)
        return false;
    *q = next ? l - kPiecesPerPicture : l;
    *s = r.s0;
    *i = r.i0;
    if (next && ++*i == n_picks) {
        *i = 0;
        ++*s;
    }
    return true;
}

}  // namespace tsel
}  // namespace efx
