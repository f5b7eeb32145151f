// k_trick.hip -- the pictures of a title that make its fast-forward and rewind streams (efx_trick_pick): every speed-th
// picture, gathered from I420 pictures in device memory or straight from the frame rings, placed in playing order for the
// fast-forward encoder and in reverse order for the rewind encoder.  The rule is trick_sel.h's.
//
// A memory-bound gather.  An item is 16 bytes of one picked picture of one stream -- 6336 items per picture -- and every
// global access is one 16-byte load or store: an item is loaded once and stored once per destination.  Items are numbered
// (stream, pick, piece) with the piece fastest, in 64 bits: 1024 streams x a few thousand picks pass 2^32 bytes.  A
// workgroup moves kTrickItemsPerBlock consecutive items; it divides its first item's number once, wave-uniformly, and a
// lane only steps over at most one picture boundary from there (trick_sel.h: run_start, locate).  The grid is sized from
// the picks, never from the pictures offered: an unpicked picture costs nothing and is never read.
//
// Ring source: a picked picture is what efx_export_frames(EFX_PIX_I420, slot = -1) writes, the strip layout un-shuffled
// with ring_px.h's row offsets and the stream's ring slot read from the record the most recent decode left.
#include <hip/hip_runtime.h>

#include "efx.h"
#include "efx_internal.h"
#include "ring_px.h"
#include "trick_sel.h"

namespace efx {

namespace {

constexpr int kPieces = tsel::kPiecesPerPicture;
constexpr int kLumaPieces = EFX_FRAME_WIDTH * EFX_FRAME_HEIGHT / 16;  // 4224: 22 per luma row
constexpr int kChromaPieces = kLumaPieces / 4;                        // 1056 per plane: 11 per chroma row
static_assert(kTrickItemsPerBlock == tsel::kRunItems, "a workgroup moves one run");
static_assert(kLumaPieces + 2 * kChromaPieces == kPieces && kPieces * 16 == kFrameBytes, "an I420 picture in 16-byte pieces");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// where piece q of a picture's I420 image lies in its ring frame (k_export's I420 branch, one piece at a time)
__device__ inline int ring_piece_off(int q)
{
    if (q < kLumaPieces) {
        const int y = q / 22;
        return ring::luma_row_off(y) + 16 * (q - 22 * y);
    }
    q -= kLumaPieces;
    const int plane = q < kChromaPieces ? 1 : 2;
    if (plane == 2)
        q -= kChromaPieces;
    const int c = q / 11;
    return ring::chroma_row_off(plane, c) + 16 * (q - 11 * c);
}

}  // namespace

template <int SOURCE>
__global__ __launch_bounds__(256) void k_trick(TrickArgs a)
{
    const uint64_t pictures = (uint64_t)a.n_streams * (uint64_t)a.n_picks;  // picked pictures of the call
    const uint64_t runs = tsel::run_count(pictures);
    for (uint64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const tsel::Run r = tsel::run_start(run, a.n_picks);  // wave-uniform
#pragma unroll
        for (int pass = 0; pass < kTrickItemsPerBlock / 256; pass++) {
            int s, i, q;
            if (!tsel::locate(r, pass * 256 + (int)threadIdx.x, a.n_picks, pictures, &s, &i, &q))
                continue;  // past the last item of the call
            const int64_t k = a.k0 + i;                                                     // pick of the title
            const int64_t j = tsel::call_picture(k, a.speed, a.first_picture);              // picture of the call
            u32x4 v;
            if (SOURCE == EFX_TRICK_FROM_RING) {
                const int stream = a.first_stream + s;
                const int slot = ring::picture_slot(a, stream, (int)j);
                const uint8_t* fr = a.src + ((size_t)stream * a.ring_depth + slot) * kFrameBytes;
                v = *reinterpret_cast<const u32x4*>(fr + ring_piece_off(q));
            } else {
                v = *reinterpret_cast<const u32x4*>(a.src + (size_t)s * a.src_stride + (size_t)j * kFrameBytes + 16 * (size_t)q);
            }
            if (a.fwd)
                *reinterpret_cast<u32x4*>(a.fwd + (size_t)s * a.fwd_stride + (size_t)tsel::fwd_image(k, a.k0) * kFrameBytes +
                                          16 * (size_t)q) = v;
            if (a.rwd)
                *reinterpret_cast<u32x4*>(a.rwd + (size_t)s * a.rwd_stride + (size_t)tsel::rwd_image(k, a.K) * kFrameBytes +
                                          16 * (size_t)q) = v;
        }
    }
}

template __global__ void k_trick<EFX_TRICK_FROM_I420>(TrickArgs);
template __global__ void k_trick<EFX_TRICK_FROM_RING>(TrickArgs);

}  // namespace efx
