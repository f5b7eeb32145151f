// k_conform.hip -- pictures at any constant rate conformed to one of the rates MPEG-1 codes (efx_conform_rate): every
// output picture is a copy of the source picture conform_sel.h names, so a source picture is dropped, kept or repeated.
//
// A memory-bound gather in k_trick's shape.  An item is 16 bytes of one output picture of one stream -- 6336 items per
// picture -- and every global access is one 16-byte load or store.  Items are numbered (stream, output, piece) with the
// piece fastest, in 64 bits.  A workgroup moves kTrickItemsPerBlock consecutive items: it divides its first item's number
// once (trick_sel.h: run_start) and finds the source pictures of the at most two output pictures its run touches, both
// wave-uniformly -- the two 64-bit divisions of conform_sel.h's source() happen once per run, none per lane or per item.
// The grid is sized from the outputs: a dropped source picture costs nothing and is never read, a repeated one is read once
// per output.
#include <hip/hip_runtime.h>

#include "conform_sel.h"
#include "efx.h"
#include "efx_internal.h"
#include "trick_sel.h"

namespace efx {

namespace {
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
static_assert(kTrickItemsPerBlock == tsel::kRunItems && tsel::kPiecesPerPicture * 16 == kFrameBytes, "k_trick's items and runs");

// A wave-uniform value pinned to scalar registers where it is computed: without it the compiler sinks the division behind
// it into every pass's lane-divergent "next picture" branch and repeats it there, per lane
__device__ inline int64_t pin_uniform(int64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
}  // namespace

__global__ __launch_bounds__(256) void k_conform(ConformArgs a)
{
    const uint64_t pictures = (uint64_t)a.n_streams * (uint64_t)a.n_out;  // output pictures of the call
    const uint64_t runs = tsel::run_count(pictures);
    const csel::Ratio ratio{a.A, a.B};
    for (uint64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const tsel::Run r = tsel::run_start(run, a.n_out);  // wave-uniform
        // the run's first output picture and the one behind it (the next stream's first when the stream ends): their
        // pictures of the call.  (Behind the call's last output nothing is located, and the index is not used.)
        const int i1 = r.i0 + 1 == a.n_out ? 0 : r.i0 + 1;
        const int64_t j0 = pin_uniform(csel::source(ratio, a.n0 + r.i0) - a.first_picture);
        const int64_t j1 = pin_uniform(csel::source(ratio, a.n0 + i1) - a.first_picture);
#pragma unroll
        for (int pass = 0; pass < kTrickItemsPerBlock / 256; pass++) {
            int s, i, q;
            if (!tsel::locate(r, pass * 256 + (int)threadIdx.x, a.n_out, pictures, &s, &i, &q))
                continue;  // past the last item of the call
            const int64_t j = i == r.i0 && s == r.s0 ? j0 : j1;
            const u32x4 v = *reinterpret_cast<const u32x4*>(a.src + (size_t)s * a.src_stride + (size_t)j * kFrameBytes + 16 * (size_t)q);
            *reinterpret_cast<u32x4*>(a.dst + (size_t)s * a.dst_stride + (size_t)i * kFrameBytes + 16 * (size_t)q) = v;
        }
    }
}

}  // namespace efx
