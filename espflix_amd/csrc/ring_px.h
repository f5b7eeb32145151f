// ring_px.h -- where the rows of a picture lie in a ring frame, and which ring slot holds a picture of the most recent
// decode: the address arithmetic k_export.hip and k_trick.hip share.  Device only.
//
// The ring holds pictures in the reference's strip layout (12 strips x 16 rows x 528 bytes; a row is 352 luma bytes and
// 176 bytes of ONE chroma plane: strip rows 0-7 carry Cb, 8-15 Cr; see include/efx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efx.h"
#include "efx_internal.h"

namespace efx {
namespace ring {

__device__ inline int luma_row_off(int y) { return (y >> 4) * kStripBytes + (y & 15) * kStride; }
// plane 1 = Cb (U): strip rows 0-7; plane 2 = Cr (V): strip rows 8-15 (k_video.hip's accessor)
__device__ inline int chroma_row_off(int plane, int c)
{
    return (c >> 3) * kStripBytes + ((c & 7) + (plane == 2 ? 8 : 0)) * kStride + EFX_FRAME_WIDTH;
}

// Picture mode: the ring slot of picture `picture` of the most recent efx_decode* of `stream`, from the ring position
// k_advance recorded for the stream's group (efx_stream_picture_slot's arithmetic).  A = ExportArgs or TrickArgs: the
// launch arguments carry n_groups, group_first[], call_pos[] and ring_depth by value.
template <class A>
__device__ inline int picture_slot(const A& a, int stream, int picture)
{
    const int32_t* cp = a.call_pos[0];
#pragma unroll
    for (int i = 1; i < kExportMaxGroups; i++)
        if (i < a.n_groups && stream >= a.group_first[i])
            cp = a.call_pos[i];
    const int pos0 = cp[2 * stream], f = cp[2 * stream + 1];
    const uint32_t q = (uint32_t)pos0 + (uint32_t)(f < 0 ? picture + 1 : max(0, picture - f));
    return (int)(q % (uint32_t)a.ring_depth);
}

}  // namespace ring
}  // namespace efx
