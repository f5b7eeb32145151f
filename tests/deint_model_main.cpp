// TEST: whole efx_deinterlace calls on the host, with deint_px.h's functions and k_deint's own walk -- items, the 64 lanes
// of a wave with their chunks, the halo words from the neighbouring lanes, the rows a missing row reads and the rows the
// kernel leaves out -- on heap blocks of exactly the bytes the contract names, so that a sanitizer build
// (-fsanitize=address,undefined) sees every byte the kernel's addressing would touch.
//
//   deint_model_main call LAYOUT SHIFT SWAP W H OFF0 OFF1 OFF2 PITCH0 PITCH1 PITCH2 BYTES N_STREAMS N_FRAMES FIRST MODE LEAD TAIL
//       the source images (N_STREAMS x N_FRAMES x BYTES) from stdin; the outputs (packed I420, N_STREAMS x n_out of
//       them) to stdout.  exit 1: a refused call; exit 3: a byte between the output images lost its fill.
//   deint_model_main count N_FRAMES LEAD TAIL MODE       efx_deinterlace_count as text
//   deint_model_main tile                                the column tile and the row band as text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "deint_px.h"

using namespace efx;

namespace {

constexpr uint8_t kFill = 0xA5;
constexpr size_t kPad = 48;  // bytes between images, a multiple of 16

struct Call {
    efx_surface s;
    const uint8_t* src;
    uint8_t* dst;
    size_t src_stride, dst_stride;
    int n_streams, n_frames, lead, frames_out, per_frame, first_field;
};

struct Lane {
    int plane, X, n;
    bool active, halo;
};

struct Frame3 {
    const uint8_t *prev, *cur, *next;
    size_t end;
};

Lane lane_of(const dpx::Item& it, int lane, int pw)
{
    const dpx::Place p = dpx::place(it, lane);
    Lane l;
    l.plane = p.plane, l.X = p.X, l.halo = p.halo;
    l.n = pw - l.X;
    l.active = l.X >= 0 && l.n > 0;
    return l;
}

dpx::Chunk fetch(const efx_surface& s, const uint8_t* img, size_t end, int ph, int r, const Lane& l, bool needed)
{
    dpx::Chunk c = {};
    if (l.active && needed)
        c = dpx::fetch_row(dpx::plane_at(s, l.plane), img, end, dpx::reflect(r, ph), l.X, l.n);
    return c;
}

// a cur row of lane `lane` with the halo words of lanes lane - 1 and lane + 1 (a shuffle from beyond the wave gives the
// lane's own word; such a lane writes nothing)
dpx::Ext cur_row(const efx_surface& s, const Frame3& f, int pw, int ph, int r, const dpx::Item& it, int lane)
{
    const Lane me = lane_of(it, lane, pw);
    const dpx::Chunk c = fetch(s, f.cur, f.end, ph, r, me, true);
    const dpx::Chunk left = lane > 0 ? fetch(s, f.cur, f.end, ph, r, lane_of(it, lane - 1, pw), true) : c;
    const dpx::Chunk right = lane < 63 ? fetch(s, f.cur, f.end, ph, r, lane_of(it, lane + 1, pw), true) : c;
    dpx::Ext x;
    x.e[0] = left.d[3], x.e[5] = right.d[0];
    for (int i = 0; i < 4; i++)
        x.e[1 + i] = c.d[i];
    if (me.active)
        dpx::clamp_cols(&x, me.X, me.n);
    return x;
}

void run_item(const Call& a, size_t frame, int k)
{
    const efx_surface& s = a.s;
    const dpx::Item it = dpx::item(s.width, s.height, k);
    const int pw = dpx::plane_w(s.width, it.plane), ph = dpx::plane_h(s.height, it.plane);
    const size_t stream = frame / (size_t)a.frames_out;
    const int jo = (int)(frame - stream * (size_t)a.frames_out), j = a.lead + jo;
    const uint8_t* first = a.src + stream * (size_t)a.n_frames * a.src_stride;
    Frame3 f;
    f.cur = first + (size_t)j * a.src_stride;
    f.prev = first + (size_t)(j > 0 ? j - 1 : j) * a.src_stride;
    f.next = first + (size_t)(j + 1 < a.n_frames ? j + 1 : j) * a.src_stride;
    f.end = (s.bytes + 15) / 16 * 16;
    const size_t n_out = (size_t)a.frames_out * a.per_frame;
    uint8_t* image0 = a.dst + (stream * n_out + (size_t)jo * a.per_frame) * a.dst_stride;
    const int keep[2] = {dpx::keeper(a.first_field, a.per_frame, 0), dpx::keeper(a.first_field, a.per_frame, 1)};
    const int miss[2] = {keep[1], keep[0]};
    bool need_prev[2], need_next[2];
    for (int q = 0; q < 2; q++) {
        need_prev[q] = miss[1 - q] >= 0 || miss[q] == 0;
        need_next[q] = miss[1 - q] >= 0 || miss[q] == 1;
    }
    const int y0 = it.band * dpx::kBandRows;
    const int y1 = y0 + dpx::kBandRows < ph ? y0 + dpx::kBandRows : ph;
    for (int lane = 0; lane < 64; lane++) {
        const Lane l = lane_of(it, lane, pw);
        if (!l.active || l.halo)
            continue;
        uint8_t* out0 = image0 + dpx::out_plane(s.width, s.height, l.plane);
        for (int y = y0; y < y1; y++) {
            const int q = y & 1;
            const size_t where = (size_t)y * pw + l.X;
            dpx::Ext C[5];
            dpx::Chunk P[5], N[5];
            for (int i = 0; i < 5; i++) {
                const int r = y - 2 + i, par = dpx::reflect(r, ph) & 1;
                C[i] = cur_row(s, f, pw, ph, r, it, lane);
                P[i] = fetch(s, f.prev, f.end, ph, r, l, need_prev[par]);
                N[i] = fetch(s, f.next, f.end, ph, r, l, need_next[par]);
            }
            if (keep[q] >= 0) {
                dpx::Chunk c;
                for (int i = 0; i < 4; i++)
                    c.d[i] = C[2].e[1 + i];
                dpx::store_chunk(out0 + keep[q] * a.dst_stride + where, c, l.n);
            }
            if (miss[q] >= 0) {
                const bool b_prev = miss[q] == 0;
                dpx::Chunk o;
                for (int i = 0; i < 4; i++) {
                    dpx::Rows r;
                    for (int w = 0; w < 3; w++)
                        r.up[w] = C[1].e[i + w], r.dn[w] = C[3].e[i + w];
                    r.pu = P[1].d[i], r.pd = P[3].d[i], r.nu = N[1].d[i], r.nd = N[3].d[i];
                    r.bm = b_prev ? P[0].d[i] : C[0].e[1 + i], r.b0 = b_prev ? P[2].d[i] : C[2].e[1 + i];
                    r.bp = b_prev ? P[4].d[i] : C[4].e[1 + i];
                    r.am = b_prev ? C[0].e[1 + i] : N[0].d[i], r.a0 = b_prev ? C[2].e[1 + i] : N[2].d[i];
                    r.ap = b_prev ? C[4].e[1 + i] : N[4].d[i];
                    o.d[i] = dpx::missing4(r);
                }
                dpx::store_chunk(out0 + miss[q] * a.dst_stride + where, o, l.n);
            }
        }
    }
}

int call(char** v)
{
    Call a = {};
    efx_surface& s = a.s;
    s.layout = atoi(v[0]), s.shift = atoi(v[1]), s.swap_uv = atoi(v[2]), s.width = atoi(v[3]), s.height = atoi(v[4]);
    for (int i = 0; i < 3; i++)
        s.offset[i] = strtoull(v[5 + i], nullptr, 10), s.pitch[i] = strtoull(v[8 + i], nullptr, 10);
    s.bytes = strtoull(v[11], nullptr, 10);
    a.n_streams = atoi(v[12]), a.n_frames = atoi(v[13]), a.first_field = atoi(v[14]);
    const int mode = atoi(v[15]), tail = atoi(v[17]);
    a.lead = atoi(v[16]);
    const int n_out = dpx::count(a.n_frames, a.lead, tail, mode);
    if (!dpx::surface_ok(s) || n_out < 0 || a.n_streams < 1 || (a.first_field != EFX_FIELD_TOP && a.first_field != EFX_FIELD_BOTTOM))
        return 1;
    a.frames_out = a.n_frames - a.lead - tail;
    a.per_frame = mode == EFX_DEINT_FIELD ? 2 : 1;
    // blocks of exactly the bytes the contract names: the last image ends where its bytes (rounded up to 16) end
    const size_t n_in = (size_t)a.n_streams * a.n_frames, total_out = (size_t)a.n_streams * n_out;
    const size_t image = (size_t)s.width * s.height * 3 / 2;
    a.src_stride = (s.bytes + 15) / 16 * 16 + kPad;
    a.dst_stride = (image + 15) / 16 * 16 + kPad;
    const size_t src_bytes = (n_in - 1) * a.src_stride + (s.bytes + 15) / 16 * 16;
    const size_t dst_bytes = (total_out - 1) * a.dst_stride + image;
    std::unique_ptr<uint8_t[]> src(new uint8_t[src_bytes]), dst(new uint8_t[dst_bytes]);
    memset(src.get(), 0x5A, src_bytes);
    memset(dst.get(), kFill, dst_bytes);
    for (size_t k = 0; k < n_in; k++)
        if (fread(src.get() + k * a.src_stride, 1, s.bytes, stdin) != s.bytes)
            return 2;
    a.src = src.get(), a.dst = dst.get();
    const int items = dpx::frame_items(s.width, s.height);
    for (size_t frame = 0; frame < (size_t)a.n_streams * a.frames_out; frame++)
        for (int k = 0; k < items; k++)
            run_item(a, frame, k);
    for (size_t k = 0; k < total_out; k++) {
        fwrite(dst.get() + k * a.dst_stride, 1, image, stdout);
        if (k + 1 < total_out)
            for (size_t b = image; b < a.dst_stride; b++)
                if (dst[k * a.dst_stride + b] != kFill)
                    return fprintf(stderr, "a byte behind output %zu lost its fill\n", k), 3;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    const std::string mode = argv[1];
    if (mode == "call" && argc == 20)
        return call(argv + 2);
    if (mode == "count" && argc == 6)
        return printf("%d\n", dpx::count(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]))), 0;
    if (mode == "tile")
        return printf("%d %d\n", dpx::kTileCols, dpx::kBandRows), 0;
    return 2;
}
