// TEST: whole efx_denoise calls on the host, with denoise_px.h's functions and k_denoise's own walk -- items, the 64 lanes
// of a wave with their chunks, the halo words from the neighbouring lanes, the band's rows with a row either side, the
// previous output kept per lane from frame to frame -- on heap blocks of exactly the bytes the contract names, so that a
// sanitizer build (-fsanitize=address,undefined) sees every byte the kernel's addressing would touch.
//
//   denoise_model_main call LAYOUT SHIFT SWAP W H OFF0 OFF1 OFF2 PITCH0 PITCH1 PITCH2 BYTES N_STREAMS N_FRAMES LS CS LT CT HAS_PREV
//       the source images (N_STREAMS x N_FRAMES x BYTES), then with HAS_PREV = 1 the streams' previous outputs (N_STREAMS
//       packed I420 pictures) from stdin; the outputs (packed I420, N_STREAMS x N_FRAMES of them) to stdout.
//       exit 1: a refused call; exit 3: a byte between the output images lost its fill.
//   denoise_model_main blend                             the temporal step's output for Tt = 1 .. 64 and all s, P in
//                                                        0 .. 255 (64 x 256 x 256 bytes) to stdout
//   denoise_model_main tile                              the column tile and the row band as text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "denoise_px.h"

using namespace efx;

namespace {

constexpr uint8_t kFill = 0xA5;
constexpr size_t kPad = 48;  // bytes between images, a multiple of 16

struct Call {
    efx_surface s;
    const uint8_t *src, *prev;
    uint8_t* dst;
    size_t src_stride, dst_stride, prev_stride;
    int n_streams, n_frames, ts[2], tt[2];
};

struct Lane {
    int plane, X, n;
    bool active, halo;
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

dpx::Chunk fetch(const efx_surface& s, const uint8_t* img, size_t end, int ph, int r, const Lane& l)
{
    const dpx::PlaneAt at = dpx::plane_at(s, l.plane);
    const int row = npx::clamp_row(r, ph);
    if (!at.pairs)  // (a lane with nothing to fetch loads the row's first chunk, as the kernel does: nobody looks at it)
        return npx::settle_plain(npx::load_plain(at, img, end, row, l.active ? l.X : 0), at, end, row, l.active ? l.X : 0);
    dpx::Chunk c = {};
    if (l.active)
        c = dpx::fetch_row(at, img, end, row, l.X, l.n);
    return c;
}

// row r of lane `lane` with the halo words of lanes lane - 1 and lane + 1 (a shuffle from beyond the wave gives the
// lane's own word; such a lane writes nothing)
dpx::Ext wide_row(const efx_surface& s, const uint8_t* img, size_t end, int pw, int ph, int r, const dpx::Item& it, int lane)
{
    const Lane me = lane_of(it, lane, pw);
    const dpx::Chunk c = fetch(s, img, end, ph, r, me);
    const dpx::Chunk left = lane > 0 ? fetch(s, img, end, ph, r, lane_of(it, lane - 1, pw)) : c;
    const dpx::Chunk right = lane < 63 ? fetch(s, img, end, ph, r, lane_of(it, lane + 1, pw)) : c;
    return npx::widen_row(c, left.d[3], right.d[0], me.active, me.X, me.n);
}

void run_item(const Call& a, size_t stream, int k)
{
    const efx_surface& s = a.s;
    const dpx::Item it = npx::item(s.width, s.height, k);
    const int pw = dpx::plane_w(s.width, it.plane), ph = dpx::plane_h(s.height, it.plane);
    const size_t end = (s.bytes + 15) / 16 * 16;
    const size_t image = (size_t)s.width * s.height * 3 / 2;
    const npx::Plane thr = npx::plane_of(a.ts[it.plane ? 1 : 0], a.tt[it.plane ? 1 : 0]);
    const int y0 = it.band * npx::kBandRows;
    const int nr = ph - y0 < npx::kBandRows ? ph - y0 : npx::kBandRows;
    for (int lane = 0; lane < 64; lane++) {
        const Lane l = lane_of(it, lane, pw);
        if (!l.active || l.halo)
            continue;
        const size_t plane_first = dpx::out_plane(s.width, s.height, l.plane);
        dpx::Chunk P[npx::kBandRows] = {};
        bool has_prev = a.prev != nullptr;
        if (has_prev)
            for (int r = 0; r < nr; r++)
                P[r] = npx::fetch_prev(a.prev + stream * a.prev_stride, (image + 15) / 16 * 16, plane_first, pw, y0 + r, l.X);
        for (int t = 0; t < a.n_frames; t++) {
            const uint8_t* img = a.src + (stream * (size_t)a.n_frames + (size_t)t) * a.src_stride;
            uint8_t* out = a.dst + (stream * (size_t)a.n_frames + (size_t)t) * a.dst_stride + plane_first + (size_t)y0 * pw + l.X;
            for (int r = 0; r < nr; r++) {
                const dpx::Ext up = wide_row(s, img, end, pw, ph, y0 + r - 1, it, lane);
                const dpx::Ext mid = wide_row(s, img, end, pw, ph, y0 + r, it, lane);
                const dpx::Ext dn = wide_row(s, img, end, pw, ph, y0 + r + 1, it, lane);
                P[r] = npx::row_out(up, mid, dn, P[r], has_prev, thr);
                dpx::store_chunk(out + (size_t)r * pw, P[r], l.n);
            }
            has_prev = true;
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
    a.n_streams = atoi(v[12]), a.n_frames = atoi(v[13]);
    a.ts[0] = atoi(v[14]), a.ts[1] = atoi(v[15]), a.tt[0] = atoi(v[16]), a.tt[1] = atoi(v[17]);
    const bool has_prev = atoi(v[18]) != 0;
    if (!npx::surface_ok(s) || a.n_streams < 1 || a.n_frames < 1)
        return 1;
    for (int i = 0; i < 2; i++)
        if (!npx::threshold_ok(a.ts[i]) || !npx::threshold_ok(a.tt[i]))
            return 1;
    // blocks of exactly the bytes the contract names: the last image ends where its bytes (rounded up to 16) end
    const size_t n = (size_t)a.n_streams * a.n_frames;
    const size_t image = (size_t)s.width * s.height * 3 / 2;
    a.src_stride = (s.bytes + 15) / 16 * 16 + kPad;
    a.dst_stride = (image + 15) / 16 * 16 + kPad;
    a.prev_stride = a.dst_stride;
    const size_t src_bytes = (n - 1) * a.src_stride + (s.bytes + 15) / 16 * 16;
    const size_t dst_bytes = (n - 1) * a.dst_stride + image;
    const size_t prev_bytes = ((size_t)a.n_streams - 1) * a.prev_stride + (image + 15) / 16 * 16;
    std::unique_ptr<uint8_t[]> src(new uint8_t[src_bytes]), dst(new uint8_t[dst_bytes]), prev(new uint8_t[prev_bytes]);
    memset(src.get(), 0x5A, src_bytes);
    memset(dst.get(), kFill, dst_bytes);
    memset(prev.get(), 0x3C, prev_bytes);
    for (size_t k = 0; k < n; k++)
        if (fread(src.get() + k * a.src_stride, 1, s.bytes, stdin) != s.bytes)
            return 2;
    if (has_prev)
        for (int i = 0; i < a.n_streams; i++)
            if (fread(prev.get() + i * a.prev_stride, 1, image, stdin) != image)
                return 2;
    a.src = src.get(), a.dst = dst.get(), a.prev = has_prev ? prev.get() : nullptr;
    const int items = npx::stream_items(s.width, s.height);
    for (size_t stream = 0; stream < (size_t)a.n_streams; stream++)
        for (int k = 0; k < items; k++)
            run_item(a, stream, k);
    for (size_t k = 0; k < n; k++) {
        fwrite(dst.get() + k * a.dst_stride, 1, image, stdout);
        if (k + 1 < n)
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
    if (mode == "call" && argc == 21)
        return call(argv + 2);
    if (mode == "blend") {
        // the temporal step for Tt = 1 .. 64 and all s, P in 0 .. 255, two samples at a time as the kernel takes them
        std::vector<uint8_t> out(64 * 65536);
        for (int tt = 1; tt <= 64; tt++)
            for (uint32_t s = 0; s < 256; s++)
                for (uint32_t p = 0; p < 256; p += 2) {
                    const uint32_t o = npx::temporal2(s * 0x00010001u, p | ((p + 1) << 16), tt, npx::blend_q(tt));
                    uint8_t* at = &out[((size_t)(tt - 1) * 256 + s) * 256 + p];
                    at[0] = (uint8_t)o, at[1] = (uint8_t)(o >> 16);
                    if ((o & 0xFF00FF00u) != 0)
                        return 3;
                }
        return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 2;
    }
    if (mode == "tile")
        return printf("%d %d\n", npx::kTileCols, npx::kBandRows), 0;
    return 2;
}
