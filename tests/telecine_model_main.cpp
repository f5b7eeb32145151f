// TEST: whole efx_detelecine calls on the host, with telecine_px.h's functions and k_telecine's own walk -- the three
// launches in order, frames, items, the 64 lanes of a wave with their chunks, the records as the only state between the
// launches -- on heap blocks of exactly the bytes the contract names, so that a sanitizer build
// (-fsanitize=address,undefined) sees every byte the kernels' addressing would touch.
//
//   telecine_model_main call LAYOUT SHIFT SWAP W H OFF0 OFF1 OFF2 PITCH0 PITCH1 PITCH2 BYTES N_STREAMS N_FRAMES FIRST LEAD NT
//       the source images (N_STREAMS x N_FRAMES x BYTES) from stdin; to stdout the outputs (packed I420, N_STREAMS x n_out
//       of them), then the records (N_STREAMS x n of 32 bytes).  exit 1: a refused call; exit 3: a byte between the
//       output images lost its fill.
//   telecine_model_main count N_FRAMES LEAD              efx_detelecine_count as text
//   telecine_model_main tile                             the chunk, the strips of a wave and the row band as text
//   telecine_model_main stripes W H NT                   the score of a W x H plane of alternating 0 / 255 lines as text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "telecine_px.h"

using namespace efx;

namespace {

constexpr uint8_t kFill = 0xA5;
constexpr size_t kPad = 48;  // bytes between images, a multiple of 16

struct Call {
    efx_surface s;
    const uint8_t* src;
    uint8_t* dst;
    efx_telecine_info* info;
    size_t src_stride, dst_stride;
    int n_streams, n_frames, lead, n, n_out, first_field, nt;
};

const uint8_t* image(const Call& a, size_t frame, int* t)
{
    const size_t stream = frame / (size_t)a.n;
    *t = a.lead + (int)(frame - stream * (size_t)a.n);
    return a.src + (stream * (size_t)a.n_frames + (size_t)*t) * a.src_stride;
}

void measure(const Call& a, size_t frame)
{
    tpx::Measure m;
    int t;
    m.cur = image(a, frame, &t);
    m.has_prev = t > 0;
    m.prev = m.has_prev ? m.cur - a.src_stride : m.cur;
    m.end = (a.s.bytes + 15) / 16 * 16;
    m.at = dpx::plane_at(a.s, 0);
    m.w = a.s.width, m.h = a.s.height;
    m.thr2 = tpx::threshold2(a.nt);
    tpx::Sums s = {0, 0, 0};
    for (int k = 0; k < tpx::measure_items(m.w, m.h); k++)
        for (int lane = 0; lane < 64; lane++) {
            if (a.first_field == EFX_FIELD_TOP)
                tpx::measure_lane<0>(m, k, lane, &s);
            else
                tpx::measure_lane<1>(m, k, lane, &s);
        }
    a.info[frame] = tpx::measured(s, m.has_prev);
}

void decide(const Call& a, size_t stream)
{
    for (int c = 0; c * tpx::kCycle < a.n; c++) {
        const int left = a.n - c * tpx::kCycle;
        tpx::decide_cycle(a.info + stream * (size_t)a.n + (size_t)c * tpx::kCycle, left < tpx::kCycle ? left : tpx::kCycle, c * (tpx::kCycle - 1));
    }
}

void weave(const Call& a, size_t frame)
{
    const efx_telecine_info r = a.info[frame];
    if (r.out < 0 || r.out >= a.n_out)
        return;
    int t;
    const uint8_t* cur = image(a, frame, &t);
    const uint8_t* other = r.match && t > 0 ? cur - a.src_stride : cur;
    uint8_t* out = a.dst + ((frame / (size_t)a.n) * (size_t)a.n_out + (size_t)r.out) * a.dst_stride;
    for (int k = 0; k < tpx::weave_items(a.s); k++)
        for (int lane = 0; lane < 64; lane++)
            tpx::weave_lane(a.s, cur, other, (a.s.bytes + 15) / 16 * 16, out, a.first_field == EFX_FIELD_TOP ? 0 : 1, k, lane);
}

int call(char** v)
{
    Call a = {};
    efx_surface& s = a.s;
    s.layout = atoi(v[0]), s.shift = atoi(v[1]), s.swap_uv = atoi(v[2]), s.width = atoi(v[3]), s.height = atoi(v[4]);
    for (int i = 0; i < 3; i++)
        s.offset[i] = strtoull(v[5 + i], nullptr, 10), s.pitch[i] = strtoull(v[8 + i], nullptr, 10);
    s.bytes = strtoull(v[11], nullptr, 10);
    a.n_streams = atoi(v[12]), a.n_frames = atoi(v[13]), a.first_field = atoi(v[14]), a.lead = atoi(v[15]), a.nt = atoi(v[16]);
    a.n = tpx::processed(a.n_frames, a.lead), a.n_out = tpx::count(a.n_frames, a.lead);
    if (!dpx::surface_ok(s) || a.n < 0 || a.n_streams < 1 || (a.first_field != EFX_FIELD_TOP && a.first_field != EFX_FIELD_BOTTOM) || a.nt < 0 ||
        a.nt > 255)
        return 1;
    // blocks of exactly the bytes the contract names: the last image ends where its bytes (rounded up to 16) end
    const size_t n_in = (size_t)a.n_streams * a.n_frames, total_out = (size_t)a.n_streams * a.n_out, frames = (size_t)a.n_streams * a.n;
    const size_t image = (size_t)s.width * s.height * 3 / 2;
    a.src_stride = (s.bytes + 15) / 16 * 16 + kPad;
    a.dst_stride = (image + 15) / 16 * 16 + kPad;
    const size_t src_bytes = (n_in - 1) * a.src_stride + (s.bytes + 15) / 16 * 16;
    const size_t dst_bytes = (total_out - 1) * a.dst_stride + image;
    std::unique_ptr<uint8_t[]> src(new uint8_t[src_bytes]), dst(new uint8_t[dst_bytes]);
    std::unique_ptr<efx_telecine_info[]> info(new efx_telecine_info[frames]);
    memset(src.get(), 0x5A, src_bytes);
    memset(dst.get(), kFill, dst_bytes);
    memset(info.get(), kFill, frames * sizeof(efx_telecine_info));
    for (size_t k = 0; k < n_in; k++)
        if (fread(src.get() + k * a.src_stride, 1, s.bytes, stdin) != s.bytes)
            return 2;
    a.src = src.get(), a.dst = dst.get(), a.info = info.get();
    for (size_t frame = 0; frame < frames; frame++)
        measure(a, frame);
    for (size_t stream = 0; stream < (size_t)a.n_streams; stream++)
        decide(a, stream);
    for (size_t frame = 0; frame < frames; frame++)
        weave(a, frame);
    for (size_t k = 0; k < total_out; k++) {
        fwrite(dst.get() + k * a.dst_stride, 1, image, stdout);
        if (k + 1 < total_out)
            for (size_t b = image; b < a.dst_stride; b++)
                if (dst[k * a.dst_stride + b] != kFill)
                    return fprintf(stderr, "a byte behind output %zu lost its fill\n", k), 3;
    }
    fwrite(info.get(), sizeof(efx_telecine_info), frames, stdout);
    return 0;
}

int stripes(int w, int h, int nt)
{
    std::unique_ptr<uint8_t[]> y(new uint8_t[(size_t)w * h]);
    for (int r = 0; r < h; r++)
        memset(y.get() + (size_t)r * w, r & 1 ? 255 : 0, (size_t)w);
    printf("%llu\n", (unsigned long long)tpx::score_plane(y.get(), (size_t)w, w, h, nt));
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    const std::string mode = argv[1];
    if (mode == "call" && argc == 19)
        return call(argv + 2);
    if (mode == "count" && argc == 4)
        return printf("%d\n", tpx::count(atoi(argv[2]), atoi(argv[3]))), 0;
    if (mode == "tile")
        return printf("%d %d %d\n", tpx::kChunk, tpx::kWaveStrips, tpx::kBandRows), 0;
    if (mode == "stripes" && argc == 5)
        return stripes(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    return 2;
}
