// TEST: whole efx_detect_scan calls on the host, with scan_px.h's functions and k_scan's own walk -- the two launches in
// order, frames, items, the 64 lanes of a wave with their chunks, the frame records as the only state between the
// launches -- on a heap block of exactly the bytes the contract names, so that a sanitizer build
// (-fsanitize=address,undefined) sees every byte the kernel's addressing would touch.
//
//   scan_model_main call LAYOUT SHIFT SWAP W H OFF0 OFF1 OFF2 PITCH0 PITCH1 PITCH2 BYTES N_STREAMS N_FRAMES LEAD ACCUMULATE
//                        NT STILL PROG INTL REP FIRST_FRAME
//       the source images (N_STREAMS x N_FRAMES x BYTES) from stdin, then what recs_device holds (N_STREAMS x 64 bytes); to
//       stdout the frame records (N_STREAMS x n of 48 bytes), then the stream records (N_STREAMS of 64 bytes).
//       exit 1: a refused call.
//   scan_model_main label CC CTB CBT DT DB W H STILL PROG INTL REP      "label repeat" as text
//   scan_model_main verdict then 16 words of a record                  "verdict first_field" as text (-1: not written)
//   scan_model_main tile                                               the chunk, the strips of a wave and the row band as text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "scan_px.h"

using namespace efx;

namespace {

constexpr size_t kPad = 48;  // bytes between images, a multiple of 16

struct Call {
    efx_surface s;
    efx_scan_opts o;
    const uint8_t* src;
    efx_scan_frame* frames;
    efx_scan_rec* recs;
    size_t src_stride;
    int n;
};

void measure(const Call& a, size_t frame)
{
    const size_t stream = frame / (size_t)a.n;
    const int t = a.o.lead + (int)(frame - stream * (size_t)a.n);
    scpx::Measure m;
    m.cur = a.src + (stream * (size_t)a.o.n_frames + (size_t)t) * a.src_stride;
    m.has_prev = true;
    m.prev = t > 0 ? m.cur - a.src_stride : m.cur;
    m.end = (a.s.bytes + 15) / 16 * 16;
    m.at = dpx::plane_at(a.s, 0);
    m.w = a.s.width, m.h = a.s.height;
    m.thr2 = tpx::threshold2(a.o.nt);
    scpx::Sums s = {0, 0, 0, 0, 0};
    if (t > 0)
        for (int k = 0; k < scpx::measure_items(m.w, m.h); k++)
            for (int lane = 0; lane < 64; lane++)
                scpx::measure_lane(m, k, lane, &s);
    a.frames[frame] = scpx::measured(s, t > 0, scpx::rule_of(a.o, m.w, m.h));
}

void count(const Call& a, size_t stream)
{
    uint32_t add[scpx::kSlots] = {};
    for (int j = 0; j < a.n; j++) {
        const efx_scan_frame& f = a.frames[stream * (size_t)a.n + j];
        const int ls = scpx::label_slot(f), rs = scpx::repeat_slot(f, scpx::phase_of(a.o.first_frame, a.o.lead + j));
        if (ls >= 0)
            add[ls]++;
        if (rs >= 0)
            add[rs]++;
    }
    uint32_t rec[16];
    memcpy(rec, a.recs + stream, sizeof rec);
    for (int k = 0; k < scpx::kSlots; k++)
        rec[k] = (a.o.accumulate ? rec[k] : 0u) + add[k];
    rec[scpx::kSlots] = 0;
    memcpy(a.recs + stream, rec, sizeof rec);
}

int call(char** v)
{
    Call a = {};
    efx_surface& s = a.s;
    s.layout = atoi(v[0]), s.shift = atoi(v[1]), s.swap_uv = atoi(v[2]), s.width = atoi(v[3]), s.height = atoi(v[4]);
    for (int i = 0; i < 3; i++)
        s.offset[i] = strtoull(v[5 + i], nullptr, 10), s.pitch[i] = strtoull(v[8 + i], nullptr, 10);
    s.bytes = strtoull(v[11], nullptr, 10);
    efx_scan_opts& o = a.o;
    o.n_streams = atoi(v[12]), o.n_frames = atoi(v[13]), o.lead = atoi(v[14]), o.accumulate = atoi(v[15]);
    o.nt = atoi(v[16]), o.still = atoi(v[17]), o.prog = atoi(v[18]), o.intl = atoi(v[19]), o.rep = atoi(v[20]);
    o.first_frame = strtoull(v[21], nullptr, 10);
    a.n = tpx::processed(o.n_frames, o.lead);
    if (!dpx::surface_ok(s) || a.n < 0 || o.n_streams < 1 || !scpx::options_ok(o))
        return 1;
    // a block of exactly the bytes the contract names: the last image ends where its bytes (rounded up to 16) end
    const size_t n_in = (size_t)o.n_streams * o.n_frames, frames = (size_t)o.n_streams * a.n;
    a.src_stride = (s.bytes + 15) / 16 * 16 + kPad;
    const size_t src_bytes = (n_in - 1) * a.src_stride + (s.bytes + 15) / 16 * 16;
    std::unique_ptr<uint8_t[]> src(new uint8_t[src_bytes]);
    std::unique_ptr<efx_scan_frame[]> recs_f(new efx_scan_frame[frames]);
    std::unique_ptr<efx_scan_rec[]> recs(new efx_scan_rec[o.n_streams]);
    memset(src.get(), 0x5A, src_bytes);
    memset(recs_f.get(), 0xA5, frames * sizeof(efx_scan_frame));
    for (size_t k = 0; k < n_in; k++)
        if (fread(src.get() + k * a.src_stride, 1, s.bytes, stdin) != s.bytes)
            return 2;
    if (fread(recs.get(), sizeof(efx_scan_rec), (size_t)o.n_streams, stdin) != (size_t)o.n_streams)
        return 2;
    a.src = src.get(), a.frames = recs_f.get(), a.recs = recs.get();
    for (size_t frame = 0; frame < frames; frame++)
        measure(a, frame);
    for (size_t stream = 0; stream < (size_t)o.n_streams; stream++)
        count(a, stream);
    fwrite(recs_f.get(), sizeof(efx_scan_frame), frames, stdout);
    fwrite(recs.get(), sizeof(efx_scan_rec), (size_t)o.n_streams, stdout);
    return 0;
}

int label(char** v)
{
    scpx::Sums s;
    s.cc = strtoull(v[0], nullptr, 10), s.ctb = strtoull(v[1], nullptr, 10), s.cbt = strtoull(v[2], nullptr, 10);
    s.dt = strtoull(v[3], nullptr, 10), s.db = strtoull(v[4], nullptr, 10);
    efx_scan_opts o = {};
    o.still = atoi(v[7]), o.prog = atoi(v[8]), o.intl = atoi(v[9]), o.rep = atoi(v[10]);
    int32_t lab, repeat;
    scpx::label(s, scpx::rule_of(o, atoi(v[5]), atoi(v[6])), &lab, &repeat);
    printf("%d %d\n", lab, repeat);
    return 0;
}

int verdict(char** v)
{
    uint32_t w[16];
    for (int i = 0; i < 16; i++)
        w[i] = (uint32_t)strtoul(v[i], nullptr, 10);
    efx_scan_rec r;
    memcpy(&r, w, sizeof r);
    int first_field = -1;
    const int kind = scpx::verdict(r, &first_field);
    printf("%d %d\n", kind, first_field);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    const std::string mode = argv[1];
    if (mode == "call" && argc == 24)
        return call(argv + 2);
    if (mode == "label" && argc == 13)
        return label(argv + 2);
    if (mode == "verdict" && argc == 18)
        return verdict(argv + 2);
    if (mode == "tile")
        return printf("%d %d %d %d\n", scpx::kChunk, scpx::kWaveStrips, scpx::kBandRows, scpx::kCycle), 0;
    return 2;
}
