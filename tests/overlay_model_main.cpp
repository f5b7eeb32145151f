// TEST: whole efx_overlay calls on the host, with overlay_px.h's functions and k_overlay's own walk -- the list's scan in
// steps, the active events with their gains in list order, the 17 tiles of 64 units, a lane's unit kept from event to
// event and stored once -- on heap blocks of exactly the bytes the contract names (the events, the atlas rounded up to 16,
// the pictures with a filled pad between the streams), so that a sanitizer build (-fsanitize=address,undefined) sees every
// byte the kernel's addressing would touch.
//
//   overlay_model_main call N_STREAMS N_PICTURES N_EVENTS FIRST_PICTURE ATLAS_BYTES
//       the events (N_EVENTS x 64 bytes), the atlas (ATLAS_BYTES) and the pictures (N_STREAMS x N_PICTURES x 101376) from
//       stdin; the pictures, then N_STREAMS status words, to stdout.  exit 1: counts out of range or short input; exit 3:
//       a byte between the streams lost its fill.
//   overlay_model_main step      the scan step (ovx::kScanStep) as text
//   overlay_model_main divide    both rounded divisions, each in both forms, against plain division over their whole
//                                ranges, and the packed luma blend against the plain one for every (Y, Cy, a); exit 2
//                                where one differs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "overlay_px.h"

using namespace efx;

namespace {

constexpr uint8_t kFill = 0xA5;
constexpr size_t kPad = 48;  // bytes between the streams, a multiple of 16

bool read_all(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

// k_overlay for one picture
uint32_t picture(const efx_overlay_event* ev, int n_events, const uint8_t* atlas, uint64_t atlas_bytes, uint8_t* pic, int stream, int64_t p)
{
    std::vector<uint32_t> active;
    bool bad = false;
    for (int base = 0; base < n_events; base += ovx::kScanStep)
        for (int t = 0; t < ovx::kScanStep && base + t < n_events; t++) {
            const efx_overlay_event e = ev[base + t];
            if (!ovx::valid(e, atlas_bytes)) {
                bad = true;
                continue;
            }
            if ((e.stream == -1 || e.stream == stream) && e.first <= p && p <= e.last && ovx::reaches(e)) {
                const int g = ovx::gain(e, p);
                if (g > 0)
                    active.push_back((uint32_t)(base + t) | ((uint32_t)g << 16));
            }
        }
    if (active.empty())
        return bad ? EFX_OVERLAY_BAD_EVENT : 0u;
    const uint8_t* end = atlas + (atlas_bytes + 15) / 16 * 16;
    for (int tile = 0; tile < ovx::kTiles; tile++)
        for (int lane = 0; lane < 64; lane++) {
            const int unit = tile * 64 + lane;
            if (unit >= ovx::kUnits)
                continue;
            const int X = (unit % ovx::kUnitsX) * ovx::kUnitCols, Y = (unit / ovx::kUnitsX) * ovx::kUnitRows;
            ovx::Unit u = {};
            for (uint32_t rec : active) {
                const ovx::Draw d = ovx::draw_of(ev[rec & 0xFFFFu], atlas, (int)(rec >> 16));
                if (ovx::last_unit(d) < tile * 64 || ovx::first_unit(d) >= tile * 64 + 64)
                    continue;
                ovx::apply(&u, d, pic, X, Y, end);
            }
            ovx::store(u, pic, X, Y);
        }
    return bad ? EFX_OVERLAY_BAD_EVENT : 0u;
}

int call(char** v)
{
    const int n_streams = atoi(v[0]), n_pictures = atoi(v[1]), n_events = atoi(v[2]);
    const int64_t first_picture = atoll(v[3]);
    const uint64_t atlas_bytes = strtoull(v[4], nullptr, 10);
    if (n_streams < 1 || n_pictures < 1 || n_events < 0 || n_events > EFX_OVERLAY_MAX_EVENTS || first_picture < 0 ||
        (int64_t)n_streams * n_pictures > 4096 || atlas_bytes > ((uint64_t)1 << 30))
        return 1;
    // (blocks of their own, of exactly the bytes that may be touched)
    std::vector<efx_overlay_event> ev((size_t)n_events);
    const size_t atlas_block = (size_t)((atlas_bytes + 15) / 16 * 16);
    uint8_t* atlas = static_cast<uint8_t*>(malloc(atlas_block ? atlas_block : 1));
    memset(atlas, kFill, atlas_block);
    const size_t row = (size_t)n_pictures * ovx::kPicture, stride = row + kPad;
    uint8_t* pics = static_cast<uint8_t*>(malloc((size_t)n_streams * stride - kPad));
    memset(pics, kFill, (size_t)n_streams * stride - kPad);
    bool ok = read_all(ev.data(), ev.size() * sizeof(efx_overlay_event)) && read_all(atlas, (size_t)atlas_bytes);
    for (int i = 0; ok && i < n_streams; i++)
        ok = read_all(pics + (size_t)i * stride, row);
    if (!ok)
        return 1;
    std::vector<uint32_t> status((size_t)n_streams, 0u);
    for (int i = 0; i < n_streams; i++)
        for (int j = 0; j < n_pictures; j++) {
            const uint32_t st = picture(ev.data(), n_events, atlas, atlas_bytes, pics + (size_t)i * stride + (size_t)j * ovx::kPicture, i,
                                        first_picture + j);
            if (j == 0)
                status[(size_t)i] |= st;
        }
    for (int i = 0; i + 1 < n_streams; i++)
        for (size_t k = row; k < stride; k++)
            if (pics[(size_t)i * stride + k] != kFill)
                return 3;
    for (int i = 0; i < n_streams; i++)
        fwrite(pics + (size_t)i * stride, 1, row, stdout);
    fwrite(status.data(), 4, status.size(), stdout);
    free(atlas);
    free(pics);
    return 0;
}

int divide()
{
    for (uint32_t t = 0; t <= 65025u; t++)
        if (ovx::div255(t) != (2 * t + 255) / 510)
            return 2;
    for (uint32_t n = 0; n <= 260610u; n++)
        if (ovx::div1020(n) != n / 1020 || (uint32_t)(((uint64_t)n * 263173u) >> 28) != n / 1020)
            return 2;
    for (uint32_t y = 0; y < 256; y++)
        for (uint32_t c = 0; c < 256; c++)
            for (uint32_t a = 0; a < 256; a += 2) {
                const uint32_t got = ovx::luma2(y * 0x00010001u, a | ((a + 1) << 16), c * 0x00010001u);
                if ((got & 0xFFFFu) != (2 * (y * (255 - a) + c * a) + 255) / 510 || (got >> 16) != (2 * (y * (254 - a) + c * (a + 1)) + 255) / 510)
                    return 2;
            }
    for (uint32_t A = 0; A < 256; A++)
        for (int g = 0; g <= 256; g++)
            if (ovx::gain4(A * 0x01010101u, g) != ((A * (uint32_t)g + 128) >> 8) * 0x01010101u)
                return 2;
    puts("ok");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "call" && argc == 7)
        return call(argv + 2);
    if (what == "step" && argc == 2) {
        printf("%d\n", ovx::kScanStep);
        return 0;
    }
    if (what == "divide" && argc == 2)
        return divide();
    fprintf(stderr, "usage: overlay_model_main call N_STREAMS N_PICTURES N_EVENTS FIRST_PICTURE ATLAS_BYTES | step | divide\n");
    return 1;
}
