// k_recon.hip -- macroblock reconstruction: IDCT + half-pel motion compensation + store (gfx950).
//
// ONE LANE PER 8x8 BLOCK, one launch per picture index (a P picture needs the previous picture of
// its own stream; streams, macroblocks and blocks are independent).
// Restates idct() (reference src/player.cpp:922-996), predict()/predict_zero()/mocomp()
// (732-889) and copy_block/add_block[_dc] (1151-1236):
//
//   * a lane dequantises its block's compact coefficient entries (k_parse) into a private
//     64 x int16 LDS block, reads them back into 64 registers (scaled by the pre-multipliers) and
//     runs 8 column + 8 row butterflies there -- the same scaled integer AAN arithmetic as the
//     reference;
//   * for predicted blocks nine 12-byte reference rows are fetched with aligned dword loads (the
//     reference's _src_align staging, player.cpp:739-759) and the four half-pel cases are one
//     branch-free packed-byte expression;
//   * the lane adds its 64 residuals to its 64 predicted pixels, clamps to 0..248 (PIN,
//     player.cpp:183-236) and issues eight 8-byte stores into the 16-line strip layout
//     (Frame, src/video.h:36-44).
//
#include <hip/hip_runtime.h>

#include "efx_internal.h"
#include "efx.h"
#include "parse_tm.h"
#include "efx_probe.h"

namespace efx {

namespace {


// v_mul_i32_i24 / v_mad_i32_i24 by name: `__mul24` is library code ((x << 8 >> 8) * (y << 8 >> 8)) that the compiler turns
// into the 24-bit multiply only where it can PROVE the operand fits -- the column pass; in the row pass it kept the two
// shifts and a quarter-rate v_mul_lo_u32 per product (40 of them: a tenth of the kernel's issue time).
__device__ inline int mul24(int a, int k)
{
    int r;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "s"(k), "v"(a));
    return r;
}
__device__ inline int mad24(int a, int k, int c)
{
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(k), "v"(c));
    return r;
}

// One 8-point pass of the reference's scaled integer IDCT (player.cpp:938-995): the same products
// and the same rounding points "(x + 128) >> 8" (integer sums are associative, so only those matter for the bits),
// written as an even / odd decomposition.
// The products use the full-rate 24-bit multiplier: every multiplied operand is a combination of AC
// coefficients only -- the DC term v0 enters through dc_sum / dc_dif and is never multiplied --
// and AC coefficients are clamped to +-2048 and scaled by a premultiplier <= 62, which bounds the
// operands by 2^19 in the column pass and 2^22.5 in the row pass (L1 norm of the linear map; the stream range_idct of
// tests/syntax_streams.py stands at those extremes, 329 654 and 1 775 219, and tests/test_syntax_streams.py computes
// them).  The low 32 bits of the 48-bit product equal the reference's wrapped 32-bit product.
// (the butterfly from its first stage on: the sums and differences of the input pairs (0,4) (2,6) (1,7) (3,5))
__device__ inline void idct8_paired(int dc_sum, int dc_dif, int c_sum, int c_dif, int p17, int m17, int p35, int m53, int& v0, int& v1,
                                    int& v2, int& v3, int& v4, int& v5, int& v6, int& v7, int half)
{
    const int c_rot = (mad24(c_dif, 362, half) >> 8) - c_sum;
    const int even0 = dc_sum + c_sum, even3 = dc_sum - c_sum;
    const int even1 = dc_dif + c_rot, even2 = dc_dif - c_rot;
    const int odd_all = p17 + p35;
    const int odd_a = (mad24(m17, 473, mad24(m53, -196, half)) >> 8) - odd_all;
    const int odd_b = odd_a - (mad24(p17 - p35, 362, half) >> 8);
    const int odd_c = -odd_b - (mad24(m53, 473, mad24(m17, 196, half)) >> 8);
    // output butterflies
    v0 = even0 + odd_all;
    v7 = even0 - odd_all;
    v1 = even1 + odd_a;
    v6 = even1 - odd_a;
    v2 = even2 - odd_b;
    v5 = even2 + odd_b;
    v3 = even3 - odd_c;
    v4 = even3 + odd_c;
}
__device__ inline void idct8(int& v0, int& v1, int& v2, int& v3, int& v4, int& v5, int& v6, int& v7, int half)
{
    // even half: inputs 0, 4 as sum / difference; inputs 2, 6 through one rotation (362 / 256);
    // odd half: inputs 1, 7 and 3, 5 as sums and differences, three rotations (473, 196, 362 over 256)
    idct8_paired(v0 + v4, v0 - v4, v2 + v6, v2 - v6, v1 + v7, v1 - v7, v3 + v5, v5 - v3, v0, v1, v2, v3, v4, v5, v6, v7, half);
}

// v_bitop3_b32: any function of three words bit by bit, table index = a << 2 | b << 1 | c (a = 0xF0, b = 0xCC, c = 0xAA).
// Full rate on gfx950 (2 cycles per wave64) where v_bfi_b32 / v_and_or_b32 / v_cndmask_b32 take 4 (profiles/r6_valu_rates.md);
// the compiler still selects those, hence by name.
template <int kTable>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c)
{
    // (the builtin: behind an inline asm statement the hazard recognizer puts an `s_nop`)
    return __builtin_amdgcn_bitop3_b32(a, b, c, kTable);
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// byte offset of plane row inside a frame (Frame::get_y/get_cr/get_cb, player.cpp:33-46)
__device__ inline int luma_row_off(int y) { return (y >> 4) * kStripBytes + (y & 15) * kStride; }
__device__ inline int chroma_row_off(int plane, int c)
{
    return (c >> 3) * kStripBytes + ((c & 7) + (plane == 2 ? 8 : 0)) * kStride + EFX_FRAME_WIDTH;
}

__device__ inline uint32_t avg_up(uint32_t a, uint32_t b)  // per byte (a + b + 1) >> 1
{
    return (a | b) - (((a ^ b) >> 1) & 0x7F7F7F7Fu);
}

__device__ inline uint32_t avg4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)  // per byte (a+b+c+d+2) >> 2
{
    const uint32_t m = 0x00FF00FFu;
    uint32_t e = (a & m) + (b & m) + (c & m) + (d & m) + 0x00020002u;
    uint32_t o = ((a >> 8) & m) + ((b >> 8) & m) + ((c >> 8) & m) + ((d >> 8) & m) + 0x00020002u;
    return ((e >> 2) & m) | (((o >> 2) & m) << 8);
}

// per byte (a + b + c + d + 2) >> 2 from byte-wise averages (v_lerp_u8: (x + y + (z & 1)) >> 1):
// with h1 = (a + b) >> 1, h2 = (c + d) >> 1 and l = the carry bits both halves dropped,
// the result is (h1 + h2 + 1 + l) >> 1 = ceil_avg(h1, h2) + (l & ~(h1 ^ h2) & 1).
__device__ inline uint32_t avg4_lerp(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t h1 = __builtin_amdgcn_lerp(a, b, 0), h2 = __builtin_amdgcn_lerp(c, d, 0);
    const uint32_t l = (a ^ b) & (c ^ d);
    return __builtin_amdgcn_lerp(h1, h2, 0x01010101u) + (l & ~(h1 ^ h2) & 0x01010101u);
}

}  // namespace

// IDCT pre-multiplier of raster position (r, c): round(32 s_r s_c), s_0 = 1, s_k = sqrt(2) cos(k pi / 16)
// -- the reference's scale_dct_q (player.cpp:161-170), as efx_tables.cpp builds it for the scan
// table; here as compile-time constants so that every register of the in-register IDCT is scaled
// by an immediate.
__device__ constexpr double kAan[8] = {1.0,          1.3870398453221475, 1.3065629648763766, 1.1758756024193588,
                                       1.0,          0.7856949583871022, 0.5411961001461970, 0.2758993792829431};
__device__ constexpr int premul_at(int r, int c) { return (int)(32.0 * kAan[r] * kAan[c] + 0.5); }

constexpr int kBlocksPerPicture = kMbCount * 6;
constexpr int kLaneDwords = 33, kLaneData = 32;  // per-lane LDS block: 64 int16 + one dword (see k_recon)
constexpr int kLaneHalfwords = 2 * kLaneDwords;

// One lane per 8x8 block, 64 consecutive blocks of a picture (in plane-row order, see below) per wave.
//
// The previous mapping (one wave per macroblock, 48 of 64 lanes in the butterflies, transposition
// through LDS) was bound by VALU issue.  Here a lane owns a whole block: it dequantises its own
// coefficient entries into a private 64 x int16 LDS block (the only use of LDS: a register file
// cannot be indexed per lane), reads the block into 64 registers, runs the 16 butterflies of the
// 2-D IDCT in registers, forms the prediction of its 8 x 8 pixels from nine 12-byte row fetches and
// stores eight 8-byte rows.  No lane ever waits for another: no barrier, no shuffle, no scalar
// bookkeeping, every lane busy.
constexpr int kPerRound = 3;  // coefficient entries a lane takes per round of the wave's entry dealing (recon_group: "Three entries")

// which block of the picture lane `lane` of block group `g` owns: macroblock, block inside it
struct BlockAt {
    bool have;
    int blk, mb;
};
__device__ __forceinline__ BlockAt block_at(int g, int lane)
{
    const int b_raw = g * 64 + lane;
    BlockAt o;
    o.have = b_raw < kBlocksPerPicture;
    const int b = o.have ? b_raw : kBlocksPerPicture - 1;
    // Block order inside a picture: by macroblock row, and inside it by plane row -- the 44 upper luma
    // blocks, the 44 lower ones, the 22 "cr" and the 22 "cb" blocks -- so that the lanes of a wave
    // write (and mostly read) long contiguous runs of every frame row they touch.
    const int mbrow = b / 132, rr = b - mbrow * 132;
    int mbx;
    if (rr < 88) {
        const int h = rr >= 44, r2 = rr - 44 * h;
        o.blk = 2 * h + (r2 & 1);
        mbx = r2 >> 1;
    } else {
        const int h = rr >= 110;
        o.blk = 4 + h;
        mbx = rr - 88 - 22 * h;
    }
    o.mb = mbrow * kMbW + mbx;
    return o;
}

// The per-block body of k_recon: plain loads of the reference frame, plain 8-byte row stores.
__device__ __forceinline__ void recon_group(uint32_t* __restrict__ lds, const uint32_t* __restrict__ coefs,
                                            const uint32_t* __restrict__ qt_custom, uint8_t* __restrict__ frames, int ring_depth,
                                            int pic, int pos0, int first_pts, int epoch, int s, int g,
                                            const uint4 rw EFX_PROBE_PARAM)
{
    int16_t* const cfh = reinterpret_cast<int16_t*>(lds);
    uint16_t* const s_pre = reinterpret_cast<uint16_t*>(lds + 64 * kLaneDwords);  // entries before the block in the wave
    uint8_t* const s_zd = reinterpret_cast<uint8_t*>(lds + 64 * kLaneDwords + 32);  // bit 7: an entry sits at scan position 0;
                                                                                    // bits 0-5: intra DC value >> 16
    const int lane = threadIdx.x;
    const BlockAt at = block_at(g, lane);
    const bool have = at.have;
    const int blk = at.blk, mb = at.mb;
    // ring position of this picture (k_advance): the reference's _current / _reference alternation, player.cpp:692-702
    const uint32_t q = (uint32_t)pos0 + (uint32_t)(first_pts < 0 ? pic + 1 : max(0, pic - first_pts));
    const uint32_t cur_slot = q % (uint32_t)ring_depth, ref_slot = (q - 1) % (uint32_t)ring_depth;
    uint8_t* const ring = frames + (size_t)s * ring_depth * kFrameBytes;  // the stream's frames (wave-uniform)
    uint8_t* cur = ring + (size_t)cur_slot * kFrameBytes;
    const uint8_t* ref = ring + (size_t)ref_slot * kFrameBytes;

    const uint32_t w_base = rw.x, w_cnt = rw.y, w_misc = rw.z, w_mv = rw.w;
    EFX_PROBE_STAMP_AFTER(3, w_base);  // the record has arrived
    // a macroblock no slice covers (or an absent picture) keeps the slot's content
    const bool live = have && (w_misc >> 24) == (uint32_t)(epoch & 0xFF);
    const uint32_t flags = (w_misc >> 16) & 0xFF;
    const bool intra = flags & 1;
    const uint64_t cnts = ((uint64_t)(w_misc & 0xFFFF) << 32) | w_cnt;  // six byte counts
    const int my_cnt = live ? (int)((cnts >> (blk * 8)) & 0xFF) : 0;
    // entries of earlier blocks of the macroblock: sum of the lower `blk` bytes
    uint32_t before = 0;
#pragma unroll
    for (int k = 0; k < 5; k++)
        before += (k < blk) ? (uint32_t)((cnts >> (k * 8)) & 0xFF) : 0u;
    const uint32_t my_base = w_base + before;

    // ---- geometry of this block's plane (predict(), player.cpp:870-889) -----------------------------
    const int mb_y = mb / kMbW, mb_x = mb - mb_y * kMbW;
    const int X = (mb_x << 5) + (int16_t)(w_mv & 0xFFFF), Y = (mb_y << 5) + (int16_t)(w_mv >> 16);
    const bool luma = blk < 4;
    // half-pel position of the block's first pixel in its plane; chroma uses the floor of the halved POSITION
    const int PX = luma ? X + (blk & 1) * 16 : (X >> 1), PY = luma ? Y + (blk >> 1) * 16 : (Y >> 1);
    const int px0 = PX >> 1, py0 = PY >> 1, hx = PX & 1, hy = PY & 1;
    const int pw = luma ? EFX_FRAME_WIDTH : EFX_FRAME_WIDTH / 2, ph = luma ? EFX_FRAME_HEIGHT : EFX_FRAME_HEIGHT / 2;
    const bool inside = px0 >= 0 && py0 >= 0 && px0 + 8 + hx <= pw && py0 + 8 + hy <= ph;
    // byte offset of plane row y inside a frame: luma rows are linear; chroma row c of "cr" / "cb"
    // sits in frame row (c >> 3) * 16 + (c & 7) [+ 8] at byte 352 (Frame, video.h:36-44)
    const int chroma_base = (blk == 5 ? 8 : 0) * kStride + EFX_FRAME_WIDTH;
    auto row_off = [&](int y) { return luma ? y * kStride : (((y >> 3) << 4) + (y & 7)) * kStride + chroma_base; };

    // ---- issue the reference fetches first: nine rows of 12 bytes from a 4-byte aligned address ------
    // (the reference's _src_align copy, player.cpp:739-759).  Bytes / rows beyond the 9 x 9 window
    // may fall outside the frame; they are never used (the frame pool ends with slack).
    uint32_t wa[9], wb[9], wc[9];
    const bool want = live && !intra;
    int16_t* mine = cfh + lane * kLaneHalfwords;
    if (!__any(want && !inside)) {
        // One byte offset for the window's first row (a 24-bit multiply: rows < 2^8), then a constant step per row; a
        // chroma window crosses from one strip's eight rows into the next strip's once, at row `jump`.  Every row is
        // loaded by every lane of a wave that predicts at all (a lane that does not -- intra, not live -- reads its
        // own position: no exec-mask region per row, and the ninth row costs less than asking whether it is needed).
        const int xa = px0 & ~3;
        const int y0 = want ? py0 : 0;
        const uint32_t off0 = (uint32_t)(luma ? mul24(y0, kStride) : mul24(((y0 >> 3) << 4) + (y0 & 7), kStride) + chroma_base) +
                              (uint32_t)(want ? xa : 0);
        const uint32_t jump = luma ? 99u : 8u - ((uint32_t)y0 & 7u);
#pragma unroll
        for (int r = 0; r < 9; r++)
            wa[r] = wb[r] = wc[r] = 0;
        if (__any(want)) {
#pragma unroll
            for (int r = 0; r < 9; r++) {
                const uint32_t off = off0 + (uint32_t)(r * kStride) + ((uint32_t)r >= jump ? 8u * kStride : 0u);
                const uint32_t* p = reinterpret_cast<const uint32_t*>(ref + off);
                wa[r] = p[0];
                wb[r] = p[1];
                wc[r] = p[2];
            }
        }
    } else {
        // some vector of this wave points outside the picture (undefined in the reference): every lane
        // builds its window pixel by pixel with clamped coordinates -- identical to the direct fetch
        // for the windows that are inside -- through its private LDS block (not yet in use)
        uint32_t* w32 = reinterpret_cast<uint32_t*>(mine);
#pragma unroll 1
        for (int i = 0; i < 27; i++) {
            const int r = i / 3, d = i - r * 3;
            uint32_t word = 0;
            if (want)
#pragma unroll 1
                for (int k = 0; k < 4; k++) {
                    const int yy = clampi(py0 + r, 0, ph - 1), xx = clampi((px0 & ~3) + d * 4 + k, 0, pw - 1);
                    const uint32_t o = (uint32_t)(row_off(yy) + xx);
                    const uint32_t byte = (uint32_t)ref[o];
                    word |= (byte & 0xFF) << (k * 8);
                }
            w32[i] = word;
        }
#pragma unroll
        for (int r = 0; r < 9; r++) {
            wa[r] = w32[r * 3];
            wb[r] = w32[r * 3 + 1];
            wc[r] = w32[r * 3 + 2];
        }
    }

    // ---- own coefficient entries -> private LDS block (dequantised, not yet pre-multiplied) ----------
    {
        uint32_t* z = reinterpret_cast<uint32_t*>(mine);
#pragma unroll
        for (int k = 0; k < kLaneData; k++)
            z[k] = 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the table written above is read below by other lanes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // The 64 blocks of the wave hold very different numbers of entries (3 on average, a dozen at the
    // maximum), so a loop in which every lane walks its own list runs at a quarter of the lanes.
    // Instead the wave's entries are dealt out one per lane: entry i belongs to the last lane whose
    // exclusive prefix count is <= i (six-step search in the prefix array), is dequantised with that
    // lane's parameters and lands in that lane's block.
    // inclusive prefix sum over the wave in the vector pipe: inside rows of 16 lanes by DPP row shifts, then the rows' totals
    // by row broadcasts (six instructions; six ds_bpermute round trips before)
    uint32_t incl = (uint32_t)my_cnt;
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, false);  // row_shr:1
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, false);  // row_shr:2
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, false);  // row_shr:4
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, false);  // row_shr:8
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1, 3
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2, 3
    const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
    const uint32_t pre = incl - (uint32_t)my_cnt;  // entries before this block in the wave (<= 64 * 64)
    const uint32_t pre_flags = pre | (flags << 16);  // flags: bit0 intra, bits 2-6 quantiser_scale, bit7 custom matrices
    s_zd[lane] = 0;
    s_pre[lane] = (uint16_t)pre;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // Three entries per lane per round: the owners are searched and all loads issued before the first entry
    // is used -- a wave is alive for as many memory round trips as it makes one after the other, and with
    // one load per loop trip the entries alone cost it three (-5.5 % per launch).
    int own[kPerRound], own_next[kPerRound];
    uint32_t ent[kPerRound], ent_next[kPerRound];
    auto fetch = [&](uint32_t i0, int (&own)[kPerRound], uint32_t (&ent)[kPerRound]) {
#pragma unroll
        for (int k = 0; k < kPerRound; k++) {
            const uint32_t i = i0 + 64 * k;
            // (L2 = 2 L, the byte offset into s_pre: the probe's address is L2 + an immediate; "prefix <= i" as the sign
            // of a difference -- both are below 2^13 -- and the step merged in by a bit operation: three full-rate
            // instructions per step, where compare + select + shift + or cost seventeen cycles -- profiles/r6_valu_rates.md)
            uint32_t L2 = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const uint32_t probe = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(s_pre) + L2 + 2 * step);
                int32_t diff = (int32_t)(i - probe);
                asm("" : "+v"(diff));  // (opaque: the compiler knows the ranges and would rebuild the compare + select)
                const uint32_t below = (uint32_t)(diff >> 31);  // all ones: prefix > i
                L2 = bitop3<0xF4>(L2, (uint32_t)(2 * step), below);             // L2 | (2 step & ~below)
            }
            const int L = (int)(L2 >> 1);
            const uint32_t o_pf = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(L2 + L2), (int)pre_flags);
            const uint32_t o_base = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(L2 + L2), (int)my_base);
            own[k] = L | (int)(o_pf >> 16 << 8);  // owner lane | its flags << 8
            // (always a load, beyond the end from entry 0: the compiler then knows how many loads are in flight and
            // the prediction below waits for the windows only)
            ent[k] = coefs[i < total ? o_base + (i - (o_pf & 0xFFFF)) : 0u];
        }
    };
    auto apply = [&](uint32_t i0) {
#pragma unroll
        for (int k = 0; k < kPerRound; k++) {
            if (i0 + 64 * k >= total)
                continue;
            const int L = own[k] & 63;
            const uint32_t e = ent[k];
            const uint32_t f = (uint32_t)own[k] >> 8;
            const bool o_intra = f & 1;
            // k_parse's stream word: raw bits << 16 | value << 6 | scan position (parse_tm.h); an intra block's first word
            // is its DC value << 6
            const int n = e & 63;
            const int level = (o_intra && n == 0) ? (int)e >> 6 : tm_level(e);
            // scan/quantiser table entry: zz | slot in the paired block layout << 8 | intra q << 16 | non-intra q << 24
            uint32_t t = lds[n * kLaneDwords + kLaneData];
            if (f & 0x80)
                t = qt_custom[n];
            if (o_intra && n == 0) {
                // b[0] = dc << 8 (player.cpp:1065) does not fit the int16 block: the value is kept as it is, its low
                // half in position 0 (no other entry of an intra block lands there), the rest beside the flag
                cfh[L * kLaneHalfwords] = (int16_t)level;
                s_zd[L] = (uint8_t)(0x80 | ((level >> 16) & 0x3F));
            } else {
                if (n == 0)
                    s_zd[L] = 0x80;
                // dequantise, player.cpp:1110-1121; |2 level +- 1| <= 511, qscale <= 31, q <= 255
                const int q = o_intra ? (int)((t >> 16) & 0xFF) : (int)(t >> 24);
                int val = level << 1;
                if (!o_intra)
                    val += (val < 0) ? -1 : 1;
                val = __mul24(__mul24(val, (int)((f >> 2) & 31)), q);
                val = (val + ((val >> 31) & 15)) >> 4;  // division by 16 truncating toward zero
                if ((val & 1) == 0)
                    val -= (val > 0) ? 1 : -1;
                val = val > 2047 ? 2047 : (val < -2048 ? -2048 : val);
                cfh[L * kLaneHalfwords + ((t >> 8) & 63)] = (int16_t)val;  // (its slot in the paired layout, efx_tables.cpp)
            }
        }
    };
    fetch(lane, own, ent);  // (also when the wave has no entry at all: the same three loads in flight on every path)

    // ---- prediction of the 8 rows, in the shadow of the entry loads just issued (a wave's life is its chain of
    // memory round trips: record -> owner search -> entries; this arithmetic needs only the windows, which were
    // requested before) -- the 27 window registers die here, before the 64 IDCT registers come alive -----------
    // All four half-pel cases of mocomp() (player.cpp:767-820) are ONE expression, (a + b + c + d + 2) >> 2 per byte with
    // a = the pixel, b = the pixel to the right if hx else a, c = the pixel below if hy else a, d = below-right / below /
    // right / a: with equal operands it degenerates exactly to (a + b + 1) >> 1 and to a.  (Lanes of one wave carry
    // different vectors, so a branch per case would execute all four.)  Built from byte-wise averages (v_lerp_u8):
    // with H = (a + b) >> 1 per WINDOW row, X = a ^ b, and h2 / x2 those of the row below if hy (else the same row's),
    // the result is lerp(H, h2, 1) + (X & x2 & ~(H ^ h2) & 1).  A window row's P (eight pixels at the block's position),
    // Q (one pixel to the right if hx: byte permutes with per-lane selectors), H and X serve the output row it is `a` for
    // and the one it is `c` for.
    uint32_t pr_lo[8], pr_hi[8];
    {
        const uint32_t selP = 0x03020100u + 0x01010101u * (uint32_t)(px0 & 3), selQ = selP + 0x01010101u * (uint32_t)hx;
        const uint32_t hym = 0u - (uint32_t)hy;
        uint32_t keep = intra ? 0u : ~0u;  // (an intra block has no prediction: its window registers hold its own position)
        asm volatile("" : "+v"(keep));     // (a mask, not a condition: sixteen full-rate ANDs instead of sixteen selects)
        auto pick = [](uint32_t m, uint32_t set, uint32_t clear) {  // bit by bit: m ? set : clear
            return bitop3<0xCA>(m, set, clear);
        };
        auto row = [&](int r, uint32_t& Hl, uint32_t& Hh, uint32_t& Xl, uint32_t& Xh) {
            const uint32_t Pl = __builtin_amdgcn_perm(wb[r], wa[r], selP), Ph = __builtin_amdgcn_perm(wc[r], wb[r], selP);
            const uint32_t Ql = __builtin_amdgcn_perm(wb[r], wa[r], selQ), Qh = __builtin_amdgcn_perm(wc[r], wb[r], selQ);
            Hl = __builtin_amdgcn_lerp(Pl, Ql, 0);
            Hh = __builtin_amdgcn_lerp(Ph, Qh, 0);
            Xl = Pl ^ Ql;
            Xh = Ph ^ Qh;
        };
        uint32_t Hl, Hh, Xl, Xh;
        row(0, Hl, Hh, Xl, Xh);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            uint32_t Hl1, Hh1, Xl1, Xh1;
            row(r + 1, Hl1, Hh1, Xl1, Xh1);
            const uint32_t h2l = pick(hym, Hl1, Hl), h2h = pick(hym, Hh1, Hh);
            const uint32_t x2l = pick(hym, Xl1, Xl), x2h = pick(hym, Xh1, Xh);
            pr_lo[r] = (__builtin_amdgcn_lerp(Hl, h2l, 0x01010101u) + (Xl & x2l & ~(Hl ^ h2l) & 0x01010101u)) & keep;
            pr_hi[r] = (__builtin_amdgcn_lerp(Hh, h2h, 0x01010101u) + (Xh & x2h & ~(Hh ^ h2h) & 0x01010101u)) & keep;
            Hl = Hl1;
            Hh = Hh1;
            Xl = Xl1;
            Xh = Xh1;
            // (one row at a time: all nine rows' permutes hoisted to the top cost 139 registers)
            asm volatile("" : "+v"(pr_lo[r]), "+v"(pr_hi[r]), "+v"(Hl), "+v"(Hh), "+v"(Xl), "+v"(Xh));
        }
    }

    if (total) {
        for (uint32_t i0 = lane;;) {  // (uniform trip count: i0 - lane < total)
            // the next round's owners are searched and its entries requested before this round's are applied
            const bool more = i0 - lane + 64 * kPerRound < total;
            if (more)
                fetch(i0 + 64 * kPerRound, own_next, ent_next);
            apply(i0);
            if (!more)
                break;
            i0 += 64 * kPerRound;
#pragma unroll
            for (int k = 0; k < kPerRound; k++) {
                own[k] = own_next[k];
                ent[k] = ent_next[k];
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t zd = s_zd[lane];
    EFX_PROBE_STAMP_AFTER(5, zd);  // the entries have been dealt out: the IDCT starts
    const bool zf = (zd & 0x80) != 0;  // an entry sits at scan position 0
    // intra DC value (22 bits: a slice adds at most 1584 differentials of +-255 to the predictor)
    const int dc_raw = (int)((uint32_t)(uint16_t)mine[0] | ((uint32_t)((int)(zd << 26) >> 26) << 16));
    // The parser hands the predictor on unclamped, and a slice can walk it far out of 0 ... 255; behind the IDCT a pixel is
    // kept in 16 bits (pair(), below).  The 63 AC coefficients of a block move a pixel by 14 062 at the most
    // (tests/test_syntax_streams.py, largest_ac_residual(), computes it and holds kDcBound against it), so a DC term beyond
    // +-kDcBound ends at 0 or 248 whatever they do: bounded there it changes no stored pixel, and DC + AC stays inside
    // +-2^15.  (One v_med3_i32.  A DC-only block does not pass here: its value is replicated whole, flat4 below.)
    constexpr int kDcBound = 16384;
    const int dc_idct = max(-kDcBound, min(kDcBound, dc_raw));

    // A block whose only coefficient sits at scan position 0 takes the reference's "n == 1"
    // shortcut (player.cpp:1133-1140): dc = b[0] >> 8 (floor), no IDCT; for intra blocks the
    // byte is replicated WITHOUT the 0..248 clamp (copy_block_dc, player.cpp:1175-1187).
    const bool dc_only = my_cnt == 1 && zf;

    // ---- 2-D IDCT in registers (idct(), player.cpp:922-996) --------------------------------------------
    // Blocks without entries run the butterflies on zeros (which stay zero).  A dc_only block has its
    // single value X at raster position 0; the butterflies turn that into X at all 64 positions
    // exactly, so clearing X's low byte makes the final (x + 128) >> 8 deliver X >> 8, the shortcut.
    int v[64];
    const int half = 128;
    if (total == 0) {
        // (wave-uniform) no block of this wave holds a coefficient -- skipped macroblocks, static background: what the
        // butterflies make of 64 zeros and the rounding constant is the rounding constant
#pragma unroll
        for (int i = 0; i < 64; i++)
            v[i] = 128;
    } else {
    const uint32_t* mine32 = reinterpret_cast<const uint32_t*>(mine);
#pragma unroll
    for (int c = 0; c < 8; c++) {
        // Column c (round 6): FOUR dwords from the private block -- the rows in the pairs the butterfly's first stage combines,
        // (0,4) (2,6) (1,7) (3,5) (efx_tables.cpp lays the block out so) -- and the first stage INCLUDING the pre-multipliers
        // as one v_dot2_i32_i16 per sum / difference, x_a p_a +- x_b p_b with the two pre-multipliers packed in a constant:
        // eight instructions where eight multiplies and eight additions stood, and half the LDS reads.
        auto dot = [](uint32_t pair, int pa, int pb) {
            // (by name: the builtin is selected as v_dot2c_i32_i16, the accumulating two-operand form, plus a v_mov to clear
            // its accumulator -- what the fusion saves)
            int r;
            asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(pair), "s"((uint32_t)(uint16_t)(short)pa | ((uint32_t)(uint16_t)(short)pb << 16)));
            return r;
        };
        const uint32_t q04 = mine32[c * 4], q26 = mine32[c * 4 + 1], q17 = mine32[c * 4 + 2], q35 = mine32[c * 4 + 3];
        int dc_sum, dc_dif;
        if (c == 0) {
            // the DC term: an intra block's is the parser's value << 8 (wider than the block's int16), and a block whose only
            // coefficient it is has its low byte cleared (the reference's n == 1 shortcut, see above)
            int v0 = __mul24((int)(int16_t)(q04 & 0xFFFF), premul_at(0, 0));
            v0 = intra ? (dc_idct << 8) : v0;
            v0 = dc_only ? (v0 & ~0xFF) : v0;
            const int v4 = __mul24((int)q04 >> 16, premul_at(4, 0));
            dc_sum = v0 + v4;
            dc_dif = v0 - v4;
        } else {
            dc_sum = dot(q04, premul_at(0, c), premul_at(4, c));
            dc_dif = dot(q04, premul_at(0, c), -premul_at(4, c));
        }
        idct8_paired(dc_sum, dc_dif, dot(q26, premul_at(2, c), premul_at(6, c)), dot(q26, premul_at(2, c), -premul_at(6, c)),
                     dot(q17, premul_at(1, c), premul_at(7, c)), dot(q17, premul_at(1, c), -premul_at(7, c)),
                     dot(q35, premul_at(3, c), premul_at(5, c)), dot(q35, -premul_at(3, c), premul_at(5, c)),
                     v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c], half);
        // one butterfly at a time (volatile asm statements keep their order): with all sixteen in
        // flight the temporaries push the kernel past 128 registers and an occupancy step
        asm volatile("" : "+v"(v[c]), "+v"(v[8 + c]), "+v"(v[16 + c]), "+v"(v[24 + c]), "+v"(v[32 + c]), "+v"(v[40 + c]),
                     "+v"(v[48 + c]), "+v"(v[56 + c]));
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
        // the final rounding "(x + 128) >> 8" (player.cpp:985-994): the first input reaches all eight outputs unscaled
        // (it is never multiplied), so the 128 is added there, once; the shift is left to the byte permutes below -- a
        // residual fits 16 bits (14 304 at the most, an intra DC term is bounded above: the same test), so bytes 1 and 2
        // of x + 128 ARE the shifted value
        v[r * 8] += 128;
        idct8(v[r * 8], v[r * 8 + 1], v[r * 8 + 2], v[r * 8 + 3], v[r * 8 + 4], v[r * 8 + 5], v[r * 8 + 6], v[r * 8 + 7], half);
        asm volatile("" : "+v"(v[r * 8]), "+v"(v[r * 8 + 1]), "+v"(v[r * 8 + 2]), "+v"(v[r * 8 + 3]), "+v"(v[r * 8 + 4]),
                     "+v"(v[r * 8 + 5]), "+v"(v[r * 8 + 6]), "+v"(v[r * 8 + 7]));
    }
    }

    // destination rows of the block (block(), player.cpp:1124-1131)
    const int dst0 = luma ? (mb_y * 16 + (blk >> 1) * 8) * kStride + mb_x * 16 + (blk & 1) * 8
                          : mb_y * kStripBytes + (blk - 4) * 8 * kStride + EFX_FRAME_WIDTH + mb_x * 8;
    // an intra block the parser abandoned is not stored (player.cpp:1106-1107)
    const bool stored = live && !(intra && my_cnt == 0);
    const bool clamped = !(intra && dc_only);

    // copy_block[_dc] / add_block[_dc], player.cpp:1151-1236, two pixels per instruction: residual pairs come out
    // of the 32-bit registers by byte permutes (which also apply the >> 8), prediction bytes are widened the same
    // way, then packed 16-bit add, max 0, min 248 (PIN, player.cpp:183-236) and one permute back to four bytes
    typedef short pk16 __attribute__((ext_vector_type(2)));
    auto pair = [](int hi, int lo) {  // (hi + 128) >> 8 : (lo + 128) >> 8 as two int16
        return __builtin_bit_cast(pk16, __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x06050201u));
    };
    auto widen = [](uint32_t p, bool upper) {  // bytes 0, 1 (or 2, 3) of p as two uint16
        return __builtin_bit_cast(pk16, __builtin_amdgcn_perm(0u, p, upper ? 0x0C030C02u : 0x0C010C00u));
    };
    const short ceiling = my_cnt == 0 ? 255 : 248;
    const pk16 zero = {0, 0}, top = {ceiling, ceiling};
    uint32_t flat4 = (uint32_t)dc_raw;  // intra DC-only block: replicated exactly as copy_block_dc does, unclamped and
    flat4 |= flat4 << 8;                // unmasked (player.cpp:1175-1187)
    flat4 |= flat4 << 16;
    uint32_t clamped_m = clamped ? ~0u : 0u;
    asm volatile("" : "+v"(clamped_m));
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint32_t p_lo = pr_lo[r], p_hi = pr_hi[r];
        const int* q = v + r * 8;
        uint32_t w[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t pp = h ? p_hi : p_lo;
            pk16 a = pair(q[4 * h + 1], q[4 * h]) + widen(pp, false);
            pk16 b = pair(q[4 * h + 3], q[4 * h + 2]) + widen(pp, true);
            a = __builtin_elementwise_min(__builtin_elementwise_max(a, zero), top);
            b = __builtin_elementwise_min(__builtin_elementwise_max(b, zero), top);
            w[h] = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, a), 0x06040200u);
        }
        // prediction only (skipped macroblock, block without coefficients) / intra DC-only replica / the clamped sum
        const uint32_t out_lo = bitop3<0xCA>(clamped_m, w[0], flat4), out_hi = bitop3<0xCA>(clamped_m, w[1], flat4);
        if (stored)
            *reinterpret_cast<uint2*>(cur + dst0 + r * kStride) = make_uint2(out_lo, out_hi);
    }
}

// ---- one launch per picture index -------------------------------------------------------------------------------------------
// grid = (streams, 25): blockIdx.x = stream, blockIdx.y = group of 64 consecutive 8x8 blocks.  With a stream count that is a
// multiple of 8 all blocks of a stream are dispatched to XCD (stream % 8).  A P picture needs the previous picture of its
// own stream: the launch boundary is the dependency.
__global__ __launch_bounds__(64) void k_recon(const MbRec* __restrict__ mbrecs, const uint32_t* __restrict__ coefs,
                                              const uint32_t* __restrict__ scan_tab,
                                              const uint32_t* __restrict__ qtab_custom, uint8_t* __restrict__ frames,
                                              int max_pictures, int ring_depth, int pic, const int32_t* __restrict__ call_pos,
                                              int epoch, int stream0)
{
    // 8640 bytes of LDS per wave (18 waves per CU; the 91 registers allow 20).  Per lane 33 dwords: 64 int16
    // coefficients and, in the 33rd (which makes the stride odd: lanes fan out over the banks), entry `lane` of the
    // default scan / quantiser table; the wave's prefix counts for the owner search; 64 bytes of per-block flags.
    // What else a lane needs to know about another lane's block (first entry, quantiser) is fetched from that lane's
    // registers (ds_bpermute).  Measured: this layout at 16 / 18 / 19 waves per CU 8.07 / 8.16 / 7.85 M frames/s
    // (19 with the search through ds_bpermute as well), the previous one (9.7 KB, 16 waves) 7.78.
    __shared__ uint32_t lds[64 * kLaneDwords + 32 + 16];
    const int lane = threadIdx.x;
    const int s = stream0 + blockIdx.x;
    // (one record per wave, placed by launch: the ring holds ten launches of 512 streams)
    EFX_PROBE_CLAIM_AT(2, blockIdx.x * gridDim.y + blockIdx.y,
                       ((long long)(epoch & 0xFF) * 16 + pic) * (gridDim.x * gridDim.y) + blockIdx.x * gridDim.y + blockIdx.y,
                       (unsigned)(epoch & 0xFF));
    EFX_PROBE_STAMP(1);
    EFX_PROBE_CYCLES_BEGIN();
    EFX_PROBE_SET(6, (unsigned long long)pic | (unsigned long long)(epoch & 0xFF) << 8 | (unsigned long long)stream0 << 16);
    // scan/quantiser table entry: zz | slot in the paired block layout << 8 | intra q << 16 | non-intra q << 24
    lds[lane * kLaneDwords + kLaneData] = scan_tab[lane];
    const BlockAt at = block_at(blockIdx.y, lane);
    const uint4 rw = *reinterpret_cast<const uint4*>(mbrecs + ((size_t)s * max_pictures + pic) * kMbCount + at.mb);
    EFX_PROBE_STAMP_AFTER(3, rw.x);  // the record has arrived
    recon_group(lds, coefs, qtab_custom + ((size_t)s * max_pictures + pic) * 64, frames, ring_depth, pic, call_pos[2 * s],
                call_pos[2 * s + 1], epoch, s, blockIdx.y, rw EFX_PROBE_PASS);
    EFX_PROBE_STAMP(4);
    EFX_PROBE_CYCLES_END(2);
}

// FNV-1a-64 of whole ring frames, one lane per frame (verification helper, not on the timed path)
__global__ void k_frame_hash(const uint8_t* __restrict__ frames, int n_frames, uint64_t* __restrict__ out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frames)
        return;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(frames + (size_t)i * kFrameBytes);
    uint64_t h = 0xcbf29ce484222325ull;
    for (int k = 0; k < kFrameBytes / 4; k++) {
        uint32_t w = p[k];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            h ^= (w >> (8 * b)) & 0xFF;
            h *= 0x100000001b3ull;
        }
    }
    out[i] = h;
}

__global__ void k_fill(uint32_t* __restrict__ p, uint32_t v, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride)
        p[i] = v;
}

}  // namespace efx

EFX_PROBE_READER(recon)
