// efx_internal.h -- structures shared by the host side of libefx and its gfx950 kernels.
//
// Pipeline of one efx_decode():
//   k_demux        (TS input, at upload) one workgroup per stream: 188-byte packets -> ES + PES PTS list
//                                                                            (player.cpp:294-307,381-493)
//   k_index        one workgroup per stream: start-code scan + header parse + the sequential state rules as scans
//                                                                            (player.cpp:1355-1367,646-730)
//   k_slice_scan   prefix sum of slice counts in picture-major order
//   k_slice_emit   dense slice descriptors
//   k_parse        one lane per slice, a token machine (parse_tm.h): VLC parse -> macroblock records + stream words
//                                                                            (player.cpp:1238-1316,999-1107,891-920)
//   k_recon        one lane per 8x8 block, one launch per picture index: dequantisation + IDCT + half-pel
//                  motion compensation + clamp + strip-layout store          (player.cpp:1110-1121,922-996,732-889,1151-1236)
#pragma once
#include <cstdint>

#include "efx.h"
#include "enc_aq.h"
#include "enc_cut.h"
#include "enc_rate.h"
#include "import_pcm.h"
#include "loudness_px.h"
#include "limit_px.h"

namespace efx {

constexpr int kMbW = 22, kMbH = 12, kMbCount = 264;
constexpr int kStride = 528, kStripBytes = 8448, kFrameBytes = 101376;
constexpr int kMaxSlicesPerPicture = 16;   // slice start codes kept per picture
constexpr int kParseLanes = 64;            // slices per k_parse wave (one lane each)
constexpr int kParseWaves = 4;             // waves of a k_parse workgroup (they share one copy of the tables in LDS)
constexpr int kIndexWaves = 4;             // waves of a k_index workgroup (one workgroup per stream)
constexpr int kMaxUnitsPerStream = 4096;   // start codes indexed per stream per decode
constexpr int kCoefsPerEsByte = 4;         // stream words a slice can need per byte: < 3 (a run/level costs >= 3 bits, a motion
                                           // code's word >= 3 with its share of the macroblock header); 4 keeps every slice's region
                                           // 16-byte aligned for k_parse's staged 16-byte stores
constexpr int kEsTailBytes = 9;            // 00 | 00 00 01 B7 | 00 00 01 B7   (player.cpp:456,472)
constexpr int kEsGuardBytes = 512;         // zero guard after the last stream (parse lanes read 128 B ahead)

// per (stream, picture)
struct PicInfo {
    uint32_t first_slice;  // index into the stream's temporary slice list
    uint16_t n_slices;
    uint8_t type;          // 1 = I, 2 = decoded with the P books (P, and B/D headers the reference ignores)
    uint8_t full_pel;
    uint8_t r_size;        // forward_f_code - 1
    uint8_t custom_q;      // 1: quantiser tables at qtab[(stream*max_pictures+pic)*64]
    uint16_t reserved;
    uint32_t seq_off;      // stream-relative offset of the governing sequence header payload
    uint32_t start_off;    // stream-relative offset of the first byte after the picture start code
};

// one PES header that carried a PTS (k_demux): ES offset of its first payload byte, 33-bit PTS
struct PesEntry {
    uint32_t es_off;
    uint32_t reserved;
    int64_t pts;
};

// decoder state that survives from one efx_decode call to the next (MpegDecoder::_fb_index, _last_pts != -1,
// _pts; reference src/player.h:37-47); efx_reset puts back the constructor's values
struct StreamState {
    uint32_t fb_index;  // frame index of the next picture's predecessor: pictures so far that swapped buffers, + 1
    uint32_t pts_seen;  // a picture header has latched a PES PTS
    int64_t pts_carry;  // newest PES PTS of the uploads so far (-1: none)
};

constexpr int64_t kNoPts = INT64_MIN;  // "this upload carried no PES PTS for the stream" (k_index -> k_advance)

struct SliceTmp {
    uint32_t off;       // stream-relative offset of the first byte after the slice start code
    uint32_t len_code;  // (bytes up to the next start code) << 8 | slice start code value
};

struct SliceDesc {
    uint32_t es_off;   // absolute offset in the ES buffer
    uint32_t es_len;   // bytes up to the next start code
    uint32_t stream;
    uint32_t pic_code_flags;  // pic | code << 8 | type << 16 | full_pel << 18 | r_size << 19 | custom_q << 22
    uint32_t mb_limit;  // the slice stops here: the nearest first macroblock, in raster order, of any other slice of the
                        // picture (264 if none; 0 for a slice superseded by a later one with the same start code) -- a
                        // (damaged) slice that runs on never writes a macroblock another parse lane writes (k_slice_emit)
    uint32_t reserved;
};

// one macroblock of one picture, written by k_parse, consumed by k_recon
struct MbRec {
    uint32_t coef_base;  // absolute index of the first coefficient entry
    uint8_t cnt[6];      // entries per block (intra: including the DC entry)
    uint8_t flags;       // bit0 intra, bit1 skipped (copy co-located), bits 2-6 quantiser_scale, bit7 loaded matrices
    uint8_t epoch;       // decode epoch that wrote the record (0 = never)
    int16_t mvx, mvy;    // half-pel luma displacement after full_pel scaling
};
static_assert(sizeof(MbRec) == 16, "MbRec must be 16 bytes");

// coefficient entry = the parser's stream word: raw code bits << 16 | table value << 6 | scan position, level by
// tm_level() (parse_tm.h); an intra block's first entry: DC value << 6.  k_recon dequantises and pre-multiplies (the
// reference's b[zz] = v * scale_dct_q[zz], player.cpp:1110-1121)

// scan / quantiser table of k_index and k_recon (the VLC tables of the slice parser are parse_tm.h's TmTables)
struct ParseTables {
    uint32_t scan[64];       // scan position n -> zz | slot in k_recon's paired block layout << 8 | default intra q << 16 | 16 << 24
};

struct DecodeCounters {
    uint32_t total_slices;
    uint32_t streams;  // streams of the group of streams these counters belong to (k_slice_scan)
    unsigned long long coefficients;
    unsigned long long macroblocks;
    uint32_t next_wave;  // k_parse: the next group of kParseLanes slices nobody has taken yet (its waves pull their work)
    uint32_t reserved;
};

// composite video geometry + tables (video.cpp:514-630)
struct VideoTables {
    int32_t line_width, line_count, hsync, hsync_long, hsync_short, burst_start, burst_width, active_start;
    int32_t pal;
    uint16_t sync_level, blanking_level, black_level, pad;
    int16_t burst0[64], burst1[64];
    uint32_t color_tab[768];
};

// Every sample of a field that is not picture or overlay: whole lines as video_isr leaves them in
// the DMA buffers (sync, burst, black; vertical blanking; the PAL half-line syncs), one template per
// line kind.  k_composite copies 16 bytes from here instead of re-deriving eight samples.
constexpr int kCompositeItemsPerBlock = 2048;  // 8-sample groups one k_composite workgroup renders (8 passes of 256 threads)
constexpr int kLineTemplates = 6;      // 0/1 normal line (PAL: _line_counter odd / even), 2 NTSC vertical blanking, 3..5 PAL sync types 0, 2, 3
constexpr int kLineTemplateWidth = 1152;  // >= 1136 samples, 16-byte multiple
struct VideoLineTemplates {
    uint16_t tpl[kLineTemplates][kLineTemplateWidth];
};
void build_video_line_templates(const VideoTables* v, VideoLineTemplates* out);

// k_export (k_export.hip): one item = 16 luma columns x 2 rows of one picture (the two rows share one chroma row), 22 x 96
// items per picture; a workgroup converts kExportItemsPerBlock consecutive items (4 passes of 256 threads)
constexpr int kExportItemsPerPicture = 22 * 96;
constexpr int kExportItemsPerBlock = 1024;
constexpr int kExportMaxGroups = 16;  // reconstruction groups of one efx_decode (efx_api.hip: kMaxGroups)

// k_export launch arguments (by value)
struct ExportArgs {
    int first_stream, ring_depth;
    int slot;     // >= 0: this ring slot of every stream; < 0: picture `picture` of the most recent efx_decode
    int picture;
    // picture mode: streams [group_first[g], group_first[g + 1]) of that call left their ring positions in call_pos[g]
    // (k_advance: call_pos[2 s] = frame index before the call, call_pos[2 s + 1] = first picture with a PTS or -1)
    int n_groups;
    int group_first[kExportMaxGroups];
    const int32_t* call_pos[kExportMaxGroups];
    int full_range;
    uint8_t* dst;
    size_t dst_stride;
};

// k_trick (k_trick.hip): one item = 16 bytes of one picked picture of one stream; a workgroup moves kTrickItemsPerBlock
// consecutive items (4 passes of 256 threads), and takes further such runs when there are more than the grid's
constexpr int kTrickItemsPerBlock = 1024;
constexpr unsigned kTrickMaxBlocks = 1u << 20;

// k_trick launch arguments (by value): efx_trick_opts, checked
struct TrickArgs {
    const uint8_t* src;  // I420 source: stream i, picture j at src + i * src_stride + j * 101376; ring source: the frame rings
    uint8_t* fwd;        // may be null: stream i, pick k at fwd + i * fwd_stride + (k - k0) * 101376
    uint8_t* rwd;        // may be null: stream i, pick k at rwd + i * rwd_stride + (K - 1 - k) * 101376
    size_t src_stride, fwd_stride, rwd_stride;
    int64_t first_picture;  // title index of the call's picture 0
    int64_t k0, K;          // the call's first pick, the picks of the whole title (trick_sel.h)
    int n_streams, n_picks, speed;
    // ring source (k_export's picture mode: ring_px.h)
    int first_stream, ring_depth, n_groups;
    int group_first[kExportMaxGroups];
    const int32_t* call_pos[kExportMaxGroups];
};

// k_import (k_import.hip): the taps of one destination index of one axis, written by k_import_taps (import_px.h: taps())
constexpr int kImportTapSlots = 132;  // ipx::kMaxTaps rounded up so that a record is a multiple of 16 bytes
struct ImportTap {
    int32_t start, count;  // source indices [start, start + count) of the (cropped) plane
    uint16_t k[kImportTapSlots];
};
// the table of a call: luma columns, luma rows, chroma columns, chroma rows of the destination rectangle
constexpr int kImportTapLX = 0, kImportTapLY = 352, kImportTapCX = 352 + 192, kImportTapCY = 352 + 192 + 176;
constexpr int kImportTapRows = 352 + 192 + 176 + 96;
constexpr int kImportBandRows = 8;            // a workgroup makes 8 luma rows and 4 rows of each chroma plane
constexpr int kImportBands = 192 / kImportBandRows;
constexpr int kImportMaxWidth = 4096;

// k_import_taps / k_import launch arguments (by value)
struct ImportArgs {
    int format;                          // efx_pixel_format of the source
    int width, height;                   // source picture
    int crop_x, crop_y, crop_w, crop_h;  // source rectangle
    int dst_x, dst_y, dst_w, dst_h;      // destination rectangle
    int full_range;
    size_t src_stride, dst_stride;
};

// k_import_surf launch arguments (by value): the ImportArgs of the surface's canonical I420 image, and the surface, checked
struct ImportSurfArgs {
    ImportArgs a;
    efx_surface s;
};

// k_crop_zero / k_crop_sums / k_crop_rects launch arguments (by value): efx_crop_opts, checked (k_cropdetect.hip)
struct CropArgs {
    const uint8_t* src;  // image k at src + k * src_stride
    uint32_t* sums;      // image k: R[0 .. height), C[0 .. width) at sums + k * sums_stride (the caller's, or the context's scratch)
    int32_t* rects;      // stream i: 8 int32 at rects + 8 i
    size_t src_stride, sums_stride;
    int n_streams, images_per_stream, n_images;
    int format, width, height, full_range, limit, round;
};

// k_crop_sums_surf8 / _surf16 launch arguments (by value): the CropArgs of the canonical image, and the surface's luma plane
struct CropSurfArgs {
    CropArgs c;
    size_t y_offset, y_pitch;  // bytes to row 0 of Y, and from a row to the next
    int shift;                 // word samples: the reduction's (surface_px.h)
};

// k_quality_zero / k_quality launch arguments (by value): efx_compare_opts, checked (k_quality.hip)
struct QualityArgs {
    const uint8_t* ref;     // image k of the reference at ref + k * ref_stride
    const uint8_t* test;    // image k of the picture under test at test + k * test_stride
    uint64_t* recs;         // image k: its efx_compare_rec, six 8-byte words at recs + 6 k
    uint32_t* mb_sse;       // image k: 264 words at mb_sse + k * mb_stride; may be null
    size_t ref_stride, test_stride, mb_stride;
    int n_images, ref_max;  // ref_max 1 .. 255 (255: the launch takes the kernel without the clamp)
};

// k_import_pcm / k_import_pcm_state launch arguments (by value): efx_import_pcm_opts, checked, as import_pcm.h's plan
struct ImportPcmArgs {
    const int16_t* src;    // stream i at src + i * src_stride
    int16_t* state;        // stream i: 128 int16 at state + i * 128 (k_import_pcm reads, k_import_pcm_state writes); null when the rates are equal
    int16_t* dst;          // stream i's plan.n_out samples at dst + i * dst_stride
    const int32_t* table;  // the prototype, ipcm::kTableLen entries
    size_t src_stride, dst_stride;
    ipcm::Plan plan;
};

// k_loud_steps / k_loud_state launch arguments (by value): efx_loudness_steps_opts, checked, as loudness_px.h's plan
struct LoudStepsArgs {
    const int16_t* pcm;    // stream i at pcm + i * pcm_stride
    int16_t* state;        // stream i: plan.hist int16 at state + i * plan.hist (k_loud_steps reads, k_loud_state writes)
    loud::StepRec* steps;  // stream i's plan.n_new records at steps + i * steps_stride + first_step
    size_t pcm_stride, steps_stride;
    int first_step;
    loud::Plan plan;
};

// k_loud_gate launch arguments (by value): efx_loudness_gate_opts, checked
struct LoudGateArgs {
    const loud::StepRec* steps;  // stream i's n_steps records at steps + i * steps_stride
    const int16_t* state;        // may be null; stream i: hist int16 at state + i * hist
    loud::GateRec* recs;         // stream i's record at recs + i
    size_t steps_stride;
    uint64_t abs_thr, target_ms;
    uint32_t ceiling;
    int n_steps, step, hist;
};

// k_pcm_gain launch arguments (by value): efx_pcm_gain_opts, checked
struct PcmGainArgs {
    const int16_t* src;          // stream i at src + i * src_stride
    const loud::GateRec* recs;   // null: fixed_gain
    int16_t* dst;                // stream i at dst + i * dst_stride; may be src
    size_t src_stride, dst_stride;
    int n_samples, fixed_gain;
};

// k_limit_peaks launch arguments (by value): efx_limit_peaks_opts, checked
struct LimitPeaksArgs {
    const int16_t* pcm;          // stream i at pcm + i * pcm_stride
    uint16_t* peaks;             // stream i's row at peaks + i * peaks_stride
    size_t pcm_stride, peaks_stride;
    int64_t entry0;              // the row's entry of the call's first block: first_sample / Bk - peaks_first
    int n_samples, bk;
};

// k_pcm_limit launch arguments (by value): efx_limit_opts, checked
struct PcmLimitArgs {
    const int16_t* src;          // stream i at src + i * src_stride
    const uint16_t* peaks;       // stream i's row of n_peaks entries at peaks + i * peaks_stride; entry 0: block peaks_first
    const loud::GateRec* recs;   // null: fixed_gain
    int16_t* dst;                // stream i at dst + i * dst_stride; may be src
    size_t src_stride, dst_stride, peaks_stride;
    int64_t first_block, peaks_first;
    uint64_t target_ms;
    int n_samples, n_peaks, bk, half, ceiling, fixed_gain, step;
    limit::DivBk div;
};

// per-stream result of k_ts_sequences
struct IdxInfo {
    int64_t first_pts, last_pts;  // origin (PTS of the first sequence start whose PTS is not -1; -1: none), last video PES' PTS
    uint32_t n_seq;
    uint32_t fast;                // list sorted and short enough for the binary search
};

// k_composite launch arguments (by value)
struct FieldArgs {
    int first_stream, ring_depth;
    int slot, other_slot;   // ring slots of the displayed frame and of the frame scrolled in
    int frame_counter;      // dither phase
    int hscroll;            // multiple of 8 in (-352, 352)
    const uint8_t* overlay; // device, 16 x 80 bytes per stream (or shared: stride 0); may be null
    size_t overlay_stride;
    int overlay_scale;      // 0 = overlay off; 63 full, (63 * blend) >> 5 while fading
    int overlay_progress;
};

// Packets of a transport stream a k_demux workgroup takes, and its threads (k_demux.hip); a multiple of four packets: 4 x 188
// bytes = 47 x 16.  16 packets x one wave: the benchmark's 253-packet streams as 16 k small workgroups instead of 2 k of 128
// packets x 256 threads, whose few long phases left the chip waiting (gather 81 -> 42 us; profiles/r5_demux.md).
constexpr int kDemuxChunk = 16;
constexpr int kDemuxThreads = 64;
static_assert(kDemuxChunk % 4 == 0 && kDemuxChunk >= 4 && kDemuxChunk <= 256, "k_demux stages whole 16-byte groups");

// SBC synthesis tables (sbc_decoder.cpp:41-71), generated from the A2DP definitions
struct SbcTables {
    int32_t syn[128];   // syn[i * 8 + k] = floor(65536 cos((i + 4)(2k + 1) pi / 16))
    int32_t proto[80];  // proto[i * 10 + j] = floor(-8 * 32768 * Proto_8_80[8 j + i])
    // IQUANT's C division by 2^bits - 1 (sbc_decoder.cpp:263-270) as a multiplication: the round-up constant
    // m' = floor(2^32 (2^l - d) / d) + 1 of Granlund & Montgomery's unsigned division (l = bits; d = 1: m' = 1, no shifts):
    // a / d = (t + ((a - t) >> 1)) >> (bits - 1), t = mulhi(m', a), for every 32-bit a
    uint32_t iq_magic[20];
};

// What k_sbc_frames leaves per (stream, frame): the header's verdict and the bit allocation -- one thread per frame with all
// 64 lanes of a wave busy, instead of once per workgroup that has the frame in reach.
struct alignas(16) SbcFrameInfo {
    uint8_t bits[2][8];       // bits of a sample of (channel, subband)
    uint8_t prefix[2][8];     // ... and where it starts inside a block's bits
    uint16_t per_block;       // bits of one block, all channels
    uint16_t framelen;        // get_samples()'s return value (0xFFFF = -1)
    uint8_t h1, bitpool, flags, pad;
    uint32_t pad2[2];
};
static_assert(sizeof(SbcFrameInfo) == 48, "SbcFrameInfo is moved as three uint4");
constexpr uint32_t kSbcSync = 1, kSbcOk = 2;  // flags: sync byte and length in order (the header moves the geometry); decodable

// What k_sbc_plan leaves per (stream, VIRTUAL frame) of a stream that is not regular (virtual frame v = frame max(v - probe, 0):
// decode_audio()'s frame-size probe decodes frame 0 once more up front).  Everything the reference chains from frame to frame
// -- the geometry a rejected frame is synthesised under, the stale samples it synthesises, where its PCM goes, where its rows
// sit on a channel's timeline of matrixing outputs -- as prefix scans, so that any chunk of frames can be decoded on its own.
struct alignas(16) SbcFramePlan {
    int32_t src[8];     // [q * 2 + c]: the frame whose get_samples() last wrote blocks 4q .. 4q+3 of channel c; -1 = the state's
    uint32_t pcm_off;   // PCM samples of this call before this frame's
    uint32_t vb[2];     // rows on channel c's timeline before this frame's
    int32_t back[2];    // the latest earlier frame with rows on channel c's timeline; -1 = none in this call
    int32_t gsrc;       // the frame whose header left the geometry this frame is synthesised under; -1 = the state's
    uint32_t geom;      // blocks | channels << 8 | synthesised << 16
    uint32_t pad;       // (k_sbc_plan's own: the first frame of the run of frames decoding under one geometry that this frame ends)
};
static_assert(sizeof(SbcFramePlan) == 64, "SbcFramePlan is moved as four uint4");

// efx_sbc_decode's work lists: streams by the kernel that decodes them (kSbcMono / kSbcStereo: regular streams -- every frame
// decodes, one geometry --, kSbcGeneral: the rest), filled by k_sbc_plan, drained by persistent workgroups
constexpr int kSbcMono = 0, kSbcStereo = 1, kSbcGeneral = 2;
struct SbcQueues {
    uint32_t count[4];  // streams on list c
    uint32_t extra[4];  // kSbcMono, kSbcStereo: single chunks of GENERAL streams that a regular kernel can take (SbcExtraItem)
};
// A chunk of a general stream whose frames -- and the frames that hold the nine blocks before it -- all decode under one
// geometry is, but for where its PCM goes, a regular stream's: k_sbc_plan hands it to the regular kernel of its kind.
struct alignas(16) SbcExtraItem {
    uint32_t entry;     // stream | block-count code << 30 (as the list entries of regular streams)
    uint32_t chunk;     // in the kernel's own chunk size
    uint32_t pcm_base;  // PCM samples of the call before the chunk's first frame
    uint32_t pad;
};

// per-stream SBC decoder state (the reference's SBC_Decode, sbc_decoder.h:12-25, with the sliding
// synthesis buffer kept as the last nine rows of matrixing outputs); all zero = sbc_init()
struct SbcState {
    int32_t hist[2][9][16];
    int32_t sb_sample[16][2][8];
    uint8_t frequency, blocks, channels, mode, allocation, subbands, bitpool, reserved;
    uint8_t pad[8];
};
static_assert(sizeof(SbcState) == 2192, "SbcState layout");

// efx_encode (k_encode.hip): per-stream state that carries from call to call (continuation), in HBM
namespace enc {
struct Tables;
}
static_assert(sizeof(enc::RateState) == 24, "RateState layout");
struct EncState {
    uint32_t pictures;  // pictures encoded since the stream started: GOP phase, temporal_reference, PTS
    uint32_t cc;        // TS continuity counter of the next packet
    uint32_t cur;       // which of the stream's two reconstruction buffers holds the newest picture
    uint32_t full;      // the output region of a call filled up: nothing more is written until the stream starts afresh
    uint32_t out_len;   // bytes written by the current call
    uint32_t status;    // EFX_ENCODE_* bits of the current call
    uint32_t g;         // pictures since the stream's last I picture, counting it; 0 = fresh (enc_cut.h)
    uint32_t pad;
    int64_t first_pts;  // PTS of picture 0
    enc::RateState rate;  // efx_encode_rc: buffer level and history (enc_rate.h)
};

// efx_enc_picture_info as k_enc_pack writes it
struct EncPictureInfo {
    uint32_t cut_i, cut_p;
    uint8_t type, pad[3];
};
static_assert(sizeof(EncPictureInfo) == 12, "EncPictureInfo layout");
constexpr int kEncInfoCap = 255;  // pictures of one call at most

// k_encode launch arguments (by value)
struct EncArgs {
    const uint8_t* src;  // I420 pictures: stream i, picture p at src + i * src_stride + p * 101376
    size_t src_stride;
    uint8_t* dst;  // output region of stream i at dst + i * dst_stride
    size_t dst_stride;
    uint32_t* len;
    uint32_t* status;
    uint8_t* recon;           // may be null: reconstruction of (stream i, picture p) at recon + (i * n_pictures + p) * 101376
    EncState* st;
    uint8_t* pics;            // two I420 reconstruction buffers per stream
    uint8_t* slices;          // per (stream, row): the coded slice, enc::kSliceCap bytes apart
    uint32_t* slice_len;
    const enc::Tables* tab;
    uint32_t* full_flag;      // host-mapped: set to `generation` when a stream fills its region (efx_encode's continuation check)
    uint32_t generation;      // of the streams: counts the fresh efx_encode calls of the context
    int64_t first_pts;
    int n_streams, n_pictures, picture, qscale, gop, search, format, f_code, cont;
    int rate_code;            // picture_rate of the streams, 1 .. 8 (efx_encode_set_picture_rate; enc_core.h)
    // efx_encode_rc (rc = 1): the quantiser of every picture comes from enc::rate_decide, not from qscale
    int rc;
    enc::RateParams rate;     // (gain: of the default picture rate; the kernels put every picture's own in its place)
    int64_t bitrate;
    uint32_t* act;            // per (stream, row): the row's summed dev and summed min(dev, zero-vector SAD) (k_enc_act)
    uint8_t* qscale_out;      // may be null: the quantiser of (stream i, picture p) at qscale_out + i * n_pictures + p, 0 = not written
    // scene cuts (enc_cut.h): cut.threshold 0 = off, k_enc_cut is not launched and the sums read as 0
    enc::CutParams cut;
    uint8_t* cut_pics;        // two decimated source pictures (enc::kCutBytes) per stream, indexed by pictures & 1
    uint32_t* cut_sums;       // per (stream, row): the row's cut_i and cut_p (k_enc_cut)
    EncPictureInfo* info;     // per (stream, picture of the call): stream i's at info + i * 255 (k_enc_pack)
    // adaptive quantisation (enc_aq.h): aq.strength 0 = off, k_enc_aq is not launched and none of the three is read or written
    enc::AqParams aq;
    uint16_t* aq_act;         // per (stream, row): the activities of the row's 22 macroblocks (k_enc_aq)
    uint32_t* aq_sums;        // per (stream, row): their sum
    uint8_t* aq_map;          // per (stream, picture of the call): 264 quantisers, stream i's at aq_map + i * 255 * 264 (k_enc_rows)
};

// k_conform (k_conform.hip) launch arguments (by value): efx_conform_opts, checked.  Items and runs are k_trick's.
struct ConformArgs {
    const uint8_t* src;  // stream i, picture j of the call at src + i * src_stride + j * 101376
    uint8_t* dst;        // stream i, output n0 + m at dst + i * dst_stride + m * 101376
    size_t src_stride, dst_stride;
    int64_t A, B;           // the reduced ratio of conform_sel.h
    int64_t first_picture;  // title index of the call's picture 0
    int64_t n0;             // the call's first output
    int n_streams, n_out;
};

// k_deint (k_deint.hip) launch arguments (by value): efx_deint_opts, checked, and the surface, checked (deint_px.h)
struct DeintArgs {
    const uint8_t* src;  // stream i, frame j of the call at src + (i * n_frames + j) * src_stride
    uint8_t* dst;        // stream i, output m at dst + (i * n_out + m) * dst_stride: packed I420, width x height
    size_t src_stride, dst_stride;
    efx_surface s;
    int n_streams, n_frames;
    int lead, frames_out;  // frames lead .. lead + frames_out - 1 of a stream have outputs
    int per_frame;         // outputs per frame: 1 (frame rate) or 2 (field rate)
    int first_field;
    int frame_items;       // dpx::frame_items(width, height)
};

// k_telecine_* (k_telecine.hip) launch arguments (by value): efx_detelecine_opts, checked, and the surface, checked
struct TelecineArgs {
    const uint8_t* src;       // stream i, frame j of the call at src + (i * n_frames + j) * src_stride
    uint8_t* dst;             // stream i, output m at dst + (i * n_out + m) * dst_stride: packed I420, width x height
    efx_telecine_info* info;  // stream i, processed frame j at info + i * n + j
    size_t src_stride, dst_stride;
    efx_surface s;
    int n_streams, n_frames;
    int lead, n, n_out;       // frames lead .. lead + n - 1 of a stream are processed and give n_out outputs
    int first_field, nt;
    int measure_items, weave_items;  // tpx::measure_items(width, height), tpx::weave_items(surface)
};

// k_scan_measure / k_scan_count (k_scan.hip) launch arguments (by value): efx_scan_opts, checked, and the surface, checked
// (scan_px.h)
struct ScanArgs {
    const uint8_t* src;      // stream i, frame j of the call at src + (i * n_frames + j) * src_stride
    efx_scan_frame* frames;  // stream i, processed frame j at frames + i * n + j
    efx_scan_rec* recs;      // stream i's counts at recs + i
    size_t src_stride;
    efx_surface s;
    int n_streams, n_frames;
    int lead, n;             // frames lead .. lead + n - 1 of a stream are processed
    int accumulate, nt;
    uint64_t first_frame;    // the title's frame number of the first offered frame
    uint64_t still_wh;       // scpx::Rule: still x width x height, and the three Q8 ratios
    uint32_t prog, intl, rep;
    int measure_items;       // scpx::measure_items(width, height)
};

// k_denoise (k_denoise.hip) launch arguments (by value): efx_denoise_opts, checked, and the surface, checked (denoise_px.h)
struct DenoiseArgs {
    const uint8_t* src;   // stream i, frame j of the call at src + (i * n_frames + j) * src_stride
    const uint8_t* prev;  // stream i's last output of the previous piece at prev + i * prev_stride: packed I420; NULL = none
    uint8_t* dst;         // stream i, output j at dst + (i * n_frames + j) * dst_stride: packed I420, width x height
    size_t src_stride, dst_stride, prev_stride;
    efx_surface s;
    int n_streams, n_frames;
    int ts[2], tt[2];     // the spatial and temporal thresholds of luma [0] and chroma [1]
    uint32_t q[2];        // npx::blend_q of tt
    int stream_items;     // npx::stream_items(width, height)
};

// k_overlay (k_overlay.hip) launch arguments (by value): efx_overlay_opts, checked (overlay_px.h)
struct OverlayArgs {
    const efx_overlay_event* events;  // n_events records
    const uint8_t* atlas;             // the bitmaps; readable up to atlas_bytes rounded up to 16
    uint8_t* pictures;                // stream i, picture j at pictures + i * stride + j * 101376
    uint32_t* status;                 // n_streams words, or NULL
    size_t stride;
    uint64_t atlas_bytes;
    int64_t first_picture;            // the title index of the call's picture 0
    int n_streams, n_pictures, n_events;
};

// k_sbc_enc launch arguments (by value): efx_sbc_encode_opts, checked, with the context's tables
namespace sbcenc {
struct Tables;
}
struct SbcEncArgs {
    const int16_t* pcm;   // stream i at pcm + i * pcm_stride
    int16_t* state;       // stream i: 2 x 72 samples at state + i * 144 (k_sbc_enc reads, k_sbc_enc_state writes)
    uint8_t* frames;      // stream i, frame f at frames + i * frame_stride + f * frame_bytes
    const sbcenc::Tables* tables;
    size_t pcm_stride, frame_stride;
    uint32_t frame_bytes;
    int n_streams, n_frames, n_groups;  // n_groups: workgroups' worth of frames per stream (four frames each)
    int frequency, blocks, mode, allocation, bitpool, layout;
};

// k_mux launch arguments (by value): efx_mux_opts, checked
struct MuxArgs {
    const uint8_t* video;      // stream i's transport stream at video + i * video_stride, video_len[i] bytes
    const uint32_t* video_len;
    const uint8_t* audio;      // stream i's frames at audio + i * audio_stride
    uint8_t* dst;
    uint32_t* len;
    uint32_t* status;
    uint32_t* video_before;    // scratch, per (stream, audio PES): video packets in front of it
    size_t video_stride, audio_stride, dst_stride;
    int64_t first_pts, first_frame;
    int n_streams, pid, frame_bytes, n_frames, frames_per_pes, samples_per_frame, sample_rate, cc;
    int n_pes, pes_packets, audio_packets;  // audio PES of a stream, packets of a full one, audio packets of a stream
};

void build_sbc_tables(SbcTables* t);
void build_import_pcm_table(int32_t* T);  // ipcm::kTableLen entries
namespace hdr {
struct Tables;
}
bool build_import_hdr_tables(hdr::Tables* t);  // t->k filled in (hdr_px.h): the two tables for t->k.peak_nits
void build_parse_tables(ParseTables* t);
void build_video_tables(int ntsc, VideoTables* t);

}  // namespace efx
