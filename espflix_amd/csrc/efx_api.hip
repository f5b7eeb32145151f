// efx_api.hip -- the C-ABI of libefx (include/efx.h): context, uploads, kernel launches.
//
// Host orchestration only; all arithmetic of the hot path lives in the k_*.hip kernels.  There
// is no CPU fallback anywhere: without a gfx950 device efx_create fails with
// EFX_ERR_NO_DEVICE / EFX_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <thread>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "efx.h"
#include "conform_sel.h"
#include "efx_internal.h"
#include "enc_core.h"
#include "colour_px.h"
#include "hdr_px.h"
#include "import_px.h"
#include "crop_px.h"
#include "deint_px.h"
#include "denoise_px.h"
#include "overlay_px.h"
#include "telecine_px.h"
#include "scan_px.h"
#include "surface_px.h"
#include "quality_px.h"
#include "parse_tm.h"
#include "sbc_enc_core.h"
#include "trick_sel.h"

namespace efx {
// kernels (k_demux.hip, k_index.hip, k_parse.hip, k_recon.hip, k_video.hip)
struct DemuxChunk;
__global__ void k_demux_scan(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*, DemuxChunk*);
__global__ void k_demux_offsets(const uint32_t*, const uint32_t*, DemuxChunk*, uint8_t*, const uint64_t*, uint32_t*, uint32_t*);
__global__ void k_demux(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*, const DemuxChunk*, uint8_t*, PesEntry*);
__global__ void k_demux_audio_scan(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*, DemuxChunk*);
__global__ void k_demux_audio_offsets(const uint32_t*, const uint32_t*, DemuxChunk*, uint32_t*);
__global__ void k_demux_audio(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*, const DemuxChunk*, uint8_t*, const uint64_t*);
__global__ void k_ts_sequences(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*, PesEntry*, IdxInfo*);
__global__ void k_idx_bins(const PesEntry*, const uint32_t*, const IdxInfo*, uint32_t, uint32_t*, size_t);
__global__ void k_index(const uint8_t*, const uint64_t*, int, PicInfo*, SliceTmp*, uint32_t*, uint32_t*, uint32_t*,
                        const uint32_t*, const PesEntry*, const uint32_t*, const uint32_t*, int64_t*, int64_t*, int, int, int);
__global__ void k_advance(StreamState*, const uint32_t*, int64_t*, const int64_t*, int, int, int, int32_t*);
__global__ void k_slice_scan(const PicInfo*, const uint32_t*, int, int, const uint32_t*, uint32_t*, DecodeCounters*);
__global__ void k_slice_emit(const PicInfo*, const SliceTmp*, const uint32_t*, const uint64_t*, const uint32_t*, int, int,
                             const uint32_t*, SliceDesc*, uint32_t*);
__global__ void k_parse(const uint8_t*, const SliceDesc*, DecodeCounters*, const TmTables*, MbRec*, TmU4*, uint32_t*, uint32_t*,
                        int, int);
__global__ void k_recon(const MbRec*, const uint32_t*, const uint32_t*, const uint32_t*, uint8_t*, int, int, int, const int32_t*, int, int);

__global__ void k_frame_hash(const uint8_t*, int, uint64_t*);
__global__ void k_fill(uint32_t*, uint32_t, size_t);
__global__ void k_composite(const uint8_t*, const VideoTables*, const VideoLineTemplates*, FieldArgs, uint16_t*);
__global__ void k_pdm(const int16_t*, int, int, int32_t*, uint16_t*);
template <int FMT, int CHROMA>
__global__ void k_export(const uint8_t*, int, ExportArgs);  // (k_export.hip: the five (format, chroma) instances)
__global__ void k_import_taps(ImportTap*, ImportArgs);  // (k_import.hip)
__global__ void k_import(const uint8_t*, uint8_t*, const ImportTap*, ImportArgs);
__global__ void k_import_surf8p(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs);
__global__ void k_import_surf8s(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs);
__global__ void k_import_surf16p(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs);
__global__ void k_import_surf16s(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs);
__global__ void k_import_surf8p_c(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs, colour::Coefs);  // (... with the colour stage)
__global__ void k_import_surf8s_c(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs, colour::Coefs);
__global__ void k_import_surf16p_c(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs, colour::Coefs);
__global__ void k_import_surf16s_c(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs, colour::Coefs);
__global__ void k_import_surf8p_h(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs, const hdr::Tables*);  // (... with the HDR stage)
__global__ void k_import_surf8s_h(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs, const hdr::Tables*);
__global__ void k_import_surf16p_h(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs, const hdr::Tables*);
__global__ void k_import_surf16s_h(const uint8_t*, uint8_t*, const ImportTap*, ImportSurfArgs, const hdr::Tables*);
__global__ void k_crop_zero(CropArgs);  // (k_cropdetect.hip)
__global__ void k_crop_sums_i420(CropArgs);
__global__ void k_crop_sums_rgb24(CropArgs);
__global__ void k_crop_sums_rgbp(CropArgs);
__global__ void k_crop_sums_surf8(CropSurfArgs);
__global__ void k_crop_sums_surf16(CropSurfArgs);
__global__ void k_crop_rects(CropArgs);
__global__ void k_quality_zero(QualityArgs);  // (k_quality.hip)
__global__ void k_quality(QualityArgs);
__global__ void k_quality_clamp(QualityArgs);
template <int SOURCE>
__global__ void k_trick(TrickArgs);  // (k_trick.hip: the I420 and the ring instance)
__global__ void k_conform(ConformArgs);  // (k_conform.hip)
__global__ void k_deint(DeintArgs);      // (k_deint.hip)
__global__ void k_denoise(DenoiseArgs);  // (k_denoise.hip)
__global__ void k_overlay(OverlayArgs);  // (k_overlay.hip)
__global__ void k_telecine_measure(TelecineArgs);  // (k_telecine.hip)
__global__ void k_telecine_decide(TelecineArgs);
__global__ void k_telecine_weave(TelecineArgs);
__global__ void k_scan_measure(ScanArgs);  // (k_scan.hip)
__global__ void k_scan_count(ScanArgs);
__global__ void k_import_pcm(ImportPcmArgs);  // (k_import_pcm.hip)
__global__ void k_import_pcm_state(ImportPcmArgs);
__global__ void k_loud_steps(LoudStepsArgs);  // (k_loudness.hip)
__global__ void k_loud_state(LoudStepsArgs);
__global__ void k_loud_gate(LoudGateArgs);
__global__ void k_pcm_gain(PcmGainArgs);
__global__ void k_limit_peaks(LimitPeaksArgs);  // (k_limit.hip)
__global__ void k_pcm_limit(PcmLimitArgs);
__global__ void k_enc_begin(EncArgs);
__global__ void k_enc_aq(EncArgs);
__global__ void k_enc_cut(EncArgs);
__global__ void k_enc_act(EncArgs);
template <bool kAq>
__global__ void k_enc_rows_t(EncArgs);  // k_encode.hip instantiates both
__global__ void k_enc_pack(EncArgs);
__global__ void k_sbc(const uint8_t*, size_t, int, int, SbcState*, const SbcTables*, int16_t*, size_t, uint32_t*, uint32_t*, int);
__global__ void k_sbc_frames(const uint8_t*, size_t, int, int, SbcFrameInfo*, uint32_t*, uint32_t*, SbcQueues*);
__global__ void k_sbc_plan(const SbcFrameInfo*, int, int, const SbcState*, SbcFramePlan*, uint32_t*, SbcQueues*, uint32_t*, int, int, uint32_t*,
                           uint32_t*, SbcExtraItem*, uint8_t*);
__global__ void k_sbc_par_stereo(const uint8_t*, size_t, int, int, const SbcState*, SbcState*, const SbcTables*, const SbcFrameInfo*, int16_t*,
                                 size_t, uint32_t*, int, SbcQueues*, const uint32_t*, int, const SbcExtraItem*, int);
__global__ void k_sbc_par_mono(const uint8_t*, size_t, int, int, const SbcState*, SbcState*, const SbcTables*, const SbcFrameInfo*, int16_t*,
                               size_t, uint32_t*, int, SbcQueues*, const uint32_t*, int, const SbcExtraItem*, int);
__global__ void k_sbc_gen(const uint8_t*, size_t, int, int, const SbcState*, SbcState*, const SbcTables*, const SbcFrameInfo*,
                          const SbcFramePlan*, int16_t*, size_t, int, SbcQueues*, const uint32_t*, int, const uint8_t*, int);
__global__ void k_sbc_finish(const uint8_t*, size_t, int, int, SbcState*, const SbcState*, const SbcTables*, int16_t*, size_t, uint32_t*,
                             uint32_t*, int, uint32_t*);
__global__ void k_sbc_enc(SbcEncArgs);
__global__ void k_sbc_enc_state(SbcEncArgs);
__global__ void k_mux(MuxArgs);
}  // namespace efx

using namespace efx;

constexpr int kSbcMonoWgPerCu = 4;  // k_sbc_par_mono workgroups per compute unit (k_sbc.hip: kSbcMonoWaves)

constexpr int kParseStreams = 2;    // parse halves in flight at once (latency-bound kernels: two overlap well)
constexpr int kMaxGroups = 16;      // an efx_decode call parses its streams in up to this many parse halves
static_assert(kMaxGroups <= kExportMaxGroups, "k_export takes every reconstruction group of a call");
constexpr int kGroupStreams = 1024;
constexpr int kTimingRing = 64;   // efx_decode calls whose stage times efx_get_timing can average
constexpr int kSlots = 3;         // parse -> recon hand-over buffer sets (one being reconstructed + two being parsed)
constexpr int kUploads = 3;       // bitstream buffers: up to two being parsed (two parse halves are in flight), one being filled --
                                  // with two, an upload had to wait for the parse half two calls back before its transfer could start

struct efx_ctx {
    efx_config cfg{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool pooled_streams = false;  // the parse / copy (and, if own_stream, reconstruction) streams go back to the pool
    unsigned stream_serial = 0;
    std::string err;

    size_t es_cap = 0;  // bytes of one ES buffer (including tails and guard)
    bool decoded = false, results_valid = false;

    ParseTables* d_tables = nullptr;
    TmTables* d_tm_tables = nullptr;  // the token machine's tables (parse_tm.h)
    uint8_t* d_frames = nullptr;
    StreamState* d_state = nullptr;  // per stream: ring position, "a PTS has been seen", newest PES PTS (k_advance)

    // One resident batch of bitstreams.  efx_upload_streams fills the buffer the last decode does NOT read
    // (staging copy on the host, H2D and k_demux on the copy stream) while the GPU still decodes the other
    // one: ingest and decode of consecutive batches overlap.
    struct Upload {
        uint8_t* d_es = nullptr;
        uint64_t* d_stream_off = nullptr;
        uint32_t* d_stream_perm = nullptr;  // streams by descending length: the order of slices inside a picture index
        // transport-stream input (allocated on the first EFX_FORMAT_TS upload)
        uint32_t* d_ts_len = nullptr;    // per stream: TS bytes
        uint32_t* d_pkt_base = nullptr;  // per stream: first entry of its PES list (= packets before it)
        uint32_t* d_es_len = nullptr;    // per stream: demuxed ES bytes (without tail)
        uint32_t* d_pes_count = nullptr;
        PesEntry* d_pes = nullptr;
        uint8_t* h_es = nullptr;         // pinned staging: the bitstreams, then the small per-stream arrays
        uint8_t* h_meta = nullptr;       // pinned: stream_off (n + 1 x u64) | perm | ts_len | pkt_base (n x u32 each)
        std::vector<uint64_t> stream_off;
        std::vector<uint32_t> es_len;    // per stream, ES input only
        int n_streams = 0;
        int sort_groups = 1;  // d_stream_perm orders the streams by length INSIDE each of this many groups (group_first)
        size_t es_used = 0, ts_bytes = 0;
        bool ts_input = false, valid = false;
        hipEvent_t uploaded = nullptr;                                  // H2D (+ k_demux) done, copy stream
        hipEvent_t last_read[kParseStreams] = {};       // newest parse half that reads this buffer
        hipEvent_t ev_demux[2] = {nullptr, nullptr};
        bool demux_timed = false;
    } up[kUploads];
    int cur_up = -1;  // batch the next efx_decode reads
    // page-locked host arenas the caller lays batches out in (efx_host_alloc / efx_host_register): base, bytes, ours to free
    struct Arena {
        uint8_t* base;
        size_t bytes;
        bool owned;
    };
    std::vector<Arena> arenas;
    hipStream_t copy_stream = nullptr;
    // transient TS staging on the device + the lists of efx_index_streams / efx_demux_audio
    uint8_t* d_ts = nullptr;
    DemuxChunk* d_demux_chunks = nullptr;  // k_demux's per-chunk totals / bases (16 bytes each; one demux runs at a time)
    size_t pes_cap = 0;
    IdxInfo* d_idx_info = nullptr;
    uint64_t* d_ts_off = nullptr;
    uint32_t* d_idx_len = nullptr;
    uint32_t* d_idx_base = nullptr;
    PesEntry* d_idx_seq = nullptr;
    bool ts_ready = false;  // every transport-stream buffer and event exists

    // kSlots sets of parse -> recon hand-over buffers: efx_decode() number n parses into slot
    // n % kSlots on parse stream n % kParseStreams while the recon stream is still reconstructing
    // earlier calls from the other slots.  The parse half is bound by the latency of its longest
    // waves (3 waves per SIMD, ~1/3 of the issue slots used), so back-to-back decodes keep two parse
    // halves and one reconstruction half on the GPU at once.  Every slot carries its own
    // index / slice-list scratch.
    struct Slot {
        uint32_t* d_pic_count = nullptr;
        uint32_t* d_status = nullptr;
        DecodeCounters* d_counters = nullptr;  // kMaxGroups of them: one per group of a call
        MbRec* d_mbrecs = nullptr;
        TmU4* d_raw = nullptr;       // k_parse's own scratch: raw macroblock records, pass 1 -> pass 2 (same shape as d_mbrecs)
        uint32_t* d_coefs = nullptr;
        // index / slice-list scratch of this call (per slot: two parse halves run concurrently)
        PicInfo* d_pics = nullptr;
        SliceTmp* d_slices_tmp = nullptr;
        uint32_t* d_qtab = nullptr;  // per (stream, picture) custom quantiser tables, read by k_recon
        uint32_t* d_slice_base = nullptr;
        SliceDesc* d_descs = nullptr;
        int64_t* d_pts = nullptr;    // per (stream, picture): PTS latched at the picture header (TS input); then, per
                                     // stream, the newest PES PTS of the upload (k_index -> k_advance)
        int32_t* d_call_pos = nullptr;  // per stream: ring position of this call's first picture, first picture with a PTS
        hipEvent_t parse_done = nullptr, recon_done = nullptr;
        int epoch = 0;
        int upload = 0;  // batch this call decoded
    } slot[kSlots];
    // stage timing: one event set per efx_decode call since efx_set_timing(1), so that a run of
    // back-to-back (overlapping) calls can be averaged afterwards without a host sync in between
    struct TimingEvents {
        // per group: parse start, index end, parse end (its parse stream), recon end [3] and recon start [4] (context stream)
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    };
    std::vector<TimingEvents> timing_ring;  // kTimingRing x kMaxGroups sets, created by efx_set_timing
    uint64_t timed_calls = 0;               // calls recorded since timing was (re-)enabled
    struct Group {
        int slot, first, count;  // hand-over slot, streams [first, first + count); its counters: d_counters[its index]
    };
    Group groups[kMaxGroups];  // reconstruction groups of the most recent efx_decode
    int n_groups = 0;
    hipEvent_t last_recon_done = nullptr;  // end of the most recently queued reconstruction group
    // Reconstruction groups queued since the host last KNEW the reconstruction stream idle (context creation, any call that
    // synchronises it: sync_all).  The launch structure of a decode call is decided from this count, not from a hipEventQuery of
    // the stream (round 5: a race against the GPU -- the same call sequence could run different launches from run to run):
    // 0 = the call finds the stream idle by the library's own book-keeping (it is split into groups, its first parse half may
    // have the whole chip), otherwise it pipelines against what is queued (one group, capped parser).  A caller that lets the
    // GPU drain WITHOUT synchronising is treated as back to back: that costs the one call some latency, never a result.
    uint64_t recon_groups_unsynced = 0;
    int last_upload = 0;       // batch the most recent efx_decode read
    int last_n_streams = 0;    // ... its stream count and format, as they were when the decode was queued (a later upload may
    bool last_ts_input = false;  // have recycled the Upload record by the time the results are fetched)
    uint64_t subcalls = 0;     // reconstruction groups launched so far: group k uses slot k % kSlots
    uint64_t parse_calls = 0;  // parse halves launched so far: half k runs on parse stream k % kParseStreams
    uint8_t timing_groups[kTimingRing] = {};    // groups of the timed call
    uint16_t timing_launches[kTimingRing] = {};  // reconstruction kernel launches of the timed call
    hipStream_t parse_streams[kParseStreams] = {};
    VideoTables* d_video[2] = {nullptr, nullptr};  // [0] PAL, [1] NTSC
    VideoLineTemplates* d_video_lines[2] = {nullptr, nullptr};
    SbcTables* d_sbc_tables = nullptr;
    sbcenc::Tables* d_sbc_enc_tables = nullptr;  // efx_sbc_encode's window and matrix (sbc_enc_core.h)
    uint32_t* d_mux_before = nullptr;            // efx_mux_av's scratch: per (stream, audio PES) the video packets in front of it
    size_t mux_before_cap = 0;
    ImportTap* d_import_taps = nullptr;          // efx_import_frames' tap table: written and read on the device, in stream order
    bool import_colour_on = false;               // efx_import_set_colour: the source matrix and range of the imports that follow
    efx_import_colour import_colour = {6, 0};
    bool import_hdr_on = false;                  // efx_import_set_hdr: supersedes the colour setting while it is on
    efx_import_hdr import_hdr = {16, 9, 9, 0, 0};
    struct HdrCopy {                             // one per distinct setting the context has used: the launch carries `device`
        hdr::Tables host;                        // the upload's source, alive until efx_destroy
        hdr::Tables* device = nullptr;
    };
    std::vector<std::unique_ptr<HdrCopy>> import_hdr_copies;
    int32_t* d_import_pcm_table = nullptr;       // efx_import_pcm's prototype filter (import_pcm.h, efx_tables.cpp)
    uint32_t* d_crop_sums = nullptr;             // efx_detect_crop's row and column sums when the caller gives no buffer:
    size_t crop_sums_cap = 0;                    // allocated at the first such call, regrown when a call needs more (elements)
    int parse_wg_cap = 0;  // k_parse workgroups resident per parse kernel while reconstruction launches are queued (0: no cap); EFX_PARSE_WG_CAP
    // launch structure (efx_set_option; the environment variables of the same names, upper case with EFX_, set the defaults)
    int opt_groups = 0;        // reconstruction groups per call: 0 = one group behind a busy reconstruction stream, groups of
                               // kGroupStreams streams when it is idle; n >= 1: always n
    int opt_parse_cap = 0;     // 0 = cap the parse kernel's residency only while reconstruction is queued; 1 always; 2 never
    int n_cus = 256;
    // efx_sbc_decode's scratch.  d_sbc_flags: n words per stream-indexed array -- [0, n) which kernel decodes the stream
    // (k_sbc_frames / k_sbc_plan), [n, 4n) the three work lists; then the SbcQueues
    uint32_t* d_sbc_flags = nullptr;
    SbcState* d_sbc_next = nullptr;   // the state a frame-parallel kernel leaves, put in place by k_sbc_commit
    size_t sbc_flags_cap = 0;
    SbcFrameInfo* d_sbc_info = nullptr;  // per (stream, frame)
    SbcFramePlan* d_sbc_plan = nullptr;  // per (stream, frame + 1)
    SbcExtraItem* d_sbc_extra = nullptr; // two lists of (stream, granule of eight frames) capacity each
    uint8_t* d_sbc_cover = nullptr;      // per (stream, granule): a regular kernel decodes it
    size_t sbc_info_cap = 0;             // in frames: streams x (frames + 1)
    size_t sbc_gran_cap = 0;             // in granules: streams x ceil(frames / 8)
    int opt_sbc_serial = 0;              // 1 = every stream through k_sbc, one wave per stream (the tests' comparison)
    bool sbc_flags_clean = false;        // d_sbc_flags[0, n) all kSbcRegularFlag (k_sbc_finish leaves them so)
    uint64_t* d_hash = nullptr;

    // efx_encode's state and scratch (allocated at the first call, for max_streams streams)
    EncState* d_enc_state = nullptr;
    uint8_t* d_enc_pics = nullptr;       // two I420 reconstruction buffers per stream
    uint8_t* d_enc_slices = nullptr;     // 12 slices of enc::kSliceCap bytes per stream
    uint32_t* d_enc_slice_len = nullptr;
    uint32_t* d_enc_act = nullptr;       // efx_encode_rc: two activity sums per (stream, macroblock row)
    uint8_t* d_enc_cut_pics = nullptr;   // scene cuts: two decimated source pictures per stream (enc_cut.h)
    uint32_t* d_enc_cut_sums = nullptr;  // ... two sums per (stream, macroblock row)
    EncPictureInfo* d_enc_info = nullptr;  // efx_encode_picture_info: kEncInfoCap records per stream, of the latest call
    enc::Tables* d_enc_tables = nullptr;
    std::unique_ptr<enc::Tables> h_enc_tables;  // the source of d_enc_tables' upload
    uint32_t* h_enc_full = nullptr;      // host-mapped: enc_generation of the streams when one of them last filled its region
    uint32_t* d_enc_full = nullptr;      // ... its device address
    bool enc_ready = false;              // every buffer above exists
    bool enc_started = false;            // streams exist that cont = 1 may continue
    uint32_t enc_generation = 0;         // fresh efx_encode calls so far: the value a call writes to *h_enc_full when a stream fills up
    int enc_n_streams = 0, enc_format = 0, enc_gop = 0;  // of the call that started them
    int enc_rate_code = enc::kRateDefault;  // ... and their picture_rate
    int enc_next_rate_code = enc::kRateDefault;  // efx_encode_set_picture_rate: the picture_rate of the streams a cont = 0 call starts
    bool enc_rc = false;                 // ... which was efx_encode_rc, at enc_bitrate / enc_vbv_bits
    int enc_bitrate = 0, enc_vbv_bits = 0;
    enc::CutParams enc_cut{0, 1};        // scene-cut settings of the streams cont = 1 continues
    enc::CutParams enc_next_cut{0, 1};   // efx_encode_set_scene_cut: those of the streams a cont = 0 call starts
    int enc_info_streams = 0, enc_info_pictures = 0;  // streams and pictures of the latest call (0: no call yet)
    enc::AqParams enc_aq{0};             // adaptive quantisation of the streams cont = 1 continues (enc_aq.h)
    enc::AqParams enc_next_aq{0};        // efx_encode_set_adaptive_quant: that of the streams a cont = 0 call starts
    bool enc_info_aq = false;            // the latest call ran with adaptive quantisation: d_enc_aq_map holds its quantisers
    uint16_t* d_enc_aq_act = nullptr;    // adaptive quantisation, allocated by the first encode with it on: 22 activities
    uint32_t* d_enc_aq_sums = nullptr;   // ... and their sum per (stream, macroblock row)
    uint8_t* d_enc_aq_map = nullptr;     // ... kEncInfoCap maps of 264 quantisers per stream, of the latest call

    // results of the last decode (fetch_results)
    int n_streams = 0;  // streams of the batch the last decode read
    std::vector<int64_t> h_pts;  // per (stream, picture), TS input only
    std::vector<uint32_t> h_pic_count, h_status;
    std::vector<int32_t> h_call_pos;
    DecodeCounters h_counters{};

    bool timing = false;
};

namespace {

// The streams of a context -- reconstruction, parse, copy -- are kept when the context goes and handed to the next context
// on the same device.  Where a stream's hardware queue sits on the command processor's pipes decides whether the parse
// halves run BESIDE the reconstruction or take turns with it (efx_create), and the runtime deals recycled queues out in
// whatever order they came back: the second context of a process decoded the same batch at 4.8 instead of 8.2 M
// frames/s (tools/efx_scale, round 3).  With the set reused as a whole every later context runs where the first one ran.
struct StreamSet {
    hipStream_t recon = nullptr, parse[kParseStreams] = {}, copy = nullptr;
    unsigned serial = 0;  // creation order: the oldest parked set of a device is handed out first (the first set a process
                          // creates is the one whose queues were dealt in the order efx_create asks for)
};
unsigned g_set_serial = 0;
std::mutex g_pool_guard;
std::vector<std::pair<int, StreamSet>> g_stream_pool;  // (device, parked set)

bool take_stream_set(int device, StreamSet* out)
{
    std::lock_guard<std::mutex> lk(g_pool_guard);
    size_t best = g_stream_pool.size();
    for (size_t i = 0; i < g_stream_pool.size(); i++)
        if (g_stream_pool[i].first == device && (best == g_stream_pool.size() || g_stream_pool[i].second.serial < g_stream_pool[best].second.serial))
            best = i;
    if (best == g_stream_pool.size())
        return false;
    *out = g_stream_pool[best].second;
    g_stream_pool.erase(g_stream_pool.begin() + (ptrdiff_t)best);
    return true;
}
void park_stream_set(int device, const StreamSet& set)
{
    std::lock_guard<std::mutex> lk(g_pool_guard);
    g_stream_pool.emplace_back(device, set);
}

// An efx_decode call that finds the GPU idle runs as G groups of about kGroupStreams streams, one after the other: each
// group is a complete parse half + reconstruction half with its own hand-over slot, so that the parse half of the next
// group runs beside the reconstruction of this one -- the call pipelines inside itself.  Back-to-back calls pipeline
// against each other and run as one group (efx_decode_range).  Streams are independent: results do not depend on G.
int group_count(int n_streams)
{
    int g = (n_streams + kGroupStreams / 2) / kGroupStreams;
    return g < 1 ? 1 : (g > kMaxGroups ? kMaxGroups : g);
}
// streams [first, end) of group g: boundaries on multiples of 8, so that a stream's workgroups stay on one XCD
int group_first(int n_streams, int groups, int g)
{
    return g >= groups ? n_streams : (int)(((int64_t)n_streams * g / groups) & ~7);
}

// A context's device is made current on every entry: efx_multi_context() hands per-device contexts to the caller's own
// thread (composite, PDM, timing, raw allocation), whose current device is whatever it was.
void bind_device(efx_ctx* c);

int fail(efx_ctx* c, int code, const char* what, hipError_t e = hipSuccess)
{
    if (c) {
        c->err = what;
        if (e != hipSuccess) {
            c->err += ": ";
            c->err += hipGetErrorString(e);
        }
    }
    return code;
}

#define EFX_HIP(call)                                              \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess)                                      \
            return fail(ctx, EFX_ERR_DEVICE, #call, e_);           \
    } while (0)

// ---- device memory ------------------------------------------------------------------------------------------------------
// Product: hipMalloc.  With EFX_GUARD=1 (or 2) in the environment every device buffer of the library -- and every buffer
// handed out through efx_device_alloc -- is its own virtual-memory mapping (hipMemAddressReserve / hipMemCreate / hipMemMap)
// that ENDS on the last mapped byte of its range (mode 1; mode 2: starts on the first), with an unmapped page on either
// side: a kernel that reads or writes one byte too far faults at once ("Memory access fault by GPU", the kernel named
// under AMD_SERIALIZE_KERNEL=3) instead of quietly touching whatever hipMalloc's pooling put there.  A debugging aid
// (bench.py --soak, profiles/r5_fault_hunt.md): the kernels' deliberate over-reads -- k_recon's window rows behind the
// last frame, the parse lanes' read-ahead behind the last stream -- stay inside the slack their buffers are allocated with.
struct GuardRec {
    void* va;
    size_t va_bytes, map_bytes, gran;
    hipMemGenericAllocationHandle_t handle;
};
std::mutex g_guard_lock;
std::vector<std::pair<void*, GuardRec>> g_guard_recs;

int guard_mode()
{
    static const int mode = [] {
        const char* e = getenv("EFX_GUARD");
        const int m = e ? atoi(e) : 0;
        if (m)
            fprintf(stderr, "libefx: EFX_GUARD=%d -- every device buffer is its own mapping between two unmapped pages (%s-aligned)\n", m,
                    m == 2 ? "start" : "end");
        return m;
    }();
    return mode;
}

hipError_t guard_alloc(void** out, size_t bytes)
{
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess)
        return e;
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    if ((e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum)) != hipSuccess)
        return e;
    if (bytes == 0)
        bytes = 16;
    GuardRec r{};
    r.gran = gran;
    r.map_bytes = (bytes + gran - 1) / gran * gran;
    r.va_bytes = r.map_bytes + 2 * gran;
    if ((e = hipMemAddressReserve(&r.va, r.va_bytes, 0, nullptr, 0)) != hipSuccess)
        return e;
    if ((e = hipMemCreate(&r.handle, r.map_bytes, &prop, 0)) != hipSuccess) {
        (void)hipMemAddressFree(r.va, r.va_bytes);
        return e;
    }
    char* base = static_cast<char*>(r.va) + gran;
    hipMemAccessDesc ad{};
    ad.location = prop.location;
    ad.flags = hipMemAccessFlagsProtReadWrite;
    if ((e = hipMemMap(base, r.map_bytes, 0, r.handle, 0)) != hipSuccess || (e = hipMemSetAccess(base, r.map_bytes, &ad, 1)) != hipSuccess) {
        (void)hipMemRelease(r.handle);
        (void)hipMemAddressFree(r.va, r.va_bytes);
        return e;
    }
    // mode 1: the buffer ENDS with the mapping, so its start is 16-byte aligned and no more (round-5 ADVICE: the comment here
    // claimed 256): every kernel is correct at 16 bytes -- the widest access is a dwordx4 -- and layouts that are tuned to
    // 128-byte lines merely straddle lines in this debugging mode.  Mode 2 (the buffer STARTS with the mapping) keeps the
    // allocator's natural alignment.
    const size_t span = (bytes + 255) & ~(size_t)255;
    void* p = guard_mode() == 2 ? base : base + (r.map_bytes - span) + (span - ((bytes + 15) & ~(size_t)15));
    {
        std::lock_guard<std::mutex> lk(g_guard_lock);
        g_guard_recs.emplace_back(p, r);
    }
    *out = p;
    return hipSuccess;
}

hipError_t dev_alloc(void** p, size_t bytes) { return guard_mode() ? guard_alloc(p, bytes) : hipMalloc(p, bytes); }

hipError_t dev_free(void* p)
{
    if (!p)
        return hipSuccess;
    if (!guard_mode())
        return hipFree(p);
    GuardRec r{};
    {
        std::lock_guard<std::mutex> lk(g_guard_lock);
        size_t i = 0;
        while (i < g_guard_recs.size() && g_guard_recs[i].first != p)
            i++;
        if (i == g_guard_recs.size())
            return hipFree(p);  // (not ours)
        r = g_guard_recs[i].second;
        g_guard_recs.erase(g_guard_recs.begin() + (ptrdiff_t)i);
    }
    (void)hipDeviceSynchronize();  // hipFree's implicit barrier
    hipError_t e = hipMemUnmap(static_cast<char*>(r.va) + r.gran, r.map_bytes);
    hipError_t e2 = hipMemRelease(r.handle);
    // (debugging mode only) The address range is NOT given back, so a long soak run under EFX_GUARD grows its address space
    // by every buffer it ever freed: a freed pointer then stays unmapped for the rest of the process (a use after free
    // faults too), and the runtime never sees an address twice -- one soak process of this round died in the HIP runtime's own
    // bookkeeping ("Memobj map does not have ptr") after some two thousand reserve / free cycles of recycled ranges.
    return e != hipSuccess ? e : e2;
}

template <typename T>
hipError_t dalloc(T** p, size_t n)
{
    return dev_alloc(reinterpret_cast<void**>(p), n * sizeof(T));
}

int sync_all(efx_ctx* ctx)
{
    EFX_HIP(hipStreamSynchronize(ctx->copy_stream));
    for (auto ps : ctx->parse_streams)
        EFX_HIP(hipStreamSynchronize(ps));
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->recon_groups_unsynced = 0;
    return EFX_OK;
}

size_t meta_bytes(size_t n) { return (n + 1) * sizeof(uint64_t) + 3 * n * sizeof(uint32_t); }

void bind_device(efx_ctx* c)
{
    if (c)
        (void)hipSetDevice(c->cfg.device);
}

}  // namespace

extern "C" {

const char* efx_status_string(int status)
{
    switch (status) {
    case EFX_OK: return "ok";
    case EFX_ERR_ARG: return "invalid argument";
    case EFX_ERR_DEVICE: return "HIP runtime error";
    case EFX_ERR_NO_DEVICE: return "no usable gfx950 device";
    case EFX_ERR_CAPACITY: return "context capacity exceeded";
    case EFX_ERR_STATE: return "call out of order";
    case EFX_ERR_STREAM: return "stream violates a decoder constraint";
    default: return "unknown status";
    }
}

const char* efx_last_error(const efx_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int efx_create(const efx_config* cfg, efx_ctx** out)
{
    if (!cfg || !out || cfg->max_streams <= 0 || cfg->max_pictures <= 0 || cfg->max_pictures > 255)
        return EFX_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
        return EFX_ERR_NO_DEVICE;
    efx_ctx* ctx = new efx_ctx;
    ctx->cfg = *cfg;
    if (ctx->cfg.ring_depth < 2)
        ctx->cfg.ring_depth = 2;
    if (ctx->cfg.max_stream_bytes == 0)
        ctx->cfg.max_stream_bytes = (size_t)16384 * cfg->max_pictures * cfg->max_streams;
    auto bail = [&](int code) {
        efx_destroy(ctx);
        return code;
    };
    if (hipSetDevice(cfg->device) != hipSuccess)
        return bail(EFX_ERR_NO_DEVICE);
    StreamSet pooled;
    if (!cfg->hip_stream && take_stream_set(cfg->device, &pooled)) {
        // the stream set of an earlier context on this device: same queues, same places
        ctx->stream = pooled.recon;
        ctx->own_stream = true;
        for (int i = 0; i < kParseStreams; i++)
            ctx->parse_streams[i] = pooled.parse[i];
        ctx->copy_stream = pooled.copy;
        ctx->pooled_streams = true;
        ctx->stream_serial = pooled.serial;
    } else if (cfg->hip_stream)
        ctx->stream = (hipStream_t)cfg->hip_stream;
    else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess)
            return bail(EFX_ERR_DEVICE);
        ctx->own_stream = true;
        ctx->pooled_streams = true;
        std::lock_guard<std::mutex> lk(g_pool_guard);
        ctx->stream_serial = ++g_set_serial;
    }
    if (!ctx->parse_streams[0]) {
        // The parse kernel is a few thousand long-running waves: give it the higher priority so its workgroups are
        // placed as soon as the reconstruction kernels of the previous call free a slot.
        // The runtime creates a stream's hardware queue at its first launch, and queues are dealt onto the
        // command processor's pipes in creation order: left to first use (reconstruction stream, first parse stream,
        // copy stream, and the second parse stream only at the second decode) the second parse stream ends up
        // taking turns with the reconstruction stream instead of running beside it -- 2.2 instead of 1.6 ms per step
        // (measured on the first context of a process, tools/exp/overlap_probe.py).  So every queue is instantiated
        // here, in this order, by an empty launch.
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess)
            return bail(EFX_ERR_DEVICE);
        for (auto& ps : ctx->parse_streams)
            if (hipStreamCreateWithPriority(&ps, hipStreamNonBlocking, hi) != hipSuccess)
                return bail(EFX_ERR_DEVICE);
        if (hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess)
            return bail(EFX_ERR_DEVICE);
        std::vector<hipStream_t> order = {ctx->stream};
        for (auto ps : ctx->parse_streams)
            order.push_back(ps);
        order.push_back(ctx->copy_stream);
        for (hipStream_t st : order) {
            hipLaunchKernelGGL(k_fill, dim3(1), dim3(64), 0, st, (uint32_t*)nullptr, 0u, (size_t)0);
            if (hipStreamSynchronize(st) != hipSuccess)
                return bail(EFX_ERR_DEVICE);
        }
    }
    const size_t n = (size_t)cfg->max_streams, P = (size_t)cfg->max_pictures, D = (size_t)ctx->cfg.ring_depth;
    ctx->es_cap = ctx->cfg.max_stream_bytes + n * (kEsTailBytes + 32) + kEsGuardBytes;
    ctx->es_cap = (ctx->es_cap + 255) & ~(size_t)255;
    if (ctx->es_cap * kCoefsPerEsByte >= 0xFFFFFFFFull)
        return bail(EFX_ERR_CAPACITY);  // coefficient indices are 32-bit
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) {
        if (e == hipSuccess)
            e = r;
    };
    A(dalloc(&ctx->d_tables, 1));
    A(dalloc(&ctx->d_tm_tables, 1));
    A(dalloc(&ctx->d_state, n));
    for (auto& u : ctx->up) {
        A(dalloc(&u.d_es, ctx->es_cap));
        A(dalloc(&u.d_stream_off, n + 1));
        A(dalloc(&u.d_stream_perm, n));
        A(hipHostMalloc(reinterpret_cast<void**>(&u.h_es), ctx->es_cap, hipHostMallocDefault));
        A(hipHostMalloc(reinterpret_cast<void**>(&u.h_meta), meta_bytes(n), hipHostMallocDefault));
        A(hipEventCreateWithFlags(&u.uploaded, hipEventDisableTiming));
        for (auto& ev : u.last_read)
            A(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (e == hipSuccess)
            A(hipMemset(u.d_es, 0, ctx->es_cap));
    }
    for (auto& sl : ctx->slot) {
        A(dalloc(&sl.d_pic_count, n));
        A(dalloc(&sl.d_status, n));
        A(dalloc(&sl.d_counters, kMaxGroups));
        A(dalloc(&sl.d_mbrecs, n * P * kMbCount));
        A(dalloc(&sl.d_raw, n * P * kMbCount));
        A(dalloc(&sl.d_coefs, ctx->es_cap * kCoefsPerEsByte));
        A(dalloc(&sl.d_pics, n * P));
        A(dalloc(&sl.d_slices_tmp, n * P * kMaxSlicesPerPicture));
        A(dalloc(&sl.d_qtab, n * P * 64));
        A(dalloc(&sl.d_slice_base, n * P + kMaxGroups));  // (one list per parse half, each with an end entry)
        A(dalloc(&sl.d_descs, n * P * kMaxSlicesPerPicture));
        A(dalloc(&sl.d_call_pos, 2 * n));
    }
    A(dalloc(&ctx->d_frames, n * D * kFrameBytes + 8192));  // slack: k_recon's window rows may over-read the last frame
    A(dalloc(&ctx->d_video[0], 1));
    A(dalloc(&ctx->d_video[1], 1));
    A(dalloc(&ctx->d_video_lines[0], 1));
    A(dalloc(&ctx->d_video_lines[1], 1));
    A(dalloc(&ctx->d_hash, n * D));
    A(dalloc(&ctx->d_sbc_tables, 1));
    A(dalloc(&ctx->d_sbc_enc_tables, 1));
    A(dalloc(&ctx->d_import_taps, kImportTapRows));
    A(dalloc(&ctx->d_import_pcm_table, ipcm::kTableLen));
    if (e != hipSuccess) {
        fprintf(stderr, "efx_create: %s\n", hipGetErrorString(e));
        return bail(EFX_ERR_DEVICE);
    }
    {
        // parse workgroups resident per parse kernel beside reconstruction launches: five for every eight compute units.
        // Measured on 256 CUs, 1024 streams x GOP 12 (tools/exp/cap_sweep2.py, profiles/r4_schedule_sweep.md): groups of 512
        // streams without a cap 8.05-8.18 M frames/s, capped at 128: 8.15-8.54; groups of 1024 capped at 128 ... 192:
        // 8.57-9.06 (flat between 144 and 192 on one box, best at 176 on another); 96 and below: the parse kernel
        // becomes the critical path.  5-slice pictures (4.4 x the tokens per slice): uncapped 7.21 M, 160: 7.55 M.
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) {
            ctx->parse_wg_cap = std::max(1, prop.multiProcessorCount * 5 / 8);
            ctx->n_cus = std::max(1, prop.multiProcessorCount);
        }
        if (const char* v = getenv("EFX_GROUPS"))
            ctx->opt_groups = atoi(v);
        if (const char* v = getenv("EFX_FORCE_PARSE_CAP"))
            ctx->opt_parse_cap = atoi(v);
        if (const char* cap = getenv("EFX_PARSE_WG_CAP"))  // (development: 0 = no cap)
            ctx->parse_wg_cap = atoi(cap);
    }
    ParseTables* pt = new ParseTables;
    build_parse_tables(pt);
    A(hipMemcpy(ctx->d_tables, pt, sizeof(ParseTables), hipMemcpyHostToDevice));
    {
        TmTables* tt = new TmTables;
        build_tm_tables(tt);
        hipError_t e_tm = hipMemcpy(ctx->d_tm_tables, tt, sizeof(TmTables), hipMemcpyHostToDevice);
        delete tt;
        A(e_tm);
    }
    delete pt;
    for (int ntsc = 0; ntsc < 2; ntsc++) {
        VideoTables vt;
        build_video_tables(ntsc, &vt);
        A(hipMemcpy(ctx->d_video[ntsc], &vt, sizeof(vt), hipMemcpyHostToDevice));
        VideoLineTemplates* lt = new VideoLineTemplates;
        build_video_line_templates(&vt, lt);
        A(hipMemcpy(ctx->d_video_lines[ntsc], lt, sizeof(*lt), hipMemcpyHostToDevice));
        delete lt;
    }
    {
        SbcTables st;
        build_sbc_tables(&st);
        A(hipMemcpy(ctx->d_sbc_tables, &st, sizeof(st), hipMemcpyHostToDevice));
        sbcenc::Tables et;
        sbcenc::build_tables(&et);
        A(hipMemcpy(ctx->d_sbc_enc_tables, &et, sizeof(et), hipMemcpyHostToDevice));
    }
    {
        std::vector<int32_t> pt(ipcm::kTableLen);
        build_import_pcm_table(pt.data());
        A(hipMemcpy(ctx->d_import_pcm_table, pt.data(), pt.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    A(hipMemset(ctx->d_frames, 0, n * D * kFrameBytes));
    for (auto& sl : ctx->slot) {
        A(hipMemset(sl.d_mbrecs, 0, n * P * kMbCount * sizeof(MbRec)));
        A(hipEventCreateWithFlags(&sl.parse_done, hipEventDisableTiming));
        A(hipEventCreateWithFlags(&sl.recon_done, hipEventDisableTiming));
    }
    if (e != hipSuccess)
        return bail(EFX_ERR_DEVICE);
    *out = ctx;
    if (efx_reset(ctx) != EFX_OK || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        *out = nullptr;
        return bail(EFX_ERR_DEVICE);
    }
    return EFX_OK;
}

void efx_destroy(efx_ctx* ctx)
{
    bind_device(ctx);
    if (!ctx)
        return;
    if (ctx->copy_stream)
        (void)hipStreamSynchronize(ctx->copy_stream);
    for (auto ps : ctx->parse_streams)
        if (ps)
            (void)hipStreamSynchronize(ps);
    if (ctx->stream)
        (void)hipStreamSynchronize(ctx->stream);
    for (auto& a : ctx->arenas) {
        if (a.owned)
            (void)hipHostFree(a.base);
        else
            (void)hipHostUnregister(a.base);
    }
    void* bufs[] = {ctx->d_tables, ctx->d_tm_tables, ctx->d_sbc_flags, ctx->d_sbc_next, ctx->d_sbc_info, ctx->d_sbc_plan, ctx->d_sbc_extra, ctx->d_sbc_cover, ctx->d_state, ctx->d_frames, ctx->d_video[0],  ctx->d_video[1], ctx->d_video_lines[0],
                    ctx->d_video_lines[1], ctx->d_hash, ctx->d_ts, ctx->d_demux_chunks, ctx->d_sbc_tables, ctx->d_idx_info, ctx->d_ts_off, ctx->d_idx_len,
                    ctx->d_idx_base, ctx->d_idx_seq, ctx->d_enc_state, ctx->d_enc_pics, ctx->d_enc_slices, ctx->d_enc_slice_len,
                    ctx->d_enc_act, ctx->d_enc_cut_pics, ctx->d_enc_cut_sums, ctx->d_enc_info, ctx->d_enc_tables, ctx->d_sbc_enc_tables, ctx->d_mux_before, ctx->d_import_taps, ctx->d_import_pcm_table,
                    ctx->d_crop_sums, ctx->d_enc_aq_act, ctx->d_enc_aq_sums, ctx->d_enc_aq_map};
    if (ctx->h_enc_full)
        (void)hipHostFree(ctx->h_enc_full);
    for (auto& te : ctx->timing_ring)
        for (auto& ev : te.ev)
            if (ev)
                (void)hipEventDestroy(ev);
    for (void* b : bufs)
        if (b)
            (void)dev_free(b);
    for (auto& c : ctx->import_hdr_copies)
        (void)dev_free(c->device);
    for (auto& u : ctx->up) {
        void* ub[] = {u.d_es, u.d_stream_off, u.d_stream_perm, u.d_ts_len, u.d_pkt_base, u.d_es_len, u.d_pes_count, u.d_pes};
        for (void* b : ub)
            if (b)
                (void)dev_free(b);
        if (u.h_es)
            (void)hipHostFree(u.h_es);
        if (u.h_meta)
            (void)hipHostFree(u.h_meta);
        hipEvent_t evs[] = {u.uploaded, u.ev_demux[0], u.ev_demux[1]};
        for (auto ev : evs)
            if (ev)
                (void)hipEventDestroy(ev);
        for (auto ev : u.last_read)
            if (ev)
                (void)hipEventDestroy(ev);
    }
    for (auto& sl : ctx->slot) {
        void* sb[] = {sl.d_pic_count, sl.d_status, sl.d_counters, sl.d_mbrecs, sl.d_raw, sl.d_coefs, sl.d_pts, sl.d_call_pos,
                      sl.d_pics,      sl.d_slices_tmp, sl.d_qtab, sl.d_slice_base, sl.d_descs};
        for (void* b : sb)
            if (b)
                (void)dev_free(b);
        if (sl.parse_done)
            (void)hipEventDestroy(sl.parse_done);
        if (sl.recon_done)
            (void)hipEventDestroy(sl.recon_done);
    }
    bool complete = ctx->own_stream && ctx->stream && ctx->copy_stream;
    for (auto ps : ctx->parse_streams)
        complete = complete && ps;
    if (ctx->pooled_streams && complete) {  // (all of them idle: synchronised above)
        StreamSet set;
        set.recon = ctx->stream;
        for (int i = 0; i < kParseStreams; i++)
            set.parse[i] = ctx->parse_streams[i];
        set.copy = ctx->copy_stream;
        set.serial = ctx->stream_serial;
        park_stream_set(ctx->cfg.device, set);
    } else {
        for (auto ps : ctx->parse_streams)
            if (ps)
                (void)hipStreamDestroy(ps);
        if (ctx->copy_stream)
            (void)hipStreamDestroy(ctx->copy_stream);
        if (ctx->own_stream && ctx->stream)
            (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}


// transport-stream buffers (first EFX_FORMAT_TS upload or first index call): the TS of stream i
// occupies the same region of d_ts that its elementary stream will occupy in d_es (an ES is never
// longer than its TS)
static int ensure_ts_buffers(efx_ctx* ctx)
{
    if (ctx->ts_ready)
        return EFX_OK;
    if (ctx->d_ts)
        return fail(ctx, EFX_ERR_DEVICE, "transport-stream buffers: an earlier allocation failed");
    const size_t n_max = (size_t)ctx->cfg.max_streams;
    ctx->pes_cap = ctx->es_cap / 188 + n_max;
    hipError_t e = dalloc(&ctx->d_ts, ctx->es_cap);
    if (e == hipSuccess)
        e = dev_alloc(reinterpret_cast<void**>(&ctx->d_demux_chunks), (ctx->pes_cap / kDemuxChunk + n_max + 2) * 16);
    for (auto& u : ctx->up) {
        if (e == hipSuccess) e = dalloc(&u.d_ts_len, n_max);
        if (e == hipSuccess) e = dalloc(&u.d_pkt_base, n_max);
        if (e == hipSuccess) e = dalloc(&u.d_es_len, n_max);
        if (e == hipSuccess) e = dalloc(&u.d_pes_count, n_max);
        if (e == hipSuccess) e = dalloc(&u.d_pes, ctx->pes_cap);
        for (auto& ev : u.ev_demux)
            if (e == hipSuccess) e = hipEventCreate(&ev);
    }
    if (e == hipSuccess) e = dalloc(&ctx->d_idx_info, n_max);
    if (e == hipSuccess) e = dalloc(&ctx->d_ts_off, n_max + 1);
    if (e == hipSuccess) e = dalloc(&ctx->d_idx_len, n_max);
    if (e == hipSuccess) e = dalloc(&ctx->d_idx_base, n_max);
    if (e == hipSuccess) e = dalloc(&ctx->d_idx_seq, ctx->pes_cap);
    for (auto& sl : ctx->slot)
        if (e == hipSuccess) e = dalloc(&sl.d_pts, n_max * (size_t)ctx->cfg.max_pictures + n_max);
    if (e != hipSuccess)
        return fail(ctx, EFX_ERR_DEVICE, "transport-stream buffers", e);
    ctx->ts_ready = true;
    return EFX_OK;
}

// efx_upload_streams (in_place = false: the caller's bytes are only ever READ, whatever the pointers look like) and
// efx_upload_streams_inplace (the batch lies in an arena in the device layout; the library writes the tails and the zero fill
// into the gaps of the layout and the transfer reads the arena)
static int upload_streams(efx_ctx* ctx, int n_streams, const uint8_t* const* data, const size_t* len, int format, bool in_place)
{
    bind_device(ctx);
    if (!ctx || !data || !len || n_streams <= 0 || (format != EFX_FORMAT_ES && format != EFX_FORMAT_TS))
        return fail(ctx, EFX_ERR_ARG, "efx_upload_streams: bad argument");
    if (n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_CAPACITY, "efx_upload_streams: more streams than max_streams");
    const bool is_ts = format == EFX_FORMAT_TS;
    if (is_ts) {
        int r = ensure_ts_buffers(ctx);
        if (r)
            return r;
    }
    static const uint8_t tail[kEsTailBytes] = {0, 0, 0, 1, 0xB7, 0, 0, 1, 0xB7};
    // offsets and lengths are built in locals and moved into the batch only when the call can no longer be
    // rejected: a refused upload leaves the resident batch (and what efx_download_es reads) untouched
    std::vector<uint64_t> stream_off((size_t)n_streams + 1, 0);
    std::vector<uint32_t> es_len((size_t)n_streams, 0);
    size_t pos = 0, packets = 0;
    for (int i = 0; i < n_streams; i++) {
        const size_t n = len[i];
        if (!data[i] && n)
            return fail(ctx, EFX_ERR_ARG, "efx_upload_streams: null stream");
        const size_t padded = (n + kEsTailBytes + 15) & ~(size_t)15;
        if (pos + padded + kEsGuardBytes > ctx->es_cap)
            return fail(ctx, EFX_ERR_CAPACITY, "efx_upload_streams: more bytes than max_stream_bytes");
        stream_off[i] = pos;
        es_len[i] = (uint32_t)n;
        packets += n / 188;
        pos += padded;
    }
    stream_off[n_streams] = pos;
    if (is_ts && packets > ctx->pes_cap)
        return fail(ctx, EFX_ERR_CAPACITY, "efx_upload_streams: PES list capacity");

    // the buffer the last decode does not read; its previous content may still be in use by an older parse
    // half (two calls back) and its staging memory by its own H2D transfer
    const int ui = (ctx->cur_up + 1) % kUploads;
    efx_ctx::Upload& u = ctx->up[ui];
    hipStream_t st = ctx->copy_stream;
    // in place (asked for by name, round-5 ADVICE: never inferred from what the pointers look like -- a caller that packs
    // streams back to back in page-locked memory and uploads them one at a time would have had the next stream's first bytes
    // overwritten by this stream's tail): the batch must lie in one arena exactly as the device buffer holds it
    // (efx_stream_layout), else the call is refused
    const uint8_t* arena_src = nullptr;
    if (in_place) {
        for (const auto& a : ctx->arenas)
            if (data[0] >= a.base && data[0] + pos <= a.base + a.bytes) {
                arena_src = data[0];
                for (int i = 1; i < n_streams && arena_src; i++)
                    if (data[i] != data[0] + stream_off[i])
                        arena_src = nullptr;
                break;
            }
        if (!arena_src)
            return fail(ctx, EFX_ERR_ARG, "efx_upload_streams_inplace: the batch does not lie in an arena of this context in the layout of efx_stream_layout");
    }
    if (u.valid) {
        // this record's pinned metadata (and, staged path, its staging buffer) are about to be rewritten by the host: its own
        // previous transfer must have read them -- three uploads ago, long done
        EFX_HIP(hipEventSynchronize(u.uploaded));
        // ... and the device buffer is free once the parse halves that read its previous batch are through (three uploads ago:
        // long done; letting the copy stream wait instead of the host was measured and is slower, 6.9 against 8.0 M frames/s)
        for (auto ev : u.last_read)
            EFX_HIP(hipEventSynchronize(ev));
    }
    u.valid = false;
    uint8_t* d_dst = is_ts ? ctx->d_ts : u.d_es;
    // small per-stream arrays, pinned: stream_off | perm | ts_len | pkt_base
    uint64_t* m_off = reinterpret_cast<uint64_t*>(u.h_meta);
    uint32_t* m_perm = reinterpret_cast<uint32_t*>(m_off + n_streams + 1);
    uint32_t *m_ts_len = m_perm + n_streams, *m_pkt_base = m_ts_len + n_streams;
    memcpy(m_off, stream_off.data(), ((size_t)n_streams + 1) * sizeof(uint64_t));
    {
        size_t pk = 0;
        for (int i = 0; i < n_streams; i++) {
            m_ts_len[i] = (uint32_t)len[i];
            m_pkt_base[i] = (uint32_t)pk;
            pk += len[i] / 188;
        }
    }
    // Stage into the pinned buffer and ship it: the streams are cut into groups, one host thread
    // copies each group, and a group's H2D transfer is queued as soon as its copy is done, so the
    // transfer of the first groups runs under the copies of the last.
    auto stage = [&](int i0, int i1) {
        for (int i = i0; i < i1; i++) {
            uint8_t* at = u.h_es + stream_off[i];
            const size_t n = len[i], padded = (size_t)(stream_off[i + 1] - stream_off[i]);
            if (n)
                memcpy(at, data[i], n);
            if (is_ts)  // raw packets; k_demux writes the ES, the end-of-data tail and the zero fill
                memset(at + n, 0, padded - n);
            else {
                memcpy(at + n, tail, kEsTailBytes);
                memset(at + n + kEsTailBytes, 0, padded - n - kEsTailBytes);
            }
        }
    };
    if (arena_src) {
        // the gaps of the layout are the library's: end-of-data tail (ES) and zero fill; then ONE transfer from caller memory
        uint8_t* w = const_cast<uint8_t*>(arena_src);
        for (int i = 0; i < n_streams; i++) {
            uint8_t* at = w + stream_off[i];
            const size_t n = len[i], padded = (size_t)(stream_off[i + 1] - stream_off[i]);
            if (is_ts)
                memset(at + n, 0, padded - n);
            else {
                memcpy(at + n, tail, kEsTailBytes);
                memset(at + n + kEsTailBytes, 0, padded - n - kEsTailBytes);
            }
        }
        if (pos)
            EFX_HIP(hipMemcpyAsync(d_dst, arena_src, pos, hipMemcpyHostToDevice, st));
    } else {
        unsigned hw = std::thread::hardware_concurrency();
        int groups = pos > ((size_t)4 << 20) ? (int)std::min<unsigned>(8u, std::max(1u, hw / 2)) : 1;
        groups = std::min(groups, n_streams);
        std::vector<std::thread> workers;
        std::vector<int> first((size_t)groups + 1);
        for (int g = 0; g <= groups; g++)
            first[g] = (int)((int64_t)n_streams * g / groups);
        int started = 0;  // groups 1 .. started have a worker; the rest are copied inline (no exception leaves the C-ABI)
        try {
            for (int g = 1; g < groups; g++) {
                workers.emplace_back(stage, first[g], first[g + 1]);
                started = g;
            }
        } catch (...) {
        }
        hipError_t e = hipSuccess;
        for (int g = 0; g < groups; g++) {
            if (g >= 1 && g <= started)
                workers[g - 1].join();
            else
                stage(first[g], first[g + 1]);
            const size_t a = stream_off[first[g]], b = stream_off[first[g + 1]];
            if (e == hipSuccess && b > a)
                e = hipMemcpyAsync(d_dst + a, u.h_es + a, b - a, hipMemcpyHostToDevice, st);
        }
        if (e != hipSuccess)
            return fail(ctx, EFX_ERR_DEVICE, "efx_upload_streams: H2D", e);
    }
    // slices of one picture index are dealt to the parse waves stream by stream: longest streams
    // first, so that a wave's 64 slices have similar bit rates (and the long waves start early)
    for (int i = 0; i < n_streams; i++)
        m_perm[i] = (uint32_t)i;
    {
        // (sorted inside every group of streams that efx_decode runs as a unit: the groups of an idle-GPU call, or the
        // pinned number of them; a call that runs as fewer, coarser groups is served by the same order)
        const int G = ctx->opt_groups > 0 ? std::min(std::min(ctx->opt_groups, kMaxGroups), std::max(1, n_streams / 8)) : group_count(n_streams);
        u.sort_groups = G;
        for (int g = 0; g < G; g++)
            std::stable_sort(m_perm + group_first(n_streams, G, g), m_perm + group_first(n_streams, G, g + 1),
                             [&](uint32_t a, uint32_t b) { return len[a] > len[b]; });
    }
    EFX_HIP(hipMemcpyAsync(u.d_stream_off, m_off, ((size_t)n_streams + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    EFX_HIP(hipMemcpyAsync(u.d_stream_perm, m_perm, (size_t)n_streams * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    u.ts_bytes = 0;
    u.demux_timed = false;
    if (is_ts) {
        EFX_HIP(hipMemsetAsync(ctx->d_ts + pos, 0, kEsGuardBytes, st));
        EFX_HIP(hipMemcpyAsync(u.d_ts_len, m_ts_len, n_streams * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        EFX_HIP(hipMemcpyAsync(u.d_pkt_base, m_pkt_base, n_streams * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        EFX_HIP(hipMemsetAsync(u.d_es + pos, 0, kEsGuardBytes, st));
        // MpegDecoder::more()/demux() for the whole batch (player.cpp:381-493)
        if (ctx->timing)
            EFX_HIP(hipEventRecord(u.ev_demux[0], st));
        {
            // chunk-parallel: per-chunk totals, the chain across a stream's chunks (and the end-of-data tail), the gather
            size_t max_len = 0;
            for (int i = 0; i < n_streams; i++)
                max_len = std::max(max_len, len[i]);
            const unsigned chunks = (unsigned)std::max<size_t>(1, (max_len / 188 + kDemuxChunk - 1) / kDemuxChunk);
            hipLaunchKernelGGL(k_demux_scan, dim3(chunks, n_streams), dim3(kDemuxThreads), 0, st, ctx->d_ts, u.d_stream_off, u.d_ts_len, u.d_pkt_base,
                               ctx->d_demux_chunks);
            hipLaunchKernelGGL(k_demux_offsets, dim3(n_streams), dim3(64), 0, st, u.d_ts_len, u.d_pkt_base, ctx->d_demux_chunks, u.d_es,
                               u.d_stream_off, u.d_es_len, u.d_pes_count);
            hipLaunchKernelGGL(k_demux, dim3(chunks, n_streams), dim3(kDemuxThreads), 0, st, ctx->d_ts, u.d_stream_off, u.d_ts_len, u.d_pkt_base,
                               ctx->d_demux_chunks, u.d_es, u.d_pes);
        }
        if (ctx->timing) {
            EFX_HIP(hipEventRecord(u.ev_demux[1], st));
            u.demux_timed = true;
        }
        EFX_HIP(hipGetLastError());
        for (int i = 0; i < n_streams; i++)
            u.ts_bytes += len[i];
    } else
        EFX_HIP(hipMemsetAsync(u.d_es + pos, 0, kEsGuardBytes, st));
    EFX_HIP(hipEventRecord(u.uploaded, st));
    // the batch is resident (as far as every later call on this context is concerned: they wait for the event)
    u.stream_off.swap(stream_off);
    u.es_len.swap(es_len);
    u.n_streams = n_streams;
    u.es_used = pos;
    u.ts_input = is_ts;
    u.valid = true;
    ctx->cur_up = ui;
    return EFX_OK;
}

int efx_upload_streams(efx_ctx* ctx, int n_streams, const uint8_t* const* data, const size_t* len, int format)
{
    return upload_streams(ctx, n_streams, data, len, format, false);
}

int efx_upload_streams_inplace(efx_ctx* ctx, int n_streams, uint8_t* const* data, const size_t* len, int format)
{
    return upload_streams(ctx, n_streams, data, len, format, true);
}


int efx_stream_layout(int n_streams, const size_t* len, size_t* offsets)
{
    if (n_streams <= 0 || !len || !offsets)
        return EFX_ERR_ARG;
    size_t pos = 0;
    for (int i = 0; i < n_streams; i++) {
        offsets[i] = pos;
        pos += (len[i] + kEsTailBytes + 15) & ~(size_t)15;  // (the rule efx_upload_streams places streams by)
    }
    offsets[n_streams] = pos;
    return EFX_OK;
}

int efx_host_alloc(efx_ctx* ctx, size_t bytes, void** host_ptr)
{
    bind_device(ctx);
    if (!ctx || !host_ptr || !bytes)
        return EFX_ERR_ARG;
    void* p = nullptr;
    EFX_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    ctx->arenas.push_back({static_cast<uint8_t*>(p), bytes, true});
    *host_ptr = p;
    return EFX_OK;
}

int efx_host_register(efx_ctx* ctx, void* host_ptr, size_t bytes)
{
    bind_device(ctx);
    if (!ctx || !host_ptr || !bytes)
        return EFX_ERR_ARG;
    EFX_HIP(hipHostRegister(host_ptr, bytes, hipHostRegisterDefault));
    ctx->arenas.push_back({static_cast<uint8_t*>(host_ptr), bytes, false});
    return EFX_OK;
}

static int drop_arena(efx_ctx* ctx, void* host_ptr, bool owned)
{
    bind_device(ctx);
    if (!ctx || !host_ptr)
        return EFX_ERR_ARG;
    for (size_t i = 0; i < ctx->arenas.size(); i++)
        if (ctx->arenas[i].base == host_ptr && ctx->arenas[i].owned == owned) {
            // a transfer may still be reading it
            if (ctx->copy_stream)
                EFX_HIP(hipStreamSynchronize(ctx->copy_stream));
            ctx->arenas.erase(ctx->arenas.begin() + (ptrdiff_t)i);
            if (owned)
                EFX_HIP(hipHostFree(host_ptr));
            else
                EFX_HIP(hipHostUnregister(host_ptr));
            return EFX_OK;
        }
    return fail(ctx, EFX_ERR_ARG, owned ? "efx_host_free: not an arena of this context" : "efx_host_unregister: not registered with this context");
}

int efx_host_free(efx_ctx* ctx, void* host_ptr) { return drop_arena(ctx, host_ptr, true); }
int efx_host_unregister(efx_ctx* ctx, void* host_ptr) { return drop_arena(ctx, host_ptr, false); }

int efx_upload_done(efx_ctx* ctx)
{
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    if (ctx->cur_up < 0)
        return 1;
    hipError_t e = hipEventQuery(ctx->up[ctx->cur_up].uploaded);
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        return 0;
    }
    return e == hipSuccess ? 1 : fail(ctx, EFX_ERR_DEVICE, "efx_upload_done", e);
}

int efx_set_option(efx_ctx* ctx, int option, int value)
{
    if (!ctx || value < 0)
        return EFX_ERR_ARG;
    switch (option) {
    case EFX_OPT_GROUPS:
        if (value > kMaxGroups)
            return EFX_ERR_ARG;
        ctx->opt_groups = value;
        return EFX_OK;
    case EFX_OPT_PARSE_CAP:
        if (value > 2)
            return EFX_ERR_ARG;
        ctx->opt_parse_cap = value;
        return EFX_OK;
    case EFX_OPT_SBC_SERIAL:
        ctx->opt_sbc_serial = value != 0;
        return EFX_OK;
    default:
        return EFX_ERR_ARG;
    }
}

int efx_get_option(efx_ctx* ctx, int option, int* value)
{
    bind_device(ctx);
    if (!ctx || !value)
        return EFX_ERR_ARG;
    switch (option) {
    case EFX_OPT_GROUPS: *value = ctx->opt_groups; return EFX_OK;
    case EFX_OPT_PARSE_CAP: *value = ctx->opt_parse_cap; return EFX_OK;
    case EFX_OPT_SBC_SERIAL: *value = ctx->opt_sbc_serial; return EFX_OK;
    default:
        return EFX_ERR_ARG;
    }
}

int efx_download_es(efx_ctx* ctx, int stream, uint8_t* dst, size_t cap, size_t* es_len)
{
    bind_device(ctx);
    if (!ctx || !es_len || ctx->cur_up < 0 || stream < 0 || stream >= ctx->up[ctx->cur_up].n_streams || (!dst && cap))
        return ctx && ctx->cur_up < 0 ? fail(ctx, EFX_ERR_STATE, "efx_download_es: no streams uploaded") : EFX_ERR_ARG;
    efx_ctx::Upload& u = ctx->up[ctx->cur_up];
    EFX_HIP(hipEventSynchronize(u.uploaded));
    size_t n;
    if (u.ts_input) {
        uint32_t v = 0;
        EFX_HIP(hipMemcpy(&v, u.d_es_len + stream, sizeof(v), hipMemcpyDeviceToHost));
        n = v;
    } else
        n = u.es_len[stream];
    *es_len = n;
    size_t c = n < cap ? n : cap;
    if (c)
        EFX_HIP(hipMemcpy(dst, u.d_es + u.stream_off[stream], c, hipMemcpyDeviceToHost));
    return EFX_OK;
}

int efx_reset(efx_ctx* ctx)
{
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    const size_t n = (size_t)ctx->cfg.max_streams;
    EFX_HIP(hipMemsetAsync(ctx->d_frames, 0, n * ctx->cfg.ring_depth * kFrameBytes, ctx->stream));
    // the constructor's state (player.cpp:354-361): frame index 1 (_reference = _fb[0], _current = _fb[1]), no PTS seen
    std::vector<StreamState> init(n);
    for (auto& st : init) {
        st.fb_index = 1;
        st.pts_seen = 0;
        st.pts_carry = -1;
    }
    EFX_HIP(hipMemcpyAsync(ctx->d_state, init.data(), n * sizeof(StreamState), hipMemcpyHostToDevice, ctx->stream));
    EFX_HIP(hipStreamSynchronize(ctx->stream));  // (pageable source)
    ctx->recon_groups_unsynced = 0;  // (the host knows the reconstruction stream idle)
    return EFX_OK;
}

int efx_play_reset(efx_ctx* ctx)
{
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    int r = sync_all(ctx);
    if (r)
        return r;
    const size_t n = (size_t)ctx->cfg.max_streams;
    std::vector<StreamState> st(n);
    EFX_HIP(hipMemcpy(st.data(), ctx->d_state, n * sizeof(StreamState), hipMemcpyDeviceToHost));
    for (auto& x : st)
        x.pts_seen = 0;  // _last_pts = -1; _fb_index and _pts survive (player.cpp:439-453)
    EFX_HIP(hipMemcpy(ctx->d_state, st.data(), n * sizeof(StreamState), hipMemcpyHostToDevice));
    return EFX_OK;
}

int efx_stream_state(efx_ctx* ctx, int stream, uint32_t* frame_index, int* pts_seen, int64_t* newest_pts)
{
    bind_device(ctx);
    if (!ctx || stream < 0 || stream >= ctx->cfg.max_streams)
        return EFX_ERR_ARG;
    int r = sync_all(ctx);
    if (r)
        return r;
    StreamState st;
    EFX_HIP(hipMemcpy(&st, ctx->d_state + stream, sizeof(st), hipMemcpyDeviceToHost));
    if (frame_index)
        *frame_index = st.fb_index;
    if (pts_seen)
        *pts_seen = (int)st.pts_seen;
    if (newest_pts)
        *newest_pts = st.pts_carry;
    return EFX_OK;
}

int efx_erase_frames(efx_ctx* ctx)
{
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    size_t bytes = (size_t)ctx->cfg.max_streams * ctx->cfg.ring_depth * kFrameBytes;
    EFX_HIP(hipMemsetAsync(ctx->d_frames, 0x30, bytes, ctx->stream));
    return EFX_OK;
}

int efx_decode_from(efx_ctx* ctx, int first_picture) { return efx_decode_range(ctx, first_picture, ctx ? ctx->cfg.max_pictures : 0); }

int efx_decode_range(efx_ctx* ctx, int first_picture, int n_pictures)
{
    bind_device(ctx);
    if (!ctx || first_picture < 0 || n_pictures < 1 || n_pictures > ctx->cfg.max_pictures)
        return EFX_ERR_ARG;
    if (ctx->cur_up < 0)
        return fail(ctx, EFX_ERR_STATE, "efx_decode: no streams uploaded");
    efx_ctx::Upload& u = ctx->up[ctx->cur_up];
    const int n_all = u.n_streams, P = ctx->cfg.max_pictures, D = ctx->cfg.ring_depth;
    // Back-to-back calls pipeline against each other -- the parse half of call n + 1 (and n + 2) runs beside the
    // reconstruction of call n -- and then ONE group per call is best whatever the batch (4096 streams, 12-slice pictures:
    // 9.3 M frames/s as one group, 9.15 M as four; 5-slice pictures 7.85 / 7.57 M; profiles/r4_schedule_sweep.md): fewer,
    // fatter reconstruction launches have fewer draining tails.  A call that finds the reconstruction stream idle (one call
    // at a time) has nothing to pipeline against but itself: it runs as groups of kGroupStreams streams, the parse half of
    // group g + 1 beside the reconstruction of group g.  Results do not depend on the split.
    const bool idle_at_call = ctx->recon_groups_unsynced == 0;  // (by the library's own count: efx_ctx::recon_groups_unsynced)
    // (efx_set_option pins the structure: the same call sequence then runs the same launches whatever the timing)
    const int G = ctx->opt_groups > 0 ? std::min(std::min(ctx->opt_groups, kMaxGroups), std::max(1, n_all / 8))
                                      : (idle_at_call ? group_count(n_all) : 1);
    {
        // The order of the slices inside a picture index (streams by descending length) was laid down at upload INSIDE the
        // groups of that moment; every group of this call must be a union of those -- else (EFX_OPT_GROUPS changed between
        // upload and decode) the order is laid down again for this call's groups, once, behind everything queued.
        bool nested = true;
        for (int g = 1; g < G && nested; g++) {
            bool found = false;
            for (int k = 0; k <= u.sort_groups && !found; k++)
                found = group_first(n_all, u.sort_groups, k) == group_first(n_all, G, g);
            nested = found;
        }
        if (!nested) {
            int r = sync_all(ctx);
            if (r)
                return r;
            std::vector<uint32_t> perm((size_t)n_all);
            for (int i = 0; i < n_all; i++)
                perm[i] = (uint32_t)i;
            auto len_of = [&](uint32_t i) { return u.stream_off[i + 1] - u.stream_off[i]; };  // (padded lengths: the same order up to ties)
            for (int g = 0; g < G; g++)
                std::stable_sort(perm.begin() + group_first(n_all, G, g), perm.begin() + group_first(n_all, G, g + 1),
                                 [&](uint32_t a, uint32_t b) { return len_of(a) > len_of(b); });
            EFX_HIP(hipMemcpy(u.d_stream_perm, perm.data(), perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            u.sort_groups = G;
        }
    }
    hipStream_t sr = ctx->stream;
    int timing_slot = -1;
    if (ctx->timing && !ctx->timing_ring.empty()) {
        timing_slot = (int)(ctx->timed_calls++ % kTimingRing);
        ctx->timing_groups[timing_slot] = (uint8_t)G;
        ctx->timing_launches[timing_slot] = (uint16_t)(G * n_pictures);
    }
    ctx->last_upload = ctx->cur_up;
    ctx->last_n_streams = u.n_streams;
    ctx->last_ts_input = u.ts_input;
    // G groups of streams, each a parse half (a parse stream, into its own hand-over slot) and behind it the group's
    // reconstruction on the context stream
    ctx->n_groups = G;
    for (int g = 0; g < G; g++) {
        const int s0 = group_first(n_all, G, g), n = group_first(n_all, G, g + 1) - s0;
        const int slot = (int)(ctx->subcalls++ % kSlots);
        ctx->groups[g] = {slot, s0, n};
        efx_ctx::Slot& sl = ctx->slot[slot];
        sl.upload = ctx->cur_up;
        // macroblock records carry the epoch that wrote them; recycle the tag space by clearing
        const bool wrap = ++sl.epoch > 255;
        if (wrap)
            sl.epoch = 1;
        const int pi = (int)(ctx->parse_calls++ % kParseStreams);
        hipStream_t sp = ctx->parse_streams[pi];
        DecodeCounters* counters = sl.d_counters + g;
        uint32_t* slice_base = sl.d_slice_base + (size_t)s0 * P + g;               // this group's own lists
        SliceDesc* descs = sl.d_descs + (size_t)s0 * P * kMaxSlicesPerPicture;

        // ---- parse half (a parse stream): index -> slice list -> VLC parse -----------------------------------
        EFX_HIP(hipStreamWaitEvent(sp, u.uploaded, 0));     // the batch is in HBM (H2D and k_demux on the copy stream)
        EFX_HIP(hipStreamWaitEvent(sp, sl.recon_done, 0));  // the group kSlots back has released this slot
        // (the WHOLE slot: its stream ranges belong to other groups in other calls, and a record the current parse
        // does not write must never match a tag of the previous 255-cycle)
        if (wrap)
            EFX_HIP(hipMemsetAsync(sl.d_mbrecs, 0, (size_t)ctx->cfg.max_streams * P * kMbCount * sizeof(MbRec), sp));
        efx_ctx::TimingEvents* te = timing_slot >= 0 ? &ctx->timing_ring[(size_t)timing_slot * kMaxGroups + g] : nullptr;
        if (te && !te->ev[0])
            for (auto& ev : te->ev)
                EFX_HIP(hipEventCreate(&ev));
        if (te)
            EFX_HIP(hipEventRecord(te->ev[0], sp));
        hipLaunchKernelGGL(k_index, dim3(n), dim3(64 * kIndexWaves), 0, sp, u.d_es, u.d_stream_off, P, sl.d_pics, sl.d_slices_tmp,
                           sl.d_pic_count, sl.d_status, sl.d_qtab, ctx->d_tables->scan, u.d_pes, u.d_pkt_base, u.d_pes_count,
                           u.ts_input ? sl.d_pts : nullptr, u.ts_input ? sl.d_pts + (size_t)ctx->cfg.max_streams * P : nullptr,
                           first_picture, s0, n_pictures);
        hipLaunchKernelGGL(k_slice_scan, dim3(1), dim3(1024), 0, sp, sl.d_pics, sl.d_pic_count, n, P, u.d_stream_perm + s0,
                           slice_base, counters);
        hipLaunchKernelGGL(k_slice_emit, dim3((n * P * kMaxSlicesPerPicture + 255) / 256), dim3(256), 0, sp, sl.d_pics,
                           sl.d_slices_tmp, sl.d_pic_count, u.d_stream_off, slice_base, n, P, u.d_stream_perm + s0, descs, sl.d_status);
        if (te)
            EFX_HIP(hipEventRecord(te->ev[1], sp));
        const int max_slices = n * P * kMaxSlicesPerPicture;
        const int parse_waves = (max_slices + kParseLanes - 1) / kParseLanes;  // (rounded UP: one lane per slice slot)
        // k_parse's waves pull groups of slices off a counter: the grid is how many of them are resident at a time (above)
        int parse_wgs = (parse_waves + kParseWaves - 1) / kParseWaves;
        // The cap protects the reconstruction launches the parser runs beside.  When the reconstruction stream has
        // nothing queued at this moment -- one call at a time, the first call after a synchronisation -- the parser
        // may have the chip: 0.84 instead of 1.38 ms per 1024 streams x 12 pictures.
        const bool recon_busy = ctx->opt_parse_cap == 1 || (ctx->opt_parse_cap == 0 && ctx->recon_groups_unsynced > 0);
        if (ctx->parse_wg_cap > 0 && recon_busy)
            parse_wgs = std::min(parse_wgs, ctx->parse_wg_cap);
        hipLaunchKernelGGL(k_parse, dim3(parse_wgs), dim3(64 * kParseWaves), 0, sp, u.d_es,
                           descs, counters, ctx->d_tm_tables, sl.d_mbrecs, sl.d_raw, sl.d_coefs, sl.d_status, P, sl.epoch);
        if (te)
            EFX_HIP(hipEventRecord(te->ev[2], sp));
        EFX_HIP(hipEventRecord(sl.parse_done, sp));
        EFX_HIP(hipEventRecord(u.last_read[pi], sp));  // the bitstream buffer is free for the upload after next

        // ---- reconstruction of the group (context stream): one launch per picture index --------------------------
        EFX_HIP(hipStreamWaitEvent(sr, sl.parse_done, 0));
        if (te)
            EFX_HIP(hipEventRecord(te->ev[4], sr));
        // ring positions of this call's pictures; the reconstruction stream orders the calls
        hipLaunchKernelGGL(k_advance, dim3((n + 255) / 256), dim3(256), 0, sr, ctx->d_state, sl.d_pic_count,
                           u.ts_input ? sl.d_pts : nullptr, u.ts_input ? sl.d_pts + (size_t)ctx->cfg.max_streams * P : nullptr, s0, n,
                           P, sl.d_call_pos);
        constexpr int kGroupsPerPicture = (kMbCount * 6 + 63) / 64;
        for (int p = 0; p < n_pictures; p++)
            hipLaunchKernelGGL(k_recon, dim3(n, kGroupsPerPicture), dim3(64), 0, sr, sl.d_mbrecs, sl.d_coefs, ctx->d_tables->scan,
                               sl.d_qtab, ctx->d_frames, P, D, p, sl.d_call_pos, sl.epoch, s0);
        if (te)
            EFX_HIP(hipEventRecord(te->ev[3], sr));
        EFX_HIP(hipEventRecord(sl.recon_done, sr));
        ctx->last_recon_done = sl.recon_done;
        ctx->recon_groups_unsynced++;
    }
    EFX_HIP(hipGetLastError());
    ctx->decoded = true;
    ctx->results_valid = false;
    return EFX_OK;
}

int efx_decode(efx_ctx* ctx) { return efx_decode_from(ctx, 0); }

int efx_sync(efx_ctx* ctx)
{
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    return sync_all(ctx);
}

static int fetch_results(efx_ctx* ctx)
{
    if (!ctx->decoded)
        return fail(ctx, EFX_ERR_STATE, "no decode has run");
    if (ctx->results_valid)
        return EFX_OK;
    int r = sync_all(ctx);
    if (r)
        return r;
    const bool ts_input = ctx->last_ts_input;
    ctx->n_streams = ctx->last_n_streams;
    const size_t P = (size_t)ctx->cfg.max_pictures;
    ctx->h_pic_count.resize(ctx->n_streams);
    ctx->h_status.resize(ctx->n_streams);
    ctx->h_call_pos.resize(2 * (size_t)ctx->n_streams);
    if (ts_input)
        ctx->h_pts.resize((size_t)ctx->n_streams * P);
    else
        ctx->h_pts.clear();
    ctx->h_counters = DecodeCounters{};
    // every group of the call left the results of ITS streams in its own hand-over slot
    for (int g = 0; g < ctx->n_groups; g++) {
        const efx_ctx::Group& gr = ctx->groups[g];
        const efx_ctx::Slot& sl = ctx->slot[gr.slot];
        const size_t f = (size_t)gr.first, c = (size_t)gr.count;
        if (!c)
            continue;
        EFX_HIP(hipMemcpy(ctx->h_pic_count.data() + f, sl.d_pic_count + f, c * sizeof(uint32_t), hipMemcpyDeviceToHost));
        EFX_HIP(hipMemcpy(ctx->h_status.data() + f, sl.d_status + f, c * sizeof(uint32_t), hipMemcpyDeviceToHost));
        EFX_HIP(hipMemcpy(ctx->h_call_pos.data() + 2 * f, sl.d_call_pos + 2 * f, 2 * c * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (ts_input)
            EFX_HIP(hipMemcpy(ctx->h_pts.data() + f * P, sl.d_pts + f * P, c * P * sizeof(int64_t), hipMemcpyDeviceToHost));
        DecodeCounters dc;
        EFX_HIP(hipMemcpy(&dc, sl.d_counters + g, sizeof(dc), hipMemcpyDeviceToHost));
        ctx->h_counters.total_slices += dc.total_slices;
        ctx->h_counters.coefficients += dc.coefficients;
        ctx->h_counters.macroblocks += dc.macroblocks;
    }
    ctx->results_valid = true;
    return EFX_OK;
}

int efx_picture_count(efx_ctx* ctx, int stream, int* n_pictures)
{
    bind_device(ctx);
    if (!ctx || !n_pictures || stream < 0)
        return EFX_ERR_ARG;
    int r = fetch_results(ctx);
    if (r)
        return r;
    if (stream >= ctx->n_streams)
        return EFX_ERR_ARG;
    *n_pictures = (int)ctx->h_pic_count[stream];
    return EFX_OK;
}

int efx_stream_status(efx_ctx* ctx, int stream, uint32_t* bits)
{
    bind_device(ctx);
    if (!ctx || !bits || stream < 0)
        return EFX_ERR_ARG;
    int r = fetch_results(ctx);
    if (r)
        return r;
    if (stream >= ctx->n_streams)
        return EFX_ERR_ARG;
    *bits = ctx->h_status[stream];
    return EFX_OK;
}

int efx_picture_pts(efx_ctx* ctx, int stream, int picture, int64_t* pts)
{
    bind_device(ctx);
    if (!ctx || !pts || stream < 0 || picture < 0)
        return EFX_ERR_ARG;
    int r = fetch_results(ctx);
    if (r)
        return r;
    if (stream >= ctx->n_streams)
        return EFX_ERR_ARG;
    if (ctx->h_pts.empty()) {
        *pts = picture;  // elementary-stream input carries no PTS: pictures are numbered
        return EFX_OK;
    }
    *pts = picture < (int)ctx->h_pic_count[stream] ? ctx->h_pts[(size_t)stream * ctx->cfg.max_pictures + picture] : -1;
    return EFX_OK;
}

int efx_stream_picture_slot(efx_ctx* ctx, int stream, int picture, int* slot)
{
    bind_device(ctx);
    if (!ctx || !slot || stream < 0 || picture < 0)
        return EFX_ERR_ARG;
    int r = fetch_results(ctx);
    if (r)
        return r;
    if (stream >= ctx->n_streams)
        return EFX_ERR_ARG;
    const int pos0 = ctx->h_call_pos[2 * (size_t)stream], f = ctx->h_call_pos[2 * (size_t)stream + 1];
    const uint32_t q = (uint32_t)pos0 + (uint32_t)(f < 0 ? picture + 1 : std::max(0, picture - f));
    *slot = (int)(q % (uint32_t)ctx->cfg.ring_depth);
    return EFX_OK;
}

int efx_picture_slot(efx_ctx* ctx, int picture)
{
    bind_device(ctx);
    int slot = 0;
    int r = efx_stream_picture_slot(ctx, 0, picture, &slot);
    return r ? r : slot;
}

int efx_frame_device_ptr(efx_ctx* ctx, int stream, int slot, void** dptr)
{
    bind_device(ctx);
    if (!ctx || !dptr || stream < 0 || stream >= ctx->cfg.max_streams || slot < 0 || slot >= ctx->cfg.ring_depth)
        return EFX_ERR_ARG;
    *dptr = ctx->d_frames + ((size_t)stream * ctx->cfg.ring_depth + slot) * kFrameBytes;
    return EFX_OK;
}

int efx_download_frame(efx_ctx* ctx, int stream, int slot, uint8_t* dst)
{
    bind_device(ctx);
    void* p;
    int r = efx_frame_device_ptr(ctx, stream, slot, &p);
    if (r || !dst)
        return r ? r : EFX_ERR_ARG;
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->recon_groups_unsynced = 0;  // (the host knows the reconstruction stream idle)
    EFX_HIP(hipMemcpy(dst, p, kFrameBytes, hipMemcpyDeviceToHost));
    return EFX_OK;
}

int efx_upload_frame(efx_ctx* ctx, int stream, int slot, const uint8_t* src)
{
    bind_device(ctx);
    void* p;
    int r = efx_frame_device_ptr(ctx, stream, slot, &p);
    if (r || !src)
        return r ? r : EFX_ERR_ARG;
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->recon_groups_unsynced = 0;  // (the host knows the reconstruction stream idle)
    EFX_HIP(hipMemcpy(p, src, kFrameBytes, hipMemcpyHostToDevice));
    return EFX_OK;
}

int efx_frame_hashes(efx_ctx* ctx, int first_stream, int n, uint64_t* out)
{
    bind_device(ctx);
    if (!ctx || !out || first_stream < 0 || n <= 0 || first_stream + n > ctx->cfg.max_streams)
        return EFX_ERR_ARG;
    const int D = ctx->cfg.ring_depth;
    const int frames = n * D;
    hipLaunchKernelGGL(k_frame_hash, dim3((frames + 63) / 64), dim3(64), 0, ctx->stream,
                       ctx->d_frames + (size_t)first_stream * D * kFrameBytes, frames, ctx->d_hash);
    EFX_HIP(hipGetLastError());
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->recon_groups_unsynced = 0;  // (the host knows the reconstruction stream idle)
    EFX_HIP(hipMemcpy(out, ctx->d_hash, (size_t)frames * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return EFX_OK;
}

int efx_video_get_params(int ntsc, efx_video_params* out)
{
    if (!out)
        return EFX_ERR_ARG;
    VideoTables vt;
    build_video_tables(ntsc ? 1 : 0, &vt);
    out->line_width = vt.line_width;
    out->line_count = vt.line_count;
    out->hsync = vt.hsync;
    out->hsync_long = vt.hsync_long;
    out->hsync_short = vt.hsync_short;
    out->burst_start = vt.burst_start;
    out->burst_width = vt.burst_width;
    out->active_start = vt.active_start;
    return EFX_OK;
}

int efx_composite_fields_ex(efx_ctx* ctx, const efx_field_opts* o, uint16_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !o || !dst_device || o->first_stream < 0 || o->n_streams <= 0 ||
        o->first_stream + o->n_streams > ctx->cfg.max_streams || o->slot < 0 || o->slot >= ctx->cfg.ring_depth)
        return EFX_ERR_ARG;
    if (o->hscroll && (o->other_slot < 0 || o->other_slot >= ctx->cfg.ring_depth || (o->hscroll & 7) ||
                       o->hscroll <= -EFX_FRAME_WIDTH || o->hscroll >= EFX_FRAME_WIDTH))
        return fail(ctx, EFX_ERR_ARG, "efx_composite_fields_ex: hscroll must be a multiple of 8 in (-352, 352)");
    if (o->overlay_blend < -1)
        return fail(ctx, EFX_ERR_ARG, "efx_composite_fields_ex: overlay_blend must be -1 or >= 0");
    FieldArgs a{};
    a.first_stream = o->first_stream;
    a.ring_depth = ctx->cfg.ring_depth;
    a.slot = o->slot;
    a.other_slot = o->hscroll ? o->other_slot : o->slot;
    a.frame_counter = o->frame_counter;
    a.hscroll = o->hscroll;
    a.overlay = o->overlay;
    a.overlay_stride = o->overlay_stride;
    // composite(), video.cpp:857-859
    int scale = 0;
    if (o->overlay_blend) {
        scale = 255 / 4;
        if (o->overlay_blend != -1 && o->overlay_blend < 32)
            scale = (scale * o->overlay_blend) >> 5;
    }
    a.overlay_scale = scale;
    a.overlay_progress = o->overlay_progress;
    const int lines = o->ntsc ? 262 : 312, groups = (o->ntsc ? 912 : 1136) / 8;  // (video_init / pal_init, video.cpp:554-630)
    const int blocks = o->n_streams * ((lines * groups + kCompositeItemsPerBlock - 1) / kCompositeItemsPerBlock);
    hipLaunchKernelGGL(k_composite, dim3(blocks), dim3(256), 0, ctx->stream, ctx->d_frames, ctx->d_video[o->ntsc ? 1 : 0],
                       ctx->d_video_lines[o->ntsc ? 1 : 0], a, dst_device);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

int efx_composite_fields(efx_ctx* ctx, int first_stream, int n_streams, int slot, int ntsc, int frame_counter,
                         uint16_t* dst_device)
{
    bind_device(ctx);
    efx_field_opts o{};
    o.first_stream = first_stream;
    o.n_streams = n_streams;
    o.slot = o.other_slot = slot;
    o.ntsc = ntsc;
    o.frame_counter = frame_counter;
    return efx_composite_fields_ex(ctx, &o, dst_device);
}

size_t efx_export_bytes(int format)
{
    switch (format) {
    case EFX_PIX_I420: return (size_t)kFrameBytes;  // 352 x 192 x 3 / 2: the same count as the strip layout
    case EFX_PIX_RGB24:
    case EFX_PIX_RGBP: return (size_t)3 * EFX_FRAME_WIDTH * EFX_FRAME_HEIGHT;
    default: return 0;
    }
}

int efx_export_frames(efx_ctx* ctx, const efx_export_opts* o, void* dst_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    const size_t image = efx_export_bytes(o->format);
    if (!dst_device || ((uintptr_t)dst_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_export_frames: dst_device must be a 16-byte aligned device pointer");
    if (!image)
        return fail(ctx, EFX_ERR_ARG, "efx_export_frames: unknown format");
    if (o->format != EFX_PIX_I420 && o->chroma != EFX_CHROMA_NEAREST && o->chroma != EFX_CHROMA_BILINEAR)
        return fail(ctx, EFX_ERR_ARG, "efx_export_frames: unknown chroma mode");
    const size_t stride = o->dst_stride ? o->dst_stride : image;
    if (stride < image || (stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_export_frames: dst_stride must be a multiple of 16 and hold an image");
    if (o->first_stream < 0 || o->n_streams <= 0 || o->first_stream > ctx->cfg.max_streams - o->n_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_export_frames: stream range outside max_streams");
    if (o->slot < -1 || o->slot >= ctx->cfg.ring_depth)
        return fail(ctx, EFX_ERR_ARG, "efx_export_frames: slot outside the ring");
    ExportArgs a{};
    a.first_stream = o->first_stream;
    a.ring_depth = ctx->cfg.ring_depth;
    a.slot = o->slot;
    a.full_range = o->full_range ? 1 : 0;
    a.dst = static_cast<uint8_t*>(dst_device);
    a.dst_stride = stride;
    if (o->slot < 0) {
        if (o->picture < 0 || o->picture >= ctx->cfg.max_pictures)
            return fail(ctx, EFX_ERR_ARG, "efx_export_frames: picture outside [0, max_pictures)");
        if (!ctx->decoded || ctx->n_groups < 1)
            return fail(ctx, EFX_ERR_STATE, "efx_export_frames: picture mode before any decode");
        if (o->first_stream + o->n_streams > ctx->last_n_streams)
            return fail(ctx, EFX_ERR_STATE, "efx_export_frames: stream range beyond the most recent decode's streams");
        // every reconstruction group of that call left its streams' ring positions in its own hand-over slot
        a.picture = o->picture;
        a.n_groups = ctx->n_groups;
        for (int g = 0; g < ctx->n_groups; g++) {
            a.group_first[g] = ctx->groups[g].first;
            a.call_pos[g] = ctx->slot[ctx->groups[g].slot].d_call_pos;
        }
    }
    const unsigned blocks = (unsigned)(((size_t)o->n_streams * kExportItemsPerPicture + kExportItemsPerBlock - 1) / kExportItemsPerBlock);
    const bool bilinear = o->chroma == EFX_CHROMA_BILINEAR;
    const uint8_t* frames = ctx->d_frames;
    if (o->format == EFX_PIX_I420)
        hipLaunchKernelGGL((k_export<EFX_PIX_I420, EFX_CHROMA_NEAREST>), dim3(blocks), dim3(256), 0, ctx->stream, frames, o->n_streams, a);
    else if (o->format == EFX_PIX_RGB24 && bilinear)
        hipLaunchKernelGGL((k_export<EFX_PIX_RGB24, EFX_CHROMA_BILINEAR>), dim3(blocks), dim3(256), 0, ctx->stream, frames, o->n_streams, a);
    else if (o->format == EFX_PIX_RGB24)
        hipLaunchKernelGGL((k_export<EFX_PIX_RGB24, EFX_CHROMA_NEAREST>), dim3(blocks), dim3(256), 0, ctx->stream, frames, o->n_streams, a);
    else if (bilinear)
        hipLaunchKernelGGL((k_export<EFX_PIX_RGBP, EFX_CHROMA_BILINEAR>), dim3(blocks), dim3(256), 0, ctx->stream, frames, o->n_streams, a);
    else
        hipLaunchKernelGGL((k_export<EFX_PIX_RGBP, EFX_CHROMA_NEAREST>), dim3(blocks), dim3(256), 0, ctx->stream, frames, o->n_streams, a);
    EFX_HIP(hipGetLastError());
    if (o->slot < 0) {
        // A hand-over slot is recycled by the decode kSlots groups later once its recon_done fires (efx_decode_range):
        // move the event of every slot whose call record the export reads behind the export.  The newest group's event
        // stays last_recon_done -- it now marks the export, which is queued after that group.
        for (int g = 0; g < ctx->n_groups; g++) {
            const efx_ctx::Group& gr = ctx->groups[g];
            if (gr.count > 0 && gr.first < o->first_stream + o->n_streams && gr.first + gr.count > o->first_stream)
                EFX_HIP(hipEventRecord(ctx->slot[gr.slot].recon_done, ctx->stream));
        }
        ctx->last_recon_done = ctx->slot[ctx->groups[ctx->n_groups - 1].slot].recon_done;
    }
    return EFX_OK;
}

size_t efx_import_src_bytes(int format, int width, int height)
{
    if (width < 2 || width > kImportMaxWidth || height < 2 || height > kImportMaxWidth)
        return 0;
    switch (format) {
    case EFX_PIX_I420: return ((width | height) & 1) ? 0 : (size_t)width * height * 3 / 2;
    case EFX_PIX_RGB24:
    case EFX_PIX_RGBP: return (size_t)width * height * 3;
    default: return 0;
    }
}

// The checks efx_import_frames and efx_import_surfaces share, `image` being the bytes of one source image: the pointers,
// n_images, the crop, the destination rectangle, the ratio and the strides, into the kernels' arguments
static int import_args(efx_ctx* ctx, const char* who, const efx_import_opts* o, size_t image, const void* src_device, uint8_t* dst_device,
                       ImportArgs* out)
{
    const std::string w = std::string(who) + ": ";
    if (!src_device || ((uintptr_t)src_device & 15) || !dst_device || ((uintptr_t)dst_device & 15))
        return fail(ctx, EFX_ERR_ARG, (w + "src_device and dst_device must be 16-byte aligned device pointers").c_str());
    if (!image)
        return fail(ctx, EFX_ERR_ARG, (w + "unknown format, or width / height outside 2 .. 4096 (I420: even)").c_str());
    if (o->n_images < 1 || o->n_images > (1 << 24))
        return fail(ctx, EFX_ERR_ARG, (w + "n_images outside 1 .. 2^24").c_str());
    ImportArgs a{};
    a.format = o->format;
    a.width = o->width;
    a.height = o->height;
    a.full_range = o->full_range ? 1 : 0;
    const int even = o->format == EFX_PIX_I420 ? 1 : 0;
    if (o->crop_w == 0) {
        a.crop_w = o->width;
        a.crop_h = o->height;
    } else {
        a.crop_x = o->crop_x, a.crop_y = o->crop_y, a.crop_w = o->crop_w, a.crop_h = o->crop_h;
        if (a.crop_x < 0 || a.crop_y < 0 || a.crop_w < 1 || a.crop_h < 1 || a.crop_x > o->width - a.crop_w ||
            a.crop_y > o->height - a.crop_h)
            return fail(ctx, EFX_ERR_ARG, (w + "crop outside the source picture").c_str());
        if (even && ((a.crop_x | a.crop_y | a.crop_w | a.crop_h) & 1))
            return fail(ctx, EFX_ERR_ARG, (w + "the crop of an I420 source must be even").c_str());
    }
    if (o->dst_w == 0) {
        a.dst_w = EFX_FRAME_WIDTH;
        a.dst_h = EFX_FRAME_HEIGHT;
    } else {
        a.dst_x = o->dst_x, a.dst_y = o->dst_y, a.dst_w = o->dst_w, a.dst_h = o->dst_h;
        if ((a.dst_x | a.dst_y | a.dst_w | a.dst_h) & 1)
            return fail(ctx, EFX_ERR_ARG, (w + "the destination rectangle must be even").c_str());
        if (a.dst_x < 0 || a.dst_y < 0 || a.dst_w < 16 || a.dst_h < 16 || a.dst_x > EFX_FRAME_WIDTH - a.dst_w ||
            a.dst_y > EFX_FRAME_HEIGHT - a.dst_h)
            return fail(ctx, EFX_ERR_ARG, (w + "destination rectangle below 16 x 16 or outside the 352 x 192 frame").c_str());
    }
    if (a.crop_w > ipx::kMaxRatio * a.dst_w || a.crop_h > ipx::kMaxRatio * a.dst_h)
        return fail(ctx, EFX_ERR_ARG, (w + "the crop is more than 32 times the destination rectangle").c_str());
    a.src_stride = o->src_stride ? o->src_stride : (image + 15) / 16 * 16;
    a.dst_stride = o->dst_stride ? o->dst_stride : (size_t)kFrameBytes;
    if (a.src_stride < image || (a.src_stride & 15))
        return fail(ctx, EFX_ERR_ARG, (w + "src_stride must be a multiple of 16 and hold an image").c_str());
    if (a.dst_stride < (size_t)kFrameBytes || (a.dst_stride & 15))
        return fail(ctx, EFX_ERR_ARG, (w + "dst_stride must be a multiple of 16 and hold an image").c_str());
    *out = a;
    return EFX_OK;
}

// The context's colour setting for a YCbCr source of `height` lines: true = a conversion, its coefficients in *k
static bool import_colour(const efx_ctx* ctx, int height, colour::Coefs* k)
{
    int32_t q[9];
    int y0;
    if (!ctx->import_colour_on || colour::coefs(ctx->import_colour.matrix, ctx->import_colour.full_range, height, q, &y0) != 1)
        return false;
    *k = colour::pack(q, y0);
    return true;
}

// The context's HDR setting for a YCbCr source of `height` lines: *tables = nullptr when it is off, else the device copy
// of the setting's tables -- made at the setting's first use: built on the host, uploaded once in stream order in front
// of the launch that reads it, kept until efx_destroy (queued calls keep theirs)
static int import_hdr(efx_ctx* ctx, int height, const hdr::Tables** tables)
{
    *tables = nullptr;
    if (!ctx->import_hdr_on)
        return EFX_OK;
    const efx_import_hdr& h = ctx->import_hdr;
    hdr::Coefs k{};
    if (!hdr::coefs(h.primaries, h.matrix, h.full_range, h.peak_nits, height, &k))
        return fail(ctx, EFX_ERR_ARG, "efx_import_set_hdr: no coefficients for this setting");  // (the setting was checked)
    for (const auto& c : ctx->import_hdr_copies)
        if (!std::memcmp(&c->host.k, &k, sizeof(k))) {
            *tables = c->device;
            return EFX_OK;
        }
    auto c = std::make_unique<efx_ctx::HdrCopy>();
    c->host.k = k;
    if (!build_import_hdr_tables(&c->host))
        return fail(ctx, EFX_ERR_ARG, "efx_import_set_hdr: the tables of this peak are not monotonic");
    EFX_HIP(dalloc(&c->device, 1));
    if (const hipError_t e = hipMemcpyAsync(c->device, &c->host, sizeof(hdr::Tables), hipMemcpyHostToDevice, ctx->stream); e != hipSuccess) {
        (void)dev_free(c->device);
        EFX_HIP(e);
    }
    *tables = c->device;
    ctx->import_hdr_copies.push_back(std::move(c));
    return EFX_OK;
}

int efx_import_set_hdr(efx_ctx* ctx, const efx_import_hdr* h)
{
    if (!ctx)
        return EFX_ERR_ARG;
    if (!h) {
        ctx->import_hdr_on = false;
        return EFX_OK;
    }
    if (!hdr::valid(h->transfer, h->primaries, h->matrix, h->full_range, h->peak_nits))
        return fail(ctx, EFX_ERR_ARG,
                    "efx_import_set_hdr: transfer must be 16 (PQ), primaries 9 or 1, matrix 1, 2, 4, 5, 6, 7 or 9 (H.273), full_range 0 or 1, "
                    "peak_nits 0 or 200 .. 10000");
    ctx->import_hdr = *h;
    ctx->import_hdr_on = true;
    return EFX_OK;
}

int efx_import_hdr_tables(const efx_import_hdr* h, int height, void* out, size_t cap)
{
    if (!h || !hdr::valid(h->transfer, h->primaries, h->matrix, h->full_range, h->peak_nits))
        return EFX_ERR_ARG;
    if (out && cap >= sizeof(hdr::Tables)) {
        auto t = std::make_unique<hdr::Tables>();
        if (!hdr::coefs(h->primaries, h->matrix, h->full_range, h->peak_nits, height, &t->k) || !build_import_hdr_tables(t.get()))
            return EFX_ERR_ARG;
        std::memcpy(out, t.get(), sizeof(hdr::Tables));
    }
    return (int)sizeof(hdr::Tables);
}

int efx_import_set_colour(efx_ctx* ctx, const efx_import_colour* c)
{
    if (!ctx)
        return EFX_ERR_ARG;
    if (!c) {
        ctx->import_colour_on = false;
        return EFX_OK;
    }
    if (!colour::valid(c->matrix, c->full_range))
        return fail(ctx, EFX_ERR_ARG, "efx_import_set_colour: matrix must be 1, 2, 4, 5, 6, 7 or 9 (H.273), full_range 0 or 1");
    ctx->import_colour = *c;
    ctx->import_colour_on = true;
    return EFX_OK;
}

int efx_import_colour_coefs(int matrix, int full_range, int height, int32_t q[9], int* y0)
{
    if (!q || !y0)
        return EFX_ERR_ARG;
    const int on = colour::coefs(matrix, full_range, height, q, y0);
    return on < 0 ? EFX_ERR_ARG : on;
}

int efx_import_frames(efx_ctx* ctx, const efx_import_opts* o, const void* src_device, uint8_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    ImportArgs a;
    if (const int rc = import_args(ctx, "efx_import_frames", o, efx_import_src_bytes(o->format, o->width, o->height), src_device, dst_device, &a))
        return rc;
    // two launches whatever n_images is; the table is written on the device, behind every earlier import's reads
    ImportSurfArgs sa{};
    colour::Coefs k;
    const hdr::Tables* ht = nullptr;
    if (o->format == EFX_PIX_I420)
        if (const int rc = import_hdr(ctx, o->height, &ht))
            return rc;
    if (ht) {
        // (as below: the planar surface of pitch = width)
        if (!spx::layout(EFX_KIND_I420, o->width, o->height, 0, 0, &sa.s))
            return fail(ctx, EFX_ERR_ARG, "efx_import_frames: no planar surface of this I420 size");
        sa.a = a;
        hipLaunchKernelGGL(k_import_taps, dim3((kImportTapRows + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_import_taps, a);
        hipLaunchKernelGGL(k_import_surf8p_h, dim3((unsigned)o->n_images * kImportBands), dim3(256), 0, ctx->stream,
                           static_cast<const uint8_t*>(src_device), dst_device, ctx->d_import_taps, sa, ht);
        EFX_HIP(hipGetLastError());
        return EFX_OK;
    }
    hipLaunchKernelGGL(k_import_taps, dim3((kImportTapRows + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_import_taps, a);
    if (o->format == EFX_PIX_I420 && import_colour(ctx, o->height, &k)) {
        // a packed I420 image is the planar surface of pitch = width (same bytes read, same output bit for bit): the
        // conversion runs in the surface kernel, and k_import stays the code it was
        if (!spx::layout(EFX_KIND_I420, o->width, o->height, 0, 0, &sa.s))
            return fail(ctx, EFX_ERR_ARG, "efx_import_frames: no planar surface of this I420 size");  // (import_args checked the size)
        sa.a = a;
        hipLaunchKernelGGL(k_import_surf8p_c, dim3((unsigned)o->n_images * kImportBands), dim3(256), 0, ctx->stream,
                           static_cast<const uint8_t*>(src_device), dst_device, ctx->d_import_taps, sa, k);
    } else {
        hipLaunchKernelGGL(k_import, dim3((unsigned)o->n_images * kImportBands), dim3(256), 0, ctx->stream,
                           static_cast<const uint8_t*>(src_device), dst_device, ctx->d_import_taps, a);
    }
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- surfaces (surface_px.h; k_import.hip, k_cropdetect.hip) ------------------------------------------------------------------------
size_t efx_surface_layout(int kind, int width, int height, size_t pitch, int plane_rows, efx_surface* out)
{
    return out ? spx::layout(kind, width, height, pitch, plane_rows, out) : 0;
}

// spx::check's verdict and the agreement of the opts with the surface as an error text; nullptr: the surface can be read
static const char* surface_fault(const efx_surface* s, int format, int width, int height)
{
    switch (spx::check(*s)) {
    case spx::kOk: break;
    case spx::kBadLayout: return "unknown surface layout";
    case spx::kBadShift: return "shift must be 1 .. 8 for a 16-bit layout and 0 for a byte layout";
    case spx::kBadSwap: return "swap_uv must be 0 or 1, and 0 for a planar layout";
    case spx::kBadSize: return "surface width / height must be even, 2 .. 4096";
    case spx::kOddWords: return "the offsets and pitches of a 16-bit layout must be even";
    case spx::kBadPitch: return "a pitch is below its plane's row bytes or above 2^20";
    case spx::kBadBytes: return "surface bytes must be below 2^40";
    default: return "a plane row ends beyond the surface's bytes";
    }
    if (format != EFX_PIX_I420 || width != s->width || height != s->height)
        return "opts->format must be EFX_PIX_I420, opts->width and height the surface's";
    return nullptr;
}

int efx_import_surfaces(efx_ctx* ctx, const efx_surface* s, const efx_import_opts* o, const void* src_device, uint8_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !s || !o)
        return EFX_ERR_ARG;
    if (const char* what = surface_fault(s, o->format, o->width, o->height))
        return fail(ctx, EFX_ERR_ARG, (std::string("efx_import_surfaces: ") + what).c_str());
    ImportSurfArgs a{};
    if (const int rc = import_args(ctx, "efx_import_surfaces", o, s->bytes, src_device, dst_device, &a.a))
        return rc;
    a.s = *s;
    // two launches, as efx_import_frames: the canonical image is I420, so its tap table is the call's
    auto* const k = s->layout == EFX_SURF_PLANAR8 ? k_import_surf8p : s->layout == EFX_SURF_SEMI8 ? k_import_surf8s
                    : s->layout == EFX_SURF_PLANAR16 ? k_import_surf16p : k_import_surf16s;
    const hdr::Tables* ht = nullptr;
    if (const int rc = import_hdr(ctx, s->height, &ht))
        return rc;
    hipLaunchKernelGGL(k_import_taps, dim3((kImportTapRows + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_import_taps, a.a);
    colour::Coefs kc;
    if (ht) {
        auto* const h = s->layout == EFX_SURF_PLANAR8 ? k_import_surf8p_h : s->layout == EFX_SURF_SEMI8 ? k_import_surf8s_h
                        : s->layout == EFX_SURF_PLANAR16 ? k_import_surf16p_h : k_import_surf16s_h;
        hipLaunchKernelGGL(h, dim3((unsigned)o->n_images * kImportBands), dim3(256), 0, ctx->stream, static_cast<const uint8_t*>(src_device),
                           dst_device, ctx->d_import_taps, a, ht);
    } else if (import_colour(ctx, s->height, &kc)) {
        auto* const c = s->layout == EFX_SURF_PLANAR8 ? k_import_surf8p_c : s->layout == EFX_SURF_SEMI8 ? k_import_surf8s_c
                        : s->layout == EFX_SURF_PLANAR16 ? k_import_surf16p_c : k_import_surf16s_c;
        hipLaunchKernelGGL(c, dim3((unsigned)o->n_images * kImportBands), dim3(256), 0, ctx->stream, static_cast<const uint8_t*>(src_device),
                           dst_device, ctx->d_import_taps, a, kc);
    } else {
        hipLaunchKernelGGL(k, dim3((unsigned)o->n_images * kImportBands), dim3(256), 0, ctx->stream, static_cast<const uint8_t*>(src_device),
                           dst_device, ctx->d_import_taps, a);
    }
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- interlaced sources (k_deint.hip) -----------------------------------------------------------------------------------------
int efx_deinterlace_count(int n_frames, int lead, int tail, int mode) { return dpx::count(n_frames, lead, tail, mode); }

int efx_deinterlace(efx_ctx* ctx, const efx_surface* s, const efx_deint_opts* o, const void* src_device, uint8_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !s || !o)
        return EFX_ERR_ARG;
    if (const char* what = surface_fault(s, EFX_PIX_I420, s->width, s->height))
        return fail(ctx, EFX_ERR_ARG, (std::string("efx_deinterlace: ") + what).c_str());
    if (!dpx::surface_ok(*s))
        return fail(ctx, EFX_ERR_ARG, "efx_deinterlace: the surface must be EFX_SURF_PLANAR8 or EFX_SURF_SEMI8, its height a multiple of 4 from 8");
    if (!src_device || ((uintptr_t)src_device & 15) || !dst_device || ((uintptr_t)dst_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_deinterlace: src_device and dst_device must be 16-byte aligned device pointers");
    if (o->first_field != EFX_FIELD_TOP && o->first_field != EFX_FIELD_BOTTOM)
        return fail(ctx, EFX_ERR_ARG, "efx_deinterlace: unknown first_field");
    const int n_out = dpx::count(o->n_frames, o->lead, o->tail, o->mode);
    if (n_out < 0)
        return fail(ctx, EFX_ERR_ARG, "efx_deinterlace: unknown mode, n_frames < 1, lead or tail not 0 / 1, or lead + tail >= n_frames");
    if (o->n_streams < 1 || (int64_t)o->n_streams * o->n_frames > INT32_MAX || (int64_t)o->n_streams * n_out > INT32_MAX)
        return fail(ctx, EFX_ERR_ARG, "efx_deinterlace: n_streams must be >= 1, the images in and the images out below 2^31");
    DeintArgs a{};
    a.src = static_cast<const uint8_t*>(src_device), a.dst = dst_device;
    const size_t image = (size_t)s->width * s->height * 3 / 2;
    a.src_stride = o->src_stride ? o->src_stride : (s->bytes + 15) / 16 * 16;
    a.dst_stride = o->dst_stride ? o->dst_stride : (image + 15) / 16 * 16;
    if (a.src_stride < s->bytes || (a.src_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_deinterlace: src_stride must be a multiple of 16 and hold an image");
    if (a.dst_stride < image || (a.dst_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_deinterlace: dst_stride must be a multiple of 16 and hold an image");
    a.s = *s;
    a.n_streams = o->n_streams, a.n_frames = o->n_frames;
    a.lead = o->lead, a.frames_out = o->n_frames - o->lead - o->tail;
    a.per_frame = o->mode == EFX_DEINT_FIELD ? 2 : 1;
    a.first_field = o->first_field;
    a.frame_items = dpx::frame_items(s->width, s->height);
    // one launch whatever the counts are (a workgroup takes further items when there are more than the grid's)
    const size_t items = (size_t)a.n_streams * a.frames_out * a.frame_items;
    const size_t wgs = (items + dpx::kWaves - 1) / dpx::kWaves;
    hipLaunchKernelGGL(k_deint, dim3((unsigned)std::min(wgs, (size_t)1 << 20)), dim3(64 * dpx::kWaves), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- telecined sources (k_telecine.hip) ---------------------------------------------------------------------------------------
int efx_detelecine_count(int n_frames, int lead) { return tpx::count(n_frames, lead); }

int efx_detelecine(efx_ctx* ctx, const efx_surface* s, const efx_detelecine_opts* o, const void* src_device, uint8_t* dst_device,
                   efx_telecine_info* info_device)
{
    bind_device(ctx);
    if (!ctx || !s || !o)
        return EFX_ERR_ARG;
    if (const char* what = surface_fault(s, EFX_PIX_I420, s->width, s->height))
        return fail(ctx, EFX_ERR_ARG, (std::string("efx_detelecine: ") + what).c_str());
    if (!dpx::surface_ok(*s))
        return fail(ctx, EFX_ERR_ARG, "efx_detelecine: the surface must be EFX_SURF_PLANAR8 or EFX_SURF_SEMI8, its height a multiple of 4 from 8");
    if (!src_device || ((uintptr_t)src_device & 15) || !dst_device || ((uintptr_t)dst_device & 15) || !info_device || ((uintptr_t)info_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_detelecine: src_device, dst_device and info_device must be 16-byte aligned device pointers");
    if (o->first_field != EFX_FIELD_TOP && o->first_field != EFX_FIELD_BOTTOM)
        return fail(ctx, EFX_ERR_ARG, "efx_detelecine: unknown first_field");
    if (o->nt < 0 || o->nt > 255)
        return fail(ctx, EFX_ERR_ARG, "efx_detelecine: nt must be 0 .. 255");
    const int n = tpx::processed(o->n_frames, o->lead);
    if (n < 0)
        return fail(ctx, EFX_ERR_ARG, "efx_detelecine: n_frames < 1, lead not 0 / 1, or lead >= n_frames");
    if (o->n_streams < 1 || (int64_t)o->n_streams * o->n_frames > INT32_MAX)
        return fail(ctx, EFX_ERR_ARG, "efx_detelecine: n_streams must be >= 1, the images in below 2^31");
    TelecineArgs a{};
    a.src = static_cast<const uint8_t*>(src_device), a.dst = dst_device, a.info = info_device;
    const size_t image = (size_t)s->width * s->height * 3 / 2;
    a.src_stride = o->src_stride ? o->src_stride : (s->bytes + 15) / 16 * 16;
    a.dst_stride = o->dst_stride ? o->dst_stride : (image + 15) / 16 * 16;
    if (a.src_stride < s->bytes || (a.src_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_detelecine: src_stride must be a multiple of 16 and hold an image");
    if (a.dst_stride < image || (a.dst_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_detelecine: dst_stride must be a multiple of 16 and hold an image");
    a.s = *s;
    a.n_streams = o->n_streams, a.n_frames = o->n_frames;
    a.lead = o->lead, a.n = n, a.n_out = tpx::count(o->n_frames, o->lead);
    a.first_field = o->first_field, a.nt = o->nt;
    a.measure_items = tpx::measure_items(s->width, s->height), a.weave_items = tpx::weave_items(*s);
    // three launches whatever the counts are (a workgroup takes further frames, cycles or items when there are more than
    // the grid's); the records carry everything from one to the next
    const size_t frames = (size_t)a.n_streams * a.n, cap = (size_t)1 << 20;
    hipLaunchKernelGGL(k_telecine_measure, dim3((unsigned)std::min(frames, cap)), dim3(64 * tpx::kMeasureWaves), 0, ctx->stream, a);
    const size_t cycles = (size_t)a.n_streams * ((a.n + tpx::kCycle - 1) / tpx::kCycle);
    hipLaunchKernelGGL(k_telecine_decide, dim3((unsigned)std::min((cycles + 255) / 256, cap)), dim3(256), 0, ctx->stream, a);
    const size_t wgs = (frames * a.weave_items + tpx::kWeaveWaves - 1) / tpx::kWeaveWaves;
    hipLaunchKernelGGL(k_telecine_weave, dim3((unsigned)std::min(wgs, cap)), dim3(64 * tpx::kWeaveWaves), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- scan type (k_scan.hip) ---------------------------------------------------------------------------------------------------
int efx_detect_scan(efx_ctx* ctx, const efx_surface* s, const efx_scan_opts* o, const void* src_device, efx_scan_frame* frames_device,
                    efx_scan_rec* recs_device)
{
    bind_device(ctx);
    if (!ctx || !s || !o)
        return EFX_ERR_ARG;
    if (const char* what = surface_fault(s, EFX_PIX_I420, s->width, s->height))
        return fail(ctx, EFX_ERR_ARG, (std::string("efx_detect_scan: ") + what).c_str());
    if (!dpx::surface_ok(*s))
        return fail(ctx, EFX_ERR_ARG, "efx_detect_scan: the surface must be EFX_SURF_PLANAR8 or EFX_SURF_SEMI8, its height a multiple of 4 from 8");
    if (!src_device || ((uintptr_t)src_device & 15) || !frames_device || ((uintptr_t)frames_device & 15) || !recs_device ||
        ((uintptr_t)recs_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_detect_scan: src_device, frames_device and recs_device must be 16-byte aligned device pointers");
    if (!scpx::options_ok(*o))
        return fail(ctx, EFX_ERR_ARG,
                    "efx_detect_scan: nt must be 0 .. 255, still 0 .. 4080, prog, intl and rep 256 .. 65535, accumulate 0 / 1");
    const int n = tpx::processed(o->n_frames, o->lead);
    if (n < 0)
        return fail(ctx, EFX_ERR_ARG, "efx_detect_scan: n_frames < 1, lead not 0 / 1, or lead >= n_frames");
    if (o->n_streams < 1 || (int64_t)o->n_streams * o->n_frames > INT32_MAX)
        return fail(ctx, EFX_ERR_ARG, "efx_detect_scan: n_streams must be >= 1, the images in below 2^31");
    ScanArgs a{};
    a.src = static_cast<const uint8_t*>(src_device), a.frames = frames_device, a.recs = recs_device;
    a.src_stride = o->src_stride ? (size_t)o->src_stride : (s->bytes + 15) / 16 * 16;
    if (a.src_stride < s->bytes || (a.src_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_detect_scan: src_stride must be a multiple of 16 and hold an image");
    a.s = *s;
    a.n_streams = o->n_streams, a.n_frames = o->n_frames;
    a.lead = o->lead, a.n = n;
    a.accumulate = o->accumulate, a.nt = o->nt;
    a.first_frame = o->first_frame;
    const scpx::Rule rule = scpx::rule_of(*o, s->width, s->height);
    a.still_wh = rule.still_wh, a.prog = rule.prog, a.intl = rule.intl, a.rep = rule.rep;
    a.measure_items = scpx::measure_items(s->width, s->height);
    // two launches whatever the counts are (a workgroup takes further frames or streams when there are more than the
    // grid's); the frame records carry everything from one to the next
    const size_t frames = (size_t)a.n_streams * a.n, cap = (size_t)1 << 20;
    hipLaunchKernelGGL(k_scan_measure, dim3((unsigned)std::min(frames, cap)), dim3(64 * scpx::kMeasureWaves), 0, ctx->stream, a);
    const size_t wgs = ((size_t)a.n_streams + scpx::kCountWaves - 1) / scpx::kCountWaves;
    hipLaunchKernelGGL(k_scan_count, dim3((unsigned)std::min(wgs, cap)), dim3(64 * scpx::kCountWaves), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

int efx_scan_verdict(const efx_scan_rec* rec, int* first_field) { return rec ? scpx::verdict(*rec, first_field) : EFX_ERR_ARG; }

// ---- noisy sources (k_denoise.hip) ----------------------------------------------------------------------------------------------
int efx_denoise(efx_ctx* ctx, const efx_surface* s, const efx_denoise_opts* o, const void* src_device, const uint8_t* prev_device,
                uint8_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !s || !o)
        return EFX_ERR_ARG;
    if (const char* what = surface_fault(s, EFX_PIX_I420, s->width, s->height))
        return fail(ctx, EFX_ERR_ARG, (std::string("efx_denoise: ") + what).c_str());
    if (!npx::surface_ok(*s))
        return fail(ctx, EFX_ERR_ARG, "efx_denoise: the surface must be EFX_SURF_PLANAR8 or EFX_SURF_SEMI8");
    if (!src_device || ((uintptr_t)src_device & 15) || !dst_device || ((uintptr_t)dst_device & 15) || ((uintptr_t)prev_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_denoise: src_device, dst_device and prev_device (when given) must be 16-byte aligned device pointers");
    if (!npx::threshold_ok(o->luma_spatial) || !npx::threshold_ok(o->chroma_spatial) || !npx::threshold_ok(o->luma_temporal) ||
        !npx::threshold_ok(o->chroma_temporal))
        return fail(ctx, EFX_ERR_ARG, "efx_denoise: every threshold must be 0 .. 64");
    if (o->n_streams < 1 || o->n_frames < 1 || (int64_t)o->n_streams * o->n_frames > INT32_MAX)
        return fail(ctx, EFX_ERR_ARG, "efx_denoise: n_streams and n_frames must be >= 1, the images below 2^31");
    DenoiseArgs a{};
    a.src = static_cast<const uint8_t*>(src_device), a.prev = prev_device, a.dst = dst_device;
    const size_t image = (size_t)s->width * s->height * 3 / 2;
    a.src_stride = o->src_stride ? (size_t)o->src_stride : (s->bytes + 15) / 16 * 16;
    a.dst_stride = o->dst_stride ? (size_t)o->dst_stride : (image + 15) / 16 * 16;
    a.prev_stride = (size_t)o->prev_stride;
    if (a.src_stride < s->bytes || (a.src_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_denoise: src_stride must be a multiple of 16 and hold an image");
    if (a.dst_stride < image || (a.dst_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_denoise: dst_stride must be a multiple of 16 and hold an image");
    if ((a.prev_stride & 15) || (prev_device && o->n_streams > 1 && a.prev_stride < image))
        return fail(ctx, EFX_ERR_ARG, "efx_denoise: prev_stride must be a multiple of 16 and, with prev_device and several streams, hold an image");
    a.s = *s;
    a.n_streams = o->n_streams, a.n_frames = o->n_frames;
    a.ts[0] = o->luma_spatial, a.ts[1] = o->chroma_spatial;
    a.tt[0] = o->luma_temporal, a.tt[1] = o->chroma_temporal;
    a.q[0] = npx::blend_q(a.tt[0]), a.q[1] = npx::blend_q(a.tt[1]);
    a.stream_items = npx::stream_items(s->width, s->height);
    // one launch whatever the counts are (a workgroup takes further items when there are more than the grid's)
    const size_t items = (size_t)a.n_streams * a.stream_items;
    const size_t wgs = (items + npx::kWaves - 1) / npx::kWaves;
    hipLaunchKernelGGL(k_denoise, dim3((unsigned)std::min(wgs, (size_t)1 << 20)), dim3(64 * npx::kWaves), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- subtitles and logos (k_overlay.hip) ----------------------------------------------------------------------------------------
int efx_overlay(efx_ctx* ctx, const efx_overlay_opts* o, const efx_overlay_event* events_device, const uint8_t* atlas_device,
                uint8_t* pictures_device, uint32_t* status_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    if (o->n_streams < 1 || o->n_pictures < 1 || o->n_events < 0 || o->n_events > EFX_OVERLAY_MAX_EVENTS || o->reserved != 0)
        return fail(ctx, EFX_ERR_ARG, "efx_overlay: n_streams and n_pictures must be >= 1, n_events 0 .. 4096, reserved 0");
    if ((int64_t)o->n_streams * o->n_pictures > INT32_MAX)
        return fail(ctx, EFX_ERR_ARG, "efx_overlay: the pictures must be below 2^31");
    if (o->first_picture < 0 || o->first_picture > ovx::kMaxIndex - o->n_pictures)
        return fail(ctx, EFX_ERR_ARG, "efx_overlay: first_picture must be >= 0 and first_picture + n_pictures at most 2^40");
    if (!pictures_device || ((uintptr_t)pictures_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_overlay: pictures_device must be a 16-byte aligned device pointer");
    if (o->n_events > 0 && (!events_device || !atlas_device))
        return fail(ctx, EFX_ERR_ARG, "efx_overlay: events_device and atlas_device must be given with n_events > 0");
    if (((uintptr_t)events_device & 7) || ((uintptr_t)status_device & 3))
        return fail(ctx, EFX_ERR_ARG, "efx_overlay: events_device must be 8-byte aligned, status_device (when given) 4-byte aligned");
    OverlayArgs a{};
    a.events = events_device, a.atlas = atlas_device, a.pictures = pictures_device, a.status = status_device;
    const uint64_t row = (uint64_t)o->n_pictures * ovx::kPicture;
    a.stride = o->stride ? (size_t)o->stride : (size_t)row;
    if (a.stride < row || (a.stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_overlay: stride must be a multiple of 16 and hold a stream's pictures");
    a.atlas_bytes = o->atlas_bytes, a.first_picture = o->first_picture;
    a.n_streams = o->n_streams, a.n_pictures = o->n_pictures, a.n_events = o->n_events;
    if (a.n_events == 0)
        return EFX_OK;  // nothing is shown: no launch
    // one launch whatever the counts are (a workgroup takes further pictures when there are more than the grid's)
    const size_t pictures = (size_t)a.n_streams * (size_t)a.n_pictures;
    hipLaunchKernelGGL(k_overlay, dim3((unsigned)std::min(pictures, (size_t)1 << 20)), dim3(ovx::kScanStep), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

int efx_overlay_check(const efx_overlay_event* events, int n_events, uint64_t atlas_bytes)
{
    for (int i = 0; events && i < n_events; i++)
        if (!ovx::valid(events[i], atlas_bytes))
            return i;
    return -1;
}

// ---- black borders (k_cropdetect.hip) -------------------------------------------------------------------------------------------
// The checks efx_detect_crop and efx_detect_crop_surfaces share, `image` being the bytes of one source image, into the
// kernels' arguments (the context's scratch for the sums when the caller gives none)
static int crop_args(efx_ctx* ctx, const char* who, const efx_crop_opts* o, size_t image, const void* src_device, efx_crop_rect* rects_device,
                     uint32_t* sums_device, CropArgs* out)
{
    const std::string w = std::string(who) + ": ";
    if (!src_device || ((uintptr_t)src_device & 15) || !rects_device || ((uintptr_t)rects_device & 15) || ((uintptr_t)sums_device & 15))
        return fail(ctx, EFX_ERR_ARG, (w + "src_device, rects_device and sums_device (when given) must be 16-byte aligned device pointers").c_str());
    if (!image)
        return fail(ctx, EFX_ERR_ARG, (w + "unknown format, or width / height outside 2 .. 4096 (I420: even)").c_str());
    if (o->n_streams < 1 || o->images_per_stream < 1 || (int64_t)o->n_streams * o->images_per_stream > INT32_MAX)
        return fail(ctx, EFX_ERR_ARG, (w + "n_streams and images_per_stream must be >= 1, their product below 2^31").c_str());
    if (o->limit < 0 || o->limit > 255)
        return fail(ctx, EFX_ERR_ARG, (w + "limit outside 0 .. 255").c_str());
    if (o->round < 2 || o->round > 64 || (o->round & 1))
        return fail(ctx, EFX_ERR_ARG, (w + "round must be even, 2 .. 64").c_str());
    CropArgs a{};
    a.src = static_cast<const uint8_t*>(src_device);
    a.rects = reinterpret_cast<int32_t*>(rects_device);
    a.n_streams = o->n_streams;
    a.images_per_stream = o->images_per_stream;
    a.n_images = o->n_streams * o->images_per_stream;
    a.format = o->format, a.width = o->width, a.height = o->height;
    a.full_range = o->full_range ? 1 : 0;
    a.limit = o->limit, a.round = o->round;
    a.src_stride = o->src_stride ? o->src_stride : (image + 15) / 16 * 16;
    a.sums_stride = o->sums_stride ? o->sums_stride : ((size_t)o->height + o->width + 3) / 4 * 4;
    if (a.src_stride < image || (a.src_stride & 15))
        return fail(ctx, EFX_ERR_ARG, (w + "src_stride must be a multiple of 16 and hold an image").c_str());
    if (a.sums_stride < (size_t)o->height + o->width || (a.sums_stride & 3))
        return fail(ctx, EFX_ERR_ARG, (w + "sums_stride must be a multiple of 4 and hold height + width sums").c_str());
    if (sums_device) {
        a.sums = sums_device;
    } else {
        const size_t need = (size_t)a.n_images * a.sums_stride;
        if (need > ctx->crop_sums_cap) {
            // (queued calls may still use the old block: this call waits for them)
            EFX_HIP(hipStreamSynchronize(ctx->stream));
            if (ctx->d_crop_sums)
                (void)dev_free(ctx->d_crop_sums);
            ctx->d_crop_sums = nullptr;
            ctx->crop_sums_cap = 0;
            EFX_HIP(dalloc(&ctx->d_crop_sums, need));
            ctx->crop_sums_cap = need;
        }
        a.sums = ctx->d_crop_sums;
    }
    *out = a;
    return EFX_OK;
}

// three launches whatever the counts are (a workgroup takes further items when there are more than the grid's)
constexpr size_t kCropGridCap = (size_t)1 << 20;
static unsigned crop_zero_wgs(const CropArgs& a) { return (unsigned)std::min(((size_t)a.n_images * a.width + 255) / 256, kCropGridCap); }
static unsigned crop_sum_wgs(const CropArgs& a)
{
    return (unsigned)std::min((size_t)a.n_images * ((a.height + cpx::kBandRows - 1) / cpx::kBandRows), kCropGridCap);
}
static unsigned crop_rect_wgs(const CropArgs& a) { return (unsigned)std::min((size_t)a.n_streams, kCropGridCap); }

int efx_detect_crop(efx_ctx* ctx, const efx_crop_opts* o, const void* src_device, efx_crop_rect* rects_device, uint32_t* sums_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    CropArgs a;
    if (const int rc = crop_args(ctx, "efx_detect_crop", o, efx_import_src_bytes(o->format, o->width, o->height), src_device, rects_device,
                                 sums_device, &a))
        return rc;
    hipLaunchKernelGGL(k_crop_zero, dim3(crop_zero_wgs(a)), dim3(256), 0, ctx->stream, a);
    auto* const k_sums = a.format == EFX_PIX_I420 ? k_crop_sums_i420 : a.format == EFX_PIX_RGB24 ? k_crop_sums_rgb24 : k_crop_sums_rgbp;
    hipLaunchKernelGGL(k_sums, dim3(crop_sum_wgs(a)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_crop_rects, dim3(crop_rect_wgs(a)), dim3(256), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

int efx_detect_crop_surfaces(efx_ctx* ctx, const efx_surface* s, const efx_crop_opts* o, const void* src_device, efx_crop_rect* rects_device,
                             uint32_t* sums_device)
{
    bind_device(ctx);
    if (!ctx || !s || !o)
        return EFX_ERR_ARG;
    if (const char* what = surface_fault(s, o->format, o->width, o->height))
        return fail(ctx, EFX_ERR_ARG, (std::string("efx_detect_crop_surfaces: ") + what).c_str());
    CropSurfArgs a{};
    if (const int rc = crop_args(ctx, "efx_detect_crop_surfaces", o, s->bytes, src_device, rects_device, sums_device, &a.c))
        return rc;
    a.y_offset = s->offset[0], a.y_pitch = s->pitch[0], a.shift = s->shift;
    hipLaunchKernelGGL(k_crop_zero, dim3(crop_zero_wgs(a.c)), dim3(256), 0, ctx->stream, a.c);
    hipLaunchKernelGGL(spx::is_words(s->layout) ? k_crop_sums_surf16 : k_crop_sums_surf8, dim3(crop_sum_wgs(a.c)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_crop_rects, dim3(crop_rect_wgs(a.c)), dim3(256), 0, ctx->stream, a.c);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- picture quality (k_quality.hip) ------------------------------------------------------------------------------------------------
double efx_compare_psnr(uint64_t sse, uint64_t samples)
{
    if (!samples)
        return NAN;
    if (!sse)
        return INFINITY;
    return 10.0 * std::log10(65025.0 * (double)samples / (double)sse);
}

double efx_compare_ssim(int64_t sum, int plane)
{
    const int64_t w = qpx::windows(plane);
    return w ? (double)sum / (65536.0 * (double)w) : NAN;
}

int efx_compare_pictures(efx_ctx* ctx, const efx_compare_opts* o, const uint8_t* ref_device, const uint8_t* test_device,
                         efx_compare_rec* recs_device, uint32_t* mb_sse_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    if (!ref_device || ((uintptr_t)ref_device & 15) || !test_device || ((uintptr_t)test_device & 15) || !recs_device ||
        ((uintptr_t)recs_device & 15) || ((uintptr_t)mb_sse_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_compare_pictures: ref_device, test_device, recs_device and mb_sse_device (when given) must be 16-byte aligned device pointers");
    if (o->n_images < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_compare_pictures: n_images must be >= 1");
    if (o->ref_max < 0 || o->ref_max > 255)
        return fail(ctx, EFX_ERR_ARG, "efx_compare_pictures: ref_max outside 0 .. 255");
    QualityArgs a{};
    a.ref = ref_device, a.test = test_device;
    a.recs = reinterpret_cast<uint64_t*>(recs_device);
    a.mb_sse = mb_sse_device;
    a.n_images = o->n_images;
    a.ref_max = o->ref_max ? o->ref_max : 255;
    a.ref_stride = o->ref_stride ? o->ref_stride : (size_t)qpx::kImageBytes;
    a.test_stride = o->test_stride ? o->test_stride : (size_t)qpx::kImageBytes;
    a.mb_stride = o->mb_stride ? o->mb_stride : (size_t)kMbCount;
    if (a.ref_stride < (size_t)qpx::kImageBytes || (a.ref_stride & 15) || a.test_stride < (size_t)qpx::kImageBytes || (a.test_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_compare_pictures: ref_stride and test_stride must be multiples of 16 and hold an image");
    if (a.mb_stride < (size_t)kMbCount || (a.mb_stride & 3))
        return fail(ctx, EFX_ERR_ARG, "efx_compare_pictures: mb_stride must be a multiple of 4 and hold 264 elements");
    // two launches whatever n_images is (a workgroup takes further items when there are more than the grid's)
    const size_t cap = (size_t)1 << 20;
    const size_t zero_wgs = ((size_t)a.n_images * 3 + 255) / 256;
    const size_t band_wgs = (size_t)a.n_images * qpx::kBands;
    hipLaunchKernelGGL(k_quality_zero, dim3((unsigned)std::min(zero_wgs, cap)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(a.ref_max < 255 ? k_quality_clamp : k_quality, dim3((unsigned)std::min(band_wgs, cap)), dim3(qpx::kThreads), 0,
                       ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- fast-forward and rewind picks (k_trick.hip) ----------------------------------------------------------------------------------
int64_t efx_trick_count(int64_t first_picture, int64_t n_pictures, int speed) { return tsel::count(first_picture, n_pictures, speed); }

int efx_trick_pick(efx_ctx* ctx, const efx_trick_opts* o, const uint8_t* src_device, uint8_t* fwd_device, uint8_t* rwd_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    const bool ring = o->source == EFX_TRICK_FROM_RING;
    if (o->source != EFX_TRICK_FROM_I420 && !ring)
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: unknown source");
    if (o->n_streams < 1 || o->n_pictures < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: n_streams and n_pictures must be >= 1");
    const int64_t picks = tsel::count(o->first_picture, o->n_pictures, o->speed);
    if (picks < 0)
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: speed outside 1 .. 255 or first_picture outside 0 .. 2^40 - 1");
    if ((uint64_t)o->n_streams * (uint64_t)picks > ((uint64_t)1 << 40))
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: more than 2^40 picked pictures in one call");
    if (!fwd_device && !rwd_device)
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: fwd_device and rwd_device are both NULL");
    if (ring ? src_device != nullptr : src_device == nullptr)
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: src_device must be given with the I420 source and NULL with the ring source");
    if (((uintptr_t)src_device | (uintptr_t)fwd_device | (uintptr_t)rwd_device) & 15)
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: src_device, fwd_device and rwd_device must be 16-byte aligned");
    if (!ring && (o->src_stride < (size_t)o->n_pictures * kFrameBytes || (o->src_stride & 15)))
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: src_stride must be a multiple of 16 and hold n_pictures pictures");
    if (fwd_device && (o->fwd_stride < (size_t)picks * kFrameBytes || (o->fwd_stride & 15)))
        return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: fwd_stride must be a multiple of 16 and hold the call's picks");
    int64_t K = 0;
    if (rwd_device) {
        if (o->total_pictures < o->first_picture + o->n_pictures)
            return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: total_pictures below first_picture + n_pictures");
        K = tsel::total_picks(o->total_pictures, o->speed);
        if (o->rwd_stride / kFrameBytes < (uint64_t)K || (o->rwd_stride & 15))
            return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: rwd_stride must be a multiple of 16 and hold the title's K picks");
    }
    TrickArgs a{};
    a.src = src_device;
    a.fwd = fwd_device;
    a.rwd = rwd_device;
    a.src_stride = o->src_stride;
    a.fwd_stride = o->fwd_stride;
    a.rwd_stride = o->rwd_stride;
    a.first_picture = o->first_picture;
    a.k0 = tsel::first_pick(o->first_picture, o->speed);
    a.K = K;
    a.n_streams = o->n_streams;
    a.n_picks = (int)picks;
    a.speed = o->speed;
    if (ring) {
        if (o->first_stream < 0 || o->n_pictures > ctx->cfg.max_pictures)
            return fail(ctx, EFX_ERR_ARG, "efx_trick_pick: first_stream below 0 or n_pictures above max_pictures");
        if (!ctx->decoded || ctx->n_groups < 1)
            return fail(ctx, EFX_ERR_STATE, "efx_trick_pick: ring source before any decode");
        if (o->first_stream > ctx->last_n_streams - o->n_streams)
            return fail(ctx, EFX_ERR_STATE, "efx_trick_pick: stream range beyond the most recent decode's streams");
        if (o->n_pictures >= ctx->cfg.ring_depth)
            return fail(ctx, EFX_ERR_STATE, "efx_trick_pick: n_pictures >= ring_depth: a picture of the call is already overwritten");
        a.src = ctx->d_frames;
        a.first_stream = o->first_stream;
        a.ring_depth = ctx->cfg.ring_depth;
        a.n_groups = ctx->n_groups;
        for (int g = 0; g < ctx->n_groups; g++) {
            a.group_first[g] = ctx->groups[g].first;
            a.call_pos[g] = ctx->slot[ctx->groups[g].slot].d_call_pos;
        }
    }
    if (picks == 0)
        return EFX_OK;  // nothing to move: no launch
    // one launch whatever the counts are (a workgroup takes further runs of items when there are more than the grid's)
    // (at most 2^40 picked pictures, checked above: fewer than 2^53 items)
    const uint64_t items = (uint64_t)o->n_streams * (uint64_t)picks * tsel::kPiecesPerPicture;
    const uint64_t runs = (items + kTrickItemsPerBlock - 1) / kTrickItemsPerBlock;
    const unsigned blocks = (unsigned)std::min<uint64_t>(runs, kTrickMaxBlocks);
    if (ring)
        hipLaunchKernelGGL((k_trick<EFX_TRICK_FROM_RING>), dim3(blocks), dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((k_trick<EFX_TRICK_FROM_I420>), dim3(blocks), dim3(256), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    if (ring) {
        // as efx_export_frames' picture mode: the hand-over slots whose call records the kernel reads are recycled only
        // behind it
        for (int g = 0; g < ctx->n_groups; g++) {
            const efx_ctx::Group& gr = ctx->groups[g];
            if (gr.count > 0 && gr.first < o->first_stream + o->n_streams && gr.first + gr.count > o->first_stream)
                EFX_HIP(hipEventRecord(ctx->slot[gr.slot].recon_done, ctx->stream));
        }
        ctx->last_recon_done = ctx->slot[ctx->groups[ctx->n_groups - 1].slot].recon_done;
    }
    return EFX_OK;
}

// ---- picture rates conformed (k_conform.hip) -------------------------------------------------------------------------------------
int64_t efx_conform_count(int in_num, int in_den, int out_code, int64_t first_picture, int64_t n_pictures)
{
    return csel::count(in_num, in_den, out_code, first_picture, n_pictures);
}

int64_t efx_conform_source(int in_num, int in_den, int out_code, int64_t n) { return csel::source_of(in_num, in_den, out_code, n); }

int efx_conform_rate(efx_ctx* ctx, const efx_conform_opts* o, const uint8_t* src_device, uint8_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    if (o->n_streams < 1 || o->n_pictures < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_conform_rate: n_streams and n_pictures must be >= 1");
    csel::Ratio r;
    if (!csel::ratio(o->in_num, o->in_den, o->out_code, &r))
        return fail(ctx, EFX_ERR_ARG, "efx_conform_rate: in_num / in_den below 1, out_code outside 1 .. 8, a reduced term of the ratio of 2^31 or "
                                      "more, or rates more than 64 : 1 apart");
    if (!csel::span_ok(r, o->first_picture, o->n_pictures))
        return fail(ctx, EFX_ERR_ARG, "efx_conform_rate: first_picture + n_pictures or the last output's index above 2^31 - 1");
    const int64_t n0 = csel::outputs(r, o->first_picture), n_out = csel::outputs(r, o->first_picture + o->n_pictures) - n0;
    if (n_out > INT32_MAX || (uint64_t)o->n_streams * (uint64_t)n_out > ((uint64_t)1 << 40))
        return fail(ctx, EFX_ERR_ARG, "efx_conform_rate: more than 2^40 output pictures in one call");
    if (!src_device || !dst_device || (((uintptr_t)src_device | (uintptr_t)dst_device) & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_conform_rate: src_device and dst_device must be 16-byte aligned device pointers");
    if (o->src_stride < (size_t)o->n_pictures * kFrameBytes || (o->src_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_conform_rate: src_stride must be a multiple of 16 and hold n_pictures pictures");
    if (o->dst_stride / kFrameBytes < (uint64_t)n_out || (o->dst_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_conform_rate: dst_stride must be a multiple of 16 and hold the call's outputs");
    if (n_out == 0)
        return EFX_OK;  // nothing to move: no launch
    ConformArgs a{};
    a.src = src_device;
    a.dst = dst_device;
    a.src_stride = o->src_stride;
    a.dst_stride = o->dst_stride;
    a.A = r.A;
    a.B = r.B;
    a.first_picture = o->first_picture;
    a.n0 = n0;
    a.n_streams = o->n_streams;
    a.n_out = (int)n_out;
    // one launch whatever the counts are (a workgroup takes further runs of items when there are more than the grid's)
    const uint64_t runs = tsel::run_count((uint64_t)o->n_streams * (uint64_t)n_out);
    hipLaunchKernelGGL(k_conform, dim3((unsigned)std::min<uint64_t>(runs, kTrickMaxBlocks)), dim3(256), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- the encoder's picture rate -----------------------------------------------------------------------------------------------------
int64_t efx_picture_pts_offset(int code, int64_t k)
{
    if (!enc::rate_code_ok(code) || k < 0 || k > ((int64_t)1 << 32))
        return -1;
    return enc::rate_pts_offset(code, k);
}

int efx_picture_rate_code(int64_t num, int64_t den) { return csel::rate_code(num, den); }

int efx_encode_set_picture_rate(efx_ctx* ctx, int code)
{
    if (!ctx)
        return EFX_ERR_ARG;
    if (!enc::rate_code_ok(code))
        return fail(ctx, EFX_ERR_ARG, "efx_encode_set_picture_rate: code outside 1 .. 8");
    ctx->enc_next_rate_code = code;
    return EFX_OK;
}

int efx_encode_set_scene_cut(efx_ctx* ctx, const efx_scene_cut* cut)
{
    if (!ctx)
        return EFX_ERR_ARG;
    if (!cut) {
        ctx->enc_next_cut = enc::CutParams{0, 1};
        return EFX_OK;
    }
    if (cut->threshold < 0 || cut->threshold > 256)
        return fail(ctx, EFX_ERR_ARG, "efx_encode_set_scene_cut: threshold outside 0 .. 256");
    if (cut->min_gop < 1 || cut->min_gop > 255)
        return fail(ctx, EFX_ERR_ARG, "efx_encode_set_scene_cut: min_gop outside 1 .. 255");
    ctx->enc_next_cut = enc::CutParams{cut->threshold, cut->min_gop};
    return EFX_OK;
}

int efx_encode_set_adaptive_quant(efx_ctx* ctx, const efx_adaptive_quant* aq)
{
    if (!ctx)
        return EFX_ERR_ARG;
    if (!aq) {
        ctx->enc_next_aq = enc::AqParams{0};
        return EFX_OK;
    }
    if (aq->strength < 0 || aq->strength > enc::kAqMaxStrength)
        return fail(ctx, EFX_ERR_ARG, "efx_encode_set_adaptive_quant: strength outside 0 .. 256");
    ctx->enc_next_aq = enc::AqParams{aq->strength};
    return EFX_OK;
}

int efx_encode_mb_quant(efx_ctx* ctx, int stream, int picture, uint8_t* out_host)
{
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    if (!ctx->enc_info_pictures)
        return fail(ctx, EFX_ERR_STATE, "efx_encode_mb_quant: no efx_encode yet");
    if (!ctx->enc_info_aq)
        return fail(ctx, EFX_ERR_STATE, "efx_encode_mb_quant: the latest efx_encode ran without adaptive quantisation");
    if (stream < 0 || stream >= ctx->enc_info_streams || picture < 0 || picture >= ctx->enc_info_pictures || !out_host)
        return fail(ctx, EFX_ERR_ARG, "efx_encode_mb_quant: stream or picture outside the latest call's, or out_host NULL");
    EFX_HIP(hipMemcpyAsync(out_host, ctx->d_enc_aq_map + ((size_t)stream * kEncInfoCap + picture) * enc::kAqMbs, enc::kAqMbs,
                           hipMemcpyDeviceToHost, ctx->stream));
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    return EFX_OK;
}

int efx_encode_picture_info(efx_ctx* ctx, int stream, efx_enc_picture_info* out_host, int cap)
{
    static_assert(sizeof(efx_enc_picture_info) == sizeof(EncPictureInfo), "efx_enc_picture_info layout");
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    if (!ctx->enc_info_pictures)
        return fail(ctx, EFX_ERR_STATE, "efx_encode_picture_info: no efx_encode yet");
    if (stream < 0 || stream >= ctx->enc_info_streams || cap < 0 || (cap > 0 && !out_host))
        return fail(ctx, EFX_ERR_ARG, "efx_encode_picture_info: stream outside the latest call's, cap negative or out_host NULL");
    const int n = std::min(cap, ctx->enc_info_pictures);
    if (n > 0)
        EFX_HIP(hipMemcpyAsync(out_host, ctx->d_enc_info + (size_t)stream * kEncInfoCap, (size_t)n * sizeof(EncPictureInfo),
                               hipMemcpyDeviceToHost, ctx->stream));
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    return ctx->enc_info_pictures;
}

size_t efx_encode_bound(int format, int n_pictures)
{
    if ((format != EFX_FORMAT_ES && format != EFX_FORMAT_TS) || n_pictures < 1 || n_pictures > 255)
        return 0;
    const size_t es = (size_t)enc::kHdrCap + (size_t)kMbH * enc::kSliceCap;  // headers + 12 worst-case slices
    const size_t pic = format == EFX_FORMAT_TS ? (size_t)enc::ts_packets((uint32_t)(es + enc::kPesHdrBytes)) * 188 : es;
    return (pic * (size_t)n_pictures + 15) / 16 * 16;
}

// efx_encode (rate == nullptr) and efx_encode_rc
static int encode_impl(efx_ctx* ctx, const efx_encode_opts* o, const efx_encode_rate* rate, const uint8_t* src_device,
                       uint8_t* dst_device, uint32_t* len_device, uint32_t* status_device, uint8_t* recon_device,
                       uint8_t* qscale_out_device)
{
    auto misaligned = [](const void* p) { return !p || ((uintptr_t)p & 15); };
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_encode: n_streams outside 1 .. max_streams");
    if (o->n_pictures < 1 || o->n_pictures > 255)
        return fail(ctx, EFX_ERR_ARG, "efx_encode: n_pictures outside 1 .. 255");
    if (o->format != EFX_FORMAT_ES && o->format != EFX_FORMAT_TS)
        return fail(ctx, EFX_ERR_ARG, "efx_encode: unknown format");
    if (o->qscale < 1 || o->qscale > 31)
        return fail(ctx, EFX_ERR_ARG, "efx_encode: qscale outside 1 .. 31");
    if (o->gop < 1 || o->gop > 255)
        return fail(ctx, EFX_ERR_ARG, "efx_encode: gop outside 1 .. 255");
    if (o->search < 0 || o->search > enc::kMaxSearch)
        return fail(ctx, EFX_ERR_ARG, "efx_encode: search outside 0 .. 15");
    if (o->cont != 0 && o->cont != 1)
        return fail(ctx, EFX_ERR_ARG, "efx_encode: cont must be 0 or 1");
    if (o->first_pts < 0 || o->first_pts >= (1ll << 33))
        return fail(ctx, EFX_ERR_ARG, "efx_encode: first_pts outside 0 .. 2^33-1");
    if (o->src_stride < (size_t)o->n_pictures * kFrameBytes || (o->src_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_encode: src_stride must be a multiple of 16 and hold n_pictures pictures");
    if (o->dst_stride & 15)
        return fail(ctx, EFX_ERR_ARG, "efx_encode: dst_stride must be a multiple of 16");
    if (misaligned(src_device) || misaligned(dst_device) || misaligned(len_device) || misaligned(status_device) ||
        (recon_device && ((uintptr_t)recon_device & 15)))
        return fail(ctx, EFX_ERR_ARG, "efx_encode: src, dst, len and status must be 16-byte aligned device pointers (recon too, unless NULL)");
    if (o->cont) {
        if (!ctx->enc_started)
            return fail(ctx, EFX_ERR_STATE, "efx_encode: cont without a previous efx_encode");
        if (o->n_streams != ctx->enc_n_streams || o->format != ctx->enc_format || o->gop != ctx->enc_gop)
            return fail(ctx, EFX_ERR_STATE, "efx_encode: cont with n_streams, format or gop other than the call that started the streams");
        if ((rate != nullptr) != ctx->enc_rc)
            return fail(ctx, EFX_ERR_STATE, "efx_encode: cont mixes efx_encode and efx_encode_rc: streams continue through the entry point that started them");
        if (rate && (rate->bitrate != ctx->enc_bitrate || rate->vbv_bits != ctx->enc_vbv_bits))
            return fail(ctx, EFX_ERR_STATE, "efx_encode_rc: cont with a bitrate or vbv_bits other than the call that started the streams");
        if (*(volatile uint32_t*)ctx->h_enc_full == ctx->enc_generation)
            return fail(ctx, EFX_ERR_STATE, "efx_encode: cont after a stream filled its output region");
    }
    if (!ctx->enc_ready) {
        // all or nothing: a context whose encoder scratch could not be allocated in full holds none of it
        const size_t n = (size_t)ctx->cfg.max_streams;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&ctx->h_enc_full), 16, hipHostMallocMapped);
        if (e == hipSuccess) {
            *ctx->h_enc_full = 0;
            e = hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_enc_full), ctx->h_enc_full, 0);
        }
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_state, n);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_pics, 2 * n * kFrameBytes);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_slices, n * kMbH * enc::kSliceCap);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_slice_len, n * kMbH);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_act, n * kMbH * 2);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_cut_pics, 2 * n * enc::kCutBytes);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_cut_sums, n * kMbH * 2);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_info, n * kEncInfoCap);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_tables, 1);
        if (e == hipSuccess) {
            ctx->h_enc_tables.reset(new enc::Tables);
            enc::build_tables(ctx->h_enc_tables.get());
            e = hipMemcpyAsync(ctx->d_enc_tables, ctx->h_enc_tables.get(), sizeof(enc::Tables), hipMemcpyHostToDevice, ctx->stream);
        }
        if (e != hipSuccess) {
            void* bufs[] = {ctx->d_enc_state, ctx->d_enc_pics, ctx->d_enc_slices, ctx->d_enc_slice_len, ctx->d_enc_act,
                            ctx->d_enc_cut_pics, ctx->d_enc_cut_sums, ctx->d_enc_info, ctx->d_enc_tables};
            for (void* b : bufs)
                (void)dev_free(b);
            if (ctx->h_enc_full)
                (void)hipHostFree(ctx->h_enc_full);
            ctx->d_enc_state = nullptr;
            ctx->d_enc_pics = ctx->d_enc_slices = nullptr;
            ctx->d_enc_slice_len = ctx->d_enc_act = ctx->h_enc_full = ctx->d_enc_full = nullptr;
            ctx->d_enc_tables = nullptr;
            ctx->d_enc_cut_pics = nullptr;
            ctx->d_enc_cut_sums = nullptr;
            ctx->d_enc_info = nullptr;
            (void)hipGetLastError();
            return fail(ctx, EFX_ERR_DEVICE, "efx_encode: cannot allocate the encoder's state and scratch", e);
        }
        ctx->enc_ready = true;
    }
    const enc::AqParams aq = o->cont ? ctx->enc_aq : ctx->enc_next_aq;
    if (aq.strength > 0 && !ctx->d_enc_aq_map) {
        // only a context that uses adaptive quantisation holds its scratch; all or nothing, like the rest
        const size_t n = (size_t)ctx->cfg.max_streams;
        hipError_t e = dalloc(&ctx->d_enc_aq_act, n * kMbH * kMbW);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_aq_sums, n * kMbH);
        if (e == hipSuccess) e = dalloc(&ctx->d_enc_aq_map, n * kEncInfoCap * enc::kAqMbs);
        if (e != hipSuccess) {
            (void)dev_free(ctx->d_enc_aq_act);
            (void)dev_free(ctx->d_enc_aq_sums);
            (void)dev_free(ctx->d_enc_aq_map);
            ctx->d_enc_aq_act = nullptr;
            ctx->d_enc_aq_sums = nullptr;
            ctx->d_enc_aq_map = nullptr;
            (void)hipGetLastError();
            return fail(ctx, EFX_ERR_DEVICE, "efx_encode: cannot allocate the scratch of adaptive quantisation", e);
        }
    }
    if (!o->cont)
        ctx->enc_generation = ctx->enc_generation + 1 ? ctx->enc_generation + 1 : 1;  // (0: no call has filled a region)
    EncArgs a{};
    a.src = src_device;
    a.src_stride = o->src_stride;
    a.dst = dst_device;
    a.dst_stride = o->dst_stride;
    a.len = len_device;
    a.status = status_device;
    a.recon = recon_device;
    a.st = ctx->d_enc_state;
    a.pics = ctx->d_enc_pics;
    a.slices = ctx->d_enc_slices;
    a.slice_len = ctx->d_enc_slice_len;
    a.tab = ctx->d_enc_tables;
    a.full_flag = ctx->d_enc_full;
    a.generation = ctx->enc_generation;
    a.first_pts = o->first_pts;
    a.n_streams = o->n_streams;
    a.n_pictures = o->n_pictures;
    a.qscale = o->qscale;
    a.gop = o->gop;
    a.search = o->search;
    a.format = o->format;
    a.f_code = o->search <= 7 ? 1 : 2;
    a.cont = o->cont;
    a.rate_code = o->cont ? ctx->enc_rate_code : ctx->enc_next_rate_code;
    a.cut = o->cont ? ctx->enc_cut : ctx->enc_next_cut;
    a.cut_pics = ctx->d_enc_cut_pics;
    a.cut_sums = ctx->d_enc_cut_sums;
    a.info = ctx->d_enc_info;
    a.aq = aq;
    a.aq_act = ctx->d_enc_aq_act;
    a.aq_sums = ctx->d_enc_aq_sums;
    a.aq_map = ctx->d_enc_aq_map;
    if (rate) {
        a.rc = 1;
        a.rate.cap = (int64_t)rate->vbv_bits * 90000;
        a.rate.gain = (int64_t)rate->bitrate * enc::kRcTick;
        a.bitrate = rate->bitrate;
        a.rate.qmin = rate->qmin;
        a.rate.qmax = rate->qmax;
        a.rate.q0 = o->qscale < rate->qmin ? rate->qmin : (o->qscale > rate->qmax ? rate->qmax : o->qscale);
        a.act = ctx->d_enc_act;
        a.qscale_out = qscale_out_device;
    }
    hipLaunchKernelGGL(k_enc_begin, dim3((unsigned)((o->n_streams + 63) / 64)), dim3(64), 0, ctx->stream, a);
    for (int p = 0; p < o->n_pictures; p++) {
        a.picture = p;
        if (a.aq.strength > 0)
            hipLaunchKernelGGL(k_enc_aq, dim3((unsigned)o->n_streams * kMbH), dim3(64), 0, ctx->stream, a);
        if (a.cut.threshold > 0)
            hipLaunchKernelGGL(k_enc_cut, dim3((unsigned)o->n_streams * kMbH), dim3(64), 0, ctx->stream, a);
        if (rate)
            hipLaunchKernelGGL(k_enc_act, dim3((unsigned)o->n_streams * kMbH), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(a.aq.strength > 0 ? k_enc_rows_t<true> : k_enc_rows_t<false>, dim3((unsigned)o->n_streams * kMbH), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_enc_pack, dim3((unsigned)o->n_streams), dim3(256), 0, ctx->stream, a);
    }
    EFX_HIP(hipGetLastError());
    ctx->enc_info_streams = o->n_streams;
    ctx->enc_info_pictures = o->n_pictures;
    ctx->enc_info_aq = a.aq.strength > 0;
    if (!o->cont) {
        ctx->enc_cut = a.cut;
        ctx->enc_aq = a.aq;
        ctx->enc_started = true;
        ctx->enc_n_streams = o->n_streams;
        ctx->enc_format = o->format;
        ctx->enc_gop = o->gop;
        ctx->enc_rate_code = a.rate_code;
        ctx->enc_rc = rate != nullptr;
        ctx->enc_bitrate = rate ? rate->bitrate : 0;
        ctx->enc_vbv_bits = rate ? rate->vbv_bits : 0;
    }
    return EFX_OK;
}

int efx_encode(efx_ctx* ctx, const efx_encode_opts* o, const uint8_t* src_device, uint8_t* dst_device, uint32_t* len_device,
               uint32_t* status_device, uint8_t* recon_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    return encode_impl(ctx, o, nullptr, src_device, dst_device, len_device, status_device, recon_device, nullptr);
}

int efx_encode_rc(efx_ctx* ctx, const efx_encode_opts* o, const efx_encode_rate* rate, const uint8_t* src_device, uint8_t* dst_device,
                  uint32_t* len_device, uint32_t* status_device, uint8_t* recon_device, uint8_t* qscale_out_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    if (!rate)
        return fail(ctx, EFX_ERR_ARG, "efx_encode_rc: rate is NULL");
    if (rate->bitrate < 8000 || rate->bitrate > 100000000)
        return fail(ctx, EFX_ERR_ARG, "efx_encode_rc: bitrate outside 8000 .. 100000000 bit/s");
    if (rate->vbv_bits < 4000 || rate->vbv_bits > 16000000)
        return fail(ctx, EFX_ERR_ARG, "efx_encode_rc: vbv_bits outside 4000 .. 16000000");
    if (rate->qmin < 1 || rate->qmin > rate->qmax || rate->qmax > 31)
        return fail(ctx, EFX_ERR_ARG, "efx_encode_rc: qmin / qmax must satisfy 1 <= qmin <= qmax <= 31");
    return encode_impl(ctx, o, rate, src_device, dst_device, len_device, status_device, recon_device, qscale_out_device);
}

int efx_pdm(efx_ctx* ctx, int n_streams, const int16_t* pcm_device, int n_samples, int32_t* state_device, uint16_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !pcm_device || !state_device || !dst_device || n_streams <= 0 || n_samples <= 0)
        return EFX_ERR_ARG;
    // k_pdm stores a sample's two words as one dword and reads the states as int32
    if (((uintptr_t)dst_device | (uintptr_t)state_device) & 3)
        return fail(ctx, EFX_ERR_ARG, "efx_pdm: dst_device and state_device must be 4-byte aligned");
    hipLaunchKernelGGL(k_pdm, dim3((n_streams + 63) / 64), dim3(64), 0, ctx->stream, pcm_device, n_streams, n_samples,
                       state_device, dst_device);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}


// ---- audio elementary stream of a batch of transport streams (push_audio's input) ------------------

int efx_demux_audio(efx_ctx* ctx, int n_streams, const uint8_t* const* ts, const size_t* len, uint8_t* audio_device,
                    size_t stride, uint32_t* audio_len_device)
{
    bind_device(ctx);
    if (!ctx || !ts || !len || !audio_device || !audio_len_device || n_streams <= 0)
        return fail(ctx, EFX_ERR_ARG, "efx_demux_audio: bad argument");
    if (n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_CAPACITY, "efx_demux_audio: more streams than max_streams");
    int r = ensure_ts_buffers(ctx);
    if (r)
        return r;
    // the TS staging buffers are shared with efx_upload_streams: nothing may be in flight
    r = sync_all(ctx);
    if (r)
        return r;
    uint8_t* const h_stage = ctx->up[0].h_es;
    std::vector<uint64_t> off((size_t)n_streams + 1), out_off((size_t)n_streams + 1);
    std::vector<uint32_t> tlen(n_streams), pbase(n_streams);
    size_t pos = 0, packets = 0, max_len = 0;
    for (int i = 0; i < n_streams; i++) {
        pbase[i] = (uint32_t)packets;
        packets += len[i] / 188;
        max_len = std::max(max_len, len[i]);
        if (!ts[i] && len[i])
            return fail(ctx, EFX_ERR_ARG, "efx_demux_audio: null stream");
        if (len[i] > stride)
            return fail(ctx, EFX_ERR_CAPACITY, "efx_demux_audio: stride smaller than a transport stream");
        const size_t padded = (len[i] + 15) & ~(size_t)15;
        if (pos + padded + kEsGuardBytes > ctx->es_cap)
            return fail(ctx, EFX_ERR_CAPACITY, "efx_demux_audio: more bytes than max_stream_bytes");
        off[i] = pos;
        out_off[i] = (uint64_t)i * stride;
        if (len[i])
            memcpy(h_stage + pos, ts[i], len[i]);
        memset(h_stage + pos + len[i], 0, padded - len[i]);
        tlen[i] = (uint32_t)len[i];
        pos += padded;
    }
    off[n_streams] = pos;
    out_off[n_streams] = (uint64_t)n_streams * stride;
    if (packets > ctx->pes_cap)
        return fail(ctx, EFX_ERR_CAPACITY, "efx_demux_audio: more packets than the context's transport-stream capacity");
    hipStream_t st = ctx->stream;
    uint64_t* d_out_off = nullptr;
    EFX_HIP(dalloc(&d_out_off, (size_t)n_streams + 1));
    hipError_t e = hipMemcpyAsync(ctx->d_ts, h_stage, pos, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_ts_off, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_out_off, out_off.data(), out_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_idx_len, tlen.data(), n_streams * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_idx_base, pbase.data(), n_streams * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const unsigned chunks = (unsigned)std::max<size_t>(1, (max_len / 188 + kDemuxChunk - 1) / kDemuxChunk);
        hipLaunchKernelGGL(k_demux_audio_scan, dim3(chunks, n_streams), dim3(kDemuxThreads), 0, st, ctx->d_ts, ctx->d_ts_off, ctx->d_idx_len, ctx->d_idx_base,
                           ctx->d_demux_chunks);
        hipLaunchKernelGGL(k_demux_audio_offsets, dim3(n_streams), dim3(64), 0, st, ctx->d_idx_len, ctx->d_idx_base, ctx->d_demux_chunks,
                           audio_len_device);
        hipLaunchKernelGGL(k_demux_audio, dim3(chunks, n_streams), dim3(kDemuxThreads), 0, st, ctx->d_ts, ctx->d_ts_off, ctx->d_idx_len, ctx->d_idx_base,
                           ctx->d_demux_chunks, audio_device, d_out_off);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the host staging buffer and d_out_off are free again
    (void)dev_free(d_out_off);
    if (e != hipSuccess)
        return fail(ctx, EFX_ERR_DEVICE, "efx_demux_audio", e);
    return EFX_OK;
}

// ---- trick-play index (indexer/indexer.cpp, espflix.cpp:573-629) -------------------------------------

int efx_index_streams(efx_ctx* ctx, int n_streams, const uint8_t* const* ts, const size_t* len, const uint32_t* trick_speed,
                      uint32_t bin_size, efx_idx_rec* recs, uint32_t* samples, size_t samples_cap)
{
    bind_device(ctx);
    if (!ctx || !ts || !len || !recs || !samples || n_streams <= 0 || bin_size == 0 || samples_cap == 0)
        return fail(ctx, EFX_ERR_ARG, "efx_index_streams: bad argument");
    if (n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_CAPACITY, "efx_index_streams: more streams than max_streams");
    int r = ensure_ts_buffers(ctx);
    if (r)
        return r;
    // the TS staging buffers are shared with efx_upload_streams: nothing may be in flight
    r = sync_all(ctx);
    if (r)
        return r;
    uint8_t* const h_stage = ctx->up[0].h_es;
    std::vector<uint64_t> off((size_t)n_streams + 1);
    std::vector<uint32_t> tlen(n_streams), base(n_streams);
    size_t pos = 0, packets = 0;
    for (int i = 0; i < n_streams; i++) {
        if (!ts[i] && len[i])
            return fail(ctx, EFX_ERR_ARG, "efx_index_streams: null stream");
        const size_t padded = (len[i] + 15) & ~(size_t)15;
        if (pos + padded + kEsGuardBytes > ctx->es_cap)
            return fail(ctx, EFX_ERR_CAPACITY, "efx_index_streams: more bytes than max_stream_bytes");
        off[i] = pos;
        if (len[i])
            memcpy(h_stage + pos, ts[i], len[i]);
        memset(h_stage + pos + len[i], 0, padded - len[i]);
        tlen[i] = (uint32_t)len[i];
        base[i] = (uint32_t)packets;
        packets += len[i] / 188;
        pos += padded;
    }
    off[n_streams] = pos;
    hipStream_t st = ctx->stream;
    uint32_t* d_samples = nullptr;
    EFX_HIP(dalloc(&d_samples, (size_t)n_streams * samples_cap));
    auto done = [&](int code) {
        (void)dev_free(d_samples);
        return code;
    };
    hipError_t e = hipMemcpyAsync(ctx->d_ts, h_stage, pos, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_ts_off, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_idx_len, tlen.data(), n_streams * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_idx_base, base.data(), n_streams * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_samples, 0, (size_t)n_streams * samples_cap * sizeof(uint32_t), st);
    if (e != hipSuccess)
        return done(fail(ctx, EFX_ERR_DEVICE, "efx_index_streams: upload", e));
    hipLaunchKernelGGL(k_ts_sequences, dim3(n_streams), dim3(256), 0, st, ctx->d_ts, ctx->d_ts_off, ctx->d_idx_len, ctx->d_idx_base,
                       ctx->d_idx_seq, ctx->d_idx_info);
    hipLaunchKernelGGL(k_idx_bins, dim3((unsigned)((samples_cap + 255) / 256), n_streams), dim3(256), 0, st, ctx->d_idx_seq,
                       ctx->d_idx_base, ctx->d_idx_info, bin_size, d_samples, samples_cap);
    std::vector<IdxInfo> info(n_streams);
    e = hipMemcpyAsync(info.data(), ctx->d_idx_info, n_streams * sizeof(IdxInfo), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(samples, d_samples, (size_t)n_streams * samples_cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return done(fail(ctx, EFX_ERR_DEVICE, "efx_index_streams: kernels", e));
    int status = EFX_OK;
    for (int i = 0; i < n_streams; i++) {
        efx_idx_rec& rec = recs[i];
        memset(&rec, 0, sizeof(rec));
        rec.first_pts = info[i].first_pts;
        rec.last_pts = info[i].last_pts;
        rec.bin_size = bin_size;
        rec.trick_speed = trick_speed ? trick_speed[i] : 1;
        const int64_t end = rec.last_pts - rec.first_pts;
        if (!info[i].n_seq || end < 0)
            continue;  // no sequence header: sample_count 0 (the indexer would index out of an empty list)
        const uint64_t count = (uint64_t)(end / bin_size) + 1;
        if (count > samples_cap) {
            status = fail(ctx, EFX_ERR_CAPACITY, "efx_index_streams: samples_cap too small");
            continue;
        }
        rec.sample_count = (uint32_t)count;
    }
    return done(status);
}

size_t efx_idx_build(const efx_idx_rec recs[3], const uint32_t* const samples[3], uint8_t* out, size_t cap)
{
    if (!recs || !samples)
        return 0;
    size_t total = 8 + 3 * sizeof(efx_idx_rec);
    for (int k = 0; k < 3; k++)
        total += 4 * (size_t)recs[k].sample_count;
    if (!out || total > cap)
        return total;
    const uint32_t sig = 'I' | ('D' << 8) | ('X' << 16), three = 3;  // merge_index, indexer.cpp:225-227
    memcpy(out, &sig, 4);
    memcpy(out + 4, &three, 4);
    uint8_t* p = out + 8;
    for (int k = 0; k < 3; k++) {
        efx_idx_rec r = recs[k];
        r.reserved = 0;
        memcpy(p, &r, sizeof(r));
        p += sizeof(r);
    }
    for (int k = 0; k < 3; k++) {
        memcpy(p, samples[k], 4 * (size_t)recs[k].sample_count);
        p += 4 * (size_t)recs[k].sample_count;
    }
    return total;
}

static void idx_recs(const void* hdr, efx_idx_rec r[3]) { memcpy(r, static_cast<const uint8_t*>(hdr) + 8, 3 * sizeof(efx_idx_rec)); }

static int64_t idx_map_pts(int64_t pts, const efx_idx_rec& r, const efx_idx_rec& video)  // espflix.cpp:589-594
{
    pts -= r.first_pts;
    pts *= video.last_pts - video.first_pts;
    const int64_t d = r.last_pts - r.first_pts;
    return d ? pts / d : 0;  // a one-picture trick stream would divide by zero in the reference
}

int64_t efx_idx_pts2pts(const void* idx_hdr, int64_t pts, int speed)  // espflix.cpp:597-604
{
    efx_idx_rec r[3];
    idx_recs(idx_hdr, r);
    if (speed == 1)
        return r[0].first_pts + idx_map_pts(pts, r[1], r[0]);
    if (speed == -1)
        return r[0].last_pts - idx_map_pts(pts, r[2], r[0]);
    return pts;
}

uint32_t efx_idx_pts2offset(const void* idx_hdr, int64_t pts, int speed)  // espflix.cpp:607-627
{
    efx_idx_rec r[3];
    idx_recs(idx_hdr, r);
    const efx_idx_rec &video = r[0], &fwd = r[1], &rwd = r[2];
    pts = std::max(std::min(pts, video.last_pts), video.first_pts);
    uint32_t offset;
    switch (speed) {
    case 1:
        offset = (uint32_t)(pts - video.first_pts) / fwd.trick_speed / fwd.bin_size;
        offset = std::min(fwd.sample_count - 1, offset);
        offset += video.sample_count;
        break;
    case -1:
        offset = (uint32_t)((video.last_pts - pts) - video.first_pts) / rwd.trick_speed / rwd.bin_size;
        offset = std::min(rwd.sample_count - 1, offset);
        offset += video.sample_count + fwd.sample_count;
        break;
    default:
        offset = (uint32_t)((pts - video.first_pts) / video.bin_size);
        offset = std::min(video.sample_count - 1, offset);
        break;
    }
    return offset * 4 + (uint32_t)(8 + 3 * sizeof(efx_idx_rec));
}

size_t efx_sbc_state_bytes(void) { return sizeof(SbcState); }

int efx_sbc_decode(efx_ctx* ctx, int n_streams, const uint8_t* frames_device, size_t stream_stride, int frame_bytes,
                   int n_frames, void* state_device, int16_t* pcm_device, size_t pcm_stride, uint32_t* ret_device,
                   uint32_t* pcm_count_device, int flags)
{
    bind_device(ctx);
    if (!ctx || !frames_device || !state_device || !pcm_device || n_streams <= 0 || n_frames < 0 || frame_bytes <= 0 ||
        (size_t)frame_bytes * (size_t)n_frames >= (1u << 28) || ((uintptr_t)state_device & 3))
        return EFX_ERR_ARG;
    SbcState* const state = static_cast<SbcState*>(state_device);
    if (n_frames == 0 || ctx->opt_sbc_serial) {
        // one wave per stream walking its frames (no frames: it leaves the state as it reads it and a PCM count of zero)
        hipLaunchKernelGGL(k_sbc, dim3(n_streams), dim3(64), 0, ctx->stream, frames_device, stream_stride, frame_bytes, n_frames, state,
                           ctx->d_sbc_tables, pcm_device, pcm_stride, ret_device, pcm_count_device, flags);
        EFX_HIP(hipGetLastError());
        return EFX_OK;
    }
    // scratch: which kernel decodes a stream + the three work lists + their counters; the states on their way; per frame the
    // bit allocation (k_sbc_frames) and, for streams that are not regular, the plan (k_sbc_plan)
    if ((size_t)n_streams > ctx->sbc_flags_cap) {
        if (ctx->d_sbc_flags)
            (void)dev_free(ctx->d_sbc_flags);
        if (ctx->d_sbc_next)
            (void)dev_free(ctx->d_sbc_next);
        ctx->d_sbc_flags = nullptr;
        ctx->d_sbc_next = nullptr;
        ctx->sbc_flags_cap = 0;
        EFX_HIP(dalloc(&ctx->d_sbc_flags, (size_t)n_streams * 4 + sizeof(SbcQueues) / 4));
        EFX_HIP(dalloc(&ctx->d_sbc_next, (size_t)n_streams));
        ctx->sbc_flags_cap = (size_t)n_streams;
        ctx->sbc_flags_clean = false;
    }
    const size_t info_need = (size_t)n_streams * ((size_t)n_frames + 1);
    if (info_need > ctx->sbc_info_cap) {
        if (ctx->d_sbc_info)
            (void)dev_free(ctx->d_sbc_info);
        if (ctx->d_sbc_plan)
            (void)dev_free(ctx->d_sbc_plan);
        ctx->d_sbc_info = nullptr;
        ctx->d_sbc_plan = nullptr;
        ctx->sbc_info_cap = 0;
        EFX_HIP(dalloc(&ctx->d_sbc_info, info_need));
        EFX_HIP(dalloc(&ctx->d_sbc_plan, info_need));
        ctx->sbc_info_cap = info_need;
    }
    // per (stream, granule of eight frames): a slot in each of the two tables of chunks a regular kernel takes, a cover byte
    const int n_gran = (n_frames + 7) / 8, extra_cap = n_streams * n_gran;
    if ((size_t)extra_cap > ctx->sbc_gran_cap) {
        if (ctx->d_sbc_extra)
            (void)dev_free(ctx->d_sbc_extra);
        if (ctx->d_sbc_cover)
            (void)dev_free(ctx->d_sbc_cover);
        ctx->d_sbc_extra = nullptr;
        ctx->d_sbc_cover = nullptr;
        ctx->sbc_gran_cap = 0;
        EFX_HIP(dalloc(&ctx->d_sbc_extra, 2 * (size_t)extra_cap));
        EFX_HIP(dalloc(&ctx->d_sbc_cover, (size_t)extra_cap));
        ctx->sbc_gran_cap = (size_t)extra_cap;
    }
    uint32_t* const d_how = ctx->d_sbc_flags;
    uint32_t* const d_lists = d_how + ctx->sbc_flags_cap;
    SbcQueues* const d_queues = reinterpret_cast<SbcQueues*>(d_how + 4 * ctx->sbc_flags_cap);
    // parallel[]: every word kSbcRegularFlag when k_sbc_frames starts -- as the previous call's k_sbc_finish left them
    if (!ctx->sbc_flags_clean)
        EFX_HIP(hipMemsetAsync(d_how, 0xFF, ctx->sbc_flags_cap * sizeof(uint32_t), ctx->stream));
    ctx->sbc_flags_clean = false;
    hipLaunchKernelGGL(k_sbc_frames, dim3((n_frames + 255) / 256, n_streams), dim3(256), 0, ctx->stream, frames_device, stream_stride,
                       frame_bytes, n_frames, ctx->d_sbc_info, ret_device, d_how, d_queues);
    hipLaunchKernelGGL(k_sbc_plan, dim3(n_streams + 1), dim3(256), 0, ctx->stream, ctx->d_sbc_info, n_frames, flags, state, ctx->d_sbc_plan,
                       d_how, d_queues, d_lists, n_streams, (int)ctx->sbc_flags_cap, ret_device, pcm_count_device, ctx->d_sbc_extra,
                       ctx->d_sbc_cover);
    // Persistent workgroups take (stream, chunk of frames) items off the list of their kind, dealt round robin; a list that
    // stayed empty costs its kernel one look.  Grids = what is resident at a time: kSbcMonoWgPerCu workgroups per compute unit
    // for the mono kernel (16 frames per item: 36 KB of LDS), 4 for the other two (35 KB of LDS).
    const long long items = (long long)n_streams * ((n_frames + 8) / 8);
    const int g_mono = (int)std::min<long long>(items, (long long)ctx->n_cus * kSbcMonoWgPerCu), g_wide = (int)std::min<long long>(items, (long long)ctx->n_cus * 4);
    hipLaunchKernelGGL(k_sbc_par_mono, dim3(g_mono), dim3(256), 0, ctx->stream, frames_device, stream_stride, frame_bytes, n_frames, state,
                       ctx->d_sbc_next, ctx->d_sbc_tables, ctx->d_sbc_info, pcm_device, pcm_stride, pcm_count_device, flags, d_queues, d_lists,
                       (int)ctx->sbc_flags_cap, ctx->d_sbc_extra, extra_cap);
    hipLaunchKernelGGL(k_sbc_par_stereo, dim3(g_wide), dim3(256), 0, ctx->stream, frames_device, stream_stride, frame_bytes, n_frames, state,
                       ctx->d_sbc_next, ctx->d_sbc_tables, ctx->d_sbc_info, pcm_device, pcm_stride, pcm_count_device, flags, d_queues, d_lists,
                       (int)ctx->sbc_flags_cap, ctx->d_sbc_extra, extra_cap);
    hipLaunchKernelGGL(k_sbc_gen, dim3(g_wide), dim3(256), 0, ctx->stream, frames_device, stream_stride, frame_bytes, n_frames, state,
                       ctx->d_sbc_next, ctx->d_sbc_tables, ctx->d_sbc_info, ctx->d_sbc_plan, pcm_device, pcm_stride, flags, d_queues, d_lists,
                       (int)ctx->sbc_flags_cap, ctx->d_sbc_cover, n_gran);
    // the new states take their place; a stream whose state no call of this library can have left is decoded by one wave
    hipLaunchKernelGGL(k_sbc_finish, dim3(n_streams), dim3(64), 0, ctx->stream, frames_device, stream_stride, frame_bytes, n_frames, state,
                       ctx->d_sbc_next, ctx->d_sbc_tables, pcm_device, pcm_stride, ret_device, pcm_count_device, flags, d_how);
    EFX_HIP(hipGetLastError());
    ctx->sbc_flags_clean = true;
    return EFX_OK;
}

// ---- SBC encode (k_sbc_enc.hip) -------------------------------------------------------------------------------------------------
size_t efx_sbc_frame_bytes(int blocks, int channels, int bitpool)
{
    if ((blocks != 4 && blocks != 8 && blocks != 12 && blocks != 16) || channels < 1 || channels > 2 || bitpool < 2 || bitpool > 128)
        return 0;
    return sbcenc::frame_bytes(blocks, channels, bitpool);
}

size_t efx_sbc_enc_state_bytes(void) { return sbcenc::kStateBytes; }

int efx_sbc_encode(efx_ctx* ctx, const efx_sbc_encode_opts* o, const int16_t* pcm_device, void* state_device, uint8_t* frames_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    auto misaligned = [](const void* p) { return !p || ((uintptr_t)p & 15); };
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: n_streams outside 1 .. max_streams");
    if (o->frequency < 0 || o->frequency > 3)
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: frequency outside 0 .. 3");
    if (o->blocks != 4 && o->blocks != 8 && o->blocks != 12 && o->blocks != 16)
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: blocks must be 4, 8, 12 or 16");
    if (o->mode != 0 && o->mode != 1)
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: mode must be 0 (mono) or 1 (dual channel): the reference decodes no joint stereo, and its stereo is not the standard's");
    if (o->allocation != 0 && o->allocation != 1)
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: allocation must be 0 (loudness) or 1 (SNR)");
    if (o->bitpool < 2 || o->bitpool > 128)
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: bitpool outside 2 .. 128");
    if (o->pcm_layout != EFX_PCM_FRAME_PLANAR && o->pcm_layout != EFX_PCM_INTERLEAVED)
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: unknown pcm_layout");
    const int channels = o->mode ? 2 : 1, spf = o->blocks * 8;
    if (o->n_frames < 1 || (long long)o->n_frames * spf >= (1ll << 31))
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: n_frames must be >= 1 and n_frames x samples per frame below 2^31");
    const size_t fb = sbcenc::frame_bytes(o->blocks, channels, o->bitpool);
    if (o->pcm_stride < (size_t)o->n_frames * spf * channels)
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: pcm_stride does not hold n_frames frames");
    if (o->frame_stride < (size_t)o->n_frames * fb || (o->frame_stride & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: frame_stride must be a multiple of 16 and hold n_frames frames");
    if (misaligned(pcm_device) || misaligned(state_device) || misaligned(frames_device))
        return fail(ctx, EFX_ERR_ARG, "efx_sbc_encode: pcm, state and frames must be 16-byte aligned device pointers");
    SbcEncArgs a{};
    a.pcm = pcm_device;
    a.state = static_cast<int16_t*>(state_device);
    a.frames = frames_device;
    a.tables = ctx->d_sbc_enc_tables;
    a.pcm_stride = o->pcm_stride;
    a.frame_stride = o->frame_stride;
    a.frame_bytes = (uint32_t)fb;
    a.n_streams = o->n_streams;
    a.n_frames = o->n_frames;
    a.n_groups = (o->n_frames + 3) / 4;
    a.frequency = o->frequency;
    a.blocks = o->blocks;
    a.mode = o->mode;
    a.allocation = o->allocation;
    a.bitpool = o->bitpool;
    a.layout = o->pcm_layout;
    // (both grid dimensions are strided over by the kernel: the caps only bound the launch)
    const dim3 grid((unsigned)std::min(a.n_groups, 1 << 20), (unsigned)std::min(a.n_streams, 65535));
    hipLaunchKernelGGL(k_sbc_enc, grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_sbc_enc_state, dim3((unsigned)a.n_streams), dim3(192), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- sound in (k_import_pcm.hip) ------------------------------------------------------------------------------------------------
static bool import_pcm_rates_ok(int in_rate, int out_rate)
{
    if (out_rate != 16000 && out_rate != 32000 && out_rate != 44100 && out_rate != 48000)
        return false;
    return in_rate >= ipcm::kMinRate && in_rate <= ipcm::kMaxRate && in_rate <= ipcm::kMaxRatio * out_rate;
}

int efx_import_pcm_out_samples(int in_rate, int out_rate, int64_t first_in, int n_in)
{
    if (!import_pcm_rates_ok(in_rate, out_rate) || first_in < 0 || first_in >= ipcm::kMaxFirstIn || n_in < 0)
        return -1;
    const int64_t n = ipcm::out_samples(in_rate, out_rate, first_in, n_in);
    return n > 0x7FFFFFFF ? -1 : (int)n;
}

int efx_import_pcm_delay(int in_rate, int out_rate)
{
    return import_pcm_rates_ok(in_rate, out_rate) ? ipcm::delay(in_rate, out_rate) : -1;
}

size_t efx_import_pcm_state_bytes(void) { return ipcm::kStateBytes; }

int efx_import_pcm_filter(int32_t* out, int cap)
{
    if (out && cap > 0) {
        std::vector<int32_t> t(ipcm::kTableLen);
        build_import_pcm_table(t.data());
        std::copy(t.begin(), t.begin() + std::min(cap, ipcm::kTableLen), out);
    }
    return ipcm::kTableLen;
}

int efx_import_pcm(efx_ctx* ctx, const efx_import_pcm_opts* o, const int16_t* src_device, void* state_device, int16_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    auto misaligned = [](const void* p) { return !p || ((uintptr_t)p & 15); };
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: n_streams outside 1 .. max_streams");
    if (!import_pcm_rates_ok(o->in_rate, o->out_rate))
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: out_rate must be 16000, 32000, 44100 or 48000, in_rate 8000 .. 192000 and at most 4 x out_rate");
    if (o->channels < 1 || o->channels > ipcm::kMaxChannels)
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: channels outside 1 .. 8");
    if (o->n_in < 1 || (long long)o->n_in * o->channels >= (1ll << 31))
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: n_in must be >= 1 and n_in x channels below 2^31");
    if (o->layout != EFX_PCM_INTERLEAVED && o->layout != EFX_PCM_PLANAR)
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: layout must be EFX_PCM_INTERLEAVED or EFX_PCM_PLANAR");
    long long wsum = 0;
    for (int c = 0; c < o->channels; c++)
        wsum += std::llabs((long long)o->mix_q15[c]);
    if (wsum > 32768)
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: the downmix weights' absolute values sum to more than 32768");
    if (o->first_in < 0 || o->first_in >= ipcm::kMaxFirstIn)
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: first_in outside 0 .. 2^40 - 1");
    const int64_t n_out = ipcm::out_samples(o->in_rate, o->out_rate, o->first_in, o->n_in);
    if (n_out > 0x7FFFFFFF)
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: more than 2^31 - 1 output samples in one call");
    if (o->src_stride < (size_t)o->n_in * o->channels || (o->src_stride & 7))
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: src_stride must be a multiple of 8 and hold n_in x channels elements");
    if (o->dst_stride < (size_t)n_out || (o->dst_stride & 7))
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: dst_stride must be a multiple of 8 and hold the call's output samples");
    const bool equal = o->in_rate == o->out_rate;
    if (misaligned(src_device) || misaligned(dst_device) || (equal ? ((uintptr_t)state_device & 15) != 0 : misaligned(state_device)))
        return fail(ctx, EFX_ERR_ARG, "efx_import_pcm: src, state and dst must be 16-byte aligned device pointers");
    ImportPcmArgs a{};
    a.src = src_device;
    a.state = equal ? nullptr : static_cast<int16_t*>(state_device);
    a.dst = dst_device;
    a.table = ctx->d_import_pcm_table;
    a.src_stride = o->src_stride;
    a.dst_stride = o->dst_stride;
    a.plan = ipcm::plan(o->in_rate, o->out_rate, o->channels, o->layout, o->mix_q15, o->first_in, o->n_in);
    if (n_out > 0) {
        // a stream's tiles go round robin over grid.y workgroups, which copy the table into LDS once each: enough
        // workgroups to fill the device, no more than there are tiles
        const int tiles = (int)((n_out + ipcm::kTile - 1) / ipcm::kTile);
        const int per_stream = std::max(1, std::min(tiles, (8 * ctx->n_cus + o->n_streams - 1) / o->n_streams));
        hipLaunchKernelGGL(k_import_pcm, dim3((unsigned)o->n_streams, (unsigned)per_stream), dim3(256), 0, ctx->stream, a);
    }
    if (!equal)
        hipLaunchKernelGGL(k_import_pcm_state, dim3((unsigned)o->n_streams), dim3(128), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- programme loudness (k_loudness.hip) ----------------------------------------------------------------------------------------
// Both stages of the K-weighting filter from their analogue prototypes by the bilinear transform (include/efx.h)
static loud::Coefs loudness_coefs(int rate)
{
    const double pi = 3.14159265358979323846;
    double c[10];
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / rate), a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0, c[6] = -2.0, c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
    loud::Coefs k{};
    for (int i = 0; i < 10; i++)
        k.c[i] = (int32_t)std::llround(c[i] * (double)(1 << loud::kCoefBits));
    return k;
}

int efx_loudness_coefs(int rate, int32_t out[10])
{
    if (!loud::rate_ok(rate) || !out)
        return EFX_ERR_ARG;
    const loud::Coefs k = loudness_coefs(rate);
    std::copy(k.c, k.c + 10, out);
    return EFX_OK;
}

size_t efx_loudness_state_bytes(int rate) { return loud::rate_ok(rate) ? 2 * (size_t)loud::hist_of(rate) : 0; }

int efx_loudness_step_count(int rate, int64_t first_sample, int n_samples)
{
    if (!loud::rate_ok(rate) || first_sample < 0 || first_sample >= loud::kMaxFirstSample || n_samples < 0)
        return -1;
    return (int)loud::step_count(rate, first_sample, n_samples);
}

double efx_loudness_lufs(uint64_t block_energy, int rate)
{
    if (!loud::rate_ok(rate))
        return std::nan("");
    if (!block_energy)
        return -HUGE_VAL;
    return -0.691 + 10.0 * std::log10((double)block_energy / (4.0 * loud::step_of(rate) * 1073741824.0 * 256.0));
}

int efx_loudness_thresholds(int rate, double target_lufs, double peak_dbfs, uint64_t* abs_thr, uint64_t* target_ms, uint32_t* ceiling)
{
    if (!loud::rate_ok(rate) || !(target_lufs >= -70.0 && target_lufs <= 0.0) || !(peak_dbfs >= -90.0 && peak_dbfs <= 0.0))
        return EFX_ERR_ARG;
    const double unit = 1073741824.0 * 256.0;  // a full-scale square's mean square with the four fraction bits
    if (abs_thr)
        *abs_thr = (uint64_t)std::llround(std::pow(10.0, (-70.0 + 0.691) / 10.0) * unit * 4.0 * loud::step_of(rate));
    if (target_ms)
        *target_ms = (uint64_t)std::llround(std::pow(10.0, (target_lufs + 0.691) / 10.0) * unit);
    if (ceiling)
        *ceiling = (uint32_t)std::max(1L, std::lround(32767.0 * std::pow(10.0, peak_dbfs / 20.0)));
    return EFX_OK;
}

int efx_loudness_steps(efx_ctx* ctx, const efx_loudness_steps_opts* o, const int16_t* pcm_device, void* state_device,
                       efx_loudness_step* steps_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    auto misaligned = [](const void* p) { return !p || ((uintptr_t)p & 15); };
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_steps: n_streams outside 1 .. max_streams");
    if (!loud::rate_ok(o->rate))
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_steps: rate must be 16000, 32000, 44100 or 48000");
    if (o->n_samples < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_steps: n_samples must be >= 1");
    if (o->first_sample < 0 || o->first_sample >= loud::kMaxFirstSample)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_steps: first_sample outside 0 .. 2^40 - 1");
    const int64_t n_new = loud::step_count(o->rate, o->first_sample, o->n_samples);
    if (o->first_step < 0 || (int64_t)o->first_step + n_new > 0x7FFFFFFF)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_steps: first_step negative or past 2^31 - 1 with the call's steps");
    if (o->pcm_stride < (size_t)o->n_samples || (o->pcm_stride & 7))
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_steps: pcm_stride must be a multiple of 8 and hold n_samples elements");
    if (o->steps_stride < (size_t)o->first_step + (size_t)n_new)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_steps: steps_stride must hold first_step + the call's new records");
    if (misaligned(pcm_device) || misaligned(state_device) || misaligned(steps_device))
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_steps: pcm, state and steps must be 16-byte aligned device pointers");
    static_assert(sizeof(efx_loudness_step) == sizeof(loud::StepRec) && sizeof(loud::StepRec) == 16, "one 16-byte store per record");
    LoudStepsArgs a{};
    a.pcm = pcm_device;
    a.state = static_cast<int16_t*>(state_device);
    a.steps = reinterpret_cast<loud::StepRec*>(steps_device);
    a.pcm_stride = o->pcm_stride;
    a.steps_stride = o->steps_stride;
    a.first_step = o->first_step;
    a.plan = loud::plan(o->rate, loudness_coefs(o->rate), o->first_sample, o->n_samples);
    if (n_new > 0)
        hipLaunchKernelGGL(k_loud_steps, dim3((unsigned)o->n_streams, (unsigned)((n_new + loud::kLanes - 1) / loud::kLanes)),
                           dim3(loud::kLanes), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_loud_state, dim3((unsigned)o->n_streams), dim3(256), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return (int)n_new;
}

int efx_loudness_gate(efx_ctx* ctx, const efx_loudness_gate_opts* o, const efx_loudness_step* steps_device, const void* state_device,
                      efx_loudness_rec* recs_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_gate: n_streams outside 1 .. max_streams");
    if (!loud::rate_ok(o->rate))
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_gate: rate must be 16000, 32000, 44100 or 48000");
    if (o->n_steps < 0 || o->n_steps > loud::kMaxSteps)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_gate: n_steps outside 0 .. 2^24");
    if (o->target_ms >= loud::kMaxTarget || o->ceiling < 1 || o->ceiling > 32767)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_gate: target_ms must be below 2^40 and ceiling 1 .. 32767");
    if (o->steps_stride < (size_t)o->n_steps)
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_gate: steps_stride must hold n_steps records");
    if (!steps_device || !recs_device || ((uintptr_t)steps_device & 15) || ((uintptr_t)recs_device & 15) || ((uintptr_t)state_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_loudness_gate: steps and recs must be 16-byte aligned device pointers, state NULL or aligned");
    static_assert(sizeof(efx_loudness_rec) == sizeof(loud::GateRec) && sizeof(loud::GateRec) == 32, "two 16-byte stores per record");
    LoudGateArgs a{};
    a.steps = reinterpret_cast<const loud::StepRec*>(steps_device);
    a.state = static_cast<const int16_t*>(state_device);
    a.recs = reinterpret_cast<loud::GateRec*>(recs_device);
    a.steps_stride = o->steps_stride;
    a.abs_thr = o->abs_thr, a.target_ms = o->target_ms, a.ceiling = o->ceiling;
    a.n_steps = o->n_steps, a.step = loud::step_of(o->rate), a.hist = loud::hist_of(o->rate);
    hipLaunchKernelGGL(k_loud_gate, dim3((unsigned)o->n_streams), dim3(256), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

int efx_pcm_gain(efx_ctx* ctx, const efx_pcm_gain_opts* o, const int16_t* src_device, const efx_loudness_rec* recs_device,
                 int16_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    auto misaligned = [](const void* p) { return !p || ((uintptr_t)p & 15); };
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_gain: n_streams outside 1 .. max_streams");
    if (o->n_samples < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_gain: n_samples must be >= 1");
    if (!recs_device && (o->fixed_gain_q12 < 1 || o->fixed_gain_q12 > loud::kMaxGain))
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_gain: fixed_gain_q12 outside 1 .. 32767");
    if (o->src_stride < (size_t)o->n_samples || (o->src_stride & 7) || o->dst_stride < (size_t)o->n_samples || (o->dst_stride & 7))
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_gain: the strides must be multiples of 8 and hold n_samples elements");
    if (misaligned(src_device) || misaligned(dst_device) || ((uintptr_t)recs_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_gain: src and dst must be 16-byte aligned device pointers, recs NULL or aligned");
    PcmGainArgs a{};
    a.src = src_device;
    a.recs = reinterpret_cast<const loud::GateRec*>(recs_device);
    a.dst = dst_device;
    a.src_stride = o->src_stride, a.dst_stride = o->dst_stride;
    a.n_samples = o->n_samples, a.fixed_gain = o->fixed_gain_q12;
    // (grid.y is strided over by the kernel: the cap only bounds the launch)
    const int per_stream = std::max(1, std::min((o->n_samples + 2047) / 2048, (8 * ctx->n_cus + o->n_streams - 1) / o->n_streams));
    hipLaunchKernelGGL(k_pcm_gain, dim3((unsigned)o->n_streams, (unsigned)per_stream), dim3(256), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- peak limiter (k_limit.hip) ---------------------------------------------------------------------------------------------------
int efx_limit_block(int rate) { return limit::block_of(rate); }

int efx_limit_gain(uint64_t gated_mean, uint32_t n_gated, uint64_t target_ms, int rate)
{
    if (!loud::rate_ok(rate) || target_ms >= loud::kMaxTarget)
        return 0;
    return loud::stream_gain_q12(gated_mean, n_gated, target_ms, loud::step_of(rate));
}

// workgroups per stream: every tile one, up to eight workgroups per compute unit over the streams (the kernels stride over
// grid.y, so the cap only bounds the launch)
static unsigned limit_grid_y(const efx_ctx* ctx, int n_streams, int n_samples, int bk)
{
    const int64_t n_tiles = ((int64_t)n_samples + (int64_t)limit::kTile * bk - 1) / ((int64_t)limit::kTile * bk);
    const int64_t share = (8 * (int64_t)ctx->n_cus + n_streams - 1) / n_streams;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::min(n_tiles, share), 65535));
}

int efx_limit_peaks(efx_ctx* ctx, const efx_limit_peaks_opts* o, const int16_t* pcm_device, uint16_t* peaks_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    auto misaligned = [](const void* p) { return !p || ((uintptr_t)p & 15); };
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_limit_peaks: n_streams outside 1 .. max_streams");
    const int bk = limit::block_of(o->rate);
    if (!bk)
        return fail(ctx, EFX_ERR_ARG, "efx_limit_peaks: rate must be 16000, 32000, 44100 or 48000");
    if (o->n_samples < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_limit_peaks: n_samples must be >= 1");
    if (o->first_sample < 0 || o->first_sample >= limit::kMaxFirstSample || o->first_sample % bk)
        return fail(ctx, EFX_ERR_ARG, "efx_limit_peaks: first_sample outside 0 .. 2^40 - 1 or not a multiple of the block length");
    const int64_t first_block = o->first_sample / bk, n_blocks = ((int64_t)o->n_samples + bk - 1) / bk;
    if (o->peaks_first < 0 || o->peaks_first > first_block)
        return fail(ctx, EFX_ERR_ARG, "efx_limit_peaks: peaks_first outside 0 .. first_sample / block length");
    if (o->pcm_stride < (uint64_t)o->n_samples || (o->pcm_stride & 7))
        return fail(ctx, EFX_ERR_ARG, "efx_limit_peaks: pcm_stride must be a multiple of 8 and hold n_samples elements");
    if (o->peaks_stride < (uint64_t)(first_block - o->peaks_first + n_blocks))
        return fail(ctx, EFX_ERR_ARG, "efx_limit_peaks: peaks_stride must hold the call's blocks behind first_sample / block length - peaks_first");
    if (misaligned(pcm_device) || misaligned(peaks_device))
        return fail(ctx, EFX_ERR_ARG, "efx_limit_peaks: pcm and peaks must be 16-byte aligned device pointers");
    LimitPeaksArgs a{};
    a.pcm = pcm_device, a.peaks = peaks_device;
    a.pcm_stride = (size_t)o->pcm_stride, a.peaks_stride = (size_t)o->peaks_stride;
    a.entry0 = first_block - o->peaks_first;
    a.n_samples = o->n_samples, a.bk = bk;
    hipLaunchKernelGGL(k_limit_peaks, dim3((unsigned)o->n_streams, limit_grid_y(ctx, o->n_streams, o->n_samples, bk)), dim3(limit::kThreads), 0,
                       ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

int efx_pcm_limit(efx_ctx* ctx, const efx_limit_opts* o, const int16_t* src_device, const uint16_t* peaks_device,
                  const efx_loudness_rec* recs_device, int16_t* dst_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    auto misaligned = [](const void* p) { return !p || ((uintptr_t)p & 15); };
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: n_streams outside 1 .. max_streams");
    const int bk = limit::block_of(o->rate);
    if (!bk)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: rate must be 16000, 32000, 44100 or 48000");
    if (o->n_samples < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: n_samples must be >= 1");
    if (o->half_window < 0 || o->half_window > limit::kMaxHalf)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: half_window outside 0 .. 64");
    if (o->first_sample < 0 || o->first_sample >= limit::kMaxFirstSample || o->first_sample % bk)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: first_sample outside 0 .. 2^40 - 1 or not a multiple of the block length");
    if (o->peaks_first < 0 || o->peaks_first >= limit::kMaxFirstSample)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: peaks_first outside 0 .. 2^40 - 1");
    if (o->n_peaks < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: n_peaks must be >= 1");
    if (o->ceiling < 1 || o->ceiling > 32767)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: ceiling outside 1 .. 32767");
    if (recs_device && o->target_ms >= loud::kMaxTarget)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: target_ms must be below 2^40");
    if (!recs_device && (o->fixed_gain_q12 < 1 || o->fixed_gain_q12 > loud::kMaxGain))
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: fixed_gain_q12 outside 1 .. 32767");
    if (o->src_stride < (uint64_t)o->n_samples || (o->src_stride & 7) || o->dst_stride < (uint64_t)o->n_samples || (o->dst_stride & 7))
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: the sample strides must be multiples of 8 and hold n_samples elements");
    if (o->peaks_stride < (uint64_t)o->n_peaks)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: peaks_stride must hold n_peaks entries");
    if (dst_device == src_device && o->dst_stride != o->src_stride)
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: in place (dst == src) needs equal sample strides");
    if (misaligned(src_device) || misaligned(dst_device) || misaligned(peaks_device) || ((uintptr_t)recs_device & 15))
        return fail(ctx, EFX_ERR_ARG, "efx_pcm_limit: src, peaks and dst must be 16-byte aligned device pointers, recs NULL or aligned");
    PcmLimitArgs a{};
    a.src = src_device, a.peaks = peaks_device, a.dst = dst_device;
    a.recs = reinterpret_cast<const loud::GateRec*>(recs_device);
    a.src_stride = (size_t)o->src_stride, a.dst_stride = (size_t)o->dst_stride, a.peaks_stride = (size_t)o->peaks_stride;
    a.first_block = o->first_sample / bk, a.peaks_first = o->peaks_first;
    a.target_ms = o->target_ms;
    a.n_samples = o->n_samples, a.n_peaks = o->n_peaks, a.bk = bk;
    a.half = o->half_window ? o->half_window : limit::kDefaultHalf;
    a.ceiling = o->ceiling, a.fixed_gain = o->fixed_gain_q12, a.step = loud::step_of(o->rate);
    a.div = limit::div_of(bk);
    hipLaunchKernelGGL(k_pcm_limit, dim3((unsigned)o->n_streams, limit_grid_y(ctx, o->n_streams, o->n_samples, bk)), dim3(limit::kThreads), 0,
                       ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

// ---- A/V multiplexer (k_mux.hip) ------------------------------------------------------------------------------------------------
int efx_mux_audio_packets(int n_frames, int frame_bytes, int frames_per_pes)
{
    if (n_frames < 0 || frame_bytes < 1 || frames_per_pes < 1 || (long long)frames_per_pes * frame_bytes > 2048)
        return -1;
    const long long full = n_frames / frames_per_pes, rest = n_frames % frames_per_pes;
    long long n = full * enc::ts_packets((uint32_t)(14 + frames_per_pes * frame_bytes));
    if (rest)
        n += enc::ts_packets((uint32_t)(14 + rest * frame_bytes));
    return n > 0x7FFFFFFF ? -1 : (int)n;
}

size_t efx_mux_bound(size_t video_bytes, int n_frames, int frame_bytes, int frames_per_pes)
{
    const int ap = efx_mux_audio_packets(n_frames, frame_bytes, frames_per_pes);
    if (ap < 0)
        return 0;
    return (video_bytes + (size_t)ap * 188 + 15) / 16 * 16;
}

int efx_mux_av(efx_ctx* ctx, const efx_mux_opts* o, const uint8_t* video_ts_device, const uint32_t* video_len_device,
               const uint8_t* audio_frames_device, uint8_t* dst_device, uint32_t* len_device, uint32_t* status_device)
{
    bind_device(ctx);
    if (!ctx || !o)
        return EFX_ERR_ARG;
    auto misaligned = [](const void* p) { return !p || ((uintptr_t)p & 15); };
    if (o->n_streams < 1 || o->n_streams > ctx->cfg.max_streams)
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: n_streams outside 1 .. max_streams");
    if (o->audio_pid != 0x101 && o->audio_pid != 0x102)
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: audio_pid must be 0x101 or 0x102");
    if (o->frame_bytes < 1 || o->n_frames < 0 || o->frames_per_pes < 1 || (long long)o->frames_per_pes * o->frame_bytes > 2048)
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: frame_bytes >= 1, n_frames >= 0, frames_per_pes >= 1 and frames_per_pes x frame_bytes <= 2048");
    if (o->samples_per_frame < 1 || o->sample_rate < 1)
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: samples_per_frame and sample_rate must be positive");
    if (o->audio_first_pts < 0 || o->audio_first_pts >= (1ll << 33) || o->audio_first_frame < 0 || o->audio_first_frame >= (1ll << 31))
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: audio_first_pts outside 0 .. 2^33-1 or audio_first_frame outside 0 .. 2^31-1");
    if (o->audio_cc < 0 || o->audio_cc > 15)
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: audio_cc outside 0 .. 15");
    if ((o->video_stride & 15) || (o->audio_stride & 15) || (o->dst_stride & 15) || o->dst_stride >= (1ull << 32) ||
        o->audio_stride < (size_t)o->n_frames * o->frame_bytes)
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: strides must be multiples of 16, audio_stride hold n_frames frames, dst_stride be below 2^32");
    const int ap = efx_mux_audio_packets(o->n_frames, o->frame_bytes, o->frames_per_pes);
    if (ap < 0)
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: too many audio packets for one call");
    if (misaligned(video_ts_device) || misaligned(video_len_device) || misaligned(dst_device) || misaligned(len_device) ||
        misaligned(status_device) || (o->n_frames > 0 && misaligned(audio_frames_device)))
        return fail(ctx, EFX_ERR_ARG, "efx_mux_av: video, video_len, dst, len and status (and audio, with frames) must be 16-byte aligned device pointers");
    MuxArgs a{};
    a.n_pes = (o->n_frames + o->frames_per_pes - 1) / o->frames_per_pes;
    const size_t need = (size_t)o->n_streams * (size_t)std::max(a.n_pes, 1);
    if (need > ctx->mux_before_cap) {
        if (ctx->d_mux_before)
            (void)dev_free(ctx->d_mux_before);
        ctx->d_mux_before = nullptr;
        ctx->mux_before_cap = 0;
        EFX_HIP(dalloc(&ctx->d_mux_before, need));
        ctx->mux_before_cap = need;
    }
    a.video = video_ts_device;
    a.video_len = video_len_device;
    a.audio = audio_frames_device;
    a.dst = dst_device;
    a.len = len_device;
    a.status = status_device;
    a.video_before = ctx->d_mux_before;
    a.video_stride = o->video_stride;
    a.audio_stride = o->audio_stride;
    a.dst_stride = o->dst_stride;
    a.first_pts = o->audio_first_pts;
    a.first_frame = o->audio_first_frame;
    a.n_streams = o->n_streams;
    a.pid = o->audio_pid;
    a.frame_bytes = o->frame_bytes;
    a.n_frames = o->n_frames;
    a.frames_per_pes = o->frames_per_pes;
    a.samples_per_frame = o->samples_per_frame;
    a.sample_rate = o->sample_rate;
    a.cc = o->audio_cc;
    a.pes_packets = (int)enc::ts_packets((uint32_t)(14 + o->frames_per_pes * o->frame_bytes));
    a.audio_packets = ap;
    hipLaunchKernelGGL(k_mux, dim3((unsigned)a.n_streams), dim3(256), 0, ctx->stream, a);
    EFX_HIP(hipGetLastError());
    return EFX_OK;
}

int efx_set_timing(efx_ctx* ctx, int enable)
{
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    if (enable && ctx->timing_ring.empty()) {
        ctx->timing_ring.resize((size_t)kTimingRing * kMaxGroups);  // (the events of a set are created at its first use)
    }
    ctx->timing = enable != 0;
    ctx->timed_calls = 0;  // (re-)enabling starts a new averaging window
    return EFX_OK;
}

int efx_get_timing(efx_ctx* ctx, efx_timing* out)
{
    bind_device(ctx);
    if (!ctx || !out)
        return EFX_ERR_ARG;
    int r = fetch_results(ctx);
    if (r)
        return r;
    efx_timing t{};
    // mean over the efx_decode calls since efx_set_timing(1) (the last kTimingRing of them);
    // fetch_results() has synchronised both streams, so every recorded event is complete
    const uint64_t n_timed = std::min<uint64_t>(ctx->timed_calls, kTimingRing);
    for (uint64_t k = 0; k < n_timed; k++) {
        // a call's stage time = the sum over its groups of streams (they run one after the other on their stream)
        const size_t call = (size_t)((ctx->timed_calls - 1 - k) % kTimingRing);
        const int G = ctx->timing_groups[call];
        for (int g = 0; g < G; g++) {
            const efx_ctx::TimingEvents& te = ctx->timing_ring[call * kMaxGroups + g];
            float a = 0, b = 0, c = 0;
            EFX_HIP(hipEventElapsedTime(&a, te.ev[0], te.ev[1]));
            EFX_HIP(hipEventElapsedTime(&b, te.ev[1], te.ev[2]));
            EFX_HIP(hipEventElapsedTime(&c, te.ev[4], te.ev[3]));
            t.index_ms += a / n_timed;
            t.parse_ms += b / n_timed;
            t.recon_ms += c / n_timed;
        }
        float d = 0;
        EFX_HIP(hipEventElapsedTime(&d, ctx->timing_ring[call * kMaxGroups].ev[0], ctx->timing_ring[call * kMaxGroups + G - 1].ev[3]));
        t.total_ms += d / n_timed;
        if (k == 0) {  // the launch structure of the newest call
            t.groups = t.parse_halves = (uint32_t)G;
            t.recon_launches = ctx->timing_launches[call];
        } else if (t.groups != (uint32_t)G || t.recon_launches != ctx->timing_launches[call])
            t.mixed = 1;
    }
    t.timed_calls = (uint32_t)n_timed;
    for (int i = 0; i < ctx->n_streams; i++)
        t.pictures += ctx->h_pic_count[i];
    t.slices = ctx->h_counters.total_slices;
    t.coefficients = ctx->h_counters.coefficients;
    {
        efx_ctx::Upload& u = ctx->up[ctx->last_upload];
        t.es_bytes = u.es_used;
        t.ts_bytes = u.ts_bytes;
        if (u.ts_input && u.demux_timed)
            EFX_HIP(hipEventElapsedTime(&t.demux_ms, u.ev_demux[0], u.ev_demux[1]));
    }
    *out = t;
    return EFX_OK;
}


// EFX_GUARD's own check (tools/guard_selftest.py): one word written at `offset_bytes` from the start of a device buffer
// (negative: in front of it).  Under the guard-page allocator the first 16-byte unit behind the buffer (mode 1) / any byte in
// front of it (mode 2) faults; without it the write lands in whatever lies there -- never call this outside that test.
int efx_debug_poke(efx_ctx* ctx, void* dptr, size_t bytes, long long offset_bytes)
{
    bind_device(ctx);
    if (!ctx || !dptr)
        return EFX_ERR_ARG;
    (void)bytes;
    char* at = static_cast<char*>(dptr) + offset_bytes;
    hipLaunchKernelGGL(k_fill, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<uint32_t*>(at), 0xDEADBEEFu, (size_t)1);
    EFX_HIP(hipGetLastError());
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->recon_groups_unsynced = 0;  // (the host knows the reconstruction stream idle)
    return EFX_OK;
}

int efx_device_alloc(efx_ctx* ctx, size_t bytes, void** dptr)
{
    bind_device(ctx);
    if (!ctx || !dptr)
        return EFX_ERR_ARG;
    EFX_HIP(dev_alloc(dptr, bytes));
    return EFX_OK;
}

int efx_device_free(efx_ctx* ctx, void* dptr)
{
    bind_device(ctx);
    if (!ctx)
        return EFX_ERR_ARG;
    EFX_HIP(dev_free(dptr));
    return EFX_OK;
}

int efx_memcpy_h2d(efx_ctx* ctx, void* dst_device, const void* src, size_t bytes)
{
    bind_device(ctx);
    if (!ctx || !dst_device || !src)
        return EFX_ERR_ARG;
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->recon_groups_unsynced = 0;  // (the host knows the reconstruction stream idle)
    EFX_HIP(hipMemcpy(dst_device, src, bytes, hipMemcpyHostToDevice));
    return EFX_OK;
}

int efx_memcpy_d2h(efx_ctx* ctx, void* dst, const void* src_device, size_t bytes)
{
    bind_device(ctx);
    if (!ctx || !dst || !src_device)
        return EFX_ERR_ARG;
    EFX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->recon_groups_unsynced = 0;  // (the host knows the reconstruction stream idle)
    EFX_HIP(hipMemcpy(dst, src_device, bytes, hipMemcpyDeviceToHost));
    return EFX_OK;
}

}  // extern "C"
