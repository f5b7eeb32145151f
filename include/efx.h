/* efx.h -- C-ABI of libefx: batched MPEG-1 video decode, composite-video line synthesis and
 * PDM modulation on AMD Instinct MI355X (gfx950).
 *
 * This is the drop-in boundary for the espflix hot path.  The reference (rossumur/espflix) has
 * no FFI layer: its host player talks to a C++ class and a handful of free functions.  Each
 * entry point below names the reference interface it stands in for (file:line under the
 * reference tree); include/efx_player.hpp re-declares that C++ surface (Frame, MpegDecoder,
 * push_video, video_isr, write_pcm_16) on top of this header for batch = 1.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 (EFX_OK) or a negative
 * efx_status; nothing throws; one context per host thread (thread-compatible).  Process-global state: none that a
 * caller can observe -- one mutex-guarded pool of parked HIP streams per device, so that a context created after
 * another was destroyed runs on the same hardware queues (streams are never destroyed).
 * Every entry point makes its context's device current for the calling thread (hipSetDevice) and leaves it so.
 * All work is queued on the context's HIP streams; efx_sync() waits for it.
 */
#ifndef EFX_H
#define EFX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EFX_FRAME_WIDTH 352          /* FB_WIDTH,  src/video.h:30 */
#define EFX_FRAME_HEIGHT 192         /* FB_HEIGHT, src/video.h:31 */
#define EFX_FRAME_STRIDE 528         /* FB_STRIDE, src/video.h:32: 352 luma + 176 chroma bytes */
#define EFX_STRIP_ROWS 16            /* FB_SLICE_HEIGHT, src/video.h:33 */
#define EFX_STRIPS 12                /* FB_SLICES, src/video.h:34 */
#define EFX_STRIP_BYTES 8448         /* 16 x 528 */
#define EFX_FRAME_BYTES 101376       /* 12 x 8448; class Frame, src/video.h:36-44 */

typedef enum efx_status {
    EFX_OK = 0,
    EFX_ERR_ARG = -1,           /* null / out-of-range argument */
    EFX_ERR_DEVICE = -2,        /* HIP runtime error (efx_last_error has the text) */
    EFX_ERR_NO_DEVICE = -3,     /* no gfx950 device / device index out of range */
    EFX_ERR_CAPACITY = -4,      /* more streams / bytes / pictures than the context was sized for */
    EFX_ERR_STATE = -5,         /* call made in the wrong order (e.g. decode before upload) */
    EFX_ERR_STREAM = -6         /* a stream violated a constraint; see efx_stream_status */
} efx_status;

/* per-stream status bits reported by efx_stream_status() */
#define EFX_STREAM_OK 0u
#define EFX_STREAM_BAD_SIZE 1u        /* sequence header is not 352x192 (frame store is fixed) */
#define EFX_STREAM_TRUNCATED 2u       /* more pictures than max_pictures: the rest was ignored */
#define EFX_STREAM_TOO_MANY_UNITS 4u  /* start-code index overflow */
#define EFX_STREAM_BAD_VLC 8u         /* an invalid code ended a slice early, or a slice's codes ran through the next start code */
#define EFX_STREAM_MB_OVERRUN 16u     /* a slice ran past the last macroblock row, or into the macroblocks of the next slice */
#define EFX_STREAM_COEF_OVERRUN 32u   /* a block ran past 64 coefficients (block dropped) */
#define EFX_STREAM_SERIAL_HUNT 64u    /* bits the reference's marker hunt (player.cpp:1360-1363: skip zero bits, DISCARD 24 bits, \
                                         take 8 as the marker) would misread: non-zero bits after a header it ignores (picture \
                                         types other than I / P, player.cpp:710-717), a user_data / extension payload that is not \
                                         made of harmless 4-byte groups (player.cpp:1328-1330), bytes ahead of the first start \
                                         code; also a slice start code ahead of the first picture header (the reference parses \
                                         it with the P books and the constructor's state; dropped here).  The reference then \
                                         acts on phantom markers; this decoder indexes byte-aligned start codes, so its output \
                                         for the stream is NOT the reference's */
#define EFX_STREAM_SLICE_ORDER 128u   /* a picture's slice start codes do not rise strictly in bitstream order (a row coded \
                                         twice, rows out of raster order).  Every slice is parsed by its own lane and stops \
                                         where any other slice of the picture starts; of slices with the same code only the \
                                         last is parsed.  The reference, one serial decoder, lets whatever comes LATER in the \
                                         bitstream overwrite: the same frames when every such slice is complete, not when one \
                                         of them is also damaged or short -- the parity claim does not cover a stream with \
                                         this bit */

/* (bit 256 of the status word is reserved and never set: it belonged to a reconstruction path that was removed, and no later
 * flag takes it) */

typedef enum efx_format {
    EFX_FORMAT_ES = 0, /* raw ISO 11172-2 video elementary stream */
    EFX_FORMAT_TS = 1  /* 188-byte transport packets, video on PID 0x100 (src/player.cpp:381-493);
                          demultiplexed on the device at upload (k_demux), PES PTS kept per picture */
} efx_format;

typedef struct efx_config {
    int device;              /* HIP device ordinal */
    int max_streams;         /* batch capacity */
    int max_pictures;        /* pictures per stream per efx_decode() call */
    int ring_depth;          /* frames kept per stream: 2 = the reference's double buffer
                                (MpegDecoder::_fb, src/player.h:37-40); max_pictures+1 keeps all.  A macroblock no slice of
                                its picture covers (a slice missing from the stream) keeps what its ring slot held: with 2
                                that is the picture two back, as in the reference; with a deeper ring something older --
                                pictures with missing slices match the reference only at ring_depth 2 */
    size_t max_stream_bytes; /* total ES bytes per upload (0 = 16 KiB x pictures x streams) */
    void* hip_stream;        /* hipStream_t to run on, or NULL for a private stream */
} efx_config;

typedef struct efx_ctx efx_ctx;

/* -- lifetime --------------------------------------------------------------------------- */
/* MpegDecoder::MpegDecoder + Frame::init (src/player.cpp:354-369,25-31): allocates the frame
 * rings (zero filled) and all scratch in HBM. */
int efx_create(const efx_config* cfg, efx_ctx** out);
void efx_destroy(efx_ctx* ctx);
const char* efx_last_error(const efx_ctx* ctx);
const char* efx_status_string(int status);

/* -- bitstream in ------------------------------------------------------------------------ */
/* Stands in for the Buffer hand-off MpegDecoder::push_full / pop_empty (src/player.cpp:371-379,
 * src/streamer.h:139-143) for a whole batch: copies n_streams byte ranges (host pointers, the
 * caller keeps ownership) into HBM.  EFX_FORMAT_TS input (188-byte packets, video on PID 0x100)
 * is demultiplexed ON THE DEVICE: MpegDecoder::more/demux/parse_pts (src/player.cpp:294-307,
 * 381-436,459-493) for the whole batch -- adaptation fields and PES headers skipped at the
 * reference's fixed offsets, one zero byte per packet that lost sync, PES PTS values kept for
 * efx_picture_pts.  Like MpegDecoder::more() at end of data (src/player.cpp:456,469-473) each
 * stream is terminated with 00 | 00 00 01 B7 | 00 00 01 B7.  Does NOT reset the frame rings.
 * Three bitstream buffers take turns: the call copies into pinned staging memory and queues the
 * transfer (and k_demux) on a copy stream, then returns; the GPU may still be decoding the previous
 * batches, so ingest and decode of consecutive batches overlap.  efx_decode decodes the batch uploaded
 * last. */
int efx_upload_streams(efx_ctx* ctx, int n_streams, const uint8_t* const* data, const size_t* len, int format);

/* In-place ingest: the reference's contract is "the caller owns the Buffer, the decoder reads it where it lies"
 * (class Buffer, src/streamer.h:139-143; filled by the app in decode_next, src/espflix.cpp:723-737, read by
 * MpegDecoder::more, src/player.cpp:459-493).  Its batch form: an ARENA of page-locked, device-visible host memory
 * (efx_host_alloc, or the caller's own memory made so by efx_host_register) in which the caller lays the streams of
 * a batch out the way the device buffer holds them -- stream i at offsets[i] of efx_stream_layout(), i.e. 16-byte
 * aligned starts with room behind every stream for the end-of-data tail.  efx_upload_streams_inplace takes such a batch
 * (every data[i] == data[0] + offsets[i], all of it inside one arena; anything else: EFX_ERR_ARG): it writes the tails and
 * the zero fill INTO the gaps the layout leaves (the only bytes of the arena the library ever writes -- hence the
 * non-const pointers), and the H2D transfer reads the caller's memory directly -- no staging copy, one transfer.  The
 * caller keeps ownership throughout and must leave the batch's bytes alone until efx_upload_done() says the transfer no
 * longer reads them.  In-place ingest is asked for BY NAME: efx_upload_streams() never writes through its `const` data
 * pointers and always takes the staged path, wherever the streams lie (round 5 inferred it from the pointer pattern). */
int efx_upload_streams_inplace(efx_ctx* ctx, int n_streams, uint8_t* const* data, const size_t* len, int format);
int efx_host_alloc(efx_ctx* ctx, size_t bytes, void** host_ptr);
int efx_host_free(efx_ctx* ctx, void* host_ptr);
int efx_host_register(efx_ctx* ctx, void* host_ptr, size_t bytes);
int efx_host_unregister(efx_ctx* ctx, void* host_ptr);
/* offsets[0 .. n_streams]: where stream i of the given lengths starts inside an arena (offsets[0] = 0), offsets[n_streams] =
 * bytes the batch occupies.  Host only. */
int efx_stream_layout(int n_streams, const size_t* len, size_t* offsets);
/* 1: the most recent efx_upload_streams[_inplace] no longer reads caller memory (always so for the staged path once the
 * call has returned); 0: its transfer is still in flight; negative: error. */
int efx_upload_done(efx_ctx* ctx);
/* The elementary stream the decoder sees for `stream` (what MpegDecoder::more() feeds the bit
 * reader, src/player.cpp:459-493), without the end-of-data tail: *es_len receives its length,
 * up to `cap` bytes are copied to dst (dst may be NULL when cap is 0). */
int efx_download_es(efx_ctx* ctx, int stream, uint8_t* dst, size_t cap, size_t* es_len);

/* A freshly constructed decoder: Frame::init (src/player.cpp:25-31) zeroes the frame rings, and the
 * per-stream state that otherwise survives from one efx_decode to the next -- the frame index
 * (_fb_index), "a picture has latched a PTS" (_last_pts != -1) and the newest PES PTS (_pts) -- goes
 * back to the constructor's values (src/player.cpp:354-361).  (MpegDecoder::reset(), 439-453, keeps
 * _fb_index and _pts across plays; call efx_reset only where a new MpegDecoder would be made.) */
int efx_reset(efx_ctx* ctx);
/* MpegDecoder::reset() between two plays on the same decoder (src/player.cpp:439-453): _last_pts = -1,
 * i.e. the next picture headers neither push nor swap until one latches a PES PTS again; the frame index,
 * the newest PES PTS and the frame contents survive.  Synchronous. */
int efx_play_reset(efx_ctx* ctx);
/* The per-stream decoder state (valid for what has been queued so far; synchronises): the frame index
 * (MpegDecoder::_fb_index: the next picture is reconstructed into slot frame_index % ring_depth if no buffer
 * swap precedes it, frame_index + 1 otherwise, from the slot before), whether a picture has latched a PTS
 * since the last (play) reset, and the newest PES PTS seen (-1: none).  Any pointer may be NULL. */
int efx_stream_state(efx_ctx* ctx, int stream, uint32_t* frame_index, int* pts_seen, int64_t* newest_pts);
/* Frame::erase (src/player.cpp:48-52): fill every ring frame with 0x30. */
int efx_erase_frames(efx_ctx* ctx);

/* -- decode ------------------------------------------------------------------------------ */
/* MpegDecoder::run() over the uploaded batch (src/player.cpp:1355-1367 and everything below
 * it: marker/sequence/gop/picture/slice/block/idct/mocomp).  Asynchronous.  The decoder keeps
 * going from call to call like the reference fed Buffer after Buffer: every stream carries its
 * frame index and its "a PTS has been latched" state (flush_picture, src/player.cpp:692-702).
 * With p the frame index before the call (1 after efx_reset) picture i of the call is
 * reconstructed into ring slot (p + s(i)) % ring_depth from slot (p + s(i) - 1) % ring_depth,
 * s(i) = i + 1 once a picture has latched a PES PTS, else max(0, i - f) with f the first picture of
 * the call that does: the reference does not swap its two buffers before the first PTS.  Elementary-
 * stream input counts every picture as carrying one.  ring_depth 2 is the reference's pair.
 * Streams are independent; a large batch decoded while the GPU is otherwise idle runs as several groups of
 * streams one after the other (the call pipelines inside itself, efx_timing::groups), back-to-back calls as one
 * group each -- the results do not depend on it. */
int efx_decode(efx_ctx* ctx);
/* The same, starting at picture `first_picture` of every uploaded stream (earlier pictures are walked
 * for their header state only): a stream with more than max_pictures pictures (EFX_STREAM_TRUNCATED)
 * is decoded by efx_decode_from(ctx, 0), (ctx, max_pictures), (ctx, 2 * max_pictures) ... */
int efx_decode_from(efx_ctx* ctx, int first_picture);
/* The same for at most n_pictures (1 ... max_pictures) pictures per stream: a caller that knows its batch holds few
 * pictures (the streaming adapter decoding a real-time play picture by picture, efx_player.hpp) pays for that many
 * reconstruction launches, not for max_pictures of them; streams with more are flagged EFX_STREAM_TRUNCATED as above. */
int efx_decode_range(efx_ctx* ctx, int first_picture, int n_pictures);
int efx_sync(efx_ctx* ctx);

/* number of pictures found in a stream by the last efx_decode (valid after efx_sync) */
int efx_picture_count(efx_ctx* ctx, int stream, int* n_pictures);
/* OR of EFX_STREAM_* bits for a stream (valid after efx_sync) */
int efx_stream_status(efx_ctx* ctx, int stream, uint32_t* bits);
/* PES PTS latched for picture `picture` (flush_picture, src/player.cpp:692-702; -1 when no PES
 * with a PTS preceded it); valid after efx_decode for TS input; ES input yields the picture index. */
int efx_picture_pts(efx_ctx* ctx, int stream, int picture, int64_t* pts);

/* -- frames out (the push_video up-call surface, src/video.h:49) ------------------------- */
/* Ring slot that holds picture `picture` of stream `stream` after the last efx_decode (valid after
 * efx_sync; see efx_decode for the arithmetic). */
int efx_stream_picture_slot(efx_ctx* ctx, int stream, int picture, int* slot);
/* The same for stream 0 as a return value (negative = efx_status): every stream of a batch shares it as
 * long as all of them decoded the same number of pictures in every call since efx_reset. */
int efx_picture_slot(efx_ctx* ctx, int picture);
/* Device pointer to a ring frame in the reference strip layout (12 x 8448 bytes). */
int efx_frame_device_ptr(efx_ctx* ctx, int stream, int slot, void** dptr);
/* Copy one ring frame to host memory (EFX_FRAME_BYTES). Synchronous. */
int efx_download_frame(efx_ctx* ctx, int stream, int slot, uint8_t* dst);
/* FNV-1a-64 of ring frames [first_stream, first_stream+n) x [0, ring_depth), computed on the
 * device, written to host memory as n x ring_depth uint64.  Synchronous. */
int efx_frame_hashes(efx_ctx* ctx, int first_stream, int n, uint64_t* out);
/* Overwrite one ring frame from host memory (tests, poster upload). Synchronous. */
int efx_upload_frame(efx_ctx* ctx, int stream, int slot, const uint8_t* src);

/* -- pictures out in standard pixel formats (k_export) ----------------------------------- */
/* The ring frames above keep the reference's strip layout, which nothing outside this library reads.  efx_export_frames
 * turns ring frames of a contiguous range of streams into one image per stream, on the device, in one launch:
 *
 *   EFX_PIX_I420   Y 192 x 352, then U (Cb) 96 x 176, then V (Cr) 96 x 176, planar, rows packed: 101 376 bytes
 *   EFX_PIX_RGB24  192 x 352 x 3 (HWC), R G B interleaved: 202 752 bytes
 *   EFX_PIX_RGBP   3 x 192 x 352 (CHW), the planes R, G, B (torchvision's layout): 202 752 bytes
 *
 * Plane mapping.  Strip rows 0-7 of the strip layout carry Cb (U) and rows 8-15 Cr (V).  The reference calls rows 0-7
 * "cr" (Frame::get_cr, src/player.cpp:38-46), but they hold MPEG-1 block 4 (cr_addr, player.cpp:830-831,1129-1130),
 * which its decoder predicts from cr_dc (player.cpp:1037,1060): block 4 is Cb in ISO 11172-2 2.4.3.7, and the
 * reference's own display path reads those rows as u_ptr (src/video.cpp:695-696).  I420's U plane is rows 0-7.
 *
 * RGB is exact integer arithmetic (espflix_amd/csrc/export_px.h), bit-reproducible anywhere:
 *   chroma at luma resolution, for luma column x, row y:
 *     EFX_CHROMA_NEAREST   C[y >> 1][x >> 1]
 *     EFX_CHROMA_BILINEAR  MPEG-1 siting (a chroma sample centred between its 2 x 2 luma samples):
 *                          cx0 = x >> 1, cx1 = clamp(cx0 + (x & 1 ? 1 : -1), 0, 175), likewise cy0 / cy1 in 0 .. 95,
 *                          c = (9 C[cy0][cx0] + 3 C[cy0][cx1] + 3 C[cy1][cx0] + C[cy1][cx1] + 8) >> 4
 *   matrix, u = U - 128, v = V - 128, t = cy (Y - y0) + 128, >> arithmetic, results clamped to 0 .. 255:
 *     R = (t + rv v) >> 8,  G = (t + gu u + gv v) >> 8,  B = (t + bu u) >> 8
 *     BT.601 studio swing (full_range 0, what MPEG-1 carries): cy 298, y0 16, rv 409, gu -100, gv -208, bu 516
 *     BT.601 full range   (full_range 1):                      cy 256, y0 0,  rv 359, gu -88,  gv -183, bu 454 */
typedef enum efx_pixel_format { EFX_PIX_I420 = 0, EFX_PIX_RGB24 = 1, EFX_PIX_RGBP = 2 } efx_pixel_format;
#define EFX_CHROMA_NEAREST 0
#define EFX_CHROMA_BILINEAR 1
typedef struct efx_export_opts {
    int first_stream, n_streams;
    int slot;          /* >= 0: this ring slot of every selected stream; -1: use `picture` */
    int picture;       /* slot < 0: picture `picture` of the most recent efx_decode* of each stream */
    int format;        /* efx_pixel_format */
    int chroma;        /* EFX_CHROMA_*; ignored for I420 */
    int full_range;    /* 0 = BT.601 studio swing (MPEG-1), 1 = full range */
    size_t dst_stride; /* bytes from one stream's image to the next; 0 = efx_export_bytes(format) */
} efx_export_opts;
/* bytes of one image in `format`; 0 for an unknown format.  Host only. */
size_t efx_export_bytes(int format);
/* Stream first_stream + i goes to dst_device + i * dst_stride (device memory, 16-byte aligned; stride a multiple of 16
 * and at least the image; the bytes between images are not written).  Asynchronous, on the context's stream: queued
 * behind the decodes before it, it reads what they reconstruct.  Picture mode (slot = -1) needs no synchronisation: the
 * ring slot of each stream (efx_stream_picture_slot's arithmetic) is read on the device from the record the most
 * recent decode left -- streams of one batch may sit in different slots.
 * EFX_ERR_ARG: dst_device NULL or not 16-byte aligned, unknown format or chroma mode, a bad dst_stride, the stream range
 * outside max_streams, slot >= ring_depth or < -1, picture outside [0, max_pictures).  EFX_ERR_STATE (picture mode):
 * no decode yet, or the stream range beyond the stream count of the most recent decode. */
int efx_export_frames(efx_ctx* ctx, const efx_export_opts* opts, void* dst_device);

/* -- pictures in: any size and pixel format to the encoder's 352 x 192 I420 (k_import) ----- */
/* efx_encode reads 352 x 192 I420 pictures; nobody's source material has that size.  efx_import_frames is the inverse of
 * efx_export_frames: it crops I420, RGB24 (HWC) or RGBP (CHW) pictures of 2 x 2 to 4096 x 4096 pixels, scales the crop
 * into a rectangle of the 352 x 192 frame and converts RGB to YCbCr, on the device, for n_images pictures at once -- the
 * first step of the reference indexer's ffmpeg line (indexer/indexer.cpp:299-309: crop=992:546:144:0 ... -s 352x192).
 *
 * Output.  Image k is read at src + k * src_stride and written at dst + k * dst_stride in the layout efx_encode reads:
 * Y 192 x 352, Cb 96 x 176, Cr 96 x 176.  With dst_stride 101376 and n_images = n_streams x n_pictures the output is an
 * efx_encode source with packed src_stride.  Pixels outside the destination rectangle are black: Y 16 (Y 0 for an RGB
 * source with full_range = 1), Cb = Cr = 128.  The bytes between output images are not written.
 *
 * The arithmetic (espflix_amd/csrc/import_px.h) is an integer function of the source bytes, bit-reproducible anywhere.
 *   Planes.  An I420 source brings three byte planes: the crop, and the crop halved for Cb and Cr.  An RGB source is
 *   converted pixel by pixel, at source resolution, into three planes of the crop's size.  Luma goes from crop_w x crop_h
 *   to dst_w x dst_h, each chroma plane from its extent to dst_w / 2 x dst_h / 2.  The centre-aligned mapping below puts a
 *   chroma sample in the middle of its 2 x 2 luma samples, which is MPEG-1's siting.
 *   RGB -> YCbCr, BT.601, >> arithmetic, results clamped to 0 .. 255:
 *     studio swing (full_range 0, what MPEG-1 carries)      full range (full_range 1)
 *     Y  = (( 66 R + 129 G +  25 B + 128) >> 8) + 16        Y  =  ( 77 R + 150 G +  29 B + 128) >> 8
 *     Cb = ((-38 R -  74 G + 112 B + 128) >> 8) + 128       Cb = ((-43 R -  85 G + 128 B + 128) >> 8) + 128
 *     Cr = ((112 R -  94 G -  18 B + 128) >> 8) + 128       Cr = ((128 R - 107 G -  21 B + 128) >> 8) + 128
 *   Taps of one axis, source extent S, destination extent D, M = max(S, D) -- a triangle filter widened by the
 *   down-scaling ratio: destination index d takes source index s with the raw weight
 *     u(s) = max(0, 2M - |(2s + 1) D - (2d + 1) S|)
 *   over every s in [0, S) with u(s) > 0 (samples beyond the edge are dropped, not replicated), with the coefficients
 *   k(s) = floor(u(s) 16384 / sum of u); what is missing to 16384 goes to the tap with the largest u, the first such tap on
 *   a tie.  S == D gives the single tap s = d: a same-size import is a copy.
 *   Two passes, horizontal first:  h = (sum of k_x p + 32) >> 6  (16 bits),  out = (sum of k_y h + 2^21) >> 22.
 *
 * Memory contract.  For image k the kernels read only bytes in [src + k * src_stride, src + k * src_stride +
 * efx_import_src_bytes() rounded up to 16) and write only the 101376 bytes of output image k.  src_device and dst_device
 * are 16-byte aligned and the strides are multiples of 16; rows inside an image start anywhere (333 x 77 RGB24), they are
 * fetched in 16-byte pieces aligned down inside that interval. */
typedef struct efx_import_opts {
    int n_images;                       /* >= 1 */
    int format;                         /* efx_pixel_format of the SOURCE: I420, RGB24 (HWC), RGBP (CHW) */
    int width, height;                  /* source picture, 2 .. 4096 each; I420: both even */
    int crop_x, crop_y, crop_w, crop_h; /* source rectangle that is used; crop_w == 0: the whole picture; I420: all even */
    int dst_x, dst_y, dst_w, dst_h;     /* rectangle of the 352 x 192 output that receives it; dst_w == 0: 0, 0, 352, 192;
                                           all even, dst_w, dst_h >= 16, inside the frame */
    int full_range;                     /* RGB sources: 0 = write BT.601 studio swing (what MPEG-1 carries), 1 = full range;
                                           ignored for I420 */
    size_t src_stride;                  /* bytes from one source image to the next; 0 = efx_import_src_bytes() rounded up to 16 */
    size_t dst_stride;                  /* bytes from one output image to the next; 0 = 101376 */
} efx_import_opts;
/* bytes of one source image; 0 for an unknown format, a width or height outside 2 .. 4096, an odd I420 size.  Host only. */
size_t efx_import_src_bytes(int format, int width, int height);
/* Asynchronous on the context's stream: no host synchronisation, two launches whatever n_images is (the tap table is
 * computed on the device in stream order, so calls with different geometry may be queued back to back), and no decoder,
 * encoder or SBC state is touched.
 * EFX_ERR_ARG: a NULL or misaligned (16 bytes) pointer, n_images < 1, an unknown format, width or height out of range, an
 * odd value where an even one is required, a crop outside the source, a destination rectangle below 16 x 16 or outside
 * the frame, a stride that is too small or not a multiple of 16, or a down-scaling ratio above 32: crop_w > 32 dst_w or
 * crop_h > 32 dst_h (a window then has at most 65 taps; 129 for the chroma of an RGB source, which goes from the full
 * crop to half the rectangle). */
int efx_import_frames(efx_ctx* ctx, const efx_import_opts* opts, const void* src_device, uint8_t* dst_device);

/* -- black borders: where the crop rectangle comes from (k_cropdetect) --------------------- */
/* Source films arrive letterboxed or pillarboxed, and efx_import_frames takes its crop from the caller.  The reference
 * indexer finds it with a second ffmpeg run (indexer/indexer.cpp:298-300: `-vf cropdetect=24:16:0`, next to the
 * `crop=992:546:144:0 ... -s 352x192` line it feeds).  efx_detect_crop is that step on the device, for a batch: it reads
 * the luma of n_streams x images_per_stream source pictures (the formats, sizes and layout of efx_import_frames) and
 * leaves one rectangle per stream.  The definition is this library's own -- the idea of cropdetect=limit:round:0, stated
 * exactly -- and an integer function of the source bytes (espflix_amd/csrc/crop_px.h), bit-reproducible anywhere.
 *
 *   Luma.  L(x, y) of a W x H image: the Y plane of an I420 source (its chroma planes are never read); for RGB24 / RGBP
 *   the Y that efx_import_frames would write, Y of the matrix above for full_range (studio swing: black is 16, so ffmpeg's
 *   default limit 24 means what it means there).
 *   Sums.  R[y] = sum over x of L(x, y), C[x] = sum over y of L(x, y), exact in uint32 (at most 4096 x 255).
 *   Classification.  Row y is picture when R[y] > limit x W, column x when C[x] > limit x H; equality is black.
 *   Per image.  An image with at least one picture row and one picture column contributes top / bottom, its first and
 *   last picture row, and left / right, its first and last picture column.  Any other image (all black: a fade inside a
 *   title) contributes nothing -- it neither widens nor resets anything.
 *   Per stream.  A stream is images_per_stream consecutive images (image k belongs to stream k / images_per_stream).
 *   Over its contributing images x1 = min left, x2 = max right, y1 = min top, y2 = max bottom, all inclusive.
 *   Rounding, per axis, bounds a .. b inclusive, r = round:  a' = a + (a & 1);  avail = b + 1 - a';  avail < 2: the axis
 *   fails;  len = avail - avail mod r when avail >= r, else avail & ~1;  pos = a' + (((avail - len) >> 1) & ~1).
 *   pos and len are even, pos >= a, pos + len <= b + 1: the rectangle lies inside the detected picture, centred to within
 *   one even step.
 *   Record.  Eight int32 per stream: x, y, w, h, x1, y1, x2, y2.  No image contributed: x1 = W, y1 = H, x2 = y2 = -1.
 *   No image contributed or an axis failed: x, y, w, h = 0, 0, W, H, the whole picture, which efx_import_frames accepts
 *   as a crop for every format.
 *
 * Memory contract (efx_import_frames').  For image k the kernels read only bytes in [src + k * src_stride, src + k *
 * src_stride + efx_import_src_bytes() rounded up to 16), for I420 only the first W x H of them rounded up to 16, in
 * 16-byte pieces aligned down inside that interval, each luma byte (RGB: each component) once.  They write the n_streams
 * records and, when sums_device is given, for image k R[0 .. H) followed by C[0 .. W) at sums_device + k * sums_stride;
 * the elements between images are not written.  With sums_device NULL the sums live in scratch of the context, allocated
 * at the first such call, regrown when a later call needs more (such a call may wait for the stream) and freed by
 * efx_destroy.
 *
 * Out of scope: handing the rectangle to efx_import_frames on the device (its geometry is a host argument: read the
 * 32-byte record back), ffmpeg's reset window and its motion-vector mode, and byte compatibility with ffmpeg's rounding
 * (which does not promise even offsets). */
typedef struct efx_crop_opts {
    int n_streams;          /* >= 1; not tied to max_streams (like efx_import_frames' n_images) */
    int images_per_stream;  /* >= 1; image k belongs to stream k / images_per_stream; n_streams x images_per_stream < 2^31 */
    int format;             /* efx_pixel_format of the source */
    int width, height;      /* as efx_import_frames: 2 .. 4096, I420 even */
    int full_range;         /* RGB sources: which luma (see above); ignored for I420 */
    int limit;              /* 0 .. 255; ffmpeg's default: 24 */
    int round;              /* even, 2 .. 64; ffmpeg's default: 16 */
    size_t src_stride;      /* bytes between images; 0 = efx_import_src_bytes() rounded up to 16; multiple of 16 */
    size_t sums_stride;     /* uint32 elements between images in sums_device; 0 = (height + width) rounded up to 4 */
} efx_crop_opts;
typedef struct efx_crop_rect { int32_t x, y, w, h, x1, y1, x2, y2; } efx_crop_rect;
/* Asynchronous on the context's stream: no host synchronisation, three launches whatever the counts are (the column
 * sums to zero, the sums, the rectangles), and no decoder, encoder, SBC or import state is touched.
 * EFX_ERR_ARG: a NULL or misaligned (16 bytes) src_device or rects_device, a misaligned sums_device, n_streams or
 * images_per_stream < 1 or their product above 2^31 - 1, an unknown format, width or height out of range (I420: odd),
 * limit outside 0 .. 255, round odd or outside 2 .. 64, a src_stride that is too small or not a multiple of 16, a
 * sums_stride below width + height or not a multiple of 4. */
int efx_detect_crop(efx_ctx* ctx, const efx_crop_opts* opts, const void* src_device, efx_crop_rect* rects_device,
                    uint32_t* sums_device /* may be NULL */);

/* -- surfaces: NV12, P010 and pitched 4:2:0 sources as decoders write them (k_import, k_cropdetect) -- */
/* No video decoder hands out packed 8-bit I420.  Hardware decoders write NV12, or P010 for 10-bit sources: a Y plane and
 * a plane of interleaved Cb Cr pairs, with a row pitch, often padded plane heights and therefore their own plane
 * offsets.  Software decoders hand out pitched planar 4:2:0, for 10 and 12 bit in 16-bit words with the value in the low
 * bits (yuv420p10le).  efx_import_surfaces and efx_detect_crop_surfaces read such pictures where they lie, each source
 * byte once, so nobody has to repack a 1080p or 2160p picture first.
 *
 * A surface describes one 4:2:0 YCbCr image in device memory by plane offsets and pitches.
 *
 *   Sample reduction.  A byte is taken as it is.  A word w (uint16, little endian) becomes
 *     min(255, (w + (1 << (shift - 1))) >> shift).
 *   shift = 8 reads P010, P012 and P016, which keep the value in the most significant bits (whatever sits in the low
 *   bits takes part in the rounding); shift = 2 reads yuv420p10le, shift = 4 yuv420p12le.  A word above the nominal range
 *   saturates.  The reduction happens once per sample, before anything else: the filter, its tap table and its
 *   accumulators are those of the 8-bit path (DESIGN.md section 8 says why).
 *   Canonical image.  The packed I420 picture of width x height with Y[y][x] = the reduction of the Y plane's sample
 *   (y, x), Cb[y][x] and Cr[y][x] = the reductions of the chroma samples (y, x); for the semi-planar layouts these are
 *   elements 2x and 2x + 1 of the pair row, swapped with swap_uv.
 *   Meaning.  Bit for bit, efx_import_surfaces and efx_detect_crop_surfaces produce what efx_import_frames and
 *   efx_detect_crop produce for the canonical images.  The opts are read as for that canonical image: format must be
 *   EFX_PIX_I420, width and height must equal the surface's; crop, destination rectangle, limit, round, sums_stride and
 *   the output layouts are unchanged; src_stride is the number of bytes between images, 0 = `bytes` rounded up to 16, a
 *   multiple of 16 and at least `bytes`; full_range is ignored.
 *   Fields come free.  The top or bottom field of an interlaced surface is the same surface with every pitch doubled,
 *   height halved, and each offset advanced by one pitch for the bottom field (height must then be a multiple of 4).
 *   That reads one field as a picture of its own; making progressive pictures of an interlaced source is
 *   efx_deinterlace's work ("interlaced sources" below).  Field-sited chroma resampling is out of scope.
 *
 * Memory contract (an extension of efx_import_frames').  For image k the kernels read only bytes in [src + k *
 * src_stride, src + k * src_stride + bytes rounded up to 16), in 16-byte pieces aligned down inside that interval, and
 * only the rows the call needs: the crop's rows for the import, the luma plane's rows for crop detection (chroma is never
 * read for it).  Bytes in pitch padding, between planes and between images are fetched at most as part of such a piece
 * and never influence a result.  All offsets are computed in 64 bits. */
#define EFX_SURF_PLANAR8  0   /* three planes of bytes: Y, Cb, Cr */
#define EFX_SURF_SEMI8    1   /* Y bytes; one plane of (Cb, Cr) byte pairs at half resolution: NV12 */
#define EFX_SURF_PLANAR16 2   /* three planes of 16-bit little-endian words */
#define EFX_SURF_SEMI16   3   /* Y words; one plane of (Cb, Cr) word pairs: P010 / P012 / P016 */
typedef struct efx_surface {
    int layout;        /* EFX_SURF_* */
    int shift;         /* 16-bit layouts: 1 .. 8, see above; byte layouts: 0 */
    int swap_uv;       /* semi-planar: 1 = the pairs are (Cr, Cb): NV21; planar: must be 0 (swap offset[1] / offset[2] for YV12) */
    int width, height; /* even, 2 .. 4096 */
    size_t offset[3];  /* bytes from the image's start to row 0 of Y, of Cb (or of the pair plane), of Cr (semi-planar: ignored) */
    size_t pitch[3];   /* bytes from a row of that plane to the next */
    size_t bytes;      /* extent of one image: every row of every plane ends at or before it */
} efx_surface;
/* Asynchronous on the context's stream like their counterparts: no host synchronisation, two launches per
 * efx_import_surfaces call and three per efx_detect_crop_surfaces call whatever the counts are (the tap table is computed
 * on the device in stream order, so queued calls with different surfaces keep their geometry), and no decoder, encoder,
 * SBC or other state is touched.
 * EFX_ERR_ARG, beyond the cases of efx_import_frames and efx_detect_crop: an unknown layout, a shift outside its range
 * for the layout, swap_uv on a planar layout, an odd or out-of-range size, a 16-bit layout with an odd offset or pitch, a
 * pitch below the plane's row bytes (width x B for Y and for a pair plane, width / 2 x B for a planar chroma plane, B = 1
 * or 2) or above 2^20, a plane row ending beyond `bytes`, `bytes` of 2^40 or more, opts->format, width or height
 * disagreeing with the surface. */
int efx_import_surfaces(efx_ctx* ctx, const efx_surface* surface, const efx_import_opts* opts, const void* src_device,
                        uint8_t* dst_device);
int efx_detect_crop_surfaces(efx_ctx* ctx, const efx_surface* surface, const efx_crop_opts* opts, const void* src_device,
                             efx_crop_rect* rects_device, uint32_t* sums_device /* may be NULL */);
typedef enum efx_surface_kind { EFX_KIND_I420, EFX_KIND_YV12, EFX_KIND_NV12, EFX_KIND_NV21, EFX_KIND_P010, EFX_KIND_P012,
                                EFX_KIND_P016, EFX_KIND_I010, EFX_KIND_I012, EFX_KIND_I016 } efx_surface_kind;
/* The conventional layout.  Y at 0 with pitch P (0 = packed row), R = plane_rows (0 = height; even, >= height).  The pair
 * plane sits at P x R with pitch P.  Planar chroma: the first chroma plane at P x R with pitch P / 2, the second at
 * P x R + (P / 2)(R / 2); YV12 stores Cr first.  bytes = P x R x 3 / 2.  Returns bytes, 0 for arguments the calls would
 * reject (planar: P not a multiple of 2 B).  Host only. */
size_t efx_surface_layout(int kind, int width, int height, size_t pitch, int plane_rows, efx_surface* out);

/* -- interlaced sources: fields to progressive pictures (k_deint) --------------------------- */
/* DVD material (480i / 576i) and broadcast or camcorder 1080i carry two fields per frame, taken at two moments.  Scaling
 * the woven frame blends those moments into ghosts wherever something moves; importing one field throws half of the
 * vertical detail of every still area away.  efx_deinterlace completes each field to a full picture at the source's
 * size, before anything is scaled: the step the reference indexer leaves to ffmpeg's yadif.  The rule is yadif's
 * spatial-temporal rule with its spatial interlacing check, stated here as this library's own, with its own edge rule:
 * an integer function of the source bytes (espflix_amd/csrc/deint_px.h), bit-reproducible anywhere.  Byte compatibility
 * with ffmpeg at picture edges is not promised.
 *
 * The rule is applied to each of the three planes of the canonical image of a surface ("surfaces" above), each with its
 * own w, h (luma: width x height; Cb, Cr: half of each).
 *
 *   Setting.  A stream is a run of frames F[0 .. N-1].  first_field says which field of a frame is earlier in time:
 *   EFX_FIELD_TOP (tff) or EFX_FIELD_BOTTOM (bff).  Output (t, i) is frame t's first (i = 0) or second (i = 1) field
 *   completed to a full picture.  Its kept parity p is the parity of that field; the top field is the even lines, p = 0.
 *   Lines y = p (mod 2) are copied from F[t] unchanged.  Lines y = 1 - p (mod 2) are made as below, from
 *
 *                                                   i = 0      i = 1
 *     cur                                           F[t]       F[t]
 *     prev                                          F[t-1]     F[t-1]
 *     next                                          F[t+1]     F[t+1]
 *     B  (the opposite-parity field just before)    F[t-1]     F[t]
 *     A  (the opposite-parity field just after)     F[t]       F[t+1]
 *
 *   A neighbour that does not exist (t - 1 < 0, t + 1 >= N) is replaced by F[t] itself.
 *   Index rule.  A row index r outside 0 .. h - 1 is replaced by r + 2 (r < 0) or r - 2 (r >= h); only -2 .. h + 1 occur.
 *   A column index is clamped to 0 .. w - 1.
 *   One missing sample at (x, y).  All values are int, >> is arithmetic.
 *     c = cur[y-1][x]   e = cur[y+1][x]
 *     d  = (B[y][x] + A[y][x]) >> 1
 *     t0 = |B[y][x] - A[y][x]| >> 1
 *     t1 = (|prev[y-1][x] - c| + |prev[y+1][x] - e|) >> 1
 *     t2 = (|next[y-1][x] - c| + |next[y+1][x] - e|) >> 1
 *     diff = max(t0, t1, t2)
 *     score(j) = sum over k in {-1, 0, 1} of |cur[y-1][x+k+j] - cur[y+1][x+k-j]|
 *     pred(j)  = (cur[y-1][x+j] + cur[y+1][x-j]) >> 1
 *     best = score(0) - 1;  sp = pred(0)
 *     for s in (-1, +1), in this order:
 *         if score(s) < best:  best = score(s);  sp = pred(s)
 *             if score(2s) < best:  best = score(2s);  sp = pred(2s)        (tried only when s improved)
 *     b = (B[y-2][x] + A[y-2][x]) >> 1;  f = (B[y+2][x] + A[y+2][x]) >> 1
 *     mx = max(d - e, d - c, min(b - c, f - e))
 *     mn = min(d - e, d - c, max(b - c, f - e))
 *     diff = max(diff, mn, -mx)
 *     out = min(max(sp, d - diff), d + diff)                                (lies in 0 .. 255 by construction)
 *
 *   Layout.  Source image i * n_frames + j is stream i's frame j, at src_device + (i * n_frames + j) * src_stride.  Outputs
 *   are packed I420 pictures of the surface's width x height, so efx_import_frames and efx_detect_crop read them as they
 *   are; with n_out = efx_deinterlace_count(), output m of stream i lies at dst_device + (i * n_out + m) * dst_stride.
 *   EFX_DEINT_FRAME writes output (t, 0) per frame (the source's frame rate), EFX_DEINT_FIELD (t, 0) then (t, 1) (its field
 *   rate: 576i25 becomes 50 pictures a second, picture_rate code 6; 480i 59.94, code 7).
 *   Pieces.  lead / tail = 1 make the first / last offered frame context only: it is read as a neighbour and has no
 *   output.  A title goes through piece by piece with one frame of overlap -- the first piece with lead = 0, tail = 1,
 *   middle pieces with 1, 1, the last with 1, 0 -- and the concatenated outputs equal those of one long call.  With
 *   lead = 0 the first frame's missing prev is the frame itself (the title's start); tail = 0 does the same at the end.
 *   Streams never see each other's frames.
 *   Surfaces.  EFX_SURF_PLANAR8 (YV12 by swapped offsets) and EFX_SURF_SEMI8 (NV12 / NV21, de-interleaved on load); width
 *   even, 2 .. 4096; height a multiple of 4, 8 .. 4096, so that chroma has whole field pairs.
 *
 * Memory contract.  For source image k the kernel reads only bytes in [src + k * src_stride, src + k * src_stride + bytes
 * rounded up to 16), 16 bytes at a time wherever a plane's rows begin, and only rows of the three planes; bytes in pitch
 * padding, between planes and between images are fetched at most as part of such an access and never influence a result.
 * It writes only the width x height x 3 / 2 bytes of each output image.  All offsets are computed in 64 bits.  The source
 * and destination regions must not overlap.
 *
 * Out of scope: the 16-bit layouts, 4:2:2, bwdif's longer filter, motion-compensated deinterlacing, inverse telecine
 * (efx_detelecine: "telecined sources" below), per-frame parity flags, field-sited chroma resampling, efx_multi_*.
 * Whether a source is interlaced at all, and in which field order: efx_detect_scan ("scan type" below). */
#define EFX_FIELD_TOP    0   /* the top field (even lines) is the earlier one: tff */
#define EFX_FIELD_BOTTOM 1   /* bff */
#define EFX_DEINT_FRAME  0   /* one output per frame: (t, 0) */
#define EFX_DEINT_FIELD  1   /* two outputs per frame: (t, 0) then (t, 1) */
typedef struct efx_deint_opts {
    int n_streams;        /* >= 1 */
    int n_frames;         /* frames per stream offered by this call, >= 1 */
    int first_field;      /* EFX_FIELD_TOP / EFX_FIELD_BOTTOM */
    int mode;             /* EFX_DEINT_FRAME / EFX_DEINT_FIELD */
    int lead, tail;       /* 0 / 1: the first / last offered frame is context only (no output for it) */
    size_t src_stride;    /* bytes between source images; 0 = the surface's bytes rounded up to 16; multiple of 16 */
    size_t dst_stride;    /* bytes between output images; 0 = efx_import_src_bytes(I420, w, h) rounded up to 16; multiple of 16 */
} efx_deint_opts;
/* Asynchronous on the context's stream: no host synchronisation, one launch whatever the counts are, and no decoder,
 * encoder, SBC, import or other state is touched.
 * EFX_ERR_ARG: everything efx_import_surfaces rejects about a surface, a 16-bit layout, a height that is not a multiple
 * of 4 or below 8, n_streams < 1, lead or tail other than 0 / 1, lead + tail >= n_frames, an unknown mode or first_field,
 * more than 2^31 - 1 images in or out, a NULL or misaligned (16 bytes) pointer, a stride that is too small or not a
 * multiple of 16.  A refused call writes nothing. */
int efx_deinterlace(efx_ctx* ctx, const efx_surface* surface, const efx_deint_opts* opts, const void* src_device,
                    uint8_t* dst_device);
/* outputs per stream of such a call; -1 for arguments it rejects.  Host only. */
int efx_deinterlace_count(int n_frames, int lead, int tail, int mode);

/* -- telecined sources: fields back to film frames (k_telecine) ----------------------------- */
/* Most NTSC DVD film material is hard-telecined: four film frames are spread over ten fields (3:2 pulldown), so two of
 * every five video frames weave fields of two different film frames.  efx_deinterlace is the wrong tool for such a
 * title: it interpolates lines whose true partner field sits one field slot away, leaves one repeated picture in every
 * five, and hands the encoder 29.97 pictures a second where the film has 23.976.  efx_detelecine finds each field's
 * partner, weaves the film frames back together and drops the repeated one: the step the reference indexer leaves to
 * ffmpeg's fieldmatch,decimate.  MPEG-1 codes 23.976 Hz as picture_rate code 1 (efx_encode_set_picture_rate).  The rule
 * is this library's own exact integer rule (espflix_amd/csrc/telecine_px.h), bit-reproducible anywhere.  Byte
 * compatibility with ffmpeg is not promised.
 *
 *   Setting.  A stream is a run of frames F[0 .. N-1] of a surface ("surfaces" above).  first_field is EFX_FIELD_TOP or
 *   EFX_FIELD_BOTTOM, with parity p = 0 or 1.  E[t] is the lines y = p (mod 2) of F[t], the earlier field; L[t] is the
 *   other lines.  weave(E[t], L[x]) is the frame with E[t]'s lines and L[x]'s lines, for each of the three planes of the
 *   canonical image; chroma lines split by their own parity, as in efx_deinterlace.  A film frame occupies two or three
 *   consecutive field slots, so the partner of E[t] is L[t] or L[t-1], never anything further away: a two-way match is
 *   complete for 3:2 and 2:2 cadences.
 *   Comb score of a woven luma plane W of width w and height h.  With nt the noise threshold in pels, 0 .. 255:
 *     v(x, y) = | W[y-2][x] + 4 W[y][x] + W[y+2][x] - 3 (W[y-1][x] + W[y+1][x]) |      for 2 <= y <= h - 3 and all x
 *     score   = sum of max(0, v - 6 nt), as uint64
 *   v is 6 x the comb amplitude on a flat area and at most 1530.  Rows 0, 1, h - 2 and h - 1 have no v: no edge rule.
 *   Per frame t.
 *     cc = score(F[t])                              (the luma plane)
 *     cp = score(weave(E[t], L[t-1]))
 *     D  = sum of |E[t] - E[t-1]| over the luma lines of parity p, all columns
 *     match = p iff 4 cp < 3 cc, else c
 *   A frame with no predecessor (t = 0 and no lead) has match c, cp = 0 and D = 2^64 - 1.
 *   Decimation.  The processed frames of a call are taken in cycles of 5 from the first processed frame on.  In every
 *   whole cycle the frame with the smallest D is dropped; a tie drops the lowest t.  A last partial cycle drops nothing.
 *   Every kept frame t gives one output, weave(E[t], L[t - match]) (match c: F[t] itself), in order.
 *   n_out = n - floor(n / 5) with n = n_frames - lead: efx_detelecine_count().
 *   Pieces.  lead = 1 makes the first offered frame context only: it supplies E[t-1] and L[t-1] and has no output and no
 *   record.  No tail is needed.  A title goes through piece by piece with one frame of overlap; every piece but the last
 *   must process a multiple of 5 frames; the concatenated outputs and records then equal those of one long call (a
 *   piece's `out` counts from 0: add the outputs of the pieces before it).  Streams never see each other's frames.
 *   Layout.  Source image i * n_frames + j is stream i's frame j, at src_device + (i * n_frames + j) * src_stride.  Outputs
 *   are packed I420 pictures of the surface's width x height, which efx_import_frames and efx_detect_crop take as they
 *   are; output m of stream i lies at dst_device + (i * n_out + m) * dst_stride.
 *   Report.  One efx_telecine_info per processed frame, stream i's processed frame j (frame lead + j) at info_device +
 *   (i * n + j): its cc, cp and D, its match, and its output index within the stream's call or -1 where it was dropped.
 *   The buffer also serves as the kernels' only scratch -- the context allocates nothing -- and its content before the
 *   call does not matter.  From it a caller reads whether a title is film at all (no frame ever matches p, no D stands
 *   out in its cycle) and which kept frames stayed combed (video inserts); acting on that is the caller's business.
 *   Surfaces.  EFX_SURF_PLANAR8 (YV12 by swapped offsets) and EFX_SURF_SEMI8 (NV12 / NV21, de-interleaved on load); width
 *   even, 2 .. 4096; height a multiple of 4, 8 .. 4096.
 *
 * Memory contract.  For source image k the kernels read only bytes in [src + k * src_stride, src + k * src_stride + bytes
 * rounded up to 16), 16 bytes at a time wherever a plane's rows begin, and only rows of the three planes: the measuring
 * launch the luma rows of every processed frame and of its predecessor, the weaving launch exactly the rows it writes (a
 * dropped frame's only where the next frame matched p).  Bytes in pitch padding, between planes and between images are
 * fetched at most as part of such an access and never influence a result.  The kernels write only the width x height x
 * 3 / 2 bytes of each output image and the n_streams x n records.  All offsets are computed in 64 bits.  The source,
 * destination and record regions must not overlap.
 *
 * Out of scope: a third (next-frame) match candidate; post-deinterlacing of frames that stay combed; cadences other than
 * cycles of 5 (PAL speed-up needs none; 2:2 phase-shifted material is matched, but nothing of it should be decimated: such
 * a caller uses the records' match only); the 16-bit layouts; chaining into efx_import_surfaces; efx_multi_*.  Whether a
 * title is telecined, and with which first_field: efx_detect_scan ("scan type" below). */
typedef struct efx_telecine_info {
    uint64_t comb_c;      /* cc */
    uint64_t comb_p;      /* cp */
    uint64_t diff;        /* D */
    int32_t match;        /* 0 = c, 1 = p */
    int32_t out;          /* the output index within the stream's call; -1 = dropped */
} efx_telecine_info;
typedef struct efx_detelecine_opts {
    int n_streams;        /* >= 1 */
    int n_frames;         /* frames per stream offered by this call, >= 1 */
    int first_field;      /* EFX_FIELD_TOP / EFX_FIELD_BOTTOM */
    int lead;             /* 0 / 1: the first offered frame is context only */
    int nt;               /* the noise threshold in pels, 0 .. 255; 10 suits DVD material */
    size_t src_stride;    /* bytes between source images; 0 = the surface's bytes rounded up to 16; multiple of 16 */
    size_t dst_stride;    /* bytes between output images; 0 = efx_import_src_bytes(I420, w, h) rounded up to 16; multiple of 16 */
} efx_detelecine_opts;
/* Asynchronous on the context's stream: no host synchronisation and no read-back (n_out is known on the host), three
 * launches whatever the counts are -- measure, decide, weave -- and no decoder, encoder, SBC, import or other state is
 * touched.
 * EFX_ERR_ARG: everything efx_deinterlace rejects about a surface, n_streams < 1, lead other than 0 / 1, lead >=
 * n_frames, an unknown first_field, nt outside 0 .. 255, more than 2^31 - 1 images in, a NULL or misaligned (16 bytes)
 * src_device, dst_device or info_device, a stride that is too small or not a multiple of 16.  A refused call writes
 * nothing. */
int efx_detelecine(efx_ctx* ctx, const efx_surface* surface, const efx_detelecine_opts* opts, const void* src_device,
                   uint8_t* dst_device, efx_telecine_info* info_device);
/* outputs per stream of such a call; -1 for arguments it rejects.  Host only. */
int efx_detelecine_count(int n_frames, int lead);

/* -- scan type: progressive, interlaced or telecined (k_scan) -------------------------------- */
/* efx_deinterlace and efx_detelecine take first_field from the caller, and neither says whether a title needs it at
 * all.  A wrong guess is the costliest mistake of the source side: a woven interlaced frame that is scaled and encoded
 * has its ghosts baked in, film that is deinterlaced where it should be detelecined keeps a repeated picture in every
 * five, a wrong field order judders in every picture.  efx_detect_scan answers the question ffmpeg users put to idet,
 * for a whole batch of streams, piece by piece: per frame a label and a repeated-field flag, per stream their counts,
 * and efx_scan_verdict makes one answer of a stream's counts.  The rule is this library's own exact integer rule
 * (espflix_amd/csrc/scan_px.h), bit-reproducible anywhere.  Byte compatibility with ffmpeg is not promised.
 *
 *   Setting.  Luma only, of the canonical image of a surface ("surfaces" above), width w and height h.  The top field is
 *   the even lines.  score(W) is the comb score of "telecined sources" above, exactly as written there, with the same nt.
 *   Per frame t that has a predecessor.  All five are uint64.
 *     cc  = score(F[t])
 *     ctb = score(the frame with the even lines of F[t]   and the odd lines of F[t-1])
 *     cbt = score(the frame with the even lines of F[t-1] and the odd lines of F[t])
 *     dt  = sum of |F[t][y][x] - F[t-1][y][x]| over even y, all x
 *     db  = the same over odd y
 *   cc is efx_detelecine's cc; for first_field TOP ctb is its cp and dt its D, for BOTTOM cbt is its cp and db its D.
 *   Label of a frame.  The options still, prog, intl and rep; the last three are Q8 ratios.  The first test that holds
 *   decides:
 *     EFX_SCAN_STILL          16 (dt + db) < still w h
 *     EFX_SCAN_PROGRESSIVE    256 min(ctb, cbt) > prog cc
 *     EFX_SCAN_TFF            256 cbt > intl ctb
 *     EFX_SCAN_BFF            256 ctb > intl cbt
 *     EFX_SCAN_UNDETERMINED   otherwise
 *   Weaving the fields of a progressive frame with those of its neighbour combs both ways; of an interlaced frame the
 *   weave that puts the later field beside the previous frame's earlier one (two field periods apart) combs more than
 *   the one that puts neighbours in time side by side.  The PROGRESSIVE test comes before the order tests on purpose:
 *   on a progressive pan ctb and cbt differ by more than 1.04, so idet's own order of tests would call it interlaced.
 *   Repeat of a frame.  None for a STILL frame.  Otherwise the first test that holds:
 *     EFX_SCAN_REPEAT_TOP     rep dt < 256 db        (the top field repeats the previous frame's)
 *     EFX_SCAN_REPEAT_BOTTOM  rep db < 256 dt
 *     EFX_SCAN_REPEAT_NONE    otherwise
 *   A frame with no predecessor (t = 0 and lead = 0) is EFX_SCAN_NONE with no repeat; its five sums are 0 and it is
 *   counted nowhere.
 *   Defaults.  prog = 384, intl = 266 and rep = 768 are idet's 1.5, 1.04 and 3 in Q8; nt = 10 is efx_detelecine's.
 *   still = 64 is a mean field difference of 4 levels: that value has NOT been measured on real material, only on the
 *   synthetic cases of the tests (profiles/scan.md).  All five are options.
 *   Records.  One efx_scan_frame per processed frame, stream i's processed frame j (frame lead + j) at frames_device +
 *   (i * n + j), n = n_frames - lead; one efx_scan_rec per stream at recs_device + i: how many of the call's processed
 *   frames got each label, and rep_top[phase] / rep_bottom[phase], how many got that repeat at phase = (first_frame +
 *   index in the call) mod 5, the index counted over the offered frames (lead + j).  first_frame is the title's frame
 *   number of the call's first offered frame, so phases are title-absolute across pieces.
 *   Pieces.  lead has efx_detelecine's meaning: the first offered frame is context only.  accumulate = 1 adds a stream's
 *   counts to what recs_device holds (reserved becomes 0), accumulate = 0 overwrites: a title goes through in pieces
 *   with one frame of overlap and no read-back, and pieces need no length rule.  Streams never see each other's frames.
 *   Layout.  Source image i * n_frames + j is stream i's frame j, at src_device + (i * n_frames + j) * src_stride.
 *   frames_device is required: it is the call's only scratch, and its earlier content does not matter.
 *   Surfaces.  Those efx_detelecine accepts.
 *   Verdict (efx_scan_verdict, a pure function of a record).  n_moving = n_prog + n_tff + n_bff + n_undet; pt is the phase
 *   with the largest rep_top and pb the one with the largest rep_bottom, the lowest phase on a tie; m = rep_top[pt] +
 *   rep_bottom[pb]; tot is the sum of all ten repeat counters.
 *     EFX_SCAN_IS_TELECINED    iff rep_top[pt] >= 1, rep_bottom[pb] >= 1, m >= 4, 4 m >= 3 tot, 5 m >= n_moving and
 *                              (pb - pt) mod 5 is 2 or 3: 2 means first_field TOP, 3 BOTTOM.  (In 2-3 pulldown with the top
 *                              field first the bottom-field repeat comes two frames after the top-field repeat; with the
 *                              bottom field first it is the other way round.)
 *     EFX_SCAN_IS_INTERLACED   else iff n_tff + n_bff > n_prog and 4 min(n_tff, n_bff) <= max(n_tff, n_bff); first_field is
 *                              TOP iff n_tff > n_bff
 *     EFX_SCAN_IS_PROGRESSIVE  else iff n_prog >= 1 and n_prog >= n_tff + n_bff
 *     EFX_SCAN_IS_UNKNOWN      otherwise: all still, no frames, the order unclear
 *   These constants are part of the definition, not a tolerance; the counts are reported so that a caller can apply a
 *   rule of its own.
 *
 * Memory contract (efx_detelecine's, for luma rows only).  For source image k the kernel reads only bytes in [src + k *
 * src_stride, src + k * src_stride + bytes rounded up to 16), 16 bytes at a time wherever the luma plane's rows begin,
 * and only luma rows, of every processed frame and of its predecessor; chroma is never read.  Bytes in pitch padding and
 * between images are fetched at most as part of such an access and never influence a result.  The kernels write only
 * the n_streams x n frame records and the n_streams stream records.  All offsets are computed in 64 bits.  The source
 * and record regions must not overlap.
 *
 * Out of scope: phase-shifted 2:2 material (it comes out as INTERLACED); mixed titles, which get one verdict per record
 * (a caller cuts the title and keeps a record per part); the 16-bit layouts; a next-frame candidate; efx_multi_*. */
#define EFX_SCAN_NONE           0   /* labels: a frame with no predecessor */
#define EFX_SCAN_STILL          1
#define EFX_SCAN_PROGRESSIVE    2
#define EFX_SCAN_TFF            3
#define EFX_SCAN_BFF            4
#define EFX_SCAN_UNDETERMINED   5
#define EFX_SCAN_REPEAT_NONE    0   /* repeats */
#define EFX_SCAN_REPEAT_TOP     1
#define EFX_SCAN_REPEAT_BOTTOM  2
#define EFX_SCAN_IS_UNKNOWN     0   /* verdicts */
#define EFX_SCAN_IS_PROGRESSIVE 1
#define EFX_SCAN_IS_INTERLACED  2
#define EFX_SCAN_IS_TELECINED   3
typedef struct efx_scan_frame {       /* 48 bytes, one per processed frame; fixed-width fields only */
    uint64_t comb;                    /* cc */
    uint64_t comb_tb;                 /* ctb */
    uint64_t comb_bt;                 /* cbt */
    uint64_t diff_top;                /* dt */
    uint64_t diff_bottom;             /* db */
    int32_t  label;                   /* EFX_SCAN_NONE .. EFX_SCAN_UNDETERMINED */
    int32_t  repeat;                  /* EFX_SCAN_REPEAT_* */
} efx_scan_frame;
typedef struct efx_scan_rec {         /* 64 bytes, one per stream */
    uint32_t n_still, n_prog, n_tff, n_bff, n_undet;
    uint32_t rep_top[5];              /* frames with EFX_SCAN_REPEAT_TOP, by phase */
    uint32_t rep_bottom[5];           /* frames with EFX_SCAN_REPEAT_BOTTOM, by phase */
    uint32_t reserved;                /* 0 */
} efx_scan_rec;
typedef struct efx_scan_opts {        /* fixed-width fields only: a binding can mirror it as a packed record */
    int32_t  n_streams;               /* >= 1 */
    int32_t  n_frames;                /* frames per stream offered by this call, >= 1 */
    int32_t  lead;                    /* 0 / 1: the first offered frame is context only */
    int32_t  accumulate;              /* 0: overwrite recs_device; 1: add to it */
    int32_t  nt;                      /* the noise threshold of the comb score in pels, 0 .. 255; default 10 */
    int32_t  still;                   /* 0 .. 4080; default 64 (synthetic material only, see above) */
    int32_t  prog, intl, rep;         /* Q8 ratios, 256 .. 65535; defaults 384, 266, 768 */
    int32_t  reserved;                /* ignored */
    uint64_t first_frame;             /* the title's frame number of the first offered frame (only its value mod 5 matters) */
    uint64_t src_stride;              /* bytes between source images; 0 = the surface's bytes rounded up to 16; multiple of 16 */
} efx_scan_opts;
/* Asynchronous on the context's stream: no host synchronisation, two launches whatever the counts are -- measure, count
 * -- nothing is allocated, and no decoder, encoder, SBC, import or other state is touched.
 * EFX_ERR_ARG: everything efx_detelecine rejects about a surface, the counts, lead and src_stride, nt outside 0 .. 255,
 * still outside 0 .. 4080, prog, intl or rep outside 256 .. 65535, accumulate other than 0 / 1, a NULL or misaligned
 * (16 bytes) src_device, frames_device or recs_device.  A refused call writes nothing. */
int efx_detect_scan(efx_ctx* ctx, const efx_surface* surface, const efx_scan_opts* opts, const void* src_device,
                    efx_scan_frame* frames_device, efx_scan_rec* recs_device);
/* The verdict of a stream's record (EFX_SCAN_IS_*), or EFX_ERR_ARG for a NULL record.  *first_field (may be NULL) is
 * written only for TELECINED and INTERLACED: EFX_FIELD_TOP / EFX_FIELD_BOTTOM.  Host only. */
int efx_scan_verdict(const efx_scan_rec* rec, int* first_field);

/* -- noisy sources: spatial and temporal noise reduction (k_denoise) ------------------------ */
/* Film grain and analogue or sensor noise are the part of a picture that motion compensation cannot predict, and at 1.5
 * Mbit/s every bit spent on noise is taken from the picture.  DVD-size sources are scaled down only 2 to 2.5 times by
 * the import, so their noise survives it.  efx_denoise filters the source pictures at their own size, before anything
 * is scaled: the step the reference indexer leaves to ffmpeg's hqdn3d.  The rule is this library's own exact integer
 * rule (espflix_amd/csrc/denoise_px.h), bit-reproducible anywhere.  Byte compatibility with ffmpeg is not promised.
 *
 * The rule is applied to each of the three planes of the canonical image of a surface ("surfaces" above), each with its
 * own w, h (luma: width x height; Cb, Cr: half of each).  Luma uses (Ts, Tt) = (luma_spatial, luma_temporal), Cb and Cr
 * use (chroma_spatial, chroma_temporal); every threshold lies in 0 .. 64.  All values are int, >> is arithmetic.
 *
 *   Spatial step.  Row and column indices are clamped to the plane.  With F the plane of the frame, c = F[y][x] and the
 *   weights K = [[1, 2, 1], [2, 4, 2], [1, 2, 1]]:
 *     v(i, j) = F[y+i][x+j]  if |F[y+i][x+j] - c| <= Ts,  else c               (i, j in -1, 0, 1)
 *     s = (sum of K[i][j] v(i, j) + 8) >> 4
 *   A thresholded 3 x 3 binomial filter: a neighbour across an edge is replaced by the centre.  Ts = 0 gives s = c.
 *   Temporal step.  Recursive over a stream's frames: P is the output sample at the same place of the stream's previous
 *   output picture.  For a stream's first picture with no `prev` (a title's start) out = s; with Tt = 0, out = s;
 *   otherwise
 *     d = s - P;  a = |d|
 *     k = 256                       if a >= Tt
 *     k = 64 + ((a a Q) >> 16)      otherwise, with Q = 12582912 / (Tt Tt)      (integer division; 12582912 = 192 x 65536)
 *     out = P + sgn(d) ((a k + 128) >> 8)
 *   out lies between s and P, so in 0 .. 255; out = P with s != P only for a = 1, so the recursion never lags a static
 *   value by more than one level; a a Q < 2^24; the rounding is symmetric in the sign of d (no brightness drift); a
 *   sample that moved by Tt or more takes the new value whole, which is why moving edges leave no trail.
 *   Layout.  Source image i * n_frames + j is stream i's frame j, at src_device + (i * n_frames + j) * src_stride.  Outputs
 *   are packed I420 pictures of the surface's width x height at dst_device + (i * n_frames + j) * dst_stride, as
 *   efx_deinterlace writes them: efx_import_frames, efx_detect_crop, efx_deinterlace and efx_detelecine (through
 *   efx_surface_layout(EFX_KIND_I420)) read them as they are.
 *   Pieces.  prev_device + i * prev_stride is stream i's last output picture of the previous piece, packed I420: a caller
 *   passes dst_prev + (n_prev - 1) * dst_stride with prev_stride = n_prev * dst_stride.  There is no copy and no state
 *   buffer, and the concatenated outputs of the pieces equal those of one long call, byte for byte.  prev_device = NULL
 *   is the title's start.  Streams never see each other's frames.
 *   Surfaces.  EFX_SURF_PLANAR8 (YV12 by swapped offsets; pitched) and EFX_SURF_SEMI8 (NV12 / NV21, de-interleaved on
 *   load); width and height even, 2 .. 4096.
 *   Settings.  Thresholds of (2 sigma, 2 sigma, 4 sigma, 4 sigma) for noise of standard deviation sigma are the measured
 *   ones (profiles/denoise.md).
 *
 * Memory contract (efx_deinterlace's).  For source image k the kernel reads only bytes in [src + k * src_stride, src + k
 * * src_stride + bytes rounded up to 16), 16 bytes at a time wherever a plane's rows begin, and only rows of the three
 * planes; of a previous output only [prev + i * prev_stride, ... + width x height x 3 / 2 rounded up to 16).  Bytes in
 * pitch padding, between planes and between images are fetched at most as part of such an access and never influence a
 * result.  It writes only the width x height x 3 / 2 bytes of each output image.  All offsets are computed in 64 bits.
 * The source, previous-output and destination regions must not overlap.
 *
 * Out of scope: the 16-bit layouts, motion-compensated filtering, a noise estimate that chooses the thresholds, state
 * at more than 8 bits, chaining into the import or the title builder, efx_multi_*. */
typedef struct efx_denoise_opts {     /* fixed-width fields only: a binding can mirror it as a packed record */
    int32_t  n_streams;               /* >= 1 */
    int32_t  n_frames;                /* frames per stream in this call, >= 1 */
    int32_t  luma_spatial, chroma_spatial, luma_temporal, chroma_temporal;   /* 0 .. 64 */
    uint64_t src_stride, dst_stride;  /* as efx_deint_opts: 0 = default, multiples of 16 */
    uint64_t prev_stride;             /* bytes between the streams' previous output pictures; multiple of 16 */
} efx_denoise_opts;
/* Asynchronous on the context's stream: no host synchronisation, one launch whatever the counts are, no scratch, and no
 * decoder, encoder, SBC, import or other state is touched.
 * EFX_ERR_ARG: everything efx_import_surfaces rejects about a surface, a 16-bit layout, a threshold outside 0 .. 64,
 * n_streams or n_frames below 1, more than 2^31 - 1 images, a NULL or misaligned (16 bytes) src_device or dst_device, a
 * misaligned prev_device, a stride that is too small or not a multiple of 16, prev_stride of 0 with prev_device given
 * and n_streams > 1.  A refused call writes nothing. */
int efx_denoise(efx_ctx* ctx, const efx_surface* surface, const efx_denoise_opts* opts, const void* src_device,
                const uint8_t* prev_device /* NULL: the title's start */, uint8_t* dst_device);

/* -- subtitles and logos: events alpha-blended into pictures (k_overlay) -------------------- */
/* The player shows one MPEG-1 picture and nothing over it but its own progress bar: text or a station logo reaches the
 * screen only burnt into the pictures before efx_encode reads them -- what ffmpeg does with subtitles= / ass= (alpha
 * masks and a colour) and overlay= (an RGBA picture).  efx_overlay blends a list of events, bitmaps shown over a span of
 * pictures, into batches of 352 x 192 I420 pictures, in place, on the device.  The rule is exact integer arithmetic
 * (espflix_amd/csrc/overlay_px.h), bit-reproducible anywhere.  All values are int, >> is arithmetic, / is integer
 * division of non-negative values.
 *
 *   Pictures.  The layout efx_encode, efx_conform_rate and efx_trick_pick read: 101376 bytes a picture (Y 192 x 352, Cb
 *   96 x 176, Cr 96 x 176), stream i's picture j at pictures + i * stride + j * 101376.  Picture j of the call has the
 *   title index p = first_picture + j.
 *   Events.  One 64-byte record each (efx_overlay_event below), bitmaps in one atlas of atlas_bytes bytes.  An event is
 *   VALID when: kind is 0 or 1; 0 <= first <= last < 2^40; stream >= -1; x and y lie in -4096 .. 4095; w and h lie in 1 ..
 *   4096; opacity <= 256; fade_in and fade_out <= 32767; with bpp = 1 (EFX_OVL_A8) or 4 (EFX_OVL_RGBA), pitch >= w bpp;
 *   for RGBA offset and pitch are multiples of 4; offset + (h - 1) pitch + w bpp <= atlas_bytes, computed in 64 bits;
 *   colour < 2^24 for A8 and 0 for RGBA; both reserved fields are 0.
 *   Activity.  Event e is active for stream s and picture j when it is valid, (stream == -1 or stream == s) and first <= p
 *   <= last.  An event whose stream is >= n_streams is never active: one list serves every shard of a batch.  Everything
 *   depends on p only, so the pieces of a title, concatenated, equal one long call; no state is carried.
 *   Gain of an event at picture p.  With k = p - first: fi = 256 if fade_in == 0 or k >= fade_in, else fi = (256 (k + 1)) /
 *   (fade_in + 1).  With k' = last - p: fo likewise from fade_out.  g = (opacity min(fi, fo) + 128) >> 8, in 0 .. 256.
 *   fade_in = 3, fade_out = 2, opacity = 256 over pictures 10 .. 20: 64 128 192 256 256 256 256 256 256 170 85.
 *   Sample alpha and colour.  For the picture's luma sample (X, Y) the bitmap sample is (X - x, Y - y); outside 0 .. w - 1,
 *   0 .. h - 1 it is absent and a = 0.  Otherwise a = (A g + 128) >> 8 with A the alpha byte: 0 .. 255, and A = 255 with
 *   g = 256 gives 255.  The colour (Cy, Ccb, Ccr) is the import's BT.601 studio-swing matrix (efx_import_frames, RGB
 *   sources, full_range = 0) of the pixel's R, G, B for RGBA (bytes R, G, B, A, straight alpha), or of `colour`
 *   (0x00RRGGBB) for A8 (one alpha byte a sample).
 *   Luma.  t = Y (255 - a) + Cy a;  out = (2 t + 255) / 510, which is t / 255 rounded half up.  a = 0 leaves Y, a = 255
 *   gives Cy.
 *   Chroma.  Premultiplied 2 x 2 down-sampling: the site (cx, cy) covers the luma samples (2 cx + i, 2 cy + j), i, j in
 *   0, 1, with alphas a_ij (0 where absent) and colours c_ij.  S = sum a_ij (<= 1020), N = sum a_ij c_ij, and
 *   out = (C (1020 - S) + N + 510) / 1020, for Cb and Cr alike.  Absent samples need no colour.  out lies between the
 *   extremes of C and the c_ij.
 *   Order.  The active events of a picture are applied in list order, each to the 8-bit result of the one before: a
 *   later event is on top.  With Y = 100, white (Cy = 235) at a = 128 then black (16) at a = 128 gives 92; the other
 *   order gives 147.
 *
 * Memory contract.  The kernel reads events only in [events, events + n_events x 64) and the atlas only in [atlas, atlas
 * + atlas_bytes rounded up to 16), 16 bytes at a time at any alignment, and only for bitmap rows and 16-byte groups of
 * columns that land inside a picture; no atlas byte of an invalid event is read.  Bytes in pitch padding and between
 * bitmaps never influence a result.  A picture with no active event is neither read nor written.  A picture with active
 * events is read and written only in the 16-byte chunks of plane rows that an active event's clipped rectangle touches
 * (chroma: the rectangle halved outward); bytes of those chunks outside the rectangle are written back unchanged.
 * Bytes between pictures (stride padding) are never written.  The atlas, event and picture regions must not overlap.
 *
 * Out of scope: rendering text or parsing subtitle files (the caller brings bitmaps), events that move or scale, other
 * blend modes, sources at their own size, the frame rings as destination, efx_multi_*. */
#define EFX_OVL_A8   0
#define EFX_OVL_RGBA 1
#define EFX_OVERLAY_BAD_EVENT 8192u  /* status_device bit: the list holds an event that is not valid; it was not drawn */
#define EFX_OVERLAY_MAX_EVENTS 4096
typedef struct efx_overlay_event {     /* 64 bytes, fixed-width fields only, little endian */
    int64_t  first;                    /* title index of the first picture that shows the event */
    int64_t  last;                     /* ... of the last one */
    uint64_t offset;                   /* byte offset of the bitmap in the atlas */
    int32_t  stream;                   /* stream of the call it belongs to, -1 = every stream */
    int32_t  x;                        /* picture column of the bitmap's top-left sample */
    int32_t  y;                        /* picture row of it; both may be negative or beyond the picture: the bitmap is clipped */
    uint32_t pitch;                    /* bytes between bitmap rows */
    uint32_t colour;                   /* EFX_OVL_A8: 0x00RRGGBB; EFX_OVL_RGBA: 0 */
    uint16_t w;                        /* bitmap width */
    uint16_t h;                        /* bitmap height */
    uint16_t opacity;                  /* 0 .. 256 */
    uint16_t fade_in;                  /* fade-in length in pictures */
    uint16_t fade_out;                 /* fade-out length in pictures */
    uint8_t  kind;                     /* EFX_OVL_A8 or EFX_OVL_RGBA */
    uint8_t  reserved0;                /* 0 */
    uint64_t reserved;                 /* 0 */
} efx_overlay_event;
typedef struct efx_overlay_opts {      /* fixed-width fields only */
    int32_t  n_streams;                /* >= 1 */
    int32_t  n_pictures;               /* pictures per stream in this call, >= 1 */
    int32_t  n_events;                 /* 0 .. 4096 */
    int32_t  reserved;                 /* 0 */
    int64_t  first_picture;            /* title index of the call's picture 0, 0 .. 2^40 - 1 */
    uint64_t stride;                   /* bytes between streams; 0 = n_pictures x 101376; multiple of 16 */
    uint64_t atlas_bytes;              /* bytes of the atlas the events may name */
} efx_overlay_opts;
/* Asynchronous on the context's stream: no host synchronisation, one launch whatever the counts are and none for n_events
 * == 0 (which returns EFX_OK), no scratch, no allocation, and no decoder, encoder, SBC or import state is touched.
 * The kernel applies the validity rule to every event it reads: an invalid event is drawn for no picture, the valid
 * events of the same list are drawn as usual, and EFX_OVERLAY_BAD_EVENT is ORed (vector atomics; the caller clears the
 * words) into every one of the n_streams words of status_device (may be NULL) when the list holds one.
 * EFX_ERR_ARG: a count out of range, more than 2^31 - 1 pictures, first_picture below 0 or first_picture + n_pictures
 * above 2^40, a non-zero reserved field, a NULL or misaligned (16 bytes) pictures_device, a NULL events_device or
 * atlas_device with n_events > 0, events_device not 8-byte aligned, status_device not 4-byte aligned, a stride that is too
 * small or not a multiple of 16.  A refused call writes nothing. */
int efx_overlay(efx_ctx* ctx, const efx_overlay_opts* opts, const efx_overlay_event* events_device, const uint8_t* atlas_device,
                uint8_t* pictures_device, uint32_t* status_device /* n_streams words, or NULL */);
/* The index of the first event of the list that is not valid for an atlas of atlas_bytes, or -1 (also for a NULL list or
 * n_events <= 0).  Host only. */
int efx_overlay_check(const efx_overlay_event* events, int n_events, uint64_t atlas_bytes);

/* -- source colour: BT.709, full-range and other YCbCr sources to BT.601 (k_import) -------- */
/* MPEG-1 carries BT.601 studio-swing YCbCr, and efx_import_frames / efx_import_surfaces copy a YCbCr source's samples
 * through.  What a decoder hands over today is mostly HD with BT.709 matrix coefficients, and phone or JPEG-derived
 * material is full range.  efx_import_set_colour names the source's matrix and range -- pass the decoder's
 * matrix_coefficients and video_full_range_flag straight in -- and the imports that follow convert to BT.601 studio
 * swing in the same kernel: no further launch, no further byte of memory traffic.
 *
 *   matrix      the H.273 matrix_coefficients code:            Kr       Kb
 *                 1      BT.709                                0.2126   0.0722
 *                 4      FCC                                   0.30     0.11
 *                 5, 6   BT.601                                0.299    0.114
 *                 7      SMPTE 240M                            0.212    0.087
 *                 9      BT.2020 non-constant luminance        0.2627   0.0593
 *                 2      unspecified: BT.709 when the source's height is above 576, BT.601 otherwise
 *               Every other code (0 GBR, 8 YCgCo, 10 BT.2020 constant luminance ...) is an invalid argument.  Code 9
 *               converts the matrix only: transfer and gamut mapping are efx_import_set_hdr's (below).
 *   full_range  0 = studio (Y 16 .. 235, C 16 .. 240), 1 = full (Y 0 .. 255, C centred on 128 over 255).
 *   The target is always BT.601 studio swing.  "Off" is code 5 or 6 with studio range, or code 2 with studio range on a
 *   source no higher than 576 lines.
 *
 *   Coefficients.  For the source's (Kr, Kb): R, G, B from the normalised (y, pb, pr); the BT.601 (y', pb', pr') of that
 *   R, G, B; scaled by the source's and the target's 8-bit ranges.  That is a 3 x 3 matrix whose first column is
 *   (., 0, 0) -- converted chroma never depends on luma -- and q = round(2^14 x exact value), computed in rational
 *   arithmetic, a literal table (espflix_amd/csrc/colour_px.h).  BT.709 studio: 16384 1627 3141; 0 16218 -1813;
 *   0 -1187 16112.
 *   One pixel, y0 = 16 (studio) or 0 (full), >> arithmetic, results clamped to 0 .. 255:
 *     Y'  = 16  + ((q00 (Y - y0) + q01 (Cb - 128) + q02 (Cr - 128) + 8192) >> 14)
 *     Cb' = 128 + ((q11 (Cb - 128) + q12 (Cr - 128) + 8192) >> 14)
 *     Cr' = 128 + ((q21 (Cb - 128) + q22 (Cr - 128) + 8192) >> 14)
 *   which is within 1 of the rounded exact map for every (Y, Cb, Cr).
 *   One picture.  The conversion applies to the 8-bit picture the import produces without it: the converted import is,
 *   bit for bit, convert(that picture), so the scaling definition above is untouched.  Only the samples inside the
 *   destination rectangle are converted; the border is BT.601 black already and stays (16, 128, 128).  A luma sample
 *   uses the unconverted Cb, Cr of its 2 x 2 block (nearest siting, as ffmpeg's colormatrix; the rectangle's offsets and
 *   sides are even, so blocks and chroma sites coincide).
 *
 * The setting applies to I420 sources of efx_import_frames and to every efx_import_surfaces call.  RGB sources convert
 * with their own BT.601 matrix and ignore it (efx_import_opts.full_range names the range they write).  Crop detection
 * reads source luma and is not touched: for a full-range source pass a limit in source terms (black is 0, not 16). */
typedef struct efx_import_colour {
    int matrix;      /* H.273 matrix_coefficients: 1, 2, 4, 5, 6, 7 or 9 */
    int full_range;  /* 0 = studio, 1 = full */
} efx_import_colour;
/* Applies to the import calls that follow, like efx_encode_set_*; NULL switches the conversion off (the default: bytes,
 * launches and allocations are then what they were).  Host state only: calls already queued keep their setting, the
 * coefficients travel in each launch's arguments.  EFX_ERR_ARG: an unknown code or a range other than 0 or 1; the
 * setting is then unchanged. */
int efx_import_set_colour(efx_ctx* ctx, const efx_import_colour* colour);
/* The coefficients of a setting for a source of `height` lines (it matters for code 2 only): q row major (q[3] = q[6] =
 * 0), *y0 = 16 or 0.  Returns 0 for "off" (q is then the identity, 16384 on the diagonal), 1 for a conversion, negative
 * (EFX_ERR_ARG) for an invalid argument or a NULL pointer.  Host only. */
int efx_import_colour_coefs(int matrix, int full_range, int height, int32_t q[9], int* y0);

/* -- HDR sources: HDR10 (PQ, BT.2020) tone-mapped to BT.601 SDR (k_import) ----------------- */
/* P010 is the surface format of HDR10 material.  The colour setting above converts its matrix only; a PQ picture then
 * comes out grey, flat and desaturated.  efx_import_set_hdr names the source's transfer, primaries, matrix, range and
 * peak, and the imports that follow tone-map to the BT.601 studio-swing SDR picture MPEG-1 carries in the same kernel
 * (what ffmpeg does with zscale=t=linear, tonemap, zscale=t=bt709): no further launch, no further byte of memory traffic.
 *
 *   import10.  The import's definition with the last rounding replaced: v10 = (sum + 2^19) >> 20, 0 .. 1020, the same
 *   taps, hround and accumulators.  The 10-bit video scale applies: studio luma 64 .. 940, chroma 512 +- 448, full range
 *   0 .. 1020 around 512.  Surfaces are still reduced to their canonical 8-bit image first.
 *   Result.  tonemap(import10(canonical image)) inside the destination rectangle; the border stays (16, 128, 128).
 *   Item.  One chroma site and its 2 x 2 luma samples; all four pixels use the site's Cb10, Cr10.  Per pixel, exact
 *   integers (espflix_amd/csrc/hdr_px.h; >> arithmetic):
 *     1. matrix: R' = clamp((qy (Y10 - y0) + qrv (Cr10 - 512) + 8192) >> 14, 0, 2^24), G' and B' likewise with (qgu, qgv)
 *        and qbu: steps of 2^-24, 64-bit sums; q = round(2^14 x 2^24 x exact) from the matrix code's (Kr, Kb) and the
 *        range, in rational arithmetic (BT.2020 studio: 313787565, 452382770, -50482164, -175281642, 577182248; y0 = 64).
 *     2. first table, per channel, PQ code -> display light relative to 100 nits in steps of 2^-24: entry i = E' = i / 2048
 *        is round(2^24 min(1, EOTF(E2 PQ(peak)) / 100)) with the SMPTE ST 2084 EOTF and the BT.2390 EETF in the PQ domain
 *        (source black 0, source peak peak_nits, target peak 100 nits, no black lift: E1 = min(1, E' / PQ(peak)), maxLum =
 *        PQ(100) / PQ(peak), KS = 1.5 maxLum - 0.5, E2 = E1 below KS and the Hermite spline from KS on).  i = R' >> 13,
 *        f = R' & 8191: L = T[i] + (((T[i + 1] - T[i]) f + 4096) >> 13) (2049 entries).
 *     3. gamut: primaries 9: the linear BT.2020 -> BT.709 matrix of BT.2087 in steps of 2^-28, from the primaries in
 *        rational arithmetic, each row's diagonal entry adjusted so that the row sums to exactly 2^28 (445734659
 *        -157743717 -19555486; -33433763 304110500 -2241281; -4872308 -26998942 300306706); primaries 1: the identity.
 *        64-bit sums, + 2^27, >> 28, clamped to 0 .. 2^24.
 *     4. second table, inverse BT.1886, E' = L^(1 / 2.4) in steps of 2^-15: with t the position of x's leading bit and
 *        s = max(0, t - 6), entry 64 s + (x >> s) holds round(2^15 (x' / 2^24)^(1 / 2.4)) for x' = (x >> s) << s; the s
 *        bits below interpolate linearly to the next entry (1217 entries, the last is x = 2^24).
 *     5. Y' = 16 + ((16763 R' + 32910 G' + 6391 B' + 2^22) >> 23).
 *   Cb' = 128 + ((-4838 R + -9498 G + 14336 B + 2^23) >> 24) and Cr' = 128 + ((14336 R - 12005 G - 2331 B + 2^23) >> 24)
 *   with R, G, B the sums of the four pixels' R', G', B' (the box is MPEG-1's centred chroma site).  Everything is
 *   rounded to 8 bits once.  Against the same map in float64 (tests/hdr_model.py) Y', Cb' and Cr' are within 1.
 *   Grey (Cb10 = Cr10 = 512) stays grey, studio black gives 16, every luma at or above the code of peak_nits gives 235.
 *
 * While the setting is on it supersedes efx_import_set_colour for YCbCr sources (it carries its own matrix and range);
 * RGB sources ignore it.  Not built: HLG, luminance-keyed or max-RGB tone mapping, highlight desaturation, dynamic
 * metadata, targets other than 100 nits. */
typedef struct efx_import_hdr {
    int transfer;    /* H.273 transfer_characteristics: 16 = SMPTE ST 2084 (PQ) */
    int primaries;   /* H.273 colour_primaries: 9 = BT.2020 (mapped to BT.709), 1 = BT.709 (no gamut step) */
    int matrix;      /* H.273 matrix_coefficients, the codes of efx_import_set_colour; normally 9 */
    int full_range;  /* 0 = studio, 1 = full */
    int peak_nits;   /* source peak (MaxCLL or the mastering display's maximum): 200 .. 10000; 0 = 1000 */
} efx_import_hdr;
/* Applies to the import calls that follow; NULL switches the stage off (the default: bytes, launches and allocations are
 * then what they were).  Calls already queued keep their setting: the context keeps one device copy of the tables per
 * distinct setting it has seen (10.7 KB of host and of device memory each, made at the setting's first import, freed by
 * efx_destroy), uploaded once in stream order, and a launch carries its pointer; no host synchronisation.  EFX_ERR_ARG:
 * any other code or a peak outside the range; the setting is then unchanged. */
int efx_import_set_hdr(efx_ctx* ctx, const efx_import_hdr* hdr);
/* Everything the kernel reads for a setting and a source of `height` lines (it matters for matrix code 2 only): 16 int32
 * (qy, qrv, qgu, qgv, qbu, y0, the nine gamut coefficients, the peak), 2052 uint32 (the first table, 2049 entries used),
 * 1224 uint16 (the second, 1217 used).  Returns the bytes (10720) and fills out when cap holds them (out may be NULL to
 * ask for the size), negative (EFX_ERR_ARG) for an invalid setting.  Host only. */
int efx_import_hdr_tables(const efx_import_hdr* hdr, int height, void* out, size_t cap);

/* -- picture quality: PSNR and SSIM of picture batches (k_quality) ------------------------- */
/* The library tells a caller how many bytes a picture took; efx_compare_pictures tells how good it is: what ffmpeg
 * answers with `-psnr` and the `ssim` filter, on the device, for a whole batch, as a reduction -- two picture sets are
 * read once and 48 bytes per picture are left.  The definition is exact integer arithmetic
 * (espflix_amd/csrc/quality_px.h), bit-reproducible anywhere.
 *
 *   Pictures.  Both inputs are I420 pictures in the layout efx_encode reads and efx_export_frames writes: Y 192 x 352,
 *   Cb 96 x 176, Cr 96 x 176, 101 376 bytes.  Image k of the reference is at ref + k x ref_stride, image k of the picture
 *   under test at test + k x test_stride.
 *   Reference clamp.  With ref_max = m (1 .. 255) every reference sample a is taken as min(a, m) before anything else;
 *   test samples are never changed.  ref_max = 0 means 255 (no clamp); m = 248 is the decoder's clamp: a source against
 *   what a decoder reconstructs from it.
 *   Blocks.  Each plane is tiled by 4 x 4 blocks, 88 x 48 for luma and 44 x 24 for each chroma plane.  For a block, with
 *   a the clamped reference and b the test samples:  s1 = sum a,  s2 = sum b,  ss = sum (a^2 + b^2),  s12 = sum a b.
 *   SSE.  Per plane sse = sum (a - b)^2 = sum over blocks of (ss - 2 s12), exact in uint64 (luma reaches 67584 x 65025 =
 *   4 394 649 600, above 2^32).
 *   Per-macroblock luma SSE (optional output).  For macroblock (r, c), r < 12, c < 22: the SSE of luma rows 16r .. 16r +
 *   15 and columns 16c .. 16c + 15, a uint32 at index 22r + c (at most 256 x 65025).
 *   SSIM.  x264's and ffmpeg's 8 x 8 window on a 4-pel grid, made exact.  A window is 2 x 2 adjacent blocks: windows
 *   (i, j) with i < rows - 1 and j < cols - 1 of the block grid, 87 x 47 = 4089 for luma and 43 x 23 = 989 for each
 *   chroma plane.  With S1, S2, SS, S12 the sums of the four blocks' values:
 *       vars  = 64 SS - S1^2 - S2^2          covar = 64 S12 - S1 S2
 *       c1 = 416                             c2 = 235963
 *       num = (2 S1 S2 + c1) (2 covar + c2)
 *       den = (S1^2 + S2^2 + c1) (vars + c2)
 *       q   = sign(num) floor(|num| 65536 / den)        (Q16, truncated toward zero)
 *   vars >= 0 and 2 |covar| <= vars, so |num| <= den < 2.9e17 and q lies in [-65536, 65536]; num and den fit a signed
 *   64-bit integer, |num| x 65536 does not: the quotient is an estimate corrected exactly with its remainder.  The plane's
 *   result is the int64 sum of q over its windows.
 *   Record.  48 bytes per image: sse[3], ssim[3] for Y, Cb, Cr.
 *   Derived values (host only).  PSNR = 10 log10(255^2 samples / sse), +infinity for sse 0, samples 67584 for luma and
 *   16896 for a chroma plane; mean SSIM = ssim / (65536 windows).  Each window's q / 65536 is lower in magnitude than the
 *   real quotient by less than 2^-16, so a plane's mean SSIM differs from a float64 evaluation by less than 2^-16.
 *   Anchors (luma).  Identical planes: sse 0, ssim 4089 x 65536 = 267 976 704.  Reference all 0 against test all 255: sse
 *   4 394 649 600, ssim 0.  The checkerboard ((x + y) & 1) x 255 against its inverse: sse 4 394 649 600, ssim
 *   4089 x -65304 = -267 028 056.  Identical chroma planes: 989 x 65536 = 64 815 104 each.
 *
 * Memory contract.  For image k the kernels read only the 101 376 bytes at ref + k x ref_stride and at test + k x
 * test_stride (ref_device == test_device is allowed), in 16-byte pieces; the luma rows 16b .. 16b + 3 (b = 1 .. 11) and
 * the chroma rows 8b .. 8b + 3 are asked for twice, by adjacent workgroups.  Every call writes all n_images records in
 * full -- it never accumulates into what the buffer held before -- and, when mb_sse_device is given, the 264 elements of
 * each image at mb_sse_device + k x mb_stride; the bytes between images are not written in any buffer.  All offsets are
 * computed in 64 bits.
 *
 * Out of scope: the frame rings as a source (export first), pictures of other sizes, Gaussian-window SSIM, MS-SSIM and
 * VMAF. */
typedef struct efx_compare_opts {
    int n_images;        /* >= 1; not tied to max_streams */
    int ref_max;         /* 0 = 255 (no clamp), else 1 .. 255 */
    size_t ref_stride;   /* bytes between reference images; 0 = 101376; multiple of 16, >= 101376 */
    size_t test_stride;  /* likewise */
    size_t mb_stride;    /* uint32 elements between images in mb_sse_device; 0 = 264; multiple of 4, >= 264 */
} efx_compare_opts;
typedef struct efx_compare_rec { uint64_t sse[3]; int64_t ssim[3]; } efx_compare_rec;
/* Asynchronous on the context's stream: no host synchronisation, two launches whatever n_images is (the records to zero,
 * the sums), no scratch memory, and no decoder, encoder, SBC or import state is touched.
 * EFX_ERR_ARG: a NULL or misaligned (16 bytes) ref_device, test_device or recs_device, a misaligned mb_sse_device,
 * n_images < 1, ref_max outside 0 .. 255, a ref_stride or test_stride below 101376 or not a multiple of 16, an mb_stride
 * below 264 or not a multiple of 4. */
int efx_compare_pictures(efx_ctx* ctx, const efx_compare_opts* opts, const uint8_t* ref_device, const uint8_t* test_device,
                         efx_compare_rec* recs_device, uint32_t* mb_sse_device /* may be NULL */);
/* 10 log10(255^2 samples / sse); +infinity for sse 0; NaN for samples 0.  Host only. */
double efx_compare_psnr(uint64_t sse, uint64_t samples);
/* sum / (65536 windows of the plane): plane 0 = Y, 1 / 2 = chroma; NaN otherwise.  Host only. */
double efx_compare_ssim(int64_t sum, int plane);

/* -- MPEG-1 encode on the device (k_encode) ---------------------------------------------- */
/* The reference plays titles that were "encoded with ffmpeg at around 1.5MBits" (README.md:87) ahead of time; nothing in it
 * writes a stream.  efx_encode turns I420 pictures in device memory (the layout efx_export_frames writes: Y 192 x 352, then
 * Cb 96 x 176, then Cr 96 x 176, 101 376 bytes) into MPEG-1 video that the reference player plays, for n_streams streams
 * at once; with decode and I420 export it makes an on-device transcode.
 *
 * The streams honour every constraint of the reference decoder: 352 x 192, I and P pictures only, a sequence header and a
 * closed GOP header before every I picture (default quantiser matrices; what the trick-play index seeks to), temporal_reference
 * = pictures since the GOP header, vbv_delay 0xFFFF, full_pel_forward_vector 0 and forward_f_code 1 (search <= 7) or 2; one
 * slice per macroblock row at quantiser_scale `qscale`; a P macroblock is intra, coded with or without motion compensation,
 * motion compensated and not coded, or skipped -- never the first or last of its slice; every vector keeps its luma and
 * chroma fetches inside the picture; every level is at most 255 in magnitude (8- and 16-bit escapes, player.cpp:1092-1099)
 * and every value the decoder clamps stays in -256..511 (levels are halved until a block fits).  TS output: PID 0x100, one
 * PES (stream id E0, PTS only) per picture, 188-byte packets, the last of a PES padded with adaptation-field stuffing; no
 * sequence_end_code, so that streams can be continued.
 *
 * Motion search: exhaustive over every full-pel vector within +-search that keeps the fetches inside the picture, then the
 * 8 half-pel neighbours of the best one with the decoder's interpolation; search 0 = the zero vector only.
 *
 * Reconstruction contract: recon_device (may be NULL) receives, in I420, exactly what a decoder holds after each picture --
 * dequantisation, the one-coefficient shortcut with its unclamped intra DC, the reference's IDCT rounding, the clamp to 0..248
 * -- at recon_device + (i * n_pictures + p) * 101376.  P pictures are predicted from it.
 *
 * Asynchronous on the context's stream, no host synchronisation, 1 + 2 x n_pictures launches whatever n_streams is.  Stream i
 * appends to dst_device + i * dst_stride and writes nothing outside that region; len_device[i] gets the bytes written by the
 * call, status_device[i] its EFX_ENCODE_* bits (both valid after efx_sync).  A picture that does not fit ends the stream's
 * output after the last whole picture and sets EFX_ENCODE_FULL; other streams go on.  dst_stride >= efx_encode_bound(format,
 * n_pictures) never sets it.  A stream's bytes depend only on its pictures, the options and its continuation state.
 *
 * cont = 1 continues the streams of the previous call: the outputs of the calls concatenated are one stream (the first picture
 * is predicted from the previous call's last reconstruction; GOP phase, temporal_reference, PTS and continuity counter carry
 * on).  qscale and search may change; EFX_ERR_STATE when there was no previous call, n_streams, format or gop differ from
 * the call that started the streams, or a stream of the previous call hit EFX_ENCODE_FULL (known to the host once that call
 * has completed, e.g. after efx_sync; a full stream is never continued on the device either).  Only the streams that cont
would continue count: a region filled before the latest cont = 0 call never refuses it, whether that call has run or not.
 *
 * The encoder's state and scratch (two pictures and twelve worst-case slices per stream) are allocated at the context's first
 * efx_encode, for max_streams streams, and freed by efx_destroy; encoding touches nothing of the decoder.
 * EFX_ERR_ARG: a field out of range, a NULL or misaligned (16 bytes) src / dst / len / status / recon pointer, src_stride
 * below n_pictures x 101376 or not a multiple of 16, dst_stride not a multiple of 16. */
#define EFX_ENCODE_FULL 512u  /* status_device bit: the output region filled up (see above) */
typedef struct efx_encode_opts {
    int n_streams;      /* streams 0 .. n_streams-1 of the context, 1 .. max_streams */
    int n_pictures;     /* pictures per stream in this call, 1 .. 255 */
    int format;         /* EFX_FORMAT_ES or EFX_FORMAT_TS */
    int qscale;         /* quantiser_scale of every slice, 1 .. 31 */
    int gop;            /* an I picture every `gop` pictures of a stream, 1 .. 255 (1 = I pictures only) */
    int search;         /* full-pel motion search radius 0 .. 15; 0 = the zero vector only */
    int cont;           /* 0: every stream starts afresh; 1: continue the streams of the previous efx_encode */
    int64_t first_pts;  /* TS, fresh streams: PTS of picture 0 (90 kHz, 0 .. 2^33-1); picture k carries first_pts + 3003 k at the
                           default picture rate (efx_encode_set_picture_rate below) */
    size_t src_stride;  /* bytes from one stream's pictures to the next (>= n_pictures * 101376, multiple of 16) */
    size_t dst_stride;  /* bytes of output region per stream (multiple of 16) */
} efx_encode_opts;
int efx_encode(efx_ctx* ctx, const efx_encode_opts* opts, const uint8_t* src_device, uint8_t* dst_device, uint32_t* len_device,
               uint32_t* status_device, uint8_t* recon_device);
/* Worst-case bytes of one stream of n_pictures pictures in `format` (0 for invalid arguments).  Host only. */
size_t efx_encode_bound(int format, int n_pictures);

/* -- the encoder's picture rate -- */
/* MPEG-1 codes eight picture rates.  P = 90 kHz ticks per picture, F = the nominal rate the GOP time code counts with:
 *   code   rate         P         F          code   rate         P        F
 *   1      24000/1001   15015/4   24         5      30           3000     30
 *   2      24           3750      24         6      50           1800     50
 *   3      25           3600      25         7      60000/1001   3003/2   60
 *   4      30000/1001   3003      30         8      60           1500     60
 * efx_encode_set_picture_rate sets the rate of the streams that later cont = 0 calls of efx_encode / efx_encode_rc start;
 * a fresh context has code 4.  Streams continued with cont = 1 keep the rate they started with, whatever was set in
 * between.  EFX_ERR_ARG: code outside 1 .. 8 (the rate set before stays).
 *
 * What the rate changes, and nothing else: the sequence header's picture_rate is the code; picture k of a stream carries
 * the PTS (first_pts + floor(k x P)) mod 2^33 -- computed from k, so no rounding accumulates; codes 1 and 7 alternate
 * between two steps (3753 / 3754, 1501 / 1502) --; the GOP header's time code of picture n is n % F pictures, (n / F) % 60
 * seconds and so on, drop_frame 0; and efx_encode_rc's gain per picture (below).  The slices of a picture do not depend on
 * the rate.  The reference decoder reads picture_rate for its drop-frame flag only (src/player.cpp:663,683) and its player
 * paces video by PTS alone (src/video.cpp:1024-1057), so a title plays at the speed its PTS say.
 *
 * efx_picture_pts_offset(code, k) = floor(k x P), host only; -1 for a code outside 1 .. 8 or k outside 0 .. 2^32.
 * efx_picture_rate_code(num, den) = the code whose rate is num / den exactly (any representation: 48/2 is code 2), or 0. */
int efx_encode_set_picture_rate(efx_ctx* ctx, int code);
int64_t efx_picture_pts_offset(int code, int64_t k);
int efx_picture_rate_code(int64_t num, int64_t den);

/* -- encode to a bit rate: one quantiser_scale per picture under a buffer model (k_encode, enc_rate.h) -- */
/* The reference's indexer prepares every title with `-b:v 1500k -maxrate 1500k -bufsize 0.25M -qmin 3`
 * (indexer/indexer.cpp:307-309): a title is playable when its short-term rate stays within what the link delivers into the
 * player's few network buffers.  efx_encode_rc encodes like efx_encode but chooses the quantiser_scale of every picture on
 * the device, per stream, so that the stream follows `bitrate` under the buffer model below.  All twelve slices of a picture
 * carry the same value.
 *
 * The buffer model.  Units are u = 1/90000 bit, in signed 64-bit integers.
 *   capacity            C = vbv_bits x 90000
 *   gain of picture k   G_k = bitrate x (offset(k + 1) - offset(k))   the 90 kHz ticks from picture k's PTS to the next one's
 *                                                   (efx_picture_pts_offset at the streams' picture rate): bitrate x 3003 at the
 *                                                   default rate, two alternating values at codes 1 and 7
 *   cost of a picture   8 x 90000 x bytes           bytes = what the picture appends to the output in `format`: headers plus
 *                                                   slices (ES), its whole 188-byte packets (TS)
 * A fresh stream starts with F = C.  For each picture written:
 *   1. F -= cost
 *   2. if F < 0 the stream gets the status bit EFX_ENCODE_VBV, which stays set for the rest of the call (like
 *      EFX_ENCODE_FULL, it is reported per call)
 *   3. F = min(C, F + G_k): a full buffer stops filling (what -maxrate means for a client that pulls); debt is carried,
 *      not forgiven
 * A picture that is not written because of EFX_ENCODE_FULL changes nothing.  F is carried across cont = 1 calls.
 *
 * The controller (espflix_amd/csrc/enc_rate.h, DESIGN.md "Rate control") decides from F, from what the stream's previous I
 * and P pictures cost per unit of activity, and from the measured activity of the picture about to be coded, so the first
 * P picture after a scene cut is not coded at the quantiser of the easy pictures before it.  Its look-ahead for picture k
 * uses G_k for every picture of its horizon.  Fixed rules:
 *   - the first picture of a fresh stream is coded at clamp(opts->qscale, qmin, qmax);
 *   - a picture that starts with F <= 0 is coded at qmax;
 *   - with qmin == qmax every picture is coded at that value (the bytes are efx_encode's at that qscale).
 * No quantiser changes inside a picture unless adaptive quantisation (below) is on, no picture is coded twice, dropped or
 * repeated; audio is outside the model.
 *
 * qscale_out_device (may be NULL): the quantiser of stream i, picture p at qscale_out_device + i * n_pictures + p; a
 * picture that was not written (EFX_ENCODE_FULL) gets 0.
 *
 * Everything efx_encode documents holds unchanged: asynchronous on the context's stream, no host synchronisation, a stream's
 * bytes depend only on its pictures, the options and its continuation state, EFX_ENCODE_FULL, cont.  1 + 3 x n_pictures
 * launches whatever n_streams is (the activity measure is a launch of its own before each picture's rows).
 * EFX_ERR_ARG, beyond efx_encode's cases: rate NULL, bitrate outside 8000 .. 100000000 bit/s, vbv_bits outside 4000 ..
 * 16000000, qmin / qmax not 1 <= qmin <= qmax <= 31.  EFX_ERR_STATE, beyond efx_encode's cases: cont = 1 with a bitrate or
 * vbv_bits other than those of the call that started the streams; efx_encode_rc continuing streams that efx_encode started,
 * or the reverse.  qmin, qmax, qscale (unused after a stream's first picture) and search may change between calls. */
#define EFX_ENCODE_VBV 4096u  /* status_device bit: the buffer model's level went below zero during the call */
typedef struct efx_encode_rate {
    int bitrate;    /* bit/s of the video bytes as written in `format`, 8000 .. 100000000 */
    int vbv_bits;   /* buffer size in bits, 4000 .. 16000000; the reference's profile: 250000 */
    int qmin, qmax; /* 1 <= qmin <= qmax <= 31; the reference's profile: qmin 3 */
} efx_encode_rate;
int efx_encode_rc(efx_ctx* ctx, const efx_encode_opts* opts, const efx_encode_rate* rate, const uint8_t* src_device,
                  uint8_t* dst_device, uint32_t* len_device, uint32_t* status_device, uint8_t* recon_device,
                  uint8_t* qscale_out_device);

/* -- scene cuts: an I picture where the content changes (k_encode's k_enc_cut, enc_cut.h) -- */
/* efx_encode places an I picture every `gop` pictures and nowhere else, so a hard cut that falls between two of them is
 * coded as a P picture whose search finds nothing, and the first seek point of the new scene is up to gop - 1 pictures
 * into it.  With scene cuts on, the encoder measures every picture against the stream's previous SOURCE picture (not the
 * reconstruction: the decision does not depend on the quantiser or the bit rate) and codes a cut as an I picture, with the
 * sequence and GOP headers every I picture carries -- which makes it a seek point of efx_index_streams.
 *
 * The measure.  Decimated luma D[y][x] = (sum of the 4 x 4 luma pels at (4 y, 4 x) + 8) >> 4, 48 x 88.  For macroblock
 * (r, c), B = the 4 x 4 block of the current D at (4 r, 4 c):
 *   mean = (sum B + 8) >> 4      dev = sum |B - mean|
 *   best = the smallest SAD of B against the previous D at (4 r + dy, 4 c + dx) over |dx|, |dy| <= 4, the candidate block
 *          wholly inside the 48 x 88 picture (the zero vector always is)
 * and for the picture cut_i = sum dev, cut_p = sum min(dev, best) over its 264 macroblocks.  Picture 0 of a fresh stream
 * has no previous picture: cut_p = cut_i.
 *
 * The rule.  g = pictures since the stream's last I picture, counting it (0 on a fresh stream).  A picture is I when it is
 * the stream's first, when g == gop, or when it is a cut:
 *   threshold > 0 && g >= min_gop && cut_p > 8192 && 256 x cut_p > threshold x cut_i
 * Afterwards g = 1 for an I picture, g + 1 otherwise.  temporal_reference is 0 for an I picture and g (before the update)
 * for a P picture; the GOP time code and the PTS still count the stream's pictures.  The floor of 8192 keeps fades from and
 * to black, whose sums are tiny and equal, from counting as cuts.  With threshold 0 the streams are those of efx_encode
 * without this section, byte for byte.  Under efx_encode_rc the controller sees phase 0 for every I picture and g for a P
 * picture; nothing else of it changes.
 *
 * efx_encode_set_scene_cut sets what the streams of later cont = 0 calls of efx_encode / efx_encode_rc start with; NULL
 * or threshold 0 = off, as in a fresh context.  Streams continued with cont = 1 keep what they started with (and the
 * decimated picture and g carry across calls), whatever was set in between.  EFX_ERR_ARG: threshold outside 0 .. 256 or
 * min_gop outside 1 .. 255 (the earlier setting stays).  One more launch per picture while it is on, whatever n_streams is.
 * The two decimated pictures per stream (4224 bytes each) are allocated with the encoder's other state at the first efx_encode.
 *
 * efx_encode_picture_info reports the pictures of the context's latest efx_encode / efx_encode_rc call for one of its
 * streams: it waits for the context's stream, writes min(cap, n_pictures) records to out_host and returns n_pictures.
 * type: 1 = I, 2 = P, 5 = I by the cut rule alone, 0 = not written (EFX_ENCODE_FULL).  cut_i and cut_p are 0 while scene
 * cuts are off.  EFX_ERR_STATE before the context's first encode; EFX_ERR_ARG: stream outside the latest call's, cap < 0,
 * out_host NULL with cap > 0. */
typedef struct efx_scene_cut {
    int threshold;  /* 0 = off, 1 .. 256: a cut needs 256 cut_p > threshold cut_i; 144 separates the cuts of the test clips */
    int min_gop;    /* 1 .. 255: no cut I picture sooner than this many pictures after the last I picture */
} efx_scene_cut;
int efx_encode_set_scene_cut(efx_ctx* ctx, const efx_scene_cut* cut);
typedef struct efx_enc_picture_info {
    uint32_t cut_i, cut_p;
    uint8_t type;
    uint8_t pad[3];
} efx_enc_picture_info;
int efx_encode_picture_info(efx_ctx* ctx, int stream, efx_enc_picture_info* out_host, int cap);

/* -- adaptive quantisation: one quantiser_scale per macroblock (k_encode's k_enc_aq, enc_aq.h) -- */
/* efx_encode and efx_encode_rc code every macroblock of a picture at the picture's quantiser q (opts->qscale, or the
 * controller's choice).  Smooth macroblocks show blocking and banding at a quantiser that textured ones hide.  With
 * adaptive quantisation on, every macroblock gets its own quantiser mq around q from the spatial activity of the SOURCE
 * picture: Test Model 5's activity and normalisation, in integers.
 *
 * Block activity, for each of the four 8 x 8 luma blocks of a macroblock: S = the sum of its 64 pels, m = (S + 32) >> 6,
 * d = sum |p - m|.  Macroblock activity a = 1 + min(d0, d1, d2, d3), 1 .. 8161.  Picture average avg = (A + 132) / 264,
 * A = the sum of a over the picture's 264 macroblocks.  With the strength s, 1 .. 256:
 *   num = (256 + s) a + 256 avg      den = 256 a + (256 + s) avg
 *   mq  = clamp((q num + (den >> 1)) / den, lo, hi)
 * lo, hi = 1, 31 under efx_encode and qmin, qmax under efx_encode_rc.  a == avg gives mq == q; s = 256 is TM5's factor
 * (2 a + avg) / (a + 2 avg), which lies between 1/2 and 2.
 *
 * Each macroblock's six blocks are transformed, quantised, range-checked and reconstructed with its mq.  The slice header
 * carries the mq of the slice's first macroblock; the slice coder keeps a current value, starting there.  A coded
 * macroblock (intra, or with a coded block pattern) whose mq differs from the current value is written with the quant
 * variant of its macroblock_type followed by five bits of mq, which becomes the current value.  A skipped macroblock or
 * one without coded blocks never changes it.  The mode decision, the search, the skip rule, the predictors, the picture
 * headers and scene cuts do not depend on any of this.
 *
 * Under efx_encode_rc the controller decides and updates exactly as without adaptive quantisation, with the picture's q;
 * qscale_out_device reports q; with qmin == qmax the clamp leaves mq == q.  The controller does not price what mq does to
 * a picture's size.  efx_encode_bound holds unchanged (enc_core.h, beside kMbMaxBits).
 *
 * efx_encode_set_adaptive_quant sets what the streams of later cont = 0 calls of efx_encode / efx_encode_rc start with;
 * NULL or strength 0 = off, as in a fresh context, and the streams are then those of the encoder without this section, byte
 * for byte, with the same launches and allocations.  Streams continued with cont = 1 keep what they started with, whatever
 * was set in between.  EFX_ERR_ARG: strength outside 0 .. 256 (the earlier setting stays).  One more launch per picture
 * while it is on, whatever n_streams is.  Its scratch (per stream 528 bytes of activities, twelve sums and 255 maps of 264
 * bytes) is allocated at the first encode with adaptive quantisation on, for max_streams streams, and freed by efx_destroy.
 *
 * efx_encode_mb_quant reports the mq of one picture of the context's latest efx_encode / efx_encode_rc call: it waits for
 * the context's stream and writes 264 bytes to out_host, macroblock (r, c) at 22 r + c; all zero for a picture that was
 * not written (EFX_ENCODE_FULL).  EFX_ERR_STATE before the context's first encode or when the latest call ran with
 * adaptive quantisation off; EFX_ERR_ARG: stream or picture outside the latest call's, out_host NULL. */
typedef struct efx_adaptive_quant {
    int strength;  /* 0 = off, 1 .. 256; 256 = TM5 */
} efx_adaptive_quant;
int efx_encode_set_adaptive_quant(efx_ctx* ctx, const efx_adaptive_quant* aq);
int efx_encode_mb_quant(efx_ctx* ctx, int stream, int picture, uint8_t* out_host);

/* -- fast-forward and rewind streams: which pictures make them (k_trick) ------------------- */
/* A title of the reference is four files: the player opens video_rwd.ts, video.ts and video_fwd.ts by name
 * (src/espflix.cpp:647,787-792) and maps between them with the three records of video.idx (589-628).  The indexer makes
 * the two trick streams with two more ffmpeg runs (indexer/indexer.cpp:308-309): `-g 3 ... -an -filter:v "setpts=PTS/15"`
 * keeps every fifteenth picture in GOPs of 3 without audio, `-vf reverse` turns that stream round.  efx_trick_pick is the
 * selection of both runs on the device, for a batch: it gathers the picked pictures as I420 images, in playing order for
 * the fast-forward encoder and in reverse order for the rewind encoder; efx_encode (gop 3) makes the streams.
 *
 * The rule (espflix_amd/csrc/trick_sel.h).  A title is the pictures t = 0 .. total-1; speed is 1 .. 255 (the reference: 15).
 *   Picture t is picked iff t mod speed == 0; it is pick k = t / speed of the K = ceil(total / speed) picks of the title.
 *   A call offers the pictures t = first_picture + j, j = 0 .. n_pictures-1.  With k0 = ceil(first_picture / speed) it
 *   holds the picks k0 .. k0 + c - 1, c = ceil((first_picture + n_pictures) / speed) - k0, which may be 0.
 *   fwd placement is call-relative: pick k goes to image k - k0 of the fwd region, so the fast-forward stream can be
 *   encoded piece by piece (efx_encode with cont = 1).
 *   rwd placement is title-absolute: pick k goes to image K - 1 - k of the rwd region, because a reversed stream cannot
 *   start before the title has ended; the region holds K images and is complete after the call that offers the last picture.
 *
 * Sources.  EFX_TRICK_FROM_I420: pictures in the layout efx_encode reads, stream i, picture j at src_device + i *
 * src_stride + j * 101376.  EFX_TRICK_FROM_RING: the frame rings; picture j of stream first_stream + i is picture j of the
 * most recent efx_decode* of that stream, and a picked picture is written as the 101376 bytes efx_export_frames with
 * EFX_PIX_I420, slot = -1, picture = j writes for that stream: the same slot arithmetic, read on the device from the record
 * the decode left -- also where export's result is whatever the slot holds (a picture ahead of the first PTS).
 *
 * Stream i's images go to fwd_device + i * fwd_stride and rwd_device + i * rwd_stride, image m at + m * 101376.
 *
 * Memory contract.  Unpicked pictures are never read; a picked picture is read once, also when both destinations are
 * given.  The call writes only the 101376 bytes of every picked image in each region given: the bytes between images,
 * between streams, and the images of picks that belong to other calls are left alone.  The regions must not overlap the
 * source or each other; the call cannot check that.
 *
 * Asynchronous on the context's stream, no host synchronisation: one launch whatever the counts are, none for a call
 * without picks (which returns EFX_OK), and no decoder, encoder, SBC or import state is touched.
 * EFX_ERR_ARG: a field out of range; more than 2^40 picked pictures (n_streams x the call's picks); both destinations
 * NULL; src_device NULL with the I420 source or not NULL with the ring source; a pointer that is not 16-byte aligned; a stride (of a region that is given; src_stride with the I420
 * source) that is too small or not a multiple of 16; total_pictures below first_picture + n_pictures when rwd_device is
 * given.  EFX_ERR_STATE (ring source): no decode yet; the stream range beyond the stream count of the most recent
 * decode; n_pictures >= ring_depth (a picture of the call would already be overwritten).
 *
 * Out of scope: blending or any filtering of the picks (ffmpeg's setpts only drops pictures as well), a rewind stream made
 * piecewise, and the multi-device entry points.  (ffmpeg's frame-rate conform is efx_conform_rate, below.) */
#define EFX_TRICK_FROM_I420 0   /* src_device: pictures in the layout efx_encode reads, stream i at src + i * src_stride */
#define EFX_TRICK_FROM_RING 1   /* the frame rings: picture j of the most recent efx_decode* of streams first_stream + i */
typedef struct efx_trick_opts {
    int n_streams;            /* >= 1 (ring: first_stream + n_streams within the most recent decode's stream count) */
    int n_pictures;           /* pictures per stream offered by this call, >= 1 (ring: <= max_pictures and < ring_depth) */
    int speed;                /* 1 .. 255 */
    int source;               /* EFX_TRICK_FROM_* */
    int first_stream;         /* ring source only, >= 0 */
    int64_t first_picture;    /* title index of the call's picture 0, 0 .. 2^40 - 1 */
    int64_t total_pictures;   /* of the title; read only when rwd_device != NULL; >= first_picture + n_pictures */
    size_t src_stride;        /* I420 source: >= n_pictures x 101376, multiple of 16 */
    size_t fwd_stride;        /* >= the call's picks x 101376, multiple of 16 */
    size_t rwd_stride;        /* >= K x 101376, multiple of 16 */
} efx_trick_opts;
int efx_trick_pick(efx_ctx* ctx, const efx_trick_opts* opts, const uint8_t* src_device /* NULL for the ring */,
                   uint8_t* fwd_device /* may be NULL */, uint8_t* rwd_device /* may be NULL */);
/* The picks a call holds: ceil((first_picture + n_pictures) / speed) - ceil(first_picture / speed).  Host only; -1 for
 * invalid arguments (first_picture outside 0 .. 2^40 - 1, n_pictures outside 0 .. 2^31 - 1, speed outside 1 .. 255). */
int64_t efx_trick_count(int64_t first_picture, int64_t n_pictures, int speed);

/* -- any constant picture rate conformed to a coded one (k_conform) -------------------------- */
/* The encoder keeps the source's picture rate where MPEG-1 can code it (efx_encode_set_picture_rate).  Sources at other
 * rates -- 15, 12.5, 48 or 120 Hz, container rates such as 1000000/41667 -- are conformed first, by dropping and repeating
 * pictures: ffmpeg's `fps` filter with round=near, stated here as this library's own definition.
 *
 * The rule (espflix_amd/csrc/conform_sel.h).  The source runs at r = in_num / in_den Hz, the output at the rate o of
 * out_code (the table above).  Source picture i, shown at time i / r, belongs to output slot floor(i o / r + 1/2); output
 * picture n shows the last source picture whose slot is <= n.  With A : B = in_num x out_den : 2 x out_num x in_den,
 * reduced by their greatest common divisor:
 *   src(n)  = floor(((2 n + 1) A - 1) / B)
 *   Nout(N) = max(0, ceil((N B + 1 - A) / (2 A)))    outputs the stream holds after its first N source pictures
 * Equal rates copy; 50 -> 25 shows 2 n; 15 -> 30 shows floor(n / 2).
 *   A call offers the source pictures first_picture + j, j = 0 .. n_pictures-1, and writes the outputs Nout(first_picture)
 *   .. Nout(first_picture + n_pictures) - 1, which may be none.  The placement is call-relative: output Nout(first_picture)
 *   + m goes to image m.  Every output's source lies inside the call, so pieces need no state, and the outputs of the
 *   pieces of a title, concatenated, are those of one long call.
 *
 * Stream i's pictures at src_device + i * src_stride + j * 101376 (I420, the layout efx_encode reads), its images at
 * dst_device + i * dst_stride + m * 101376.
 *
 * Memory contract.  A dropped source picture is never read, a repeated one is read once per output.  The call writes
 * only the 101376 bytes of every output image: the bytes between images and between streams are left alone.  The regions
 * must not overlap; the call cannot check that.
 *
 * Asynchronous on the context's stream, no host synchronisation: one launch whatever the counts are, none for a call
 * without outputs (which returns EFX_OK), and no decoder, encoder, SBC or import state is touched.
 * EFX_ERR_ARG: a field out of range; a reduced A or B of 2^31 or more; first_picture + n_pictures or an output's index
 * above 2^31 - 1; rates more than 64 : 1 apart, either way; more than 2^40 output pictures (n_streams x the call's
 * outputs); a NULL or misaligned (16 bytes) pointer; a stride that is too small or not a multiple of 16.
 *
 * Out of scope: blending or motion interpolation; a flush of the last partial output period (when the output rate is the
 * lower one, up to one output picture at the end of a title is not produced); the frame rings as source; input whose rate
 * varies; and the multi-device entry points. */
typedef struct efx_conform_opts {
    int n_streams;          /* >= 1 */
    int n_pictures;         /* source pictures per stream offered by this call, >= 1 */
    int32_t in_num, in_den; /* the source's rate in Hz as a fraction, both >= 1 */
    int out_code;           /* the output's rate: picture_rate code 1 .. 8 */
    int64_t first_picture;  /* title index of the call's source picture 0, >= 0 */
    size_t src_stride;      /* >= n_pictures x 101376, multiple of 16 */
    size_t dst_stride;      /* >= the call's outputs x 101376, multiple of 16 */
} efx_conform_opts;
int efx_conform_rate(efx_ctx* ctx, const efx_conform_opts* opts, const uint8_t* src_device, uint8_t* dst_device);
/* The outputs a call holds, Nout(first_picture + n_pictures) - Nout(first_picture) (n_pictures may be 0), and the title
 * index src(n) of the source picture of output n.  Host only; -1 for arguments the call rejects. */
int64_t efx_conform_count(int in_num, int in_den, int out_code, int64_t first_picture, int64_t n_pictures);
int64_t efx_conform_source(int in_num, int in_den, int out_code, int64_t n);

/* -- composite video out (video_init / video_isr, src/video.cpp:572-630,1122-1198) -------- */
typedef struct efx_video_params {
    int line_width, line_count;        /* samples per line, lines per field */
    int hsync, hsync_long, hsync_short;
    int burst_start, burst_width, active_start;
} efx_video_params;
/* geometry video_init(ntsc) establishes: NTSC 912 x 262, PAL 1136 x 312 */
int efx_video_get_params(int ntsc, efx_video_params* out);
/* One field per selected stream: n_streams x line_count x line_width uint16 DAC words into
 * dst (device memory), from ring slot `slot` of streams first_stream..+n.  frame_counter
 * supplies the dither phase (_frame_counter & 1, src/video.cpp:701).  Asynchronous. */
int efx_composite_fields(efx_ctx* ctx, int first_stream, int n_streams, int slot, int ntsc, int frame_counter,
                         uint16_t* dst_device);

/* The same with the two display features of video_isr that involve more than the front frame:
 *  - hscroll: the ease-in / ease-out slide between the two Frames of a pair (_hscroll,
 *    src/video.cpp:1077-1088,1146-1154): a multiple of 8 in (-352, 352); h > 0 shows `slot` from
 *    column h followed by `other_slot` from column 0, h < 0 shows `other_slot` from column
 *    352 + h followed by `slot` from column 0;
 *  - the 80 x 16 time / progress-bar overlay (composite(), src/video.cpp:838-887; the buffer
 *    _video_composite, src/video.h:52-55) on the sixteen lines starting two lines below the
 *    picture: overlay_blend is _video_composite_blend (0 off, -1 or >= 32 full, 1..31 fading --
 *    the caller decrements it once per field as video_isr does, src/video.cpp:1192-1193),
 *    overlay_progress is _video_composite_progress (0..240).
 * overlay (device memory) holds n_streams blocks of 1280 bytes overlay_stride apart, or one
 * block shared by all streams when overlay_stride is 0; NULL with a non-zero blend draws the
 * bar over an all-zero text area. */
typedef struct efx_field_opts {
    int first_stream, n_streams;
    int slot, other_slot;
    int ntsc;
    int frame_counter;
    int hscroll;
    const uint8_t* overlay;
    size_t overlay_stride;
    int overlay_blend;
    int overlay_progress;
} efx_field_opts;
int efx_composite_fields_ex(efx_ctx* ctx, const efx_field_opts* opts, uint16_t* dst_device);

/* -- PDM audio out (pdm_second_order / write_pcm_16, espflix.ino:73-145) ------------------ */
/* n_streams independent modulators.  pcm: n_streams x n_samples int16 (stream-major, device);
 * state: n_streams x 3 int32 (_i0,_i1,_i2; device, updated in place); dst: n_streams x
 * 2*n_samples uint16 (device).  Asynchronous.
 * Alignment: dst_device and state_device must be 4-byte aligned (a sample's two words leave as one
 * 32-bit store; EFX_ERR_ARG otherwise), pcm_device 2-byte aligned.  Streams whose PCM and output
 * both start on a 16-byte boundary are read and written eight samples at a time; any other n_samples
 * or alignment gives the same words, sample by sample. */
int efx_pdm(efx_ctx* ctx, int n_streams, const int16_t* pcm_device, int n_samples, int32_t* state_device,
            uint16_t* dst_device);

/* The audio half of MpegDecoder::demux (src/player.cpp:421-433) for a batch of transport streams:
 * the bytes push_audio() (src/video.h:50, src/video.cpp:1006-1019) would receive -- payloads of PID
 * 0x101 / 0x102 behind the PES header, only while the latest audio PES header carried a PTS -- are
 * written to audio_device + i * stride (device memory, stride >= the longest transport stream) and
 * their count to audio_len_device[i].  Feed efx_sbc_decode from there.  ts / len are host pointers;
 * synchronous. */
int efx_demux_audio(efx_ctx* ctx, int n_streams, const uint8_t* const* ts, const size_t* len, uint8_t* audio_device,
                    size_t stride, uint32_t* audio_len_device);

/* -- trick-play index (indexer/indexer.cpp; ESPFlix::idx_hdr, src/espflix.cpp:573-629) -------- */
/* idx_rec as the indexer writes it (indexer/indexer.cpp:22-28): 28 bytes of fields + 4 of padding */
typedef struct efx_idx_rec {
    int64_t first_pts, last_pts;
    uint32_t bin_size, trick_speed, sample_count;
    uint32_t reserved;
} efx_idx_rec;
/* make_index(src) + pts2seq (indexer/indexer.cpp:86-217) for a batch of transport streams, on the
 * device: every video PES that starts a sequence header contributes (PTS, packet number); each
 * bin of bin_size ticks between the first such PTS and the last video PTS gets the packet number
 * of the nearest one.  recs[i] describes stream i (trick_speed[i] is recorded, 1 if the array is
 * NULL); its samples are written to samples + i * samples_cap.  A stream without a sequence header
 * gets sample_count 0.  efx_idx_rec.first_pts is the PTS of the first sequence start, in stream
 * order, whose PTS is not -1 (a PTS field with a wrong marker nibble parses as -1, a PES without a
 * PTS as 0; indexer.cpp:129-131); -1 if there is none (the bins then start at -1, as the
 * indexer's do).  sample_count is also 0 when last_pts < first_pts.  EFX_ERR_CAPACITY: a stream
 * needs more than samples_cap samples (its sample_count is 0, the other streams' records are
 * complete).  Host pointers; synchronous. */
int efx_index_streams(efx_ctx* ctx, int n_streams, const uint8_t* const* ts, const size_t* len, const uint32_t* trick_speed,
                      uint32_t bin_size, efx_idx_rec* recs, uint32_t* samples, size_t samples_cap);
/* merge_index (indexer/indexer.cpp:219-237): the bytes of video.idx -- 'IDX', 3, the main /
 * fast-forward / rewind records, then their samples.  Returns the size needed; writes only if it
 * fits in cap. */
size_t efx_idx_build(const efx_idx_rec recs[3], const uint32_t* const samples[3], uint8_t* out, size_t cap);
/* idx_hdr::pts2offset and idx_hdr::pts2pts (src/espflix.cpp:597-627) on the 104-byte header of a
 * video.idx: byte offset of the sample to read (get_index, src/espflix.cpp:823-829) for a
 * main-timeline PTS at speed 0 / 1 / -1, and trick-stream PTS -> main-timeline PTS.  The sample,
 * times 188, is the byte offset at which to start efx_upload_streams(EFX_FORMAT_TS). */
uint32_t efx_idx_pts2offset(const void* idx_hdr, int64_t pts, int speed);
int64_t efx_idx_pts2pts(const void* idx_hdr, int64_t pts, int speed);

/* -- SBC audio decode (sbc_decoder, src/sbc_decoder.cpp:346-378; decode_audio, src/video.cpp:962-989) -- */
/* Bytes of decoder state per stream (the reference's SBC_Decode, src/sbc_decoder.h:12-25).  All
 * zero is sbc_init(). */
size_t efx_sbc_state_bytes(void);
#define EFX_SBC_PROBE_FIRST 1 /* decode frame 0 once more up front and drop that PCM: decode_audio()'s
                                 frame-size probe (src/video.cpp:964-972) synthesises the first frame twice */
/* n_streams independent decoders.  frames: n_frames frames of frame_bytes per stream,
 * stream_stride bytes apart (device); state: n_streams x efx_sbc_state_bytes() (device, updated);
 * pcm: per stream pcm_stride int16 apart (device), frames back to back, blocks x 8 x channels
 * samples each with the channel blocks NOT interleaved (src/sbc_decoder.h:27); ret (device, may
 * be NULL): per (stream, frame) sbc_decoder()'s return value in the low 16 bits (0xFFFF = -1) and
 * its decoded byte count in the high 16; pcm_count (device, may be NULL): samples written per
 * stream.  8 subbands, mono / dual / stereo; joint stereo, 4 subbands, a bad sync byte (and a
 * bitpool above 128, which hangs the reference) are rejected exactly as sbc_decoder() does --
 * including its re-synthesis of the previous subband samples.  Asynchronous.
 * Every stream is decoded in chunks of frames that run side by side (espflix_amd/csrc/k_sbc.hip): what the reference
 * chains from frame to frame -- a rejected frame is synthesised from the samples and under the geometry the state holds
 * -- is resolved into prefix scans over the stream's frames first.  `state` must be zeros or what a call left there
 * (the filter memory is multiplied as 24-bit values, which every value a call can leave fits).
 * frame_bytes x n_frames < 2^28 per call (bit positions inside a stream are 32-bit): longer streams take several
 * calls, the state carries over; EFX_ERR_ARG otherwise. */
int efx_sbc_decode(efx_ctx* ctx, int n_streams, const uint8_t* frames_device, size_t stream_stride, int frame_bytes,
                   int n_frames, void* state_device, int16_t* pcm_device, size_t pcm_stride, uint32_t* ret_device,
                   uint32_t* pcm_count_device, int flags);

/* -- SBC audio encode: PCM -> frames the reference decodes (espflix_amd/csrc/k_sbc_enc.hip, sbc_enc_core.h) -- */
/* The inverse of efx_sbc_decode for what the reference decoder accepts and plays like every other SBC decoder: 8 subbands
 * (src/sbc_decoder.cpp:291-292), mono or dual channel.  Not offered: joint stereo (rejected there) and mode 2 "stereo" --
 * its bit_allocation gives every channel the whole bitpool (src/sbc_decoder.cpp:151-232), so a mode-2 frame it plays is
 * not one other decoders play.  The player itself decodes mono frames of at most 16 blocks into a 128-sample buffer
 * (src/video.cpp:978-985) and expects 48 kHz, 16 blocks, 64-byte frames (src/video.cpp:953-987): bitpool 28.
 * A frame: 9C, frequency / blocks / mode / allocation / subbands, bitpool, CRC-8 (x^8+x^4+x^3+x^2+1, initial value 0x0F,
 * over bytes 1 and 2 and the scale factors; the reference ignores it, other decoders check it), 4-bit scale factors, the
 * quantised samples block-major, channel, subband, most significant bit first (get_samples, src/sbc_decoder.cpp:273-341).
 * The analysis is A2DP Appendix B's with the subband samples halved, which is the reference's amplitude convention
 * (a sample is reconstructed inside (-2^scale, 2^scale), src/sbc_decoder.cpp:257-264,330-334): PCM encoded here and decoded
 * by it (or by efx_sbc_decode) returns at unity gain, 73 samples late.  All integer; tests/sbc_enc_model_main.cpp writes
 * the same bytes on the host. */
#define EFX_PCM_FRAME_PLANAR 0  /* what efx_sbc_decode writes: per frame, channel 0's blocks x 8 samples, then channel 1's */
#define EFX_PCM_INTERLEAVED  1  /* L R L R ...; the same as FRAME_PLANAR for mono */
typedef struct efx_sbc_encode_opts {
    int n_streams;     /* 1 .. max_streams */
    int n_frames;      /* frames per stream in this call, >= 1; n_frames x samples per frame < 2^31 */
    int frequency;     /* header field 0..3 = 16 / 32 / 44.1 / 48 kHz (selects the loudness offsets) */
    int blocks;        /* 4, 8, 12, 16 */
    int mode;          /* 0 mono, 1 dual channel */
    int allocation;    /* 0 loudness, 1 SNR */
    int bitpool;       /* 2 .. 128 (above 128 the reference hangs) */
    int pcm_layout;    /* EFX_PCM_* */
    size_t pcm_stride;    /* int16 elements from one stream's PCM to the next, >= n_frames x blocks x 8 x channels */
    size_t frame_stride;  /* bytes from one stream's frames to the next, >= n_frames x frame bytes, a multiple of 16 */
} efx_sbc_encode_opts;
/* 4 + 4 channels + ceil(blocks x channels x bitpool / 8); 0 for arguments efx_sbc_encode rejects.  Host only. */
size_t efx_sbc_frame_bytes(int blocks, int channels, int bitpool);
/* Bytes of encoder state per stream: the last 72 samples of each channel.  All zero = a fresh encoder.  Host only. */
size_t efx_sbc_enc_state_bytes(void);
/* n_streams independent encoders.  pcm (device): stream i at pcm + i x pcm_stride; state (device, updated): n_streams x
 * efx_sbc_enc_state_bytes(); frames (device): stream i's n_frames frames back to back from frames + i x frame_stride --
 * the layout efx_sbc_decode reads (frames, stream_stride, frame_bytes), so one call's output is the other's input.  Bytes
 * between the streams' regions are left alone.  Asynchronous on the context's stream, two launches whatever the counts;
 * touches nothing of the video decoder, the video encoder or the SBC decoder.  A longer stream takes several calls, the
 * state carries the analysis filter's memory over: the frames are those of one long call.
 * EFX_ERR_ARG: a field out of range, mode 2 or 3, a NULL or misaligned (16 bytes) pcm / state / frames pointer, a stride
 * too small or (frame_stride) not a multiple of 16. */
int efx_sbc_encode(efx_ctx* ctx, const efx_sbc_encode_opts* opts, const int16_t* pcm_device, void* state_device,
                   uint8_t* frames_device);

/* -- sound in: PCM of any rate and channel count to the SBC rates, mono (k_import_pcm) ------ */
/* efx_sbc_encode and the player want 48 kHz mono int16 (src/video.cpp:953-987); source audio is 44.1 kHz stereo, 48 kHz
 * 5.1 or 96 kHz.  efx_import_pcm is the `-ar 48000 -ac 1` of the reference indexer's ffmpeg line
 * (indexer/indexer.cpp:307) on the device: it downmixes 1 .. 8 channels to one and resamples 8 .. 192 kHz to one of the
 * SBC header's four rates, for n_streams streams at once, in pieces of any length.
 *
 * Meaning.  With r = in_rate and o = out_rate a stream that has taken N input frames in total has produced
 * ceil(N o / r) output samples, so a call writes ceil((first_in + n_in) o / r) - ceil(first_in o / r) samples per stream
 * (efx_import_pcm_out_samples; possibly 0), at dst + i * dst_stride.  Calls with first_in carried on (first_in += n_in,
 * the same state) give the samples of one long call.  Output n sits at input time n r / o - W, W = efx_import_pcm_delay
 * input frames (16 / out_rate seconds when r <= o: 0.33 ms at 48 kHz): the filter is causal, the tail comes out when the
 * caller feeds W zero frames.  Nothing compensates the delay.
 *
 * The arithmetic (espflix_amd/csrc/import_pcm.h) is an integer function of the source bytes, bit-reproducible anywhere;
 * >> is arithmetic, div and mod are those of non-negative operands, clamp16 clamps to -32768 .. 32767.
 *   Downmix.  m[j] = clamp16((sum over c of w[c] x[j][c] + 16384) >> 15), w = mix_q15, or floor(32768 / channels) each
 *   when all eight are zero.  sum |w| <= 32768, so the sum fits 32 bits.
 *   r == o.  y[n] = m[n]: no filter, no delay, the state is neither read nor written.
 *   Otherwise the prototype is the default design of ffmpeg's resampler, which is what the indexer's line runs: 32 taps
 *   at ratios >= 1, a Kaiser window of beta 9, cutoff 0.97:
 *     p(u) = 0.97 sinc(0.97 u) I0(9 sqrt(1 - (u / 16)^2)) / I0(9) for |u| < 16, 0 from there on   (sinc(x) = sin(pi x) / (pi x))
 *   tabulated as T[i] = round(2^Q p(i / P)), i = 0 .. 16 P (T[16 P] = 0), with P = 512 and Q = 22 (efx_import_pcm_filter).
 *   M = max(r, o), W = ceil(16 M / o) (<= 64 because r <= 4 o).  For output n: a = n r, fl = a div o, and the taps are
 *   j = fl - 2W + 1 .. fl; m[j] of a fresh stream is 0 for j < 0.  For each tap
 *     e = |j o - a + W o|,  q = (e P) div M,  rho = (e P) mod M;   k = 0 when q >= 16 P, else
 *     f = (rho 4096) div M,  k = T[q] + (((T[q + 1] - T[q]) f) >> 12)
 *   acc = sum of k m[j] in 64 bits; when r > o the filter is M / o times as wide and acc = floor(acc o / r);
 *     y[n] = clamp16((acc + 2^(Q - 1)) >> Q)
 *   (the largest sum of |k| over the phases is 2.28 x 2^Q: hence the clamp).  e grows by o from tap to tap, so
 *   (e P 4096) div M = 4096 q + f steps with a carry: no division per tap.
 *
 * State.  efx_import_pcm_state_bytes() = 256 bytes per stream, 16-byte aligned: the 127 newest mixed samples m[first_in -
 * 127 .. first_in - 1] as int16 and one zero; 2W - 1 <= 127 of them are the history the next call's taps reach.  All zero
 * = a fresh stream.
 *
 * Memory contract.  For stream i the kernels read only the n_in x channels int16 elements from src + i * src_stride, in
 * 16-byte pieces aligned down inside that interval (a last piece that would end behind it is read element by element),
 * and write only the call's output samples of stream i.  src_device, state_device and dst_device are 16-byte aligned, the
 * strides are multiples of 8 elements. */
#define EFX_PCM_PLANAR 2  /* efx_import_pcm: channel c of a call's n_in frames at + c * n_in elements */
typedef struct efx_import_pcm_opts {
    int n_streams;        /* 1 .. max_streams */
    int n_in;             /* input sample frames per stream in this call, >= 1; n_in x channels < 2^31 */
    int in_rate;          /* Hz, 8000 .. 192000, and in_rate <= 4 * out_rate */
    int out_rate;         /* 16000, 32000, 44100 or 48000 (the SBC header's four) */
    int channels;         /* 1 .. 8 */
    int layout;           /* EFX_PCM_INTERLEAVED: frames of `channels` samples; EFX_PCM_PLANAR: channel c at + c * n_in elements */
    int mix_q15[8];       /* downmix weights; all zero = floor(32768 / channels) each; sum of |w| over the channels <= 32768 */
    int64_t first_in;     /* index in the stream of this call's first input frame (0 on a fresh stream), 0 .. 2^40 - 1 */
    size_t src_stride;    /* int16 elements between streams, >= n_in * channels, multiple of 8 */
    size_t dst_stride;    /* int16 elements between streams, >= the call's output count, multiple of 8 */
} efx_import_pcm_opts;
/* Asynchronous on the context's stream: no host synchronisation, at most two launches whatever the counts (the outputs;
 * the hand-over of the history, a launch of its own because the last tile must not overwrite what the first still reads;
 * none for a call without output samples, one when the rates are equal), so calls with different rates may be queued
 * back to back.  No decoder, encoder or SBC state is touched.  state_device may be NULL when the rates are equal.
 * EFX_ERR_ARG: a field out of range, n_in x channels >= 2^31, in_rate > 4 out_rate, an out_rate that is not one of the
 * four, an unknown layout, sum |w| > 32768, first_in negative or >= 2^40, a NULL or misaligned (16 bytes) pointer, a stride
 * that is too small or not a multiple of 8. */
int efx_import_pcm(efx_ctx* ctx, const efx_import_pcm_opts* opts, const int16_t* src_device, void* state_device,
                   int16_t* dst_device);
/* ceil((first_in + n_in) o / r) - ceil(first_in o / r); -1 for rates, a first_in or an n_in (< 0) that efx_import_pcm
 * rejects or a count above 2^31 - 1.  Host only. */
int efx_import_pcm_out_samples(int in_rate, int out_rate, int64_t first_in, int n_in);
/* W, in input frames; 0 when the rates are equal; -1 for rates efx_import_pcm rejects.  Host only. */
int efx_import_pcm_delay(int in_rate, int out_rate);
/* 256.  Host only. */
size_t efx_import_pcm_state_bytes(void);
/* The table T: copies min(cap, length) entries to out (may be NULL with cap 0) and returns the length, 16 P + 1.  Host only. */
int efx_import_pcm_filter(int32_t* out, int cap);

/* -- programme loudness and levelling (k_loudness.hip) ------------------------------------------- */
/* The reference plays sound through a 1-bit pin at a fixed gain (pdm_second_order, src/video.cpp), so a title is as loud
 * as its source was.  These calls measure the loudness of mono int16 PCM at the four SBC rates -- what efx_import_pcm
 * writes and efx_sbc_encode reads -- by ITU-R BS.1770-4 / EBU R 128 for n_streams streams at once: gated integrated
 * loudness, maximum momentary loudness and sample peak (ffmpeg's ebur128); derive one gain per stream for a target
 * loudness under a peak ceiling (loudnorm in linear mode); and apply it (volume) -- all on the device, the gain never
 * visits the host.  Sample peak with a ceiling of -1 dBFS stands in for true peak: no oversampling.  Not measured: true
 * peak, loudness range, short-term loudness.  A title whose peaks cap that one gain goes through the peak limiter of the
 * next section (efx_limit_peaks, efx_pcm_limit) in efx_pcm_gain's place; there is no compressor and no dynamic mode.
 *
 * Meaning.  step = rate / 10 samples (100 ms: 1600, 3200, 4410, 4800), W = step / 2.  Step s of a stream covers samples
 * s step .. (s + 1) step - 1.  Its energy is DEFINED by a K-weighting filter that starts at rest at sample s step - W and
 * runs over the W + step samples up to the step's end (samples in front of the stream's first are zero); only the step's
 * own samples are measured.  The high pass's double pole at 38 Hz has a time constant of 4 ms, so after 50 ms the step's
 * energy is that of a filter with the whole history to within a few 1e-8 (tests/test_loudness_model.py measures it against
 * a serial float64 evaluation); in exchange every (stream, step) is independent work.
 *
 * The arithmetic (espflix_amd/csrc/loudness_px.h) is an integer function of the samples, bit-reproducible anywhere; >> is
 * arithmetic, floor() of non-negative operands, int32 / int64 / uint64 as stated.
 *   Coefficients (efx_loudness_coefs).  Both stages from their analogue prototypes by the bilinear transform, in double on
 *   the host, each rounded to an int32 as round(2^28 c).  With K = tan(pi f0 / rate):
 *     shelf:     f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; Vh = 10^(G / 20),
 *                Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2:
 *                b0 = (Vh + Vb K / Q + K^2) / a0, b1 = 2 (K^2 - Vh) / a0, b2 = (Vh - Vb K / Q + K^2) / a0,
 *                a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0
 *     high pass: f0 = 38.13547087602444, Q = 0.5003270373238773: b = 1, -2, 1 exactly, a1, a2 as above with these K, Q
 *   (at 48 kHz: the coefficients BS.1770 prints).  out[0 .. 4] = b0 b1 b2 a1 a2 of the shelf, out[5 .. 9] of the high pass.
 *   Recurrence, direct form I, all values int32 with 12 fraction bits, products and sums int64:
 *     x0 = 4096 x[n]
 *     y[n] = (b0 x0[n] + b1 x0[n-1] + b2 x0[n-2] - a1 y[n-1] - a2 y[n-2] + 2^27) >> 28     (shelf)
 *     z[n] = (b0' y[n] + b1' y[n-1] + b2' y[n-2] - a1' z[n-1] - a2' z[n-2] + 2^27) >> 28    (high pass)
 *   (|y|, |z| < 3.4 x 2^27 and a sum of products < 2^61 for any input: tests/test_loudness_model.py).
 *   Step energy (uint64).  s[n] = (z[n] + 128) >> 8 keeps four fraction bits; E = sum of s[n]^2 over the step's samples.
 *   Step peak.  The largest |x[n]| of the step's samples, 32768 for -32768.
 *   Blocks.  B_j = E_j + E_j+1 + E_j+2 + E_j+3, j = 0 .. n_steps - 4: 400 ms, 75 % overlap; fewer than 4 steps: no block.
 *   Gates.  Absolute: B_j > abs_thr; n_abs of them, S_abs their sum (up to 80 bits).  Relative: 10 B_j n_abs > S_abs among
 *   those; n_gated of them, S_gated their sum.  gated_mean = floor(S_gated / n_gated), 0 when n_gated = 0 (the sum itself
 *   passes 64 bits after some ten minutes of full scale, so the record carries the mean); max_block = the largest B_j of
 *   all blocks.  efx_loudness_lufs turns a block energy -- gated_mean: integrated, max_block: maximum momentary -- into LUFS.
 *   Gain.  T = target_ms, C = ceiling (efx_loudness_thresholds), peak = the largest step peak (and state sample):
 *     g = floor(sqrt(min(floor(2^24 T 4 step / gated_mean), 2^32)))         (128-bit dividend)
 *     g = min(g, floor(4096 C / peak)), then clamped to 1 .. 32767          (Q12: just under +18 dB)
 *     g = 4096 when n_gated = 0 or peak = 0.
 *   (The first line, clamped to 1 .. 32767 and 4096 when n_gated = 0, is the stream gain G of the peak limiter:
 *   efx_limit_gain.)
 *   Apply.  y = clamp16((x g + 2048) >> 12); g = 4096 returns x.
 *
 * State.  efx_loudness_state_bytes(rate) per stream, 16-byte aligned: the newest H = (W + step + 7) & ~7 samples of the
 * stream as int16, oldest first (zeros in front of a stream's first sample): the pending samples of the unfinished step
 * and the run-in before them.  All zero = a fresh stream.
 *
 * Memory contract.  efx_loudness_steps reads, for stream i, only the n_samples int16 from pcm + i * pcm_stride, in 16-byte
 * pieces aligned down inside that interval (a last piece that would end behind it element by element), and the stream's
 * state; it writes only the call's new step records, 16 bytes each with one store, and the state.  efx_loudness_gate reads
 * n_steps records per stream (and the states) and writes 32 bytes per stream.  efx_pcm_gain reads and writes only the
 * n_samples samples of each stream and reads gain_q12 of each record.  All device pointers are 16-byte aligned, the sample
 * strides are multiples of 8 elements.  No decoder, encoder or SBC state is touched; every call is asynchronous on the
 * context's stream without host synchronisation, so steps -> gate -> gain -> efx_sbc_encode queue back to back. */
typedef struct efx_loudness_step {   /* one 100 ms step */
    uint64_t energy;                 /* E */
    uint32_t peak;                   /* 0 .. 32768 */
    uint32_t zero;
} efx_loudness_step;
typedef struct efx_loudness_rec {    /* one stream, 32 bytes */
    uint64_t gated_mean;             /* floor(S_gated / n_gated): the integrated loudness as a block energy; 0: nothing passed */
    uint64_t max_block;              /* the largest block: maximum momentary loudness */
    uint32_t n_gated;                /* blocks above both gates */
    uint32_t n_blocks;               /* max(n_steps - 3, 0) */
    uint32_t n_abs;                  /* blocks above the absolute gate */
    uint16_t peak;                   /* sample peak, 0 .. 32768 */
    uint16_t gain_q12;               /* 1 .. 32767 */
} efx_loudness_rec;
typedef struct efx_loudness_steps_opts {
    int n_streams;        /* 1 .. max_streams */
    int n_samples;        /* samples per stream in this call, >= 1 */
    int rate;             /* 16000, 32000, 44100 or 48000 */
    int first_step;       /* records already written for these streams: the call's first new record goes to index first_step */
    int64_t first_sample; /* index in the stream of this call's first sample (0 on a fresh stream), 0 .. 2^40 - 1 */
    size_t pcm_stride;    /* int16 elements between streams, >= n_samples, multiple of 8 */
    size_t steps_stride;  /* records between streams, >= first_step + the call's new steps */
} efx_loudness_steps_opts;
/* Appends, per stream, every step that becomes whole with this call's samples -- efx_loudness_step_count(rate,
 * first_sample, n_samples) records, possibly 0 -- at steps + i * steps_stride + first_step, and returns that count (>= 0).
 * Pieces of any length: calls with first_sample and first_step carried on and the same state give the records of one long
 * call.  At most two launches (the records; the hand-over of the state, a launch of its own because the last wave must not
 * overwrite what the first still reads).  Errors are negative.
 * EFX_ERR_ARG: n_streams, n_samples, first_step or first_sample out of range, a rate that is not one of the four, a NULL
 * or misaligned (16 bytes) pointer, pcm_stride too small or not a multiple of 8, steps_stride too small. */
int efx_loudness_steps(efx_ctx* ctx, const efx_loudness_steps_opts* opts, const int16_t* pcm_device, void* state_device,
                       efx_loudness_step* steps_device);
typedef struct efx_loudness_gate_opts {
    int n_streams;        /* 1 .. max_streams */
    int n_steps;          /* records per stream, 0 .. 2^24 */
    int rate;
    uint64_t abs_thr;     /* efx_loudness_thresholds */
    uint64_t target_ms;   /* below 2^40 */
    uint32_t ceiling;     /* 1 .. 32767 */
    size_t steps_stride;  /* records between streams, >= n_steps */
} efx_loudness_gate_opts;
/* One efx_loudness_rec per stream at recs + i.  state_device may be NULL; given, every sample of the streams' states
 * counts towards the peak: they all belong to the stream, and with n_steps = all its whole steps the peak is then that of
 * every sample it has taken, the pending ones included.  One launch.
 * EFX_ERR_ARG: a field out of range, a rate that is not one of the four, a NULL steps / recs pointer, a misaligned
 * (16 bytes) pointer, steps_stride too small. */
int efx_loudness_gate(efx_ctx* ctx, const efx_loudness_gate_opts* opts, const efx_loudness_step* steps_device,
                      const void* state_device, efx_loudness_rec* recs_device);
typedef struct efx_pcm_gain_opts {
    int n_streams;        /* 1 .. max_streams */
    int n_samples;        /* samples per stream, >= 1 */
    int fixed_gain_q12;   /* 1 .. 32767: every stream's gain when recs_device is NULL (else ignored) */
    size_t src_stride;    /* int16 elements between streams, >= n_samples, multiples of 8 */
    size_t dst_stride;
} efx_pcm_gain_opts;
/* dst[i][n] = clamp16((src[i][n] g_i + 2048) >> 12), g_i = recs[i].gain_q12 read on the device.  dst_device == src_device
 * (with equal strides) works in place; otherwise the two must not overlap.  One launch.  The records are those
 * efx_loudness_gate wrote (gain_q12 1 .. 32767): the kernel takes the field as it finds it and cannot report a bad one, so a
 * record the caller made up with gain_q12 = 0 -- a zeroed one -- silences its stream.
 * EFX_ERR_ARG: a field out of range (fixed_gain_q12 only without records), a NULL or misaligned (16 bytes) src / dst, a
 * misaligned recs, a stride too small or not a multiple of 8. */
int efx_pcm_gain(efx_ctx* ctx, const efx_pcm_gain_opts* opts, const int16_t* src_device, const efx_loudness_rec* recs_device,
                 int16_t* dst_device);
/* -0.691 + 10 log10(block_energy / (4 step 32768^2 256)) LUFS; -HUGE_VAL for 0 (nothing passed the gates); NaN for a rate
 * that is not one of the four.  The only logarithm.  Host only. */
double efx_loudness_lufs(uint64_t block_energy, int rate);
/* abs_thr = round(10^((-70 + 0.691) / 10) 32768^2 256 x 4 step), target_ms = round(10^((target_lufs + 0.691) / 10)
 * 32768^2 256), ceiling = round(32767 x 10^(peak_dbfs / 20)).  EFX_ERR_ARG for a rate that is not one of the four,
 * target_lufs outside -70 .. 0 or peak_dbfs outside -90 .. 0.  Host only. */
int efx_loudness_thresholds(int rate, double target_lufs, double peak_dbfs, uint64_t* abs_thr, uint64_t* target_ms,
                            uint32_t* ceiling);
/* The ten coefficients; EFX_ERR_ARG for a rate that is not one of the four.  Host only. */
int efx_loudness_coefs(int rate, int32_t out[10]);
/* 2 H: 4800, 9600, 13232 or 14400; 0 for a rate that is not one of the four.  Host only. */
size_t efx_loudness_state_bytes(int rate);
/* floor((first_sample + n_samples) / step) - floor(first_sample / step); -1 for arguments efx_loudness_steps rejects.
 * Host only. */
int efx_loudness_step_count(int rate, int64_t first_sample, int n_samples);

/* -- peak limiter (k_limit.hip) -------------------------------------------------------------------- */
/* efx_pcm_gain gives a stream ONE gain, min(loudness gain, floor(4096 C / peak)): a single loud sample anywhere caps the
 * gain of the whole title, and a peaky title stays far under its target.  The limiter applies the full loudness gain G
 * everywhere and reduces it smoothly around the samples that would pass the ceiling (ffmpeg's alimiter behind volume).
 * It looks ahead and behind by whole windows and has NO recurrence -- a sliding minimum followed by a box average, not an
 * attack / release envelope follower -- so every block of a stream is independent work and pieces equal one long call.
 * Sample peak, as in the section above: no oversampling, true peak is not measured.  No compressor, no dynamic mode.
 * The limited title lands slightly UNDER the target, by the energy of what was limited (about 1.3 LU on a title whose
 * bursts would otherwise have cost 9 LU: tests/test_limit_model.py); no second measuring pass trims that shortfall.
 *
 * The rule (espflix_amd/csrc/limit_px.h; tests/limit_model.py restates it), in exact integers; >> is arithmetic, floor()
 * of non-negative operands:
 *   Block length.  Bk = 16, 32, 48, 48 samples at 16000, 32000, 44100, 48000 Hz (efx_limit_block): about 1 ms, a whole
 *   number of 32-byte pieces.  Block b of a stream holds samples b Bk .. b Bk + Bk - 1; the last may be partial.
 *   Block peak.  p[b] = the largest |x| of the block's samples, 32768 for -32768, a uint16_t; blocks in front of the
 *   stream and behind it have p = 0.
 *   Stream gain G (Q12, 1 .. 32767).  floor(sqrt(min(floor(2^24 T 4 step / gated_mean), 2^32))) clamped to 1 .. 32767,
 *   4096 when n_gated = 0: the loudness gain of the section above without its peak cap (efx_limit_gain), worked out on
 *   the device from the stream's efx_loudness_rec with T = target_ms; or fixed_gain_q12 when no records are given.
 *   Required gain.  r[b] = G where p[b] = 0, else min(G, floor(4096 C / p[b])), C = ceiling 1 .. 32767; r may be 0.
 *   Then |x| r <= 4096 C, so (x r + 2048) >> 12 lies in -C .. C.
 *   Nodes.  Node b is the border between blocks b - 1 and b: q[b] = min(r[b - 1], r[b]).
 *   Smoothing.  With the half window H (1 .. 64 blocks, default 32) and W = 2 H + 1:
 *     M[j] = min(q[j - H] .. q[j + H]),  a[b] = floor((M[b - H] + .. + M[b + H]) / W).
 *   Every M of the sum has q[b] inside its window, so a[b] <= q[b].
 *   Gain of sample n of block b, t = n - b Bk:  g = floor((a[b] (Bk - t) + a[b + 1] t) / Bk)  <= r[b].
 *   Output.  y = clamp16((x g + 2048) >> 12); the clamp never acts.
 * Two consequences.  Where no block has r < G the output is efx_pcm_gain's with gain G, bit for bit.  The samples of
 * blocks b0 .. b1 - 1 depend on the peaks of blocks b0 - 2 H - 1 .. b1 + 2 H and on nothing else.
 *
 * Pieces.  The block grid is anchored at stream sample 0 and there is no state: a piece begins at a multiple of Bk and
 * every piece but a stream's last is a whole number of blocks.  A title takes two passes, as for efx_pcm_gain: the first
 * measures (efx_loudness_steps) and takes the peaks (efx_limit_peaks) of every piece; after efx_loudness_gate the second
 * limits every piece (efx_pcm_limit).  The caller keeps the peaks: the whole title's row (2 bytes per millisecond), or for
 * each piece the 2 H + 1 blocks either side of it as far as the stream has them.
 *
 * Memory contract.  efx_limit_peaks reads, for stream i, only the n_samples int16 from pcm + i * pcm_stride and writes only
 * the ceil(n_samples / Bk) entries from peaks + i * peaks_stride + first_sample / Bk - peaks_first.  efx_pcm_limit reads only
 * the n_samples samples of each stream, entries 0 .. n_peaks - 1 of each row and gated_mean and n_gated of each record, and
 * writes only the n_samples samples of each stream: bytes of a row behind n_samples stay as they were.  Samples go in
 * 16-byte pieces, a last partial piece element by element.  All device pointers are 16-byte aligned, the sample strides
 * are multiples of 8 elements.  Both calls are one launch each, asynchronous on the context's stream, without allocation
 * or host synchronisation: steps -> gate -> peaks -> limit -> efx_sbc_encode queue back to back. */
typedef struct efx_limit_peaks_opts {  /* fixed-width fields only */
    int32_t n_streams;      /* 1 .. max_streams */
    int32_t n_samples;      /* samples per stream in this call, >= 1; a multiple of Bk on every piece but a stream's last */
    int32_t rate;           /* 16000, 32000, 44100 or 48000 */
    int32_t reserved;
    int64_t first_sample;   /* index in the stream of this call's first sample: a multiple of Bk, 0 .. 2^40 - 1 */
    int64_t peaks_first;    /* the stream block that entry 0 of a row holds, 0 .. first_sample / Bk */
    uint64_t pcm_stride;    /* int16 elements between streams, >= n_samples, multiple of 8 */
    uint64_t peaks_stride;  /* entries between rows, >= first_sample / Bk - peaks_first + ceil(n_samples / Bk) */
} efx_limit_peaks_opts;
/* p of the call's blocks: entry first_sample / Bk - peaks_first of stream i's row receives its first block's peak.  One
 * launch; it reads the samples only.
 * EFX_ERR_ARG: n_streams, n_samples, first_sample or peaks_first out of range, first_sample not a multiple of Bk, a rate
 * that is not one of the four, a NULL or misaligned (16 bytes) pointer, pcm_stride too small or not a multiple of 8,
 * peaks_stride too small. */
int efx_limit_peaks(efx_ctx* ctx, const efx_limit_peaks_opts* opts, const int16_t* pcm_device, uint16_t* peaks_device);
typedef struct efx_limit_opts {        /* fixed-width fields only */
    int32_t n_streams;      /* 1 .. max_streams */
    int32_t n_samples;      /* samples per stream in this call, >= 1 */
    int32_t rate;           /* 16000, 32000, 44100 or 48000 */
    int32_t half_window;    /* H in blocks, 1 .. 64; 0 = 32 */
    int32_t ceiling;        /* C, 1 .. 32767 (efx_loudness_thresholds) */
    int32_t fixed_gain_q12; /* 1 .. 32767: every stream's G when recs_device is NULL (else ignored) */
    int32_t n_peaks;        /* entries of a row, >= 1; a block outside the row counts as p = 0 */
    int32_t reserved;
    int64_t first_sample;   /* index in the stream of this call's first sample: a multiple of Bk, 0 .. 2^40 - 1 */
    int64_t peaks_first;    /* the stream block that entry 0 of a row holds, 0 .. 2^40 - 1 */
    uint64_t target_ms;     /* T, below 2^40 (efx_loudness_thresholds); used with recs_device */
    uint64_t src_stride;    /* int16 elements between streams, >= n_samples, multiples of 8 */
    uint64_t dst_stride;
    uint64_t peaks_stride;  /* entries between rows, >= n_peaks */
} efx_limit_opts;
/* dst[i][n] = the rule's y for stream i's samples first_sample .. first_sample + n_samples - 1, G_i from recs[i] on the
 * device (or fixed_gain_q12), the peaks those an earlier efx_limit_peaks left.  dst_device == src_device (with equal
 * strides) works in place -- the peaks were taken by the earlier launch, so no workgroup reads what another writes --
 * otherwise the two must not overlap.  One launch.  It queues behind efx_loudness_gate and in front of efx_sbc_encode.
 * EFX_ERR_ARG: n_streams, n_samples, half_window, ceiling, n_peaks, first_sample or peaks_first out of range, first_sample
 * not a multiple of Bk, target_ms (with records) or fixed_gain_q12 (without) out of range, a rate that is not one of the
 * four, a NULL or misaligned (16 bytes) src / peaks / dst, a misaligned recs, a sample stride too small or not a multiple
 * of 8, peaks_stride below n_peaks, dst_device == src_device with unequal sample strides. */
int efx_pcm_limit(efx_ctx* ctx, const efx_limit_opts* opts, const int16_t* src_device, const uint16_t* peaks_device,
                  const efx_loudness_rec* recs_device, int16_t* dst_device);
/* Bk: 16, 32, 48 or 48; 0 for a rate that is not one of the four.  Host only. */
int efx_limit_block(int rate);
/* G of a stream from the fields of its efx_loudness_rec; 0 for a rate that is not one of the four or target_ms >= 2^40.
 * Host only. */
int efx_limit_gain(uint64_t gated_mean, uint32_t n_gated, uint64_t target_ms, int rate);

/* -- A/V multiplexer: video transport stream + SBC frames -> a title (espflix_amd/csrc/k_mux.hip) -- */
/* The reference player takes its audio from PES packets on PID 0x101 / 0x102 of the transport stream that carries the
 * video on PID 0x100 (MpegDecoder::demux, src/player.cpp:421-433).  Output, byte for byte (tests/mux_model.py restates it):
 *  - audio PES: 00 00 01 C0, PES_packet_length = 8 + payload (the player compares it with what arrived,
 *    src/player.cpp:390-396,431-432), 80 80 05, the 5-byte PTS of the PES's first frame, then frames_per_pes frames (the
 *    last PES of a call may hold fewer); 188-byte packets on audio_pid, payload_unit_start on the first, the continuity
 *    counter running on from audio_cc, the last packet padded with adaptation-field stuffing as efx_encode pads video;
 *  - the unit of interleaving is a PES: its packets stay together, video packets are copied unchanged.  Units appear in
 *    PTS order, audio first at equal PTS, the order inside each kind kept; a video PES without PTS counts as having its
 *    predecessor's (before the first PTS: as earlier than all audio); audio later than the last video PES follows it.
 *    Nothing is unwrapped at 2^33: a video PTS is compared as written (its 33 bits), an audio PTS as audio_first_pts +
 *    floor(frame x samples_per_frame x 90000 / sample_rate) BEFORE it is masked to the 33 bits that are written.  Audio PTS
 *    therefore never decrease (the placement is a binary search over them), and once they pass 2^33 the remaining audio
 *    PES count as later than every video PES and follow the last one, whatever the video's wrapped PTS say;
 *  - no PAT / PMT: the reference player does not read them (its own clips carry them on PIDs 0 and 0x1000, it skips them). */
#define EFX_MUX_FULL      1024u  /* status bit: the output region is too small; the stream's length is 0 */
#define EFX_MUX_BAD_VIDEO 2048u  /* status bit: video_len not a multiple of 188, a packet without 0x47 or not on PID 0x100,
                                    or a first packet that does not start a PES; the stream's length is 0 */
typedef struct efx_mux_opts {
    int n_streams;            /* 1 .. max_streams */
    int audio_pid;            /* 0x101 or 0x102 (the reference's own clips use 0x102) */
    int frame_bytes;          /* SBC frame size */
    int n_frames;             /* audio frames per stream in this call, >= 0 */
    int frames_per_pes;       /* >= 1; frames_per_pes x frame_bytes <= 2048: half the player's 4 KiB audio ring (src/video.cpp:957) */
    int samples_per_frame;    /* blocks x 8 */
    int sample_rate;          /* Hz */
    int64_t audio_first_pts;  /* 90 kHz PTS of frame 0 of the title */
    int64_t audio_first_frame;/* index in the title of this call's first frame: frame k of the call carries
                                 audio_first_pts + floor((audio_first_frame + k) x samples_per_frame x 90000 / sample_rate) */
    int audio_cc;             /* continuity counter of the first audio packet, 0..15 */
    size_t video_stride, audio_stride, dst_stride;   /* bytes between streams; multiples of 16 */
} efx_mux_opts;
/* video_ts / video_len (device) are what efx_encode(EFX_FORMAT_TS) left in dst_device / len_device: the lengths are read on
 * the device, so encode -> mux needs no host synchronisation.  audio_frames (device): stream i's frames at
 * audio_frames + i x audio_stride (may be NULL when n_frames is 0).  The title of stream i goes to dst + i x dst_stride, its
 * length to len[i], EFX_MUX_* bits (0 = fine) to status[i]; a stream with a status bit set has length 0 and its region is not
 * written.  Stateless: a title made in several calls passes audio_first_frame and audio_cc on (efx_mux_audio_packets).
 * Asynchronous on the context's stream, one launch.  EFX_ERR_ARG: a field out of range, a stride that is not a multiple of
 * 16 (dst_stride: or 2^32 and above), audio_stride below n_frames x frame_bytes, a NULL or misaligned (16 bytes) pointer. */
int efx_mux_av(efx_ctx* ctx, const efx_mux_opts* opts, const uint8_t* video_ts_device, const uint32_t* video_len_device,
               const uint8_t* audio_frames_device, uint8_t* dst_device, uint32_t* len_device, uint32_t* status_device);
/* A dst_stride that never gives EFX_MUX_FULL for video_bytes of video (0 for invalid arguments).  Host only. */
size_t efx_mux_bound(size_t video_bytes, int n_frames, int frame_bytes, int frames_per_pes);
/* Audio packets efx_mux_av writes per stream: add to audio_cc (mod 16) for the next call (-1 for invalid arguments).  Host only. */
int efx_mux_audio_packets(int n_frames, int frame_bytes, int frames_per_pes);

/* -- measurement -------------------------------------------------------------------------- */
typedef struct efx_timing {
    float index_ms, parse_ms, recon_ms, total_ms; /* HIP-event stage times, mean over the efx_decode calls
                                                     since efx_set_timing(ctx, 1) (at most the last 64) */
    uint64_t pictures, slices, coefficients, es_bytes;
    float demux_ms;    /* k_demux of the last EFX_FORMAT_TS upload (0 for ES input or timing off at upload) */
    uint32_t timed_calls; /* efx_decode calls averaged in the stage times */
    uint64_t ts_bytes; /* transport-stream bytes of the last upload */
    uint32_t groups;   /* reconstruction groups of the newest call: one k_recon launch per group and picture index; the
                          stage times above are sums over them */
    uint16_t parse_halves; /* parse halves (k_index ... k_parse over a group's streams, on the parse streams) of the newest call:
                              one per reconstruction group, so always equal to `groups` */
    uint16_t mixed;    /* 1: the averaged calls did not all run with the newest call's structure (a call that found the GPU
                          idle is split into groups, one queued behind another is not): per-launch figures derived from
                          the means are off */
    uint32_t recon_launches; /* reconstruction kernel launches of the newest call: groups x pictures */
} efx_timing;
/* Enable HIP-event timing of the decode stages (events recorded on the kernels' own streams);
 * enabling (again) starts a new averaging window. */
int efx_set_timing(efx_ctx* ctx, int enable);
int efx_get_timing(efx_ctx* ctx, efx_timing* out);

/* Launch structure.  Results never depend on it; by default part of it follows what the GPU is doing when a call is
 * queued (a call that finds the reconstruction stream idle is split into groups and its parse kernel is not capped), so the
 * same call sequence can run as different launches from run to run.  Benchmarks and tests pin it. */
typedef enum efx_option {
    EFX_OPT_GROUPS = 1,      /* reconstruction groups per efx_decode: 0 = automatic (above), n >= 1 = always n */
    EFX_OPT_PARSE_CAP = 2,   /* k_parse's residency cap: 0 = only while reconstruction is queued, 1 = always, 2 = never */
    EFX_OPT_SBC_SERIAL = 7   /* 1 = efx_sbc_decode runs every stream through the one-wave-per-stream kernel (the comparison the tests
                                run the frame-parallel kernels against); 0 = default */
    /* The numbers 3, 4, 5, 6 and 8 are not reused: 3 ... 6 drove a single-launch reconstruction and 8 selected a one-pass
     * demultiplexer, both measured slower and removed (tools/exp/rejected/README.md).  efx_set_option and efx_get_option
     * return EFX_ERR_ARG for them. */
} efx_option;
/* Debugging aid of the guard-page allocator (EFX_GUARD=1 / 2 in the environment: every device buffer of the library and of
 * efx_device_alloc becomes its own mapping that ends -- mode 2: starts -- on an unmapped page, so that a kernel reading or
 * writing past a buffer faults at once): writes one word at `offset_bytes` from the start of a buffer (negative: in front of
 * it).  tools/guard_selftest.py uses it to show that the allocator catches what it is there to catch. */
int efx_debug_poke(efx_ctx* ctx, void* dptr, size_t bytes, long long offset_bytes);
int efx_set_option(efx_ctx* ctx, int option, int value);
int efx_get_option(efx_ctx* ctx, int option, int* value);

/* -- several devices of one node ----------------------------------------------------------------- */
/* The reference decodes one stream on one core; its batch form here shards by STREAM and nothing else (SURVEY.md 8e,
 * BASELINE.json north_star): streams are independent, so stream k of a batch of n goes to device floor(k * R / n) of
 * the R devices -- contiguous blocks -- and no collective touches the data path.  An efx_multi owns one efx_ctx and one
 * host thread per device (a HIP context is bound to the thread that drives it); every call below fans out to the
 * devices, each working on its own block, and returns when all of them have QUEUED (decode) or FINISHED (upload,
 * sync, queries) their part.  The per-device contexts are the ordinary ones: efx_multi_context(m, r) hands out device
 * r's for everything this section does not wrap (composite fields, PDM, timing ...), to be used from the caller's
 * thread only while no efx_multi_* call is in flight.  What MpegDecoder::run() is to one stream
 * (src/player.cpp:1355-1367) efx_multi_decode is to a node's worth of them. */
/* NUMA placement of a device's host side (host only, no device call): the node sysfs publishes for a PCI device
 * ("0000:c1:00.0", as hipDeviceGetPCIBusId prints it; -1 = unknown / single node), that node's CPUs, and binding the
 * CALLING thread to them (returns how many CPUs the new mask holds, 0 = left alone: unknown node, or none of its CPUs are
 * available to this process).  efx_multi_create binds each device's worker thread this way before the thread creates its
 * context -- its pinned staging buffers are then first touched on the device's own node -- unless EFX_NUMA=0.  A
 * one-process-per-GPU launcher calls efx_numa_bind_thread itself before efx_create (bench.py does, per rank). */
int efx_numa_node_of_pci(const char* pci_bus_id);
int efx_numa_cpus_of_node(int node, int* cpus, int cap);
int efx_numa_bind_thread(int node);

typedef struct efx_multi efx_multi;
/* first stream of part `part` when `total` streams are dealt to `parts` devices: ceil(part * total / parts); part ==
 * parts gives total.  Pure function (no device needed): the partition the multi-device calls and bench.py use. */
int efx_partition_first(int total, int parts, int part);
/* cfg->max_streams is the PER-DEVICE capacity, cfg->device is ignored; devices[r] = HIP ordinal of device r. */
int efx_multi_create(const efx_config* cfg, const int* devices, int n_devices, efx_multi** out);
void efx_multi_destroy(efx_multi* m);
int efx_multi_device_count(const efx_multi* m);
efx_ctx* efx_multi_context(efx_multi* m, int r);
const char* efx_multi_last_error(const efx_multi* m);
/* efx_upload_streams for a batch of n_streams <= n_devices x max_streams streams, dealt as above */
int efx_multi_upload_streams(efx_multi* m, int n_streams, const uint8_t* const* data, const size_t* len, int format);
/* where stream k of the last upload lives: device index and its index in that device's batch */
int efx_multi_locate(const efx_multi* m, int stream, int* device_index, int* local_stream);
int efx_multi_decode(efx_multi* m);  /* efx_decode on every device; asynchronous */
int efx_multi_sync(efx_multi* m);
int efx_multi_reset(efx_multi* m);
/* per stream of the last upload, in batch order: pictures decoded, status bits (either pointer may be NULL) */
int efx_multi_results(efx_multi* m, int* n_pictures, uint32_t* status);
/* efx_frame_hashes of every stream of the last upload, in batch order: out[n_streams][ring_depth] */
int efx_multi_frame_hashes(efx_multi* m, uint64_t* out);

/* raw device allocations for callers without their own allocator (bench, tests) */
int efx_device_alloc(efx_ctx* ctx, size_t bytes, void** dptr);
int efx_device_free(efx_ctx* ctx, void* dptr);
int efx_memcpy_h2d(efx_ctx* ctx, void* dst_device, const void* src, size_t bytes);
int efx_memcpy_d2h(efx_ctx* ctx, void* dst, const void* src_device, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* EFX_H */
