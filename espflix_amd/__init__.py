"""espflix_amd -- Python host binding (ctypes) for libefx, the MI355X-native espflix hot path.

This package is a thin mirror of the C-ABI in include/efx.h (which in turn stands in for the
reference's MpegDecoder / Frame / push_video / video_isr / write_pcm_16 surface, reference
src/player.h:34-165, src/video.h:36-50, src/video.cpp:1122, espflix.ino:123).  All work happens
in hand-written HIP kernels inside espflix_amd/libefx.so; there is NO CPU fallback: importing
works anywhere, but creating a Decoder without the built library or without a gfx950 device
raises immediately.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

# the C-ABI's structs, record dtypes and signatures live in _abi.py; they are part of this module's surface
from ._abi import (DENOISE_OPTS_DTYPE, ENC_PICTURE_INFO_DTYPE, LIMIT_OPTS_DTYPE, LIMIT_PEAKS_OPTS_DTYPE, LOUDNESS_REC_DTYPE, LOUDNESS_STEP_DTYPE, SCAN_FRAME_DTYPE,  # noqa: F401
                   OVERLAY_EVENT_DTYPE, OVERLAY_OPTS_DTYPE, SCAN_OPTS_DTYPE, SCAN_REC_DTYPE, TELECINE_INFO, _P, _SYMBOLS,
                   _AdaptiveQuant, _CompareOpts, _CompareRec, _Config, _ConformOpts, _CropOpts, _DeintOpts, _DetelecineOpts,
                   _EncodeOpts, _EncodeRate, _EncPictureInfo, _ExportOpts, _FieldOpts, _IdxRec, _ImportColour, _ImportHdr,
                   _ImportOpts, _ImportPcmOpts, _LoudnessGateOpts, _LoudnessStepsOpts, _MuxOpts, _PcmGainOpts, _SbcEncodeOpts,
                   _SceneCut, _Surface, _Timing, _TrickOpts, _VideoParams)

FRAME_WIDTH = 352
FRAME_HEIGHT = 192
FRAME_STRIDE = 528
STRIP_ROWS = 16
STRIPS = 12
STRIP_BYTES = 8448
FRAME_BYTES = 101376

OPT_GROUPS, OPT_PARSE_CAP, OPT_SBC_SERIAL = 1, 2, 7   # efx_option (3 ... 6 and 8 belonged to removed paths and are refused)
SBC_PROBE_FIRST = 1
PIX_I420, PIX_RGB24, PIX_RGBP = 0, 1, 2     # efx_pixel_format
CHROMA_NEAREST, CHROMA_BILINEAR = 0, 1
_PIX_FORMATS = {"i420": PIX_I420, "rgb24": PIX_RGB24, "rgbp": PIX_RGBP}
_CHROMA_MODES = {"nearest": CHROMA_NEAREST, "bilinear": CHROMA_BILINEAR}
FORMAT_ES = 0
FORMAT_TS = 1

STREAM_BAD_SIZE = 1
STREAM_TRUNCATED = 2
STREAM_TOO_MANY_UNITS = 4
STREAM_BAD_VLC = 8
STREAM_MB_OVERRUN = 16
STREAM_COEF_OVERRUN = 32
STREAM_SERIAL_HUNT = 64   # the reference would misread bits between two start codes (its marker hunt is bit-serial): see efx.h
STREAM_SLICE_ORDER = 128  # slice start codes of a picture not strictly rising in bitstream order: see efx.h
ENCODE_FULL = 512         # efx_encode: the stream's output region filled up (efx.h)
ENCODE_VBV = 4096         # efx_encode_rc: the buffer model's level went below zero during the call (efx.h)
SCENE_CUT_DEFAULT = 144   # scene_cut=True: the threshold that separates the cuts of the test clips (profiles/scene_cut.md)
PICTURE_I, PICTURE_P, PICTURE_CUT_I = 1, 2, 5   # efx_enc_picture_info.type
AQ_DEFAULT = 256          # aq=True: Test Model 5's factor (profiles/adaptive_quant.md)
MUX_FULL = 1024           # efx_mux_av: the stream's output region is too small, nothing written (efx.h)
MUX_BAD_VIDEO = 2048      # efx_mux_av: the video input is not a transport stream of PID 0x100 that starts with a PES (efx.h)
OVERLAY_BAD_EVENT = 8192  # efx_overlay: the list holds an event that is not valid; it was not drawn (efx.h)
OVL_A8, OVL_RGBA = 0, 1   # efx_overlay_event.kind
OVERLAY_MAX_EVENTS = 4096
PCM_FRAME_PLANAR, PCM_INTERLEAVED = 0, 1   # efx_sbc_encode_opts.pcm_layout
PCM_PLANAR = 2                             # efx_import_pcm_opts.layout (or PCM_INTERLEAVED)
TRICK_FROM_I420, TRICK_FROM_RING = 0, 1    # efx_trick_opts.source
_PCM_LAYOUTS = {"interleaved": PCM_INTERLEAVED, "planar": PCM_PLANAR}
_SBC_FREQUENCY = {16000: 0, 32000: 1, 44100: 2, 48000: 3}  # the SBC header's code of efx_import_pcm's output rates

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EFX_LIB") or os.path.join(_HERE, "libefx.so")  # EFX_LIB: development builds


class EfxError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libefx status {status}: {message}")
        self.status = status


@dataclass
class CompareResult:
    """Quality of pictures against a reference (Decoder.compare; the definition: include/efx.h).  Axis -1: Y, Cb, Cr."""
    sse: np.ndarray        # (..., 3) uint64: sum of squared errors of each plane
    ssim_q16: np.ndarray   # (..., 3) int64: sum over the plane's windows of the Q16 SSIM
    psnr: np.ndarray       # (..., 3) float64: 10 log10(255^2 samples / sse), inf for sse 0
    ssim: np.ndarray       # (..., 3) float64: ssim_q16 / (65536 x windows)
    mb_sse: object = None  # (..., 12, 22) uint32: luma SSE of every macroblock, when asked for


@dataclass
class LoudnessResult:
    """Programme loudness of mono PCM streams by ITU-R BS.1770-4 / EBU R 128 (Decoder.loudness; the definition:
    include/efx.h).  One entry per stream."""
    integrated: np.ndarray     # float64 LUFS: gated integrated loudness, -inf where no block passed the gates
    momentary_max: np.ndarray  # float64 LUFS: the loudest 400 ms block, -inf without a block (or all silence)
    peak_dbfs: np.ndarray      # float64: sample peak, -inf for silence
    gain_db: np.ndarray        # float64: 20 log10(gain_q12 / 4096)
    gain_q12: np.ndarray       # int32: the gain that takes the stream to the target under the peak ceiling
    n_blocks: np.ndarray       # int64: 400 ms blocks
    n_gated: np.ndarray        # int64: blocks above both gates


@dataclass
class ScanResult:
    """The scan type of one stream (Decoder.detect_scan, scan_verdict; the definition: include/efx.h, "scan type")."""
    kind: str              # "progressive", "interlaced", "telecined" or "unknown"
    first_field: object    # "top" or "bottom" for "interlaced" and "telecined", else None
    rec: np.ndarray        # the stream's counts: a SCAN_REC_DTYPE record


@dataclass
class EncodeResult:
    streams: list          # bytes written per stream by the call
    status: np.ndarray     # EFX_ENCODE_* bits per stream
    recon: object = None   # (n, P, 101376) reconstruction (torch tensor or NumPy array), when asked for
    qscales: object = None  # (n, P) uint8 array: every picture's quantiser_scale (0 = not written), when bitrate is given
    types: object = None   # (n, P) uint8 array: 1 = I, 2 = P, 5 = I placed by the scene-cut rule alone, 0 = not written
    cut_scores: object = None  # (n, P, 2) uint32 array: every picture's (cut_i, cut_p) (efx.h "scene cuts"; 0 while they are off)
    quality: object = None  # CompareResult of shape (n, P): the reconstruction against the source (ref_max=248), with quality=True


_lib = None


def load_library() -> C.CDLL:
    """Load libefx.so and bind every entry point; raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make lib` (or __graft_entry__.build()); "
                          "espflix_amd has no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the C-ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def video_params(ntsc: bool) -> dict:
    """Geometry video_init(ntsc) establishes (reference src/video.cpp:572-630)."""
    p = _VideoParams()
    _check(None, load_library().efx_video_get_params(1 if ntsc else 0, C.byref(p)))
    return {n: getattr(p, n) for n, _ in _VideoParams._fields_}


def idx_build(recs3, samples3) -> bytes:
    """merge_index: video.idx bytes from three (rec dict, samples) results of Decoder.index_streams."""
    lib = load_library()
    recs = (_IdxRec * 3)(*[_IdxRec(**r) for r in recs3])
    arrs = [np.ascontiguousarray(s, dtype=np.uint32) for s in samples3]
    ptrs = (_P * 3)(*[a.ctypes.data for a in arrs])
    n = lib.efx_idx_build(recs, ptrs, None, 0)
    out = np.zeros(n, dtype=np.uint8)
    assert lib.efx_idx_build(recs, ptrs, out.ctypes.data, n) == n
    return out.tobytes()


def idx_pts2offset(idx: bytes, pts: int, speed: int) -> int:
    h = np.frombuffer(idx[:104], dtype=np.uint8).copy()
    return int(load_library().efx_idx_pts2offset(h.ctypes.data, pts, speed))


def idx_pts2pts(idx: bytes, pts: int, speed: int) -> int:
    h = np.frombuffer(idx[:104], dtype=np.uint8).copy()
    return int(load_library().efx_idx_pts2pts(h.ctypes.data, pts, speed))


def export_bytes(fmt) -> int:
    """Bytes of one exported image ("i420", "rgb24", "rgbp" or an EFX_PIX_* value; 0 for an unknown format)."""
    return int(load_library().efx_export_bytes(_PIX_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)))


def _export_shape(fmt: str, n: int):
    return {"i420": (n, FRAME_BYTES), "rgb24": (n, FRAME_HEIGHT, FRAME_WIDTH, 3), "rgbp": (n, 3, FRAME_HEIGHT, FRAME_WIDTH)}[fmt]


def i420_planes(t):
    """(Y, U, V) views of exported I420 images: a flat (n, 101376) tensor / array -> (n, 192, 352), (n, 96, 176) twice
    (a single image of 101376 bytes -> the same without the leading axis).  U is Cb, V is Cr."""
    lead = tuple(t.shape[:-1])
    y_bytes, c_bytes = FRAME_WIDTH * FRAME_HEIGHT, FRAME_WIDTH * FRAME_HEIGHT // 4
    y = t[..., :y_bytes].reshape(lead + (FRAME_HEIGHT, FRAME_WIDTH))
    u = t[..., y_bytes:y_bytes + c_bytes].reshape(lead + (FRAME_HEIGHT // 2, FRAME_WIDTH // 2))
    v = t[..., y_bytes + c_bytes:].reshape(lead + (FRAME_HEIGHT // 2, FRAME_WIDTH // 2))
    return y, u, v


def import_src_bytes(fmt, width: int, height: int) -> int:
    """Bytes of one source image of efx_import_frames ("i420", "rgb24", "rgbp" or an EFX_PIX_* value); 0 for an unknown
    format, a width or height outside 2 .. 4096, or an odd I420 size."""
    code = _PIX_FORMATS.get(fmt, -1) if isinstance(fmt, str) else int(fmt)
    return int(load_library().efx_import_src_bytes(code, width, height))


# the source matrices of efx_import_set_colour by name: H.273 matrix_coefficients codes ("auto": 2, unspecified)
_COLOUR_MATRICES = {"bt709": 1, "auto": 2, "fcc": 4, "bt601": 6, "smpte240m": 7, "bt2020": 9}
_COLOUR_RANGES = {"studio": 0, "full": 1}


def _colour_setting(matrix, src_range):
    """(matrix code, full_range) of matrix= / src_range= as the import methods take them; None when neither is given.
    matrix None beside a src_range means BT.601: the range alone is converted."""
    if matrix is None and src_range is None:
        return None
    if isinstance(matrix, str):
        if matrix not in _COLOUR_MATRICES:
            raise ValueError(f"unknown matrix {matrix!r}: one of {sorted(_COLOUR_MATRICES)}, an H.273 code or None")
        matrix = _COLOUR_MATRICES[matrix]
    if src_range is not None and src_range not in _COLOUR_RANGES:
        raise ValueError(f"unknown src_range {src_range!r}: 'studio' or 'full'")
    return (6 if matrix is None else int(matrix)), _COLOUR_RANGES[src_range or "studio"]


def colour_coefs(matrix, src_range: str = "studio", height: int = 0):
    """The conversion an import applies to a YCbCr source of this matrix ("bt601", "bt709", "fcc", "smpte240m", "bt2020",
    "auto" or an H.273 matrix_coefficients code; "auto" and 2 mean BT.709 above 576 lines of height, else BT.601) and
    range ("studio" or "full"): (on, q, y0) with on False for "off" (BT.601 studio swing already), q the nine
    coefficients in steps of 2^-14, row major, and y0 the source's black (efx_import_colour_coefs; the arithmetic:
    include/efx.h).  Raises ValueError for a matrix the library rejects.  Host only."""
    code, full = _colour_setting(matrix, src_range)
    q, y0 = (C.c_int32 * 9)(), C.c_int()
    rc = load_library().efx_import_colour_coefs(code, full, height, q, C.byref(y0))
    if rc < 0:
        raise ValueError(f"matrix {matrix!r} is not one the import converts (H.273 codes 1, 2, 4, 5, 6, 7, 9)")
    return bool(rc), [int(v) for v in q], int(y0.value)


def colour_source_limit(limit: int, src_range: str = "studio") -> int:
    """Crop detection reads source luma, and a full-range source's black is 0, not 16: the largest source luma whose
    converted value (the chroma terms at zero) is <= limit, which is the limit to detect with.  limit itself for
    "studio", 9 for limit=24 and "full"; 0 when even luma 0 converts to more than limit.  Host only."""
    if src_range not in _COLOUR_RANGES:
        raise ValueError(f"unknown src_range {src_range!r}: 'studio' or 'full'")
    if src_range == "studio":
        return limit
    _, q, y0 = colour_coefs("bt601", src_range)
    return max((y for y in range(256) if min(255, max(0, 16 + ((q[0] * (y - y0) + 8192) >> 14))) <= limit), default=0)


# efx_import_set_hdr by name: H.273 transfer_characteristics and colour_primaries codes
_HDR_TRANSFERS = {"pq": 16, "smpte2084": 16}
_HDR_PRIMARIES = {"bt2020": 9, "bt709": 1}
HDR_GAMMA_ENTRIES, _HDR_GAMMA_SLOTS = 1217, 1224   # the second table's entries and its padded size (espflix_amd/csrc/hdr_px.h)


def _hdr_setting(transfer, primaries, matrix, src_range, peak_nits):
    """The five ints of an efx_import_hdr from transfer= / primaries= / matrix= / src_range= / peak_nits= as the import
    methods take them (names or H.273 codes; primaries and matrix None: BT.2020, peak None: 1000); None when transfer is
    None.  The library checks the codes."""
    if transfer is None:
        if primaries is not None or peak_nits is not None:
            raise ValueError("primaries= and peak_nits= describe an HDR source: pass transfer='pq' with them")
        return None
    if isinstance(transfer, str):
        if transfer not in _HDR_TRANSFERS:
            raise ValueError(f"unknown transfer {transfer!r}: 'pq' or the H.273 code 16")
        transfer = _HDR_TRANSFERS[transfer]
    if isinstance(primaries, str):
        if primaries not in _HDR_PRIMARIES:
            raise ValueError(f"unknown primaries {primaries!r}: one of {sorted(_HDR_PRIMARIES)} or an H.273 code")
        primaries = _HDR_PRIMARIES[primaries]
    code, full = _colour_setting("bt2020" if matrix is None else matrix, src_range)
    return int(transfer), 9 if primaries is None else int(primaries), code, full, 1000 if peak_nits is None else int(peak_nits)


def hdr_tables(peak_nits: int = 1000, primaries="bt2020", matrix="bt2020", src_range: str = "studio", height: int = 0,
               transfer="pq") -> dict:
    """Everything the HDR stage of an import reads for a setting (efx_import_hdr_tables; the arithmetic: include/efx.h,
    "HDR sources"): {"matrix": [qy, qrv, qgu, qgv, qbu], "y0", "gamut": nine Q14 coefficients, "peak_nits", "pq": the
    first table (uint32, n + 1 entries: PQ code i / n -> display light relative to 100 nits in steps of 2^-24), "gamma":
    the second (uint16, 1217 entries: inverse BT.1886 in steps of 2^-15), "raw": the bytes as the kernel reads them}.
    Raises ValueError for a setting the library rejects.  Host only."""
    h = _ImportHdr(*_hdr_setting(transfer, primaries, matrix, src_range, peak_nits))
    lib = load_library()
    size = lib.efx_import_hdr_tables(C.byref(h), height, None, 0)
    if size < 0:
        raise ValueError("not an HDR setting the import converts: transfer 16 (PQ), primaries 9 or 1, a matrix of colour_coefs(), "
                         "peak_nits 0 or 200 .. 10000")
    raw = np.zeros(size, dtype=np.uint8)
    if lib.efx_import_hdr_tables(C.byref(h), height, raw.ctypes.data, size) != size:
        raise ValueError("efx_import_hdr_tables failed")
    k = raw[:64].view(np.int32)
    pq_bytes = size - 64 - 2 * _HDR_GAMMA_SLOTS   # the first table: 2^n + 1 entries padded by three
    pq = raw[64:64 + pq_bytes].view(np.uint32)[:pq_bytes // 4 - 3]
    gam = raw[64 + pq_bytes:].view(np.uint16)
    return {"matrix": [int(v) for v in k[:5]], "y0": int(k[5]), "gamut": [int(v) for v in k[6:15]], "peak_nits": int(k[15]),
            "pq": pq.copy(), "gamma": gam[:HDR_GAMMA_ENTRIES].copy(), "raw": raw}


# efx_surface_kind: the conventional layouts of decoders' surfaces (the 16-bit kinds hold uint16 samples)
_SURFACE_KINDS = {"i420": 0, "yv12": 1, "nv12": 2, "nv21": 3, "p010": 4, "p012": 5, "p016": 6, "i010": 7, "i012": 8, "i016": 9}
SURF_PLANAR8, SURF_SEMI8, SURF_PLANAR16, SURF_SEMI16 = 0, 1, 2, 3  # efx_surface.layout


def surface_layout(kind: str, width: int, height: int, pitch: int = 0, plane_rows: int = 0) -> _Surface:
    """The efx_surface of a decoder's picture (efx_surface_layout): kind "i420", "yv12", "nv12", "nv21", "p010", "p012",
    "p016", "i010", "i012" or "i016", Y at 0 with `pitch` bytes per row (0 = packed rows) and plane_rows rows per luma
    plane (0 = height), the chroma plane(s) behind it; .bytes is the extent of one image.  The fields may be edited, for
    a decoder with other offsets or for one field of an interlaced picture.  Host only."""
    if kind not in _SURFACE_KINDS:
        raise ValueError(f"unknown surface kind {kind!r}: one of {sorted(_SURFACE_KINDS)}")
    s = _Surface()
    if not load_library().efx_surface_layout(_SURFACE_KINDS[kind], width, height, pitch, plane_rows, C.byref(s)):
        raise ValueError(f"no {kind} surface of {width} x {height} with pitch {pitch} and {plane_rows} plane rows "
                         "(even sizes 2 .. 4096, pitch >= a row and <= 2^20, even plane_rows >= height)")
    return s


def _surface_source(src, kind, width, height, pitch, plane_rows):
    """(surface, n, src as (n, bytes) uint8) of import_pictures' / detect_crop's source when fmt is a surface kind."""
    if width is None or height is None:
        raise ValueError(f"a {kind} source needs width= and height=")
    surf = surface_layout(kind, width, height, pitch, plane_rows)
    shape = tuple(src.shape)
    if isinstance(src, np.ndarray):
        wide = src.dtype == np.uint16
    else:
        import torch
        wide = isinstance(src, torch.Tensor) and src.dtype == torch.uint16
    if wide and surf.layout not in (SURF_PLANAR16, SURF_SEMI16):
        raise ValueError(f"a {kind} source holds bytes, not uint16 samples")
    if len(shape) != 2 or shape[1] * (2 if wide else 1) != surf.bytes:
        raise ValueError(f"a {kind} source of this geometry must have shape (n, {surf.bytes}) uint8" +
                         (f" or (n, {surf.bytes // 2}) uint16" if surf.layout in (SURF_PLANAR16, SURF_SEMI16) else "") + f", got {shape}")
    if wide:  # the same memory as bytes (little endian)
        src = np.ascontiguousarray(src).view(np.uint8) if isinstance(src, np.ndarray) else src.contiguous().view(torch.uint8)
    return surf, shape[0], src


def letterbox_rect(width: int, height: int):
    """The destination rectangle (x, y, w, h) of fit="letterbox" for a source (or crop) of width x height: the largest
    rectangle of that aspect ratio with even sides inside 352 x 192, centred.  Integer rule: where width * 192 >=
    height * 352 the rectangle is 352 wide and floor(352 * height / width) high, otherwise 192 high and
    floor(192 * width / height) wide; that side is rounded down to even and is at least 16; x = (352 - w) // 2 and
    y = (192 - h) // 2, each rounded down to even.  Host only."""
    if width < 1 or height < 1:
        raise ValueError("width and height must be positive")
    if width * FRAME_HEIGHT >= height * FRAME_WIDTH:
        w, h = FRAME_WIDTH, max(16, (FRAME_WIDTH * height // width) & ~1)
    else:
        w, h = max(16, (FRAME_HEIGHT * width // height) & ~1), FRAME_HEIGHT
    return ((FRAME_WIDTH - w) // 2) & ~1, ((FRAME_HEIGHT - h) // 2) & ~1, w, h


def cover_crop(width: int, height: int, region=None):
    """The crop (x, y, w, h) of fit="cover": the largest centred rectangle of the frame's 11 : 6 shape inside region =
    (x, y, w, h) of a width x height picture (None: the whole picture).  Integer rule: where w * 192 >= h * 352 the
    height stays and w' = floor(h * 352 / 192) rounded down to even, otherwise the width stays and h' =
    floor(w * 192 / 352) rounded down to even; x' = x + (((w - w') >> 1) & ~1), and y' likewise: an even step from the
    region's corner, centred to within one.  cover_crop(1280, 546) == (140, 0, 1000, 546).  Host only."""
    x, y, w, h = region or (0, 0, width, height)
    if w < 1 or h < 1 or x < 0 or y < 0 or x + w > width or y + h > height:
        raise ValueError(f"region {(x, y, w, h)} is not a rectangle of a {width} x {height} picture")
    if w * FRAME_HEIGHT >= h * FRAME_WIDTH:
        cw, ch = (h * FRAME_WIDTH // FRAME_HEIGHT) & ~1, h
    else:
        cw, ch = w, (w * FRAME_HEIGHT // FRAME_WIDTH) & ~1
    if cw < 1 or ch < 1:
        raise ValueError(f"region {(x, y, w, h)} is too thin for a rectangle of the frame's shape")
    return x + (((w - cw) >> 1) & ~1), y + (((h - ch) >> 1) & ~1), cw, ch


def _import_geometry(shape, fmt, width, height):
    """(fmt, n, width, height) of import_pictures' source from its shape."""
    shape = tuple(shape)
    if fmt is None:
        if len(shape) == 4:
            fmt = "rgb24" if shape[3] == 3 else "rgbp"
        elif len(shape) == 2:
            fmt = "i420"
        else:
            raise ValueError(f"cannot infer the pixel format from shape {shape}")
    if fmt not in _PIX_FORMATS:
        raise ValueError(f"unknown format {fmt!r}: one of {sorted(_PIX_FORMATS)}")
    if fmt == "i420":
        if width is None or height is None:
            raise ValueError("an i420 source needs width= and height=")
        if len(shape) != 2 or shape[1] != width * height * 3 // 2:
            raise ValueError(f"an i420 source must have shape (n, {width * height * 3 // 2}), got {shape}")
        return fmt, shape[0], width, height
    if len(shape) != 4 or shape[3 if fmt == "rgb24" else 1] != 3:
        raise ValueError(f"a {fmt} source must have shape " + ("(n, H, W, 3)" if fmt == "rgb24" else "(n, 3, H, W)") + f", got {shape}")
    h, w = (shape[1], shape[2]) if fmt == "rgb24" else (shape[2], shape[3])
    if (width is not None and width != w) or (height is not None and height != h):
        raise ValueError(f"width= / height= disagree with shape {shape}")
    return fmt, shape[0], w, h


COMPARE_SAMPLES = (67584, 16896, 16896)   # samples of the Y, Cb and Cr plane (efx_compare_psnr)


def compare_psnr(sse: int, samples: int = COMPARE_SAMPLES[0]) -> float:
    """10 log10(255^2 samples / sse) of a plane's sum of squared errors (efx_compare_psnr); inf for sse 0.  Host only."""
    return float(load_library().efx_compare_psnr(int(sse), int(samples)))


def compare_ssim(total: int, plane: int = 0) -> float:
    """The mean SSIM of a plane (0 = Y, 1 / 2 = chroma) from its Q16 sum (efx_compare_ssim); NaN for another plane.
    Host only."""
    return float(load_library().efx_compare_ssim(int(total), int(plane)))


def _compare_result(recs: np.ndarray, lead: tuple, mb=None) -> CompareResult:
    """recs: (n, 6) uint64 records as downloaded."""
    sse = np.ascontiguousarray(recs[:, :3])
    q = np.ascontiguousarray(recs[:, 3:]).view(np.int64)
    psnr = np.array([[compare_psnr(v, COMPARE_SAMPLES[p]) for p, v in enumerate(row)] for row in sse.tolist()], dtype=np.float64)
    ssim = np.array([[compare_ssim(v, p) for p, v in enumerate(row)] for row in q.tolist()], dtype=np.float64)
    return CompareResult(sse.reshape(*lead, 3), q.reshape(*lead, 3), psnr.reshape(*lead, 3), ssim.reshape(*lead, 3),
                         None if mb is None else mb.reshape(*lead, 12, 22))


def encode_bound(fmt: int, n_pictures: int) -> int:
    """Worst-case bytes of one encoded stream of n_pictures pictures (efx_encode_bound; 0 for invalid arguments)."""
    return int(load_library().efx_encode_bound(fmt, n_pictures))


def trick_count(first_picture: int, n_pictures: int, speed: int) -> int:
    """Picks among the pictures first_picture .. first_picture + n_pictures - 1 of a title at `speed` (every speed-th picture
    of the title, counted from picture 0): ceil((first_picture + n_pictures) / speed) - ceil(first_picture / speed)
    (efx_trick_count; -1 for invalid arguments)."""
    return int(load_library().efx_trick_count(first_picture, n_pictures, speed))


# the picture rates MPEG-1 codes (picture_rate 1 .. 8; include/efx.h)
PICTURE_RATES = {1: Fraction(24000, 1001), 2: Fraction(24), 3: Fraction(25), 4: Fraction(30000, 1001), 5: Fraction(30),
                 6: Fraction(50), 7: Fraction(60000, 1001), 8: Fraction(60)}
_FLOAT_RATES = {23.976: PICTURE_RATES[1], 29.97: PICTURE_RATES[4], 59.94: PICTURE_RATES[7]}


def _rate(fps) -> Fraction:
    """A picture rate given as Fraction, "num/den", int or float (23.976, 29.97 and 59.94 mean the x/1001 rates)."""
    if isinstance(fps, bool) or fps is None:
        raise ValueError(f"not a picture rate: {fps!r}")
    if isinstance(fps, float):
        f = _FLOAT_RATES[fps] if fps in _FLOAT_RATES else Fraction(repr(fps))
    else:
        f = Fraction(fps)
    if f <= 0:
        raise ValueError(f"not a picture rate: {fps!r}")
    return f


def picture_rate_code(fps) -> int:
    """The MPEG-1 picture_rate code (1 .. 8) whose rate is exactly fps, or 0 (efx_picture_rate_code)."""
    f = _rate(fps)
    if f.numerator >= 1 << 63 or f.denominator >= 1 << 63:
        return 0
    return int(load_library().efx_picture_rate_code(f.numerator, f.denominator))


def _fps_code(fps) -> int:
    """fps= of the encode calls as a code: None = 30000/1001; a rate MPEG-1 does not code is a ValueError."""
    if fps is None:
        return 4
    code = picture_rate_code(fps)
    if not code:
        raise ValueError(f"fps={fps!r} is not a rate MPEG-1 codes: one of {', '.join(str(r) for r in PICTURE_RATES.values())} "
                         "(conform other rates first: fps_out=, Decoder.conform)")
    return code


def picture_pts_offset(fps, k: int) -> int:
    """90 kHz ticks from picture 0 to picture k of a stream encoded at fps: floor(k x 90000 / fps)
    (efx_picture_pts_offset; -1 for k outside 0 .. 2^32)."""
    return int(load_library().efx_picture_pts_offset(_fps_code(fps), k))


def conform_count(fps_in, fps_out, first_picture: int, n_pictures: int) -> int:
    """Output pictures of a conform call that offers the source pictures first_picture .. first_picture + n_pictures - 1 of
    a title at fps_in for an output at fps_out, a coded rate (efx_conform_count; -1 for arguments the call rejects)."""
    f = _rate(fps_in)
    if f.numerator >= 1 << 31 or f.denominator >= 1 << 31:
        return -1
    return int(load_library().efx_conform_count(f.numerator, f.denominator, _fps_code(fps_out), first_picture, n_pictures))


FIELD_TOP, FIELD_BOTTOM = 0, 1   # efx_deint_opts.first_field
DEINT_FRAME, DEINT_FIELD = 0, 1  # efx_deint_opts.mode
_FIRST_FIELDS = {"top": FIELD_TOP, "tff": FIELD_TOP, "bottom": FIELD_BOTTOM, "bff": FIELD_BOTTOM}
_DEINT_RATES = {"frame": DEINT_FRAME, "field": DEINT_FIELD}


def _deint_setting(first_field, rate):
    if first_field not in _FIRST_FIELDS:
        raise ValueError(f"unknown first_field {first_field!r}: 'top' (or 'tff') or 'bottom' (or 'bff')")
    if rate not in _DEINT_RATES:
        raise ValueError(f"unknown rate {rate!r}: 'field' (two pictures per frame) or 'frame' (one)")
    return _FIRST_FIELDS[first_field], _DEINT_RATES[rate]


def deinterlace_count(n_frames: int, *, rate: str = "field", lead: bool = False, tail: bool = False) -> int:
    """Pictures per stream a deinterlace call makes of n_frames offered frames (efx_deinterlace_count; -1 for arguments
    the call rejects): rate "field" two per frame, "frame" one; lead / tail: the first / last frame is context only."""
    _, mode = _deint_setting("top", rate)
    return int(load_library().efx_deinterlace_count(n_frames, 1 if lead else 0, 1 if tail else 0, mode))


def detelecine_count(n_frames: int, *, lead: bool = False) -> int:
    """Film frames per stream a detelecine call makes of n_frames offered frames (efx_detelecine_count; -1 for arguments
    the call rejects): of the n = n_frames - lead processed frames one in every whole cycle of five is dropped."""
    return int(load_library().efx_detelecine_count(n_frames, 1 if lead else 0))


# efx_scan_frame.label / .repeat and the verdicts of efx_scan_verdict
SCAN_NONE, SCAN_STILL, SCAN_PROGRESSIVE, SCAN_TFF, SCAN_BFF, SCAN_UNDETERMINED = range(6)
SCAN_REPEAT_NONE, SCAN_REPEAT_TOP, SCAN_REPEAT_BOTTOM = range(3)
_SCAN_KINDS = ("unknown", "progressive", "interlaced", "telecined")
SCAN_DEFAULTS = dict(nt=10, still=64, prog=384, intl=266, rep=768)   # still: not measured on real material (profiles/scan.md)


def scan_verdict(rec) -> ScanResult:
    """The verdict of one stream's counts, a SCAN_REC_DTYPE record (efx_scan_verdict; host only)."""
    r = np.array(rec, dtype=SCAN_REC_DTYPE).reshape(1)
    first = C.c_int(-1)
    kind = int(load_library().efx_scan_verdict(r.ctypes.data, C.byref(first)))
    if not 0 <= kind < len(_SCAN_KINDS):
        raise ValueError("not a scan record")
    return ScanResult(_SCAN_KINDS[kind], {FIELD_TOP: "top", FIELD_BOTTOM: "bottom"}.get(first.value), r[0])


DENOISE_MAX_THRESHOLD = 64   # efx_denoise_opts: every threshold lies in 0 .. 64


def denoise_thresholds(sigma: float) -> tuple:
    """(luma_spatial, chroma_spatial, luma_temporal, chroma_temporal) for noise of standard deviation sigma, in levels:
    (2 sigma, 2 sigma, 4 sigma, 4 sigma), rounded and clamped to 64 -- the settings measured in profiles/denoise.md.
    Host only."""
    if not sigma >= 0:
        raise ValueError(f"sigma must be >= 0, got {sigma!r}")
    t = lambda v: int(min(DENOISE_MAX_THRESHOLD, v + 0.5))
    return t(2 * sigma), t(2 * sigma), t(4 * sigma), t(4 * sigma)


class Overlay:
    """One event of Decoder.overlay() / make_title(overlays=): a bitmap shown over the pictures first .. last of a title.
    bitmap: (h, w) uint8 alpha drawn in `colour` (R, G, B) -- what libass or Pillow's text mask gives -- or (h, w, 4)
    uint8 R, G, B, A with straight alpha (`colour` is then not used).  x, y: the picture column and row of its top-left
    sample; it is clipped to the picture.  stream: the stream it belongs to, -1 = every stream.  opacity: 0 .. 256.
    fade_in, fade_out: pictures over which it comes and goes.  Events that show the same array object share its bytes."""
    __slots__ = ("bitmap", "first", "last", "x", "y", "colour", "stream", "opacity", "fade_in", "fade_out")

    def __init__(self, bitmap, first: int, last: int, x: int, y: int, colour=(255, 255, 255), stream: int = -1, opacity: int = 256,
                 fade_in: int = 0, fade_out: int = 0):
        self.bitmap, self.first, self.last, self.x, self.y = bitmap, first, last, x, y
        self.colour, self.stream, self.opacity, self.fade_in, self.fade_out = colour, stream, opacity, fade_in, fade_out

    def __repr__(self):
        return (f"Overlay({tuple(np.shape(self.bitmap))}, first={self.first}, last={self.last}, x={self.x}, y={self.y}, "
                f"stream={self.stream})")


def overlay_span(fps, start_s, end_s) -> tuple:
    """(first, last): the pictures of a title at fps (any constant rate, as for conform) whose display begins inside the
    time span [start_s, end_s) in seconds -- first = ceil(start x fps), last = ceil(end x fps) - 1 -- in exact rational
    arithmetic (times may be Fractions, "num/den" strings, ints or floats, a float counting as its exact binary value).
    ValueError for a span that holds no picture or begins before 0."""
    f, a, b = _rate(fps), Fraction(start_s), Fraction(end_s)
    first, last = math.ceil(a * f), math.ceil(b * f) - 1
    if a < 0 or last < first:
        raise ValueError(f"the span {start_s!r} .. {end_s!r} s holds no picture at {f} pictures per second")
    return first, last


def overlay_pack(overlays, names=None) -> tuple:
    """(events, atlas) of a list of Overlay: the efx_overlay_event records (OVERLAY_EVENT_DTYPE) in list order, and one
    uint8 atlas that holds every distinct bitmap object once, row after row (pitch = the row's bytes), each at a 16-byte
    aligned offset, its length a multiple of 16.  ValueError, naming the event, for a bitmap of another shape or type or
    a value that does not fit its field (names: the numbers to name the events by, where they are not their places)."""
    events = np.zeros(len(overlays), dtype=OVERLAY_EVENT_DTYPE)
    placed, parts, size = {}, [], 0
    for k, o in enumerate(overlays):
        i = k if names is None else names[k]
        b = o.bitmap
        if not isinstance(b, np.ndarray) or b.dtype != np.uint8 or not (b.ndim == 2 or (b.ndim == 3 and b.shape[2] == 4)) or b.size == 0:
            raise ValueError(f"event {i} ({o!r}): bitmap must be a non-empty (h, w) or (h, w, 4) uint8 array")
        if id(b) not in placed:
            placed[id(b)] = size
            data = np.ascontiguousarray(b).reshape(-1)
            parts.append(data)
            pad = -data.size % 16
            if pad:
                parts.append(np.zeros(pad, dtype=np.uint8))
            size += data.size + pad
        rgba = b.ndim == 3
        try:
            r, g, bl = (0, 0, 0) if rgba else (int(v) for v in o.colour)
            if not all(0 <= v <= 255 for v in (r, g, bl)):
                raise OverflowError("a colour component outside 0 .. 255")
            values = (o.first, o.last, placed[id(b)], o.stream, o.x, o.y, b.shape[1] * (4 if rgba else 1), r << 16 | g << 8 | bl,
                      b.shape[1], b.shape[0], o.opacity, o.fade_in, o.fade_out, OVL_RGBA if rgba else OVL_A8, 0, 0)
            events[k] = values
            if any(int(got) != int(v) for got, v in zip(events[k].tolist(), values)):
                raise OverflowError("a value wrapped")
        except (OverflowError, TypeError, ValueError) as exc:
            raise ValueError(f"event {i} ({o!r}): a value does not fit its field of efx_overlay_event") from exc
    atlas = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return events, atlas


def overlay_check(events, atlas_bytes: int) -> int:
    """efx_overlay_check: the index of the first record of events (OVERLAY_EVENT_DTYPE) that is not valid for an atlas of
    atlas_bytes, or -1."""
    ev = np.ascontiguousarray(events, dtype=OVERLAY_EVENT_DTYPE)
    return int(load_library().efx_overlay_check(ev.ctypes.data, len(ev), atlas_bytes))


def sbc_state_bytes() -> int:
    return int(load_library().efx_sbc_state_bytes())


def sbc_frame_bytes(blocks: int, channels: int, bitpool: int) -> int:
    """Bytes of an SBC frame of 8 subbands (efx_sbc_frame_bytes; 0 for arguments efx_sbc_encode rejects)."""
    return int(load_library().efx_sbc_frame_bytes(blocks, channels, bitpool))


def sbc_enc_state_bytes() -> int:
    return int(load_library().efx_sbc_enc_state_bytes())


def import_pcm_out_samples(in_rate: int, out_rate: int, first_in: int, n_in: int) -> int:
    """Samples per stream an import_pcm call writes: ceil((first_in + n_in) o / r) - ceil(first_in o / r)
    (efx_import_pcm_out_samples; -1 for invalid arguments)."""
    return int(load_library().efx_import_pcm_out_samples(in_rate, out_rate, first_in, n_in))


def import_pcm_delay(in_rate: int, out_rate: int) -> int:
    """The resampler's delay W in input frames, 0 for equal rates (efx_import_pcm_delay; -1 for invalid rates)."""
    return int(load_library().efx_import_pcm_delay(in_rate, out_rate))


def import_pcm_state_bytes() -> int:
    return int(load_library().efx_import_pcm_state_bytes())


def import_pcm_filter() -> np.ndarray:
    """The resampler's prototype table T (efx_import_pcm_filter): int32, 16 P + 1 entries."""
    lib = load_library()
    t = np.empty(lib.efx_import_pcm_filter(None, 0), dtype=np.int32)
    lib.efx_import_pcm_filter(t.ctypes.data, t.size)
    return t


def loudness_lufs(block_energy: int, rate: int) -> float:
    """A block energy of an efx_loudness_rec (gated_mean: integrated, max_block: maximum momentary) in LUFS
    (efx_loudness_lufs); -inf for 0."""
    return float(load_library().efx_loudness_lufs(int(block_energy), rate))


def loudness_thresholds(rate: int, target: float = -23.0, peak: float = -1.0):
    """(abs_thr, target_ms, ceiling): the integers efx_loudness_gate takes for a target in LUFS and a peak ceiling in
    dBFS (efx_loudness_thresholds)."""
    a, t, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
    if load_library().efx_loudness_thresholds(rate, float(target), float(peak), C.byref(a), C.byref(t), C.byref(c)) != 0:
        raise ValueError("rate must be 16000, 32000, 44100 or 48000, target -70 .. 0 LUFS and peak -90 .. 0 dBFS")
    return int(a.value), int(t.value), int(c.value)


def loudness_coefs(rate: int) -> np.ndarray:
    """The K-weighting filter's ten Q28 coefficients at `rate` (efx_loudness_coefs): b0 b1 b2 a1 a2 of the shelf, then of
    the high pass."""
    out = (C.c_int32 * 10)()
    if load_library().efx_loudness_coefs(rate, out) != 0:
        raise ValueError("rate must be 16000, 32000, 44100 or 48000")
    return np.array(out, dtype=np.int32)


def loudness_state_bytes(rate: int) -> int:
    """Bytes of loudness state per stream (efx_loudness_state_bytes; 0 for a rate that is not one of the four)."""
    return int(load_library().efx_loudness_state_bytes(rate))


def loudness_step_count(rate: int, first_sample: int, n_samples: int) -> int:
    """Steps of 100 ms that become whole with n_samples more samples (efx_loudness_step_count; -1 for invalid arguments)."""
    return int(load_library().efx_loudness_step_count(rate, first_sample, n_samples))


def limit_block(rate: int) -> int:
    """Samples of a block of the peak limiter at `rate` (efx_limit_block): 16, 32, 48 or 48; 0 for a rate that is not one of
    the four."""
    return int(load_library().efx_limit_block(rate))


def _limit_blocks(samples: int, rate: int) -> int:
    """Blocks of `samples` samples at `rate`: the entries of a stream's peaks row.  ValueError for a rate that is not one of
    the four."""
    bk = limit_block(rate)
    if not bk:
        raise ValueError("rate must be 16000, 32000, 44100 or 48000")
    return -(-samples // bk)


def limit_gain(gated_mean: int, n_gated: int, target_ms: int, rate: int) -> int:
    """The gain (Q12, 1 .. 32767) the limiter aims at for a stream whose efx_loudness_rec holds gated_mean and n_gated
    (efx_limit_gain): the loudness gain to target_ms (loudness_thresholds(rate, target)[1]) without the record's peak
    cap; 4096 when n_gated is 0.  0 for arguments out of range."""
    return int(load_library().efx_limit_gain(int(gated_mean), int(n_gated), int(target_ms), rate))


def mux_bound(video_bytes: int, n_frames: int, frame_bytes: int, frames_per_pes: int) -> int:
    """A dst_stride with which efx_mux_av never reports MUX_FULL (efx_mux_bound; 0 for invalid arguments)."""
    return int(load_library().efx_mux_bound(video_bytes, n_frames, frame_bytes, frames_per_pes))


def mux_audio_packets(n_frames: int, frame_bytes: int, frames_per_pes: int) -> int:
    """Audio packets efx_mux_av writes per stream: add to audio_cc (mod 16) for the next call."""
    return int(load_library().efx_mux_audio_packets(n_frames, frame_bytes, frames_per_pes))


def _count_pictures(es: bytes) -> int:
    """picture_start_codes (00 00 01 00) of an elementary stream."""
    a = np.frombuffer(es, dtype=np.uint8)
    if a.size < 4:
        return 0
    return int(np.count_nonzero((a[:-3] == 0) & (a[1:-2] == 0) & (a[2:-1] == 1) & (a[3:] == 0)))


def _check(ctx, status: int):
    if status != 0:
        lib = load_library()
        msg = lib.efx_status_string(status).decode()
        if ctx:
            detail = lib.efx_last_error(ctx).decode()
            if detail:
                msg += f" ({detail})"
        raise EfxError(status, msg)


@dataclass
class Timing:
    index_ms: float
    parse_ms: float
    recon_ms: float
    total_ms: float
    pictures: int
    slices: int
    coefficients: int
    es_bytes: int
    demux_ms: float = 0.0
    ts_bytes: int = 0
    timed_calls: int = 0
    groups: int = 1  # reconstruction groups of the newest call: one k_recon launch per group and picture index
    parse_halves: int = 1  # parse halves of the newest call: one per group
    mixed: int = 0   # 1: the averaged calls did not all run with that structure
    recon_launches: int = 0  # reconstruction kernel launches of the newest call (groups x pictures)


class DeviceBuffer:
    """A raw HBM allocation owned by a Decoder context."""

    def __init__(self, dec: "Decoder", nbytes: int):
        self._dec = dec
        self.nbytes = nbytes
        p = _P()
        _check(dec._ctx, dec._lib.efx_device_alloc(dec._ctx, nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        _check(self._dec._ctx, self._dec._lib.efx_memcpy_h2d(self._dec._ctx, self.ptr, a.ctypes.data, a.nbytes))

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _check(self._dec._ctx, self._dec._lib.efx_memcpy_d2h(self._dec._ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self._dec._lib.efx_device_free(self._dec._ctx, self.ptr)
            self.ptr = None


def _ptr(b):
    """What the *_to calls pass on: a DeviceBuffer's pointer, a raw pointer or None as it is (where the C side takes no
    null it says so itself)."""
    return b.ptr if isinstance(b, DeviceBuffer) else b


def _r16(v: int) -> int:
    return (v + 15) // 16 * 16


def _r8(v: int) -> int:
    return (v + 7) // 8 * 8


class _Scratch:
    """The temporaries of one convenience call (Decoder._scratch()): device buffers, freed on exit, and tensors, held
    until then.  On exit through an exception the library's stream is waited for first: queued calls may still use
    them."""

    def __init__(self, dec: "Decoder"):
        self._dec, self._bufs, self._kept = dec, [], []

    def alloc(self, nbytes: int) -> DeviceBuffer:
        """At least 16 bytes, so that an empty batch needs no guard."""
        buf = DeviceBuffer(self._dec, max(16, nbytes))
        self._bufs.append(buf)
        return buf

    def zeros(self, nbytes: int) -> DeviceBuffer:
        """alloc() and an upload of zeros, which synchronises the library's stream: before anything is queued."""
        buf = self.alloc(nbytes)
        buf.upload(np.zeros(nbytes, dtype=np.uint8))
        return buf

    def keep(self, tensor):
        self._kept.append(tensor)
        return tensor

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            try:
                self._dec.sync()
            except EfxError:
                pass
        for b in self._bufs:
            b.free()
        return False


class Decoder:
    """Batched MpegDecoder: `max_streams` independent streams, `max_pictures` pictures per decode.

    ring_depth = 2 reproduces the reference's two frame buffers (_fb[2], src/player.h:37-40);
    ring_depth = max_pictures + 1 keeps every decoded picture resident.
    """

    def __init__(self, max_streams: int, max_pictures: int, ring_depth: int = 2, device: int = 0,
                 max_stream_bytes: int = 0, hip_stream: int = 0):
        self._lib = load_library()
        self._ctx = _P()
        cfg = _Config(device, max_streams, max_pictures, ring_depth, max_stream_bytes, hip_stream or None)
        _check(None, self._lib.efx_create(C.byref(cfg), C.byref(self._ctx)))
        self.max_streams, self.max_pictures, self.ring_depth = max_streams, max_pictures, max(2, ring_depth)
        self.device = device
        self.hip_stream = hip_stream
        self.n_streams = 0
        self._enc_rate_code = 4  # picture_rate of the streams cont=True continues

    def close(self):
        if self._ctx:
            self._lib.efx_destroy(self._ctx)
            self._ctx = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- bitstream in ---------------------------------------------------------------------
    def upload(self, streams, fmt: int = FORMAT_ES):
        """streams: sequence of bytes / uint8 arrays (one per stream)."""
        arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray, memoryview))
                else np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
        n = len(arrs)
        ptrs = (_P * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        _check(self._ctx, self._lib.efx_upload_streams(self._ctx, n, ptrs, lens, fmt))
        self.n_streams = n

    def prepare_upload(self, streams):
        """The ctypes argument arrays of upload() for a batch that is uploaded repeatedly (ingest benchmarks)."""
        arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray, memoryview))
                else np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
        n = len(arrs)
        return arrs, (_P * n)(*[a.ctypes.data for a in arrs]), (C.c_size_t * n)(*[a.size for a in arrs]), n

    def upload_prepared(self, prepared, fmt: int = FORMAT_ES, in_place: bool = False):
        """in_place: efx_upload_streams_inplace -- the batch must lie in an arena of this context (place_in_arena); the
        library writes the tails into the layout's gaps and the transfer reads the arena.  Otherwise the staged path."""
        _, ptrs, lens, n = prepared
        fn = self._lib.efx_upload_streams_inplace if in_place else self._lib.efx_upload_streams
        _check(self._ctx, fn(self._ctx, n, ptrs, lens, fmt))
        self.n_streams = n

    # -- in-place ingest (efx_host_alloc / efx_stream_layout / efx_upload_done) ---------------
    def host_arena(self, nbytes: int) -> np.ndarray:
        """Page-locked host memory of this context as a uint8 array (freed with the context)."""
        p = _P()
        _check(self._ctx, self._lib.efx_host_alloc(self._ctx, nbytes, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def place_in_arena(self, arena: np.ndarray, streams):
        """Lay a batch out in `arena` the way efx_stream_layout prescribes and return the prepared argument arrays
        for upload_prepared(..., in_place=True): such a batch is transferred straight from the arena, no staging copy."""
        arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray, memoryview))
                else np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
        n = len(arrs)
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        off = (C.c_size_t * (n + 1))()
        _check(self._ctx, self._lib.efx_stream_layout(n, lens, off))
        assert off[n] <= arena.size, "arena too small for the batch"
        base = arena.ctypes.data
        for a, o in zip(arrs, off):
            arena[o:o + a.size] = a
        return arena, (_P * n)(*[base + off[i] for i in range(n)]), lens, n

    def upload_done(self) -> bool:
        r = self._lib.efx_upload_done(self._ctx)
        if r < 0:
            _check(self._ctx, r)
        return bool(r)

    def set_option(self, option: int, value: int):
        _check(self._ctx, self._lib.efx_set_option(self._ctx, option, value))

    def get_option(self, option: int) -> int:
        v = C.c_int()
        _check(self._ctx, self._lib.efx_get_option(self._ctx, option, C.byref(v)))
        return v.value

    def reset(self):
        _check(self._ctx, self._lib.efx_reset(self._ctx))

    def play_reset(self):
        """MpegDecoder::reset() between plays: the PTS latch is cleared, the ring position survives."""
        _check(self._ctx, self._lib.efx_play_reset(self._ctx))

    def stream_state(self, stream: int = 0):
        """(frame index, a PTS has been latched, newest PES PTS) of a stream."""
        fi, seen, pts = C.c_uint32(), C.c_int(), C.c_int64()
        _check(self._ctx, self._lib.efx_stream_state(self._ctx, stream, C.byref(fi), C.byref(seen), C.byref(pts)))
        return fi.value, bool(seen.value), pts.value

    def erase_frames(self):
        _check(self._ctx, self._lib.efx_erase_frames(self._ctx))

    # -- decode ---------------------------------------------------------------------------
    def decode(self, sync: bool = True, first_picture: int = 0, n_pictures: int | None = None):
        """efx_decode (first_picture = 0) / efx_decode_from / efx_decode_range (at most n_pictures pictures per stream):
        the decoder keeps going from call to call."""
        if n_pictures is None:
            _check(self._ctx, self._lib.efx_decode_from(self._ctx, first_picture))
        else:
            _check(self._ctx, self._lib.efx_decode_range(self._ctx, first_picture, n_pictures))
        if sync:
            self.sync()

    def sync(self):
        _check(self._ctx, self._lib.efx_sync(self._ctx))

    def picture_count(self, stream: int) -> int:
        n = C.c_int()
        _check(self._ctx, self._lib.efx_picture_count(self._ctx, stream, C.byref(n)))
        return n.value

    def stream_status(self, stream: int) -> int:
        b = C.c_uint32()
        _check(self._ctx, self._lib.efx_stream_status(self._ctx, stream, C.byref(b)))
        return b.value

    def es(self, stream: int) -> bytes:
        """The elementary stream the decoder sees for `stream` (device-demultiplexed for TS input)."""
        n = C.c_size_t()
        _check(self._ctx, self._lib.efx_download_es(self._ctx, stream, None, 0, C.byref(n)))
        buf = (C.c_uint8 * max(n.value, 1))()
        _check(self._ctx, self._lib.efx_download_es(self._ctx, stream, buf, n.value, C.byref(n)))
        return bytes(buf[: n.value])

    def picture_pts(self, stream: int, picture: int) -> int:
        p = C.c_int64()
        _check(self._ctx, self._lib.efx_picture_pts(self._ctx, stream, picture, C.byref(p)))
        return p.value

    def picture_slot(self, picture: int, stream: int = 0) -> int:
        """Ring slot of a picture of the last decode (synchronises)."""
        slot = C.c_int()
        _check(self._ctx, self._lib.efx_stream_picture_slot(self._ctx, stream, picture, C.byref(slot)))
        return slot.value

    # -- frames out -----------------------------------------------------------------------
    def frame_ptr(self, stream: int, slot: int) -> int:
        p = _P()
        _check(self._ctx, self._lib.efx_frame_device_ptr(self._ctx, stream, slot, C.byref(p)))
        return p.value

    def download_frame(self, stream: int, slot: int) -> np.ndarray:
        out = np.empty(FRAME_BYTES, dtype=np.uint8)
        _check(self._ctx, self._lib.efx_download_frame(self._ctx, stream, slot, out.ctypes.data))
        return out

    def download_picture(self, stream: int, picture: int) -> np.ndarray:
        return self.download_frame(stream, self.picture_slot(picture))

    def upload_frame(self, stream: int, slot: int, frame: np.ndarray):
        f = np.ascontiguousarray(frame, dtype=np.uint8)
        assert f.size == FRAME_BYTES
        _check(self._ctx, self._lib.efx_upload_frame(self._ctx, stream, slot, f.ctypes.data))

    def frame_hashes(self, first_stream: int = 0, n: int | None = None) -> np.ndarray:
        """FNV-1a-64 of every ring frame, shape (n, ring_depth), computed on the device."""
        n = self.n_streams - first_stream if n is None else n
        out = np.empty((n, self.ring_depth), dtype=np.uint64)
        _check(self._ctx, self._lib.efx_frame_hashes(self._ctx, first_stream, n, out.ctypes.data))
        return out

    # -- pictures out (efx_export_frames) ---------------------------------------------------
    def _export_opts(self, fmt, first_stream, n_streams, picture, slot, chroma, full_range, dst_stride=0):
        if fmt not in _PIX_FORMATS:
            raise ValueError(f"unknown format {fmt!r}: one of {sorted(_PIX_FORMATS)}")
        if chroma not in _CHROMA_MODES:
            raise ValueError(f"unknown chroma mode {chroma!r}: one of {sorted(_CHROMA_MODES)}")
        if picture is not None and slot is not None:
            raise ValueError("give picture= (of the most recent decode) or slot= (a ring slot), not both")
        if slot is None and picture is None:
            picture = 0
        n = (self.n_streams - first_stream) if n_streams is None else n_streams
        return n, _ExportOpts(first_stream, n, -1 if slot is None else slot, 0 if picture is None else picture,
                              _PIX_FORMATS[fmt], _CHROMA_MODES[chroma], 1 if full_range else 0, dst_stride)

    def export_to(self, dst: DeviceBuffer | int, fmt: str = "rgb24", *, first_stream: int = 0, n_streams: int | None = None,
                  picture: int | None = None, slot: int | None = None, chroma: str = "bilinear", full_range: bool = False,
                  dst_stride: int = 0):
        """efx_export_frames into raw device memory (a DeviceBuffer or a pointer), asynchronous on the library's stream:
        image i at dst + i * dst_stride (0 = packed).  Arguments as export()."""
        _, o = self._export_opts(fmt, first_stream, n_streams, picture, slot, chroma, full_range, dst_stride)
        ptr = dst.ptr if isinstance(dst, DeviceBuffer) else dst
        _check(self._ctx, self._lib.efx_export_frames(self._ctx, C.byref(o), ptr))

    def export(self, fmt: str = "rgb24", *, first_stream: int = 0, n_streams: int | None = None, picture: int | None = None,
               slot: int | None = None, chroma: str = "bilinear", full_range: bool = False, out=None, sync: bool = True):
        """Decoded pictures as a torch uint8 tensor on the decoder's device, converted there (no host round trip):
        fmt "rgb24" -> (n, 192, 352, 3), "rgbp" -> (n, 3, 192, 352), "i420" -> (n, 101376) (i420_planes() splits it).
        Streams first_stream ... + n_streams (default: the rest of the last upload); picture p of the most recent decode
        (picture=, the default: p = 0) or ring slot k of every stream (slot=).  chroma "bilinear" (MPEG-1 siting) or
        "nearest"; full_range False = BT.601 studio swing (what MPEG-1 carries).  out: a preallocated contiguous uint8
        tensor of that size on this device, or a DeviceBuffer (then returned as is).

        The kernel runs on the library's stream.  sync=True (default) waits for it, so the tensor is ready for any torch
        stream.  sync=False is only safe when the decoder was created with hip_stream= the handle (.cuda_stream) of
        torch's current stream and that stream is a torch.cuda.Stream(), not the default
        stream (whose handle, 0, makes the library create a private stream) -- the tensor is then ordered like any torch
        op on that stream -- or when the caller calls sync() before using the tensor."""
        import torch

        n, o = self._export_opts(fmt, first_stream, n_streams, picture, slot, chroma, full_range)
        shape = _export_shape(fmt, n)
        nbytes = n * export_bytes(fmt)
        if isinstance(out, DeviceBuffer):
            if out.nbytes < nbytes:
                raise ValueError(f"out holds {out.nbytes} bytes, the export needs {nbytes}")
            result, ptr = out, out.ptr
        else:
            device = torch.device("cuda", self.device)
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=device)
            if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != device:
                raise ValueError(f"out must be a uint8 tensor on {device}")
            if not out.is_contiguous() or out.numel() != nbytes:
                raise ValueError(f"out must be contiguous with {nbytes} elements (shape {shape})")
            result, ptr = out.view(shape), out.data_ptr()
        _check(self._ctx, self._lib.efx_export_frames(self._ctx, C.byref(o), ptr))
        if sync:
            self.sync()
        return result

    def export_host(self, fmt: str = "rgb24", *, first_stream: int = 0, n_streams: int | None = None,
                    picture: int | None = None, slot: int | None = None, chroma: str = "bilinear",
                    full_range: bool = False) -> np.ndarray:
        """export() for callers without torch: converted on the device, returned as a NumPy array of the same shape."""
        n, o = self._export_opts(fmt, first_stream, n_streams, picture, slot, chroma, full_range)
        buf = DeviceBuffer(self, n * export_bytes(fmt))
        try:
            _check(self._ctx, self._lib.efx_export_frames(self._ctx, C.byref(o), buf.ptr))
            self.sync()
            return buf.download(np.uint8, buf.nbytes).reshape(_export_shape(fmt, n))
        finally:
            buf.free()

    # -- pictures in (efx_import_frames) ----------------------------------------------------
    def import_to(self, src: DeviceBuffer | int, dst: DeviceBuffer | int, *, n_images: int, fmt: str, width: int, height: int,
                  crop=None, dst_rect=None, full_range: bool = False, src_stride: int = 0, dst_stride: int = 0, surface=None,
                  matrix=None, src_range: str | None = None, transfer=None, primaries=None, peak_nits: int | None = None):
        """efx_import_frames on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream:
        source image i (fmt "i420", "rgb24" or "rgbp", width x height) at src + i * src_stride (0 = import_src_bytes()
        rounded up to 16), its 352 x 192 I420 picture at dst + i * dst_stride (0 = 101376).  crop = (x, y, w, h) of the
        source (None: all of it), dst_rect = (x, y, w, h) of the output that receives it (None: all of it), the rest is
        black.  surface: an efx_surface from surface_layout() -- the images are then read as that surface describes them
        (efx_import_surfaces: NV12, P010, pitched planes ...), fmt must be "i420", width and height the surface's, and
        src_stride 0 means surface.bytes rounded up to 16.
        matrix, src_range: the YCbCr source's matrix and range as colour_coefs() takes them; the picture is converted to
        BT.601 studio swing in the same kernel (efx_import_set_colour around this call; the context's setting, see
        set_import_colour(), is put back behind it).  Both None: the context's setting applies, which is "off" unless
        set_import_colour() was called.  RGB sources take neither (ValueError): full_range names the range they write.
        transfer="pq" (with primaries= "bt2020" or "bt709", peak_nits= 200 .. 10000, default 1000): the source is HDR10
        and is tone-mapped to SDR in the same kernel (efx_import_set_hdr around this call; set_import_hdr()'s setting is
        put back behind it); matrix= (default "bt2020") and src_range= then describe the HDR source and the colour
        setting is not used.  RGB sources take none of these (ValueError)."""
        if fmt not in _PIX_FORMATS:
            raise ValueError(f"unknown format {fmt!r}: one of {sorted(_PIX_FORMATS)}")
        hdr = _hdr_setting(transfer, primaries, matrix, src_range, peak_nits)
        colour = _colour_setting(matrix, src_range) if hdr is None else None
        if (colour is not None or hdr is not None) and fmt != "i420":
            raise ValueError("matrix=, src_range= and transfer= describe a YCbCr source; an RGB source is converted with BT.601 (full_range=)")
        if hdr is not None:
            _check(self._ctx, self._lib.efx_import_set_hdr(self._ctx, C.byref(_ImportHdr(*hdr))))
        o = _ImportOpts(n_images, _PIX_FORMATS[fmt], width, height, *(crop or (0, 0, 0, 0)), *(dst_rect or (0, 0, 0, 0)),
                        1 if full_range else 0, src_stride, dst_stride)
        if colour is not None:
            _check(self._ctx, self._lib.efx_import_set_colour(self._ctx, C.byref(_ImportColour(*colour))))
        try:
            if surface is not None:
                _check(self._ctx, self._lib.efx_import_surfaces(self._ctx, C.byref(surface), C.byref(o), _ptr(src), _ptr(dst)))
            else:
                _check(self._ctx, self._lib.efx_import_frames(self._ctx, C.byref(o), _ptr(src), _ptr(dst)))
        finally:
            if colour is not None:
                self._apply_import_colour()
            if hdr is not None:
                self._apply_import_hdr()

    def set_import_colour(self, matrix=None, src_range: str | None = None):
        """The matrix and range of the YCbCr sources of the imports that follow (efx_import_set_colour), as
        colour_coefs() takes them; both None switches the conversion off, which is the default.  An import method's own
        matrix= / src_range= overrides it for that call."""
        colour = _colour_setting(matrix, src_range)
        _check(self._ctx, self._lib.efx_import_set_colour(self._ctx, C.byref(_ImportColour(*colour)) if colour is not None else None))
        self._import_colour = colour

    def set_import_hdr(self, transfer=None, primaries=None, matrix=None, src_range: str | None = None, peak_nits: int | None = None):
        """The HDR description of the YCbCr sources of the imports that follow (efx_import_set_hdr): transfer "pq" (or
        16), primaries "bt2020" / "bt709" (or 9 / 1), matrix and src_range as colour_coefs() takes them (default BT.2020,
        studio), peak_nits the source's peak (MaxCLL or the mastering display's maximum, 200 .. 10000; default 1000).
        While it is on it supersedes set_import_colour().  transfer None switches it off, which is the default.  An import
        method's own transfer= overrides it for that call."""
        hdr = _hdr_setting(transfer, primaries, matrix, src_range, peak_nits)
        _check(self._ctx, self._lib.efx_import_set_hdr(self._ctx, C.byref(_ImportHdr(*hdr)) if hdr is not None else None))
        self._import_hdr = hdr

    def _apply_import_hdr(self):
        hdr = getattr(self, "_import_hdr", None)
        self._lib.efx_import_set_hdr(self._ctx, C.byref(_ImportHdr(*hdr)) if hdr is not None else None)

    def _apply_import_colour(self):
        colour = getattr(self, "_import_colour", None)
        self._lib.efx_import_set_colour(self._ctx, C.byref(_ImportColour(*colour)) if colour is not None else None)

    # -- what the convenience methods share: temporaries, staging, the wait for torch, rows back ------
    def _scratch(self) -> _Scratch:
        return _Scratch(self)

    def _wait_for_torch(self, own_stream_ok: bool = False) -> bool:
        """Synchronise torch's current stream on the decoder's device, so that the library's stream may read what torch
        wrote; returns whether it waited.  own_stream_ok: no wait when that stream is the decoder's own (hip_stream=),
        where the calls are ordered behind torch's work anyway."""
        import torch
        cur = torch.cuda.current_stream(torch.device("cuda", self.device))
        if own_stream_ok and self.hip_stream and cur.cuda_stream == self.hip_stream:
            return False
        cur.synchronize()
        return True

    def _stage(self, s: _Scratch, src, n: int, row: int, *, stride: int | None = None, dtype=np.uint8, what: str = "src"):
        """n rows of `row` elements of src in device memory, row i at i * stride elements (None: row rounded up so that
        every row starts 16-byte aligned): (pointer, array input?, copied?).  A NumPy array is uploaded into a buffer of
        s, zero-padded where stride != row.  A tensor of that dtype on the decoder's device is used in place when it is
        packed (stride == row) and 16-byte aligned, else copied to a zeroed (n, stride) tensor; s keeps it, and the
        caller waits for torch (_wait_for_torch) before it queues what reads it."""
        dtype = np.dtype(dtype)
        if stride is None:
            stride = _r16(row * dtype.itemsize) // dtype.itemsize
        if isinstance(src, np.ndarray):
            host = np.ascontiguousarray(src, dtype=dtype).reshape(n, row)
            if stride != row:
                host, packed = np.zeros((n, stride), dtype=dtype), host
                host[:, :row] = packed
            buf = s.alloc(host.nbytes)
            buf.upload(host)
            return buf.ptr, True, False
        import torch
        device = torch.device("cuda", self.device)
        if not isinstance(src, torch.Tensor) or src.dtype != getattr(torch, dtype.name) or src.device != device:
            raise ValueError(f"{what} must be a {dtype.name} tensor on {device} (or a NumPy array)")
        flat = src.contiguous()
        if stride != row or flat.data_ptr() % 16:
            flat, packed = torch.zeros((n, stride), dtype=src.dtype, device=device), flat
            flat[:, :row] = packed.view(n, row)
        s.keep(flat)
        return flat.data_ptr(), False, flat is not src

    def _rows_out(self, s: _Scratch, is_array: bool, n: int, row: int, stride: int):
        """Where a call writes n rows of `row` bytes, `stride` apart, and how they come back: (pointer, fetch).  For array
        input a buffer of s, and fetch() -- after the sync -- downloads it and crops the rows; for tensor input a fresh
        tensor, which fetch() returns, cropped and made contiguous only where stride != row."""
        if is_array:
            buf = s.alloc(n * stride)
            return buf.ptr, lambda: np.ascontiguousarray(buf.download(np.uint8, n * stride).reshape(n, stride)[:, :row])
        import torch
        out = torch.empty((n, stride), dtype=torch.uint8, device=torch.device("cuda", self.device))
        return out.data_ptr(), lambda: out if stride == row else out[:, :row].contiguous()

    def _frames_to_pictures(self, src, fmt, width, height, pitch, plane_rows, n_streams, count, queue):
        """What deinterlace() and detelecine() share.  count(n_frames) gives (pictures, records) per stream or raises;
        queue(src, dst, records, **kw) is the *_to call, kw the surface, the counts and the strides.  Returns (pictures,
        records as TELECINE_INFO of shape (n_streams, records), None where count asks for none)."""
        surf, total, src = _surface_source(src, fmt, width, height, pitch, plane_rows)
        if n_streams < 1 or total % n_streams:
            raise ValueError(f"{total} source images do not make {n_streams} streams of equal length")
        n_frames = total // n_streams
        n_out, n_rec = count(n_frames)
        image = width * height * 3 // 2
        stride, dstride = _r16(surf.bytes), _r16(image)
        with self._scratch() as s:
            src_ptr, is_array, _ = self._stage(s, src, total, surf.bytes, stride=stride)
            if not is_array:
                self._wait_for_torch(own_stream_ok=True)
            ibuf = s.alloc(n_streams * n_rec * TELECINE_INFO.itemsize) if n_rec else None
            dst_ptr, fetch = self._rows_out(s, is_array, n_streams * n_out, image, dstride)
            queue(src_ptr, dst_ptr, ibuf, surface=surf, n_streams=n_streams, n_frames=n_frames, src_stride=stride, dst_stride=dstride)
            self.sync()
            return fetch(), ibuf.download(TELECINE_INFO, n_streams * n_rec).reshape(n_streams, n_rec) if ibuf else None

    # -- interlaced sources (efx_deinterlace) -------------------------------------------------
    def deinterlace_to(self, src: DeviceBuffer | int, dst: DeviceBuffer | int, *, surface: _Surface, n_streams: int = 1, n_frames: int,
                       first_field: str = "top", rate: str = "field", lead: bool = False, tail: bool = False, src_stride: int = 0,
                       dst_stride: int = 0) -> int:
        """efx_deinterlace on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: frame j of
        stream i, read as `surface` (surface_layout(): I420, YV12, NV12, NV21, pitched or packed) describes it, at src +
        (i * n_frames + j) * src_stride (0 = surface.bytes rounded up to 16); the progressive pictures, packed I420 of
        the surface's size, at dst + (i * n_out + m) * dst_stride (0 = width * height * 3 / 2 rounded up to 16).
        first_field "top" (tff) or "bottom" (bff); rate "field": both fields of a frame become pictures (576i25 gives 50
        pictures a second), "frame": the first field only; lead / tail: the first / last offered frame is context only,
        for a title that goes through in pieces with one frame of overlap.  The rule: include/efx.h, "interlaced
        sources".  Returns n_out, the pictures per stream (deinterlace_count)."""
        first, mode = _deint_setting(first_field, rate)
        o = _DeintOpts(n_streams, n_frames, first, mode, 1 if lead else 0, 1 if tail else 0, src_stride, dst_stride)
        _check(self._ctx, self._lib.efx_deinterlace(self._ctx, C.byref(surface), C.byref(o), _ptr(src), _ptr(dst)))
        return int(self._lib.efx_deinterlace_count(n_frames, o.lead, o.tail, mode))

    def deinterlace(self, src, *, fmt: str = "i420", width: int, height: int, pitch: int = 0, plane_rows: int = 0,
                    first_field: str = "top", rate: str = "field", n_streams: int = 1, lead: bool = False, tail: bool = False):
        """Interlaced frames as progressive pictures of the same size, made on the device (deinterlace_to).  src: a NumPy
        array or a uint8 torch tensor on the decoder's device of shape (n_streams * n_frames, bytes), stream by stream,
        bytes being surface_layout(fmt, width, height, pitch, plane_rows).bytes; fmt "i420", "yv12", "nv12" or "nv21",
        width even, height a multiple of 4 from 8.  Returns (n_streams * n_out, width * height * 3 / 2) uint8 packed I420
        pictures, n_out = deinterlace_count(n_frames, ...): what import_pictures(fmt="i420", width=, height=) and
        detect_crop() take; a tensor for a tensor (no host round trip), an array for an array.  Synchronises: torch's
        current stream before (tensor input), the library's after."""
        def count(n_frames):
            n_out = deinterlace_count(n_frames, rate=rate, lead=lead, tail=tail)
            if n_out < 0:
                raise ValueError(f"deinterlace: {n_frames} frames with lead={lead}, tail={tail} leave no frame with an output")
            return n_out, 0

        def queue(src_ptr, dst_ptr, _, **kw):
            self.deinterlace_to(src_ptr, dst_ptr, first_field=first_field, rate=rate, lead=lead, tail=tail, **kw)

        return self._frames_to_pictures(src, fmt, width, height, pitch, plane_rows, n_streams, count, queue)[0]

    # -- telecined sources (efx_detelecine) ---------------------------------------------------
    def detelecine_to(self, src: DeviceBuffer | int, dst: DeviceBuffer | int, info: DeviceBuffer | int, *, surface: _Surface,
                      n_streams: int = 1, n_frames: int, first_field: str = "top", lead: bool = False, nt: int = 10, src_stride: int = 0,
                      dst_stride: int = 0) -> int:
        """efx_detelecine on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: frame j of
        stream i, read as `surface` (surface_layout(): I420, YV12, NV12, NV21, pitched or packed) describes it, at src +
        (i * n_frames + j) * src_stride (0 = surface.bytes rounded up to 16); the film frames, packed I420 of the
        surface's size, at dst + (i * n_out + m) * dst_stride (0 = width * height * 3 / 2 rounded up to 16); one 32-byte
        record (TELECINE_INFO) per processed frame at info + (i * n + j) * 32, n = n_frames - lead, whatever info held
        before.  first_field "top" (tff) or "bottom" (bff); lead: the first offered frame is context only, for a title
        that goes through in pieces with one frame of overlap (every piece but the last processes a multiple of 5
        frames); nt: the noise threshold of the comb score in pels.  The rule: include/efx.h, "telecined sources".
        Returns n_out, the film frames per stream (detelecine_count)."""
        if first_field not in _FIRST_FIELDS:
            raise ValueError(f"unknown first_field {first_field!r}: 'top' (or 'tff') or 'bottom' (or 'bff')")
        o = _DetelecineOpts(n_streams, n_frames, _FIRST_FIELDS[first_field], 1 if lead else 0, nt, src_stride, dst_stride)
        _check(self._ctx, self._lib.efx_detelecine(self._ctx, C.byref(surface), C.byref(o), _ptr(src), _ptr(dst), _ptr(info)))
        return int(self._lib.efx_detelecine_count(n_frames, o.lead))

    def detelecine(self, src, *, fmt: str = "i420", width: int, height: int, pitch: int = 0, plane_rows: int = 0,
                   first_field: str = "top", n_streams: int = 1, lead: bool = False, nt: int = 10, info: bool = False):
        """Telecined frames (3:2 pulldown) as the film's frames, of the same size, made on the device (detelecine_to).  src:
        a NumPy array or a uint8 torch tensor on the decoder's device of shape (n_streams * n_frames, bytes), stream by
        stream, bytes being surface_layout(fmt, width, height, pitch, plane_rows).bytes; fmt "i420", "yv12", "nv12" or
        "nv21", width even, height a multiple of 4 from 8.  Returns (n_streams * n_out, width * height * 3 / 2) uint8
        packed I420 pictures, n_out = detelecine_count(n_frames, lead=lead): what import_pictures(fmt="i420", width=,
        height=) and detect_crop() take, to be encoded at fps=23.976; a tensor for a tensor (no host round trip), an
        array for an array.  With info=True it returns (pictures, records): the records a structured NumPy array
        (TELECINE_INFO) of shape (n_streams, n_frames - lead).  Synchronises: torch's current stream before (tensor
        input), the library's after."""
        def count(n_frames):
            n_out = detelecine_count(n_frames, lead=lead)
            if n_out < 0:
                raise ValueError(f"detelecine: {n_frames} frames with lead={lead} leave no frame to process")
            return n_out, n_frames - (1 if lead else 0)

        def queue(src_ptr, dst_ptr, records, **kw):
            self.detelecine_to(src_ptr, dst_ptr, records, first_field=first_field, lead=lead, nt=nt, **kw)

        out, records = self._frames_to_pictures(src, fmt, width, height, pitch, plane_rows, n_streams, count, queue)
        return (out, records) if info else out

    # -- scan type (efx_detect_scan) ----------------------------------------------------------
    def detect_scan_to(self, src: DeviceBuffer | int, frames: DeviceBuffer | int, recs: DeviceBuffer | int, *, surface: _Surface,
                       n_streams: int = 1, n_frames: int, lead: bool = False, first_frame: int = 0, accumulate: bool = False,
                       nt: int = 10, still: int = 64, prog: int = 384, intl: int = 266, rep: int = 768, src_stride: int = 0) -> int:
        """efx_detect_scan on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: frame j of
        stream i, read as `surface` (surface_layout(): I420, YV12, NV12, NV21, pitched or packed) describes it, at src +
        (i * n_frames + j) * src_stride (0 = surface.bytes rounded up to 16); one 48-byte record (SCAN_FRAME_DTYPE) per
        processed frame at frames + (i * n + j) * 48, n = n_frames - lead, whatever frames held before; stream i's counts
        (SCAN_REC_DTYPE, 64 bytes) at recs + 64 i, written, or with accumulate added to what lies there.  lead: the first
        offered frame is context only; first_frame: its number in the title, which keeps the repeat phases title-absolute
        when a title goes through in pieces with one frame of overlap.  nt, still, prog, intl, rep: the rule's options
        (include/efx.h, "scan type").  Returns n, the frame records per stream."""
        o = np.zeros(1, dtype=SCAN_OPTS_DTYPE)
        o[0] = (n_streams, n_frames, 1 if lead else 0, 1 if accumulate else 0, nt, still, prog, intl, rep, 0, first_frame, src_stride)
        _check(self._ctx, self._lib.efx_detect_scan(self._ctx, C.byref(surface), o.ctypes.data, _ptr(src), _ptr(frames), _ptr(recs)))
        return n_frames - (1 if lead else 0)

    def detect_scan(self, src, *, fmt: str = "i420", width: int, height: int, pitch: int = 0, plane_rows: int = 0, n_streams: int = 1,
                    lead: bool = False, first_frame: int = 0, recs=None, frames: bool = False, nt: int = 10, still: int = 64,
                    prog: int = 384, intl: int = 266, rep: int = 768):
        """Whether streams are progressive, interlaced or telecined, and in which field order, found on the device
        (detect_scan_to).  src: a NumPy array or a uint8 torch tensor on the decoder's device of shape (n_streams *
        n_frames, bytes), stream by stream, as detelecine() takes it.  recs: the records of the title's previous piece
        (the .rec of this method's results, or a SCAN_REC_DTYPE array of n_streams), to add to; the piece then begins
        with the previous piece's last frame (lead=True) and first_frame is that frame's number in the title.  Returns a
        list of ScanResult(kind, first_field, rec), one per stream; with frames=True (results, frame records), the
        records a SCAN_FRAME_DTYPE array of shape (n_streams, n_frames - lead).  Synchronises: torch's current stream
        before (tensor input), the library's after."""
        surf, total, src = _surface_source(src, fmt, width, height, pitch, plane_rows)
        if n_streams < 1 or total < 1 or total % n_streams:
            raise ValueError(f"{total} source images do not make {n_streams} streams of equal length")
        n_frames = total // n_streams
        n = n_frames - (1 if lead else 0)
        if n < 1:
            raise ValueError(f"detect_scan: {n_frames} frames with lead={lead} leave no frame to process")
        if recs is not None:
            recs = np.array([r.rec if isinstance(r, ScanResult) else r for r in recs], dtype=SCAN_REC_DTYPE).reshape(-1)
            if len(recs) != n_streams:
                raise ValueError(f"recs must hold {n_streams} records, got {len(recs)}")
        stride = _r16(surf.bytes)
        with self._scratch() as s:
            src_ptr, is_array, _ = self._stage(s, src, total, surf.bytes, stride=stride)
            if not is_array:
                self._wait_for_torch(own_stream_ok=True)
            fbuf = s.alloc(n_streams * n * SCAN_FRAME_DTYPE.itemsize)
            rbuf = s.alloc(n_streams * SCAN_REC_DTYPE.itemsize)
            if recs is not None:
                rbuf.upload(recs)
            self.detect_scan_to(src_ptr, fbuf, rbuf, surface=surf, n_streams=n_streams, n_frames=n_frames, lead=lead, first_frame=first_frame,
                                accumulate=recs is not None, nt=nt, still=still, prog=prog, intl=intl, rep=rep, src_stride=stride)
            self.sync()
            results = [scan_verdict(r) for r in rbuf.download(SCAN_REC_DTYPE, n_streams)]
            return (results, fbuf.download(SCAN_FRAME_DTYPE, n_streams * n).reshape(n_streams, n)) if frames else results

    # -- noisy sources (efx_denoise) ----------------------------------------------------------
    def denoise_to(self, src: DeviceBuffer | int, dst: DeviceBuffer | int, *, surface: _Surface, n_streams: int = 1, n_frames: int,
                   luma_spatial: int = 0, chroma_spatial: int = 0, luma_temporal: int = 0, chroma_temporal: int = 0,
                   prev: DeviceBuffer | int | None = None, src_stride: int = 0, dst_stride: int = 0, prev_stride: int = 0) -> int:
        """efx_denoise on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: frame j of
        stream i, read as `surface` (surface_layout(): I420, YV12, NV12, NV21, pitched or packed) describes it, at src +
        (i * n_frames + j) * src_stride (0 = surface.bytes rounded up to 16); the filtered pictures, packed I420 of the
        surface's size, at dst + (i * n_frames + j) * dst_stride (0 = width * height * 3 / 2 rounded up to 16).  The
        thresholds, 0 .. 64 in levels (denoise_thresholds(sigma)): a neighbour further than *_spatial from a sample stays
        out of its 3 x 3 average; a sample that moved by *_temporal or more against the stream's previous output takes
        the new value whole, a smaller change is blended.  prev: stream i's last output of the previous piece, packed
        I420, at prev + i * prev_stride -- a pointer into that call's dst; None = the title's start.  The rule:
        include/efx.h, "noisy sources".  Returns n_frames, the pictures per stream."""
        o = np.zeros(1, dtype=DENOISE_OPTS_DTYPE)
        o[0] = (n_streams, n_frames, luma_spatial, chroma_spatial, luma_temporal, chroma_temporal, src_stride, dst_stride, prev_stride)
        _check(self._ctx, self._lib.efx_denoise(self._ctx, C.byref(surface), o.ctypes.data, _ptr(src), _ptr(prev), _ptr(dst)))
        return n_frames

    def denoise(self, src, *, fmt: str = "i420", width: int, height: int, pitch: int = 0, plane_rows: int = 0,
                luma_spatial: int = 0, chroma_spatial: int = 0, luma_temporal: int = 0, chroma_temporal: int = 0,
                n_streams: int = 1, prev=None):
        """Noisy frames as filtered pictures of the same size, made on the device (denoise_to).  src: a NumPy array or a
        uint8 torch tensor on the decoder's device of shape (n_streams * n_frames, bytes), stream by stream, bytes being
        surface_layout(fmt, width, height, pitch, plane_rows).bytes; fmt "i420", "yv12", "nv12" or "nv21", width and
        height even.  prev: the streams' last pictures of the previous piece, (n_streams, width * height * 3 / 2) as
        this method returned them (array or tensor), None at a title's start.  Returns (n_streams * n_frames, width *
        height * 3 / 2) uint8 packed I420 pictures: what import_pictures(fmt="i420", width=, height=), detect_crop(),
        deinterlace() and detelecine() take; a tensor for a tensor (no host round trip), an array for an array.
        Synchronises: torch's current stream before (tensor input), the library's after."""
        surf, total, src = _surface_source(src, fmt, width, height, pitch, plane_rows)
        if n_streams < 1 or total < 1 or total % n_streams:
            raise ValueError(f"{total} source images do not make {n_streams} streams of equal length")
        for name, t in (("luma_spatial", luma_spatial), ("chroma_spatial", chroma_spatial), ("luma_temporal", luma_temporal),
                        ("chroma_temporal", chroma_temporal)):
            if not 0 <= t <= DENOISE_MAX_THRESHOLD:
                raise ValueError(f"{name}={t!r}: a threshold lies in 0 .. {DENOISE_MAX_THRESHOLD}")
        image = width * height * 3 // 2
        if prev is not None and tuple(prev.shape) != (n_streams, image):
            raise ValueError(f"prev must have shape ({n_streams}, {image}), got {tuple(prev.shape)}")
        stride, dstride = _r16(surf.bytes), _r16(image)
        with self._scratch() as s:
            src_ptr, is_array, _ = self._stage(s, src, total, surf.bytes, stride=stride)
            prev_ptr = self._stage(s, prev, n_streams, image, stride=dstride, what="prev")[0] if prev is not None else None
            if not is_array or not (prev is None or isinstance(prev, np.ndarray)):
                self._wait_for_torch(own_stream_ok=True)
            dst_ptr, fetch = self._rows_out(s, is_array, total, image, dstride)
            self.denoise_to(src_ptr, dst_ptr, surface=surf, n_streams=n_streams, n_frames=total // n_streams, luma_spatial=luma_spatial,
                            chroma_spatial=chroma_spatial, luma_temporal=luma_temporal, chroma_temporal=chroma_temporal, prev=prev_ptr,
                            src_stride=stride, dst_stride=dstride, prev_stride=dstride)
            self.sync()
            return fetch()

    # -- subtitles and logos (efx_overlay) ----------------------------------------------------
    def overlay_to(self, pictures: DeviceBuffer | int, events: DeviceBuffer | int | None, atlas: DeviceBuffer | int | None, *,
                   n_streams: int, n_pictures: int, n_events: int, atlas_bytes: int, first_picture: int = 0, stride: int = 0,
                   status: DeviceBuffer | int | None = None):
        """efx_overlay on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream and in
        place: the n_events records at events (OVERLAY_EVENT_DTYPE, overlay_pack()) whose bitmaps lie in the atlas_bytes
        bytes at atlas are blended into picture j of stream i at pictures + i * stride + j * 101376 (stride 0 = packed),
        picture j being first_picture + j of the title.  status: n_streams uint32 the caller cleared, or None; an event
        that is not valid is not drawn and sets OVERLAY_BAD_EVENT in every word.  The rule: include/efx.h, "subtitles
        and logos"."""
        o = np.zeros(1, dtype=OVERLAY_OPTS_DTYPE)
        o[0] = (n_streams, n_pictures, n_events, 0, first_picture, stride, atlas_bytes)
        _check(self._ctx, self._lib.efx_overlay(self._ctx, o.ctypes.data, _ptr(events), _ptr(atlas), _ptr(pictures), _ptr(status)))

    def overlay(self, pictures, overlays, *, first_picture: int = 0, inplace: bool = False):
        """(n, P, 101376) I420 pictures, as encode() takes them, with a list of Overlay burnt in on the device
        (overlay_to): a uint8 tensor on the decoder's device (a tensor is returned) or a NumPy array (an array is
        returned).  Picture j of every stream is first_picture + j of the title, which is what Overlay.first / .last
        count.  The bitmaps are packed into one atlas (overlay_pack: an array object shared by several events once);
        events that no picture of this piece can show are dropped, the rest is checked on the host (ValueError naming
        the event).  The result is a copy unless inplace=True with a packed, 16-byte aligned tensor, which is then
        changed and returned.  EfxError if the device reports an invalid event all the same.  Synchronises: torch's
        current stream before (tensor input), the library's after."""
        if len(pictures.shape) != 3 or pictures.shape[-1] != FRAME_BYTES or pictures.shape[0] < 1 or pictures.shape[1] < 1:
            raise ValueError(f"pictures must have shape (n, P, {FRAME_BYTES}), got {tuple(pictures.shape)}")
        n, P = int(pictures.shape[0]), int(pictures.shape[1])
        is_array = isinstance(pictures, np.ndarray)
        kept = [(i, o) for i, o in enumerate(overlays) if not (o.last < first_picture or o.first >= first_picture + P or o.stream >= n)]
        if len(kept) > OVERLAY_MAX_EVENTS:
            raise ValueError(f"{len(kept)} events can show in this piece; a call takes {OVERLAY_MAX_EVENTS}")
        events, atlas = overlay_pack([o for _, o in kept], names=[i for i, _ in kept])
        bad = overlay_check(events, atlas.size)
        if bad >= 0:
            raise ValueError(f"event {kept[bad][0]} ({kept[bad][1]!r}) is not a valid efx_overlay_event (include/efx.h, "
                             f"\"subtitles and logos\"): {events[bad]}")
        if inplace and is_array:
            raise ValueError("inplace=True needs a tensor on the device")
        with self._scratch() as s:
            if is_array:
                buf = s.alloc(n * P * FRAME_BYTES)
                buf.upload(np.ascontiguousarray(pictures, dtype=np.uint8))
                ptr, out = buf.ptr, None
            else:
                out = pictures if inplace else pictures.clone().contiguous()
                ptr, _, copied = self._stage(s, out, n * P, FRAME_BYTES, what="pictures")
                if copied:
                    raise ValueError("inplace=True needs a packed, 16-byte aligned tensor")
                self._wait_for_torch()
            if len(events):
                ebuf, abuf = s.alloc(events.nbytes), s.alloc(atlas.size)
                ebuf.upload(events)
                abuf.upload(atlas)
                status = s.zeros(4 * n)
                self.overlay_to(ptr, ebuf, abuf, n_streams=n, n_pictures=P, n_events=len(events), atlas_bytes=atlas.size,
                                first_picture=first_picture, status=status)
                self.sync()
                st = status.download(np.uint32, n)
                if st.any():
                    raise EfxError(-1, f"efx_overlay: status {st.tolist()} (OVERLAY_BAD_EVENT = {OVERLAY_BAD_EVENT})")
            if is_array:
                return buf.download(np.uint8, n * P * FRAME_BYTES).reshape(n, P, FRAME_BYTES)
            return out

    # -- black borders (efx_detect_crop) ----------------------------------------------------
    def detect_crop_to(self, src: DeviceBuffer | int, rects: DeviceBuffer | int, *, n_streams: int, images_per_stream: int,
                       fmt: str, width: int, height: int, limit: int = 24, round: int = 16, full_range: bool = False,
                       src_stride: int = 0, sums: DeviceBuffer | int | None = None, sums_stride: int = 0, surface=None):
        """efx_detect_crop on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: source
        image k (fmt "i420", "rgb24" or "rgbp", width x height) at src + k * src_stride (0 = import_src_bytes() rounded
        up to 16) belongs to stream k // images_per_stream; stream i's record of eight int32 (x, y, w, h, x1, y1, x2,
        y2; the definition: include/efx.h) goes to rects + 32 i.  sums: when given, receives per image the height row
        sums and the width column sums (uint32), image k at + 4 * k * sums_stride bytes (0 = height + width rounded up
        to 4).  surface: an efx_surface from surface_layout() -- the luma is then read as that surface describes it
        (efx_detect_crop_surfaces), fmt must be "i420", width and height the surface's."""
        if fmt not in _PIX_FORMATS:
            raise ValueError(f"unknown format {fmt!r}: one of {sorted(_PIX_FORMATS)}")
        o = _CropOpts(n_streams, images_per_stream, _PIX_FORMATS[fmt], width, height, 1 if full_range else 0, limit, round,
                      src_stride, sums_stride)
        if surface is not None:
            _check(self._ctx, self._lib.efx_detect_crop_surfaces(self._ctx, C.byref(surface), C.byref(o), _ptr(src), _ptr(rects), _ptr(sums)))
            return
        _check(self._ctx, self._lib.efx_detect_crop(self._ctx, C.byref(o), _ptr(src), _ptr(rects), _ptr(sums)))

    def detect_crop(self, src, *, fmt: str | None = None, width: int | None = None, height: int | None = None,
                    images_per_stream: int | None = None, limit: int = 24, round: int = 16,
                    full_range: bool = False, pitch: int = 0, plane_rows: int = 0, src_range: str | None = None) -> np.ndarray:
        """The black borders of source pictures, found on the device (efx_detect_crop): an int32 array of shape
        (n_streams, 8) with x, y, w, h -- the crop for import_pictures(crop=...) -- and the bounds x1, y1, x2, y2 of the
        detected picture (inclusive; x2 < x1: every image was black, the crop is the whole picture).  src as
        import_pictures takes it (arrays and tensors, fmt / width / height likewise).  Every images_per_stream
        consecutive images form a stream with one rectangle, the union of its images; None: all images are one stream.
        A row or column is picture when its mean luma exceeds limit (for RGB sources the luma import_pictures would
        write with this full_range); the rectangle's sides are multiples of round where there is room, even otherwise.
        fmt may also be a surface kind of surface_layout() ("nv12", "p010", ...; "i420" with pitch= or plane_rows=), as
        import_pictures takes it.  src_range: "full" for a full-range YCbCr source, whose black is 0 -- limit then names
        the luma after conversion and the detection runs with colour_source_limit(limit, src_range) (RGB sources:
        ValueError).  Waits for the result."""
        if src_range is not None and src_range not in _COLOUR_RANGES:
            raise ValueError(f"unknown src_range {src_range!r}: 'studio' or 'full'")
        surface = None
        if fmt in _SURFACE_KINDS and (fmt != "i420" or pitch or plane_rows):
            surface, n, src = _surface_source(src, fmt, width, height, pitch, plane_rows)
            fmt, image = "i420", surface.bytes
        else:
            fmt, n, width, height = _import_geometry(src.shape, fmt, width, height)
            image = import_src_bytes(fmt, width, height)
        if not image or n < 1:
            raise ValueError(f"{fmt} pictures of {width} x {height} cannot be read (2 .. 4096, i420: even; n >= 1)")
        if src_range is not None:
            if fmt != "i420":
                raise ValueError("src_range= describes a YCbCr source; for an RGB source full_range= chooses the luma")
            limit = colour_source_limit(limit, src_range)
        per = n if images_per_stream is None else images_per_stream
        if per < 1 or n % per:
            raise ValueError(f"images_per_stream={images_per_stream} does not divide the {n} images")
        stride = _r16(image)
        with self._scratch() as s:
            src_ptr, is_array, _ = self._stage(s, src, n, image, stride=stride)
            if not is_array:
                self._wait_for_torch(own_stream_ok=True)
            return self._detect_rects(s, src_ptr, n // per, per, fmt, width, height, limit, round, full_range, stride, surface)

    def _detect_rects(self, s: _Scratch, src_ptr, n_streams, per, fmt, width, height, limit, round, full_range, stride,
                      surface=None) -> np.ndarray:
        rbuf = s.alloc(32 * n_streams)
        self.detect_crop_to(src_ptr, rbuf, n_streams=n_streams, images_per_stream=per, fmt=fmt, width=width, height=height,
                            limit=limit, round=round, full_range=full_range, src_stride=stride, surface=surface)
        self.sync()
        return rbuf.download(np.int32, 8 * n_streams).reshape(n_streams, 8)

    # -- picture quality (efx_compare_pictures) ------------------------------------------------
    def compare_to(self, ref: DeviceBuffer | int, test: DeviceBuffer | int, recs: DeviceBuffer | int, *, n_images: int,
                   ref_max: int = 0, ref_stride: int = 0, test_stride: int = 0, mb_sse: DeviceBuffer | int | None = None,
                   mb_stride: int = 0):
        """efx_compare_pictures on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream:
        I420 image k of the reference at ref + k * ref_stride and of the picture under test at test + k * test_stride
        (0 = 101376), its 48-byte record (uint64 sse[3], int64 ssim[3] for Y, Cb, Cr; the definition: include/efx.h) to
        recs + 48 k.  ref_max: reference samples above it count as it (0 = no clamp, 248 = the decoder's).  mb_sse: when
        given, receives every macroblock's luma SSE (uint32), image k at + 4 * k * mb_stride bytes (0 = 264)."""
        o = _CompareOpts(n_images, ref_max, ref_stride, test_stride, mb_stride)
        _check(self._ctx, self._lib.efx_compare_pictures(self._ctx, C.byref(o), _ptr(ref), _ptr(test), _ptr(recs), _ptr(mb_sse)))

    def compare(self, ref, test, *, ref_max: int = 0, macroblocks: bool = False) -> CompareResult:
        """PSNR and SSIM of pictures against reference pictures, measured on the device (efx_compare_pictures): ref and
        test are (..., 101376) I420 pictures (the layout encode() takes and export("i420") gives) of the same leading
        shape, uint8 NumPy arrays or torch tensors on the decoder's device (tensors are used in place).  ref_max:
        reference samples above it count as it -- 0 = no clamp, 248 = the decoder's clamp, for a source against its
        reconstruction.  Returns a CompareResult of the leading shape; macroblocks=True adds every macroblock's luma
        SSE.  Synchronises: torch's current stream before (tensor input), the library's after."""
        lead = tuple(ref.shape[:-1])
        if ref.shape[-1] != FRAME_BYTES or tuple(test.shape) != tuple(ref.shape):
            raise ValueError(f"ref and test must have the same shape (..., {FRAME_BYTES}), got {tuple(ref.shape)} and {tuple(test.shape)}")
        n = int(np.prod(lead, dtype=np.int64))
        if n < 1:
            raise ValueError("no pictures to compare")
        with self._scratch() as s:
            ref_ptr, ref_is_array, _ = self._stage(s, ref, n, FRAME_BYTES, what="pictures")
            test_ptr, test_is_array = ref_ptr, ref_is_array
            if test is not ref:
                test_ptr, test_is_array, _ = self._stage(s, test, n, FRAME_BYTES, what="pictures")
            if not (ref_is_array and test_is_array):
                self._wait_for_torch()
            out = s.alloc(48 * n + (264 * 4 * n if macroblocks else 0))
            self.compare_to(ref_ptr, test_ptr, out, n_images=n, ref_max=ref_max, mb_sse=out.ptr + 48 * n if macroblocks else None)
            self.sync()
            recs = out.download(np.uint64, 6 * n).reshape(n, 6)
            mb = None
            if macroblocks:
                mb = np.empty(264 * n, dtype=np.uint32)
                _check(self._ctx, self._lib.efx_memcpy_d2h(self._ctx, mb.ctypes.data, out.ptr + 48 * n, mb.nbytes))
            return _compare_result(recs, lead, mb)

    def _encode_quality(self, q_buf: DeviceBuffer, n: int, P: int, types: np.ndarray) -> CompareResult:
        """The records encode() / encode_av() queued behind the encode; pictures that were not written give zeros."""
        recs = q_buf.download(np.uint64, 6 * n * P).reshape(n * P, 6)
        recs[types.reshape(-1) == 0] = 0
        res = _compare_result(recs, (n, P))
        unwritten = types.reshape(n, P) == 0
        res.psnr[unwritten] = 0.0
        res.ssim[unwritten] = 0.0
        return res

    def import_pictures(self, src, *, fmt: str | None = None, width: int | None = None, height: int | None = None, crop=None,
                        fit: str = "stretch", full_range: bool = False, out=None, sync: bool = True, crop_limit: int = 24,
                        crop_round: int = 16, pitch: int = 0, plane_rows: int = 0, matrix=None, src_range: str | None = None,
                        transfer=None, primaries=None, peak_nits: int | None = None, deinterlace: str | None = None,
                        field_rate: bool = False):
        """Pictures of any size as (n, 101376) I420 pictures of 352 x 192, the layout encode() takes, cropped, scaled and
        converted on the device (efx_import_frames; the arithmetic: include/efx.h).  src: a NumPy array, or a uint8
        torch tensor on the decoder's device, of shape (n, H, W, 3) for "rgb24", (n, 3, H, W) for "rgbp", or
        (n, H * W * 3 // 2) for "i420" together with width= and height=; fmt=None infers the format from the shape (four
        axes: rgb24 when the last one is 3, else rgbp; two axes: i420).  crop = (x, y, w, h) of the source, or "auto":
        the black borders of the call's images, taken as one stream, are found on the device (detect_crop with
        limit=crop_limit, round=crop_round) and cut off; the 32-byte record is read back, which is one synchronisation
        of the library's stream in front of the import.
        fit="stretch" fills the frame; fit="letterbox" keeps the aspect ratio of the source (of the crop, given or
        detected): the picture goes into letterbox_rect(w, h), the largest centred rectangle of that ratio with even
        sides, and the rest of the frame is black; fit="cover" narrows the crop (given, detected or the whole picture)
        to cover_crop(), the largest centred rectangle of the frame's shape inside it, and fills the frame with that.
        full_range: RGB sources only, False = BT.601 studio swing (what MPEG-1 carries).
        fmt may also be a surface kind of surface_layout(): "yv12", "nv12", "nv21", "p010", "p012", "p016", "i010", "i012",
        "i016", or "i420" with pitch= or plane_rows=, together with width=, height=, pitch= (bytes per luma row, 0 =
        packed) and plane_rows= (rows per luma plane, 0 = height).  src then has shape (n, bytes) as uint8, bytes being
        surface_layout(...).bytes, or for the 16-bit kinds (n, bytes / 2) as uint16; the pictures are read where they lie
        (efx_import_surfaces), 16-bit samples rounded to 8 bits.
        matrix, src_range: what a YCbCr source carries -- pass the decoder's matrix_coefficients (or "bt709", "bt601",
        "fcc", "smpte240m", "bt2020", "auto": BT.709 above 576 lines) and "studio" or "full"; the picture is converted to
        the BT.601 studio swing MPEG-1 carries in the same kernel (colour_coefs(); include/efx.h, "source colour").
        Both None: the context's setting (set_import_colour(); off by default).  With src_range="full", crop="auto"
        detects with colour_source_limit(crop_limit, src_range), since such a source's black is 0.  RGB sources take
        neither (ValueError).
        transfer="pq", primaries="bt2020" (or "bt709"), peak_nits=1000: an HDR10 source -- what a decoder reports as
        transfer_characteristics 16 and colour_primaries 9, the peak from MaxCLL or the mastering display -- is tone-mapped
        to the BT.601 SDR picture in the same kernel (hdr_tables(); include/efx.h, "HDR sources"); matrix= (default
        "bt2020") and src_range= then describe the HDR source.  Crop detection needs nothing: PQ studio black is the code
        of SDR studio black.  RGB sources take none of these (ValueError).
        deinterlace="tff" or "bff" (YCbCr 8-bit sources: "i420", "yv12", "nv12", "nv21"; height a multiple of 4): the batch
        is one stream of consecutive interlaced frames with that field first; it is deinterlaced on the device at the
        source's size (deinterlace_to; include/efx.h, "interlaced sources") and the progressive pictures are imported
        with the arguments given, crop="auto" detecting on them.  field_rate=True makes a picture of every field: 2 n
        pictures come back, to be encoded at twice the frame rate (576i25: fps=50).  None, the default, changes nothing.
        deinterlace="auto": the batch, taken as one stream, is scanned on the device first (detect_scan_to, default
        options; one read-back, like crop="auto"): an interlaced stream proceeds as "tff" or "bff" says, a progressive or
        unknown one as None, and telecined film raises ValueError -- it goes through detelecine() first.

        Returns a tensor for tensor input and an array for array input.  out: a preallocated contiguous uint8 tensor
        of n * 101376 elements on this device, or a DeviceBuffer (then returned as is); with out given, array input
        returns out as well.

        The kernels run on the library's stream.  For tensor input torch's current stream is synchronised first unless
        it is the decoder's stream (hip_stream=).  sync=True (default) waits for the import.  sync=False is only safe
        under the conditions export() names: the decoder lives on torch's current stream, or the caller calls sync()
        before using the result."""
        if fit not in ("stretch", "letterbox", "cover"):
            raise ValueError(f"unknown fit {fit!r}: 'stretch', 'letterbox' or 'cover'")
        if isinstance(crop, str) and crop != "auto":
            raise ValueError(f"unknown crop {crop!r}: a rectangle (x, y, w, h), None or 'auto'")
        surface = None
        if fmt in _SURFACE_KINDS and (fmt != "i420" or pitch or plane_rows):
            surface, n, src = _surface_source(src, fmt, width, height, pitch, plane_rows)
            fmt, image = "i420", surface.bytes
        else:
            fmt, n, width, height = _import_geometry(src.shape, fmt, width, height)
            image = import_src_bytes(fmt, width, height)
        if not image or n < 1:
            raise ValueError(f"{fmt} pictures of {width} x {height} cannot be imported (2 .. 4096, i420: even; n >= 1)")
        if (_colour_setting(matrix, src_range) is not None or _hdr_setting(transfer, primaries, matrix, src_range, peak_nits) is not None) \
                and fmt != "i420":
            raise ValueError("matrix=, src_range= and transfer= describe a YCbCr source; an RGB source is converted with BT.601 (full_range=)")
        if src_range is not None:
            crop_limit = colour_source_limit(crop_limit, src_range)
        if deinterlace in (None, "auto") and field_rate:
            raise ValueError("field_rate=True needs deinterlace='tff' or 'bff'")
        if deinterlace is not None:
            if deinterlace not in ("tff", "bff", "auto"):
                raise ValueError(f"unknown deinterlace {deinterlace!r}: 'tff', 'bff', 'auto' or None")
            if fmt != "i420" or (surface is not None and surface.layout not in (SURF_PLANAR8, SURF_SEMI8)):
                raise ValueError("deinterlace= takes 8-bit YCbCr sources: 'i420', 'yv12', 'nv12' or 'nv21'")
            if height % 4 or height < 8:
                raise ValueError(f"an interlaced source's height must be a multiple of 4 from 8, got {height}")
        stride = _r16(image)
        with self._scratch() as s:
            src_ptr, is_array, copied = self._stage(s, src, n, image, stride=stride)
            waited = not is_array and self._wait_for_torch(own_stream_ok=True)
            sync = sync or (copied and waited)  # (torch may hand a staging copy's memory out again on its own stream)
            if deinterlace == "auto":
                deinterlace = self._scan_for_import(s, src_ptr, surface if surface is not None else surface_layout("i420", width, height), n, stride)
            if deinterlace is not None:
                # the progressive pictures, packed I420 at the source's size, in a buffer of this call: the import's source
                dstride = _r16(width * height * 3 // 2)
                rate = "field" if field_rate else "frame"
                dbuf = s.alloc(deinterlace_count(n, rate=rate) * dstride)
                n = self.deinterlace_to(src_ptr, dbuf, surface=surface if surface is not None else surface_layout("i420", width, height),
                                        n_frames=n, first_field=deinterlace, rate=rate, src_stride=stride, dst_stride=dstride)
                src_ptr, stride, surface = dbuf.ptr, dstride, None
            nbytes = n * FRAME_BYTES
            if isinstance(crop, str):
                rec = self._detect_rects(s, src_ptr, 1, n, fmt, width, height, crop_limit, crop_round, full_range, stride, surface)
                crop = tuple(int(v) for v in rec[0, :4])
            if fit == "cover":
                crop = cover_crop(width, height, crop)
            rect = None
            if fit == "letterbox":
                rect = letterbox_rect(*(crop[2:] if crop else (width, height)))
            obuf = None
            if isinstance(out, DeviceBuffer):
                if out.nbytes < nbytes:
                    raise ValueError(f"out holds {out.nbytes} bytes, the import needs {nbytes}")
                result, ptr = out, out.ptr
            elif out is None and is_array:
                obuf = s.alloc(nbytes)
                result, ptr = None, obuf.ptr
            else:
                import torch
                device = torch.device("cuda", self.device)
                if out is None:
                    out = torch.empty((n, FRAME_BYTES), dtype=torch.uint8, device=device)
                if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != device:
                    raise ValueError(f"out must be a uint8 tensor on {device}")
                if not out.is_contiguous() or out.numel() != nbytes:
                    raise ValueError(f"out must be contiguous with {nbytes} elements (shape {(n, FRAME_BYTES)})")
                result, ptr = out.view(n, FRAME_BYTES), out.data_ptr()
            self.import_to(src_ptr, ptr, n_images=n, fmt=fmt, width=width, height=height, crop=crop, dst_rect=rect,
                           full_range=full_range, src_stride=stride, surface=surface, matrix=matrix, src_range=src_range,
                           transfer=transfer, primaries=primaries, peak_nits=peak_nits)
            if sync or is_array or deinterlace is not None:
                self.sync()  # (the buffers of this call that the import reads or writes are freed on the way out)
            if obuf is not None:
                result = obuf.download(np.uint8, nbytes).reshape(n, FRAME_BYTES)
            return result

    def _scan_for_import(self, s: _Scratch, src_ptr, surface, n: int, stride: int):
        """deinterlace="auto" of import_pictures: the call's n images scanned as one stream (detect_scan_to with the
        default options, one read-back): "tff" / "bff" for an interlaced stream, None for a progressive or unknown one;
        a telecined one is the caller's to detelecine first."""
        if n < 2:
            return None  # (no frame has a predecessor: unknown)
        fbuf, rbuf = s.alloc(n * SCAN_FRAME_DTYPE.itemsize), s.alloc(SCAN_REC_DTYPE.itemsize)
        self.detect_scan_to(src_ptr, fbuf, rbuf, surface=surface, n_frames=n, src_stride=stride)
        self.sync()
        res = scan_verdict(rbuf.download(SCAN_REC_DTYPE, 1)[0])
        if res.kind == "telecined":
            raise ValueError(f"deinterlace='auto': the pictures are telecined film ({res.first_field} field first): make the film's frames "
                             f"with detelecine(first_field={res.first_field!r}) and import those")
        return {"top": "tff", "bottom": "bff"}[res.first_field] if res.kind == "interlaced" else None

    # -- MPEG-1 encode (efx_encode) ------------------------------------------------------------
    def encode_to(self, src: DeviceBuffer | int, dst: DeviceBuffer | int, length: DeviceBuffer | int,
                  status: DeviceBuffer | int, *, n_streams: int, n_pictures: int, qscale: int = 8, gop: int = 12,
                  search: int = 7, fmt: int = FORMAT_TS, cont: bool = False, first_pts: int = 0, src_stride: int = 0,
                  dst_stride: int = 0, recon: DeviceBuffer | int | None = None, bitrate: int | None = None,
                  vbv_bits: int = 250_000, qmin: int = 3, qmax: int = 31, qscale_out: DeviceBuffer | int | None = None, fps=None,
                  scene_cut: int | bool | None = None, min_gop: int | None = None, aq: int | bool | None = None):
        """efx_encode on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: stream i's
        pictures at src + i * src_stride (0 = packed), its bytes appended to dst + i * dst_stride (0 = efx_encode_bound),
        uint32 byte counts and status bits to length / status, the reconstruction to recon (optional).

        bitrate (bit/s): efx_encode_rc instead -- every picture's quantiser chosen on the device under the buffer model
        of efx.h (vbv_bits, qmin, qmax; qscale is the first picture's), the n_streams x n_pictures quantisers to
        qscale_out (optional).  The defaults are the profile of the reference's indexer.

        fps: the picture rate of fresh streams, one of PICTURE_RATES as Fraction, "24000/1001", int or 23.976 / 29.97 /
        59.94; None = 30000/1001 (efx_encode_set_picture_rate in front of every cont=False call, so a rate never stays in
        force from an earlier call).  With cont=True the streams keep their rate: fps must be None or that rate.

        scene_cut: fresh streams code an I picture where the content changes (efx_encode_set_scene_cut, likewise in front
        of every cont=False call): the threshold 1 .. 256, True = SCENE_CUT_DEFAULT, None / False / 0 = off; min_gop: no
        such I picture sooner than this after the last one, None = max(1, gop // 2).  With cont=True the streams keep what
        they started with and both are ignored.

        aq: fresh streams give every macroblock its own quantiser around the picture's (efx_encode_set_adaptive_quant,
        likewise in front of every cont=False call): the strength 1 .. 256, True = AQ_DEFAULT, None / False / 0 = off.
        With cont=True the streams keep what they started with and it is ignored."""
        if not cont:
            strength = _AdaptiveQuant(AQ_DEFAULT if aq is True else int(aq or 0))
            _check(self._ctx, self._lib.efx_encode_set_adaptive_quant(self._ctx, C.byref(strength)))
            threshold = SCENE_CUT_DEFAULT if scene_cut is True else int(scene_cut or 0)
            sc = _SceneCut(threshold, max(1, gop // 2) if min_gop is None else int(min_gop))
            _check(self._ctx, self._lib.efx_encode_set_scene_cut(self._ctx, C.byref(sc)))
        if cont:
            if fps is not None and _fps_code(fps) != self._enc_rate_code:
                raise ValueError(f"fps={fps!r} with cont=True: the streams run at {PICTURE_RATES[self._enc_rate_code]}")
        else:
            code = _fps_code(fps)
            _check(self._ctx, self._lib.efx_encode_set_picture_rate(self._ctx, code))
        o = _EncodeOpts(n_streams, n_pictures, fmt, qscale, gop, search, 1 if cont else 0, first_pts,
                        src_stride or n_pictures * FRAME_BYTES, dst_stride or encode_bound(fmt, n_pictures))
        if bitrate is None:
            _check(self._ctx, self._lib.efx_encode(self._ctx, C.byref(o), _ptr(src), _ptr(dst), _ptr(length), _ptr(status), _ptr(recon)))
        else:
            r = _EncodeRate(bitrate, vbv_bits, qmin, qmax)
            _check(self._ctx, self._lib.efx_encode_rc(self._ctx, C.byref(o), C.byref(r), _ptr(src), _ptr(dst), _ptr(length), _ptr(status),
                                                      _ptr(recon), _ptr(qscale_out)))
        if not cont:
            self._enc_rate_code = code
        return o.dst_stride

    def encode(self, pictures, *, qscale: int = 8, gop: int = 12, search: int = 7, fmt: int = FORMAT_TS, cont: bool = False,
               first_pts: int = 0, recon: bool = False, dst_stride: int = 0, bitrate: int | None = None,
               vbv_bits: int = 250_000, qmin: int = 3, qmax: int = 31, fps=None, scene_cut: int | bool | None = None,
               min_gop: int | None = None, quality: bool = False, aq: int | bool | None = None) -> EncodeResult:
        """Encode (n, P, 101376) I420 pictures (the layout export("i420") writes) into n MPEG-1 streams of P pictures: a uint8
        torch tensor on the decoder's device or a NumPy array.  Stream i takes the pictures of row i (the order export()
        gives streams).  Returns each stream's bytes, its status bits and, with recon=True, what a decoder reconstructs
        (a tensor on the device for tensor input, else an array).  cont=True continues the streams of the previous encode
        (qscale and search may change).  Synchronises: torch's current stream before (tensor input), the library's after.

        dst_stride: bytes of device memory for each stream's output, 0 = encode_bound(fmt, P), the size that can never fill
        up -- about 357 kB (ES) / 365 kB (TS) per picture, 10 to 100 times what a picture usually takes: 1024 streams x 24
        TS pictures reserve some 9 GB for the call.  A smaller region is fine where the caller knows its content; a stream
        that does not fit ends after its last whole picture with status ENCODE_FULL (its bytes so far are returned) and can
        only be encoded again from the start (cont=False), with a larger dst_stride.

        bitrate (bit/s of the bytes in fmt): rate control (efx_encode_rc) under a buffer of vbv_bits bits, quantisers
        qmin..qmax, qscale for the first picture of a fresh stream; the result's qscales holds every picture's quantiser
        and status may carry ENCODE_VBV.  cont=True must keep bitrate and vbv_bits.

        fps: the streams' picture rate as for encode_to (None = 30000/1001): picture k carries first_pts +
        picture_pts_offset(fps, k).

        scene_cut, min_gop: as for encode_to.  The result's types holds every picture's type and cut_scores its two sums
        (zeros while scene cuts are off), with or without the option.

        aq: adaptive quantisation as for encode_to; encode_mb_quant(stream, picture) afterwards gives a picture's
        quantisers.

        quality=True: the reconstruction is kept on the device (in a buffer of the call's own when recon=False) and
        compared with the source right behind the encode, on the same stream (compare_to with ref_max=248, the
        decoder's clamp); the result's quality is the CompareResult of shape (n, P), zeros for pictures that were not
        written.  Without it nothing is launched or allocated for this."""
        lead = tuple(pictures.shape[:-1])
        if len(lead) != 2 or pictures.shape[-1] != FRAME_BYTES:
            raise ValueError(f"pictures must have shape (n, P, {FRAME_BYTES}), got {tuple(pictures.shape)}")
        n, P = lead
        with self._scratch() as s:
            src_ptr, is_array, _ = self._stage(s, pictures, n * P, FRAME_BYTES, what="pictures")
            rec_t = None
            if not is_array:
                self._wait_for_torch()
                if recon:
                    import torch
                    rec_t = torch.empty((n, P, FRAME_BYTES), dtype=torch.uint8, device=torch.device("cuda", self.device))
            stride = dst_stride or encode_bound(fmt, P)
            dst, meta = s.alloc(n * stride), s.alloc(2 * 4 * n + 16)
            q_buf = s.alloc(n * P) if bitrate is not None else None
            rec_buf = rec_ptr = None
            if rec_t is not None:
                rec_ptr = rec_t.data_ptr()
            elif recon or quality:
                rec_buf = s.alloc(n * P * FRAME_BYTES)
                rec_ptr = rec_buf.ptr
            status_off = _r16(4 * n)
            self.encode_to(src_ptr, dst, meta.ptr, meta.ptr + status_off, n_streams=n, n_pictures=P, qscale=qscale, gop=gop,
                           search=search, fmt=fmt, cont=cont, first_pts=first_pts, dst_stride=stride, recon=rec_ptr,
                           bitrate=bitrate, vbv_bits=vbv_bits, qmin=qmin, qmax=qmax, qscale_out=q_buf, fps=fps, scene_cut=scene_cut,
                           min_gop=min_gop, aq=aq)
            qual_buf = None
            if quality and n * P:
                qual_buf = s.alloc(48 * n * P)
                self.compare_to(src_ptr, rec_ptr, qual_buf, n_images=n * P, ref_max=248)
            self.sync()
            streams, st = self._download_streams(dst.ptr, stride, meta.ptr, meta.ptr + status_off, n)
            out_rec = rec_t
            if rec_t is None and recon:
                out_rec = rec_buf.download(np.uint8, n * P * FRAME_BYTES).reshape(n, P, FRAME_BYTES)
            qs = q_buf.download(np.uint8, n * P).reshape(n, P) if q_buf is not None else None
            info = self.encode_picture_info(n)
            types = np.ascontiguousarray(info["type"])
            qual = self._encode_quality(qual_buf, n, P, types) if qual_buf is not None else None
            return EncodeResult(streams, st, out_rec, qs, types, np.stack([info["cut_i"], info["cut_p"]], axis=-1), qual)

    def encode_picture_info(self, n_streams: int) -> np.ndarray:
        """The pictures of the latest encode call (efx_encode_picture_info; synchronises): a structured array
        (n_streams, P) with the fields cut_i, cut_p (uint32) and type (uint8: PICTURE_I, PICTURE_P, PICTURE_CUT_I, 0 = not
        written)."""
        count = self._lib.efx_encode_picture_info(self._ctx, 0, None, 0)
        if count < 0:
            _check(self._ctx, count)
        out = np.zeros((n_streams, count), dtype=ENC_PICTURE_INFO_DTYPE)
        for i in range(n_streams):
            got = self._lib.efx_encode_picture_info(self._ctx, i, out[i].ctypes.data_as(C.POINTER(_EncPictureInfo)), count)
            if got < 0:
                _check(self._ctx, got)
        return out

    def encode_mb_quant(self, stream: int, picture: int) -> np.ndarray:
        """The quantisers of one picture of the latest encode call, which ran with aq (efx_encode_mb_quant; synchronises):
        a (12, 22) uint8 array, all zero for a picture that was not written."""
        out = np.zeros((12, 22), dtype=np.uint8)
        _check(self._ctx, self._lib.efx_encode_mb_quant(self._ctx, stream, picture, out.ctypes.data))
        return out

    # -- video / audio out ----------------------------------------------------------------
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def composite_fields(self, dst: DeviceBuffer | int, first_stream: int, n_streams: int, slot: int, ntsc: bool,
                         frame_counter: int):
        ptr = dst.ptr if isinstance(dst, DeviceBuffer) else dst
        _check(self._ctx, self._lib.efx_composite_fields(self._ctx, first_stream, n_streams, slot, 1 if ntsc else 0,
                                                         frame_counter, ptr))

    def composite_fields_ex(self, dst: DeviceBuffer | int, first_stream: int, n_streams: int, slot: int, ntsc: bool,
                            frame_counter: int, other_slot: int | None = None, hscroll: int = 0,
                            overlay: DeviceBuffer | int | None = None, overlay_stride: int = 0, overlay_blend: int = 0,
                            overlay_progress: int = 0):
        """video_isr with the two-frame slide (_hscroll) and the overlay / progress bar (composite())."""
        o = _FieldOpts(first_stream, n_streams, slot, slot if other_slot is None else other_slot, 1 if ntsc else 0,
                       frame_counter, hscroll, _ptr(overlay), overlay_stride, overlay_blend, overlay_progress)
        _check(self._ctx, self._lib.efx_composite_fields_ex(self._ctx, C.byref(o), _ptr(dst)))

    def demux_audio(self, streams, audio: DeviceBuffer | int, stride: int, audio_len: DeviceBuffer | int):
        """Audio elementary streams (push_audio's input) of a batch of transport streams, on the device."""
        arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray, memoryview))
                else np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
        n = len(arrs)
        ptrs = (_P * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        _check(self._ctx, self._lib.efx_demux_audio(self._ctx, n, ptrs, lens, _ptr(audio), stride, _ptr(audio_len)))

    def index_streams(self, streams, trick_speed=None, bin_size: int = 7500, samples_cap: int = 0):
        """make_index + pts2seq for a batch of transport streams.  Returns [(rec dict, samples)]."""
        arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray, memoryview))
                else np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
        n = len(arrs)
        cap = samples_cap or max(16, max(a.size // 188 for a in arrs) + 2)
        ptrs = (_P * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        recs = (_IdxRec * n)()
        samples = np.zeros((n, cap), dtype=np.uint32)
        sp = None if trick_speed is None else (C.c_uint32 * n)(*trick_speed)
        _check(self._ctx, self._lib.efx_index_streams(self._ctx, n, ptrs, lens, sp, bin_size, recs, samples.ctypes.data, cap))
        return [({f: getattr(recs[i], f) for f, _ in _IdxRec._fields_}, samples[i, :recs[i].sample_count].copy())
                for i in range(n)]

    def sbc_decode(self, n_streams: int, frames: DeviceBuffer | int, stream_stride: int, frame_bytes: int, n_frames: int,
                   state: DeviceBuffer | int, pcm: DeviceBuffer | int, pcm_stride: int, ret: DeviceBuffer | int | None = None,
                   pcm_count: DeviceBuffer | int | None = None, probe_first: bool = False):
        _check(self._ctx, self._lib.efx_sbc_decode(self._ctx, n_streams, _ptr(frames), stream_stride, frame_bytes, n_frames,
                                                   _ptr(state), _ptr(pcm), pcm_stride, _ptr(ret), _ptr(pcm_count), 1 if probe_first else 0))

    # -- sound in (efx_import_pcm) -----------------------------------------------------------
    def import_pcm_to(self, src: DeviceBuffer | int, state: DeviceBuffer | int | None, dst: DeviceBuffer | int, *, n_streams: int,
                      n_in: int, in_rate: int, out_rate: int = 48000, channels: int = 1, layout: int = PCM_INTERLEAVED, weights=None,
                      first_in: int = 0, src_stride: int = 0, dst_stride: int = 0) -> int:
        """efx_import_pcm on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: stream i's
        n_in frames of `channels` int16 samples at src + i x src_stride elements (0 = n_in x channels rounded up to 8), its
        mono samples at out_rate at dst + i x dst_stride elements (0 = the call's output count rounded up to 8), the
        streams' states (import_pcm_state_bytes() each, zeros = fresh; None only for equal rates) updated in place.
        weights: up to 8 Q15 downmix weights (None: 32768 // channels each).  Returns the call's output count."""
        w = [int(v) for v in (weights if weights is not None else ())]
        if len(w) > 8:
            raise ValueError("at most 8 downmix weights")
        n_out = import_pcm_out_samples(in_rate, out_rate, first_in, n_in) if n_in >= 0 else -1
        o = _ImportPcmOpts(n_streams, n_in, in_rate, out_rate, channels, layout, (C.c_int * 8)(*(w + [0] * (8 - len(w)))), first_in,
                           src_stride or _r8(max(0, n_in * channels)), dst_stride or _r8(max(0, n_out)))
        _check(self._ctx, self._lib.efx_import_pcm(self._ctx, C.byref(o), _ptr(src), _ptr(state), _ptr(dst)))
        return n_out

    def import_pcm(self, pcm, *, rate: int, out_rate: int = 48000, layout: str = "interleaved", weights=None, cont: bool = False,
                   flush: bool = False):
        """int16 PCM of any rate (8 .. 192 kHz, at most 4 x out_rate) and 1 .. 8 channels as mono at out_rate (16000, 32000,
        44100 or 48000), the input of sbc_encode(), downmixed and resampled on the device (efx_import_pcm; the arithmetic:
        include/efx.h).  pcm: a NumPy array, or an int16 torch tensor on the decoder's device, of shape [n, frames] (mono)
        or [n, frames, channels] (layout="interleaved") or [n, channels, frames] (layout="planar").  weights: Q15 downmix
        weights, one per channel (None: 32768 // channels each).  Returns an int16 torch tensor [n, n_out] on the device,
        n_out = ceil(frames x out_rate / rate) for a fresh stream.

        cont=True continues the streams of this object's previous import_pcm (the filter's history and the position are
        kept); otherwise the streams start afresh.  flush=True appends the filter's delay W = import_pcm_delay(rate,
        out_rate) of zero frames, so that the tail of the input comes out.  Synchronises torch's current stream before and
        the library's after."""
        import torch
        device = torch.device("cuda", self.device)
        if layout not in _PCM_LAYOUTS:
            raise ValueError(f"unknown layout {layout!r}: 'interleaved' or 'planar'")
        if isinstance(pcm, np.ndarray):
            pcm = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int16)).to(device)
        if not isinstance(pcm, torch.Tensor) or pcm.dtype != torch.int16 or pcm.device != device or pcm.dim() not in (2, 3):
            raise ValueError(f"pcm must be int16 [n, frames] or [n, frames, channels] on {device} (or a NumPy array)")
        if pcm.dim() == 2:
            pcm = pcm.unsqueeze(2 if layout == "interleaved" else 1)
        n = int(pcm.shape[0])
        frames, channels = (int(pcm.shape[1]), int(pcm.shape[2])) if layout == "interleaved" else (int(pcm.shape[2]), int(pcm.shape[1]))
        W = import_pcm_delay(rate, out_rate)
        if W < 0 or not 1 <= channels <= 8 or n < 1:
            raise ValueError("rate, out_rate or the channel count out of range")
        if flush and W:
            pcm = torch.cat([pcm, torch.zeros((n, W, channels) if layout == "interleaved" else (n, channels, W), dtype=torch.int16,
                                              device=device)], dim=1 if layout == "interleaved" else 2)
            frames += W
        if frames < 1:
            raise ValueError("no input frames")
        key = (n, rate, out_rate, channels)
        st = getattr(self, "_import_pcm_state", None)
        if not cont or st is None or st[0] != key:
            if cont:
                raise EfxError(-5, "import_pcm: cont without a previous import_pcm of as many streams, channels and the same rates")
            st = (key, torch.zeros((n, import_pcm_state_bytes()), dtype=torch.uint8, device=device), 0)
        _, state, first_in = st
        n_out = import_pcm_out_samples(rate, out_rate, first_in, frames)
        if n_out < 0:
            raise ValueError("too many frames for one call")
        src_stride, dst_stride = _r8(frames * channels), _r8(max(n_out, 1))
        with self._scratch() as s:
            src_ptr, _, _ = self._stage(s, pcm, n, frames * channels, stride=src_stride, dtype=np.int16, what="pcm")
            out = torch.zeros((n, dst_stride), dtype=torch.int16, device=device)
            self._wait_for_torch()
            self.import_pcm_to(src_ptr, state.data_ptr(), out.data_ptr(), n_streams=n, n_in=frames, in_rate=rate,
                               out_rate=out_rate, channels=channels, layout=_PCM_LAYOUTS[layout], weights=weights, first_in=first_in,
                               src_stride=src_stride, dst_stride=dst_stride)
            self.sync()
        self._import_pcm_state = (key, state, first_in + frames)
        return out[:, :n_out]

    # -- programme loudness (efx_loudness_steps, efx_loudness_gate, efx_pcm_gain) ------------------
    def loudness_steps_to(self, pcm: DeviceBuffer | int, state: DeviceBuffer | int, steps: DeviceBuffer | int, *, n_streams: int,
                          n_samples: int, rate: int, first_sample: int = 0, first_step: int | None = None, pcm_stride: int = 0,
                          steps_stride: int = 0) -> int:
        """efx_loudness_steps on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: stream
        i's n_samples mono int16 samples at pcm + i x pcm_stride elements (0 = n_samples rounded up to 8); every 100 ms step
        that becomes whole is appended as a 16-byte record (LOUDNESS_STEP_DTYPE) at steps + (i x steps_stride + first_step)
        records (first_step None = first_sample // step; steps_stride 0 = first_step + the call's steps); the streams'
        states (loudness_state_bytes(rate) each, zeros = fresh) are updated in place.  A title fed in pieces carries
        first_sample (+= n_samples) and the state on.  Returns the count appended."""
        if first_step is None:
            first_step = first_sample // max(1, rate // 10)
        n_new = loudness_step_count(rate, first_sample, n_samples) if n_samples >= 0 else -1
        o = _LoudnessStepsOpts(n_streams, n_samples, rate, first_step, first_sample, pcm_stride or (max(0, n_samples) + 7) // 8 * 8,
                               steps_stride or first_step + max(0, n_new))
        ret = self._lib.efx_loudness_steps(self._ctx, C.byref(o), _ptr(pcm), _ptr(state), _ptr(steps))
        if ret < 0:
            _check(self._ctx, ret)
        return ret

    def loudness_gate_to(self, steps: DeviceBuffer | int, state: DeviceBuffer | int | None, recs: DeviceBuffer | int, *,
                         n_streams: int, n_steps: int, rate: int, target: float = -23.0, peak: float = -1.0, thresholds=None,
                         steps_stride: int = 0):
        """efx_loudness_gate on raw device memory, asynchronous on the library's stream: n_steps step records per stream
        (steps_stride records apart, 0 = n_steps) become one 32-byte record per stream (LOUDNESS_REC_DTYPE) at recs: both
        gates, the largest block, the peak (with a state: its samples included) and the gain to `target` LUFS under `peak`
        dBFS.  thresholds: (abs_thr, target_ms, ceiling) instead of loudness_thresholds(rate, target, peak)."""
        a, t, c = thresholds if thresholds is not None else loudness_thresholds(rate, target, peak)
        o = _LoudnessGateOpts(n_streams, n_steps, rate, a, t, c, steps_stride or max(0, n_steps))
        _check(self._ctx, self._lib.efx_loudness_gate(self._ctx, C.byref(o), _ptr(steps), _ptr(state), _ptr(recs)))

    def pcm_gain_to(self, src: DeviceBuffer | int, recs: DeviceBuffer | int | None, dst: DeviceBuffer | int, *, n_streams: int,
                    n_samples: int, fixed_gain_q12: int = 4096, src_stride: int = 0, dst_stride: int = 0):
        """efx_pcm_gain on raw device memory, asynchronous on the library's stream: dst = clamp16((src x g + 2048) >> 12),
        each stream's g read on the device from its record at recs (None: fixed_gain_q12 for all).  dst may be src.
        Strides in elements, 0 = n_samples rounded up to 8."""
        r8 = (max(0, n_samples) + 7) // 8 * 8
        o = _PcmGainOpts(n_streams, n_samples, fixed_gain_q12, src_stride or r8, dst_stride or r8)
        _check(self._ctx, self._lib.efx_pcm_gain(self._ctx, C.byref(o), _ptr(src), _ptr(recs), _ptr(dst)))

    # -- peak limiter (efx_limit_peaks, efx_pcm_limit) ------------------------------------------------
    def limit_peaks_to(self, pcm: DeviceBuffer | int, peaks: DeviceBuffer | int, *, n_streams: int, n_samples: int, rate: int,
                       first_sample: int = 0, peaks_first: int = 0, pcm_stride: int = 0, peaks_stride: int = 0):
        """efx_limit_peaks on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: the peak
        (uint16, 0 .. 32768) of every block of limit_block(rate) samples of stream i's n_samples samples at pcm +
        i x pcm_stride elements (0 = n_samples rounded up to 8) goes to entry first_sample / Bk - peaks_first onwards of
        the stream's row of peaks_stride entries (0 = just those).  first_sample is a multiple of Bk, and so is n_samples
        on every piece but a stream's last."""
        bk = max(1, limit_block(rate))
        o = np.zeros(1, dtype=LIMIT_PEAKS_OPTS_DTYPE)
        o[0] = (n_streams, n_samples, rate, 0, first_sample, peaks_first, pcm_stride or (max(0, n_samples) + 7) // 8 * 8,
                peaks_stride or max(0, first_sample // bk - peaks_first) + -(-max(0, n_samples) // bk))
        _check(self._ctx, self._lib.efx_limit_peaks(self._ctx, o.ctypes.data, _ptr(pcm), _ptr(peaks)))

    def pcm_limit_to(self, src: DeviceBuffer | int, peaks: DeviceBuffer | int, recs: DeviceBuffer | int | None, dst: DeviceBuffer | int,
                     *, n_streams: int, n_samples: int, rate: int, n_peaks: int, half_window: int = 0, first_sample: int = 0,
                     peaks_first: int = 0, target: float = -23.0, peak: float = -1.0, thresholds=None, fixed_gain_q12: int = 4096,
                     src_stride: int = 0, dst_stride: int = 0, peaks_stride: int = 0):
        """efx_pcm_limit on raw device memory, asynchronous on the library's stream: the look-ahead limiter of include/efx.h
        ("peak limiter") over stream i's n_samples samples that begin at stream sample first_sample, with the block peaks
        limit_peaks_to left: entry 0 of a row (n_peaks entries, peaks_stride apart, 0 = n_peaks) is stream block
        peaks_first, a block outside the row counts as silent.  Each stream's gain is worked out on the device from its
        record at recs (those of loudness_gate_to) and the target -- thresholds: (abs_thr, target_ms, ceiling) instead of
        loudness_thresholds(rate, target, peak) -- or is fixed_gain_q12 for all when recs is None; the ceiling is `peak`
        dBFS.  half_window: H in blocks of about 1 ms, 1 .. 64, 0 = 32.  dst may be src.  Sample strides in elements, 0 =
        n_samples rounded up to 8.

        A title fed in pieces takes two passes, as normalize() explains: loudness_steps_to and limit_peaks_to over every
        piece (the peaks into one row for the whole title, or the caller keeps 2H + 1 blocks either side of each piece),
        one loudness_gate_to, then pcm_limit_to per piece."""
        _, t, c = thresholds if thresholds is not None else loudness_thresholds(rate, target, peak)
        r8 = (max(0, n_samples) + 7) // 8 * 8
        o = np.zeros(1, dtype=LIMIT_OPTS_DTYPE)
        o[0] = (n_streams, n_samples, rate, half_window, c, fixed_gain_q12, n_peaks, 0, first_sample, peaks_first, t, src_stride or r8,
                dst_stride or r8, peaks_stride or max(0, n_peaks))
        _check(self._ctx, self._lib.efx_pcm_limit(self._ctx, o.ctypes.data, _ptr(src), _ptr(peaks), _ptr(recs), _ptr(dst)))

    def _limit_queue(self, s_peaks: DeviceBuffer, src_ptr: int, recs, dst_ptr: int, n: int, samples: int, stride: int, rate: int,
                     half_window: int, thr, fixed_gain_q12: int = 4096):
        """peaks -> limit over whole fresh streams with a peaks buffer of n x ceil(samples / Bk) entries: launches only."""
        nb = _limit_blocks(samples, rate)
        self.limit_peaks_to(src_ptr, s_peaks, n_streams=n, n_samples=samples, rate=rate, pcm_stride=stride, peaks_stride=nb)
        self.pcm_limit_to(src_ptr, s_peaks, recs, dst_ptr, n_streams=n, n_samples=samples, rate=rate, n_peaks=nb,
                          half_window=half_window, thresholds=thr, fixed_gain_q12=fixed_gain_q12, src_stride=stride,
                          dst_stride=stride, peaks_stride=nb)

    def limit(self, pcm, rate: int, *, gain_q12: int = 4096, peak: float = -1.0, half_window: int = 32):
        """The peak limiter alone: mono int16 PCM [n_streams, samples] at `rate` (a NumPy array or a torch tensor on the
        decoder's device), every stream whole, scaled by gain_q12 / 4096 with the gain reduced smoothly around the samples
        that would pass `peak` dBFS (include/efx.h, "peak limiter"): peaks -> limit queued back to back.  Returns int16
        [n_streams, samples] of the input's kind; no output sample is above the ceiling."""
        import torch
        device = torch.device("cuda", self.device)
        is_array = isinstance(pcm, np.ndarray)
        if is_array:
            pcm = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int16)).to(device)
        if len(getattr(pcm, "shape", ())) != 2 or pcm.shape[1] < 1:
            raise ValueError(f"pcm must be int16 [n_streams, samples] on {device} (or a NumPy array)")
        n, samples = int(pcm.shape[0]), int(pcm.shape[1])
        n_peaks = _limit_blocks(samples, rate)
        stride = _r8(samples)
        thr = loudness_thresholds(rate, -23.0, peak)
        with self._scratch() as s:
            src_ptr, _, _ = self._stage(s, pcm, n, samples, stride=stride, dtype=np.int16, what="pcm")
            out = torch.empty((n, stride), dtype=torch.int16, device=device)
            d_peaks = s.alloc(_r16(2 * n * n_peaks))
            self._wait_for_torch()
            self._limit_queue(d_peaks, src_ptr, None, out.data_ptr(), n, samples, stride, rate, half_window, thr, gain_q12)
            self.sync()
        return out[:, :samples].cpu().numpy() if is_array else out[:, :samples]

    def _loudness_buffers(self, s: _Scratch, n: int, samples: int, rate: int, target: float, peak: float):
        """What measuring n fresh streams of `samples` samples needs, made ready in the scratch s: (state (zeroed), steps,
        records) on the device, the step count and the thresholds.  The upload synchronises the library's stream, so
        this comes before anything is queued that the host is not to wait for."""
        n_steps = loudness_step_count(rate, 0, samples)
        if n_steps < 0:
            raise ValueError("rate must be 16000, 32000, 44100 or 48000")
        thr = loudness_thresholds(rate, target, peak)
        return (s.zeros(n * loudness_state_bytes(rate)), s.alloc(16 * n * max(1, n_steps)), s.alloc(32 * n)), n_steps, thr

    def _loudness_queue(self, src_ptr: int, n: int, samples: int, stride: int, rate: int, prepared):
        """steps -> gate with _loudness_buffers' result: launches only, nothing synchronised.  Returns the records' buffer."""
        (d_state, d_steps, d_recs), n_steps, thr = prepared
        self.loudness_steps_to(src_ptr, d_state, d_steps, n_streams=n, n_samples=samples, rate=rate, pcm_stride=stride,
                               steps_stride=max(1, n_steps))
        self.loudness_gate_to(d_steps, d_state, d_recs, n_streams=n, n_steps=n_steps, rate=rate, thresholds=thr,
                              steps_stride=max(1, n_steps))
        return d_recs

    @staticmethod
    def _loudness_result(recs: np.ndarray, rate: int) -> LoudnessResult:
        with np.errstate(divide="ignore"):
            return LoudnessResult(
                integrated=np.array([loudness_lufs(int(v), rate) for v in recs["gated_mean"]], dtype=np.float64),
                momentary_max=np.array([loudness_lufs(int(v), rate) for v in recs["max_block"]], dtype=np.float64),
                peak_dbfs=20.0 * np.log10(recs["peak"].astype(np.float64) / 32768.0),
                gain_db=20.0 * np.log10(recs["gain_q12"].astype(np.float64) / 4096.0),
                gain_q12=recs["gain_q12"].astype(np.int32), n_blocks=recs["n_blocks"].astype(np.int64),
                n_gated=recs["n_gated"].astype(np.int64))

    def loudness(self, pcm, rate: int, *, target: float = -23.0, peak: float = -1.0) -> LoudnessResult:
        """Programme loudness of mono int16 PCM [n_streams, samples] at `rate` (16000, 32000, 44100 or 48000; a NumPy array
        or a torch tensor on the decoder's device), every stream from its first sample, measured on the device by ITU-R
        BS.1770-4 / EBU R 128 (include/efx.h), and the gain that would take each stream to `target` LUFS with its sample
        peak no higher than `peak` dBFS.  Synchronises torch's current stream before and the library's after."""
        return self._measure(pcm, rate, target, peak, gain=False)[1]

    def normalize(self, pcm, rate: int, *, target: float = -23.0, peak: float = -1.0, limiter: bool = False, half_window: int = 32):
        """loudness() and the gain applied, measure -> gate -> gain queued back to back with the gain read on the device:
        returns (pcm_out, LoudnessResult), pcm_out int16 [n_streams, samples], a NumPy array for a NumPy input, else a
        torch tensor on the device.  The result describes the input; the output sits at target (or as close as the peak
        ceiling and the gain's range of 1/4096 .. just under 8 allow).

        A title fed in pieces needs the whole title measured before its first sample is scaled, so it takes two passes
        over the *_to calls: loudness_steps_to over every piece (first_sample and the state carried on), one
        loudness_gate_to over all its steps, then pcm_gain_to per piece with the records it left.

        limiter=True: steps -> gate -> peaks -> limit in place of steps -> gate -> gain.  One loud sample no longer caps
        the gain of the whole title: every stream gets the full loudness gain -- limit_gain(gated_mean, n_gated, target_ms,
        rate), not the result's gain_q12, which stays the capped gain of the record -- reduced smoothly within half_window
        blocks of about 1 ms (1 .. 64) around the samples that would pass `peak` dBFS.  A stream whose cap does not bind
        comes out bit for bit as without the limiter.  The limited title lands slightly under the target, by the energy
        of what was limited; no second pass measures it again.  In pieces: limit_peaks_to over every piece in the first
        pass, into a row the caller keeps, and pcm_limit_to per piece in the second (pcm_limit_to's docstring)."""
        out, res = self._measure(pcm, rate, target, peak, gain=True, limiter=limiter, half_window=half_window)
        return (out.cpu().numpy() if isinstance(pcm, np.ndarray) else out), res

    def _measure(self, pcm, rate: int, target: float, peak: float, gain: bool, limiter: bool = False, half_window: int = 32):
        """loudness() and normalize(): (the scaled PCM as a tensor [n_streams, samples] when gain, else None, the result)."""
        import torch
        device = torch.device("cuda", self.device)
        if isinstance(pcm, np.ndarray):
            pcm = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int16)).to(device)
        if len(getattr(pcm, "shape", ())) != 2 or pcm.shape[1] < 1:
            raise ValueError(f"pcm must be int16 [n_streams, samples] on {device} (or a NumPy array)")
        n, samples = int(pcm.shape[0]), int(pcm.shape[1])
        stride = _r8(samples)
        with self._scratch() as s:
            src_ptr, _, _ = self._stage(s, pcm, n, samples, stride=stride, dtype=np.int16, what="pcm")
            out = torch.empty((n, stride), dtype=torch.int16, device=device) if gain else None
            self._wait_for_torch()
            prepared = self._loudness_buffers(s, n, samples, rate, target, peak)
            d_peaks = s.alloc(_r16(2 * n * _limit_blocks(samples, rate))) if gain and limiter else None
            d_recs = self._loudness_queue(src_ptr, n, samples, stride, rate, prepared)
            if d_peaks is not None:
                self._limit_queue(d_peaks, src_ptr, d_recs, out.data_ptr(), n, samples, stride, rate, half_window, prepared[2])
            elif gain:
                self.pcm_gain_to(src_ptr, d_recs, out.data_ptr(), n_streams=n, n_samples=samples, src_stride=stride, dst_stride=stride)
            self.sync()
            res = self._loudness_result(d_recs.download(np.uint8, 32 * n).view(LOUDNESS_REC_DTYPE), rate)
        return (out[:, :samples] if gain else None), res

    # -- SBC encode (efx_sbc_encode) and A/V multiplexing (efx_mux_av) ------------------------------
    def sbc_encode_to(self, pcm: DeviceBuffer | int, state: DeviceBuffer | int, frames: DeviceBuffer | int, *, n_streams: int,
                      n_frames: int, blocks: int = 16, mode: int = 0, allocation: int = 0, bitpool: int = 28, frequency: int = 3,
                      pcm_layout: int = PCM_FRAME_PLANAR, pcm_stride: int = 0, frame_stride: int = 0) -> int:
        """efx_sbc_encode on raw device memory, asynchronous on the library's stream: stream i's int16 PCM at pcm + i x
        pcm_stride elements (0 = packed), its frames back to back from frames + i x frame_stride bytes (0 = the frames'
        size rounded up to 16), the encoders' states (sbc_enc_state_bytes() each, zeros = fresh) updated in place.  Returns
        the frame stride used."""
        ch = 2 if mode else 1
        fb = sbc_frame_bytes(blocks, ch, bitpool)
        o = _SbcEncodeOpts(n_streams, n_frames, frequency, blocks, mode, allocation, bitpool, pcm_layout,
                           pcm_stride or n_frames * blocks * 8 * ch, frame_stride or (n_frames * fb + 15) // 16 * 16)
        _check(self._ctx, self._lib.efx_sbc_encode(self._ctx, C.byref(o), _ptr(pcm), _ptr(state), _ptr(frames)))
        return o.frame_stride

    def sbc_encode(self, pcm, *, blocks: int = 16, mode: int = 0, allocation: int = 0, bitpool: int = 28, frequency: int = 3,
                   pcm_layout: int = PCM_FRAME_PLANAR, cont: bool = False):
        """Encode int16 PCM [n_streams, samples] (a NumPy array, or a torch tensor on the decoder's device) into SBC frames:
        a uint8 torch tensor [n_streams, n_frames, frame_bytes] on the device (samples must be a whole number of frames:
        blocks x 8 x channels values each).  cont=True continues the streams of the previous sbc_encode of this object (the
        analysis filter's memory is kept on the device); otherwise the encoders start afresh.  Synchronises torch's current
        stream before and the library's after."""
        import torch
        device = torch.device("cuda", self.device)
        if isinstance(pcm, np.ndarray):
            pcm = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int16)).to(device)
        if len(getattr(pcm, "shape", ())) != 2:
            raise ValueError(f"pcm must be an int16 [n_streams, samples] tensor on {device} (or a NumPy array)")
        ch = 2 if mode else 1
        n, per = pcm.shape[0], blocks * 8 * ch
        if pcm.shape[1] == 0 or pcm.shape[1] % per:
            raise ValueError(f"samples per stream must be a positive multiple of {per}")
        n_frames = pcm.shape[1] // per
        fb = sbc_frame_bytes(blocks, ch, bitpool)
        if not fb:
            raise ValueError("blocks, mode or bitpool out of range")
        st = getattr(self, "_sbc_enc_state", None)
        if not cont or st is None or st.shape[0] != n:
            if cont:
                raise EfxError(-5, "sbc_encode: cont without a previous sbc_encode of as many streams")
            st = torch.zeros((n, sbc_enc_state_bytes()), dtype=torch.uint8, device=device)
        stride = _r16(n_frames * fb)
        out = torch.empty((n, stride), dtype=torch.uint8, device=device)
        with self._scratch() as s:
            # (a whole number of frames: rows of a multiple of 32 samples, packed)
            pcm_ptr, _, _ = self._stage(s, pcm, n, pcm.shape[1], stride=pcm.shape[1], dtype=np.int16, what="pcm")
            self._wait_for_torch()
            self.sbc_encode_to(pcm_ptr, st.data_ptr(), out.data_ptr(), n_streams=n, n_frames=n_frames, blocks=blocks, mode=mode,
                               allocation=allocation, bitpool=bitpool, frequency=frequency, pcm_layout=pcm_layout,
                               pcm_stride=pcm.shape[1], frame_stride=stride)
            self.sync()
        self._sbc_enc_state = st
        return out[:, :n_frames * fb].reshape(n, n_frames, fb)

    def mux_to(self, video: DeviceBuffer | int, video_len: DeviceBuffer | int, audio: DeviceBuffer | int | None,
               dst: DeviceBuffer | int, length: DeviceBuffer | int, status: DeviceBuffer | int, *, n_streams: int, frame_bytes: int,
               n_frames: int, video_stride: int, audio_stride: int, dst_stride: int, frames_per_pes: int = 8,
               audio_pid: int = 0x101, samples_per_frame: int = 128, sample_rate: int = 48000, audio_first_pts: int = 0,
               audio_first_frame: int = 0, audio_cc: int = 0):
        """efx_mux_av on raw device memory, asynchronous on the library's stream: video / video_len are what encode_to left in
        dst / length, so encode_to -> sbc_encode_to -> mux_to needs no synchronisation in between."""
        o = _MuxOpts(n_streams, audio_pid, frame_bytes, n_frames, frames_per_pes, samples_per_frame, sample_rate, audio_first_pts,
                     audio_first_frame, audio_cc, video_stride, audio_stride, dst_stride)
        _check(self._ctx, self._lib.efx_mux_av(self._ctx, C.byref(o), _ptr(video), _ptr(video_len), _ptr(audio), _ptr(dst), _ptr(length), _ptr(status)))

    def mux(self, video_streams, frames, *, frames_per_pes: int = 8, audio_pid: int = 0x101, samples_per_frame: int = 128,
            sample_rate: int = 48000, audio_first_pts: int = 0, audio_first_frame: int = 0, audio_cc: int = 0,
            dst_stride: int = 0):
        """Multiplex video transport streams (a list of bytes / uint8 arrays, as encode(fmt=FORMAT_TS) returns them) with SBC
        frames (uint8 [n_streams, n_frames, frame_bytes]: a NumPy array or a torch tensor as sbc_encode returns it; n_frames
        may be 0).  Returns (titles: list of bytes, status: uint32 array of MUX_* bits).  Synchronises."""
        n = len(video_streams)
        arrs = [np.frombuffer(v, dtype=np.uint8) if isinstance(v, (bytes, bytearray, memoryview))
                else np.ascontiguousarray(v, dtype=np.uint8) for v in video_streams]
        if not isinstance(frames, np.ndarray):
            frames = frames.cpu().numpy()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 3 or frames.shape[0] != n:
            raise ValueError("frames must have shape (n_streams, n_frames, frame_bytes)")
        n_frames, fb = frames.shape[1], frames.shape[2]
        v_stride = _r16(max(1, max(a.size for a in arrs)))
        a_stride = _r16(max(1, n_frames * fb))
        stride = dst_stride or mux_bound(v_stride, n_frames, fb, frames_per_pes)
        with self._scratch() as s:
            host_v = np.zeros((n, v_stride), dtype=np.uint8)
            for i, a in enumerate(arrs):
                host_v[i, :a.size] = a
            v_ptr, _, _ = self._stage(s, host_v, n, v_stride)
            a_ptr, _, _ = self._stage(s, frames, n, n_frames * fb, stride=a_stride)
            d_dst, d_meta = s.alloc(n * stride), s.alloc(3 * _r16(4 * n))
            d_meta.upload(np.array([a.size for a in arrs], dtype=np.uint32))
            p_len, p_st = d_meta.ptr + _r16(4 * n), d_meta.ptr + 2 * _r16(4 * n)
            self.mux_to(v_ptr, d_meta.ptr, a_ptr, d_dst, p_len, p_st, n_streams=n, frame_bytes=fb, n_frames=n_frames,
                        video_stride=v_stride, audio_stride=a_stride, dst_stride=stride, frames_per_pes=frames_per_pes,
                        audio_pid=audio_pid, samples_per_frame=samples_per_frame, sample_rate=sample_rate,
                        audio_first_pts=audio_first_pts, audio_first_frame=audio_first_frame, audio_cc=audio_cc)
            self.sync()
            return self._download_streams(d_dst.ptr, stride, p_len, p_st, n)

    def _download_streams(self, dst_ptr: int, stride: int, len_ptr: int, status_ptr: int, n: int):
        lens, st = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        _check(self._ctx, self._lib.efx_memcpy_d2h(self._ctx, lens.ctypes.data, len_ptr, 4 * n))
        _check(self._ctx, self._lib.efx_memcpy_d2h(self._ctx, st.ctypes.data, status_ptr, 4 * n))
        out = []
        for i in range(n):
            b = np.empty(int(lens[i]), dtype=np.uint8)
            if b.size:
                _check(self._ctx, self._lib.efx_memcpy_d2h(self._ctx, b.ctypes.data, dst_ptr + i * stride, b.size))
            out.append(b.tobytes())
        return out, st

    def encode_av(self, pictures, pcm, *, qscale: int = 8, gop: int = 12, search: int = 7, first_pts: int = 0, blocks: int = 16,
                  allocation: int = 0, bitpool: int = 28, frequency: int = 3, sample_rate: int = 48000, frames_per_pes: int = 8,
                  audio_pid: int = 0x101, bitrate: int | None = None, vbv_bits: int = 250_000, qmin: int = 3, qmax: int = 31,
                  pcm_rate: int | None = None, pcm_layout: str = "interleaved", fps=None, scene_cut: int | bool | None = None,
                  min_gop: int | None = None, quality: bool = False, aq: int | bool | None = None, loudness: float | None = None,
                  peak: float = -1.0, limiter: bool = False, half_window: int = 32):
        """Pictures + PCM -> complete titles: encode (transport streams) -> sbc_encode (mono) -> mux, queued back to back on
        the library's stream with nothing synchronised in between.  pictures: (n, P, 101376) I420 as for encode(); pcm: int16
        [n, samples], a whole number of frames of blocks x 8 samples; the audio starts at the first picture's PTS.  Every
        stream starts afresh.  Returns (titles: list of bytes, status: uint32 array of ENCODE_* | MUX_* bits).

        bitrate: rate control of the video leg only, as for encode(): the rate and the buffer model cover the video PID's
        packets; the audio packets the multiplexer adds are outside the model.

        pcm_rate: the PCM is source audio at this rate, [n, frames] or [n, frames, channels] ([n, channels, frames] with
        pcm_layout="planar"): it goes through import_pcm_to (equal downmix weights) into a device buffer zero-padded to whole
        SBC frames, queued in front of sbc_encode_to with nothing synchronised in between.  The output rate is sample_rate
        (16000, 32000, 44100 or 48000) and `frequency` follows it.  The resampler's delay (16 output samples, 0.33 ms at
        48 kHz) is not compensated.

        fps: the video's picture rate as for encode() (None = 30000/1001).  The audio's PTS come from the sample count
        and do not depend on it.

        scene_cut, min_gop: I pictures at the video's scene cuts, as for encode(); encode_picture_info(n) afterwards
        gives the pictures' types.

        aq: adaptive quantisation of the video, as for encode().

        loudness: a target in LUFS (EBU R 128: -23.0).  The mono PCM that sbc_encode_to is about to read -- behind the
        import, when there is one -- is measured (loudness_steps_to, loudness_gate_to) and scaled in place (pcm_gain_to)
        to that programme loudness with its sample peak no higher than `peak` dBFS, queued in front of sbc_encode_to
        with nothing synchronised in between: the gain stays on the device.  None (the default): no launch, no
        allocation, the title's bytes are what they were without the keyword.

        limiter, half_window: with loudness=, the peak limiter (limit_peaks_to, pcm_limit_to) takes pcm_gain_to's place, as
        for normalize(limiter=True): the full loudness gain, reduced around the samples that would pass `peak` dBFS, so
        that a few loud samples do not hold the whole title under its target.  Without loudness= they do nothing.  False
        (the default): no launch and no allocation of the limiter's, the title's bytes are what they were.

        quality=True: the video's reconstruction is kept in a device buffer of the call's own and compared with the
        pictures right behind the encode, on the same stream, as for encode(); the call then returns (titles, status,
        quality), quality the CompareResult of shape (n, P), zeros for pictures that were not written."""
        import torch
        device = torch.device("cuda", self.device)
        to_dev = lambda t, dt: torch.from_numpy(np.ascontiguousarray(t)).to(device) if isinstance(t, np.ndarray) else t
        pictures, pcm = to_dev(pictures, np.uint8), to_dev(pcm, np.int16)
        imp = None
        if pcm_rate is not None:
            if pcm_layout not in _PCM_LAYOUTS or sample_rate not in _SBC_FREQUENCY or import_pcm_delay(pcm_rate, sample_rate) < 0:
                raise ValueError("pcm_layout, pcm_rate or sample_rate out of range (efx_import_pcm)")
            if pcm.dtype != torch.int16 or pcm.dim() not in (2, 3) or pcm.device != device:
                raise ValueError(f"pcm must be int16 [n, frames] or [n, frames, channels] on {device}")
            if pcm.dim() == 2:
                pcm = pcm.unsqueeze(2 if pcm_layout == "interleaved" else 1)
            in_frames, in_ch = (int(pcm.shape[1]), int(pcm.shape[2])) if pcm_layout == "interleaved" else (int(pcm.shape[2]), int(pcm.shape[1]))
            n_out = import_pcm_out_samples(pcm_rate, sample_rate, 0, in_frames)
            if in_frames < 1 or not 1 <= in_ch <= 8 or n_out < 0:
                raise ValueError("pcm: no frames, too many frames or more than 8 channels")
            frequency = _SBC_FREQUENCY[sample_rate]
            imp = (pcm, in_frames, in_ch, _r8(in_frames * in_ch))
            # the resampled stream, zero-padded to whole frames: what sbc_encode_to reads
            pcm = torch.zeros((int(pcm.shape[0]), -(-n_out // (blocks * 8)) * blocks * 8), dtype=torch.int16, device=device)
        if pictures.dtype != torch.uint8 or pictures.dim() != 3 or pictures.shape[-1] != FRAME_BYTES or pictures.device != device:
            raise ValueError(f"pictures must be uint8 (n, P, {FRAME_BYTES}) on {device}")
        n, P = int(pictures.shape[0]), int(pictures.shape[1])
        if pcm.dtype != torch.int16 or pcm.dim() != 2 or pcm.shape[0] != n or pcm.device != device or pcm.shape[1] % (blocks * 8):
            raise ValueError("pcm must be int16 [n, samples], samples a multiple of blocks x 8")
        samples = int(pcm.shape[1])
        n_frames = samples // (blocks * 8)
        fb = sbc_frame_bytes(blocks, 1, bitpool)
        v_stride = encode_bound(FORMAT_TS, P)
        a_stride = _r16(max(1, n_frames * fb))
        stride = mux_bound(v_stride, n_frames, fb, frames_per_pes)
        with self._scratch() as s:
            d_v, d_a, d_dst = s.alloc(n * v_stride), s.alloc(n * a_stride), s.alloc(n * stride)
            d_meta, d_state = s.alloc(4 * _r16(4 * n)), s.zeros(n * sbc_enc_state_bytes())
            if imp is not None:
                d_istate = s.zeros(n * import_pcm_state_bytes())
            p_vlen, p_vst, p_len, p_st = (d_meta.ptr + k * _r16(4 * n) for k in range(4))
            d_rec = d_qual = None
            if quality and n * P:
                d_rec, d_qual = s.alloc(n * P * FRAME_BYTES), s.alloc(48 * n * P)
            loud = None
            if loudness is not None and n_frames:
                # (buffers and the zeroed state now: an upload waits for what is queued on the library's stream)
                loud_rate = {v: k for k, v in _SBC_FREQUENCY.items()}[frequency]
                loud = self._loudness_buffers(s, n, samples, loud_rate, loudness, peak)
                d_lpeaks = s.alloc(_r16(2 * n * _limit_blocks(samples, loud_rate))) if limiter else None
                if imp is None:
                    pcm = pcm.clone()  # (scaled in place: the caller's tensor stays as it is)
            pic_ptr, _, _ = self._stage(s, pictures, n * P, FRAME_BYTES, what="pictures")
            pcm_ptr, _, _ = self._stage(s, pcm, n, samples, stride=samples, dtype=np.int16, what="pcm")  # (whole frames: packed)
            if imp is not None:
                imp_ptr, _, _ = self._stage(s, imp[0], n, imp[1] * imp[2], stride=imp[3], dtype=np.int16, what="pcm")
            self._wait_for_torch()
            self.encode_to(pic_ptr, d_v, p_vlen, p_vst, n_streams=n, n_pictures=P, qscale=qscale, gop=gop, search=search,
                           fmt=FORMAT_TS, first_pts=first_pts, dst_stride=v_stride, bitrate=bitrate, vbv_bits=vbv_bits, qmin=qmin,
                           qmax=qmax, fps=fps, scene_cut=scene_cut, min_gop=min_gop, recon=d_rec, aq=aq)
            if d_qual is not None:
                self.compare_to(pic_ptr, d_rec, d_qual, n_images=n * P, ref_max=248)
            if imp is not None:
                self.import_pcm_to(imp_ptr, d_istate, pcm_ptr, n_streams=n, n_in=imp[1], in_rate=pcm_rate,
                                   out_rate=sample_rate, channels=imp[2], layout=_PCM_LAYOUTS[pcm_layout], src_stride=imp[3],
                                   dst_stride=samples)
            if loud is not None:
                d_lrecs = self._loudness_queue(pcm_ptr, n, samples, samples, loud_rate, loud)
                if d_lpeaks is not None:
                    self._limit_queue(d_lpeaks, pcm_ptr, d_lrecs, pcm_ptr, n, samples, samples, loud_rate, half_window, loud[2])
                else:
                    self.pcm_gain_to(pcm_ptr, d_lrecs, pcm_ptr, n_streams=n, n_samples=samples, src_stride=samples, dst_stride=samples)
            if n_frames:
                self.sbc_encode_to(pcm_ptr, d_state, d_a, n_streams=n, n_frames=n_frames, blocks=blocks, mode=0,
                                   allocation=allocation, bitpool=bitpool, frequency=frequency, pcm_stride=samples,
                                   frame_stride=a_stride)
            self.mux_to(d_v, p_vlen, d_a, d_dst, p_len, p_st, n_streams=n, frame_bytes=fb, n_frames=n_frames, video_stride=v_stride,
                        audio_stride=a_stride, dst_stride=stride, frames_per_pes=frames_per_pes, audio_pid=audio_pid,
                        samples_per_frame=blocks * 8, sample_rate=sample_rate, audio_first_pts=first_pts)
            self.sync()
            titles, st = self._download_streams(d_dst.ptr, stride, p_len, p_st, n)
            vst = np.empty(n, dtype=np.uint32)
            _check(self._ctx, self._lib.efx_memcpy_d2h(self._ctx, vst.ctypes.data, p_vst, 4 * n))
            if quality:
                types = np.ascontiguousarray(self.encode_picture_info(n)["type"]) if n * P else np.zeros((n, P), dtype=np.uint8)
                qual = self._encode_quality(d_qual, n, P, types) if d_qual is not None else _compare_result(np.zeros((0, 6), np.uint64), (n, P))
                return titles, st | vst, qual
            return titles, st | vst

    # -- picture rates (efx_conform_rate) ----------------------------------------------------------------
    def conform_to(self, src: DeviceBuffer | int, dst: DeviceBuffer | int, *, n_streams: int, n_pictures: int, fps_in, fps_out,
                   first_picture: int = 0, src_stride: int = 0, dst_stride: int = 0) -> int:
        """efx_conform_rate on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: the
        source pictures first_picture .. first_picture + n_pictures - 1 of a title at fps_in (any constant rate: Fraction,
        "num/den", int or float), stream i's at src + i * src_stride (0 = packed), become the output pictures at fps_out
        (a coded rate) that show them, by dropping and repeating pictures (the rule: include/efx.h), stream i's at dst + i *
        dst_stride (0 = packed: the call's outputs).  Returns the call's outputs (conform_count)."""
        f, code = _rate(fps_in), _fps_code(fps_out)
        n_out = conform_count(f, fps_out, first_picture, n_pictures)
        if n_out < 0:
            raise ValueError(f"conform {f} -> {PICTURE_RATES[code]}: the rates, first_picture={first_picture} or "
                             f"n_pictures={n_pictures} are out of range (efx_conform_rate)")
        o = _ConformOpts(n_streams, n_pictures, f.numerator, f.denominator, code, first_picture,
                         src_stride or n_pictures * FRAME_BYTES, dst_stride or n_out * FRAME_BYTES)
        _check(self._ctx, self._lib.efx_conform_rate(self._ctx, C.byref(o), _ptr(src), _ptr(dst)))
        return n_out

    def conform(self, pictures, fps_in, fps_out, *, first_picture: int = 0):
        """(n, P, 101376) I420 pictures at fps_in as (n, P', 101376) pictures at fps_out, a rate MPEG-1 codes, conformed on
        the device (conform_to): a uint8 tensor on the decoder's device (a tensor is returned) or a NumPy array (an array
        is returned).  P' = conform_count(fps_in, fps_out, first_picture, P), which may be 0.  Synchronises: torch's
        current stream before (tensor input), the library's after."""
        if len(pictures.shape) != 3 or pictures.shape[-1] != FRAME_BYTES or pictures.shape[0] < 1 or pictures.shape[1] < 1:
            raise ValueError(f"pictures must have shape (n, P, {FRAME_BYTES}), got {tuple(pictures.shape)}")
        n, P = int(pictures.shape[0]), int(pictures.shape[1])
        n_out = conform_count(fps_in, fps_out, first_picture, P)
        if n_out < 0:
            raise ValueError(f"conform {fps_in!r} -> {fps_out!r}: out of range (efx_conform_rate)")
        with self._scratch() as s:
            src_ptr, is_array, _ = self._stage(s, pictures, n * P, FRAME_BYTES, what="pictures")
            if not is_array:
                self._wait_for_torch()
            dst_ptr, fetch = self._rows_out(s, is_array, n, n_out * FRAME_BYTES, n_out * FRAME_BYTES)
            if n_out:  # (no output pictures: nothing to queue, and an empty tensor has no address)
                self.conform_to(src_ptr, dst_ptr, n_streams=n, n_pictures=P, fps_in=fps_in, fps_out=fps_out, first_picture=first_picture)
            self.sync()
            return fetch().reshape(n, n_out, FRAME_BYTES)

    def make_poster(self, image, *, qscale: int = 2, fps=24, **import_kw) -> bytes:
        """poster.ts of a title, which the reference's player opens for every title it browses (src/espflix.cpp:1060-1068)
        and its indexer makes with `-filter:v fps=fps=24 -q 2` (indexer/indexer.cpp:306): the image -- one picture as
        import_pictures takes it, (H, W, 3), (3, H, W) or with a leading axis of 1 -- imported (import_kw: fmt, fit, crop,
        matrix, src_range ...), then one I picture at qscale and fps as a transport stream."""
        if len(image.shape) == 3:
            image = image[None]
        if image.shape[0] != 1:
            raise ValueError("make_poster takes one image")
        pic = self.import_pictures(image, **import_kw)
        res = self.encode(pic.reshape(1, 1, FRAME_BYTES), qscale=qscale, gop=1, fmt=FORMAT_TS, fps=fps)
        if int(res.status[0]):
            raise EfxError(-5, f"make_poster: the encoder's status is {int(res.status[0]):#x}")
        return res.streams[0]

    # -- fast-forward and rewind streams (efx_trick_pick) --------------------------------------------
    def trick_pick_to(self, src: DeviceBuffer | int | None, fwd: DeviceBuffer | int | None, rwd: DeviceBuffer | int | None, *,
                      n_streams: int, n_pictures: int, speed: int = 15, first_picture: int = 0, total_pictures: int = 0,
                      source: int = TRICK_FROM_I420, first_stream: int = 0, src_stride: int = 0, fwd_stride: int = 0,
                      rwd_stride: int = 0) -> int:
        """efx_trick_pick on raw device memory (DeviceBuffers or pointers), asynchronous on the library's stream: of the
        pictures first_picture .. first_picture + n_pictures - 1 of a title, every one whose title index is a multiple of
        speed goes, as a 101376-byte I420 image, to fwd (may be None) in playing order from image 0 of the call, and to rwd
        (may be None) at image K - 1 - k of the title's K = ceil(total_pictures / speed) picks (the rule: include/efx.h).
        source TRICK_FROM_I420: stream i's pictures at src + i * src_stride (0 = packed); TRICK_FROM_RING: src is None,
        picture j is picture j of the most recent decode of stream first_stream + i.  fwd_stride / rwd_stride 0 = packed
        (the call's picks / K images).  Returns the call's picks (trick_count)."""
        picks = trick_count(first_picture, n_pictures, speed)
        K = trick_count(0, max(0, total_pictures), speed)
        o = _TrickOpts(n_streams, n_pictures, speed, source, first_stream, first_picture, total_pictures,
                       src_stride or max(0, n_pictures) * FRAME_BYTES, fwd_stride or max(0, picks) * FRAME_BYTES,
                       rwd_stride or max(0, K) * FRAME_BYTES)
        _check(self._ctx, self._lib.efx_trick_pick(self._ctx, C.byref(o), _ptr(src), _ptr(fwd), _ptr(rwd)))
        return picks

    def trick_streams(self, pictures=None, *, title=None, speed: int = 15, gop: int = 3, qscale: int = 8, search: int = 7,
                      bitrate: int | None = None, vbv_bits: int = 250_000, qmin: int = 3, qmax: int = 31, first_pts: int = 0,
                      piece: int | None = None, fps=None, aq: int | bool | None = None):
        """The fast-forward and the rewind stream of n titles (the reference indexer's `-g 3 ... setpts=PTS/15` and
        `-vf reverse` runs, indexer/indexer.cpp:308-309): every speed-th picture of a title, encoded in playing order and in
        reverse order as transport streams with GOPs of `gop` pictures.  Returns (fwd: list of bytes, rwd: list of bytes,
        status: uint32 [2, n] of ENCODE_* bits, row 0 fwd, row 1 rwd).

        pictures: (n, P, 101376) I420 as for encode() (a uint8 tensor on the decoder's device or a NumPy array): the picks
        are taken from them in pieces of `piece` pictures (None: all at once).
        title: instead, a list of n transport streams (as encode_av / encode return them): they are uploaded once and
        decoded in pieces of `piece` pictures (None, and at most: min(max_pictures, ring_depth - 1)), and after each piece
        the picks are taken straight from the frame rings.  The titles must hold the same number of pictures (ValueError)
        and decode with status 0 (EfxError); the decoder's state is that of the title's last piece afterwards.  The rewind
        placement needs the picture count before the first pick: it is taken on the host, from each title's demultiplexed
        elementary stream (es(): one device-to-host copy of every title's video bytes, scanned for picture start codes),
        because the decoder's own count covers one call's pictures only.

        Either way each piece's picks are encoded as they come, continuing the fast-forward stream (encode_to, cont), with
        nothing synchronised between the pick and the encode of a piece; the rewind stream is encoded after the last piece
        (the encoder keeps one set of streams per context, and a reversed stream cannot start before the title has ended).
        Both streams start at first_pts; trick picture k carries first_pts + picture_pts_offset(fps, k) (fps as for
        encode(): None = 30000/1001, first_pts + 3003 k).  qscale, search, bitrate ... qmax and aq as for encode().  Synchronises: torch's current stream before (tensor input), the library's after."""
        if (pictures is None) == (title is None):
            raise ValueError("give pictures or title=, not both")
        if not 1 <= speed <= 255:
            raise ValueError("speed must be 1 .. 255")
        _fps_code(fps)
        with self._scratch() as s:
            if pictures is not None:
                if len(pictures.shape) != 3 or pictures.shape[-1] != FRAME_BYTES or pictures.shape[1] < 1 or pictures.shape[0] < 1:
                    raise ValueError(f"pictures must have shape (n, P, {FRAME_BYTES}), got {tuple(pictures.shape)}")
                n, P = int(pictures.shape[0]), int(pictures.shape[1])
                src_ptr, is_array, _ = self._stage(s, pictures, n * P, FRAME_BYTES, what="pictures")
                if not is_array:
                    self._wait_for_torch()
                step = P if piece is None else piece
                if step < 1:
                    raise ValueError("piece must be >= 1")
            else:
                n = len(title)
                self.upload(title, FORMAT_TS)
                counts = [_count_pictures(self.es(i)) for i in range(n)]
                P = counts[0]
                if P < 1 or any(c != P for c in counts):
                    raise ValueError(f"the titles of a batch must hold the same number of pictures (at least 1), got {counts}")
                limit = min(self.max_pictures, self.ring_depth - 1)
                step = limit if piece is None else piece
                if not 1 <= step <= limit:
                    raise ValueError(f"piece must be 1 .. min(max_pictures, ring_depth - 1) = {limit}")
            K = trick_count(0, P, speed)
            pieces = [(first, min(step, P - first)) for first in range(0, P, step)]
            picks = [trick_count(first, cnt, speed) for first, cnt in pieces]
            fwd_cap = max(picks)
            d_fwd, d_rwd = s.alloc(n * fwd_cap * FRAME_BYTES), s.alloc(n * K * FRAME_BYTES)
            # every encode call (at most 255 pictures) writes a region of its own; the bytes are put together at the end
            split = lambda c: [(a, min(255, c - a)) for a in range(0, c, 255)]
            calls = [[sub for c in picks for sub in split(c)], split(K)]
            total = sum(n * encode_bound(FORMAT_TS, c) for side in calls for _, c in side)
            d_dst, d_meta = s.alloc(total), s.alloc(2 * _r16(4 * n) * sum(len(side) for side in calls))
            done = []  # (side, offset of the region in d_dst, its stride, offset of the byte counts in d_meta)
            state = {"dst": 0, "meta": 0}

            def encode_call(side, src, src_stride, count, cont):
                stride = self.encode_to(src, d_dst.ptr + state["dst"], d_meta.ptr + state["meta"],
                                        d_meta.ptr + state["meta"] + _r16(4 * n), n_streams=n, n_pictures=count, qscale=qscale,
                                        gop=gop, search=search, fmt=FORMAT_TS, cont=cont, first_pts=first_pts,
                                        src_stride=src_stride, bitrate=bitrate, vbv_bits=vbv_bits, qmin=qmin, qmax=qmax,
                                        fps=fps, aq=aq)
                done.append((side, state["dst"], stride, state["meta"]))
                state["dst"] += n * stride
                state["meta"] += 2 * _r16(4 * n)

            started = False
            for (first, cnt), c in zip(pieces, picks):
                if title is not None:
                    self.decode(sync=False, first_picture=first, n_pictures=cnt)
                    self.trick_pick_to(None, d_fwd, d_rwd, n_streams=n, n_pictures=cnt, speed=speed, first_picture=first,
                                       total_pictures=P, source=TRICK_FROM_RING, fwd_stride=fwd_cap * FRAME_BYTES)
                else:
                    self.trick_pick_to(src_ptr + first * FRAME_BYTES, d_fwd, d_rwd, n_streams=n, n_pictures=cnt, speed=speed,
                                       first_picture=first, total_pictures=P, src_stride=P * FRAME_BYTES,
                                       fwd_stride=fwd_cap * FRAME_BYTES)
                for a, sub in split(c):
                    encode_call(0, d_fwd.ptr + a * FRAME_BYTES, fwd_cap * FRAME_BYTES, sub, started)
                    started = True
                if title is not None:
                    for i in range(n):  # (synchronises: behind the piece's encode)
                        bits = self.stream_status(i) & ~STREAM_TRUNCATED
                        if bits or self.picture_count(i) != cnt:
                            raise EfxError(-5, f"trick_streams: title {i} decodes with status {bits:#x}, {self.picture_count(i)} of "
                                               f"{cnt} pictures from picture {first}")
            for a, sub in split(K):
                encode_call(1, d_rwd.ptr + a * FRAME_BYTES, K * FRAME_BYTES, sub, a > 0)
            self.sync()
            out, status = ([b""] * n, [b""] * n), np.zeros((2, n), dtype=np.uint32)
            for side, off, stride, meta in done:
                part, st = self._download_streams(d_dst.ptr + off, stride, d_meta.ptr + meta, d_meta.ptr + meta + _r16(4 * n), n)
                out[side][:] = [x + y for x, y in zip(out[side], part)]
                status[side] |= st
            return out[0], out[1], status

    def make_title(self, pictures, pcm, *, speed: int = 15, trick_gop: int = 3, fps=None, fps_out=None, poster=None, aq: int | bool | None = None,
                   overlays=None, **encode_av):
        """A complete title directory per stream, as the reference's indexer leaves it (indexer/indexer.cpp:292-321) and its
        player opens it (src/espflix.cpp:647,787-792): returns (list of n dicts {"video.ts", "video_fwd.ts", "video_rwd.ts",
        "video.idx"} of bytes, status: uint32 [3, n], rows video.ts (ENCODE_* | MUX_* bits), video_fwd.ts, video_rwd.ts).

        video.ts is encode_av(pictures, pcm, **encode_av).  The trick streams are trick_streams(pictures, speed=speed,
        gop=trick_gop) with the same qscale, search, first_pts, aq and rate-control keywords, without audio.  They are made
        from the SOURCE pictures, one generation better than the reference, whose ffmpeg runs recode the finished
        video.ts.  video.idx is idx_build over index_streams([main, fwd, rwd], trick_speed=[1, speed, speed]), one call per
        title -- max_stream_bytes must hold the three streams of a title -- or, on a context with max_streams below 3, one
        call per stream (the same records: a stream's record does not depend on the others).

        fps: the pictures' rate (None = 30000/1001).  A rate MPEG-1 codes is encoded as it is: video.ts and both trick
        streams carry its code, and trick picture k is at first_pts + picture_pts_offset(fps, k).  Any other rate needs
        fps_out, a coded rate (ValueError otherwise: nothing is guessed): the pictures are conformed on the device
        (conform) before encode_av and trick_streams see them.  The PCM is not touched: the audio's PTS come from its
        sample count.  poster: an image as make_poster takes it; the dictionaries then hold "poster.ts" as well.

        scene_cut=, min_gop= (among **encode_av) apply to video.ts only: the trick streams keep their GOPs of trick_gop.
        aq: adaptive quantisation as for encode(), of video.ts and of both trick streams.

        loudness=, peak=, limiter=, half_window= (among **encode_av): video.ts's sound levelled to a target in LUFS, with
        the peak limiter if asked, as for encode_av().

        overlays: a list of Overlay (subtitles, a logo) burnt into the pictures once, on the device (overlay()), after
        any conform: Overlay.first / .last are indices of the CODED timeline, picture 0 being the first coded picture
        (overlay_span(fps_out or fps, start, end) gives them for times).  The burnt pictures feed both encode_av and
        trick_streams, so the trick streams show the text too; the caller's pictures are not changed.  Without overlays
        the bytes, launches and allocations are what they were."""
        conformed = False
        if fps is not None and fps_out is None and not picture_rate_code(fps):
            raise ValueError(f"fps={fps!r} is not a rate MPEG-1 codes; give fps_out=, one of "
                             f"{', '.join(str(r) for r in PICTURE_RATES.values())}")
        if fps_out is not None:
            _fps_code(fps_out)
            if fps is None:
                raise ValueError("fps_out= needs fps=, the rate of the pictures")
            if _rate(fps) != _rate(fps_out):
                if isinstance(pictures, np.ndarray):
                    import torch
                    pictures = torch.from_numpy(np.ascontiguousarray(pictures)).to(torch.device("cuda", self.device))
                pictures = self.conform(pictures, fps, fps_out)
                conformed = True
            fps = fps_out
        if overlays is not None and len(overlays):
            pictures = self.overlay(pictures, overlays, inplace=conformed)  # (conform's result is this call's own)
        titles, st = self.encode_av(pictures, pcm, fps=fps, aq=aq, **encode_av)
        keys = ("qscale", "search", "first_pts", "bitrate", "vbv_bits", "qmin", "qmax")
        fwd, rwd, tst = self.trick_streams(pictures, speed=speed, gop=trick_gop, fps=fps, aq=aq,
                                           **{k: encode_av[k] for k in keys if k in encode_av})
        poster_ts = None if poster is None else self.make_poster(poster)
        out = []
        for main, f, r in zip(titles, fwd, rwd):
            three, speeds = [main, f, r], [1, speed, speed]
            if self.max_streams >= 3:
                res = self.index_streams(three, trick_speed=speeds)
            else:  # (efx_index_streams takes at most max_streams streams: a stream's record does not depend on the others)
                res = [self.index_streams([s], trick_speed=[sp])[0] for s, sp in zip(three, speeds)]
            out.append({"video.ts": main, "video_fwd.ts": f, "video_rwd.ts": r,
                        "video.idx": idx_build([rec for rec, _ in res], [smp for _, smp in res])})
            if poster_ts is not None:
                out[-1]["poster.ts"] = poster_ts
        return out, np.vstack([st[None], tst])

    def pdm(self, n_streams: int, pcm: DeviceBuffer | int, n_samples: int, state: DeviceBuffer | int,
            dst: DeviceBuffer | int):
        _check(self._ctx, self._lib.efx_pdm(self._ctx, n_streams, _ptr(pcm), n_samples, _ptr(state), _ptr(dst)))

    # -- measurement ----------------------------------------------------------------------
    def set_timing(self, enable: bool):
        _check(self._ctx, self._lib.efx_set_timing(self._ctx, 1 if enable else 0))

    def timing(self) -> Timing:
        t = _Timing()
        _check(self._ctx, self._lib.efx_get_timing(self._ctx, C.byref(t)))
        return Timing(t.index_ms, t.parse_ms, t.recon_ms, t.total_ms, t.pictures, t.slices, t.coefficients, t.es_bytes,
                      t.demux_ms, t.ts_bytes, t.timed_calls, max(1, t.groups), max(1, t.parse_halves), t.mixed, t.recon_launches)


def partition_first(total: int, parts: int, part: int) -> int:
    """First stream of part `part` when `total` streams are dealt to `parts` devices (efx_partition_first): stream k lives on
    device floor(k * parts / total).  Host-only."""
    return load_library().efx_partition_first(total, parts, part)


def numa_node_of_pci(bus_id: str) -> int:
    """NUMA node sysfs publishes for a PCI device (efx_numa_node_of_pci; -1: unknown).  Host-only."""
    return load_library().efx_numa_node_of_pci(bus_id.encode())


def numa_cpus_of_node(node: int):
    buf = (C.c_int * 4096)()
    n = load_library().efx_numa_cpus_of_node(node, buf, 4096)
    return [buf[i] for i in range(min(n, 4096))]


def numa_bind_thread(node: int) -> int:
    """Bind the calling thread to the CPUs of `node` that it may already use; returns how many (0: mask left alone)."""
    return load_library().efx_numa_bind_thread(node)


class MultiDecoder:
    """efx_multi: one context and one host thread per device of a node, streams dealt in contiguous blocks (no collective
    on the data path).  max_streams is the per-device capacity."""

    def __init__(self, devices, max_streams: int, max_pictures: int, ring_depth: int = 2, max_stream_bytes: int = 0):
        self._lib = load_library()
        self._m = _P()
        cfg = _Config(0, max_streams, max_pictures, ring_depth, max_stream_bytes, None)
        devs = (C.c_int * len(devices))(*devices)
        st = self._lib.efx_multi_create(C.byref(cfg), devs, len(devices), C.byref(self._m))
        if st != 0:
            raise EfxError(st, self._lib.efx_status_string(st).decode())
        self.ring_depth, self.n_streams = max(2, ring_depth), 0

    def _check(self, st):
        if st != 0:
            raise EfxError(st, (self._lib.efx_multi_last_error(self._m) or b"").decode() or self._lib.efx_status_string(st).decode())

    def upload(self, streams, fmt: int = FORMAT_ES):
        arrs = [np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
        n = len(arrs)
        ptrs = (_P * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        self._check(self._lib.efx_multi_upload_streams(self._m, n, ptrs, lens, fmt))
        self.n_streams = n

    def decode(self, sync: bool = True):
        self._check(self._lib.efx_multi_decode(self._m))
        if sync:
            self.sync()

    def sync(self):
        self._check(self._lib.efx_multi_sync(self._m))

    def locate(self, stream: int):
        d, l = C.c_int(), C.c_int()
        self._check(self._lib.efx_multi_locate(self._m, stream, C.byref(d), C.byref(l)))
        return d.value, l.value

    def results(self):
        n = (C.c_int * self.n_streams)()
        st = (C.c_uint32 * self.n_streams)()
        self._check(self._lib.efx_multi_results(self._m, n, st))
        return np.array(n[:]), np.array(st[:])

    def frame_hashes(self) -> np.ndarray:
        out = np.empty((self.n_streams, self.ring_depth), dtype=np.uint64)
        self._check(self._lib.efx_multi_frame_hashes(self._m, out.ctypes.data))
        return out

    def close(self):
        if self._m:
            self._lib.efx_multi_destroy(self._m)
            self._m = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
