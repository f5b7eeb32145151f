"""The C-ABI of include/efx.h as ctypes and NumPy see it: one ctypes.Structure per struct, the record dtypes of the
structs that arrive in arrays, and every entry point's signature.  espflix_amd re-exports all of it under these names.
tests/test_abi_layout.py builds a C program over efx.h and holds every size and field offset here against it."""
import ctypes as C

import numpy as np


class _Config(C.Structure):
    _fields_ = [
        ("device", C.c_int),
        ("max_streams", C.c_int),
        ("max_pictures", C.c_int),
        ("ring_depth", C.c_int),
        ("max_stream_bytes", C.c_size_t),
        ("hip_stream", C.c_void_p),
    ]


class _VideoParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("line_width", "line_count", "hsync", "hsync_long", "hsync_short",
                                       "burst_start", "burst_width", "active_start")]


class _FieldOpts(C.Structure):
    _fields_ = [("first_stream", C.c_int), ("n_streams", C.c_int), ("slot", C.c_int), ("other_slot", C.c_int),
                ("ntsc", C.c_int), ("frame_counter", C.c_int), ("hscroll", C.c_int), ("overlay", C.c_void_p),
                ("overlay_stride", C.c_size_t), ("overlay_blend", C.c_int), ("overlay_progress", C.c_int)]


class _ExportOpts(C.Structure):
    _fields_ = [("first_stream", C.c_int), ("n_streams", C.c_int), ("slot", C.c_int), ("picture", C.c_int), ("format", C.c_int),
                ("chroma", C.c_int), ("full_range", C.c_int), ("dst_stride", C.c_size_t)]


class _ImportOpts(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_images", "format", "width", "height", "crop_x", "crop_y", "crop_w", "crop_h",
                                       "dst_x", "dst_y", "dst_w", "dst_h", "full_range")] + \
               [("src_stride", C.c_size_t), ("dst_stride", C.c_size_t)]


class _CropOpts(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_streams", "images_per_stream", "format", "width", "height", "full_range", "limit",
                                       "round")] + \
               [("src_stride", C.c_size_t), ("sums_stride", C.c_size_t)]


class _Surface(C.Structure):
    """efx_surface: one 4:2:0 YCbCr image in device memory by plane offsets and pitches (surface_layout() makes one)."""
    _fields_ = [(n, C.c_int) for n in ("layout", "shift", "swap_uv", "width", "height")] + \
               [("offset", C.c_size_t * 3), ("pitch", C.c_size_t * 3), ("bytes", C.c_size_t)]


class _DeintOpts(C.Structure):
    """efx_deint_opts: one efx_deinterlace call."""
    _fields_ = [(n, C.c_int) for n in ("n_streams", "n_frames", "first_field", "mode", "lead", "tail")] + \
               [("src_stride", C.c_size_t), ("dst_stride", C.c_size_t)]


class _DetelecineOpts(C.Structure):
    """efx_detelecine_opts: one efx_detelecine call."""
    _fields_ = [(n, C.c_int) for n in ("n_streams", "n_frames", "first_field", "lead", "nt")] + \
               [("src_stride", C.c_size_t), ("dst_stride", C.c_size_t)]


class _ImportColour(C.Structure):
    """efx_import_colour: the source's H.273 matrix_coefficients code and its range (1 = full)."""
    _fields_ = [("matrix", C.c_int), ("full_range", C.c_int)]


class _ImportHdr(C.Structure):
    """efx_import_hdr: the source's H.273 transfer, primaries and matrix codes, its range (1 = full) and its peak in nits."""
    _fields_ = [(n, C.c_int) for n in ("transfer", "primaries", "matrix", "full_range", "peak_nits")]


class _CompareOpts(C.Structure):
    _fields_ = [("n_images", C.c_int), ("ref_max", C.c_int), ("ref_stride", C.c_size_t), ("test_stride", C.c_size_t),
                ("mb_stride", C.c_size_t)]


class _CompareRec(C.Structure):
    _fields_ = [("sse", C.c_uint64 * 3), ("ssim", C.c_int64 * 3)]


class _TrickOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_pictures", C.c_int), ("speed", C.c_int), ("source", C.c_int), ("first_stream", C.c_int),
                ("first_picture", C.c_int64), ("total_pictures", C.c_int64), ("src_stride", C.c_size_t),
                ("fwd_stride", C.c_size_t), ("rwd_stride", C.c_size_t)]


class _ConformOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_pictures", C.c_int), ("in_num", C.c_int32), ("in_den", C.c_int32), ("out_code", C.c_int),
                ("first_picture", C.c_int64), ("src_stride", C.c_size_t), ("dst_stride", C.c_size_t)]


class _EncodeOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_pictures", C.c_int), ("format", C.c_int), ("qscale", C.c_int), ("gop", C.c_int),
                ("search", C.c_int), ("cont", C.c_int), ("first_pts", C.c_int64), ("src_stride", C.c_size_t),
                ("dst_stride", C.c_size_t)]


class _EncodeRate(C.Structure):
    _fields_ = [("bitrate", C.c_int), ("vbv_bits", C.c_int), ("qmin", C.c_int), ("qmax", C.c_int)]


class _SceneCut(C.Structure):
    _fields_ = [("threshold", C.c_int), ("min_gop", C.c_int)]


class _AdaptiveQuant(C.Structure):
    _fields_ = [("strength", C.c_int)]


class _EncPictureInfo(C.Structure):
    _fields_ = [("cut_i", C.c_uint32), ("cut_p", C.c_uint32), ("type", C.c_uint8), ("pad", C.c_uint8 * 3)]


class _SbcEncodeOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_frames", C.c_int), ("frequency", C.c_int), ("blocks", C.c_int), ("mode", C.c_int),
                ("allocation", C.c_int), ("bitpool", C.c_int), ("pcm_layout", C.c_int), ("pcm_stride", C.c_size_t),
                ("frame_stride", C.c_size_t)]


class _ImportPcmOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_in", C.c_int), ("in_rate", C.c_int), ("out_rate", C.c_int), ("channels", C.c_int),
                ("layout", C.c_int), ("mix_q15", C.c_int * 8), ("first_in", C.c_int64), ("src_stride", C.c_size_t),
                ("dst_stride", C.c_size_t)]


class _LoudnessStepsOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_samples", C.c_int), ("rate", C.c_int), ("first_step", C.c_int),
                ("first_sample", C.c_int64), ("pcm_stride", C.c_size_t), ("steps_stride", C.c_size_t)]


class _LoudnessGateOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_steps", C.c_int), ("rate", C.c_int), ("abs_thr", C.c_uint64),
                ("target_ms", C.c_uint64), ("ceiling", C.c_uint32), ("steps_stride", C.c_size_t)]


class _PcmGainOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("n_samples", C.c_int), ("fixed_gain_q12", C.c_int), ("src_stride", C.c_size_t),
                ("dst_stride", C.c_size_t)]


class _MuxOpts(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("audio_pid", C.c_int), ("frame_bytes", C.c_int), ("n_frames", C.c_int),
                ("frames_per_pes", C.c_int), ("samples_per_frame", C.c_int), ("sample_rate", C.c_int),
                ("audio_first_pts", C.c_int64), ("audio_first_frame", C.c_int64), ("audio_cc", C.c_int),
                ("video_stride", C.c_size_t), ("audio_stride", C.c_size_t), ("dst_stride", C.c_size_t)]


class _IdxRec(C.Structure):
    _fields_ = [("first_pts", C.c_int64), ("last_pts", C.c_int64), ("bin_size", C.c_uint32), ("trick_speed", C.c_uint32),
                ("sample_count", C.c_uint32), ("reserved", C.c_uint32)]


class _Timing(C.Structure):
    _fields_ = [("index_ms", C.c_float), ("parse_ms", C.c_float), ("recon_ms", C.c_float), ("total_ms", C.c_float),
                ("pictures", C.c_uint64), ("slices", C.c_uint64), ("coefficients", C.c_uint64), ("es_bytes", C.c_uint64),
                ("demux_ms", C.c_float), ("timed_calls", C.c_uint32), ("ts_bytes", C.c_uint64), ("groups", C.c_uint32),
                ("parse_halves", C.c_uint16), ("mixed", C.c_uint16), ("recon_launches", C.c_uint32)]


# efx_loudness_step and efx_loudness_rec as NumPy sees them
LOUDNESS_STEP_DTYPE = np.dtype([("energy", "<u8"), ("peak", "<u4"), ("zero", "<u4")])
LOUDNESS_REC_DTYPE = np.dtype([("gated_mean", "<u8"), ("max_block", "<u8"), ("n_gated", "<u4"), ("n_blocks", "<u4"),
                               ("n_abs", "<u4"), ("peak", "<u2"), ("gain_q12", "<u2")])
# efx_telecine_info: the record efx_detelecine writes per processed frame
TELECINE_INFO = np.dtype([("comb_c", "<u8"), ("comb_p", "<u8"), ("diff", "<u8"), ("match", "<i4"), ("out", "<i4")])
# efx_enc_picture_info: the record efx_encode_picture_info gives per picture
ENC_PICTURE_INFO_DTYPE = np.dtype([("cut_i", "<u4"), ("cut_p", "<u4"), ("type", "u1"), ("pad", "u1", 3)])
# efx_denoise_opts: the options of one efx_denoise call, passed by the address of a one-element record array (fixed-width
# fields only, so the record is the struct)
DENOISE_OPTS_DTYPE = np.dtype([("n_streams", "<i4"), ("n_frames", "<i4"), ("luma_spatial", "<i4"), ("chroma_spatial", "<i4"),
                               ("luma_temporal", "<i4"), ("chroma_temporal", "<i4"), ("src_stride", "<u8"), ("dst_stride", "<u8"),
                               ("prev_stride", "<u8")])
# efx_scan_opts (passed like efx_denoise_opts), efx_scan_frame (one per processed frame) and efx_scan_rec (one per stream)
SCAN_OPTS_DTYPE = np.dtype([("n_streams", "<i4"), ("n_frames", "<i4"), ("lead", "<i4"), ("accumulate", "<i4"), ("nt", "<i4"),
                            ("still", "<i4"), ("prog", "<i4"), ("intl", "<i4"), ("rep", "<i4"), ("reserved", "<i4"),
                            ("first_frame", "<u8"), ("src_stride", "<u8")])
SCAN_FRAME_DTYPE = np.dtype([("comb", "<u8"), ("comb_tb", "<u8"), ("comb_bt", "<u8"), ("diff_top", "<u8"), ("diff_bottom", "<u8"),
                             ("label", "<i4"), ("repeat", "<i4")])
SCAN_REC_DTYPE = np.dtype([("n_still", "<u4"), ("n_prog", "<u4"), ("n_tff", "<u4"), ("n_bff", "<u4"), ("n_undet", "<u4"),
                           ("rep_top", "<u4", 5), ("rep_bottom", "<u4", 5), ("reserved", "<u4")])
# efx_overlay_event (one 64-byte record per event, an array of them is the list) and efx_overlay_opts (passed like
# efx_denoise_opts)
OVERLAY_EVENT_DTYPE = np.dtype([("first", "<i8"), ("last", "<i8"), ("offset", "<u8"), ("stream", "<i4"), ("x", "<i4"), ("y", "<i4"),
                                ("pitch", "<u4"), ("colour", "<u4"), ("w", "<u2"), ("h", "<u2"), ("opacity", "<u2"),
                                ("fade_in", "<u2"), ("fade_out", "<u2"), ("kind", "u1"), ("reserved0", "u1"), ("reserved", "<u8")])
OVERLAY_OPTS_DTYPE = np.dtype([("n_streams", "<i4"), ("n_pictures", "<i4"), ("n_events", "<i4"), ("reserved", "<i4"),
                               ("first_picture", "<i8"), ("stride", "<u8"), ("atlas_bytes", "<u8")])
# efx_limit_peaks_opts and efx_limit_opts (passed like efx_denoise_opts)
LIMIT_PEAKS_OPTS_DTYPE = np.dtype([("n_streams", "<i4"), ("n_samples", "<i4"), ("rate", "<i4"), ("reserved", "<i4"),
                                   ("first_sample", "<i8"), ("peaks_first", "<i8"), ("pcm_stride", "<u8"), ("peaks_stride", "<u8")])
LIMIT_OPTS_DTYPE = np.dtype([("n_streams", "<i4"), ("n_samples", "<i4"), ("rate", "<i4"), ("half_window", "<i4"), ("ceiling", "<i4"),
                             ("fixed_gain_q12", "<i4"), ("n_peaks", "<i4"), ("reserved", "<i4"), ("first_sample", "<i8"),
                             ("peaks_first", "<i8"), ("target_ms", "<u8"), ("src_stride", "<u8"), ("dst_stride", "<u8"),
                             ("peaks_stride", "<u8")])

# every symbol include/efx.h declares: (name, restype, argtypes)
_P = C.c_void_p
_SYMBOLS = {
    "efx_create": (C.c_int, [C.POINTER(_Config), C.POINTER(_P)]),
    "efx_destroy": (None, [_P]),
    "efx_last_error": (C.c_char_p, [_P]),
    "efx_status_string": (C.c_char_p, [C.c_int]),
    "efx_upload_streams": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t), C.c_int]),
    "efx_upload_streams_inplace": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t), C.c_int]),
    "efx_download_es": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "efx_host_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "efx_host_free": (C.c_int, [_P, _P]),
    "efx_host_register": (C.c_int, [_P, _P, C.c_size_t]),
    "efx_host_unregister": (C.c_int, [_P, _P]),
    "efx_stream_layout": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "efx_upload_done": (C.c_int, [_P]),
    "efx_debug_poke": (C.c_int, [_P, _P, C.c_size_t, C.c_longlong]),
    "efx_set_option": (C.c_int, [_P, C.c_int, C.c_int]),
    "efx_get_option": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "efx_reset": (C.c_int, [_P]),
    "efx_erase_frames": (C.c_int, [_P]),
    "efx_play_reset": (C.c_int, [_P]),
    "efx_stream_state": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "efx_decode": (C.c_int, [_P]),
    "efx_decode_from": (C.c_int, [_P, C.c_int]),
    "efx_decode_range": (C.c_int, [_P, C.c_int, C.c_int]),
    "efx_stream_picture_slot": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "efx_sync": (C.c_int, [_P]),
    "efx_picture_count": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "efx_stream_status": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32)]),
    "efx_picture_pts": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "efx_picture_slot": (C.c_int, [_P, C.c_int]),
    "efx_frame_device_ptr": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "efx_download_frame": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "efx_frame_hashes": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "efx_upload_frame": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "efx_video_get_params": (C.c_int, [C.c_int, C.POINTER(_VideoParams)]),
    "efx_export_bytes": (C.c_size_t, [C.c_int]),
    "efx_export_frames": (C.c_int, [_P, C.POINTER(_ExportOpts), _P]),
    "efx_import_src_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "efx_import_frames": (C.c_int, [_P, C.POINTER(_ImportOpts), _P, _P]),
    "efx_detect_crop": (C.c_int, [_P, C.POINTER(_CropOpts), _P, _P, _P]),
    "efx_import_surfaces": (C.c_int, [_P, C.POINTER(_Surface), C.POINTER(_ImportOpts), _P, _P]),
    "efx_detect_crop_surfaces": (C.c_int, [_P, C.POINTER(_Surface), C.POINTER(_CropOpts), _P, _P, _P]),
    "efx_surface_layout": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(_Surface)]),
    "efx_deinterlace": (C.c_int, [_P, C.POINTER(_Surface), C.POINTER(_DeintOpts), _P, _P]),
    "efx_deinterlace_count": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "efx_detelecine": (C.c_int, [_P, C.POINTER(_Surface), C.POINTER(_DetelecineOpts), _P, _P, _P]),
    "efx_detelecine_count": (C.c_int, [C.c_int, C.c_int]),
    "efx_detect_scan": (C.c_int, [_P, C.POINTER(_Surface), _P, _P, _P, _P]),
    "efx_scan_verdict": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "efx_denoise": (C.c_int, [_P, C.POINTER(_Surface), _P, _P, _P, _P]),
    "efx_overlay": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "efx_overlay_check": (C.c_int, [_P, C.c_int, C.c_uint64]),
    "efx_import_set_colour": (C.c_int, [_P, C.POINTER(_ImportColour)]),
    "efx_import_colour_coefs": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "efx_import_set_hdr": (C.c_int, [_P, C.POINTER(_ImportHdr)]),
    "efx_import_hdr_tables": (C.c_int, [C.POINTER(_ImportHdr), C.c_int, C.c_void_p, C.c_size_t]),
    "efx_compare_pictures": (C.c_int, [_P, C.POINTER(_CompareOpts), _P, _P, _P, _P]),
    "efx_compare_psnr": (C.c_double, [C.c_uint64, C.c_uint64]),
    "efx_compare_ssim": (C.c_double, [C.c_int64, C.c_int]),
    "efx_trick_pick": (C.c_int, [_P, C.POINTER(_TrickOpts), _P, _P, _P]),
    "efx_trick_count": (C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    "efx_encode": (C.c_int, [_P, C.POINTER(_EncodeOpts), _P, _P, _P, _P, _P]),
    "efx_encode_rc": (C.c_int, [_P, C.POINTER(_EncodeOpts), C.POINTER(_EncodeRate), _P, _P, _P, _P, _P, _P]),
    "efx_encode_bound": (C.c_size_t, [C.c_int, C.c_int]),
    "efx_encode_set_picture_rate": (C.c_int, [_P, C.c_int]),
    "efx_encode_set_scene_cut": (C.c_int, [_P, C.POINTER(_SceneCut)]),
    "efx_encode_picture_info": (C.c_int, [_P, C.c_int, C.POINTER(_EncPictureInfo), C.c_int]),
    "efx_encode_set_adaptive_quant": (C.c_int, [_P, C.POINTER(_AdaptiveQuant)]),
    "efx_encode_mb_quant": (C.c_int, [_P, C.c_int, C.c_int, C.c_void_p]),
    "efx_picture_pts_offset": (C.c_int64, [C.c_int, C.c_int64]),
    "efx_picture_rate_code": (C.c_int, [C.c_int64, C.c_int64]),
    "efx_conform_rate": (C.c_int, [_P, C.POINTER(_ConformOpts), _P, _P]),
    "efx_conform_count": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64]),
    "efx_conform_source": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int64]),
    "efx_composite_fields": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "efx_composite_fields_ex": (C.c_int, [_P, C.POINTER(_FieldOpts), _P]),
    "efx_demux_audio": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t), _P, C.c_size_t, _P]),
    "efx_index_streams": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t), _P, C.c_uint32, _P, _P, C.c_size_t]),
    "efx_idx_build": (C.c_size_t, [_P, C.POINTER(_P), _P, C.c_size_t]),
    "efx_idx_pts2offset": (C.c_uint32, [_P, C.c_int64, C.c_int]),
    "efx_idx_pts2pts": (C.c_int64, [_P, C.c_int64, C.c_int]),
    "efx_sbc_state_bytes": (C.c_size_t, []),
    "efx_sbc_decode": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.c_int, C.c_int, _P, _P, C.c_size_t, _P, _P, C.c_int]),
    "efx_sbc_frame_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "efx_sbc_enc_state_bytes": (C.c_size_t, []),
    "efx_sbc_encode": (C.c_int, [_P, C.POINTER(_SbcEncodeOpts), _P, _P, _P]),
    "efx_import_pcm": (C.c_int, [_P, C.POINTER(_ImportPcmOpts), _P, _P, _P]),
    "efx_import_pcm_out_samples": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int]),
    "efx_import_pcm_delay": (C.c_int, [C.c_int, C.c_int]),
    "efx_import_pcm_state_bytes": (C.c_size_t, []),
    "efx_import_pcm_filter": (C.c_int, [_P, C.c_int]),
    "efx_loudness_steps": (C.c_int, [_P, C.POINTER(_LoudnessStepsOpts), _P, _P, _P]),
    "efx_loudness_gate": (C.c_int, [_P, C.POINTER(_LoudnessGateOpts), _P, _P, _P]),
    "efx_pcm_gain": (C.c_int, [_P, C.POINTER(_PcmGainOpts), _P, _P, _P]),
    "efx_loudness_lufs": (C.c_double, [C.c_uint64, C.c_int]),
    "efx_loudness_thresholds": (C.c_int, [C.c_int, C.c_double, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint32)]),
    "efx_loudness_coefs": (C.c_int, [C.c_int, C.POINTER(C.c_int32)]),
    "efx_loudness_state_bytes": (C.c_size_t, [C.c_int]),
    "efx_loudness_step_count": (C.c_int, [C.c_int, C.c_int64, C.c_int]),
    "efx_limit_peaks": (C.c_int, [_P, _P, _P, _P]),
    "efx_pcm_limit": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "efx_limit_block": (C.c_int, [C.c_int]),
    "efx_limit_gain": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int]),
    "efx_mux_av": (C.c_int, [_P, C.POINTER(_MuxOpts), _P, _P, _P, _P, _P, _P]),
    "efx_mux_bound": (C.c_size_t, [C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "efx_mux_audio_packets": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "efx_pdm": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "efx_set_timing": (C.c_int, [_P, C.c_int]),
    "efx_get_timing": (C.c_int, [_P, C.POINTER(_Timing)]),
    "efx_partition_first": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "efx_numa_node_of_pci": (C.c_int, [C.c_char_p]),
    "efx_numa_cpus_of_node": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_int]),
    "efx_numa_bind_thread": (C.c_int, [C.c_int]),
    "efx_multi_create": (C.c_int, [C.POINTER(_Config), C.POINTER(C.c_int), C.c_int, C.POINTER(_P)]),
    "efx_multi_destroy": (None, [_P]),
    "efx_multi_device_count": (C.c_int, [_P]),
    "efx_multi_context": (_P, [_P, C.c_int]),
    "efx_multi_last_error": (C.c_char_p, [_P]),
    "efx_multi_upload_streams": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t), C.c_int]),
    "efx_multi_locate": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "efx_multi_decode": (C.c_int, [_P]),
    "efx_multi_sync": (C.c_int, [_P]),
    "efx_multi_reset": (C.c_int, [_P]),
    "efx_multi_results": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "efx_multi_frame_hashes": (C.c_int, [_P, _P]),
    "efx_device_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "efx_device_free": (C.c_int, [_P, _P]),
    "efx_memcpy_h2d": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "efx_memcpy_d2h": (C.c_int, [_P, _P, _P, C.c_size_t]),
}
