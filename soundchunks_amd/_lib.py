"""ctypes binding of the in-tree C-ABI library (include/soundchunks.h).

The library is built in-tree by ``__graft_entry__.build()`` (or
``make -C soundchunks_amd/csrc``) into ``soundchunks_amd/lib/libsoundchunks_amd.so``.
There is no CPU fallback: if the library or a gfx950 device is missing, every
compute call raises.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libsoundchunks_amd.so"


class GscOptions(ctypes.Structure):
    """Mirror of ``gsc_options`` (TEncoder fields, encoder.lpr:1486-1509)."""

    _fields_ = [
        ("bit_rate", ctypes.c_int),
        ("precision", ctypes.c_int),
        ("low_cut", ctypes.c_double),
        ("high_cut", ctypes.c_double),
        ("chunk_bit_depth", ctypes.c_int),
        ("chunk_size", ctypes.c_int),
        ("chunks_per_frame", ctypes.c_int),
        ("reduce_bass_band", ctypes.c_int),
        ("vfr", ctypes.c_double),
        ("chunk_blend", ctypes.c_int),
        ("frame_length", ctypes.c_double),
        ("python_reduce", ctypes.c_int),
        ("verbose", ctypes.c_int),
    ]


class GscTiming(ctypes.Structure):
    _fields_ = [
        ("host_prepare_ms", ctypes.c_double),
        ("host_frames_ms", ctypes.c_double),
        ("gpu_yakmo_ms", ctypes.c_double),
        ("gpu_scan_ms", ctypes.c_double),
        ("gpu_knnfit_ms", ctypes.c_double),
        ("host_post_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("frames", ctypes.c_int),
        ("reduce_frames", ctypes.c_int),
        ("points", ctypes.c_longlong),
        ("scan_passes", ctypes.c_longlong),
        ("scan_slow", ctypes.c_longlong),
        ("scan_point_passes", ctypes.c_longlong),
        ("knnfit_pairs", ctypes.c_longlong),
        ("scan_launches", ctypes.c_int),
        ("knnfit_launches", ctypes.c_int),
        ("scan_restarts", ctypes.c_longlong),
        ("gpu_dsp_ms", ctypes.c_double),
        ("post_overlap_ms", ctypes.c_double),
        ("post_groups", ctypes.c_int),
        ("gpu_recon_ms", ctypes.c_double),
        ("knnfit_overflow", ctypes.c_longlong),
    ]


class GscDecodeTiming(ctypes.Structure):
    """Mirror of ``gsc_decode_timing``."""

    _fields_ = [
        ("host_index_ms", ctypes.c_double),
        ("h2d_ms", ctypes.c_double),
        ("gpu_unpack_ms", ctypes.c_double),
        ("gpu_synth_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("frames", ctypes.c_int),
        ("symbols", ctypes.c_longlong),
        ("samples", ctypes.c_longlong),
        ("h2d_bytes", ctypes.c_longlong),
    ]


class GscOpenTiming(ctypes.Structure):
    """Mirror of ``gsc_open_timing``."""

    _fields_ = [
        ("host_ms", ctypes.c_double),
        ("upload_ms", ctypes.c_double),
        ("verify_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("uploaded_bytes", ctypes.c_longlong),
        ("checkpoints", ctypes.c_longlong),
    ]


class GscSetOpenTiming(ctypes.Structure):
    """Mirror of ``gsc_set_open_timing``."""

    _fields_ = [
        ("host_ms", ctypes.c_double),
        ("upload_ms", ctypes.c_double),
        ("expand_ms", ctypes.c_double),
        ("verify_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("uploaded_bytes", ctypes.c_longlong),
        ("streams", ctypes.c_longlong),
        ("frames", ctypes.c_longlong),
        ("checkpoints", ctypes.c_longlong),
        ("device_allocations", ctypes.c_int),
        ("h2d_copies", ctypes.c_int),
        ("launches", ctypes.c_int),
        ("synchronisations", ctypes.c_int),
    ]


class GscCrop(ctypes.Structure):
    """Mirror of ``gsc_crop``: per-channel sample positions of one stream."""

    _fields_ = [("stream", ctypes.c_int), ("begin", ctypes.c_longlong), ("count", ctypes.c_longlong)]


class GscCropFormat(ctypes.Structure):
    """Mirror of ``gsc_crop_format``: what ``gsc_decode_crops_fmt`` writes."""

    _fields_ = [("dtype", ctypes.c_int), ("layout", ctypes.c_int), ("length", ctypes.c_longlong),
                ("out_rate", ctypes.c_int), ("out_channels", ctypes.c_int)]


class GscCropCallStats(ctypes.Structure):
    """Mirror of ``gsc_crop_call_stats``."""

    _fields_ = [("launches", ctypes.c_int), ("allocations", ctypes.c_int), ("copies", ctypes.c_int),
                ("synchronisations", ctypes.c_int), ("host_ms", ctypes.c_double)]


PCM_INT16, PCM_FLOAT32 = 0, 1
LAYOUT_TC, LAYOUT_CT = 0, 1


_FP = ctypes.POINTER(ctypes.c_float)
_IP = ctypes.POINTER(ctypes.c_int)
_U8P = ctypes.POINTER(ctypes.c_uint8)
_I16P = ctypes.POINTER(ctypes.c_int16)
_SZP = ctypes.POINTER(ctypes.c_size_t)
_LLP = ctypes.POINTER(ctypes.c_longlong)

# name -> (restype, argtypes); every symbol declared in include/soundchunks.h
SIGNATURES = {
    "yakmo_create": (ctypes.c_void_p, [ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int]),
    "yakmo_destroy": (None, [ctypes.c_void_p]),
    "yakmo_load_train_data": (None, [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(_FP)]),
    "yakmo_train_on_data": (None, [ctypes.c_void_p, _IP]),
    "yakmo_get_centroids": (None, [ctypes.c_void_p, ctypes.POINTER(_FP)]),
    "ann_kdtree_create": (ctypes.c_void_p, [ctypes.POINTER(_FP), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int]),
    "ann_kdtree_destroy": (None, [ctypes.c_void_p]),
    "ann_kdtree_search": (ctypes.c_int, [ctypes.c_void_p, _FP, ctypes.c_float, _FP]),
    "ann_kdtree_pri_search": (ctypes.c_int, [ctypes.c_void_p, _FP, ctypes.c_float, _FP]),
    "ann_kdtree_search_multi": (None, [ctypes.c_void_p, _IP, _FP, ctypes.c_int, _FP, ctypes.c_float]),
    "ann_kdtree_pri_search_multi": (None, [ctypes.c_void_p, _IP, _FP, ctypes.c_int, _FP, ctypes.c_float]),
    "gsc_default_options": (None, [ctypes.POINTER(GscOptions)]),
    "gsc_parse_options": (None, [ctypes.POINTER(GscOptions), ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]),
    "gsc_encode_wav": (ctypes.c_int, [_U8P, ctypes.c_size_t, ctypes.POINTER(GscOptions), ctypes.POINTER(_U8P),
                                      ctypes.POINTER(ctypes.c_size_t)]),
    "gsc_encode_wav_frames": (ctypes.c_int, [_U8P, ctypes.c_size_t, ctypes.POINTER(GscOptions), ctypes.c_int,
                                             ctypes.c_int, ctypes.POINTER(_U8P), ctypes.POINTER(ctypes.c_size_t),
                                             _IP]),
    "gsc_encode_wav_recon": (ctypes.c_int, [_U8P, ctypes.c_size_t, ctypes.POINTER(GscOptions), ctypes.POINTER(_U8P),
                                            ctypes.POINTER(ctypes.c_size_t),
                                            ctypes.POINTER(ctypes.POINTER(ctypes.c_int16)),
                                            ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_double)]),
    "gsc_count_frames": (ctypes.c_int, [_U8P, ctypes.c_size_t, ctypes.POINTER(GscOptions), _IP]),
    "gsc_prepare": (ctypes.c_void_p, [_U8P, ctypes.c_size_t, ctypes.POINTER(GscOptions)]),
    "gsc_prepared_frame_count": (ctypes.c_int, [ctypes.c_void_p]),
    "gsc_prepared_frame_chunks": (ctypes.c_int, [ctypes.c_void_p, _IP]),
    "gsc_prepared_frame_bounds": (ctypes.c_int, [ctypes.c_void_p, _IP, _IP]),
    "gsc_prepare_frames": (ctypes.c_void_p, [_U8P, ctypes.c_size_t, ctypes.POINTER(GscOptions), _IP, _IP, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int]),
    "gsc_prepare_many": (ctypes.c_void_p, [ctypes.POINTER(_U8P), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int,
                                           ctypes.POINTER(GscOptions)]),
    "gsc_prepared_file_count": (ctypes.c_int, [ctypes.c_void_p]),
    "gsc_prepared_file_frames": (ctypes.c_int, [ctypes.c_void_p, _IP]),
    "gsc_encode_prepared_files": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_U8P),
                                                 ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    "gsc_encode_prepared": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_U8P),
                                           ctypes.POINTER(ctypes.c_size_t)]),
    "gsc_encode_prepared_frames": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_U8P),
                                                  ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    "gsc_encode_prepared_with_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                      ctypes.POINTER(_U8P), ctypes.POINTER(ctypes.c_size_t),
                                                      ctypes.POINTER(_U8P), ctypes.POINTER(ctypes.c_size_t)]),
    "gsc_prepared_prepare_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "gsc_prepared_free": (None, [ctypes.c_void_p]),
    "gsc_frame_dsp": (ctypes.c_int, [_U8P, ctypes.c_size_t, ctypes.POINTER(GscOptions), ctypes.c_int, _IP,
                                     ctypes.POINTER(_FP), _IP]),
    "gsc_yakmo_seed_means": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _FP, ctypes.c_int, _FP]),
    "gsc_yakmo_seed_means_frames": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _IP, _FP, _IP, _FP, _IP]),
    "gsc_yakmo_chain_test": (ctypes.c_int, [ctypes.c_int, _FP, ctypes.c_int, ctypes.c_float, _IP, _FP, _FP, _FP,
                                            _FP]),
    "gsc_scan_reduce": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _FP, ctypes.c_int, _FP, _IP, ctypes.c_int, _IP]),
    "gsc_birch_labels": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _FP, ctypes.c_int, _IP]),
    "gsc_knnfit_assign": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _FP, ctypes.c_int, _FP, ctypes.c_float, _IP]),
    "gsc_knnfit_assign_frames": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _IP, _FP, _IP, _FP, _FP, _IP, _IP]),
    "gsc_index_create": (ctypes.c_void_p, [_U8P, ctypes.c_size_t]),
    "gsc_index_frame_count": (ctypes.c_int, [ctypes.c_void_p]),
    "gsc_index_info": (ctypes.c_int, [ctypes.c_void_p, _IP, _IP, _LLP]),
    "gsc_index_frames": (ctypes.c_int, [ctypes.c_void_p, _SZP, _IP, _IP, _IP, _LLP]),
    "gsc_index_free": (None, [ctypes.c_void_p]),
    "gsc_index_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_U8P), _SZP]),
    "gsc_index_create_with_table": (ctypes.c_void_p, [_U8P, ctypes.c_size_t, _U8P, ctypes.c_size_t]),
    "gsc_stream_open_with_table": (ctypes.c_void_p, [_U8P, ctypes.c_size_t, _U8P, ctypes.c_size_t]),
    "gsc_last_open_timing": (None, [ctypes.POINTER(GscOpenTiming)]),
    "gsc_stream_set_open": (ctypes.c_void_p, [ctypes.POINTER(_U8P), _SZP, ctypes.POINTER(_U8P), _SZP, ctypes.c_int]),
    "gsc_stream_set_count": (ctypes.c_int, [ctypes.c_void_p]),
    "gsc_stream_set_stream": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "gsc_stream_set_free": (None, [ctypes.c_void_p]),
    "gsc_last_set_open_timing": (None, [ctypes.POINTER(GscSetOpenTiming)]),
    "gsc_stream_tables": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _I16P, _U8P]),
    "gsc_encode_prepared_files_with_tables": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                             ctypes.POINTER(_U8P), _SZP, _SZP, ctypes.POINTER(_U8P),
                                                             _SZP, _SZP]),
    "gsc_decode_checkpoint_symbols": (ctypes.c_int, []),
    "gsc_index_locate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, _IP, _LLP, _IP, _LLP]),
    "gsc_stream_open": (ctypes.c_void_p, [_U8P, ctypes.c_size_t]),
    "gsc_stream_free": (None, [ctypes.c_void_p]),
    "gsc_stream_info": (ctypes.c_int, [ctypes.c_void_p, _IP, _IP, _LLP, _IP]),
    "gsc_stream_index": (ctypes.c_void_p, [ctypes.c_void_p]),
    "gsc_stream_device": (ctypes.c_int, [ctypes.c_void_p]),
    "gsc_decode_crops": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(GscCrop),
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                                        ctypes.c_void_p, _LLP]),
    "gsc_decode_crops_fmt": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(GscCrop),
                                            ctypes.c_int, ctypes.POINTER(GscCropFormat), ctypes.c_void_p,
                                            ctypes.c_void_p, _LLP]),
    "gsc_crop_binding_create": (ctypes.c_void_p, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int]),
    "gsc_crop_binding_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "gsc_crop_binding_mix": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p]),
    "gsc_mix_model": (ctypes.c_int, [_I16P, _LLP, ctypes.c_int, _I16P]),
    "gsc_crop_binding_last_call": (None, [ctypes.POINTER(GscCropCallStats)]),
    "gsc_crop_binding_free": (None, [ctypes.c_void_p]),
    "gsc_envelope_layout": (ctypes.c_int, [_LLP, ctypes.c_int, ctypes.c_int, _LLP]),
    "gsc_crop_binding_envelope": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_longlong, ctypes.c_void_p]),
    "gsc_crop_binding_fidelity": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), _LLP,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
                                                 ctypes.c_void_p]),
    "gsc_crop_plan_model": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
                                           ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, _LLP, _IP, _IP, _LLP,
                                           _LLP]),
    "gsc_resample_table": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _IP, _IP,
                                          ctypes.POINTER(ctypes.POINTER(ctypes.c_int32))]),
    "gsc_resample_prepare": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "gsc_resample_tile": (ctypes.c_int, []),
    "gsc_stream_decode_samples": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, _I16P]),
    "gsc_decode_indexed": (ctypes.c_int, [_U8P, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(_I16P), _SZP]),
    "gsc_decode": (ctypes.c_int, [_U8P, ctypes.c_size_t, ctypes.POINTER(_I16P), _SZP, _IP, _IP]),
    "gsc_decode_many": (ctypes.c_int, [ctypes.POINTER(_U8P), _SZP, ctypes.c_int, ctypes.POINTER(_I16P), _SZP, _IP,
                                       _IP]),
    "gsc_last_decode_timing": (None, [ctypes.POINTER(GscDecodeTiming)]),
    "gsc_last_timing": (None, [ctypes.POINTER(GscTiming)]),
    "gsc_device_count": (ctypes.c_int, []),
    "gsc_set_device": (ctypes.c_int, [ctypes.c_int]),
    "gsc_last_error": (ctypes.c_char_p, []),
    "gsc_free": (None, [ctypes.c_void_p]),
}

_lib = None


class GscError(RuntimeError):
    pass


def load(path: str | os.PathLike | None = None) -> ctypes.CDLL:
    """Load the product library (fails loudly if it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path is not None else Path(os.environ.get("GSC_LIB", LIB_PATH))
    if not p.exists():
        raise GscError(f"{p} not built; run __graft_entry__.build() or make -C soundchunks_amd/csrc")
    lib = ctypes.CDLL(str(p))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise GscError(load().gsc_last_error().decode(errors="replace"))
