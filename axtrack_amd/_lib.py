"""ctypes binding of libaxtrack_hip.so (include/axtrack_hip.h). No CPU fallback: if the HIP
library is missing or a call fails, this module raises."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AXT_LIB_PATH: a diagnostic build of the same library (profiles/wino_stamps.py); there is still no fallback
LIB_PATH = os.environ.get('AXT_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libaxtrack_hip.so')

c_void_p, c_int, c_float, c_double, c_size_t, c_int64 = (
    ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_int64)

# name -> (restype, argtypes); mirrors include/axtrack_hip.h one to one
SIGNATURES = {
    'axt_last_error': (ctypes.c_char_p, []),
    'axt_abi_version': (c_int, []),
    'axt_detector_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, ctypes.POINTER(c_void_p)]),
    'axt_detector_destroy': (None, [c_void_p]),
    'axt_detector_set_arith': (c_int, [c_void_p, c_int]),
    'axt_detector_set_fused_front': (c_int, [c_void_p, c_int]),
    'axt_detector_device_bytes': (c_size_t, [c_void_p]),
    'axt_cnn_forward': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'axt_cnn_forward_frames': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                       c_void_p, c_void_p]),
    'axt_cnn_features_frames': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                        c_void_p, c_void_p]),
    'axt_cnn_front_frames': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    'axt_cnn_back': (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    'axt_cnn_flops_per_tile': (c_double, []),
    'axt_detector_set_profiling': (c_int, [c_void_p, c_int]),
    'axt_detector_read_profile': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    'axt_cnn_kernel_flops_per_tile': (c_double, [c_int]),
    'axt_preprocess_u16': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_int, c_float, c_void_p,
                                   c_void_p]),
    'axt_preprocess_stats_u16': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_int, c_void_p, c_void_p,
                                         ctypes.POINTER(c_size_t), c_void_p]),
    'axt_preprocess_u16_framewise': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_int, c_void_p,
                                             c_void_p, c_void_p]),
    'axt_tile_occupancy': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'axt_decode_stitch_nms': (c_int, [c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    'axt_grid_create': (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    'axt_grid_destroy': (None, [c_void_p]),
    'axt_obs_costs': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p, c_void_p]),
    'axt_path_cost': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                              c_int, c_void_p, c_void_p]),
    'axt_path_cells': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                               c_int, c_void_p, c_void_p, c_void_p]),
    'axt_build_arcs': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                               c_int, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p,
                               c_void_p]),
    'axt_box_histograms': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p]),
    'axt_mcf_solve': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                              c_void_p, c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]),
    'axt_mcf_solve_duals': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                    c_void_p, c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int64),
                                    c_void_p, c_void_p, ctypes.POINTER(c_int64)]),
    'axt_mcf_shard_begin': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                    ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64)]),
    'axt_mcf_shard_export': (c_int, [c_void_p, c_void_p]),
    'axt_mcf_shard_finish': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int),
                                     ctypes.POINTER(c_int64)]),
    'axt_mcf_shard_finish_duals': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int),
                                           ctypes.POINTER(c_int64), c_void_p, c_void_p, ctypes.POINTER(c_int64)]),
    'axt_mcf_shard_free': (None, [c_void_p]),
    'axt_hungarian_pairs': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'axt_chain_tracks': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'axt_ided_table': (c_int, [c_void_p] * 5 + [c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'axt_detection_confusion': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                        c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'axt_mot_scores': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, ctypes.POINTER(c_size_t), c_void_p]),
    'axt_arc_cost_int': (c_int64, [c_double, c_int, c_int64, c_int64]),
    'axt_track_links': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    'axt_link_paths': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                               c_int, c_void_p, c_void_p, c_void_p]),
    'axt_link_cells': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                               ctypes.POINTER(c_int64), c_void_p]),
    'axt_target_tile_size': (c_int, []),
    'axt_target_field': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int),
                                 c_void_p]),
    'axt_target_sample': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                  c_void_p, c_void_p, c_void_p]),
    'axt_target_paths': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                 c_void_p, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    'axt_segment_tile_size': (c_int, []),
    'axt_segment_edges': (c_int, [c_void_p, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    'axt_segment_histogram': (c_int, [c_void_p, c_int64, c_double, c_double, c_void_p, c_void_p]),
    'axt_segment_close': (c_int, [c_void_p, c_int, c_int, c_double, c_int, c_void_p, c_void_p]),
    'axt_segment_flood': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, ctypes.POINTER(c_int), c_void_p]),
    'axt_yolo_targets': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'axt_head_trainer_create': (c_int, [c_int, c_int, c_int, c_int] + [c_void_p] * 6 + [c_int, ctypes.POINTER(c_void_p)]),
    'axt_head_trainer_destroy': (None, [c_void_p]),
    'axt_head_trainer_device_bytes': (c_size_t, [c_void_p]),
    'axt_head_trainer_read_weights': (c_int, [c_void_p] * 7),
    'axt_head_trainer_read_moments': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                              ctypes.POINTER(c_int64)]),
    'axt_head_trainer_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'axt_head_trainer_loss': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_double, c_double,
                                      c_void_p, c_void_p, c_void_p]),
    'axt_head_trainer_step': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_double, c_double, c_double,
                                      c_double, c_double, c_void_p]),
    'axt_head_trainer_input_grad': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'axt_cnn_block_features_frames': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int,
                                              c_void_p, c_void_p]),
    'axt_conv_trainer_create': (c_int, [c_int, c_int, c_int, c_int] + [c_void_p] * 6 + [c_int, ctypes.POINTER(c_void_p)]),
    'axt_conv_trainer_destroy': (None, [c_void_p]),
    'axt_conv_trainer_device_bytes': (c_size_t, [c_void_p]),
    'axt_conv_trainer_read_weights': (c_int, [c_void_p] * 5),
    'axt_conv_trainer_read_moments': (c_int, [c_void_p, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int64)]),
    'axt_conv_trainer_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'axt_conv_trainer_step': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_double, c_double, c_double,
                                      c_double, c_double, c_void_p]),
    'axt_conv_trainer_input_grad': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'axt_conv_trainer_set_batch_stats': (c_int, [c_void_p, c_int, c_double]),
    'axt_conv_trainer_read_stats': (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p, c_void_p]),
    'axt_maxpool2_forward': (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    'axt_maxpool2_backward': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    'axt_conv_trainer_create_strided': (c_int, [c_int] * 5 + [c_void_p] * 6 + [c_int, ctypes.POINTER(c_void_p)]),
    'axt_tile_stacks': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                c_void_p]),
    'axt_detector_load_conv_block': (c_int, [c_void_p, c_int] + [c_void_p] * 7),
    'axt_detector_load_linear': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'axt_conv_trainer_export': (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    'axt_head_trainer_export': (c_int, [c_void_p, c_void_p, c_void_p]),
    'axt_tiff_decode_u16': (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p,
                                    c_void_p]),
    'axt_jpeg_scan_bound': (c_int64, [c_int, c_int]),
    'axt_jpeg_scratch_bytes': (c_int64, [c_int, c_int, c_int]),
    'axt_jpeg_encode_rgb8': (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                     c_int64, c_void_p]),
    'axt_augment_frame_chunk': (c_int, []),
    'axt_augment_frames': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float,
                                   c_float, c_float, c_void_p, c_void_p, c_void_p]),
    'axt_render_tile_size': (c_int, []),
    'axt_render_frames': (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
}

# exported and bound like the above, but declared under csrc/ (axt_tiff_inflate.h, axt_tiff_deflate.h) and not yet part of
# the public ABI of include/, whose contract table lists every prototype there
INTERNAL_SIGNATURES = {
    'axt_tiff_inflate_u16': (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    'axt_tiff_deflate_bound': (c_int64, [c_int64]),
    'axt_tiff_deflate_u16': (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'axt_tiff_compact_streams': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
}

_lib = None


class AxtError(RuntimeError):
    pass


def load():
    """Load the HIP library; raise (never fall back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AxtError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                           f'or `make -C axtrack_amd/csrc`. axtrack_amd has no CPU fallback.')
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in {**SIGNATURES, **INTERNAL_SIGNATURES}.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc < 0:
        raise AxtError(f'{what} failed ({rc}): {load().axt_last_error().decode()}')
    return rc


def dptr(t):
    """Device (or host) address of a torch tensor / numpy array; None -> NULL."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()
