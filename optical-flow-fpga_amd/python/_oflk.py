"""ctypes binding of liboflk.so (include/oflk.h) -- the only native dependency of
the drop-in modules in this directory.

There is no CPU fallback: if the library is missing, or no MI355X-class GPU is
usable, every call raises.  Build with ``python __graft_entry__.py`` (or
``make -C optical-flow-fpga_amd/csrc``).
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("OFLK_LIB", _HERE.parent / "liboflk.so"))

OFLK_OK = 0
OFLK_ERR_INVALID = -1
OFLK_ERR_NO_DEVICE = -2
OFLK_ERR_HIP = -3
OFLK_ERR_UNSUPPORTED = -4
OFLK_ERR_NOMEM = -5

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int)
_f64p = ctypes.POINTER(ctypes.c_double)
_vp = ctypes.c_void_p
_I, _U, _F, _D, _Z = ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_double, ctypes.c_size_t

# The runs of arguments that many declarations share, in the field order of the C side's structs (and of the records below)
_KLT = [_I] * 3 + [_F] * 5 + [_I]   # KltConfig: levels, window_size, iters, alpha, beta, max_residual, quality_level, min_distance, max_corners
_TRACKING = _KLT + [_I]             # ... and detect_every (Tracking)
_RANSAC = [_I, _F, _U]              # hypotheses, threshold, seed
_FIT = [_I] + _RANSAC               # FitConfig: model, then the above (Fit)
_WINDOW = [_f64p, _I]               # TrajWindow: weights, radius (Window)
_ALIGN = [_I] * 5 + [_F]            # AlignConfig: H, W, levels, iterations, model, min_share
_ROBUST = [_F, _I]                  # ... robust_delta, photometric, of the robust forms
_ALIGN_D_IO = [_vp, _vp, _vp, _Z, _vp, _vp, _vp]        # d_model_in, d_status_in, d_workspace, workspace_bytes, d_model_out, d_status_out, d_stats
_ALIGN_H_IO = [_f32p, _i32p, _f32p, _i32p, _f64p]       # model_in, status_in, model_out, status_out, stats
_STAB_OUT = [_f32p, _f32p, _i32p, _vp]                  # correction, model_out, counts_out, held (behind the frames out)
_INTERP = [_F, _F, _I, _f64p, _I]   # InterpConfig: alpha, beta, refine, taus, n (Interp)
_DENOISE = [_I, _F]                 # radius, strength, behind alpha, beta (and the sequence forms' flow_median) (Denoise)

# every exported symbol of include/oflk.h: name -> (restype, argtypes)
SIGNATURES = {
    "oflk_version": (ctypes.c_char_p, []),
    "oflk_device_count": (ctypes.c_int, []),
    "oflk_last_error": (ctypes.c_char_p, []),
    "oflk_set_device": (ctypes.c_int, [ctypes.c_int]),
    "oflk_compute_gradients": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p]),
    "oflk_from_gradients": (ctypes.c_int, [_f32p, _f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p]),
    "oflk_single_scale": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p]),
    "oflk_pyramid_level_dims": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, _i32p]),
    "oflk_build_pyramid": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.POINTER(_f32p)]),
    "oflk_build_pyramid_w": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_double),
                                            ctypes.c_int, ctypes.POINTER(_f32p)]),
    "oflk_warp": (ctypes.c_int, [_f32p, _f32p, _f32p, ctypes.c_int, ctypes.c_int, _f32p]),
    "oflk_upsample_flow": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p]),
    "oflk_upsample_staged": (ctypes.c_int, [ctypes.c_int] * 4),
    "oflk_pyramid_step_fused": (ctypes.c_int, [ctypes.c_int] * 5),
    "oflk_pyramid_step_form": (ctypes.c_int, [ctypes.c_int] * 5),
    "oflk_pyramid_step_half": (ctypes.c_int, [ctypes.c_int] * 5),
    "oflk_pyramidal": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _i32p]),
    "oflk_single_scale_batch": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p]),
    "oflk_pyramidal_batch": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _i32p]),
    "oflk_single_scale_u8": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p]),
    "oflk_pyramidal_u8": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _i32p]),
    "oflk_u8_to_f32": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
    "oflk_plan_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "oflk_plan_destroy": (ctypes.c_int, [_vp]),
    "oflk_plan_workspace_bytes": (ctypes.c_size_t, [_vp]),
    "oflk_plan_single_scale": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "oflk_plan_pyramidal": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "oflk_plan_single_scale_u8": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "oflk_plan_pyramidal_u8": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "oflk_single_scale_batch_multi": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p]),
    "oflk_pyramidal_batch_multi": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _i32p]),
    "oflk_pyramidal_u8_multi": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _i32p]),
    "oflk_pyramidal_sequence": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 6 + [_f32p, _f32p, _f32p, _i32p]),
    "oflk_pyramidal_sequence_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [_f32p, _f32p, _f32p, _i32p]),
    "oflk_pyramidal_sequence_multi": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 7 + [_f32p, _f32p, _f32p, _i32p]),
    "oflk_single_scale_sequence": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 4 + [_f32p, _f32p]),
    "oflk_plan_pyramidal_sequence": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "oflk_plan_pyramidal_sequence_u8": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "oflk_plan_pyramidal_sequence_fb": (ctypes.c_int, [_vp] * 7),
    "oflk_plan_pyramidal_sequence_fb_u8": (ctypes.c_int, [_vp] * 7),
    "oflk_plan_read_log_backward": (ctypes.c_int, [_vp, _f32p, _i32p, _vp]),
    "oflk_plan_read_uncertain_backward": (ctypes.c_int, [_vp, _i32p, _vp]),
    "oflk_plan_resolve_uncertain_sequence_fb": (ctypes.c_int, [_vp] * 7 + [_i32p]),
    "oflk_plan_resolve_uncertain_sequence_fb_u8": (ctypes.c_int, [_vp] * 7 + [_i32p]),
    "oflk_fb_consistency": (ctypes.c_int, [_vp] * 4 + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [_vp] * 5),
    "oflk_fb_consistency_host": (ctypes.c_int, [_f32p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [_f32p, _f32p, _vp, _vp]),
    "oflk_pyramidal_sequence_fb": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 6 + [ctypes.c_float] * 2 + [_f32p] * 6 + [_vp, _vp]),
    "oflk_pyramidal_sequence_fb_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [ctypes.c_float] * 2 + [_f32p] * 6 + [_vp, _vp]),
    "oflk_interpolate_frames": (ctypes.c_int, [_vp] + [_I] * 4 + [_vp] * 4 + _INTERP + [_vp, _vp, _vp]),
    "oflk_interpolate_frames_host": (ctypes.c_int, [_f32p] + [_I] * 3 + [_f32p] * 4 + _INTERP + [_f32p, _vp]),
    "oflk_interpolate_frames_host_u8": (ctypes.c_int, [_vp] + [_I] * 3 + [_f32p] * 4 + _INTERP + [_vp, _vp]),
    "oflk_interpolate_sequence": (ctypes.c_int, [_f32p] + [_I] * 6 + _INTERP + [_f32p, _vp]),
    "oflk_interpolate_sequence_u8": (ctypes.c_int, [_vp] + [_I] * 6 + _INTERP + [_vp, _vp]),
    "oflk_interpolate_frames_packed": (ctypes.c_int, [_vp] + [_I] * 4 + [_vp] * 4 + _INTERP + [_vp, _vp, _vp]),
    "oflk_interpolate_frames_nv12": (ctypes.c_int, [_vp] + [_I] * 4 + [_vp] * 4 + _INTERP + [_vp, _vp, _vp]),
    "oflk_interpolate_frames_packed_host": (ctypes.c_int, [_vp] + [_I] * 4 + [_f32p] * 4 + _INTERP + [_vp, _vp]),
    "oflk_interpolate_frames_nv12_host": (ctypes.c_int, [_vp] + [_I] * 4 + [_f32p] * 4 + _INTERP + [_vp, _vp]),
    "oflk_interpolate_sequence_packed": (ctypes.c_int, [_vp] + [_I] * 8 + _INTERP + [_vp, _vp]),
    "oflk_interpolate_sequence_nv12": (ctypes.c_int, [_vp] + [_I] * 7 + _INTERP + [_vp, _vp]),
    "oflk_flow_median": (ctypes.c_int, [_vp, _vp] + [_I] * 4 + [_vp]),
    "oflk_flow_median_host": (ctypes.c_int, [_f32p, _f32p] + [_I] * 4),
    "oflk_flow_median_tile": (ctypes.c_int, [_i32p, _i32p]),
    "oflk_pyramidal_sequence_fb_median": (ctypes.c_int, [_f32p] + [_I] * 6 + [_F] * 2 + [_I] + [_f32p] * 6 + [_vp, _vp]),
    "oflk_pyramidal_sequence_fb_median_u8": (ctypes.c_int, [_vp] + [_I] * 6 + [_F] * 2 + [_I] + [_f32p] * 6 + [_vp, _vp]),
    "oflk_interpolate_sequence_median": (ctypes.c_int, [_f32p] + [_I] * 6 + _INTERP + [_I, _f32p, _vp]),
    "oflk_interpolate_sequence_median_u8": (ctypes.c_int, [_vp] + [_I] * 6 + _INTERP + [_I, _vp, _vp]),
    "oflk_interpolate_sequence_packed_median": (ctypes.c_int, [_vp] + [_I] * 8 + _INTERP + [_I, _vp, _vp]),
    "oflk_interpolate_sequence_nv12_median": (ctypes.c_int, [_vp] + [_I] * 7 + _INTERP + [_I, _vp, _vp]),
    "oflk_denoise_frames_host": (ctypes.c_int, [_f32p] + [_I] * 3 + [_f32p] * 4 + [_F, _F] + _DENOISE + [_f32p, _vp]),
    "oflk_denoise_frames_host_u8": (ctypes.c_int, [_vp] + [_I] * 3 + [_f32p] * 4 + [_F, _F] + _DENOISE + [_vp, _vp]),
    "oflk_denoise_sequence": (ctypes.c_int, [_f32p] + [_I] * 6 + [_F, _F, _I] + _DENOISE + [_f32p, _vp]),
    "oflk_denoise_sequence_u8": (ctypes.c_int, [_vp] + [_I] * 6 + [_F, _F, _I] + _DENOISE + [_vp, _vp]),
    "oflk_track_points": (ctypes.c_int, [_vp] * 4 + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, _vp]),
    "oflk_track_points_host": (ctypes.c_int, [_f32p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [_i32p, _f32p, ctypes.c_int, _f32p, _vp]),
    "oflk_pyramidal_sequence_tracks": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 6 + [ctypes.c_float] * 2 + [_i32p, _f32p, ctypes.c_int, _f32p, _vp]),
    "oflk_pyramidal_sequence_tracks_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [ctypes.c_float] * 2 + [_i32p, _f32p, ctypes.c_int, _f32p, _vp]),
    "oflk_sparse_lk": (ctypes.c_int, [_f32p, _f32p] + [ctypes.c_int] * 5 + [_f32p, ctypes.c_int, _f32p, _vp, _f32p]),
    "oflk_sparse_lk_u8": (ctypes.c_int, [_vp, _vp] + [ctypes.c_int] * 5 + [_f32p, ctypes.c_int, _f32p, _vp, _f32p]),
    "oflk_plan_sparse_tracks": (ctypes.c_int, [_vp, _vp, ctypes.c_int] + [ctypes.c_float] * 3 + [ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, _vp]),
    "oflk_pyramidal_sequence_sparse_tracks": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 6 + [ctypes.c_float] * 3 + [_i32p, _f32p, ctypes.c_int, _f32p, _vp]),
    "oflk_pyramidal_sequence_sparse_tracks_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [ctypes.c_float] * 3 + [_i32p, _f32p, ctypes.c_int, _f32p, _vp]),
    "oflk_pyramidal_sequence_klt_sparse": (ctypes.c_int, [_f32p] + [_I] * 3 + _KLT + [_i32p, _f32p, _f32p, _f32p, _vp]),
    "oflk_pyramidal_sequence_klt_sparse_u8": (ctypes.c_int, [_vp] + [_I] * 3 + _KLT + [_i32p, _f32p, _f32p, _f32p, _vp]),
    "oflk_pyramidal_sequence_klt_sparse_replenish": (ctypes.c_int, [_f32p] + [_I] * 3 + _TRACKING + [_f32p, _vp, _vp, _i32p, _f32p]),
    "oflk_pyramidal_sequence_klt_sparse_replenish_u8": (ctypes.c_int, [_vp] + [_I] * 3 + _TRACKING + [_f32p, _vp, _vp, _i32p, _f32p]),
    "oflk_plan_sparse_klt_replenish": (ctypes.c_int, [_vp, _vp, ctypes.c_int] + [ctypes.c_float] * 5 + [ctypes.c_int] * 3 + [_vp, ctypes.c_size_t] + [_vp] * 8),
    "oflk_corner_score": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp, _vp]),
    "oflk_corner_score_host": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 4 + [_f32p]),
    "oflk_corner_score_host_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_f32p]),
    "oflk_good_features_workspace": (ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "oflk_good_features": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [ctypes.c_float] * 2 + [ctypes.c_int, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "oflk_good_features_host": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + [ctypes.c_int, _i32p, _f32p, _f32p]),
    "oflk_good_features_host_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + [ctypes.c_int, _i32p, _f32p, _f32p]),
    "oflk_pyramidal_sequence_klt": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 6 + [ctypes.c_float] * 4 + [ctypes.c_int, _i32p, _f32p, _f32p, _f32p, _vp]),
    "oflk_pyramidal_sequence_klt_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [ctypes.c_float] * 4 + [ctypes.c_int, _i32p, _f32p, _f32p, _f32p, _vp]),
    "oflk_pyramidal_sequence_klt_replenish": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 6 + [ctypes.c_float] * 4 + [ctypes.c_int] * 2 + [_f32p, _vp, _vp, _i32p]),
    "oflk_pyramidal_sequence_klt_replenish_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [ctypes.c_float] * 4 + [ctypes.c_int] * 2 + [_f32p, _vp, _vp, _i32p]),
    "oflk_replenish_features_host": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_int] * 2 + [_f32p, _vp, _i32p, _f32p, _vp, _i32p]),
    "oflk_replenish_features_host_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_int] * 2 + [_f32p, _vp, _i32p, _f32p, _vp, _i32p]),
    "oflk_replenish_features_workspace": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "oflk_replenish_features": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + [ctypes.c_int] * 2 + [_vp, _vp, _vp, ctypes.c_size_t] + [_vp] * 5),
    "oflk_tracker_create": (ctypes.c_int, [ctypes.POINTER(_vp)] + [_I] * 4 + _TRACKING),
    "oflk_tracker_destroy": (ctypes.c_int, [_vp]),
    "oflk_tracker_reset": (ctypes.c_int, [_vp, _vp]),
    "oflk_tracker_workspace_bytes": (ctypes.c_size_t, [_vp]),
    "oflk_tracker_frame_index": (ctypes.c_int, [_vp]),
    "oflk_tracker_push_device": (ctypes.c_int, [_vp, _vp, _vp]),
    "oflk_tracker_row_device": (ctypes.c_int, [_vp] + [ctypes.POINTER(_vp)] * 6),
    "oflk_tracker_read_row": (ctypes.c_int, [_vp, _f32p, _vp, _vp, _i32p, _f32p, _i32p, _vp]),
    "oflk_tracker_push": (ctypes.c_int, [_vp, _vp, _f32p, _vp, _vp, _i32p, _f32p, _i32p]),
    "oflk_tracker_add_points": (ctypes.c_int, [_vp, _f32p, ctypes.c_int, _vp]),
    "oflk_motion_workspace": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_size_t)]),
    "oflk_estimate_motion": (ctypes.c_int, [_vp] * 3 + [_I] * 3 + _FIT + [_vp, _Z] + [_vp] * 4),
    "oflk_tracks_motion": (ctypes.c_int, [_vp] * 3 + [_I] * 3 + _FIT + [_vp, _Z] + [_vp] * 4),
    "oflk_estimate_motion_host": (ctypes.c_int, [_f32p, _f32p, _vp] + [_I] * 3 + _FIT + [_f32p, _vp, _i32p]),
    "oflk_homography_workspace": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_size_t)]),
    "oflk_estimate_homography": (ctypes.c_int, [_vp] * 3 + [_I] * 3 + _RANSAC + [_vp, _Z] + [_vp] * 4),
    "oflk_tracks_homography": (ctypes.c_int, [_vp] * 3 + [_I] * 3 + _RANSAC + [_vp, _Z] + [_vp] * 4),
    "oflk_estimate_homography_host": (ctypes.c_int, [_f32p, _f32p, _vp] + [_I] * 3 + _RANSAC + [_f32p, _vp, _i32p]),
    "oflk_tracker_set_motion": (ctypes.c_int, [_vp] + _FIT),
    "oflk_tracker_motion_device": (ctypes.c_int, [_vp] + [ctypes.POINTER(_vp)] * 3),
    "oflk_tracker_read_motion": (ctypes.c_int, [_vp, _f32p, _vp, _i32p, _vp]),
    "oflk_stabilize_trajectory": (ctypes.c_int, [_vp, _vp, _I] + _WINDOW + [_vp] * 4),
    "oflk_warp_affine": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp] * 4),
    "oflk_stabilize_trajectory_host": (ctypes.c_int, [_f32p, _i32p, _I] + _WINDOW + [_f32p, _f64p, _vp]),
    "oflk_warp_affine_host": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 3 + [_f64p, _f32p, _vp]),
    "oflk_warp_affine_host_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 3 + [_f64p, _vp, _vp]),
    "oflk_warp_perspective": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp] * 4),
    "oflk_warp_perspective_host": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 3 + [_f64p, _f32p, _vp]),
    "oflk_warp_perspective_host_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 3 + [_f64p, _vp, _vp]),
    "oflk_stabilize_sequence": (ctypes.c_int, [_f32p] + [_I] * 3 + _TRACKING + _FIT + _WINDOW + [_f32p] + _STAB_OUT),
    "oflk_stabilize_sequence_u8": (ctypes.c_int, [_vp] + [_I] * 3 + _TRACKING + _FIT + _WINDOW + [_vp] + _STAB_OUT),
    "oflk_mosaic_chain": (ctypes.c_int, [_vp, _vp] + [ctypes.c_int] * 4 + [ctypes.c_double] + [_vp] * 6),
    "oflk_mosaic_chain_host": (ctypes.c_int, [_f32p, _i32p] + [ctypes.c_int] * 4 + [ctypes.c_double, _f64p, _f64p, _f64p, _vp, _vp]),
    "oflk_mosaic_canvas": (ctypes.c_int, [_f64p, _vp, ctypes.c_int] + [_i32p] * 4),
    "oflk_mosaic_state_bytes": (ctypes.c_size_t, [ctypes.c_int] * 2),
    "oflk_mosaic_accumulate": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp, _vp] + [ctypes.c_int] * 5 + [_vp, ctypes.c_size_t, _vp]),
    "oflk_mosaic_resolve": (ctypes.c_int, [_vp] + [ctypes.c_int] * 3 + [_vp] * 3),
    "oflk_mosaic_composite_host": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 3 + [_f64p, _vp] + [ctypes.c_int] * 5 + [_f32p, _i32p]),
    "oflk_mosaic_composite_host_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 3 + [_f64p, _vp] + [ctypes.c_int] * 5 + [_vp, _i32p]),
    "oflk_mosaic_sequence": (ctypes.c_int, [_f32p] + [_I] * 3 + _TRACKING + _RANSAC + [_I, _D, _I, _f32p, _Z, _i32p, _i32p, _f64p, _vp, _vp, _f32p, _i32p]),
    "oflk_mosaic_sequence_u8": (ctypes.c_int, [_vp] + [_I] * 3 + _TRACKING + _RANSAC + [_I, _D, _I, _vp, _Z, _i32p, _i32p, _f64p, _vp, _vp, _f32p, _i32p]),
    "oflk_mosaic_accumulate_exposure": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp, _vp, _vp] + [ctypes.c_int] * 5 + [_vp, ctypes.c_size_t, _vp]),
    "oflk_mosaic_composite_exposure_host": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 3 + [_f64p, _vp, _f64p] + [ctypes.c_int] * 5 + [_f32p, _i32p]),
    "oflk_mosaic_composite_exposure_host_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 3 + [_f64p, _vp, _f64p] + [ctypes.c_int] * 5 + [_vp, _i32p]),
    "oflk_mosaic_median_capacity": (ctypes.c_int, []),
    "oflk_mosaic_median": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp, _vp, _vp] + [ctypes.c_int] * 4 + [_vp, _vp, _vp]),
    "oflk_mosaic_median_host": (ctypes.c_int, [_f32p] + [ctypes.c_int] * 3 + [_f64p, _vp, _f64p] + [ctypes.c_int] * 4 + [_f32p, _i32p]),
    "oflk_mosaic_median_host_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 3 + [_f64p, _vp, _f64p] + [ctypes.c_int] * 4 + [_vp, _i32p]),
    "oflk_exposure_chain_host": (ctypes.c_int, [_f32p, _i32p, ctypes.c_int, ctypes.c_int, _f64p]),
    "oflk_align_workspace": (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_size_t)]),
    "oflk_align_refine": (ctypes.c_int, [_vp, _vp, _I, _I] + _ALIGN + _ALIGN_D_IO + [_vp]),
    "oflk_align_sequence": (ctypes.c_int, [_vp, _I, _I] + _ALIGN + _ALIGN_D_IO + [_vp]),
    "oflk_align_refine_host": (ctypes.c_int, [_f32p, _f32p, _I] + _ALIGN + _ALIGN_H_IO),
    "oflk_align_refine_host_u8": (ctypes.c_int, [_vp, _vp, _I] + _ALIGN + _ALIGN_H_IO),
    "oflk_align_sequence_host": (ctypes.c_int, [_f32p, _I] + _ALIGN + _ALIGN_H_IO),
    "oflk_align_sequence_host_u8": (ctypes.c_int, [_vp, _I] + _ALIGN + _ALIGN_H_IO),
    "oflk_align_photo_workspace": (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_size_t)]),
    "oflk_align_refine_photo": (ctypes.c_int, [_vp, _vp, _I, _I] + _ALIGN + _ALIGN_D_IO + [_vp, _vp]),
    "oflk_align_sequence_photo": (ctypes.c_int, [_vp, _I, _I] + _ALIGN + _ALIGN_D_IO + [_vp, _vp]),
    "oflk_align_refine_photo_host": (ctypes.c_int, [_f32p, _f32p, _I] + _ALIGN + _ALIGN_H_IO + [_f32p]),
    "oflk_align_refine_photo_host_u8": (ctypes.c_int, [_vp, _vp, _I] + _ALIGN + _ALIGN_H_IO + [_f32p]),
    "oflk_align_sequence_photo_host": (ctypes.c_int, [_f32p, _I] + _ALIGN + _ALIGN_H_IO + [_f32p]),
    "oflk_align_sequence_photo_host_u8": (ctypes.c_int, [_vp, _I] + _ALIGN + _ALIGN_H_IO + [_f32p]),
    "oflk_align_robust_workspace": (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_size_t)]),
    "oflk_align_refine_robust": (ctypes.c_int, [_vp, _vp, _I, _I] + _ALIGN + _ROBUST + _ALIGN_D_IO + [_vp, _vp]),
    "oflk_align_sequence_robust": (ctypes.c_int, [_vp, _I, _I] + _ALIGN + _ROBUST + _ALIGN_D_IO + [_vp, _vp]),
    "oflk_align_refine_robust_host": (ctypes.c_int, [_f32p, _f32p, _I] + _ALIGN + _ROBUST + _ALIGN_H_IO + [_f32p]),
    "oflk_align_refine_robust_host_u8": (ctypes.c_int, [_vp, _vp, _I] + _ALIGN + _ROBUST + _ALIGN_H_IO + [_f32p]),
    "oflk_align_sequence_robust_host": (ctypes.c_int, [_f32p, _I] + _ALIGN + _ROBUST + _ALIGN_H_IO + [_f32p]),
    "oflk_align_sequence_robust_host_u8": (ctypes.c_int, [_vp, _I] + _ALIGN + _ROBUST + _ALIGN_H_IO + [_f32p]),
    "oflk_align_weights": (ctypes.c_int, [_vp, _vp] + [ctypes.c_int] * 5 + [ctypes.c_float, _vp, _vp, _vp, _vp]),
    "oflk_align_weights_host": (ctypes.c_int, [_f32p, _f32p] + [ctypes.c_int] * 4 + [ctypes.c_float, _f32p, _f32p, _f32p]),
    "oflk_align_weights_host_u8": (ctypes.c_int, [_vp, _vp] + [ctypes.c_int] * 4 + [ctypes.c_float, _f32p, _f32p, _f32p]),
    "oflk_stabilize_trajectory_ring": (ctypes.c_int, [_vp, _vp] + [_I] * 4 + _WINDOW + [_vp] * 3),
    "oflk_stabilizer_create": (ctypes.c_int, [ctypes.POINTER(_vp)] + [_I] * 4 + _TRACKING + _FIT + _WINDOW),
    "oflk_stabilizer_destroy": (ctypes.c_int, [_vp]),
    "oflk_stabilizer_reset": (ctypes.c_int, [_vp, _vp]),
    "oflk_stabilizer_workspace_bytes": (ctypes.c_size_t, [_vp]),
    "oflk_stabilizer_lag": (ctypes.c_int, [_vp]),
    "oflk_stabilizer_frame_index": (ctypes.c_int, [_vp]),
    "oflk_stabilizer_push_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32p, _vp]),
    "oflk_stabilizer_push": (ctypes.c_int, [_vp, _vp, _vp, _vp, _f32p, _i32p]),
    "oflk_stabilizer_flush_device": (ctypes.c_int, [_vp, _vp, _vp, _i32p, _i32p, _vp]),
    "oflk_stabilizer_flush": (ctypes.c_int, [_vp, _vp, _vp, _f32p, _i32p, _i32p]),
    "oflk_stabilizer_correction_device": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "oflk_stabilizer_tracker": (_vp, [_vp]),
    "oflk_luma_u8": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp, _vp]),
    "oflk_luma_u8_host": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp]),
    "oflk_warp_affine_packed": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp] * 4),
    "oflk_warp_perspective_packed": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp] * 4),
    "oflk_warp_affine_packed_host": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_f64p, _vp, _vp]),
    "oflk_warp_perspective_packed_host": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_f64p, _vp, _vp]),
    "oflk_stabilize_sequence_packed": (ctypes.c_int, [_vp] + [_I] * 5 + _TRACKING + _FIT + _WINDOW + [_vp] + _STAB_OUT),
    "oflk_stabilizer_create_packed": (ctypes.c_int, [ctypes.POINTER(_vp)] + [_I] * 5 + _TRACKING + _FIT + _WINDOW),
    "oflk_nv12_frame_bytes": (ctypes.c_size_t, [ctypes.c_int] * 2),
    "oflk_warp_affine_nv12": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp] * 4),
    "oflk_warp_perspective_nv12": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp] * 4),
    "oflk_warp_affine_nv12_host": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_f64p, _vp, _vp]),
    "oflk_warp_perspective_nv12_host": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_f64p, _vp, _vp]),
    "oflk_stabilize_sequence_nv12": (ctypes.c_int, [_vp] + [_I] * 4 + _TRACKING + _FIT + _WINDOW + [_vp] + _STAB_OUT),
    "oflk_stabilizer_create_nv12": (ctypes.c_int, [ctypes.POINTER(_vp)] + [_I] * 4 + _TRACKING + _FIT + _WINDOW),
    "oflk_shard_range": (None, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p, _i32p]),
    "oflk_single_scale_fp16": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, _f32p, _f32p]),
    "oflk_rtl_stream_length": (ctypes.c_long, [ctypes.c_int, ctypes.c_int]),
    "oflk_rtl_flow_u8": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "oflk_rtl_flow_u8_device": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "oflk_plan_single_scale_fp16": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_float, _vp]),
    "oflk_plan_resolve_uncertain": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32p]),
    "oflk_plan_resolve_uncertain_u8": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32p]),
    "oflk_last_resolved": (ctypes.c_int, []),
    "oflk_device_mean_error": (ctypes.c_double, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    "oflk_decision_guard": (ctypes.c_double, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "oflk_plan_read_uncertain": (ctypes.c_int, [_vp, _i32p, _vp]),
    "oflk_plan_read_level_flow": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _vp]),
    "oflk_pyramidal_last_level_flow": (ctypes.c_int, [ctypes.c_int] * 8 + [_f32p, _f32p]),
    "oflk_pyramidal_last_uncertain": (ctypes.c_int, [ctypes.c_int] * 6 + [_i32p]),
    "oflk_plan_read_log": (ctypes.c_int, [_vp, _f32p, _i32p, _vp]),
    "oflk_plan_set_profiling": (ctypes.c_int, [_vp, ctypes.c_int]),
    "oflk_plan_set_arithmetic": (ctypes.c_int, [_vp, ctypes.c_int]),
    "oflk_plan_set_kernels": (ctypes.c_int, [_vp, ctypes.c_int]),
    "oflk_multi_rehearsal": (ctypes.c_int, [ctypes.c_int]),
    "oflk_set_host_arithmetic": (ctypes.c_int, [ctypes.c_int]),
    "oflk_tolerant_relaxes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "oflk_plan_metrics": (ctypes.c_int, [_vp, _vp, _vp, _f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), _vp]),
    "oflk_flow_metrics": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "oflk_plan_kernel_times": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long), ctypes.c_int]),
}

_lib: Optional[ctypes.CDLL] = None


class OflkError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"liboflk error {code}: {message}")
        self.code = code


def lib() -> ctypes.CDLL:
    """Load liboflk.so once; raise loudly when it is not built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} not found: the HIP extension is not built. "
                "Run `python __graft_entry__.py` or `make -C optical-flow-fpga_amd/csrc`. "
                "There is no CPU fallback."
            )
        L = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if a declared symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
        # opt-in arithmetic of the host entry points (default: the reference's values): OFLK_ARITH=contracted | tolerant
        mode = {"": 0, "exact": 0, "contracted": 1, "tolerant": 2}.get(os.environ.get("OFLK_ARITH", "").strip().lower())
        if mode is None:
            raise ValueError(f"OFLK_ARITH={os.environ['OFLK_ARITH']!r}: expected exact, contracted or tolerant")
        if mode:
            check(L.oflk_set_host_arithmetic(mode))
    return _lib


def check(rc: int) -> None:
    if rc != OFLK_OK:
        msg = lib().oflk_last_error().decode("utf-8", "replace")
        if rc == OFLK_ERR_INVALID:
            raise ValueError(f"liboflk: {msg}")
        raise OflkError(rc, msg)


def version() -> str:
    return lib().oflk_version().decode()


def device_count() -> int:
    return int(lib().oflk_device_count())


def as_f32(a) -> np.ndarray:
    """What the reference's callers hand over: float32 [H, W]; convert anything else."""
    arr = np.ascontiguousarray(a, dtype=np.float32)
    if arr.ndim != 2:
        raise ValueError(f"expected a 2-D array, got shape {arr.shape}")
    return arr


def both_u8(a, b) -> bool:
    """True when both frames are 2-D uint8 arrays (the reference's .bin frame format)."""
    return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == np.uint8 and b.dtype == np.uint8
            and a.ndim == 2 and b.ndim == 2)


def ptr(a: np.ndarray):
    return a.ctypes.data_as(_f32p)


def pix(arr: np.ndarray):
    """the C pointer of a contiguous float32 or uint8 frame array"""
    return arr.ctypes.data if arr.dtype == np.uint8 else ptr(arr)


def pixels(arr: np.ndarray, name: str):
    """The one pixel-type dispatch: (pix(arr), the library's function `name`, `name`_u8 for a uint8 array)"""
    return pix(arr), getattr(lib(), name + ("_u8" if arr.dtype == np.uint8 else ""))


def as_sequence(frames) -> Tuple[np.ndarray, bool]:
    """Frames of a sequence -- a (T, H, W) array or a sequence of 2-D arrays -- as one contiguous (T, H, W) array: uint8
    when every frame is uint8 (True is returned), float32 otherwise.  ValueError for T < 2, frames that are not 2-D, mixed
    shapes or mixed dtypes; nothing here touches a device."""
    if isinstance(frames, np.ndarray):
        if frames.ndim != 3:
            raise ValueError(f"expected a (T, H, W) array of frames, got shape {frames.shape}")
        items = list(frames)
    else:
        items = [np.asarray(f) for f in frames]
        for f in items:
            if f.ndim != 2:
                raise ValueError(f"every frame must be a 2-D array, got shape {f.shape}")
        if items and len({f.shape for f in items}) > 1:
            raise ValueError(f"frames of mixed shapes: {sorted({f.shape for f in items})}")
        if items and len({f.dtype for f in items}) > 1:
            raise ValueError(f"frames of mixed dtypes: {sorted(str(d) for d in {f.dtype for f in items})}")
    if len(items) < 2:
        raise ValueError(f"a sequence needs at least 2 frames, got {len(items)}")
    u8 = items[0].dtype == np.uint8
    arr = np.ascontiguousarray(frames if isinstance(frames, np.ndarray) else np.stack(items), dtype=np.uint8 if u8 else np.float32)
    if arr.shape[1] < 1 or arr.shape[2] < 1:
        raise ValueError(f"empty frames: shape {arr.shape}")
    return arr, u8


def same_shape(*arrs: np.ndarray) -> Tuple[int, int]:
    s = arrs[0].shape
    for a in arrs[1:]:
        if a.shape != s:
            raise ValueError(f"shape mismatch: {s} vs {a.shape}")
    return int(s[0]), int(s[1])


class Plan:
    """Device-resident plan (oflk_plan_*): B pairs of H x W, pointers are raw
    device addresses (e.g. torch.Tensor.data_ptr()), stream a hipStream_t handle."""

    def __init__(self, device: int, B: int, H: int, W: int, levels: int = 3, window_size: int = 5,
                 iters: int = 3):
        self._h = _vp()
        self.B, self.H, self.W, self.levels, self.window_size, self.iters = B, H, W, levels, window_size, iters
        check(lib().oflk_plan_create(ctypes.byref(self._h), device, B, H, W, levels, window_size, iters))

    def close(self) -> None:
        if self._h:
            lib().oflk_plan_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return int(lib().oflk_plan_workspace_bytes(self._h))

    def single_scale(self, d_prev: int, d_curr: int, d_u: int, d_v: int, stream: int = 0) -> None:
        check(lib().oflk_plan_single_scale(self._h, d_prev, d_curr, d_u, d_v, stream))

    def pyramidal(self, d_prev: int, d_curr: int, d_u: int, d_v: int, stream: int = 0) -> None:
        check(lib().oflk_plan_pyramidal(self._h, d_prev, d_curr, d_u, d_v, stream))

    def pyramidal_sequence(self, d_frames: int, d_u: int, d_v: int, stream: int = 0, u8: bool = False) -> None:
        """d_frames: device frames [B+1][H][W] (float32, or uint8 with u8=True); flow b (frames b -> b+1) into d_u, d_v
        [B][H][W].  Resolve flagged pairs with resolve_uncertain(d_frames, d_frames + H*W * itemsize, ...)."""
        fn = lib().oflk_plan_pyramidal_sequence_u8 if u8 else lib().oflk_plan_pyramidal_sequence
        check(fn(self._h, d_frames, d_u, d_v, stream))

    def pyramidal_sequence_fb(self, d_frames: int, d_uf: int, d_vf: int, d_ub: int, d_vb: int, stream: int = 0,
                              u8: bool = False) -> None:
        """Both directions on one pyramid: flow b (frames b -> b+1) into d_uf, d_vf and (frames b+1 -> b) into d_ub, d_vb, all
        [B][H][W].  Resolve flagged pairs with resolve_uncertain_sequence_fb, then run fb_consistency."""
        fn = lib().oflk_plan_pyramidal_sequence_fb_u8 if u8 else lib().oflk_plan_pyramidal_sequence_fb
        check(fn(self._h, d_frames, d_uf, d_vf, d_ub, d_vb, stream))

    def read_log_backward(self, stream: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """read_log of the backward pass of the last pyramidal_sequence_fb call."""
        log = np.zeros((self.B, self.levels, max(self.iters, 1), 2), np.float32)
        runs = np.zeros((self.B, self.levels), np.int32)
        check(lib().oflk_plan_read_log_backward(self._h, ptr(log), runs.ctypes.data_as(_i32p), stream))
        return log, runs

    def read_uncertain_backward(self, stream: int = 0) -> np.ndarray:
        """read_uncertain of the backward pass of the last pyramidal_sequence_fb call."""
        m = np.zeros((self.B, self.levels), np.int32)
        check(lib().oflk_plan_read_uncertain_backward(self._h, m.ctypes.data_as(_i32p), stream))
        return m

    def resolve_uncertain_sequence_fb(self, d_frames: int, d_uf: int, d_vf: int, d_ub: int, d_vb: int, stream: int = 0,
                                      u8: bool = False) -> int:
        """Redo the flagged pairs of both directions of the last pyramidal_sequence_fb call; returns how many (both)."""
        n = ctypes.c_int(0)
        fn = lib().oflk_plan_resolve_uncertain_sequence_fb_u8 if u8 else lib().oflk_plan_resolve_uncertain_sequence_fb
        check(fn(self._h, d_frames, d_uf, d_vf, d_ub, d_vb, stream, ctypes.byref(n)))
        return int(n.value)

    def single_scale_fp16(self, d_prev: int, d_curr: int, d_u: int, d_v: int, pixel_max: float = 255.0, stream: int = 0) -> None:
        """BASELINE config 5: fp16 gradients / accumulators (opt-in, approximate)."""
        check(lib().oflk_plan_single_scale_fp16(self._h, d_prev, d_curr, d_u, d_v, float(pixel_max), stream))

    def single_scale_u8(self, d_prev: int, d_curr: int, d_u: int, d_v: int, stream: int = 0) -> None:
        """d_prev / d_curr: device uint8 frames [B][H][W] (read by the kernels as they are)."""
        check(lib().oflk_plan_single_scale_u8(self._h, d_prev, d_curr, d_u, d_v, stream))

    def pyramidal_u8(self, d_prev: int, d_curr: int, d_u: int, d_v: int, stream: int = 0) -> None:
        check(lib().oflk_plan_pyramidal_u8(self._h, d_prev, d_curr, d_u, d_v, stream))

    def read_log(self, stream: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        log = np.zeros((self.B, self.levels, max(self.iters, 1), 2), np.float32)
        runs = np.zeros((self.B, self.levels), np.int32)
        check(lib().oflk_plan_read_log(self._h, ptr(log), runs.ctypes.data_as(_i32p), stream))
        return log, runs

    def read_uncertain(self, stream: int = 0) -> np.ndarray:
        """[B][levels] bit masks: bit k = exit decision after iteration k taken within the level's band around the threshold
        (oflk_decision_guard: at least 5e-5 relative)."""
        m = np.zeros((self.B, self.levels), np.int32)
        check(lib().oflk_plan_read_uncertain(self._h, m.ctypes.data_as(_i32p), stream))
        return m

    def resolve_uncertain(self, d_prev: int, d_curr: int, d_u: int, d_v: int, stream: int = 0, u8: bool = False) -> int:
        """Redo the pairs whose exit decisions were flagged, in NumPy's summation order; returns how many."""
        n = ctypes.c_int(0)
        fn = lib().oflk_plan_resolve_uncertain_u8 if u8 else lib().oflk_plan_resolve_uncertain
        check(fn(self._h, d_prev, d_curr, d_u, d_v, stream, ctypes.byref(n)))
        return int(n.value)

    def read_level_flow(self, level: int, pair: int, shape, stream: int = 0):
        u = np.empty(shape, np.float32)
        v = np.empty(shape, np.float32)
        check(lib().oflk_plan_read_level_flow(self._h, int(level), int(pair), ptr(u), ptr(v), stream))
        return u, v

    def metrics(self, d_u: int, d_v: int, u_true, v_true, region, stream: int = 0) -> np.ndarray:
        """[B][5] = mae_u, mae_v, rmse, epe, aae of device-resident flows over mask[y0:y1, x0:x1]."""
        ut = np.ascontiguousarray(u_true, np.float32).reshape(self.B)
        vt = np.ascontiguousarray(v_true, np.float32).reshape(self.B)
        out = np.zeros((self.B, 5), np.float64)
        y0, y1, x0, x1 = (int(r) for r in region)
        check(lib().oflk_plan_metrics(self._h, d_u, d_v, ptr(ut), ptr(vt), y0, y1, x0, x1,
                                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), stream))
        return out

    def set_arithmetic(self, mode: int) -> None:
        """0 = exact (default: the reference's values), 1 = contracted (opt-in: fused multiply-adds in the Gaussian pyramid)."""
        check(lib().oflk_plan_set_arithmetic(self._h, int(mode)))

    def set_kernels(self, choice: int) -> None:
        """0: automatic (5x5 single-scale streams when the launch is large enough; doubtful tiles redone in NumPy's order);
        1: the tile kernel throughout; 2: the streaming kernel whenever the window is 5x5"""
        check(lib().oflk_plan_set_kernels(self._h, int(choice)))

    def set_profiling(self, enabled) -> None:
        """False/0 off, True/1 every kernel, 2 only the dominant kernel (finest-level LK iteration)."""
        check(lib().oflk_plan_set_profiling(self._h, int(enabled)))

    def kernel_times(self) -> dict:
        n = 32
        names = (ctypes.c_char_p * n)()
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_long * n)()
        k = lib().oflk_plan_kernel_times(self._h, names, ms, cnt, n)
        if k < 0:
            check(k)
        return {names[i].decode(): {"total_ms": ms[i], "launches": cnt[i]} for i in range(k)}


def check_int(name: str, v, lo: int, hi: Optional[int] = None, what: Optional[str] = None) -> int:
    """v as an int; ValueError "`name` must be an integer `what`, got v" unless v is integral (not a bool) and in [lo, hi].
    what defaults to ">= lo", or "in [lo, hi]" with hi."""
    if isinstance(v, bool) or int(v) != v or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(f"{name} must be an integer {what or (f'>= {lo}' if hi is None else f'in [{lo}, {hi}]')}, got {v!r}")
    return int(v)


def check_fb_params(alpha: float, beta: float) -> Tuple[float, float]:
    """alpha, beta of the forward-backward test as float32; ValueError unless both are finite and >= 0."""
    with np.errstate(over="ignore"):   # a value beyond float32's range becomes inf, and is refused below
        a, b = np.float32(alpha), np.float32(beta)
    if not (np.isfinite(a) and a >= 0 and np.isfinite(b) and b >= 0):
        raise ValueError(f"alpha and beta must be finite and >= 0, got {alpha!r}, {beta!r}")
    return float(a), float(b)


def fb_consistency(d_uf: int, d_vf: int, d_ub: int, d_vb: int, B: int, H: int, W: int, alpha: float = 0.01, beta: float = 0.5,
                   d_err_f: int = 0, d_err_b: int = 0, d_valid_f: int = 0, d_valid_b: int = 0, stream: int = 0) -> None:
    """oflk_fb_consistency on device pointers ([B][H][W]; err float32, valid uint8); 0 leaves an output out (not all four)."""
    check(lib().oflk_fb_consistency(d_uf, d_vf, d_ub, d_vb, int(B), int(H), int(W), float(alpha), float(beta),
                                    d_err_f or None, d_err_b or None, d_valid_f or None, d_valid_b or None, stream))


INTERP_MAX_TAUS = 16   # OFLK_INTERP_MAX_TAUS


class Interp(NamedTuple):
    """The settings of the interpolation calls, in the argument order of the C ABI (InterpConfig); taus is kept alive here"""
    alpha: float
    beta: float
    refine: int
    taus: np.ndarray   # float64 (n,)

    def args(self):
        return self.alpha, self.beta, self.refine, _f64(self.taus), len(self.taus)


def check_interp(alpha: float, beta: float, refine, taus, factor=None) -> Interp:
    """The interpolation settings as the library takes them.  taus None: factor = k >= 2 stands for j / k, j = 1 .. k-1,
    formed in float64.  ValueError for alpha, beta as check_fb_params, a refine outside [1, 8], a factor that is not an
    integer in [2, INTERP_MAX_TAUS + 1], taus that are not 1 .. INTERP_MAX_TAUS finite values strictly between 0 and 1."""
    a, b = check_fb_params(alpha, beta)
    refine = check_int("refine", refine, 1, 8)
    if taus is None:
        k = check_int("factor", factor, 2, INTERP_MAX_TAUS + 1)
        taus = np.arange(1, k, dtype=np.float64) / np.float64(k)
    t = np.ascontiguousarray(taus, np.float64)
    if t.ndim != 1 or not 1 <= t.size <= INTERP_MAX_TAUS:
        raise ValueError(f"taus must be 1 to {INTERP_MAX_TAUS} values, got shape {t.shape}")
    if not np.all(np.isfinite(t) & (t > 0) & (t < 1)):
        raise ValueError(f"every tau must be finite and strictly between 0 and 1, got {t.tolist()!r}")
    return Interp(a, b, refine, t)


def interpolate_frames(d_frames: int, B: int, H: int, W: int, d_uf: int, d_vf: int, d_ub: int, d_vb: int, taus, d_out: int,
                       d_status: int = 0, alpha: float = 0.01, beta: float = 0.5, refine: int = 2, u8: bool = False,
                       stream: int = 0) -> None:
    """oflk_interpolate_frames on device pointers: frames [B+1][H][W] (uint8 with u8), flows [B][H][W], the in-between frames
    of the times taus into d_out [B][n][H][W] of the frames' type and d_status [B][n][H][W] uint8 (0: no status)."""
    cfg = check_interp(alpha, beta, refine, taus)
    check(lib().oflk_interpolate_frames(d_frames, int(bool(u8)), int(B), int(H), int(W), d_uf, d_vf, d_ub, d_vb, *cfg.args(),
                                        d_out, d_status or None, stream))


def interpolate_frames_layout(layout: "FrameLayout", d_frames: int, B: int, H: int, W: int, d_uf: int, d_vf: int, d_ub: int,
                              d_vb: int, taus, d_out: int, d_status: int = 0, alpha: float = 0.01, beta: float = 0.5,
                              refine: int = 2, stream: int = 0) -> None:
    """oflk_interpolate_frames_packed (layout ("_packed", (channels,))) or oflk_interpolate_frames_nv12 (("_nv12", (siting,)))
    on device pointers: uint8 frames [B+1] and d_out [B][n] of the layout's frames, flows [B][H][W], d_status [B][n][H][W]
    (0: no status); asynchronous."""
    cfg = check_interp(alpha, beta, refine, taus)
    fn = getattr(lib(), "oflk_interpolate_frames" + layout.suffix)
    check(fn(d_frames or None, int(B), int(H), int(W), int(layout.args[0]), d_uf or None, d_vf or None, d_ub or None, d_vb or None,
             *cfg.args(), d_out or None, d_status or None, stream))


def interpolate_host(layout: "FrameLayout", arr: np.ndarray, H: int, W: int, flows, cfg: Interp, status: bool):
    """oflk_interpolate_frames_host[_u8] (the default layout) or oflk_interpolate_frames{_packed,_nv12}_host on a contiguous
    array of B+1 frames of the layout and four float32 flows (B, H, W): (new (B, n) + the frame's shape, status (B, n, H, W)
    or None)"""
    B, n = arr.shape[0] - 1, len(cfg.taus)
    flows = [np.ascontiguousarray(f, np.float32) for f in flows]
    for f in flows:
        if f.shape != (B, H, W):
            raise ValueError(f"every flow must have shape {(B, H, W)}, got {f.shape}")
    new = np.empty((B, n) + arr.shape[1:], arr.dtype)
    st = np.empty((B, n, H, W), np.uint8) if status else None
    if layout.suffix:
        src, fn = arr.ctypes.data, getattr(lib(), "oflk_interpolate_frames" + layout.suffix + "_host")
    else:
        src, fn = pixels(arr, "oflk_interpolate_frames_host")
    check(fn(src, B, H, W, *layout.args[:1], *(ptr(f) for f in flows), *cfg.args(), pix(new), None if st is None else st.ctypes.data))
    return new, st


def interpolate_sequence_host(layout: "FrameLayout", arr: np.ndarray, H: int, W: int, levels: int, window_size: int, iters: int,
                              cfg: Interp, flow_median: int = 0):
    """oflk_interpolate_sequence[_u8] (the default layout) or oflk_interpolate_sequence{_packed,_nv12} on a contiguous array
    of T frames of the layout: (new (T-1, n) + the frame's shape, status (T-1, n, H, W)).  flow_median (checked: 0, 3, 5, 7 or
    9) other than 0: the _median form of that call"""
    T, n = arr.shape[0], len(cfg.taus)
    new, st = np.empty((T - 1, n) + arr.shape[1:], arr.dtype), np.empty((T - 1, n, H, W), np.uint8)
    median = "_median" if flow_median else ""
    if layout.suffix:
        src, fn = arr.ctypes.data, getattr(lib(), "oflk_interpolate_sequence" + layout.suffix + median)
    else:
        src, fn = pixels(arr, "oflk_interpolate_sequence" + median)
    check(fn(src, T, H, W, *layout.args, int(levels), int(window_size), int(iters), *cfg.args(), *((flow_median,) if flow_median else ()),
             pix(new), st.ctypes.data))
    return new, st


FLOW_MEDIAN_SIZES = (3, 5, 7, 9)


def check_flow_median(flow_median) -> int:
    """the flow_median setting of the sequence calls as an int: 0 (off) or a window of FLOW_MEDIAN_SIZES; ValueError otherwise"""
    if isinstance(flow_median, bool) or not isinstance(flow_median, (int, np.integer)) or int(flow_median) not in (0,) + FLOW_MEDIAN_SIZES:
        raise ValueError(f"flow_median must be 0, 3, 5, 7 or 9, got {flow_median!r}")
    return int(flow_median)


def flow_median_tile() -> Tuple[int, int]:
    """oflk_flow_median_tile (host only): the (rows, columns) of output pixels of one block of oflk_flow_median"""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().oflk_flow_median_tile(ctypes.byref(th), ctypes.byref(tw)))
    return th.value, tw.value


def flow_median(d_in: int, d_out: int, P: int, H: int, W: int, size: int = 5, stream: int = 0) -> None:
    """oflk_flow_median on device pointers: the size x size median of each of the P planes d_in [P][H][W] float32 into d_out
    (not d_in); asynchronous."""
    check(lib().oflk_flow_median(d_in or None, d_out or None, int(P), int(H), int(W), int(size), stream))


def flow_median_host(planes: np.ndarray, size: int = 5) -> np.ndarray:
    """oflk_flow_median_host on a float32 array (..., H, W): every plane's size x size median, the same shape"""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or int(size) not in FLOW_MEDIAN_SIZES:
        raise ValueError(f"size must be 3, 5, 7 or 9, got {size!r}")
    a = np.ascontiguousarray(planes, np.float32)
    if a.ndim < 2 or a.size == 0:
        raise ValueError(f"expected a non-empty (..., H, W) array of flow planes, got shape {a.shape}")
    H, W = a.shape[-2:]
    out = np.empty_like(a)
    check(lib().oflk_flow_median_host(ptr(a), ptr(out), a.size // (H * W), H, W, int(size)))
    return out


DENOISE_MAX_RADIUS = 4   # OFLK_DENOISE_MAX_RADIUS


class Denoise(NamedTuple):
    """The settings of the denoising calls, in the argument order of the C ABI (DenoiseConfig, flow_median between the
    test's parameters and the rest in the sequence forms)"""
    alpha: float
    beta: float
    radius: int
    strength: float


def check_denoise(alpha: float, beta: float, radius, strength) -> Denoise:
    """The denoising settings as the library takes them.  ValueError for alpha, beta as check_fb_params, a radius that is
    not an integer in [1, DENOISE_MAX_RADIUS], a strength that is not finite and > 0 as a float32."""
    a, b = check_fb_params(alpha, beta)
    radius = check_int("radius", radius, 1, DENOISE_MAX_RADIUS)
    with np.errstate(over="ignore"):   # a value beyond float32's range becomes inf, and is refused below
        s = np.float32(strength)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"strength must be finite and > 0, got {strength!r}")
    return Denoise(a, b, radius, float(s))


def denoise_host(arr: np.ndarray, flows, cfg: Denoise, count: bool):
    """oflk_denoise_frames_host[_u8] on a contiguous (B+1, H, W) array of frames and four float32 flows (B, H, W): (out of the
    frames' shape and type, count (B+1, H, W) uint8 or None)"""
    B, H, W = arr.shape[0] - 1, arr.shape[1], arr.shape[2]
    flows = [np.ascontiguousarray(f, np.float32) for f in flows]
    for f in flows:
        if f.shape != (B, H, W):
            raise ValueError(f"every flow must have shape {(B, H, W)}, got {f.shape}")
    out = np.empty_like(arr)
    cnt = np.empty(arr.shape, np.uint8) if count else None
    src, fn = pixels(arr, "oflk_denoise_frames_host")
    check(fn(src, B, H, W, *(ptr(f) for f in flows), *cfg, pix(out), None if cnt is None else cnt.ctypes.data))
    return out, cnt


def denoise_sequence_host(arr: np.ndarray, levels: int, window_size: int, iters: int, cfg: Denoise, flow_median: int, count: bool):
    """oflk_denoise_sequence[_u8] on a contiguous (T, H, W) array of frames; flow_median is checked (0, 3, 5, 7 or 9): (out of
    the frames' shape and type, count (T, H, W) uint8 or None)"""
    T, H, W = arr.shape
    out = np.empty_like(arr)
    cnt = np.empty(arr.shape, np.uint8) if count else None
    src, fn = pixels(arr, "oflk_denoise_sequence")
    check(fn(src, T, H, W, int(levels), int(window_size), int(iters), cfg.alpha, cfg.beta, int(flow_median), cfg.radius, cfg.strength,
             pix(out), None if cnt is None else cnt.ctypes.data))
    return out, cnt


def as_queries(queries, T: int) -> Tuple[Optional[np.ndarray], np.ndarray]:
    """Track queries as the C ABI takes them: (qt, qxy) with qt int32 (N,) frame indices in [0, T-1] (None for (N, 2)
    queries: every one at frame 0) and qxy float32 (N, 2) (x, y).  queries: (N, 3) (t, x, y) or (N, 2) (x, y), N >= 1.
    ValueError otherwise; nothing here touches a device."""
    q = np.asarray(queries)
    if q.ndim != 2 or q.shape[1] not in (2, 3) or q.shape[0] < 1:
        raise ValueError(f"queries must be an (N, 3) (t, x, y) or (N, 2) (x, y) array with N >= 1, got shape {q.shape}")
    if q.shape[1] == 2:
        return None, np.ascontiguousarray(q, np.float32)
    t = q[:, 0]
    if not np.all(np.isfinite(t)) or not np.array_equal(t, np.floor(t)) or t.min() < 0 or t.max() > T - 1:
        raise ValueError(f"query frames must be integers in [0, {T - 1}]")
    return np.ascontiguousarray(t, np.int32), np.ascontiguousarray(q[:, 1:], np.float32)


def track_points(d_uf: int, d_vf: int, d_ub: int, d_vb: int, B: int, H: int, W: int, d_qxy: int, N: int, d_tracks: int,
                 d_visible: int, alpha: float = 0.01, beta: float = 0.5, t0: int = 0, d_qt: int = 0, stream: int = 0) -> None:
    """oflk_track_points on device pointers: flows [B][H][W] of pairs t0 .. t0+B-1, queries d_qxy [N][2] float32 (x, y) and
    d_qt [N] int32 (0: every query at frame 0), rows of frames t0 .. t0+B into d_tracks [B+1][N][2] float32 and d_visible
    [B+1][N] uint8 (row 0 is read for queries of an earlier frame: the previous call's last row)."""
    check(lib().oflk_track_points(d_uf, d_vf, d_ub, d_vb, int(B), int(H), int(W), float(alpha), float(beta), int(t0),
                                  d_qt or None, d_qxy, int(N), d_tracks, d_visible, stream))


CORNER_WINDOWS = (3, 5, 7, 9, 11)


def check_sparse_params(shape, num_levels, window_size, num_iterations, max_residual: float = 0.0) -> Tuple[int, int, int, float]:
    """The sparse tracker's configuration as the C ABI takes it: (levels, window, iterations, max_residual as float32).
    ValueError unless levels >= 1, iterations >= 1, the window is odd in [3, 11], every pyramid level of `shape` = (H, W)
    is at least 2 x 2 and max_residual is >= 0 (inf allowed: no residual test).  Nothing here touches a device."""
    check_int("num_levels", num_levels, 1)
    check_int("num_iterations", num_iterations, 1)
    if window_size not in CORNER_WINDOWS:
        raise ValueError(f"window_size must be one of {CORNER_WINDOWS}, got {window_size!r}")
    h, w = int(shape[0]), int(shape[1])
    for l in range(int(num_levels) - 1, -1, -1):
        if h < 2 or w < 2:
            raise ValueError(f"pyramid level {l} of {shape[0]} x {shape[1]} frames would be {h} x {w}: the sparse tracker needs 2 x 2")
        h, w = int(h * 0.5), int(w * 0.5)
    with np.errstate(over="ignore"):
        r = np.float32(max_residual)
    if not r >= 0:
        raise ValueError(f"max_residual must be >= 0 (inf: no residual test), got {max_residual!r}")
    return int(num_levels), int(window_size), int(num_iterations), float(r)


def sparse_tracks(plan: "Plan", d_frames: int, d_qxy: int, N: int, d_tracks: int, d_visible: int, alpha: float = 0.01,
                  beta: float = 0.5, max_residual: float = 4.0, t0: int = 0, d_qt: int = 0, u8: bool = False,
                  stream: int = 0) -> None:
    """oflk_plan_sparse_tracks on device pointers: d_frames [B+1][H][W] (float32, or uint8 with u8) are frames t0 .. t0+B of
    the plan's B pairs; queries, rows and row 0 as track_points.  No flow field is computed or stored."""
    check(lib().oflk_plan_sparse_tracks(plan._h, d_frames, int(bool(u8)), float(alpha), float(beta), float(max_residual), int(t0),
                                        d_qt or None, d_qxy, int(N), d_tracks, d_visible, stream))


def sparse_klt_replenish(plan: "Plan", d_frames: int, d_workspace: int, workspace_bytes: int, d_qt: int, d_qxy: int,
                         d_tracks: int, d_visible: int, d_born: int, d_detected: int, max_corners: int, detect_every: int,
                         quality_level: float = 0.01, min_distance: float = 10.0, alpha: float = 0.01, beta: float = 0.5,
                         max_residual: float = 4.0, t0: int = 0, d_residual: int = 0, u8: bool = False, stream: int = 0) -> None:
    """oflk_plan_sparse_klt_replenish on device pointers: d_frames [B+1][H][W] (float32, or uint8 with u8) are frames
    t0 .. t0+B of the plan's B pairs; K = max_corners slots in d_qt [K] int32 / d_qxy [K][2]; rows into d_tracks [B+1][K][2],
    d_visible, d_born [B+1][K] uint8, d_detected [B+1] int32 and d_residual [B+1][K] float32 (0: none).  t0 > 0 continues
    from the previous call's d_qt, d_qxy and last row (this call's row 0).  d_workspace of at least
    replenish_features_workspace bytes."""
    check(lib().oflk_plan_sparse_klt_replenish(plan._h, d_frames, int(bool(u8)), float(alpha), float(beta), float(max_residual),
                                               float(quality_level), float(min_distance), int(max_corners), int(detect_every),
                                               int(t0), d_workspace or None, int(workspace_bytes), d_qt or None, d_qxy or None,
                                               d_tracks or None, d_visible or None, d_born or None, d_detected or None,
                                               d_residual or None, stream))


def check_feature_params(max_corners, quality_level: float, min_distance: float, window_size: int) -> Tuple[int, float, float, int]:
    """The detection parameters as the C ABI takes them: (K, q, md, window) with q, md float32; ValueError unless K >= 1,
    q in [0, 1], md finite and >= 0 and the window odd in [3, 11].  Nothing here touches a device."""
    check_int("max_corners", max_corners, 1)
    with np.errstate(over="ignore"):
        q, md = np.float32(quality_level), np.float32(min_distance)
    if not (np.isfinite(q) and 0 <= q <= 1):
        raise ValueError(f"quality_level must be in [0, 1], got {quality_level!r}")
    if not (np.isfinite(md) and md >= 0):
        raise ValueError(f"min_distance must be finite and >= 0, got {min_distance!r}")
    if window_size not in CORNER_WINDOWS:
        raise ValueError(f"window_size must be one of {CORNER_WINDOWS}, got {window_size!r}")
    return int(max_corners), float(q), float(md), int(window_size)


DETECT_EVERY_MAX = 2 ** 31 - 1


def check_detect_every(detect_every, lo: int = 1) -> int:
    """detect_every as the C int: an integer >= lo (1 for the sequence calls, 0 -- never detect -- for the online ones),
    clamped to DETECT_EVERY_MAX, which no sequence reaches; ValueError otherwise"""
    return min(check_int("detect_every", detect_every, lo), DETECT_EVERY_MAX)


class Tracking(NamedTuple):
    """The sparse tracker's settings, checked, in the field order of the C side's KltConfig, then detect_every: the record
    is the run of arguments that every C call which takes them takes (`*tracking`; .klt for a call without detect_every,
    whose record says DETECT_EVERY_MAX: it detects on frame 0 alone)."""
    levels: int
    window_size: int
    iters: int
    alpha: float
    beta: float
    max_residual: float
    quality_level: float
    min_distance: float
    max_corners: int
    detect_every: int = DETECT_EVERY_MAX   # a call that takes none detects on frame 0 alone, which is what this value says

    @property
    def klt(self) -> tuple:
        return self[:9]


def check_tracking(shape, num_levels, window_size, num_iterations, alpha, beta, max_residual, max_corners, quality_level,
                   min_distance, detect_every=None, min_every: int = 1) -> Tracking:
    """The Tracking record of a caller's arguments, refused in this order: check_fb_params, check_sparse_params for frames
    of `shape` = (H, W), check_feature_params, check_detect_every (detect_every None: the call takes none).  A caller that
    parses its frames between the first two calls check_fb_params itself before it does: the order is the caller's."""
    a, b = check_fb_params(alpha, beta)
    L, win, it, r = check_sparse_params(shape, num_levels, window_size, num_iterations, max_residual)
    K, q, md, win = check_feature_params(max_corners, quality_level, min_distance, win)
    return Tracking(L, win, it, a, b, r, q, md, K, *(() if detect_every is None else (check_detect_every(detect_every, min_every),)))


class Fit(NamedTuple):
    """The RANSAC fit's settings, checked (check_motion_params), in the field order of the C side's FitConfig: `*fit` is
    the run of C arguments; .ransac the run of the homography calls, which take no model (check_ransac_params gives it)."""
    model: int
    hypotheses: int
    threshold: float
    seed: int

    @property
    def ransac(self) -> tuple:
        return self[1:]


class Window(NamedTuple):
    """The trajectory filter's window (check_window), as the C side's TrajWindow: .args is the run of C arguments"""
    weights: np.ndarray   # radius + 1 float64, contiguous
    radius: int

    @property
    def args(self) -> tuple:
        return _f64(self.weights), self.radius


def check_window(radius, sigma=None) -> Window:
    """the Window of stabilize_weights(radius, sigma), with its ValueErrors"""
    w = stabilize_weights(radius, sigma)
    return Window(w, int(w.size) - 1)


def check_refine(refine_iterations, refine_photometric=False, refine_robust_delta=None) -> int:
    """refine_iterations of the stabilise and mosaic calls as an int >= 0; ValueError for anything else, or for
    refine_photometric or refine_robust_delta without it"""
    n = check_int("refine_iterations", refine_iterations, 0)
    if refine_photometric and n == 0:
        raise ValueError("refine_photometric needs refine_iterations > 0")
    if refine_robust_delta is not None and n == 0:
        raise ValueError("refine_robust_delta needs refine_iterations > 0")
    return n


class FrameLayout(NamedTuple):
    """How a frame lies in memory, as the C side's FrameLayout: planes of one value per pixel (the default), interleaved
    colour ("_packed", args (channels, order)) or NV12 ("_nv12", args (siting,)).  suffix names the form of
    oflk_stabilize_sequence* / oflk_stabilizer_create*, args is what that form takes behind H and W."""
    suffix: str = ""
    args: tuple = ()

    def frame_shape(self, H: int, W: int) -> tuple:
        """the shape of one H x W frame's array"""
        if self.suffix == "_nv12":
            return (3 * H // 2, W)
        return (H, W, self.args[0]) if self.suffix else (H, W)


def as_frames(frames) -> Tuple[np.ndarray, bool]:
    """One frame (H, W) or a batch (F, H, W) (an array or a sequence of 2-D arrays) as a contiguous (F, H, W) array: uint8
    when every frame is uint8 (True is returned), float32 otherwise.  ValueError for anything else; no device call."""
    if isinstance(frames, np.ndarray) and frames.ndim == 2:
        frames = frames[None]
    if isinstance(frames, np.ndarray):
        if frames.ndim != 3:
            raise ValueError(f"expected an (H, W) frame or an (F, H, W) batch, got shape {frames.shape}")
        items = list(frames)
    else:
        items = [np.asarray(f) for f in frames]
        if any(f.ndim != 2 for f in items) or len({f.shape for f in items}) > 1:
            raise ValueError("expected 2-D frames of one shape")
    if not items or items[0].shape[0] < 1 or items[0].shape[1] < 1:
        raise ValueError("no frames, or empty frames")
    u8 = all(f.dtype == np.uint8 for f in items)
    arr = np.ascontiguousarray(frames if isinstance(frames, np.ndarray) else np.stack(items), dtype=np.uint8 if u8 else np.float32)
    return arr, u8


def corner_score(d_frames: int, F: int, H: int, W: int, d_score: int, window_size: int = 5, u8: bool = False,
                 stream: int = 0) -> None:
    """oflk_corner_score on device pointers: frames [F][H][W] (float32, or uint8 with u8) -> d_score [F][H][W] float32."""
    check(lib().oflk_corner_score(d_frames, int(bool(u8)), int(F), int(H), int(W), int(window_size), d_score, stream))


def good_features_workspace(F: int, H: int, W: int, window_size: int = 5, min_distance: float = 10.0,
                            max_corners: int = 100) -> int:
    """bytes of oflk_good_features' workspace for this shape"""
    n = ctypes.c_size_t(0)
    check(lib().oflk_good_features_workspace(int(F), int(H), int(W), int(window_size), float(min_distance), int(max_corners),
                                             ctypes.byref(n)))
    return int(n.value)


def good_features(d_frames: int, F: int, H: int, W: int, d_workspace: int, workspace_bytes: int, d_count: int, d_xy: int,
                  d_score: int, max_corners: int, quality_level: float = 0.01, min_distance: float = 10.0,
                  window_size: int = 5, u8: bool = False, stream: int = 0) -> None:
    """oflk_good_features on device pointers: frames [F][H][W] -> d_count [F] int32, d_xy [F][K][2] float32 (x, y),
    d_score [F][K] float32; d_workspace of at least good_features_workspace bytes."""
    check(lib().oflk_good_features(d_frames, int(bool(u8)), int(F), int(H), int(W), int(window_size), float(quality_level),
                                   float(min_distance), int(max_corners), d_workspace, int(workspace_bytes), d_count, d_xy,
                                   d_score, stream))


def replenish_features_workspace(H: int, W: int, window_size: int = 5, min_distance: float = 10.0, max_corners: int = 100) -> int:
    """bytes of oflk_replenish_features' workspace for this shape"""
    n = ctypes.c_size_t(0)
    check(lib().oflk_replenish_features_workspace(int(H), int(W), int(window_size), float(min_distance), int(max_corners),
                                                  ctypes.byref(n)))
    return int(n.value)


def replenish_features(d_frame: int, H: int, W: int, t: int, d_xy: int, d_visible: int, d_workspace: int, workspace_bytes: int,
                       d_qt: int, d_qxy: int, d_born: int, d_detected: int, max_corners: int, quality_level: float = 0.01,
                       min_distance: float = 10.0, window_size: int = 5, u8: bool = False, stream: int = 0) -> None:
    """oflk_replenish_features on device pointers: one detection on frame t [H][W] away from the alive slots of d_xy [K][2] /
    d_visible [K]; the new points go into the free slots of d_qt [K] int32 (= t) and d_qxy [K][2], d_born [K] uint8 marks
    them and d_detected [1] int32 counts them; d_workspace of at least replenish_features_workspace bytes."""
    check(lib().oflk_replenish_features(d_frame, int(bool(u8)), int(H), int(W), int(window_size), float(quality_level),
                                        float(min_distance), int(max_corners), int(t), d_xy, d_visible, d_workspace,
                                        int(workspace_bytes), d_qt, d_qxy, d_born, d_detected, stream))


MOTION_MODELS = {"translation": 0, "similarity": 1, "affine": 2}
MOTION_MAX_HYPOTHESES = 65536


def check_motion_params(model, hypotheses, threshold: float, seed) -> "Fit":
    """The fit's parameters as the C ABI takes them, a Fit: (model code, hypotheses, threshold as float32, seed as uint32);
    ValueError for an unknown model, hypotheses outside [1, MOTION_MAX_HYPOTHESES], a threshold that is not finite and
    positive or a seed outside uint32.  Nothing here touches a device."""
    code = MOTION_MODELS.get(model) if isinstance(model, str) else (model if model in (0, 1, 2) and not isinstance(model, bool) else None)
    if code is None:
        raise ValueError(f"model must be one of {sorted(MOTION_MODELS)}, got {model!r}")
    return Fit(int(code), *check_ransac_params(hypotheses, threshold, seed))


def check_ransac_params(hypotheses, threshold: float, seed) -> Tuple[int, float, int]:
    """What the motion and the homography fit share of check_motion_params: (hypotheses, threshold as float32, seed as
    uint32), with its ValueErrors"""
    check_int("hypotheses", hypotheses, 1, MOTION_MAX_HYPOTHESES)
    with np.errstate(over="ignore"):
        thr = np.float32(threshold)
    if not (np.isfinite(thr) and thr > 0):
        raise ValueError(f"threshold must be finite and > 0, got {threshold!r}")
    check_int("seed", seed, 0, 2 ** 32 - 1, "in [0, 2^32)")
    return int(hypotheses), float(thr), int(seed)


def motion_workspace(S: int, N: int, hypotheses: int) -> int:
    """bytes of the workspace of oflk_estimate_motion (S steps of N correspondences) and oflk_tracks_motion (S = T-1, N = K)"""
    n = ctypes.c_size_t(0)
    check(lib().oflk_motion_workspace(int(S), int(N), int(hypotheses), ctypes.byref(n)))
    return int(n.value)


def estimate_motion(d_src: int, d_dst: int, d_valid: int, S: int, N: int, d_workspace: int, workspace_bytes: int, d_model: int,
                    d_inlier: int, d_counts: int, model: int = 1, hypotheses: int = 256, threshold: float = 1.0, seed: int = 0,
                    step0: int = 0, stream: int = 0) -> None:
    """oflk_estimate_motion on device pointers: d_src, d_dst [S][N][2] float32, d_valid [S][N] uint8 or 0 -> d_model [S][6]
    float32, d_inlier [S][N] uint8, d_counts [S][3] int32 (n_inliers, n_valid, status); asynchronous on `stream`."""
    check(lib().oflk_estimate_motion(d_src or None, d_dst or None, d_valid or None, int(S), int(N), int(step0), int(model),
                                     int(hypotheses), float(threshold), int(seed), d_workspace or None, int(workspace_bytes),
                                     d_model or None, d_inlier or None, d_counts or None, stream))


def tracks_motion(d_tracks: int, d_visible: int, d_born: int, T: int, K: int, d_workspace: int, workspace_bytes: int,
                  d_model: int, d_inlier: int, d_counts: int, model: int = 1, hypotheses: int = 256, threshold: float = 1.0,
                  seed: int = 0, t0: int = 0, stream: int = 0) -> None:
    """oflk_tracks_motion on device pointers: rows d_tracks [T][K][2], d_visible [T][K], d_born [T][K] or 0 -> the T-1 steps'
    d_model [T-1][6], d_inlier [T-1][K], d_counts [T-1][3]; the workspace is motion_workspace(T-1, K, hypotheses)."""
    check(lib().oflk_tracks_motion(d_tracks or None, d_visible or None, d_born or None, int(T), int(K), int(t0), int(model),
                                   int(hypotheses), float(threshold), int(seed), d_workspace or None, int(workspace_bytes),
                                   d_model or None, d_inlier or None, d_counts or None, stream))


def estimate_motion_host(src: np.ndarray, dst: np.ndarray, valid: Optional[np.ndarray], model: int, hypotheses: int,
                         threshold: float, seed: int, step0: int = 0):
    """oflk_estimate_motion_host: contiguous float32 (S, N, 2) arrays and an optional uint8 (S, N) mask in; (model (S, 6)
    float32, inlier (S, N) uint8, counts (S, 3) int32) out"""
    S, N = src.shape[:2]
    out, inl, cnt = np.empty((S, 6), np.float32), np.empty((S, N), np.uint8), np.empty((S, 3), np.int32)
    check(lib().oflk_estimate_motion_host(ptr(src), ptr(dst), None if valid is None else valid.ctypes.data, S, N, int(step0),
                                          int(model), int(hypotheses), float(threshold), int(seed), ptr(out), inl.ctypes.data,
                                          cnt.ctypes.data_as(_i32p)))
    return out, inl, cnt


def homography_workspace(S: int, N: int, hypotheses: int) -> int:
    """bytes of the workspace of oflk_estimate_homography (S steps of N correspondences) and oflk_tracks_homography (S = T-1,
    N = K)"""
    n = ctypes.c_size_t(0)
    check(lib().oflk_homography_workspace(int(S), int(N), int(hypotheses), ctypes.byref(n)))
    return int(n.value)


def estimate_homography(d_src: int, d_dst: int, d_valid: int, S: int, N: int, d_workspace: int, workspace_bytes: int, d_model: int,
                        d_inlier: int, d_counts: int, hypotheses: int = 256, threshold: float = 1.0, seed: int = 0, step0: int = 0,
                        stream: int = 0) -> None:
    """oflk_estimate_homography on device pointers: d_src, d_dst [S][N][2] float32, d_valid [S][N] uint8 or 0 -> d_model
    [S][9] float32, d_inlier [S][N] uint8, d_counts [S][3] int32 (n_inliers, n_valid, status); asynchronous on `stream`."""
    check(lib().oflk_estimate_homography(d_src or None, d_dst or None, d_valid or None, int(S), int(N), int(step0), int(hypotheses),
                                         float(threshold), int(seed), d_workspace or None, int(workspace_bytes), d_model or None,
                                         d_inlier or None, d_counts or None, stream))


def tracks_homography(d_tracks: int, d_visible: int, d_born: int, T: int, K: int, d_workspace: int, workspace_bytes: int,
                      d_model: int, d_inlier: int, d_counts: int, hypotheses: int = 256, threshold: float = 1.0, seed: int = 0,
                      t0: int = 0, stream: int = 0) -> None:
    """oflk_tracks_homography on device pointers: rows d_tracks [T][K][2], d_visible [T][K], d_born [T][K] or 0 -> the T-1
    steps' d_model [T-1][9], d_inlier [T-1][K], d_counts [T-1][3]; the workspace is homography_workspace(T-1, K, hypotheses)."""
    check(lib().oflk_tracks_homography(d_tracks or None, d_visible or None, d_born or None, int(T), int(K), int(t0), int(hypotheses),
                                       float(threshold), int(seed), d_workspace or None, int(workspace_bytes), d_model or None,
                                       d_inlier or None, d_counts or None, stream))


def estimate_homography_host(src: np.ndarray, dst: np.ndarray, valid: Optional[np.ndarray], hypotheses: int, threshold: float,
                             seed: int, step0: int = 0):
    """oflk_estimate_homography_host: contiguous float32 (S, N, 2) arrays and an optional uint8 (S, N) mask in; (model (S, 9)
    float32, inlier (S, N) uint8, counts (S, 3) int32) out"""
    S, N = src.shape[:2]
    out, inl, cnt = np.empty((S, 9), np.float32), np.empty((S, N), np.uint8), np.empty((S, 3), np.int32)
    check(lib().oflk_estimate_homography_host(ptr(src), ptr(dst), None if valid is None else valid.ctypes.data, S, N, int(step0),
                                              int(hypotheses), float(threshold), int(seed), ptr(out), inl.ctypes.data,
                                              cnt.ctypes.data_as(_i32p)))
    return out, inl, cnt


STABILIZE_MAX_RADIUS = 64


def stabilize_weights(radius, sigma=None) -> np.ndarray:
    """The window of the trajectory filter as the C ABI takes it: radius + 1 float64 Gaussian weights
    exp(-0.5 (i / sigma)^2), sigma defaulting to radius / 2 (1.0 for radius 0), formed here on the host.  ValueError for a
    radius outside [0, STABILIZE_MAX_RADIUS], a sigma that is not finite and positive, or a weight that underflows to 0."""
    radius = check_int("radius", radius, 0, STABILIZE_MAX_RADIUS)
    if sigma is None:
        sigma = radius / 2 if radius > 0 else 1.0
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be finite and > 0, got {sigma!r}")
    w = np.exp(-0.5 * (np.arange(radius + 1) / sigma) ** 2)
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError(f"sigma {sigma!r} is too small for radius {radius}: a weight underflows to 0")
    return np.ascontiguousarray(w, np.float64)


def _f64(a: np.ndarray):
    return a.ctypes.data_as(_f64p)


def stabilize_trajectory(d_model: int, d_counts: int, T: int, weights: np.ndarray, d_correction: int, d_map: int, d_held: int = 0,
                         stream: int = 0) -> None:
    """oflk_stabilize_trajectory on device pointers: d_model [T-1][6] float32, d_counts [T-1][3] int32 or 0, the host weights
    (radius = len - 1) -> d_correction [T][6] float32, d_map [T][6] float64, d_held [T-1] uint8 or 0; asynchronous."""
    w = np.ascontiguousarray(weights, np.float64)
    check(lib().oflk_stabilize_trajectory(d_model or None, d_counts or None, int(T), _f64(w), int(w.size) - 1, d_correction or None,
                                          d_map or None, d_held or None, stream))


def stabilize_trajectory_ring(d_model_ring: int, d_counts_ring: int, cap: int, f0: int, n: int, T: int, weights: np.ndarray,
                              d_correction: int, d_map: int, stream: int = 0) -> None:
    """oflk_stabilize_trajectory_ring on device pointers: step s at slot s % cap of d_model_ring [cap][6] float32 and
    d_counts_ring [cap][3] int32 (or 0); frames f0 .. f0 + n - 1 of a stream of T frames (T = -1: open, n = 1) ->
    d_correction [n][6] float32, d_map [n][6] float64; asynchronous."""
    w = np.ascontiguousarray(weights, np.float64)
    check(lib().oflk_stabilize_trajectory_ring(d_model_ring or None, d_counts_ring or None, int(cap), int(f0), int(n), int(T), _f64(w),
                                               int(w.size) - 1, d_correction or None, d_map or None, stream))


def warp_affine(d_frames: int, F: int, H: int, W: int, d_map: int, d_out: int, d_inside: int = 0, u8: bool = False,
                stream: int = 0) -> None:
    """oflk_warp_affine on device pointers: frames and d_out [F][H][W] (float32, or uint8 with u8), d_map [F][6] float64,
    d_inside [F][H][W] uint8 or 0; asynchronous."""
    check(lib().oflk_warp_affine(d_frames or None, int(bool(u8)), int(F), int(H), int(W), d_map or None, d_out or None,
                                 d_inside or None, stream))


def warp_perspective(d_frames: int, F: int, H: int, W: int, d_map: int, d_out: int, d_inside: int = 0, u8: bool = False,
                     stream: int = 0) -> None:
    """oflk_warp_perspective on device pointers: oflk_warp_affine's arguments with d_map [F][9] float64; asynchronous."""
    check(lib().oflk_warp_perspective(d_frames or None, int(bool(u8)), int(F), int(H), int(W), d_map or None, d_out or None,
                                      d_inside or None, stream))


def stabilize_trajectory_host(model: np.ndarray, counts: Optional[np.ndarray], T: int, weights: np.ndarray):
    """oflk_stabilize_trajectory_host: contiguous float32 (T-1, 6) models and optional int32 (T-1, 3) counts in;
    (correction (T, 6) float32, map (T, 6) float64, held (T-1,) uint8) out"""
    corr, mp, held = np.empty((T, 6), np.float32), np.empty((T, 6), np.float64), np.empty(max(T - 1, 0), np.uint8)
    check(lib().oflk_stabilize_trajectory_host(ptr(model) if T > 1 else None, None if counts is None or T < 2 else counts.ctypes.data_as(_i32p),
                                               int(T), _f64(weights), int(weights.size) - 1, ptr(corr), _f64(mp),
                                               held.ctypes.data if T > 1 else None))
    return corr, mp, held


def warp_affine_host(frames: np.ndarray, maps: np.ndarray, inside: bool = False):
    """oflk_warp_affine_host[_u8] -- oflk_warp_perspective_host[_u8] for (F, 9) maps --: contiguous (F, H, W) float32 or uint8
    frames and (F, 6) float64 maps in; the warped frames and, when asked for, the inside mask (else None) out"""
    F, H, W = frames.shape
    out = np.empty_like(frames)
    ins = np.empty((F, H, W), np.uint8) if inside else None
    src, fn = pixels(frames, "oflk_warp_perspective_host" if maps.shape[-1] == 9 else "oflk_warp_affine_host")
    check(fn(src, F, H, W, _f64(maps), pix(out), None if ins is None else ins.ctypes.data))
    return out, ins


COLOUR_ORDERS = {"rgb": 0, "bgr": 1}


def check_colour_order(order) -> int:
    """the C ABI's code of a channel order given by name; ValueError for anything else"""
    if not isinstance(order, str) or order not in COLOUR_ORDERS:
        raise ValueError(f"order must be one of {sorted(COLOUR_ORDERS)}, got {order!r}")
    return COLOUR_ORDERS[order]


def is_packed(frames, ndim: int = 4) -> bool:
    """True for an array with a trailing channel axis: `ndim` dimensions where the grey form has ndim - 1"""
    return isinstance(frames, np.ndarray) and frames.ndim == ndim


def as_packed(frames, what: str = "(F, H, W, C)") -> np.ndarray:
    """Interleaved colour frames as one contiguous uint8 (F, H, W, C) array, C in {3, 4} and H, W >= 2.  ValueError for
    anything else, float32 colour included; no device call."""
    if not isinstance(frames, np.ndarray) or frames.ndim != 4:
        raise ValueError(f"expected a {what} array of colour frames, got shape {np.shape(frames)}")
    if frames.dtype != np.uint8:
        raise ValueError(f"colour frames must be uint8 (float32 colour is not offered), got {frames.dtype}")
    F, H, W, C = frames.shape
    if C not in (3, 4):
        raise ValueError(f"colour frames must have 3 or 4 interleaved channels, got {C}")
    if F < 1 or H < 2 or W < 2:
        raise ValueError(f"expected at least one frame of at least 2 x 2 pixels, got shape {frames.shape}")
    return np.ascontiguousarray(frames)


def luma(d_frames: int, F: int, H: int, W: int, channels: int, d_luma: int, order: int = 0, stream: int = 0) -> None:
    """oflk_luma_u8 on device pointers: d_frames [F][H][W][channels] uint8 -> d_luma [F][H][W] uint8; asynchronous."""
    check(lib().oflk_luma_u8(d_frames or None, int(F), int(H), int(W), int(channels), int(order), d_luma or None, stream))


def luma_host(frames: np.ndarray, order: int = 0) -> np.ndarray:
    """oflk_luma_u8_host: contiguous uint8 (F, H, W, C) frames in, their (F, H, W) uint8 luma out"""
    F, H, W, C = frames.shape
    out = np.empty((F, H, W), np.uint8)
    check(lib().oflk_luma_u8_host(frames.ctypes.data, F, H, W, C, int(order), out.ctypes.data))
    return out


def warp_affine_packed(d_frames: int, F: int, H: int, W: int, channels: int, d_map: int, d_out: int, d_inside: int = 0,
                       stream: int = 0) -> None:
    """oflk_warp_affine_packed on device pointers: frames and d_out [F][H][W][channels] uint8, d_map [F][6] float64, d_inside
    [F][H][W] uint8 or 0; asynchronous."""
    check(lib().oflk_warp_affine_packed(d_frames or None, int(F), int(H), int(W), int(channels), d_map or None, d_out or None,
                                        d_inside or None, stream))


def warp_perspective_packed(d_frames: int, F: int, H: int, W: int, channels: int, d_map: int, d_out: int, d_inside: int = 0,
                            stream: int = 0) -> None:
    """oflk_warp_perspective_packed on device pointers: oflk_warp_affine_packed's arguments with d_map [F][9]; asynchronous."""
    check(lib().oflk_warp_perspective_packed(d_frames or None, int(F), int(H), int(W), int(channels), d_map or None, d_out or None,
                                             d_inside or None, stream))


def warp_packed_host(frames: np.ndarray, maps: np.ndarray, inside: bool = False):
    """oflk_warp_affine_packed_host -- oflk_warp_perspective_packed_host for (F, 9) maps --: contiguous uint8 (F, H, W, C) frames
    and float64 maps in; the warped frames and, when asked for, the (F, H, W) inside mask (else None) out"""
    F, H, W, C = frames.shape
    out = np.empty_like(frames)
    ins = np.empty((F, H, W), np.uint8) if inside else None
    fn = lib().oflk_warp_perspective_packed_host if maps.shape[-1] == 9 else lib().oflk_warp_affine_packed_host
    check(fn(frames.ctypes.data, F, H, W, C, _f64(maps), out.ctypes.data, None if ins is None else ins.ctypes.data))
    return out, ins


OFLK_SITING_LEFT, OFLK_SITING_CENTER = 0, 1
NV12_SITINGS = {"left": OFLK_SITING_LEFT, "center": OFLK_SITING_CENTER}


def check_nv12_siting(siting) -> int:
    """the C ABI's code of a chroma siting given by name; ValueError for anything else"""
    if not isinstance(siting, str) or siting not in NV12_SITINGS:
        raise ValueError(f"siting must be one of {sorted(NV12_SITINGS)}, got {siting!r}")
    return NV12_SITINGS[siting]


def as_nv12(frames, what: str = "(F, 3H/2, W)") -> np.ndarray:
    """NV12 frames as one contiguous uint8 (F, 3H/2, W) array: rows 0 .. H-1 of a frame are its Y plane, the H/2 rows behind
    them its interleaved U, V pairs; H and W even and >= 4.  ValueError for anything else; no device call."""
    if not isinstance(frames, np.ndarray) or frames.ndim != 3:
        raise ValueError(f"expected a {what} array of NV12 frames, got shape {np.shape(frames)}")
    if frames.dtype != np.uint8:
        raise ValueError(f"NV12 frames must be uint8, got {frames.dtype}")
    F, R, W = frames.shape
    if R % 3 or (2 * R // 3) % 2:
        raise ValueError(f"an NV12 frame has 3H/2 rows with H even, got {R} rows")
    if W % 2:
        raise ValueError(f"NV12 frames need an even W, got {W}")
    if F < 1 or 2 * R // 3 < 4 or W < 4:
        raise ValueError(f"expected at least one NV12 frame of at least 4 x 4 pixels, got shape {frames.shape}")
    return np.ascontiguousarray(frames)


def warp_affine_nv12(d_frames: int, F: int, H: int, W: int, d_map: int, d_out: int, d_inside: int = 0, siting: int = 0,
                     stream: int = 0) -> None:
    """oflk_warp_affine_nv12 on device pointers: frames and d_out [F][H W 3 / 2] uint8, d_map [F][6] float64, d_inside
    [F][H][W] uint8 or 0; asynchronous."""
    check(lib().oflk_warp_affine_nv12(d_frames or None, int(F), int(H), int(W), int(siting), d_map or None, d_out or None,
                                      d_inside or None, stream))


def warp_perspective_nv12(d_frames: int, F: int, H: int, W: int, d_map: int, d_out: int, d_inside: int = 0, siting: int = 0,
                          stream: int = 0) -> None:
    """oflk_warp_perspective_nv12 on device pointers: oflk_warp_affine_nv12's arguments with d_map [F][9]; asynchronous."""
    check(lib().oflk_warp_perspective_nv12(d_frames or None, int(F), int(H), int(W), int(siting), d_map or None, d_out or None,
                                           d_inside or None, stream))


def warp_nv12_host(frames: np.ndarray, maps: np.ndarray, siting: int = 0, inside: bool = False):
    """oflk_warp_affine_nv12_host -- oflk_warp_perspective_nv12_host for (F, 9) maps --: contiguous uint8 (F, 3H/2, W) frames
    and float64 maps in; the warped frames and, when asked for, the (F, H, W) inside mask (else None) out"""
    F, R, W = frames.shape
    H = 2 * R // 3
    out = np.empty_like(frames)
    ins = np.empty((F, H, W), np.uint8) if inside else None
    fn = lib().oflk_warp_perspective_nv12_host if maps.shape[-1] == 9 else lib().oflk_warp_affine_nv12_host
    check(fn(frames.ctypes.data, F, H, W, int(siting), _f64(maps), out.ctypes.data, None if ins is None else ins.ctypes.data))
    return out, ins


MOSAIC_BLENDS = {"mean": 0, "feather": 1, "first": 2, "last": 3}


def check_mosaic_blend(blend) -> int:
    """the C ABI's code of a blend given by name; ValueError for anything else"""
    if not isinstance(blend, str) or blend not in MOSAIC_BLENDS:
        raise ValueError(f"blend must be one of {sorted(MOSAIC_BLENDS)}, got {blend!r}")
    return MOSAIC_BLENDS[blend]


def mosaic_state_bytes(Hc: int, Wc: int) -> int:
    """bytes of the canvas state of oflk_mosaic_accumulate / oflk_mosaic_resolve (0: the canvas is refused)"""
    return int(lib().oflk_mosaic_state_bytes(int(Hc), int(Wc)))


def mosaic_chain(d_model: int, d_counts: int, T: int, anchor: int, H: int, W: int, extent: float, d_from_anchor: int, d_to_anchor: int,
                 d_box: int, d_held: int, d_dropped: int, stream: int = 0) -> None:
    """oflk_mosaic_chain on device pointers: d_model [T-1][9] float32, d_counts [T-1][3] int32 or 0 -> d_from_anchor, d_to_anchor
    [T][9] float64, d_box [T][4] float64, d_held [T-1] uint8 or 0, d_dropped [T] uint8; asynchronous."""
    check(lib().oflk_mosaic_chain(d_model or None, d_counts or None, int(T), int(anchor), int(H), int(W), float(extent),
                                  d_from_anchor or None, d_to_anchor or None, d_box or None, d_held or None, d_dropped or None, stream))


def mosaic_chain_host(model: np.ndarray, counts: Optional[np.ndarray], T: int, anchor: int, H: int, W: int, extent: float):
    """oflk_mosaic_chain_host: contiguous float32 (T-1, 9) models and optional int32 (T-1, 3) counts in; (from_anchor (T, 9),
    to_anchor (T, 9), box (T, 4) float64, held (T-1,), dropped (T,) uint8) out"""
    fr, to, box = np.empty((T, 9), np.float64), np.empty((T, 9), np.float64), np.empty((T, 4), np.float64)
    held, drop = np.empty(max(T - 1, 0), np.uint8), np.empty(T, np.uint8)
    check(lib().oflk_mosaic_chain_host(ptr(model) if T > 1 else None, None if counts is None or T < 2 else counts.ctypes.data_as(_i32p),
                                       int(T), int(anchor), int(H), int(W), float(extent), _f64(fr), _f64(to), _f64(box),
                                       held.ctypes.data if T > 1 else None, drop.ctypes.data))
    return fr, to, box, held, drop


def mosaic_canvas(box: np.ndarray, dropped: np.ndarray):
    """oflk_mosaic_canvas (host only): (x0, y0, Wc, Hc) of the boxes that are not dropped"""
    box, dropped = np.ascontiguousarray(box, np.float64), np.ascontiguousarray(dropped, np.uint8)
    v = [ctypes.c_int() for _ in range(4)]
    check(lib().oflk_mosaic_canvas(_f64(box), dropped.ctypes.data, int(dropped.size), *[ctypes.byref(c) for c in v]))
    return tuple(int(c.value) for c in v)


def mosaic_accumulate(d_frames: int, F: int, H: int, W: int, d_map: int, d_skip: int, x0: int, y0: int, Hc: int, Wc: int, blend: int,
                      d_state: int, state_bytes: int, u8: bool = False, stream: int = 0, d_exposure: Optional[int] = None) -> None:
    """oflk_mosaic_accumulate on device pointers: adds d_frames [F][H][W] (float32, or uint8 with u8) under d_map [F][9] float64
    (d_skip [F] uint8 or 0) to the canvas state d_state; asynchronous.  d_exposure given: oflk_mosaic_accumulate_exposure with
    the frames' (eg, eb) [F][2] float64."""
    fn = lib().oflk_mosaic_accumulate if d_exposure is None else lib().oflk_mosaic_accumulate_exposure
    check(fn(d_frames or None, int(bool(u8)), int(F), int(H), int(W), d_map or None, d_skip or None,
             *(() if d_exposure is None else (d_exposure or None,)), int(x0), int(y0), int(Hc), int(Wc), int(blend), d_state or None,
             int(state_bytes), stream))


def mosaic_resolve(d_state: int, Hc: int, Wc: int, d_out: int, d_count: int = 0, u8: bool = False, stream: int = 0) -> None:
    """oflk_mosaic_resolve on device pointers: d_out [Hc][Wc] (float32, or uint8 with u8), d_count [Hc][Wc] int32 or 0;
    asynchronous."""
    check(lib().oflk_mosaic_resolve(d_state or None, int(Hc), int(Wc), int(bool(u8)), d_out or None, d_count or None, stream))


def mosaic_composite_host(frames: np.ndarray, maps: np.ndarray, skip: Optional[np.ndarray], x0: int, y0: int, Hc: int, Wc: int,
                          blend: int, count: bool = False, exposure: Optional[np.ndarray] = None):
    """oflk_mosaic_composite_host[_u8]: contiguous (F, H, W) float32 or uint8 frames, (F, 9) float64 maps and optional (F,) uint8
    skip flags in; the (Hc, Wc) mosaic and, when asked for, the int32 count (else None) out.  exposure given (contiguous (F, 2)
    float64): oflk_mosaic_composite_exposure_host[_u8]"""
    F, H, W = frames.shape
    out = np.empty((Hc, Wc), frames.dtype)
    cnt = np.empty((Hc, Wc), np.int32) if count else None
    src, fn = pixels(frames, "oflk_mosaic_composite_host" if exposure is None else "oflk_mosaic_composite_exposure_host")
    check(fn(src, F, H, W, _f64(maps), None if skip is None else skip.ctypes.data, *(() if exposure is None else (_f64(exposure),)),
             int(x0), int(y0), int(Hc), int(Wc), int(blend), pix(out), None if cnt is None else cnt.ctypes.data_as(_i32p)))
    return out, cnt


def check_mosaic_canvas(canvas_shape, origin):
    """canvas_shape and origin of mosaic_composite and mosaic_median as (Hc, Wc, x0, y0); ValueError otherwise"""
    if len(canvas_shape) != 2 or int(canvas_shape[0]) < 1 or int(canvas_shape[1]) < 1:
        raise ValueError(f"canvas_shape must be (Hc, Wc) with Hc, Wc >= 1, got {canvas_shape!r}")
    Hc, Wc = int(canvas_shape[0]), int(canvas_shape[1])
    if Hc * Wc >= 2 ** 30:
        raise ValueError(f"a canvas of 2^30 pixels or more is not supported, got {Hc} x {Wc}")
    if len(origin) != 2 or any(isinstance(v, bool) or int(v) != v or abs(int(v)) >= 2 ** 31 for v in origin):
        raise ValueError(f"origin must be two integers (x0, y0), got {origin!r}")
    return Hc, Wc, int(origin[0]), int(origin[1])


def check_mosaic_flags(F: int, skip, exposure):
    """skip as contiguous (F,) uint8 flags or None, exposure as contiguous (F, 2) float64 or None; ValueError otherwise"""
    sk = None
    if skip is not None:
        sk = np.asarray(skip)
        if sk.shape != (F,):
            raise ValueError(f"skip must have shape {(F,)}, got {sk.shape}")
        sk = np.ascontiguousarray(sk != 0, np.uint8)
    ex = None
    if exposure is not None:
        ex = np.ascontiguousarray(exposure, np.float64)
        if ex.shape != (F, 2):
            raise ValueError(f"exposure must have shape {(F, 2)}, got {ex.shape}")
    return sk, ex


def mosaic_median_capacity() -> int:
    """oflk_mosaic_median_capacity (host only): the samples a pixel of the temporal median keeps on chip"""
    return int(lib().oflk_mosaic_median_capacity())


def mosaic_median(d_frames: int, F: int, H: int, W: int, d_map: int, d_skip: int, d_exposure: int, x0: int, y0: int, Hc: int, Wc: int,
                  d_out: int, d_count: int = 0, u8: bool = False, stream: int = 0) -> None:
    """oflk_mosaic_median on device pointers: the temporal median of d_frames [F][H][W] (float32, or uint8 with u8) under d_map
    [F][9] float64 (d_skip [F] uint8 or 0, d_exposure [F][2] float64 or 0) -> d_out [Hc][Wc] of the frames' type, d_count
    [Hc][Wc] int32 or 0; asynchronous."""
    check(lib().oflk_mosaic_median(d_frames or None, int(bool(u8)), int(F), int(H), int(W), d_map or None, d_skip or None,
                                   d_exposure or None, int(x0), int(y0), int(Hc), int(Wc), d_out or None, d_count or None, stream))


def mosaic_median_host(frames: np.ndarray, maps: np.ndarray, skip: Optional[np.ndarray], exposure: Optional[np.ndarray], x0: int, y0: int,
                       Hc: int, Wc: int, count: bool = False):
    """oflk_mosaic_median_host[_u8]: contiguous (F, H, W) float32 or uint8 frames, (F, 9) float64 maps, optional (F,) uint8 skip
    flags and optional (F, 2) float64 exposure in; the (Hc, Wc) median and, when asked for, the int32 count (else None) out"""
    F, H, W = frames.shape
    out = np.empty((Hc, Wc), frames.dtype)
    cnt = np.empty((Hc, Wc), np.int32) if count else None
    src, fn = pixels(frames, "oflk_mosaic_median_host")
    check(fn(src, F, H, W, _f64(maps), None if skip is None else skip.ctypes.data, None if exposure is None else _f64(exposure),
             int(x0), int(y0), int(Hc), int(Wc), pix(out), None if cnt is None else cnt.ctypes.data_as(_i32p)))
    return out, cnt


def exposure_chain_host(photo: np.ndarray, status: Optional[np.ndarray], T: int, anchor: int) -> np.ndarray:
    """oflk_exposure_chain_host (host only): contiguous float32 (T-1, 2) step (g, b) and optional int32 (T-1,) statuses in; the
    frames' (eg, eb) (T, 2) float64 out"""
    out = np.empty((T, 2), np.float64)
    check(lib().oflk_exposure_chain_host(ptr(photo) if T > 1 else None,
                                         None if status is None or T < 2 else status.ctypes.data_as(_i32p), int(T), int(anchor), _f64(out)))
    return out


ALIGN_KINDS = {"affine": 0, "homography": 1}


def check_align_params(kind, levels, iterations, min_share: float) -> Tuple[int, int, int, float]:
    """the C ABI's model code and the checked levels, iterations and min_share of the alignment calls; ValueError otherwise"""
    if not isinstance(kind, str) or kind not in ALIGN_KINDS:
        raise ValueError(f"kind must be one of {sorted(ALIGN_KINDS)}, got {kind!r}")
    check_int("levels", levels, 1)
    check_int("iterations", iterations, 1)
    ms = float(min_share)
    if not 0.0 < ms <= 1.0:
        raise ValueError(f"min_share must be in (0, 1], got {min_share!r}")
    return ALIGN_KINDS[kind], int(levels), int(iterations), ms


def check_robust_delta(robust_delta) -> float:
    """the checked Huber threshold of the robust alignment calls, in grey levels; ValueError otherwise"""
    if isinstance(robust_delta, bool) or not isinstance(robust_delta, (int, float, np.integer, np.floating)):
        raise ValueError(f"robust_delta must be a number, got {robust_delta!r}")
    with np.errstate(all="ignore"):
        d = float(np.float32(robust_delta))
    if not (np.isfinite(d) and d > 0.0):
        raise ValueError(f"robust_delta must be finite and > 0 as float32, got {robust_delta!r}")
    return d


def align_workspace(S: int, H: int, W: int, levels: int, model: int, photometric: bool = False, robust: bool = False) -> int:
    """bytes of the workspace of oflk_align_refine for S steps (oflk_align_sequence: S = T - 1); photometric: of
    oflk_align_refine_photo (oflk_align_photo_workspace); robust: of oflk_align_refine_robust (oflk_align_robust_workspace)"""
    n = ctypes.c_size_t(0)
    fn = getattr(lib(), "oflk_align_robust_workspace" if robust else "oflk_align_photo_workspace" if photometric else "oflk_align_workspace")
    check(fn(int(S), int(H), int(W), int(levels), int(model), *((int(bool(photometric)),) if robust else ()), ctypes.byref(n)))
    return int(n.value)


def _align_device(name: str, frames: tuple, levels, iterations, model, min_share, d_model_in, d_status_in, d_workspace,
                  workspace_bytes, d_model_out, d_status_out, d_stats, stream, d_photo_out, robust_delta) -> None:
    """the one body of align_refine and align_sequence: chooses the plain, _photo or _robust form of `name` and gives it
    that form's extra arguments (robust_delta and the photometric flag behind min_share, d_photo_out before the stream)"""
    form, settings, photo = "", (), ()
    if robust_delta is not None:
        form, settings, photo = "_robust", (float(robust_delta), int(d_photo_out is not None)), (d_photo_out or None,)
    elif d_photo_out is not None:
        form, photo = "_photo", (d_photo_out or None,)
    check(getattr(lib(), name + form)(*frames, int(levels), int(iterations), int(model), float(min_share), *settings,
                                      d_model_in or None, d_status_in or None, d_workspace or None, int(workspace_bytes),
                                      d_model_out or None, d_status_out or None, d_stats or None, *photo, stream))


def align_refine(d_a: int, d_b: int, S: int, H: int, W: int, levels: int, iterations: int, model: int, min_share: float,
                 d_model_in: int, d_status_in: int, d_workspace: int, workspace_bytes: int, d_model_out: int, d_status_out: int,
                 d_stats: int, u8: bool = False, stream: int = 0, d_photo_out: Optional[int] = None,
                 robust_delta: Optional[float] = None) -> None:
    """oflk_align_refine on device pointers: d_a, d_b [S][H][W] (float32, or uint8 with u8), d_model_in / d_model_out [S][6 | 9]
    float32, d_status_in [S] int32 or 0, d_status_out [S] int32, d_stats [S][4] float64; asynchronous.  d_photo_out given:
    oflk_align_refine_photo with (g, b) [S][2] float32 out and a workspace of align_workspace(..., photometric=True) bytes.
    robust_delta given: oflk_align_refine_robust (photometric when d_photo_out is given), d_stats [S][8] and a workspace of
    align_workspace(..., robust=True) bytes; the C call checks robust_delta."""
    _align_device("oflk_align_refine", (d_a or None, d_b or None, int(bool(u8)), int(S), int(H), int(W)), levels, iterations, model,
                  min_share, d_model_in, d_status_in, d_workspace, workspace_bytes, d_model_out, d_status_out, d_stats, stream,
                  d_photo_out, robust_delta)


def align_sequence(d_frames: int, T: int, H: int, W: int, levels: int, iterations: int, model: int, min_share: float,
                   d_model_in: int, d_status_in: int, d_workspace: int, workspace_bytes: int, d_model_out: int, d_status_out: int,
                   d_stats: int, u8: bool = False, stream: int = 0, d_photo_out: Optional[int] = None,
                   robust_delta: Optional[float] = None) -> None:
    """oflk_align_sequence on device pointers: the T-1 steps t -> t+1 of d_frames [T][H][W], with align_refine's other
    arguments for S = T - 1; asynchronous.  d_photo_out given: oflk_align_sequence_photo.  robust_delta given:
    oflk_align_sequence_robust."""
    _align_device("oflk_align_sequence", (d_frames or None, int(bool(u8)), int(T), int(H), int(W)), levels, iterations, model,
                  min_share, d_model_in, d_status_in, d_workspace, workspace_bytes, d_model_out, d_status_out, d_stats, stream,
                  d_photo_out, robust_delta)


def _align_host(a: np.ndarray, b: Optional[np.ndarray], model_in: np.ndarray, status_in: Optional[np.ndarray], levels: int,
                iterations: int, model: int, min_share: float, photometric: bool, robust_delta: Optional[float]):
    """the one body of align_host and align_robust_host: (model, status, stats, photo) of the plain, _photo or _robust host
    form.  The forms differ in the stats' width (4, robust 8), in the photo output (none, (S, 2), robust: (S, 2) preset to
    (1, 0) and passed only with photometric) and in the robust form's two scalars behind min_share."""
    robust = robust_delta is not None
    F, H, W = a.shape
    S = F if b is not None else F - 1
    out = np.empty_like(model_in)
    st, stats = np.empty(S, np.int32), np.empty((S, 8 if robust else 4), np.float64)
    photo = np.empty((S, 2), np.float32) if robust or photometric else None
    if robust:
        photo[:] = (1.0, 0.0)
    settings = (int(H), int(W), int(levels), int(iterations), int(model), float(min_share))
    io = (ptr(model_in), None if status_in is None else status_in.ctypes.data_as(_i32p), ptr(out), st.ctypes.data_as(_i32p), _f64(stats))
    if robust:
        settings += (float(robust_delta), int(bool(photometric)))
        io += (ptr(photo) if photometric else None,)
    elif photometric:
        io += (ptr(photo),)
    pa, fn = pixels(a, ("oflk_align_refine" if b is not None else "oflk_align_sequence")
                    + ("_robust" if robust else "_photo" if photometric else "") + "_host")
    check(fn(*((pa, pix(b), S) if b is not None else (pa, F)), *settings, *io))
    return out, st, stats, photo


def align_host(a: np.ndarray, b: Optional[np.ndarray], model_in: np.ndarray, status_in: Optional[np.ndarray], levels: int,
               iterations: int, model: int, min_share: float, photometric: bool = False):
    """oflk_align_refine_host[_u8] (b given: contiguous (S, H, W) arrays of one type) or oflk_align_sequence_host[_u8] (b None:
    a holds the S + 1 frames); contiguous float32 (S, 6 | 9) models and optional int32 (S,) statuses in; (model (S, nc) float32,
    status (S,) int32, stats (S, 4) float64) out.  photometric: the _photo_ forms, with (g, b) (S, 2) float32 as a fourth output"""
    r = _align_host(a, b, model_in, status_in, levels, iterations, model, min_share, photometric, None)
    return r if photometric else r[:3]


def align_robust_host(a: np.ndarray, b: Optional[np.ndarray], model_in: np.ndarray, status_in: Optional[np.ndarray], levels: int,
                      iterations: int, model: int, min_share: float, robust_delta: float, photometric: bool = False):
    """oflk_align_refine_robust_host[_u8] (b given) or oflk_align_sequence_robust_host[_u8] (b None), with align_host's arrays;
    (model (S, nc) float32, status (S,) int32, stats (S, 8) float64, photo (S, 2) float32) out, photo (1, 0) without
    photometric.  The C call checks robust_delta."""
    return _align_host(a, b, model_in, status_in, levels, iterations, model, min_share, photometric, robust_delta)


def align_weights(d_a: int, d_b: int, S: int, H: int, W: int, model: int, robust_delta: float, d_model: int, d_photo: int,
                  d_weights: int, u8: bool = False, stream: int = 0) -> None:
    """oflk_align_weights on device pointers: d_a, d_b [S][H][W], d_model [S][6 | 9] float32, d_photo [S][2] float32 or 0,
    d_weights [S][H][W] float32; asynchronous"""
    check(lib().oflk_align_weights(d_a or None, d_b or None, int(bool(u8)), int(S), int(H), int(W), int(model), float(robust_delta),
                                   d_model or None, d_photo or None, d_weights or None, stream))


def align_weights_host(a: np.ndarray, b: np.ndarray, model_in: np.ndarray, model: int, robust_delta: float,
                       photo: Optional[np.ndarray] = None) -> np.ndarray:
    """oflk_align_weights_host[_u8]: contiguous (S, H, W) arrays of one type, float32 (S, 6 | 9) models, optional float32 (S, 2)
    gains and biases -> (S, H, W) float32"""
    S, H, W = a.shape
    out = np.empty((S, H, W), np.float32)
    pa, fn = pixels(a, "oflk_align_weights_host")
    check(fn(pa, pix(b), int(S), int(H), int(W), int(model), float(robust_delta), ptr(model_in), None if photo is None else ptr(photo),
             ptr(out)))
    return out


class Tracker:
    """Online sparse KLT tracker (oflk_tracker_*): K = max_corners slots on `device`, one frame per push.  Pointers are raw
    device addresses, stream a hipStream_t handle; the rows are those of the statement in include/oflk.h.  The arguments
    are the C ABI's and are checked there; creation makes no device call."""

    def __init__(self, device: int, H: int, W: int, u8: bool, max_corners: int, detect_every: int, levels: int = 3,
                 window_size: int = 5, iters: int = 3, alpha: float = 0.01, beta: float = 0.5, max_residual: float = 4.0,
                 quality_level: float = 0.01, min_distance: float = 10.0):
        self._h = _vp()
        self.H, self.W, self.u8, self.K = int(H), int(W), bool(u8), int(max_corners)
        trk = Tracking(int(levels), int(window_size), int(iters), float(alpha), float(beta), float(max_residual), float(quality_level),
                       float(min_distance), int(max_corners), int(detect_every))
        check(lib().oflk_tracker_create(ctypes.byref(self._h), int(device), int(H), int(W), int(bool(u8)), *trk))

    _owned = True   # False: the handle belongs to a Stabilizer

    @classmethod
    def _borrowed(cls, handle, H: int, W: int, u8: bool, max_corners: int) -> "Tracker":
        t = cls.__new__(cls)
        t._h, t._owned = handle, False
        t.H, t.W, t.u8, t.K = int(H), int(W), bool(u8), int(max_corners)
        return t

    def close(self) -> None:
        if self._h and self._owned:
            lib().oflk_tracker_destroy(self._h)
        self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return int(lib().oflk_tracker_workspace_bytes(self._h))

    @property
    def frame_index(self) -> int:
        return int(lib().oflk_tracker_frame_index(self._h))

    def reset(self, stream: int = 0) -> None:
        check(lib().oflk_tracker_reset(self._h, stream))

    def push_device(self, d_frame: int, stream: int = 0) -> None:
        check(lib().oflk_tracker_push_device(self._h, d_frame or None, stream))

    def row_device(self) -> Tuple[int, int, int, int, int, int]:
        """device addresses of xy, visible, born, birth, residual, detected of the last pushed frame"""
        p = [_vp() for _ in range(6)]
        check(lib().oflk_tracker_row_device(self._h, *[ctypes.byref(q) for q in p]))
        return tuple(int(q.value) for q in p)

    def _row(self):
        K = self.K
        return (np.empty((K, 2), np.float32), np.empty(K, np.uint8), np.empty(K, np.uint8), np.empty(K, np.int32),
                np.empty(K, np.float32), np.empty(1, np.int32))

    @staticmethod
    def _row_args(r):
        return ptr(r[0]), r[1].ctypes.data, r[2].ctypes.data, r[3].ctypes.data_as(_i32p), ptr(r[4]), r[5].ctypes.data_as(_i32p)

    def read_row(self, stream: int = 0):
        """(xy (K, 2) float32, visible (K,) uint8, born (K,) uint8, birth (K,) int32, residual (K,) float32, detected int)"""
        r = self._row()
        check(lib().oflk_tracker_read_row(self._h, *self._row_args(r), stream))
        return r[:5] + (int(r[5][0]),)

    def push(self, frame: np.ndarray):
        """a contiguous host frame (H, W) of the tracker's element type in, the row (as read_row) out"""
        want = np.uint8 if self.u8 else np.float32
        if not (isinstance(frame, np.ndarray) and frame.dtype == want and frame.shape == (self.H, self.W)
                and frame.flags["C_CONTIGUOUS"]):
            raise ValueError(f"expected a contiguous {np.dtype(want).name} frame of shape {(self.H, self.W)}")
        r = self._row()
        check(lib().oflk_tracker_push(self._h, frame.ctypes.data, *self._row_args(r)))
        return r[:5] + (int(r[5][0]),)

    def add_points(self, pts, stream: int = 0) -> None:
        """(n, 2) host points (x, y), n >= 1"""
        p = np.ascontiguousarray(pts, np.float32)
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"points must be an (n, 2) array of (x, y), got shape {p.shape}")
        check(lib().oflk_tracker_add_points(self._h, ptr(p), int(p.shape[0]), stream))

    def set_motion(self, model: int, hypotheses: int = 256, threshold: float = 1.0, seed: int = 0) -> None:
        """the motion row of the pushes from the next one on; model -1: off"""
        check(lib().oflk_tracker_set_motion(self._h, int(model), int(hypotheses), float(threshold), int(seed)))

    def motion_device(self) -> Tuple[int, int, int]:
        """device addresses of model [6], inlier [K], counts [3] of the last push's motion row"""
        p = [_vp() for _ in range(3)]
        check(lib().oflk_tracker_motion_device(self._h, *[ctypes.byref(q) for q in p]))
        return tuple(int(q.value) for q in p)

    def read_motion(self, stream: int = 0):
        """(model (6,) float32, inlier (K,) uint8, counts (3,) int32) of the last push's motion row"""
        m, inl, cnt = np.empty(6, np.float32), np.empty(self.K, np.uint8), np.empty(3, np.int32)
        check(lib().oflk_tracker_read_motion(self._h, ptr(m), inl.ctypes.data, cnt.ctypes.data_as(_i32p), stream))
        return m, inl, cnt


class Stabilizer:
    """Online fixed-lag stabiliser (oflk_stabilizer_*): a Tracker with its motion row on, a delay line of radius + 1 frames
    and a ring of step models on `device`; the push of frame t emits frame t - radius, flush() the rest.  Pointers are raw
    device addresses, stream a hipStream_t handle.  The arguments are the C ABI's and are checked there; creation makes no
    device call.  `tracker` is the inner Tracker (owned by the stabiliser): its rows and motion, add_points."""

    def __init__(self, device: int, H: int, W: int, u8: bool, max_corners: int, detect_every: int, model: int, weights: np.ndarray,
                 hypotheses: int = 256, threshold: float = 1.0, seed: int = 0, levels: int = 3, window_size: int = 5, iters: int = 3,
                 alpha: float = 0.01, beta: float = 0.5, max_residual: float = 4.0, quality_level: float = 0.01,
                 min_distance: float = 10.0, channels: int = 0, order: int = 0, nv12: bool = False, siting: int = 0):
        self._h = _vp()
        self.H, self.W, self.u8, self.K = int(H), int(W), bool(u8), int(max_corners)
        self.channels = int(channels)   # 0: grey frames (H, W); 3 or 4: packed uint8 frames (H, W, channels), luma to the tracker
        self.nv12 = bool(nv12)          # NV12 uint8 frames (3H/2, W), their Y plane to the tracker
        w = np.ascontiguousarray(weights, np.float64)
        self.radius = int(w.size) - 1
        trk = Tracking(int(levels), int(window_size), int(iters), float(alpha), float(beta), float(max_residual), float(quality_level),
                       float(min_distance), int(max_corners), int(detect_every))
        tail = (*trk, *Fit(int(model), int(hypotheses), float(threshold), int(seed)), *Window(w, self.radius).args)
        if self.nv12 and (not self.u8 or self.channels):
            raise ValueError("NV12 frames are uint8 and have no channel axis")
        if self.channels and not self.nv12 and not self.u8:
            raise ValueError("colour frames must be uint8 (float32 colour is not offered)")
        self.layout = (FrameLayout("_nv12", (int(siting),)) if self.nv12 else
                       FrameLayout("_packed", (self.channels, int(order))) if self.channels else FrameLayout())
        create = getattr(lib(), "oflk_stabilizer_create" + self.layout.suffix)
        check(create(ctypes.byref(self._h), int(device), int(H), int(W), *(self.layout.args or (int(bool(u8)),)), *tail))
        self.tracker = Tracker._borrowed(_vp(lib().oflk_stabilizer_tracker(self._h)), H, W, u8, max_corners)

    def close(self) -> None:
        if self._h:
            self.tracker.close()
            lib().oflk_stabilizer_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return int(lib().oflk_stabilizer_workspace_bytes(self._h))

    @property
    def lag(self) -> int:
        return int(lib().oflk_stabilizer_lag(self._h))

    @property
    def frame_index(self) -> int:
        return int(lib().oflk_stabilizer_frame_index(self._h))

    def reset(self, stream: int = 0) -> None:
        check(lib().oflk_stabilizer_reset(self._h, stream))

    def push_device(self, d_frame: int, d_out: int, d_inside: int = 0, stream: int = 0) -> int:
        """the index of the frame written to d_out (and d_inside), or -1 when nothing was"""
        e = ctypes.c_int(-1)
        check(lib().oflk_stabilizer_push_device(self._h, d_frame or None, d_out or None, d_inside or None, ctypes.byref(e), stream))
        return int(e.value)

    def flush_device(self, d_out: int, d_inside: int = 0, stream: int = 0) -> Tuple[int, int]:
        """(first, count) of the frames written to d_out [radius][H][W] (and d_inside)"""
        first, count = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().oflk_stabilizer_flush_device(self._h, d_out or None, d_inside or None, ctypes.byref(first), ctypes.byref(count),
                                                 stream))
        return int(first.value), int(count.value)

    def correction_device(self) -> Tuple[int, int]:
        """device addresses of correction [rows][6] float32 and map [rows][6] float64 of the last emission"""
        c, m = _vp(), _vp()
        check(lib().oflk_stabilizer_correction_device(self._h, ctypes.byref(c), ctypes.byref(m)))
        return int(c.value), int(m.value)

    def _dtype(self):
        return np.uint8 if self.u8 else np.float32

    def _shape(self):
        return self.layout.frame_shape(self.H, self.W)

    def push(self, frame: np.ndarray, inside: bool = False):
        """a contiguous host frame (H, W) -- (H, W, channels) for a colour stabiliser -- of the stabiliser's element type in;
        (emitted index or -1, frame of that shape or None, correction (6,) float32 or None, inside (H, W) uint8 or None) out"""
        if not (isinstance(frame, np.ndarray) and frame.dtype == self._dtype() and frame.shape == self._shape()
                and frame.flags["C_CONTIGUOUS"]):
            raise ValueError(f"expected a contiguous {np.dtype(self._dtype()).name} frame of shape {self._shape()}")
        out, corr = np.empty(self._shape(), self._dtype()), np.empty(6, np.float32)
        ins = np.empty((self.H, self.W), np.uint8) if inside else None
        e = ctypes.c_int(-1)
        check(lib().oflk_stabilizer_push(self._h, frame.ctypes.data, out.ctypes.data, None if ins is None else ins.ctypes.data,
                                         ptr(corr), ctypes.byref(e)))
        if e.value < 0:
            return -1, None, None, None
        return int(e.value), out, corr, ins

    def flush(self, inside: bool = False):
        """(first, frames (count, H, W) or (count, H, W, channels), correction (count, 6) float32, inside (count, H, W) uint8
        or None)"""
        n = max(self.radius, 1)
        out, corr = np.empty((n,) + self._shape(), self._dtype()), np.empty((n, 6), np.float32)
        ins = np.empty((n, self.H, self.W), np.uint8) if inside else None
        first, count = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().oflk_stabilizer_flush(self._h, out.ctypes.data, None if ins is None else ins.ctypes.data, ptr(corr),
                                          ctypes.byref(first), ctypes.byref(count)))
        c = int(count.value)
        return int(first.value), out[:c], corr[:c], None if ins is None else ins[:c]
