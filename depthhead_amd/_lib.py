"""ctypes binding of libdepthhead_hip.so (include/depthhead_hip.h).

There is NO CPU fallback: if the HIP library is missing or fails to load, importing the product
path raises.  `load()` never builds anything by itself; `depthhead_amd.build.build()` (called by
`__graft_entry__.build()`) does.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdepthhead_hip.so")

DH_OK = 0
ERRORS = {-1: "DH_EINVAL", -2: "DH_EFOREST", -3: "DH_EHIP", -4: "DH_ENOMEM", -5: "DH_ESIZE", -6: "DH_ESTATE"}

POSE_DTYPE = np.dtype([("mid_point", "<f4", (3,)), ("reserved", "<u4"), ("rotation", "<f8", (3,))], align=True)
assert POSE_DTYPE.itemsize == 40
# dh_support: vote support of a pose (head bounding box of the supporting windows' centres, counts, mass)
SUPPORT_DTYPE = np.dtype([("x", "<u4"), ("y", "<u4"), ("width", "<u4"), ("height", "<u4"), ("windows", "<u4"), ("hits", "<u4"),
                          ("mass", "<u8"), ("total_mass", "<u8")], align=True)
assert SUPPORT_DTYPE.itemsize == 40
SUPPORT_RADIUS = 30   # DH_SUPPORT_RADIUS
# dh_head: one detected head of a frame (dh_predict_heads*): its pose and its vote support
HEAD_DTYPE = np.dtype([("pose", POSE_DTYPE), ("support", SUPPORT_DTYPE)], align=True)
assert HEAD_DTYPE.itemsize == 80 and HEAD_DTYPE.fields["support"][1] == 40
MAX_HEADS = 4          # DH_MAX_HEADS
HEADS_SUPPRESS = 2     # DH_HEADS_SUPPRESS (guess-grid cells)
# dh_head_track: one track slot of a multi-head tracker (dh_multi_tracker_*): id (0 = free), counters and its last head
TRACK_DTYPE = np.dtype([("id", "<u4"), ("age", "<u4"), ("hits", "<u4"), ("misses", "<u4"), ("head", HEAD_DTYPE)], align=True)
assert TRACK_DTYPE.itemsize == 96 and TRACK_DTYPE.fields["head"][1] == 16
MAX_TRACKS = 8             # DH_MAX_TRACKS
TRACK_GATE = 100           # DH_TRACK_GATE (cells = mm)
TRACK_MAX_MISSES = 3       # DH_TRACK_MAX_MISSES
# dh_rig_person / dh_rig_track: a person fused from the heads of a rig's cameras, and one track slot of a rig tracker
RIG_PERSON_DTYPE = np.dtype([("views", "<u8"), ("mass", "<u8"), ("cell", "<i4", (3,)), ("n_views", "<u4"), ("world", "<f4", (3,)),
                             ("id", "<u4"), ("best_cam", "<u4"), ("best_head", "<u4")], align=True)
assert RIG_PERSON_DTYPE.itemsize == 56
RIG_TRACK_DTYPE = np.dtype([("id", "<u4"), ("age", "<u4"), ("hits", "<u4"), ("misses", "<u4"), ("person", RIG_PERSON_DTYPE)],
                           align=True)
assert RIG_TRACK_DTYPE.itemsize == 72 and RIG_TRACK_DTYPE.fields["person"][1] == 16
RIG_MAX_CAMERAS = 64       # DH_RIG_MAX_CAMERAS
RIG_MAX_PERSONS = 16       # DH_RIG_MAX_PERSONS
RIG_MAX_TRACKS = 16        # DH_RIG_MAX_TRACKS
RIG_FUSE_GATE = 100        # DH_RIG_FUSE_GATE (cells = mm)


# dh_render_instance: one posed mesh of a render call (dh_render_depth*)
RENDER_INSTANCE_DTYPE = np.dtype([("frame", "<u4"), ("mesh", "<u4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"),
                                  ("flags", "<u4")], align=True)
assert RENDER_INSTANCE_DTYPE.itemsize == 64
RENDER_HEAD = 1            # DH_RENDER_HEAD
RENDER_MAX_SIZE = 16384    # DH_RENDER_MAX_SIZE


class RenderParams(C.Structure):
    """dh_render_params"""
    _fields_ = [("noise_amplitude", C.c_uint32), ("reserved0", C.c_uint32), ("hole_probability", C.c_double), ("seed", C.c_uint64),
                ("reserved", C.c_uint64 * 2)]


# dh_fit_record: what one fitted instance reports (dh_fit_depth*)
FIT_RECORD_DTYPE = np.dtype([("points", "<u4"), ("steps", "<u4"), ("status", "<u4"), ("reserved", "<u4"), ("sum_r2_fixed", "<i8")],
                            align=True)
assert FIT_RECORD_DTYPE.itemsize == 24
FIT_MAX_POINTS = 32768     # DH_FIT_MAX_POINTS
FIT_MAX_EXTENT = 4096      # DH_FIT_MAX_EXTENT (mm)


class FitParams(C.Structure):
    """dh_fit_params (`lam` is the header's `lambda`)"""
    _fields_ = [("coarse_iterations", C.c_uint32), ("iterations", C.c_uint32), ("gate", C.c_double * 2), ("lam", C.c_double),
                ("min_points", C.c_uint32), ("reserved0", C.c_uint32), ("reserved", C.c_uint64 * 2)]


# dh_fit_track_state / dh_fit_track_record: a fit tracker's per-camera state and what one step reports for a camera
FIT_TRACK_STATE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("t_prev", "<f4", (3,)), ("tracked", "<u4"),
                                  ("have_prev", "<u4"), ("age", "<u4"), ("lost", "<u4")], align=True)
assert FIT_TRACK_STATE_DTYPE.itemsize == 76
FIT_TRACK_RECORD_DTYPE = np.dtype([("instance", RENDER_INSTANCE_DTYPE), ("fit", FIT_RECORD_DTYPE), ("status", "<u4"), ("age", "<u4"),
                                   ("lost", "<u4"), ("reserved", "<u4")], align=True)
assert FIT_TRACK_RECORD_DTYPE.itemsize == 104 and FIT_TRACK_RECORD_DTYPE.fields["fit"][1] == 64
FIT_TRACK_ANGLES = 120     # DH_FIT_TRACK_ANGLES


class FitTrackParams(C.Structure):
    """dh_fit_track_params"""
    _fields_ = [("iterations_tracked", C.c_uint32), ("keep_points", C.c_uint32), ("rms_max", C.c_double), ("max_jump", C.c_double),
                ("conf_num", C.c_uint32), ("conf_den", C.c_uint32), ("min_windows", C.c_uint32), ("max_coast", C.c_uint32),
                ("reserved", C.c_uint64 * 2)]


# dh_shape_record: what one shape step reports for a subject (dh_fit_shape*)
SHAPE_RECORD_DTYPE = np.dtype([("delta", "<f8", (8,)), ("points", "<u4"), ("instances", "<u4"), ("status", "<u4"), ("reserved", "<u4"),
                               ("sum_r2_fixed", "<i8")], align=True)
assert SHAPE_RECORD_DTYPE.itemsize == 88
SHAPE_MAX_FIELDS = 8       # DH_SHAPE_MAX_FIELDS
SHAPE_MAX_SUBJECTS = 256   # DH_SHAPE_MAX_SUBJECTS
SHAPE_SKIP = 0xFFFFFFFF    # DH_SHAPE_SKIP
SHAPE_MAX_FIELD = 256      # DH_SHAPE_MAX_FIELD (mm)
SHAPE_MAX_GATE = 256       # DH_SHAPE_MAX_GATE (mm)
SHAPE_MAX_TERMS = 1 << 23  # DH_SHAPE_MAX_TERMS
# dh_subject_state: one subject of a dh_fit_subjects (its coefficients, counters, flags)
SUBJECT_STATE_DTYPE = np.dtype([("coeffs", "<f8", (8,)), ("applied", "<u4"), ("rejected", "<u4"), ("flags", "<u4"), ("zero_normals", "<u4")],
                               align=True)
assert SUBJECT_STATE_DTYPE.itemsize == 80
SUBJECTS_MAX_TRIS = 131072  # DH_SUBJECTS_MAX_TRIS
SUBJECT_CLAMPED, SUBJECT_NONFINITE = 1, 2   # DH_SUBJECT_*
# dh_surface_record: what one surface step reports for a subject (dh_fit_surface_subjects*)
SURFACE_RECORD_DTYPE = np.dtype([("status", "<u4"), ("points", "<u4"), ("instances", "<u4"), ("observed", "<u4"), ("clamped", "<u4"),
                                 ("rejected", "<u4"), ("sum_r2_fixed", "<i8"), ("max_abs", "<f8")], align=True)
assert SURFACE_RECORD_DTYPE.itemsize == 40
SURFACE_OK, SURFACE_FEW_POINTS = 0, 1       # DH_SURFACE_*
SURFACE_MAX_OFFSET = 64        # DH_SURFACE_MAX_OFFSET (mm)
SURFACE_MAX_SCALE = 64         # DH_SURFACE_MAX_SCALE
SURFACE_MAX_CELLS = 1 << 22    # DH_SURFACE_MAX_CELLS
SURFACE_MAX_ITERATIONS = 256   # DH_SURFACE_MAX_ITERATIONS
SURFACE_LDS_POINTS = 10112     # the solve keeps its two buffers in LDS up to this many vertices (dh_fit.h)


class SurfaceParams(C.Structure):
    """dh_surface_params"""
    _fields_ = [("gate", C.c_double), ("min_cos2", C.c_double), ("mu", C.c_double), ("eps", C.c_double), ("min_count", C.c_uint32),
                ("min_points", C.c_uint32), ("iterations", C.c_uint32), ("reserved0", C.c_uint32), ("reserved", C.c_uint64 * 2)]


# dh_ident_record: what identification reports for one fitted instance (dh_fit_identify_subjects*)
IDENT_RECORD_DTYPE = np.dtype([("status", "<u4"), ("best", "<u4"), ("second", "<u4"), ("eligible", "<u4"), ("points_best", "<u4"),
                               ("points_second", "<u4"), ("sum_r2_best", "<i8"), ("sum_r2_second", "<i8")], align=True)
assert IDENT_RECORD_DTYPE.itemsize == 40
IDENT_OK, IDENT_SKIPPED, IDENT_NO_CANDIDATE, IDENT_FAR, IDENT_AMBIGUOUS = 0, 1, 2, 3, 4   # DH_IDENT_*
IDENT_UNKNOWN = 0xFFFFFFFF         # DH_IDENT_UNKNOWN (== DH_SHAPE_SKIP)
IDENT_MAX_PAIRS = 1 << 22          # DH_IDENT_MAX_PAIRS
IDENT_DEFAULT_MAX_RMS = 1.68       # DH_IDENT_DEFAULT_MAX_RMS (mm)
IDENT_VIEWS_DEFAULT_MAX_RMS = 2.58  # DH_IDENT_VIEWS_DEFAULT_MAX_RMS (mm)


class IdentParams(C.Structure):
    """dh_ident_params (`lam` is the header's `lambda`)"""
    _fields_ = [("iterations", C.c_uint32), ("min_points", C.c_uint32), ("gate", C.c_double), ("lam", C.c_double), ("max_rms", C.c_double),
                ("min_ratio", C.c_double), ("reserved", C.c_uint64 * 3)]


# dh_subject_track_state / dh_subject_track_record: a subject fit tracker's per-camera state and what one step reports for a camera
SUBJECT_TRACK_STATE_DTYPE = np.dtype([("fit", FIT_TRACK_STATE_DTYPE), ("subject", "<u4"), ("wait", "<u4"), ("tries", "<u4"),
                                      ("bound_age", "<u4")], align=True)
assert SUBJECT_TRACK_STATE_DTYPE.itemsize == 92
SUBJECT_TRACK_RECORD_DTYPE = np.dtype([("track", FIT_TRACK_RECORD_DTYPE), ("ident", IDENT_RECORD_DTYPE), ("subject", "<u4"), ("model", "<u4"),
                                       ("identified", "<u4"), ("tries", "<u4")], align=True)
assert SUBJECT_TRACK_RECORD_DTYPE.itemsize == 160 and SUBJECT_TRACK_RECORD_DTYPE.fields["ident"][1] == 104


class SubjectTrackParams(C.Structure):
    """dh_subject_track_params"""
    _fields_ = [("retry", C.c_uint32), ("max_tries", C.c_uint32), ("reserved", C.c_uint64 * 2)]


# dh_view_instance / dh_view_fit_record: one world-posed model seen by several cameras, and what its fit reports (dh_fit_depth_views*)
VIEW_INSTANCE_DTYPE = np.dtype([("first_cam", "<u4"), ("model", "<u4"), ("views", "<u8"), ("R", "<f4", (9,)), ("t", "<f4", (3,)),
                                ("scale", "<f4"), ("flags", "<u4")], align=True)
assert VIEW_INSTANCE_DTYPE.itemsize == 72
VIEW_FIT_RECORD_DTYPE = np.dtype([("points", "<u4"), ("steps", "<u4"), ("status", "<u4"), ("reserved", "<u4"), ("sum_r2_fixed", "<i8"),
                                  ("views_used", "<u8")], align=True)
assert VIEW_FIT_RECORD_DTYPE.itemsize == 32
FIT_VIEW_TOLERANCE = 0.001  # DH_FIT_VIEW_TOLERANCE


# dh_rig_fit_state / dh_rig_fit_record: one entry of a rig fit tracker's per-rig state, and what one step reports for a slot
RIG_FIT_STATE_DTYPE = np.dtype([("id", "<u4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("t_prev", "<f4", (3,)), ("views_used", "<u8"),
                                ("tracked", "<u4"), ("have_prev", "<u4"), ("age", "<u4"), ("lost", "<u4")], align=True)
assert RIG_FIT_STATE_DTYPE.itemsize == 88 and RIG_FIT_STATE_DTYPE.fields["views_used"][1] == 64
RIG_FIT_RECORD_DTYPE = np.dtype([("instance", VIEW_INSTANCE_DTYPE), ("fit", VIEW_FIT_RECORD_DTYPE), ("id", "<u4"), ("status", "<u4"),
                                 ("age", "<u4"), ("lost", "<u4"), ("person", "<u4"), ("reserved", "<u4")], align=True)
assert RIG_FIT_RECORD_DTYPE.itemsize == 128 and RIG_FIT_RECORD_DTYPE.fields["fit"][1] == 72
RIG_FIT_NO_PERSON = 0xFFFFFFFF   # dh_rig_fit_record.person of an unseen entry


# dh_rig_subject_state / dh_rig_subject_record: an entry of a rig subject fit tracker's state, and what one step reports for a slot
RIG_SUBJECT_STATE_DTYPE = np.dtype([("fit", RIG_FIT_STATE_DTYPE), ("subject", "<u4"), ("wait", "<u4"), ("tries", "<u4"), ("bound_age", "<u4")],
                                   align=True)
assert RIG_SUBJECT_STATE_DTYPE.itemsize == 104
RIG_SUBJECT_RECORD_DTYPE = np.dtype([("track", RIG_FIT_RECORD_DTYPE), ("ident", IDENT_RECORD_DTYPE), ("subject", "<u4"), ("model", "<u4"),
                                     ("identified", "<u4"), ("tries", "<u4")], align=True)
assert RIG_SUBJECT_RECORD_DTYPE.itemsize == 184 and RIG_SUBJECT_RECORD_DTYPE.fields["ident"][1] == 128


class RigFitTrackParams(C.Structure):
    """dh_rig_fit_track_params"""
    _fields_ = [("iterations_tracked", C.c_uint32), ("keep_points", C.c_uint32), ("rms_max", C.c_double), ("max_jump", C.c_double),
                ("max_coast", C.c_uint32), ("max_misses", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class ShapeParams(C.Structure):
    """dh_shape_params (`lam` is the header's `lambda`)"""
    _fields_ = [("gate", C.c_double), ("lam", C.c_double), ("min_points", C.c_uint32), ("reserved0", C.c_uint32),
                ("reserved", C.c_uint64 * 2)]


# dh_calib_record: what one calibration step reports for a camera (dh_fit_calibrate_views*)
CALIB_RECORD_DTYPE = np.dtype([("V", "<f4", (9,)), ("u", "<f4", (3,)), ("points", "<u4"), ("pairs", "<u4"), ("status", "<u4"),
                               ("reserved", "<u4"), ("sum_r2_fixed", "<i8"), ("delta", "<f8", (6,))], align=True)
assert CALIB_RECORD_DTYPE.itemsize == 120
CALIB_SKIP = 0xFFFFFFFF    # DH_CALIB_SKIP
CALIB_ARM_UNIT = 64        # DH_CALIB_ARM_UNIT (mm)
CALIB_MAX_ARM = 2048       # DH_CALIB_MAX_ARM (mm)


class CalibParams(C.Structure):
    """dh_calib_params (`lam` is the header's `lambda`)"""
    _fields_ = [("gate", C.c_double), ("lam", C.c_double), ("pivot", C.c_double * 3), ("min_points", C.c_uint32),
                ("reserved0", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class RigTrackParams(C.Structure):
    """dh_rig_track_params"""
    _fields_ = [("max_heads", C.c_int32), ("radius", C.c_uint32), ("fuse_gate", C.c_uint32), ("gate", C.c_uint32),
                ("max_misses", C.c_uint32)]


class MultiTrackParams(C.Structure):
    """dh_multi_track_params"""
    _fields_ = [("max_heads", C.c_int32), ("radius", C.c_uint32), ("gate", C.c_uint32), ("max_misses", C.c_uint32)]


class ForestDesc(C.Structure):
    _fields_ = [("n_trees", C.c_uint32), ("roots", C.c_void_p), ("n_nodes", C.c_uint32), ("nodes", C.c_void_p),
                ("n_leaves", C.c_uint32), ("leaf_prob", C.c_void_p), ("off_begin", C.c_void_p),
                ("rot_begin", C.c_void_p), ("offsets", C.c_void_p), ("rotations", C.c_void_p)]


class Params(C.Structure):
    _fields_ = [("stepwidth", C.c_uint32), ("subimage_width", C.c_uint32), ("subimage_height", C.c_uint32),
                ("gaussian_sigma", C.c_float), ("meanshift_iterations", C.c_uint32)]


class Timing(C.Structure):
    _fields_ = [("traverse_ms", C.c_float), ("vote_ms", C.c_float), ("cluster_ms", C.c_float),
                ("total_ms", C.c_float), ("n_frames", C.c_uint32), ("boxsum_ms", C.c_float),
                ("emit_ms", C.c_float), ("reserved", C.c_uint32)]


# every symbol include/depthhead_hip.h declares
EXPORTS = [
    "dh_last_error", "dh_version", "dh_forest_create", "dh_forest_destroy", "dh_forest_info",
    "dh_predictor_create", "dh_predictor_destroy", "dh_predictor_update_sigma", "dh_predictor_sigma",
    "dh_predict_batch", "dh_predict_batch_device", "dh_predict_batch_rle", "dh_biwi_decode_depth_device", "dh_host_alloc", "dh_host_free", "dh_predictor_reserve", "dh_predictor_set_forking", "dh_patch_grid",
    "dh_predict_mask", "dh_predict_mask_device", "dh_hough_image", "dh_hough_image_device", "dh_build_hough_image", "dh_build_hough_image_device",
    "dh_predict_from2dhough", "dh_predict_from2dhough_device",
    "dh_biwi_decode_depth", "dh_biwi_parse_cal", "dh_biwi_parse_pose",
    "dh_graph_capture", "dh_graph_launch", "dh_graph_destroy",
    "dh_set_profiling", "dh_get_timing", "dh_debug_enable", "dh_debug_leaf_indices", "dh_debug_patch_flags",
    "dh_debug_grids", "dh_debug_guesses", "dh_debug_votes", "dh_debug_meanshift", "dh_debug_hit_counts", "dh_debug_geometry", "dh_debug_tile_shifts", "dh_debug_window_totals",
    "dh_trainer_create", "dh_trainer_destroy", "dh_trainer_add_frames", "dh_trainer_fit", "dh_trainer_stats", "dh_forest_export",
    "dh_cameras_create", "dh_cameras_destroy", "dh_predict_batch_cameras", "dh_predict_batch_cameras_device",
    "dh_tracker_create", "dh_tracker_destroy", "dh_tracker_reset", "dh_tracker_step", "dh_tracker_step_device",
    "dh_tracker_state", "dh_tracker_capture",
    "dh_predict_batch_support", "dh_predict_batch_support_device", "dh_predict_batch_cameras_support",
    "dh_predict_batch_cameras_support_device", "dh_tracker_step_support", "dh_tracker_step_support_device",
    "dh_predict_heads", "dh_predict_heads_device", "dh_predict_heads_cameras", "dh_predict_heads_cameras_device",
    "dh_multi_tracker_create", "dh_multi_tracker_destroy", "dh_multi_tracker_reset", "dh_multi_tracker_step",
    "dh_multi_tracker_step_device", "dh_multi_tracker_state", "dh_multi_tracker_capture",
    "dh_rig_create", "dh_rig_destroy", "dh_rig_tracker_create", "dh_rig_tracker_destroy", "dh_rig_tracker_reset",
    "dh_rig_tracker_step", "dh_rig_tracker_step_device", "dh_rig_tracker_state", "dh_rig_tracker_capture",
    "dh_mesh_create", "dh_mesh_destroy", "dh_mesh_info", "dh_renderer_create", "dh_renderer_destroy",
    "dh_renderer_set_profiling", "dh_renderer_timing",
    "dh_render_depth", "dh_render_depth_cameras", "dh_render_depth_device", "dh_render_depth_cameras_device",
    "dh_fit_model_create", "dh_fit_model_destroy", "dh_fit_model_info", "dh_fit_params_default", "dh_fitter_create",
    "dh_fitter_destroy", "dh_fit_depth", "dh_fit_depth_cameras", "dh_fit_depth_device", "dh_fit_depth_cameras_device",
    "dh_fit_track_params_default", "dh_fit_tracker_angles", "dh_fit_tracker_create", "dh_fit_tracker_destroy", "dh_fit_tracker_reset",
    "dh_fit_tracker_state", "dh_fit_tracker_step_poses", "dh_fit_tracker_step_poses_device", "dh_fit_tracker_step",
    "dh_fit_tracker_step_device",
    "dh_fit_basis_create", "dh_fit_basis_destroy", "dh_fit_basis_info", "dh_shape_params_default", "dh_fit_shape", "dh_fit_shape_cameras",
    "dh_fit_shape_device", "dh_fit_shape_cameras_device", "dh_fit_shape_views", "dh_fit_shape_views_device",
    "dh_calib_params_default", "dh_fit_calibrate_views", "dh_fit_calibrate_views_device",
    "dh_fit_views_create", "dh_fit_views_destroy", "dh_fit_views_info", "dh_fit_depth_views", "dh_fit_depth_views_device",
    "dh_rig_fit_track_params_default", "dh_rig_fit_tracker_create", "dh_rig_fit_tracker_destroy", "dh_rig_fit_tracker_reset",
    "dh_rig_fit_tracker_state", "dh_rig_fit_tracker_step_persons", "dh_rig_fit_tracker_step_persons_device", "dh_rig_fit_tracker_step",
    "dh_rig_fit_tracker_step_device",
    "dh_fit_subjects_create", "dh_fit_subjects_destroy", "dh_fit_subjects_info", "dh_fit_subjects_model", "dh_fit_subjects_set_coeffs",
    "dh_fit_subjects_state", "dh_fit_subjects_read", "dh_fit_subjects_update", "dh_fit_subjects_update_device", "dh_fit_shape_subjects", "dh_fit_shape_subjects_cameras",
    "dh_fit_shape_subjects_device", "dh_fit_shape_subjects_cameras_device", "dh_fit_depth_carried_device",
    "dh_fit_depth_cameras_carried_device",
    "dh_fit_subjects_create_surface", "dh_fit_subjects_set_offsets", "dh_fit_subjects_read_offsets", "dh_fit_surface_params_default",
    "dh_fit_surface_subjects", "dh_fit_surface_subjects_cameras", "dh_fit_surface_subjects_device", "dh_fit_surface_subjects_cameras_device",
    "dh_fit_ident_params_default", "dh_fit_identify_subjects", "dh_fit_identify_subjects_cameras", "dh_fit_identify_subjects_device",
    "dh_fit_identify_subjects_cameras_device",
    "dh_fit_ident_views_params_default", "dh_fit_identify_subjects_views", "dh_fit_identify_subjects_views_device",
    "dh_subject_track_params_default", "dh_subject_fit_tracker_create", "dh_subject_fit_tracker_destroy", "dh_subject_fit_tracker_reset",
    "dh_subject_fit_tracker_state", "dh_subject_fit_tracker_info", "dh_subject_fit_tracker_set_enrolled", "dh_subject_fit_tracker_bind",
    "dh_subject_fit_tracker_step_poses", "dh_subject_fit_tracker_step_poses_device", "dh_subject_fit_tracker_step",
    "dh_subject_fit_tracker_step_device",
    "dh_rig_subject_fit_tracker_create", "dh_rig_subject_fit_tracker_destroy", "dh_rig_subject_fit_tracker_reset",
    "dh_rig_subject_fit_tracker_state", "dh_rig_subject_fit_tracker_info", "dh_rig_subject_fit_tracker_set_enrolled",
    "dh_rig_subject_fit_tracker_bind", "dh_rig_subject_fit_tracker_step_persons", "dh_rig_subject_fit_tracker_step_persons_device",
    "dh_rig_subject_fit_tracker_step", "dh_rig_subject_fit_tracker_step_device",
]


class TrainParams(C.Structure):
    _fields_ = [("stepwidth", C.c_uint32), ("subimage_width", C.c_uint32), ("subimage_height", C.c_uint32),
                ("max_depth", C.c_uint32), ("n_trees", C.c_uint32), ("subset_per_tree", C.c_uint32),
                ("subrect_feature_scale", C.c_double), ("features_per_node", C.c_uint32), ("min_subset_size", C.c_uint32),
                ("steepness", C.c_double), ("seed", C.c_uint64)]


class TrainStats(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("pool_size", C.c_uint64), ("pool_positives", C.c_uint64), ("neg_det", C.c_uint64),
                ("levels", C.c_uint32), ("reserved", C.c_uint32)]


class DepthheadError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


_lib = None


def load():
    """Load the HIP library; raises if it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if os.environ.get("DH_NO_TORCH_PRELOAD") != "1":
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  Two HIP runtimes in one process do
        # not both see the GPU, so when torch is installed it is imported FIRST: the loader then
        # resolves this library's libamdhip64.so.7 to the copy torch already mapped.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    path = os.environ.get("DH_LIB_PATH") or LIB_PATH   # tools/ only: the -DDH_PROFILING_KNOBS twin
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the depthhead_amd product path has no CPU fallback)")
    lib = C.CDLL(path)
    for name in EXPORTS:
        fn = getattr(lib, name)   # AttributeError if an export is missing
        fn.restype = C.c_int
    lib.dh_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def check(rc: int):
    if rc != DH_OK:
        raise DepthheadError(rc, load().dh_last_error().decode("utf-8", "replace"))


def vp(x):
    """void* from a numpy array, an int address (device pointer) or None."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    return C.c_void_p(int(x))


def ref(struct):
    """byref(struct), or None for None: a params argument that may be absent."""
    return None if struct is None else C.byref(struct)


def intrinsics(K_or_cameras):
    """(suffix of the call's name, its argument) for one K ([3, 3] or an `IntrinsicMatrix`) or a `tracking.Cameras` table."""
    cams = getattr(K_or_cameras, "_h", None)
    if cams is not None:
        return "_cameras", cams
    return "", held(np.ascontiguousarray(getattr(K_or_cameras, "mat", K_or_cameras), dtype=np.float32).reshape(9))


def stream_of(device, stream=None) -> int:
    """The stream handle a _device form is ordered on: `stream`, or for None the current torch stream of `device` (an ordinal
    or a torch.device)."""
    if stream is not None:
        return int(stream)
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def held(array: np.ndarray):
    """void* from a numpy array that carries the array, which so lives as long as the pointer does: for an array made on the way."""
    p = C.c_void_p(array.ctypes.data)
    p.array = array
    return p


class _Handle:
    """Owner of library handles.  `close()` -- also at the end of a `with` block and at garbage collection, where what it
    raises is swallowed -- destroys each handle of `_handles`, (attribute, destroy function) pairs, once and in that order."""
    _handles: tuple = ()

    def close(self):
        for attr, destroy in self._handles:
            h = getattr(self, attr, None)
            if h and h.value:
                getattr(self._lib, destroy)(h)
                setattr(self, attr, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def pinned_empty(shape, dtype) -> np.ndarray:
    """A numpy array in page-locked host memory (dh_host_alloc): frame batches filled in place are uploaded by
    asynchronous DMA at PCIe speed.  The memory is released when the array (and every view of it) is gone."""
    import weakref
    lib = load()
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    ptr = C.c_void_p()
    check(lib.dh_host_alloc(C.c_size_t(max(1, count * dt.itemsize)), C.byref(ptr)))
    raw = (C.c_uint8 * max(1, count * dt.itemsize)).from_address(ptr.value)
    weakref.finalize(raw, lib.dh_host_free, C.c_void_p(ptr.value))
    return np.frombuffer(raw, dtype=dt, count=count).reshape(shape)
