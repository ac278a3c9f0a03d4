"""The signature of every C entry point, declared once: name without its prefix -> (restype, [argtypes]).

GFBE holds the exports of include/gfbe.h, RCCL those of include/gfbe_rccl.h, LC6 those of include/gfbe_lc6.h (they live in the
product library under the prefix gfbe_lc6_), KLT those of include/gfbe_klt.h (prefix gfbe_klt_, likewise), DET those of
include/gfbe_det.h (prefix gfbe_det_, likewise), OBS those of include/gfbe_obs.h (prefix gfbe_obs_, likewise), KFD those of
include/gfbe_kfd.h (prefix gfbe_kfd_, likewise), PNP those of include/gfbe_pnp.h (prefix gfbe_pnp_, likewise), GFO what the CPU oracle (prefix gfo_) shares with the product. tests/test_abi.py checks GFBE and RCCL against the prototypes of their headers,
tests/test_lc6_host.py LC6, tests/test_klt_model.py KLT, tests/test_det_model.py DET, tests/test_obs_model.py OBS, tests/test_kfd_model.py KFD, tests/test_pnp_model.py PNP. abi.bind(lib, prefix) applies a
table to a loaded library; nothing else in the package assigns restype / argtypes.

Spelling: opaque handles (gfbe_ctx *, gfbe_ftab *, gfbe_batch *, ...) and void * are V, their out-parameters PV; gfbe_status is
an int32; struct pointers are pointers to the ctypes mirrors of abi.py.
"""
import ctypes as C

from .abi import (DetOptions, DmapOptions, FeatureList, FtabOptions, GnssObs, GnssState, ImuPreint, KfdOptions, KltOptions, Lc4Options, Lc6Options, LdbOptions, LdbVocab, LineReducedV,
                  LineStepped, LineWindow, ObsOptions, Options, PnpOptions, Prior, State, Summary, VmapOptions, VregOptions, VregSummary, WheelPreint, Window)

from .abi import EqOptions, GateOptions

P = C.POINTER
i, i64, d, V, PV, STR = C.c_int32, C.c_int64, C.c_double, C.c_void_p, P(C.c_void_p), C.c_char_p
PD, PF, PI, PI16, PI64, PU8, PU16, PU64, PC = P(d), P(C.c_float), P(i), P(C.c_int16), P(i64), P(C.c_uint8), P(C.c_uint16), P(C.c_uint64), P(C.c_char)
PPW, PPLW = P(P(Window)), P(P(LineWindow))          # const gfbe_window *const *, const gfbe_line_window *const *
ALLREDUCE_FN = C.CFUNCTYPE(i, V, V, i64, V)          # gfbe_allreduce_fn(user, device_ptr, n_doubles, hip_stream)

_LC4_SOLVE = (i, [V, P(Lc4Options), i, PD, PD, PI, PU8, i, PI, PI, PD, PD, PD, PD, P(Summary)])

GFBE = {
    # context
    "default_options": (None, [P(Options)]),
    "options_size": (i, []),
    "create": (i, [PV, i, P(Options)]),
    "destroy": (None, [V]),
    "last_error": (STR, [V]),
    "create_note": (STR, [V]),
    "version": (STR, []),
    "set_stream": (i, [V, V]),
    # a13: landmark bookkeeping
    "feature_count": (i, [P(FeatureList)]),
    "visual_factor_count": (i, [P(FeatureList), i]),
    "build_visual_factors": (i, [P(FeatureList), i, PI, PI, PI, PD, PD, PD, PD, PD, PD, PD, PU8]),
    "set_depth": (None, [P(FeatureList), PD, PD, PI]),
    # f1: feature tables
    "ftab_default_options": (None, [P(FtabOptions)]),
    "ftab_create": (i, [V, i, i, P(FtabOptions), PV]),
    "ftab_destroy": (None, [V, V]),
    "ftab_add_frame": (i, [V, V, PI, PI, PI, PD, PD, PI, PI, PD]),
    "ftab_remove_back_shift_depth": (i, [V, V, PD, PD]),
    "ftab_remove_back": (i, [V, V]),
    "ftab_remove_front": (i, [V, V, PI]),
    "ftab_remove_outlier": (i, [V, V, PI, PI]),
    "ftab_remove_failures": (i, [V, V]),
    "ftab_clear_depth": (i, [V, V]),
    "ftab_set_depth": (i, [V, V, PI, PD]),
    "ftab_get_depth_vector": (i, [V, V, PI, PD, PI]),
    "ftab_triangulate": (i, [V, V, PD, PD, i]),
    "ftab_check_outliers": (i, [V, V, PD, PD, i, PI, PI, PI]),
    "ftab_size": (i, [V, V, PI]),
    "ftab_download": (i, [V, V, i, PI, PI, PI, PD, PD, PD, PI, PI]),
    "batch_upload_tables": (i, [V, V, i, PPW, PV]),
    "batch_feature_count": (i, [V, i]),
    "slide_window_state": (None, [P(State), i]),
    # f3: pose graph, f3b: loop-closure graph
    "pg_eval": (i, [V, i, PD, i, PI, PD, d, d, i, PI, PD, d, PD, PD, PD, PD]),
    "pg_solve": (i, [V, i, PD, i, PI, PD, d, d, i, PI, PD, d, i, PD, P(Summary)]),
    "lc4_default_options": (None, [P(Lc4Options)]),
    "lc4_eval": (i, [V, P(Lc4Options), i, PD, PD, i, PI, PI, PU8, PD, PD, PD, PD]),
    "lc4_solve": _LC4_SOLVE,
    "lc4_solve_long": _LC4_SOLVE,
    # f3c: dense map
    "dmap_default_options": (None, [P(DmapOptions)]),
    "dmap_create": (i, [V, i, i, P(DmapOptions), PV]),
    "dmap_destroy": (None, [V, V]),
    "dmap_add_keyframe": (i, [V, V, PD, i, PF, PU8]),
    "dmap_rebuild": (i, [V, V, i, PD]),
    "dmap_filter": (i, [V, V, PU8, PI, PF, PU8]),
    "dmap_size": (i, [V, V, PI]),
    "dmap_download_cloud": (i, [V, V, PF, PU8, PI, PI]),
    "dmap_download_keyframe": (i, [V, V, i, PI, PF, PU8]),
    # f3d: loop database
    "ldb_default_options": (None, [P(LdbOptions)]),
    "ldb_create": (i, [V, P(LdbVocab), i, i64, P(LdbOptions), PV]),
    "ldb_destroy": (None, [V, V]),
    "ldb_transform": (i, [V, V, i, PU64, PI, PI, PI, PD]),
    "ldb_add_keyframe": (i, [V, V, i, PU64, PF, PF, i, PI, PI, PI, PI, PD]),
    "ldb_match": (i, [V, V, i, i, PU64, PU8, PI, PI, PI, PI, PF, PF]),
    "ldb_size": (i, [V, V, PI]),
    "ldb_download_entry": (i, [V, V, i, PI, PI, PD, PI, PU64, PF, PF]),
    # f4: LiDAR factors, voxel map, registration, scan
    "lio_linearize": (i, [V, i, i, PD, PD, PD, PD, PD, d, PD, PD, PD, PD, PD, PD, PD]),
    "vmap_default_options": (None, [P(VmapOptions)]),
    "vmap_create": (i, [V, i, P(VmapOptions), PV]),
    "vmap_destroy": (None, [V, V]),
    "vmap_add_points": (i, [V, V, i, PD, i]),
    "vmap_erase_far": (i, [V, V, PD]),
    "vmap_size": (i, [V, V, PI, PI, PI, PI]),
    "vmap_download": (i, [V, V, PI16, PI, PD]),
    "vmap_upload": (i, [V, V, i, PI16, PI, PD]),
    "vmap_associate": (i, [V, V, i, i, PD, PD, PD, PD, i, PI, PI, PD, PD, PD, PD, PD, PI, PD, PI, PI]),
    "vmap_linearize": (i, [V, V, i, d, PD, PD, PD, PD, PD, PD, PD]),
    "vmap_localizability": (i, [V, V, PD, PI]),
    "vreg_default_options": (None, [P(VregOptions)]),
    "vmap_register": (i, [V, V, P(VregOptions), i, i, PD, PD, PD, PD, PD, PD, i, PD, PD, P(VregSummary)]),
    "vmap_add_scan": (i, [V, V, i, i, PD, PD, PD, PD, i, PD]),
    "scan_create": (i, [V, i, PV]),
    "scan_destroy": (None, [V, V]),
    "scan_upload": (i, [V, V, i, PD, PD, PD, PD]),
    "scan_subsample": (i, [V, V, d]),
    "scan_undistort": (i, [V, V, i, PD, PD]),
    "scan_keypoints": (i, [V, V, i, PD, PD, d, PI]),
    "scan_size": (i, [V, V, PI, PI, PI]),
    "scan_download": (i, [V, V, i, PI, PD, PD, PD]),
    "vmap_register_scan": (i, [V, V, P(VregOptions), i, V, PD, PD, PD, PD, i, PD, PD, P(VregSummary)]),
    "vmap_add_scan_handle": (i, [V, V, i, V, PD, PD, i]),
    # f2: optional in-window factors, GNSS
    "plane_eval": (i, [V, i, PD, PD, PD, d, PD, PD, PD, PD]),
    "anchor_eval": (i, [V, i, PD, PD, d, PD, PD, PD]),
    "orientation_subset_plus": (None, [PD, PD, PU8, PD]),
    "gnss_eval": (i, [V, i, P(GnssObs), PD, P(State), P(GnssState), PD, d, PD, PD, PD, PD, PD]),
    # line landmarks and line tables
    "line_eval": (i, [V, i, PD, PD, PD, PD, d, i, PD, PD, PD, PD, PD]),
    "line_refine": (i, [V, i, PPLW, d, d, i, PD, PU8, P(Summary)]),
    "line_reduce": (i, [V, i, PPLW, i, d, d, d, P(LineReducedV)]),
    "line_step": (i, [V, i, PPLW, P(LineReducedV), d, d, d, PD, PD, PD, PD, P(LineStepped)]),
    "ltab_create": (i, [V, i, i, PV]),
    "ltab_destroy": (None, [V, V]),
    "ltab_add_frame": (i, [V, V, PI, PI, PI, PD, PI]),
    "ltab_triangulate": (i, [V, V, PD, PD]),
    "ltab_remove_back_shift": (i, [V, V, PD, PD]),
    "ltab_remove_back": (i, [V, V]),
    "ltab_remove_front": (i, [V, V, PI]),
    "ltab_refine": (i, [V, V, PD, PD, d, d, i, P(Summary)]),
    "ltab_reduce": (i, [V, V, i, PD, PD, d, d, d, P(LineReducedV)]),
    "ltab_keep_records": (i, [V, V, i]),
    "ltab_step": (i, [V, V, PD, PD, d, d, PD, PD, PD, PD, P(LineStepped)]),
    "ltab_commit": (i, [V, V, PU8]),
    "ltab_size": (i, [V, V, PI]),
    "ltab_line_count": (i, [V, V, PI]),
    "ltab_download": (i, [V, V, i, PI, PI, PI, PD, PU8, PD]),
    "ltab_upload": (i, [V, V, i, i, PI, PI, PI, PD, PU8, PD]),
    # the window solve, batches, profiling, sharding
    "eval_factors": (i, [V, P(Window), i, PD, PD, PD, PD, PD, PD, PD, PD]),
    "preintegrate_imu": (i, [V, i, PI, PD, PD, PD, PD, P(ImuPreint)]),
    "preintegrate_wheel": (i, [V, i, PI, PD, PD, PD, PD, P(WheelPreint)]),
    "solve_window": (i, [V, P(Window), i, P(State), PD, P(Prior), P(Summary)]),
    "solve_batch": (i, [V, i, PPW, i, P(State), P(PD), P(P(Prior)), P(Summary)]),
    "batch_upload": (i, [V, i, PPW, PV]),
    "batch_solve": (i, [V, V, i]),
    "batch_download": (i, [V, V, P(State), P(PD), P(P(Prior)), P(Summary)]),
    "batch_free": (None, [V, V]),
    "profile_enable": (i, [V, i]),
    "profile_count": (i, [V]),
    "profile_get": (i, [V, i, P(STR), PI64, PD, PD]),
    "profile_reset": (None, [V]),
    "host_times": (None, [V, PD]),
    "debug_timing": (i, [V, V, i, PD]),
    "debug_vector": (i, [V, V, i, i, PD]),
    "set_allreduce": (i, [V, ALLREDUCE_FN, V, i, i]),
}

RCCL = {            # prefix gfbe_rccl_
    "unique_id": (i, [PC]),
    "create": (i, [PV, PC, i, i, i]),
    "destroy": (None, [V]),
    "allreduce": (i, [V, V, i64, V]),
    "last_error": (i, [V]),
    "calls": (i64, [V]),
    "bytes": (i64, [V]),
    "comm_count": (i, [V]),
}

LC6 = {             # prefix gfbe_lc6_ (the 6-DoF loop-closure graph; symbols of the product library)
    "default_options": (None, [P(Lc6Options)]),
    "eval": (i, [V, P(Lc6Options), i, PD, PD, i, PI, PI, PU8, PD, PD, PD, PD]),
    "solve": (i, [V, P(Lc6Options), i, PD, PD, PI, PU8, i, PI, PI, PD, PD, PD, PD, P(Summary)]),
}

KLT = {             # prefix gfbe_klt_ (the optical-flow tracker; symbols of the product library)
    "default_options": (None, [P(KltOptions)]),
    "create": (i, [V, i, i, i, i, P(KltOptions), PV]),
    "destroy": (None, [V, V]),
    "push_image": (i, [V, V, PU8]),
    "set_points": (i, [V, V, PI, PF, PI, PI]),
    "track": (i, [V, V, PU8, PF, PI, PF, PF, PI, PI, PI]),
    "flow": (i, [V, V, i, i, i, PI, PF, PF, PU8, PF]),
    "download_level": (i, [V, V, i, i, i, PU8, PI16, PI]),
}

DET = {             # prefix gfbe_det_ (corner detection on a tracker's images and points; symbols of the product library)
    "default_options": (None, [P(DetOptions)]),
    "create": (i, [V, V, P(DetOptions), PV]),
    "destroy": (None, [V, V]),
    "set_next_id": (i, [V, V, PI]),
    "detect": (i, [V, V, PI, PF, PI, PI, PI]),
    "corners": (i, [V, V, i, d, i, PI, PF, PF]),
    "download": (i, [V, V, i, PF, PU8]),
}

OBS = {             # prefix gfbe_obs_ (the frame observations between the tracker and the feature tables; symbols of the product library)
    "default_options": (None, [P(ObsOptions)]),
    "create": (i, [V, V, PD, P(ObsOptions), PV]),
    "destroy": (None, [V, V]),
    "reset": (i, [V, V]),
    "observe": (i, [V, V, PD, PU16, PI, PI, PD, PI]),
    "add_frame": (i, [V, V, V, PI, PD, PI, PI, PD]),
    "remove_outliers": (i, [V, V, PI, PI, PI]),
    "predict": (i, [V, V, V, PI, PD, PD, PD, PF, PI]),
    "download_prev": (i, [V, V, i, PI, PI, PF]),
}

KFD = {             # prefix gfbe_kfd_ (the keyframe descriptors between the tracker and the loop database; symbols of the product library)
    "default_options": (None, [P(KfdOptions)]),
    "create": (i, [V, i, i, i, PI, PD, P(KfdOptions), PV]),
    "destroy": (None, [V, V]),
    "push_image": (i, [V, V, i, PU8]),
    "capture": (i, [V, V, V, i]),
    "extract": (i, [V, V, i, PI, PF, PI, PF, PU64, PI]),
    "describe": (i, [V, V, i, PI, PF, PU64, PI]),
    "add_keyframe": (i, [V, V, i, V, i, PI, PI, PI, PI, PD]),
    "match": (i, [V, V, i, V, i, PU8, PI, PI, PI, PI, PF, PF]),
    "download": (i, [V, V, i, i, PU8, PU8]),
}

_PNP_RESULTS = [PI, PI, PD, PD, PI, PI]      # n_inliers, has_loop, loop_info, pnp_pose, best, refine_flag
_PNP_MATCHED = [PI, PI, PF, PF, PU8]         # n_matched, matched_src, matched_pt, matched_pt_norm, status_pnp
PNP = {             # prefix gfbe_pnp_ (the loop verification between the loop database's matches and a loop edge; symbols of the product library)
    "default_options": (None, [P(PnpOptions)]),
    "create": (i, [V, P(PnpOptions), PV]),
    "destroy": (None, [V, V]),
    "verify": (i, [V, V, i, PI, PF, PF, PD, PD, PU8] + _PNP_RESULTS + [PI, PI, PD, PI]),
    "find_connection": (i, [V, V, V, i, i, PU64, PF, PD, PD] + _PNP_MATCHED + _PNP_RESULTS),
    "find_connection_kfd": (i, [V, V, V, i, V, i, PF, PD, PD] + _PNP_MATCHED + _PNP_RESULTS),
}

EQ = {              # prefix gfbe_eq_ (the image equalisation in front of the tracker and the keyframe descriptors; symbols of the product library;
    # include/gfbe_eq.h, checked against it by tests/test_eq_model.py)
    "default_options": (None, [P(EqOptions)]),
    "create": (i, [V, i, i, i, P(EqOptions), PV]),
    "destroy": (None, [V, V]),
    "apply": (i, [V, V, PU8, PU8]),
    "push_klt": (i, [V, V, V, PU8]),
    "push_kfd": (i, [V, V, V, i, PU8]),
    "download_lut": (i, [V, V, PU8]),
}

GATE = {            # prefix gfbe_gate_ (the sensor gate on the feature tables: stationarity, wheel anomaly, the wheel prediction; symbols of the product library;
    # include/gfbe_gate.h, checked against it by tests/test_gate_model.py)
    "default_options": (None, [P(GateOptions)]),
    "create": (i, [V, i, P(GateOptions), PV]),
    "destroy": (None, [V, V]),
    "frame": (i, [V, V, V, PI, PI, PD, PD, PI, PD, PD, PD, PD, d, PI, PI, PD, PI, PI, PI, PI, PD, PD, PD, PD, PD, PD, PD]),
    "pair_stats": (i, [V, V, V, i, PI, PD, PI, PI]),
    "corresponding": (i, [V, V, V, i, PI, PI, PI, PD, PD, PI]),
}


def _oracle(name):
    """The oracle's flavour of a shared entry point: the compute calls take `const gfbe_options *` where the product takes its
    context, the pre-integrations take no leading argument; the rest (the ftab / pg / eval calls ignore their void *) is the same."""
    res, args = GFBE[name]
    if name in ("eval_factors", "solve_window"):
        return res, [P(Options)] + args[1:]
    if name in ("preintegrate_imu", "preintegrate_wheel"):
        return res, args[1:]
    return res, args


GFO = {name: _oracle(name) for name in GFBE}
TABLES = {"gfbe_": GFBE, "gfo_": GFO, "gfbe_rccl_": RCCL, "gfbe_lc6_": LC6, "gfbe_klt_": KLT, "gfbe_det_": DET, "gfbe_obs_": OBS,
          "gfbe_kfd_": KFD, "gfbe_pnp_": PNP}
TABLES["gfbe_eq_"] = EQ
TABLES["gfbe_gate_"] = GATE


def declare(lib, prefix, table):
    """Types every entry of `table` that `lib` exports under `prefix`; the others are skipped (a test's host-only build, the oracle)."""
    for name, (res, args) in table.items():
        f = getattr(lib, prefix + name, None)
        if f is not None:
            f.restype, f.argtypes = res, args
