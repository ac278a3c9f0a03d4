"""ctypes binding of the product library csrc/libgfbe.so (HIP, gfx950) — the host-side mirror of
Estimator::optimization() (estimator.cpp:2951-3698) over the C ABI of include/gfbe.h.

There is deliberately no CPU path here: if the library is missing, a symbol is missing, or no GPU
is visible, the call raises BackendError (gfbe_status GFBE_NO_DEVICE). The CPU oracle lives in
oracle/ and is only ever loaded by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi, signatures

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
# GFBE_LIB: an alternative build of the library (tools/diag_variants.py compares kernel variants built side by side)
_SO = os.environ.get("GFBE_LIB") or os.path.join(_CSRC, "libgfbe.so")

# Every symbol include/gfbe.h / include/gfbe_rccl.h declares: the keys of the signature tables (checked against the headers by
# tests/test_abi.py on CPU).
EXPORTS = ["gfbe_" + name for name in signatures.GFBE]
RCCL_EXPORTS = ["gfbe_rccl_" + name for name in signatures.RCCL]
LC6_EXPORTS = ["gfbe_lc6_" + name for name in signatures.LC6]      # include/gfbe_lc6.h: symbols of the product library
KLT_EXPORTS = ["gfbe_klt_" + name for name in signatures.KLT]      # include/gfbe_klt.h: likewise
DET_EXPORTS = ["gfbe_det_" + name for name in signatures.DET]      # include/gfbe_det.h: likewise
OBS_EXPORTS = ["gfbe_obs_" + name for name in signatures.OBS]      # include/gfbe_obs.h: likewise
KFD_EXPORTS = ["gfbe_kfd_" + name for name in signatures.KFD]      # include/gfbe_kfd.h: likewise
PNP_EXPORTS = ["gfbe_pnp_" + name for name in signatures.PNP]      # include/gfbe_pnp.h: likewise
EQ_EXPORTS = ["gfbe_eq_" + name for name in signatures.EQ]         # include/gfbe_eq.h: likewise
GATE_EXPORTS = ["gfbe_gate_" + name for name in signatures.GATE]   # include/gfbe_gate.h: likewise


class BackendError(RuntimeError):
    pass


def lib_path():
    return _SO


def sources():
    return sorted(os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".cpp")))


DIAG_SO = os.path.join(_CSRC, "libgfbe_diag.so")


def build_native(force=False, verbose=False, out=None, extra_flags=None, fp_contract="off", diag=False):
    """hipcc --offload-arch=gfx950 -> csrc/libgfbe.so (cross-compiles without a GPU). Every source is compiled to its own
    object (in parallel, only when it is older than the source or a header) and the objects are linked: a one-file change
    rebuilds in seconds. `out` / `extra_flags` / `fp_contract`: side-by-side variant builds (tools/diag_variants.py)."""
    from concurrent.futures import ThreadPoolExecutor
    if diag:
        out = out or DIAG_SO
        extra_flags = list(extra_flags or []) + ["-DGFBE_DIAG=1"]
    so = out or os.path.join(_CSRC, "libgfbe.so")
    srcs = sources()
    hdrs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".hpp"))]
    hdrs += [os.path.join(os.path.dirname(_HERE), "include", h) for h in ("gfbe.h", "gfbe_lc6.h", "gfbe_klt.h", "gfbe_det.h", "gfbe_obs.h", "gfbe_kfd.h", "gfbe_pnp.h")]
    hdrs.append(os.path.join(os.path.dirname(_HERE), "include", "gfbe_eq.h"))
    hdrs.append(os.path.join(os.path.dirname(_HERE), "include", "gfbe_gate.h"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = os.environ.get("GFBE_EXTRA_FLAGS", "").split() if extra_flags is None else list(extra_flags)
    cflags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=" + fp_contract, "-munsafe-fp-atomics",
              "-Wall", "-Wno-unused-function", "-pthread", "-I", os.path.join(os.path.dirname(_HERE), "include")] + flags
    tag = "default" if (out is None and not flags and fp_contract == "off") else os.path.splitext(os.path.basename(so))[0]
    odir = os.path.join(_CSRC, "build", tag)
    os.makedirs(odir, exist_ok=True)
    stamp = os.path.join(odir, "flags.txt")
    if not os.path.exists(stamp) or open(stamp).read() != " ".join(cflags):
        force = True
    hnew = max(os.path.getmtime(h) for h in hdrs)
    jobs, objs = [], []
    for src in srcs:
        obj = os.path.join(odir, os.path.basename(src) + ".o")
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hnew):
            jobs.append([hipcc] + cflags + ["-c", src, "-o", obj])
    if not jobs and os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(o) for o in objs):
        return so

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", so] + objs)
    with open(stamp, "w") as f:
        f.write(" ".join(cflags))
    return so


_RCCL_SO = os.path.join(_CSRC, "libgfbe_rccl.so")


def build_rccl_hook(force=False, verbose=False):
    """csrc/rccl/gfbe_rccl_hook.cpp -> csrc/libgfbe_rccl.so (the native all-reduce hook of include/gfbe_rccl.h; links librccl)."""
    src = os.path.join(_CSRC, "rccl", "gfbe_rccl_hook.cpp")
    deps = [src, os.path.join(os.path.dirname(_HERE), "include", "gfbe_rccl.h")]
    if not force and os.path.exists(_RCCL_SO) and all(os.path.getmtime(_RCCL_SO) >= os.path.getmtime(d) for d in deps):
        return _RCCL_SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", "/opt/rocm/include",
           "-o", _RCCL_SO, src, "-L/opt/rocm/lib", "-lrccl", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return _RCCL_SO


class Backend(abi.CApi):
    prefix = "gfbe_"

    def __init__(self, device=0, options=None, so=None):
        _SO = so or globals()["_SO"]          # (so: another build of the library, e.g. DIAG_SO)
        if not os.path.exists(_SO):
            raise BackendError("HIP extension %s is missing: run __graft_entry__.build() (no CPU fallback)" % _SO)
        self.lib = abi.bind(abi.bind(abi.bind(abi.bind(abi.bind(C.CDLL(_SO), "gfbe_"), abi.LC6_PREFIX), abi.KLT_PREFIX), abi.DET_PREFIX), abi.OBS_PREFIX)
        abi.bind(self.lib, abi.KFD_PREFIX)
        abi.bind(self.lib, abi.PNP_PREFIX)
        abi.bind(self.lib, abi.EQ_PREFIX)
        abi.bind(self.lib, abi.GATE_PREFIX)
        self.opt = options or abi.default_options()
        self.ctx = C.c_void_p()
        rc = self.lib.gfbe_create(C.byref(self.ctx), int(device), C.byref(self.opt))
        if rc != abi.OK:
            raise BackendError("gfbe_create(device=%d) failed with status %d (%s)" % (device, rc, self._err()))
        self.create_note = (self.lib.gfbe_create_note(self.ctx) or b"").decode()   # (a remark, not an error: e.g. speculative_linearization switched off for a batch)
        self.head = self.ctx
        self.device = device
        self._cb = None

    def _err(self):
        try:
            return (self.lib.gfbe_last_error(self.ctx) or b"").decode()
        except Exception:
            return "?"

    def check(self, rc, what):
        if rc not in (abi.OK, abi.NO_CONVERGENCE):
            raise BackendError("gfbe_%s failed with status %d: %s" % (what, rc, self._err()))
        return rc

    def _call(self, fn, *args, **kw):
        """fn(lib, "gfbe_", ctx, ...) of abi.py; its RuntimeError becomes a BackendError that carries gfbe_last_error."""
        try:
            return fn(self.lib, "gfbe_", self.ctx, *args, **kw)
        except RuntimeError as e:
            raise BackendError("%s: %s" % (e, self._err()))

    def close(self):
        if self.ctx:
            self.lib.gfbe_destroy(self.ctx)
            self.ctx = C.c_void_p()
        hook = getattr(self, "_rccl_hook", None)      # (the native all-reduce hook's communicator lives as long as the context)
        if hook is not None:
            hook.close()
            self._rccl_hook = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def version(self):
        return self.lib.gfbe_version().decode()

    def set_stream(self, stream_ptr):
        self.check(self.lib.gfbe_set_stream(self.ctx, C.c_void_p(stream_ptr)), "set_stream")

    # ---- line landmarks (gfbe_line_eval / gfbe_line_refine)
    def line_eval(self, pose, ex_cam, orth, obs, sqrt_info=400.0, robustify=True):
        """lineProjectionFactor at n (pose, line, observation) triples: r [n][2], J_pose / J_ex [n][2][7], J_orth [n][2][4], cost."""
        return self._call(abi.line_eval, pose, ex_cam, orth, obs, sqrt_info, robustify)

    def line_refine(self, windows, sqrt_info=400.0, cauchy_scale=1.0, max_num_iterations=8):
        """onlyLineOpt() + removeLineOutlier() of each line window (dicts as synth_line.LineScenario makes them, or
        abi.LineWindowHolder): per window plucker [n][6] (ineligible lines unchanged), keep [n], summary."""
        return self._call(abi.line_refine, windows, sqrt_info, cauchy_scale, max_num_iterations)

    def line_reduce(self, windows, mode=abi.LINE_REDUCE_SOLVE, sqrt_info=400.0, huber_width=1.0, mu=0.0, want=abi.LINE_REDUCE_KEYS):
        """The line loops of optimizationwithLine() linearised and reduced onto the 72 pose / extrinsic dims (dims 0..71 of the dense
        block): per window H [72][72], g, U, bp, cost, n_eligible, n_failed and the per-line records Vinv, bl, W, failed. For device-
        resident tables: line_tables(...).reduce(...)."""
        return self._call(abi.line_reduce, windows, mode, sqrt_info, huber_width, mu, want)

    def line_reduce_v(self, windows, mode=abi.LINE_REDUCE_SOLVE, sqrt_info=400.0, huber_width=1.0, mu=0.0, want=abi.LINE_REDUCE_KEYS_V):
        """line_reduce with the record V (the lower triangle of V_l without mu) beside Vinv, bl, W, failed: what line_step takes."""
        return self._call(abi.line_reduce_v, windows, mode, sqrt_info, huber_width, mu, want)

    def line_step(self, windows, records, y_p, v_p, rest, radius, sqrt_info=400.0, huber_width=1.0, mu=0.0, want=abi.LINE_STEP_KEYS):
        """The step half of a joint iteration over the line blocks (gfbe_line_step): back-substitution, the lines' dogleg shares, the
        dogleg coefficients from rest + shares, the candidate lines / poses and the candidate line cost. records: line_reduce_v's result.
        For device-resident tables: line_tables(...).keep_records() / reduce_v / step / commit."""
        return self._call(abi.line_step, windows, records, y_p, v_p, rest, radius, sqrt_info, huber_width, mu, want)

    def line_tables(self, n_tables=1, capacity=1024):
        """W device-resident line tables (abi.LineTables: FeatureManager::linefeature and its per-frame operations, gfbe_ltab_*)."""
        return self._call(abi.LineTables, n_tables, capacity)

    def voxel_map(self, voxel_capacity=1 << 16, **options):
        """A device-resident voxel map of the LiDAR odometry (abi.VoxelMap: map_incremental, lasermap_fov_segment and the scan-to-map
        association of addSurfCostFactor, gfbe_vmap_*). options: fields of gfbe_vmap_options."""
        return self._call(abi.VoxelMap, voxel_capacity, **options)

    def scan(self, capacity=1 << 16):
        """A device-resident LiDAR scan (abi.Scan: subSampleFrame, Undistort, transformPoint + gridSampling, gfbe_scan_*) for
        VoxelMap.register_scan / add_scan_handle."""
        return self._call(abi.Scan, capacity)

    def dense_map(self, point_capacity=1 << 16, keyframe_capacity=1024, **options):
        """The dense RGB-D map of the loop-closure thread held on the device (abi.DenseMap: addKeyFrame's capped insert, updatePath's
        rebuild at the corrected poses and the radius filter, gfbe_dmap_*). options: fields of gfbe_dmap_options."""
        return self._call(abi.DenseMap, point_capacity, keyframe_capacity, **options)

    def loop_graph6(self):
        """The 6-DoF loop-closure graph (include/gfbe_lc6.h) on this context."""
        return abi.LoopGraph6(self.lib, self.ctx)

    def tracker(self, n_cameras, rows, cols, point_capacity=512, **options):
        """The optical-flow tracker (abi.Tracker: image pyramids, pyramidal Lucas-Kanade and the tracking half of trackImage for
        n_cameras cameras, include/gfbe_klt.h). options: fields of gfbe_klt_options."""
        return abi.Tracker(self.lib, self.ctx, n_cameras, rows, cols, point_capacity, **options)

    def detector(self, tracker, **options):
        """Corner detection on a tracker's images and held points (abi.Detector: setMask, goodFeaturesToTrack and addPoints of
        trackImage, include/gfbe_det.h). Close it before its tracker. options: fields of gfbe_det_options."""
        return abi.Detector(self.lib, self.ctx, tracker, **options)

    def observer(self, tracker, cameras, **options):
        """The frame observations on a tracker's held points (abi.Observer: undistortedPts, ptsVelocity, the depth lookup and the
        id-ordered frame of trackImage, its hand-over to FeatureTables, removeOutliers and the prediction, include/gfbe_obs.h).
        cameras [n_cameras, 8] = fx fy cx cy k1 k2 p1 p2. Close it before its tracker. options: fields of gfbe_obs_options."""
        return abi.Observer(self.lib, self.ctx, tracker, cameras, **options)

    def describer(self, n_cameras, rows, cols, pattern, cameras, **options):
        """The keyframe descriptors (abi.KeyframeDescriber: the blurred image, FAST corners, BRIEF descriptors and keypoints_norm of a
        keyframe for n_cameras cameras and their hand-over to a LoopDatabase, include/gfbe_kfd.h). pattern [4, 256] = x1 y1 x2 y2 of
        the BRIEF pairs, cameras [n_cameras, 8] = fx fy cx cy k1 k2 p1 p2. options: fields of gfbe_kfd_options."""
        return abi.KeyframeDescriber(self.lib, self.ctx, n_cameras, rows, cols, pattern, cameras, **options)

    def equalizer(self, n_cameras, rows, cols, **options):
        """The image equalisation (abi.Equalizer: CLAHE of n_cameras uint8 images on the device, on its own or in front of a Tracker's
        push_image and a KeyframeDescriber's push_image, include/gfbe_eq.h). options: fields of gfbe_eq_options."""
        return abi.Equalizer(self.lib, self.ctx, n_cameras, rows, cols, **options)

    def sensor_gate(self, n_robots, **options):
        """The sensor gate (abi.SensorGate: the reference's per-frame stationarity and wheel-anomaly detectors and the wheel prediction of
        the newest frame for n_robots robots on the FeatureTables of the same library and context, include/gfbe_gate.h). options: fields
        of gfbe_gate_options."""
        return abi.SensorGate(self.lib, self.ctx, n_robots, **options)

    def loop_verifier(self, **options):
        """The loop verification (abi.LoopVerifier: P3P RANSAC on matched pairs, the refit on the inliers, loop_info and its acceptance
        test for a batch of problems, and findConnection's chain from window descriptors to the decision behind one wait,
        include/gfbe_pnp.h). options: fields of gfbe_pnp_options."""
        return abi.LoopVerifier(self.lib, self.ctx, **options)

    def loop_database(self, voc, keyframe_capacity=1024, descriptor_capacity=1 << 20, **options):
        """The loop database of the loop-closure thread held on the device (abi.LoopDatabase: detectLoop's vocabulary query and decision,
        addKeyFrameIntoVoc and searchByBRIEFDes, gfbe_ldb_*). voc: abi.LdbVocabHolder or its dict; options: fields of gfbe_ldb_options."""
        return self._call(abi.LoopDatabase, voc, keyframe_capacity, descriptor_capacity, **options)

    # ---- device-resident batch
    def batch_upload(self, snaps):
        if isinstance(snaps, WindowSet):      # prebuilt pointer array: no per-call Python work (the end-to-end loops of bench.py)
            holders, arr = snaps.holders, snaps.arr
        else:
            holders = [s if isinstance(s, abi.WindowHolder) else abi.WindowHolder(s) for s in snaps]
            arr = (C.POINTER(abi.Window) * len(holders))(*[C.pointer(h.c) for h in holders])
        batch = C.c_void_p()
        self.check(self.lib.gfbe_batch_upload(self.ctx, len(holders), arr, C.byref(batch)), "batch_upload")
        return Batch(self, batch, holders)

    def batch_upload_tables(self, tables, snaps):
        """snaps: window snapshots WITHOUT visual factors (state, pre-integrations, prior, flags); the landmarks of window w
        come from table w of `tables` (abi.FeatureTables on this library) without leaving the device."""
        ws = snaps if isinstance(snaps, WindowSet) else WindowSet([strip_visual(s) for s in snaps])
        batch = C.c_void_p()
        self.check(self.lib.gfbe_batch_upload_tables(self.ctx, tables.h, len(ws.holders), ws.arr, C.byref(batch)), "batch_upload_tables")
        if ws is not snaps:       # (a prebuilt WindowSet is the caller's: its holders are left as they are)
            for w, h in enumerate(ws.holders):
                h.n_feature_override = int(self.lib.gfbe_batch_feature_count(batch, w))
        return Batch(self, batch, ws.holders)

    def solve_batch(self, snaps, margin_flag=abi.MARGIN_NONE):
        b = self.batch_upload(snaps)
        try:
            b.solve(margin_flag)
            return b.download()
        finally:
            b.free()

    # ---- profiling hooks
    def profile_enable(self, on=True):
        self.check(self.lib.gfbe_profile_enable(self.ctx, int(on)), "profile_enable")

    def profile_reset(self):
        self.lib.gfbe_profile_reset(self.ctx)

    def profile(self):
        out = []
        for i in range(self.lib.gfbe_profile_count(self.ctx)):
            name = C.c_char_p()
            launches = C.c_int64()
            ms = C.c_double()
            by = C.c_double()
            self.lib.gfbe_profile_get(self.ctx, i, C.byref(name), C.byref(launches), C.byref(ms), C.byref(by))
            out.append(dict(name=name.value.decode(), launches=launches.value, total_ms=ms.value, bytes=by.value))
        return out

    def host_times(self):
        """gfbe_host_times: ms of the calling thread in the last upload (packing | the rest) and the last download (waiting for the device | unpacking)."""
        out = (C.c_double * 4)()
        self.lib.gfbe_host_times(self.ctx, out)
        return dict(upload_pack_ms=out[0], upload_rest_ms=out[1], download_wait_ms=out[2], download_unpack_ms=out[3])

    # ---- multi-GPU landmark sharding: the native hook (libgfbe_rccl.so: ncclAllReduce on the solver's stream)
    def set_allreduce_native(self, fn_ptr, user_ptr, rank, world_size):
        """fn_ptr: address of a gfbe_allreduce_fn (e.g. gfbe_rccl_allreduce), user_ptr: its handle."""
        self._cb = C.cast(fn_ptr, signatures.ALLREDUCE_FN)
        self.check(self.lib.gfbe_set_allreduce(self.ctx, self._cb, C.c_void_p(user_ptr), int(rank), int(world_size)), "set_allreduce")

    # ---- the same through a Python callable (torch.distributed in the caller; the tests' gloo flavour)
    def set_allreduce(self, fn, rank, world_size):
        CB = signatures.ALLREDUCE_FN

        def call(user, ptr, n, stream):      # (0, or 1 when the Python hook raised: the solve then returns GFBE_DEVICE_ERROR)
            try:
                fn(ptr, n, stream)
                return 0
            except Exception:                # noqa: BLE001 — an exception must not unwind through the C library
                import traceback
                traceback.print_exc()
                return 1
        self._cb = CB(call) if fn is not None else C.cast(None, CB)
        self.check(self.lib.gfbe_set_allreduce(self.ctx, self._cb, None, int(rank), int(world_size)), "set_allreduce")


def strip_visual(snap):
    """Window snapshot without its visual part (what gfbe_batch_upload_tables reads from the host)."""
    s = dict(snap)
    for k in ("vis_feature_index", "vis_imu_i", "vis_imu_j", "vis_pts_i", "vis_pts_j", "vis_vel_i", "vis_vel_j", "vis_td_i", "vis_td_j"):
        s[k] = np.zeros(0)
    s["para_feature"], s["feature_const"] = np.zeros(0), np.zeros(0, np.uint8)
    return s


class WindowSet:
    """A list of windows with the ctypes pointer array gfbe_batch_upload takes, built once (bench.py's end-to-end loops
    re-upload the same host structures every step; the library re-packs and re-copies them every time)."""

    def __init__(self, snaps):
        self.holders = [s if isinstance(s, abi.WindowHolder) else abi.WindowHolder(s) for s in snaps]
        self.arr = (C.POINTER(abi.Window) * len(self.holders))(*[C.pointer(h.c) for h in self.holders])


class DownloadBuffers:
    """Pre-allocated outputs of gfbe_batch_download for n windows of up to max_features landmarks."""

    def __init__(self, n, max_features):
        self.n = n
        self.states = (abi.State * n)()
        self.feats = np.zeros((n, max(int(max_features), 1)))
        self.fptr = (abi.PD * n)(*[abi._pd(self.feats[k]) for k in range(n)])
        self.priors = [abi.PriorHolder() for _ in range(n)]
        self.pptr = (C.POINTER(abi.Prior) * n)(*[C.pointer(p.c) for p in self.priors])
        self.sums = (abi.Summary * n)()


class Batch:
    def __init__(self, be, handle, holders):
        self.be, self.h, self.holders = be, handle, holders
        self.n = len(holders)

    def solve(self, margin_flag=abi.MARGIN_NONE):
        self.be.check(self.be.lib.gfbe_batch_solve(self.be.ctx, self.h, int(margin_flag)), "batch_solve")

    def download(self, raise_on_failure=True):
        """Per-window results. raise_on_failure=False: a window whose linear solves all failed (status NUMERICAL_FAILURE) does not
        raise — every window's own outcome is in its "status" (the batch's windows are independent)."""
        n = self.n
        states = (abi.State * n)()
        feats = [np.zeros(getattr(h, "n_feature_override", h.n_feature)) for h in self.holders]
        fptr = (abi.PD * n)(*[abi._pd(f) for f in feats])
        priors = [abi.PriorHolder() for _ in range(n)]
        pptr = (C.POINTER(abi.Prior) * n)(*[C.pointer(p.c) for p in priors])
        sums = (abi.Summary * n)()
        rc = self.be.lib.gfbe_batch_download(self.be.ctx, self.h, states, fptr, pptr, sums)
        if raise_on_failure or rc != abi.NUMERICAL_FAILURE:
            self.be.check(rc, "batch_download")
        out = []
        for k in range(n):
            out.append(dict(state=abi.state_to_dict(states[k]), feature=feats[k],
                            prior=priors[k].to_dict() if priors[k].c.valid else None,
                            summary=abi.summary_to_dict(sums[k]), perf=abi.summary_perf(sums[k]), status=sums[k].status))
        return out

    def download_into(self, bufs):
        """gfbe_batch_download into pre-allocated buffers (no per-window Python work); returns the status."""
        return self.be.check(self.be.lib.gfbe_batch_download(self.be.ctx, self.h, bufs.states, bufs.fptr, bufs.pptr, bufs.sums), "batch_download")

    def debug_timing(self, w=0):
        out = np.zeros(32)
        self.be.lib.gfbe_debug_timing(self.be.ctx, self.h, int(w), abi._pd(out))
        return out

    def debug_vector(self, which, w=0):
        out = np.zeros(abi.DENSE_DIM)
        self.be.check(self.be.lib.gfbe_debug_vector(self.be.ctx, self.h, int(w), int(which), abi._pd(out)), "debug_vector")
        return out

    def free(self):
        if self.h:
            self.be.lib.gfbe_batch_free(self.be.ctx, self.h)
            self.h = C.c_void_p()
