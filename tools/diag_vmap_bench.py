#!/usr/bin/env python3
"""Times the device voxel map (gfbe_vmap_add_points / associate / associate + linearize) against a single-thread C++ host
restatement on std::unordered_map (tests/vmap_host_shim.cpp, hmap_*; its linearisation is the CPU oracle's gfo_lio_linearize), at
2 000 keypoints on maps of 2e4, 2e5 and 2e6 points. Host clock around the synchronised call, the two legs alternating, seven
repetitions after a warm-up; median and max - min per leg. Writes profiles/vmap_bench.txt.

    python tools/diag_vmap_bench.py [--sizes 20000,200000,2000000] [--out profiles/vmap_bench.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _gfbe_import import gf      # noqa: E402
import oracle_lib      # noqa: E402

abi = gf.abi
PD = C.POINTER(C.c_double)
N_KP, REPS = 2000, 7
IOPT = ("max_num_points_in_voxel", "voxel_neighborhood", "max_number_neighbors", "min_number_neighbors", "threshold_voxel_occupancy",
        "num_closest_neighbors", "max_num_residuals")
DOPT = ("size_voxel_map", "min_distance_points", "max_distance", "max_dist_to_plane_icp", "power_planarity", "weight_alpha", "weight_neighborhood")


def _p(a):
    return a.ctypes.data_as(PD)


def build_shim():
    so = os.path.join(ROOT, "tests", "_build", "libvmap_host_shim_o3.so")
    src = os.path.join(ROOT, "tests", "vmap_host_shim.cpp")
    deps = [src, os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_vmap.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-ffp-contract=off", "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.hmap_create.restype = C.c_void_p
    return lib


def scene(n_map, rng):
    """A ground plane with 4 mm of noise sampled at 195 points / m^2, 1.3 n_map samples: min_distance_points rejects about a quarter,
    so that about n_map points stay in the map (the count is reported); keypoints on the same plane."""
    side = np.sqrt(1.3 * n_map / 195.0)
    def plane(n):
        p = rng.uniform(-side / 2, side / 2, (n, 3))
        p[:, 2] = rng.normal(0, 0.004, n)
        return p
    return plane(int(1.3 * n_map)), plane(N_KP), [plane(N_KP) for _ in range(REPS + 1)]


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def register_leg(sizes, out):
    """gfbe_vmap_register (ct = 1, default options) beside the host-driven loop it replaces: per outer iteration one synchronised
    associate and lm_iterations + 1 synchronised linearize calls, the counts taken from the register call's own summary."""
    be = gf.Backend(device=0)
    lines = ["registration loop: gfbe_vmap_register (one host wait) against the same number of synchronised associate / linearize calls, %d keypoints, ct = 1, ms" % N_KP,
             "median [max - min] of %d repetitions after a warm-up; host clock around the call(s)" % REPS, ""]
    pb = np.array([0.0, 0.0, 1.0, 0, 0, 0, 1.0])
    pe = np.array([0.02, 0.01, 1.0, 0, 0, np.sin(0.005), np.cos(0.005)])
    for n_map in sizes:
        rng = np.random.default_rng(n_map)
        world, kp, _ = scene(n_map, rng)
        raw = np.ascontiguousarray(kp - [0, 0, 1.0])
        alpha = np.ascontiguousarray(rng.uniform(0, 1, N_KP))
        dm = be.voxel_map(max(1 << 12, n_map // 4))
        dm.add_points(world)
        sb, se = pb + [0.01, -0.01, 0.02, 0, 0, 0, 0], pe + [0.01, -0.01, 0.02, 0, 0, 0, 0]
        _, _, sm = dm.register(1, raw, alpha, sb, se, pb[:3], pb[3:])
        K = sm["outer_iterations"]
        calls = [(1, int(sm["lm_iterations"][k]) + 1) for k in range(K)]

        def host_driven():
            for _, nl in calls:
                dm.associate(1, raw, alpha, sb, se)
                for _ in range(nl):
                    dm.linearize(1, 31.6, sb, se)
        tr, th = [], []
        for i in range(REPS + 1):
            x, y = timed(lambda: dm.register(1, raw, alpha, sb, se, pb[:3], pb[3:])), timed(host_driven)
            if i:
                tr.append(x)
                th.append(y)
        lines.append("map %d points: %d outer iterations, n_res %d, %d associate + %d linearize calls" % (dm.size()["n_points"], K, sm["n_res"][0], K, sum(c[1] for c in calls)))
        lines.append("  register %8.3f [%6.3f]   host-driven calls %8.3f [%6.3f]" % (np.median(tr), max(tr) - min(tr), np.median(th), max(th) - min(th)))
        print("\n".join(lines[-2:]), flush=True)
        dm.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,200000,2000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vmap_bench.txt"))
    ap.add_argument("--register", action="store_true", help="the registration loop leg (written to profiles/vreg_bench.txt)")
    a = ap.parse_args()
    if a.register:
        return register_leg([int(s) for s in a.sizes.split(",")], os.path.join(ROOT, "profiles", "vreg_bench.txt"))
    shim, orc = build_shim(), oracle_lib.load()
    be = gf.Backend(device=0)
    lines = ["voxel map: device (gfbe_vmap_*) against a single-thread host restatement (std::unordered_map), %d keypoints, ms" % N_KP,
             "median [max - min] of %d alternating repetitions after a warm-up; host clock around the synchronised call" % REPS, ""]
    pb = np.array([0.0, 0.0, 1.0, 0, 0, 0, 1.0])
    pe = np.array([0.02, 0.01, 1.0, 0, 0, np.sin(0.005), np.cos(0.005)])
    for n_map in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(n_map)
        world, kp, adds = scene(n_map, rng)
        raw = np.ascontiguousarray(kp - [0, 0, 1.0])      # (near enough to the body frame of both poses)
        alpha = np.ascontiguousarray(rng.uniform(0, 1, N_KP))
        dm = be.voxel_map(max(1 << 12, n_map // 4))
        o = {k: getattr(dm.opt, k) for k in IOPT + DOPT}
        iopt, dopt = np.array([o[k] for k in IOPT], np.int32), np.array([o[k] for k in DOPT], np.float64)
        hm = C.c_void_p(shim.hmap_create(iopt.ctypes.data_as(C.POINTER(C.c_int)), _p(dopt)))
        dm.add_points(world)
        shim.hmap_add_points(hm, len(world), _p(np.ascontiguousarray(world)), 0)
        sz, hs = dm.size(), (C.c_int * 2)()
        shim.hmap_size(hm, hs)
        assert (sz["n_voxels"], sz["n_points"]) == (hs[0], hs[1]) and not sz["overflow"], (sz, list(hs))
        R = o["max_num_residuals"]
        src, pts, nrm, off, alo, w = np.zeros(R, np.int32), np.zeros((R, 3)), np.zeros((R, 3)), np.zeros(R), np.zeros(R), np.zeros(R)
        nres = [0]

        def h_assoc():
            nres[0] = shim.hmap_associate(hm, 1, N_KP, _p(raw), _p(alpha), _p(pb), _p(pe), 0, src.ctypes.data_as(C.POINTER(C.c_int)), _p(pts), _p(nrm),
                                          _p(off), _p(alo), _p(w))

        def h_both():
            h_assoc()
            n = nres[0]
            abi.lio_linearize(orc.lib, "gfo_", None, 1, pts[:n], nrm[:n], off[:n], alo[:n], w[:n], 10.0, pb, pe, blocks=False)

        def d_add(p):
            dm.add_points(p)
            dm.size()      # (add_points does not wait: the size call synchronises)

        legs = {"add_points": (lambda i: d_add(adds[i]), lambda i: shim.hmap_add_points(hm, N_KP, _p(np.ascontiguousarray(adds[i])), 0)),
                "associate": (lambda i: dm.associate(1, raw, alpha, pb, pe), lambda i: h_assoc()),
                "associate+linearize": (lambda i: (dm.associate(1, raw, alpha, pb, pe), dm.linearize(1, 10.0, pb, pe)), lambda i: h_both())}
        lines.append("map %d points (%d voxels), n_res %d" % (sz["n_points"], sz["n_voxels"], dm.associate(1, raw, alpha, pb, pe)["n_res"]))
        for name in ("associate", "associate+linearize", "add_points"):
            dev, host = legs[name]
            td, th = [], []
            for i in range(REPS + 1):      # repetition 0 is the warm-up
                x, y = timed(lambda: dev(i)), timed(lambda: host(i))
                if i:
                    td.append(x)
                    th.append(y)
            lines.append("  %-20s device %8.3f [%6.3f]   host %8.3f [%6.3f]" % (name, np.median(td), max(td) - min(td), np.median(th), max(th) - min(th)))
            print(lines[-1], flush=True)
        dm.close()
        shim.hmap_destroy(hm)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
