#!/usr/bin/env python3
"""Times the dense RGB-D map (gfbe_dmap_*) host to host on the synthetic corridor of synth_dmap.DenseScene, 1 000 and 5 000 keyframes of
up to 2 852 points (depth_dist 10, depth_boundary 10 on 640 x 480): one gfbe_dmap_add_keyframe into the filled map, gfbe_dmap_rebuild
at corrected poses, gfbe_dmap_filter on the rebuilt cloud and, for scale, gfbe_lc4_solve on a graph of the same number of keyframes.
Median and max - min of `--reps` repetitions after a warm-up. An insert and a rebuild return without waiting, so each is timed with
the gfbe_dmap_size call behind it (one wait and a 64-byte read). Every figure comes with the bytes the operation must move (pool
and cloud rows once, no table traffic) as a fraction of the HBM peak of 8 TB/s.

The rank rounds' share of a rebuild is the difference to the same rebuild under rebuild_cap 1 (no rank launch; it also keeps and
writes fewer points, so the figure is an upper bound). The comparison figure is the sequential walk of the model compiled for one host
thread (hdmap_insert of tests/dmap_host_shim.cpp on std::unordered_map): a restatement by this project, not the reference's PCL
octree, of which no build exists here. Writes profiles/dmap_bench.txt.

    python tools/diag_dmap_bench.py [--reps 15] [--sizes 1000,5000] [--out profiles/dmap_bench.txt]
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
from _gfbe_import import gf      # noqa: E402

HBM_PEAK = 8.0e12
KEYS = ("t", "ypr", "sequence", "fixed", "loop_i", "loop_c", "loop_meas")


def host_shim():
    out = os.path.join(ROOT, "tests", "_build", "libdmap_host_shim.so")
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                        "-o", out, os.path.join(ROOT, "tests", "dmap_host_shim.cpp")], check=True)
    lib = C.CDLL(out)
    lib.hdmap_new.restype = C.c_void_p
    lib.hdmap_free.argtypes = [C.c_void_p]
    lib.hdmap_insert.argtypes = [C.c_void_p, gf.abi.PD, gf.abi.PD, C.c_int, gf.abi.PF, C.c_int, C.c_int] + [C.c_double] * 4 + [gf.abi.PF]
    return lib


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), max(t) - min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", default="1000,5000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmap_bench.txt"))
    a = ap.parse_args()
    be = gf.Backend(device=0)
    lg = gf.abi.LoopGraph(be.lib, "gfbe_", be.ctx)
    shim = host_shim()
    lines = ["gfbe_dmap_*, host to host, median ms (max - min) of %d repetitions after a warm-up; bytes moved as a fraction of 8 TB/s" % a.reps]
    for n_kf in [int(s) for s in a.sizes.split(",")]:
        scene = gf.synth_dmap.DenseScene(seed=n_kf)
        extra = a.reps + 2
        poses = scene.poses(n_kf + extra, dwell=6)
        frames = [scene.keyframe(p) for p in poses]
        total = sum(len(f[0]) for f in frames)
        fixed = scene.corrected(poses[:n_kf])
        maps = {cap: be.dense_map(total, n_kf + extra, ex_cam=scene.ex_cam, rebuild_cap=cap) for cap in (5, 1)}
        dm = maps[5]
        t0 = time.perf_counter()
        for m in maps.values():
            for k in range(n_kf):
                m.add_keyframe(poses[k], *frames[k])
        sz = dm.size()
        maps[1].size()
        fill_ms = (time.perf_counter() - t0) * 1e3 / 2
        lines.append("%d keyframes, %d points offered, %d stored, %d voxels (filling the map: %.0f ms, %.3f ms per keyframe with the generator's arrays ready)"
                     % (n_kf, sum(len(f[0]) for f in frames[:n_kf]), sz["n_stored"], sz["n_voxels"], fill_ms, fill_ms / n_kf))
        # rebuild (the corrected and the original poses alternate), with and without rank rounds
        flip = [0]

        def rebuild(m):
            flip[0] ^= 1
            m.rebuild(fixed if flip[0] else poses[:n_kf])
            return m.size()
        r5, s5 = timed(lambda: rebuild(dm), a.reps)
        r1, s1 = timed(lambda: rebuild(maps[1]), a.reps)
        dm.rebuild(fixed)
        sz = dm.size()
        by = sz["n_stored"] * (12 + 3 + 4) + sz["n_cloud"] * (12 + 3 + 4 + 4)
        lines.append("  rebuild            %9.3f (%6.3f)  %9d pool points -> %9d cloud points, %8d voxels; %6.1f MB, %.2f %% of peak"
                     % (r5, s5, sz["n_stored"], sz["n_cloud"], sz["n_voxels"], by / 1e6, 100 * by / (r5 * 1e-3) / HBM_PEAK))
        lines.append("  rebuild, cap 1     %9.3f (%6.3f)  no rank rounds: the four rounds of cap 5 cost at most %.3f ms, %.0f %% of the rebuild" % (r1, s1, r5 - r1, 100 * (r5 - r1) / r5))
        # the filter on the rebuilt cloud
        f1, fs1 = timed(lambda: dm.filter(compact=False), a.reps)
        nf = dm.size()
        res = dm.filter(compact=True)
        f2, fs2 = timed(lambda: dm.filter(compact=True), max(3, a.reps // 3))
        by = sz["n_cloud"] * (12 * 3 + 1)
        lines.append("  filter, flags only %9.3f (%6.3f)  kept %d of %d; fast path (own cell > 10 points) %d = %.2f %%, walk %d; %6.1f MB, %.2f %% of peak (includes the %d-byte download)"
                     % (f1, fs1, res["n_keep"], sz["n_cloud"], nf["n_fast"], 100.0 * nf["n_fast"] / max(1, sz["n_cloud"]), sz["n_cloud"] - nf["n_fast"], by / 1e6,
                        100 * by / (f1 * 1e-3) / HBM_PEAK, sz["n_cloud"]))
        lines.append("  filter, compacted  %9.3f (%6.3f)  with the kept points' xyz and rgb downloaded (%.1f MB over the host link)" % (f2, fs2, res["n_keep"] * 15 / 1e6))
        # one insert into the filled map
        k = [n_kf]

        def insert():
            dm.add_keyframe(poses[k[0]], *frames[k[0]])
            k[0] += 1
            return dm.size()
        i1, is1 = timed(insert, a.reps)
        lines.append("  add_keyframe       %9.3f (%6.3f)  %d points offered per call; %.1f KB, %.4f %% of peak"
                     % (i1, is1, len(frames[n_kf][0]), len(frames[n_kf][0]) * 30 / 1e3, 100 * len(frames[n_kf][0]) * 30 / (i1 * 1e-3) / HBM_PEAK))
        # for scale: the 4-DoF solve on a graph of as many keyframes
        g = gf.synth.loop_graph(n=n_kf, n_loop=16, seed=n_kf + 16, laps=4, yaw_bias=0.05, scale_err=0.02)
        l1, ls1 = timed(lambda: lg.solve(*[g[q] for q in KEYS]), a.reps)
        lines.append("  gfbe_lc4_solve     %9.3f (%6.3f)  %d keyframes, 16 loop edges (for scale)" % (l1, ls1, n_kf))
        # the sequential walk, compiled, one host thread: the rebuild's work on the downloaded lists
        lists = [dm.keyframe(q)["pts"] for q in range(n_kf)]
        h = shim.hdmap_new()
        ex = np.ascontiguousarray(scene.ex_cam)
        world = np.zeros((max(len(p) for p in lists) + 1, 3), np.float32)
        t0 = time.perf_counter()
        kept = 0
        for q in range(n_kf):
            kept += shim.hdmap_insert(h, np.ascontiguousarray(fixed[q]).ctypes.data_as(gf.abi.PD), ex.ctypes.data_as(gf.abi.PD), len(lists[q]), lists[q].ctypes.data_as(gf.abi.PF), 5, 0,
                                      -10000.0, 0.01, -0.5, 2.0, world.ctypes.data_as(gf.abi.PF))
        walk = (time.perf_counter() - t0) * 1e3
        shim.hdmap_free(h)
        lines.append("  host walk          %9.0f            one thread, std::unordered_map, the rebuild only (kept %d: %s the device's cloud); this project's restatement, not PCL"
                     % (walk, kept, "equals" if kept == sz["n_cloud"] else "DIFFERS from"))
        for m in maps.values():
            m.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
