"""Counts, on the benchmark's eight windows and without a GPU, the work k_schur's lean form and k_vis_chunk issue per landmark tile
against the work the result needs (profiles/schur_steps_ab.txt). Tiles as in bench.py::schur_tile_pairs: a start
frame's landmarks longest track first in tiles of 64, start-frame groups {0, 1}, {2}, {3, 4, 5}, {6 .. 10}, compact panel columns
[gradient | poses from the group's first start frame].

    python tools/count_schur_steps.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _gfbe_import import gf      # noqa: E402

NF = 11
FIRST = {0: 0, 1: 0, 2: 2, 3: 3, 4: 3, 5: 3, 6: 6, 7: 6, 8: 6, 9: 6, 10: 6}


def tiles(snap):
    """[(start frame, track lengths of the occupied rows, longest first)] of a window's landmark tiles."""
    fi, ii = np.asarray(snap["vis_feature_index"]), np.asarray(snap["vis_imu_i"])
    L = len(snap["para_feature"])
    m = np.bincount(fi, minlength=L)
    start = np.zeros(L, int)
    start[fi] = ii
    out = []
    for s in range(NF):
        ms = np.sort(m[(start == s) & (m > 0)])[::-1]
        out += [(s, ms[q:q + 64]) for q in range(0, len(ms), 64)]
    return out


def block(s, m):
    return (6 * (s - FIRST[s] + int(m) + 1)) >> 4


def wave_pairs(jl):
    """Pairs (I, J), I <= J <= jl, numbered column-major and dealt 4 q + wave: [(I, J)] per wave."""
    pairs = [(i, j) for j in range(jl + 1) for i in range(j + 1)]
    return [[p for idx, p in enumerate(pairs) if idx % 4 == w] for w in range(4)]


def main():
    synth = gf.synth
    snaps = [synth.Scenario(seed=20250708 + 2 + 100 * u, n_landmarks=2000, use_wheel=True).window(1) for u in range(8)]
    n_tiles = allot = ran = loads_now = loads_need = 0
    hp_now = hp_need = mfma_now = mfma_need = path_now = path_need = pairs = diag = 0
    vis_now = vis_need = vis_single = lanes = lane_steps = 0
    for sn in snaps:
        for s, ms in tiles(sn):
            kmax, m0, rows = NF - 1 - s, int(ms[0]), len(ms)
            n_tiles += 1
            allot += kmax
            ran += min(m0, kmax)
            # d wave-loads per tile: three doubles per observation step, one wave each (parts 1 .. 3: steps part - 1 + 3 u; part 0: the
            # tenth). Today every part issues three blocks (nine loads) and part 0 three: 30; needed: the steps that ran
            loads_now += 30
            loads_need += 3 * min(m0, kmax)
            # lm_hP read: 64 rows x 24 B per block loaded (today every step the start frame allots; a part's loads beyond are clamped
            # onto its last one)
            hp_now += 64 * 24 * kmax
            hp_need += 64 * 24 * min(m0, kmax)
            # matrix-core instructions: per pair four per group of four k-steps (16 rows) up to the last occupied row
            nk = (rows + 3) // 4
            groups = (nk + 3) // 4
            jl = block(s, m0)
            wp = wave_pairs(jl)
            pairs += sum(len(p) for p in wp)
            diag += sum(i == j for p in wp for (i, j) in p)
            now = [4 * groups * len(p) for p in wp]
            need = [sum(4 for (i, j) in p for c in range(groups) if j <= block(s, ms[16 * c])) for p in wp]
            mfma_now += sum(now)
            mfma_need += sum(need)
            path_now += max(now)
            path_need += max(need)
            # k_vis_chunk: step k multiplies sixteen k-steps; needed: in groups of four, up to the last lane with k < m
            for k in range(m0):
                act = int((ms > k).sum())
                vis_now += 16
                vis_need += 4 * ((act + 15) // 16)
                vis_single += (act + 3) // 4
                lanes += act
                lane_steps += 64
    W = float(len(snaps))
    print("windows %d, tiles per window %.1f" % (len(snaps), n_tiles / W))
    print("k_schur  observation steps per tile: allotted %.2f, run %.2f" % (allot / n_tiles, ran / n_tiles))
    print("k_schur  d wave-loads per tile: today %.1f, needed %.1f" % (loads_now / n_tiles, loads_need / n_tiles))
    print("k_schur  lm_hP read per window: today %.0f KB, needed %.0f KB" % (hp_now / W / 1e3, hp_need / W / 1e3))
    print("k_schur  matrix-core instructions per window: today %.0f, needed %.0f (%+.1f %%)" % (mfma_now / W, mfma_need / W, 100.0 * (mfma_need / mfma_now - 1)))
    print("k_schur  on the longest wave's path per window: today %.0f, needed %.0f" % (path_now / W, path_need / W))
    print("k_schur  pairs issued per window %.0f, of them diagonal %.0f" % (pairs / W, diag / W))
    print("k_vis_chunk  matrix-core instructions per window: today %.0f, in groups of four k-steps %.0f (%+.1f %%), by single k-steps %.0f (%+.1f %%)"
          % (vis_now / W, vis_need / W, 100.0 * (vis_need / vis_now - 1), vis_single / W, 100.0 * (vis_single / vis_now - 1)))
    print("k_vis_chunk  lane use over the steps a tile runs: %.2f" % (lanes / lane_steps))


if __name__ == "__main__":
    main()
