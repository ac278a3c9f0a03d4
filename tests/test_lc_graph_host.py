"""The graph construction of the loop-closure solves (lc_build_graph, ground-fusion2_amd/csrc/gfbe_loopgraph.h) without a GPU, for both
models, through tests/lc4_host_shim.cpp and tests/lc6_host_shim.cpp: which sequence edges exist, who is in the problem, which loop
edges are kept, and the per-pose CSR of loop shares, against the rules written out here in plain Python (not against lc4_np / lc6_np)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDRS = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_loopgraph6.h", "gfbe_loopgraph.h")]
PD, PI, PU8 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)

# nine poses, two sequences, sequence 0 constant; loop edges (loop_i, loop_c): into a constant pose, between two constant poses
# (dropped), both ends free — pose 5 takes shares of edges 0 (as loop_i) and 2 (as loop_c)
N = 9
SEQUENCE = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1], np.int32)
FIXED = np.array([1, 1, 1, 1, 0, 0, 0, 0, 0], np.uint8)
LOOP_I = np.array([5, 3, 8], np.int32)
LOOP_C = np.array([1, 0, 5], np.int32)


def _graph_by_the_rules(span):
    emask, free = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    for i in range(N):
        for k in range(1, span + 1):
            if i - k >= 0 and SEQUENCE[i] == SEQUENCE[i - k] and not (FIXED[i] and FIXED[i - k]):
                emask[i] |= 1 << (k - 1)
                free[i] = free[i - k] = 1
    loop_on = np.array([not (FIXED[c] and FIXED[i]) for i, c in zip(LOOP_I, LOOP_C)], np.uint8)
    rows = [[] for _ in range(N)]
    for l, (i, c) in enumerate(zip(LOOP_I, LOOP_C)):
        if loop_on[l]:
            free[i] = free[c] = 1
            rows[c].append(2 * l)
            rows[i].append(2 * l + 1)
    return emask, free & (1 - FIXED), loop_on, rows


def _shim(dof):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_loopgraph.h cannot be built for the host")
    src, out = os.path.join(ROOT, "tests", "lc%d_host_shim.cpp" % dof), os.path.join(BUILD, "lc%d_host_shim.so" % dof)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + HDRS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src], check=True)
    return C.CDLL(out)


@pytest.mark.parametrize("span", [1, 4])
@pytest.mark.parametrize("dof", [4, 6])
def test_graph_construction_follows_the_rules(dof, span):
    rot_len, meas_len = {4: (3, 6), 6: (4, 7)}[dof]
    rng = np.random.default_rng(7)
    t, rot = rng.standard_normal((N, 3)), rng.standard_normal((N, rot_len))
    L = len(LOOP_I)
    emask, free, loop_on = np.full(N, 255, np.uint8), np.full(N, 255, np.uint8), np.full(L, 255, np.uint8)
    lp_begin, lp_entry, meas = np.full(N + 1, -1, np.int32), np.full(2 * L, -1, np.int32), np.zeros((N, 4, meas_len))
    used = getattr(_shim(dof), "shim_lc%d_graph" % dof)(
        C.c_int(N), C.c_int(span), t.ctypes.data_as(PD), rot.ctypes.data_as(PD), SEQUENCE.ctypes.data_as(PI), FIXED.ctypes.data_as(PU8), C.c_int(L),
        LOOP_I.ctypes.data_as(PI), LOOP_C.ctypes.data_as(PI), emask.ctypes.data_as(PU8), free.ctypes.data_as(PU8), loop_on.ctypes.data_as(PU8),
        lp_begin.ctypes.data_as(PI), lp_entry.ctypes.data_as(PI), meas.ctypes.data_as(PD))
    want_emask, want_free, want_on, rows = _graph_by_the_rules(span)
    assert np.array_equal(emask, want_emask) and np.array_equal(free, want_free) and np.array_equal(loop_on, want_on)
    assert list(want_on) == [1, 0, 1] and want_free[1] == 0 and want_free[5] == 1 and want_free[4] == 1
    # the CSR: each pose's row holds 2 l + side in ascending l
    assert lp_begin[0] == 0 and used == lp_begin[N] == sum(len(r) for r in rows) == 4
    for i in range(N):
        assert list(lp_entry[lp_begin[i]:lp_begin[i + 1]]) == rows[i], i
    assert rows[5] == [1, 4] and rows[1] == [0] and rows[8] == [5] and not rows[0] and not rows[3]
    # a measurement is formed exactly where an edge exists
    exists = (want_emask[:, None] >> np.arange(4)[None, :]) & 1
    assert np.array_equal(meas.any(axis=2), exists.astype(bool))
