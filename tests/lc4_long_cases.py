"""The cases of gfbe_lc4_solve_long shared by tests/test_lc4_long_host.py (CPU: margins, r_cpu, the golden's digest) and
tests/test_gpu_lc4_long.py (the device against the longdouble model): figure-of-eight graphs of synth.loop_graph with more than 64 loop
edges, each the smallest shape at which one part of the blocked capacitance path can go wrong. The model is tests/lc4_np.py unchanged
(its band path and plan() do not depend on MAX_LOOPS); criterion, bounds K and the seed rule are those of tests/lc4_cases.py: no
decision nearer to its threshold than 1e3 u A, FP64 and longdouble decide alike, a seed that fails that is replaced, never skipped.

The 512-loop case is too slow for the model to solve live (minutes on one core): its reference is recorded once by
tests/golden/make_golden_lc4_long.py into tests/golden/lc4_long_cap.npz, together with a digest of the input arrays."""
import functools
import hashlib
import os

import numpy as np

import lc4_cases as lc
import lc4_np as m

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lc4_long_cap.npz")
CAP = "n700_512_loops"


def cases():
    """The live cases: their references are solved by the model in the test process."""
    out = {}
    out["n132_65_loops"] = lc.graph(n=132, n_loop=65, seed=21, laps=2)                               # 17 tile columns of capacitance: the first size past the one-workgroup kernel
    out["n200_80_loops"] = lc.graph(n=200, n_loop=80, seed=22, laps=2)                               # 20 tiles, five iterations
    out["n260_129_loops"] = lc.graph(n=260, n_loop=129, seed=23, laps=2, opt=dict(max_num_iterations=2))      # cap 516 padded to 528: a ragged last tile, 33 tiles
    two = lc.graph(n=300, n_loop=70, seed=26, laps=2, n_fixed_sequence=100)                          # loops from sequence 1 into the constant sequence 0: half of each U column group is zero
    two["g"]["fixed"][two["g"]["loop_i"][0]] = 1                                                     # ... and one loop edge with both ends constant: dropped, its block of S is the identity
    out["n300_two_sequences_70_loops"] = two
    out["n140_yaw_wrap_66_loops"] = lc.graph(n=140, n_loop=66, seed=27, laps=2, yaw0=140.0)          # headings on both sides of +-180: the wrap in x (+) S y
    return out


def cap_case():
    """512 loop edges: 128 tiles of capacitance, a panel of 2800 x 2064, M = 175. Two iterations."""
    return lc.graph(n=700, n_loop=512, seed=25, laps=4, opt=dict(max_num_iterations=2))


def all_cases():
    out = cases()
    out[CAP] = cap_case()
    return out


def unusable_case():
    """A 65-loop graph with one non-finite translation of a free pose: five invalid steps, Ceres' numerical failure."""
    c = lc.graph(n=132, n_loop=65, seed=21, laps=2)
    c["g"]["t"][7, 1] = np.nan
    return c


def input_digest(c):
    """SHA-256 over the arrays a solve takes (as the C ABI sees them) and the options."""
    h = hashlib.sha256()
    for k, dt in zip(lc.ARG_KEYS, (np.float64, np.float64, np.int32, np.uint8, np.int32, np.int32, np.float64)):
        a = np.ascontiguousarray(c["g"][k], dt)
        h.update(k.encode() + str(a.shape).encode() + a.tobytes())
    h.update(repr(sorted(c["opt"].items())).encode())
    return h.hexdigest()


def split(x):
    """A longdouble array as a float64 high / low pair."""
    x = np.asarray(x, m.LD)
    hi = x.astype(np.float64)
    return hi, (x - hi.astype(m.LD)).astype(np.float64)


def join(hi, lo):
    return np.asarray(hi, m.LD) + np.asarray(lo, m.LD)


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    ref = dict(t=join(z["t_hi"], z["t_lo"]), yaw=join(z["yaw_hi"], z["yaw_lo"]), drift=join(z["drift_hi"], z["drift_lo"]),
               cost_history=list(join(z["cost_hi"], z["cost_lo"])), A_cost=[float(v) for v in z["A_cost"]], g_l1=[float(v) for v in z["g_l1"]],
               A_pose=float(z["A_pose"]), accepted=[int(v) for v in z["accepted_ld"]])
    ref["final_cost"] = ref["cost_history"][-1]
    ref["iterations"], ref["termination"], ref["status"], ref["num_successful"] = (int(v) for v in z["decisions_ld"])
    f64 = dict(accepted=[int(v) for v in z["accepted_f64"]])
    f64["iterations"], f64["termination"], f64["status"], f64["num_successful"] = (int(v) for v in z["decisions_f64"])
    return dict(ref=ref, f64=f64, margin=float(z["margin"]), r_cpu=dict(pose=float(z["r_cpu_pose"]), cost=float(z["r_cpu_cost"])), digest=str(z["digest"]))


@functools.lru_cache(maxsize=None)
def reference(name, dtype="ld"):
    """The model's solve of a case (band path): computed once per process and left unchanged; the 512-loop case from the golden."""
    if name == CAP:
        return golden()["ref" if dtype == "ld" else "f64"]
    c = cases()[name]
    return m.solve(*c["args"], opt=c["opt"], dt=m.LD if dtype == "ld" else np.float64, path="band")
