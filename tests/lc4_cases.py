"""The cases shared by tests/test_lc4_model.py (CPU: decision margins, r_cpu, convergence) and tests/test_gpu_lc4.py (the device against
the longdouble model): figure-of-eight graphs of synth.loop_graph at the sizes at which the kernels can go wrong — super-block counts
on both sides of a power of two, a ragged last super-block, 0 / 1 / 64 loop edges — and the graph shapes the reference produces.
Seeds are chosen so that no discrete decision is nearer to its threshold than 1e3 times the bound of the quantity compared (asserted on
the CPU by test_lc4_model.py); a seed whose margins are too small is replaced, never skipped."""
import functools

import numpy as np

from _gfbe_import import gf
import lc4_np as m

synth = gf.synth
ARG_KEYS = ("t", "ypr", "sequence", "fixed", "loop_i", "loop_c", "loop_meas")


def graph(opt=None, converging=False, **kw):
    g = synth.loop_graph(**kw)
    return dict(g=g, args=tuple(g[k] for k in ARG_KEYS), opt=m.options(**(opt or {})), converging=converging)


def cases():
    out = {}
    out["n2_loop_into_constant"] = graph(n=2, n_loop=1, seed=1, laps=1)                              # one super-block, no sweep; the loop's other end is pose 0
    out["n5_no_loop"] = graph(n=5, n_loop=0, seed=2, laps=1)                                         # two super-blocks, three padding poses, panel of one column
    out["n63_one_loop"] = graph(n=63, n_loop=1, seed=3)                                              # M = 16 (a power of two), one padding pose
    out["n64_shapes"] = graph(n=64, n_loop=8, seed=4, loop_into_first=True, loop_same_block=True)    # M = 16 exactly; loop into the constant pose, loop within a super-block
    out["n65_64_loops"] = graph(n=65, n_loop=64, seed=5)                                             # M = 17; the full capacitance system, 17 tile columns of panel
    out["n257_two_sequences"] = graph(n=257, n_loop=16, seed=6, n_fixed_sequence=100)                # M = 65; sequence 0 constant, loops from sequence 1 into it
    out["n257_64_loops"] = graph(n=257, n_loop=64, seed=7)
    out["n1001_convergence"] = graph(n=1001, n_loop=8, seed=8, yaw_bias=0.05, scale_err=0.02, converging=True)
    out["all_fixed"] = graph(n=20, n_loop=3, seed=9)
    out["all_fixed"]["g"]["fixed"][:] = 1
    out["yaw_wrap"] = graph(n=63, n_loop=4, seed=10, yaw0=140.0)                                     # headings on both sides of +-180
    out["max_it_0"] = graph(n=64, n_loop=8, seed=11, opt=dict(max_num_iterations=0))
    out["max_it_1"] = graph(n=64, n_loop=8, seed=11, opt=dict(max_num_iterations=1))
    # a start far off: the sequence edges are formed from the start itself, so "far" means loop measurements that contradict it — yaw off
    # by 175 degrees, translations by hundreds of metres, the loss opened so that they pull at full weight: four steps in a row are rejected
    far = graph(n=65, n_loop=8, seed=12, throw=1.0, opt=dict(max_num_iterations=12, huber_delta=1e4))
    rng = np.random.default_rng(12)
    far["g"]["loop_meas"][:, 3] = (far["g"]["loop_meas"][:, 3] + 175 * rng.choice([-1, 1], 8) + 180) % 360 - 180
    far["g"]["loop_meas"][:, :3] += rng.normal(0, 200, (8, 3))
    out["far_start"] = far
    return out


def unusable_case():
    """A non-finite translation of a free pose: H and g are NaN, every pivot test fails, five invalid steps in a row end the solve as
    Ceres' numerical failure. Not one of cases(): its margins are NaN by construction."""
    c = graph(n=20, n_loop=2, seed=13, laps=1)
    c["g"]["t"][7, 1] = np.nan
    return c


@functools.lru_cache(maxsize=None)
def reference(name, dtype="ld"):
    """The model's solve of a case (band path), computed once per process and left unchanged."""
    c = cases()[name]
    return m.solve(*c["args"], opt=c["opt"], dt=m.LD if dtype == "ld" else np.float64, path="band")


def decisions(res):
    return (res["iterations"], tuple(res["accepted"]), res["termination"], res["status"], res["num_successful"])


def margin_ratio(res):
    """The smallest decision margin of a solve in units of u x the absolute sum behind the quantity compared."""
    return min((mg / (m.U * max(A, 1e-300)) for _, mg, A in res["margins"] if np.isfinite(mg)), default=np.inf)


def solve_ratios(dev, ref):
    """Worst |X_dev - X_ref| / (u A_X) per output array of a solve, against the longdouble model `ref`; dev: dict(t, yaw, cost_history)."""
    A_pose = max(ref["A_pose"], 1e-300)
    pose = max(float(np.abs(np.asarray(dev["t"], m.LD) - ref["t"]).max()), float(np.abs(np.asarray(dev["yaw"], m.LD) - ref["yaw"]).max())) / (m.U * A_pose)
    cost = 0.0
    for k, c in enumerate(ref["cost_history"]):
        A = ref["A_cost"][k] + (ref["g_l1"][k] * A_pose if k else 0.0)
        cost = max(cost, float(abs(m.LD(dev["cost_history"][k]) - c)) / (m.U * max(A, 1e-300)))
    return dict(pose=pose, cost=cost)


def eval_case(name):
    """The edge list gfbe_lc4_eval takes for a case: the model's graph at the input poses, moved off the start by a seeded perturbation
    so that residuals and the corrector are exercised."""
    c = cases()[name]
    G = m.build_graph(*c["args"], c["opt"])
    rng = np.random.default_rng(len(name))
    t = np.asarray(c["g"]["t"]) + rng.normal(0, 0.05, c["g"]["t"].shape)
    ypr = np.asarray(c["g"]["ypr"]).copy()
    ypr[:, 0] = (ypr[:, 0] + rng.normal(0, 1.0, len(ypr)) + 180.0) % 360.0 - 180.0
    return dict(t=t, ypr=ypr, edge_i=G["edge_i"], edge_j=G["edge_j"], kind=G["kind"], meas=G["meas"], opt=c["opt"])


def eval_ratios(dev, ref):
    out = {}
    for k, A in (("r", "A_r"), ("J", "A_J")):
        if ref[k].size:
            out[k] = float((np.abs(np.asarray(dev[k], m.LD) - ref[k]).astype(np.float64) / (m.U * np.maximum(ref[A], 1e-300))).max())
        else:
            out[k] = 0.0
    out["cost"] = float(abs(m.LD(dev["cost"]) - ref["cost"])) / (m.U * max(ref["A_cost"], 1e-300))
    return out


# K_X: the smallest power of two >= 4 r_cpu, r_cpu = the FP64 model against the longdouble model over every case (measured by
# test_lc4_model.py::test_bounds_cover_four_times_the_cpu_ratio, which fails when a K here is not that power of two). Units u A_X.
K = dict(r=8, J=8, eval_cost=1, pose=2, cost=1)      # r_cpu: r 1.43, J 1.42, eval_cost 0.17, pose 0.28, cost 0.13; device worst: see tests/test_gpu_lc4.py
