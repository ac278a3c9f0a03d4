"""The cases shared by tests/test_lc6_model.py (CPU: decision margins, r_cpu) and tests/test_gpu_lc6.py (the device against the
longdouble model): figure-of-eight graphs of synth.loop_graph6 at the smallest sizes at which each kernel of gfbe_loopgraph6.hip can go
wrong — n = 1, 3, 4, 5, 9 (three super-blocks, not a power of two), 65 (17 super-blocks), 257; 0, 1, 2 (inside one 16-column tile of the
capacitance system), 3 (crosses a tile) and 128 loop edges (the cap: the panel fill and the gather run their grid-stride loops; the
implementation has no other hand-over in the loop count); loops within one super-block, between neighbouring ones, far apart and onto a
constant pose; span 1 .. 4; two sequences; the Huber loss inactive and active; a first step that is rejected; poses at the identity
whose step is exactly zero; a measurement whose error quaternion has w < 0.
Seeds are chosen so that no discrete decision is nearer to its threshold than MARGIN times the bound of the quantity compared (asserted
on the CPU by test_lc6_model.py); a case whose margins are too small is replaced, never skipped."""
import functools

import numpy as np

from _gfbe_import import gf
import lc6_np as m

synth = gf.synth
ARG_KEYS = ("t", "q", "sequence", "fixed", "loop_i", "loop_c", "loop_meas")
MARGIN = 1e3


def graph(opt=None, **kw):
    g = synth.loop_graph6(**kw)
    return dict(g=g, opt=m.options(**(opt or {})))


def args(c):
    return tuple(c["g"][k] for k in ARG_KEYS)


def _with_identity_tail(c, k=3):
    """k more keyframes of a sequence of their own, every one the identity pose at the origin: their sequence edges have residuals that
    are exactly zero in any precision, so their gradient and their step are exactly zero (|d| = 0 in Plus) while they are free."""
    g = c["g"]
    n = len(g["t"])
    g["t"] = np.concatenate([g["t"], np.zeros((k, 3))])
    g["q"] = np.concatenate([g["q"], np.tile([1.0, 0, 0, 0], (k, 1))])
    g["sequence"] = np.concatenate([g["sequence"], np.full(k, 2, np.int32)])
    g["fixed"] = np.concatenate([g["fixed"], np.zeros(k, np.uint8)])
    g["true_t"] = np.concatenate([g["true_t"], np.zeros((k, 3))])
    g["identity_tail"] = (n, n + k)
    return c


def cases():
    out = {}
    out["n1"] = graph(n=1, n_loop=0, seed=1, laps=1)                                                   # the constant first pose alone: nothing to solve
    out["n3_loop_into_constant"] = graph(n=3, seed=2, laps=1, loops=[(0, 2)])                          # one super-block, no sweep; the loop's other end is pose 0
    out["n4_two_loops"] = graph(n=4, seed=3, laps=1, loops=[(0, 2), (1, 3)])                           # a full super-block; 12 capacitance rows: one tile
    out["n5_three_loops"] = graph(n=5, seed=4, laps=1, loops=[(0, 2), (1, 3), (1, 4)])                 # two super-blocks, one sweep; 18 rows: two tiles; a loop between neighbours
    out["n5_no_loop"] = graph(n=5, n_loop=0, seed=5, laps=1)                                           # panel of one column, no capacitance system
    for span in (1, 2, 3):                                                                             # three super-blocks (not a power of two); a loop far apart
        out["n9_span%d" % span] = graph(n=9, seed=5 + span, laps=1, loops=[(0, 8), (2, 5)], opt=dict(span=span))
    out["n9_huber_inactive"] = graph(n=9, seed=9, laps=1, loops=[(1, 7), (2, 5)], yaw_bias=1e-5, scale_err=1e-6, meas_noise=1e-5)
    out["n65_shapes"] = graph(n=65, n_loop=8, seed=10, loop_into_first=True, loop_same_block=True)     # M = 17; loop into the constant pose, loop within a super-block
    out["n65_outlier"] = graph(n=65, n_loop=6, seed=11)                                                # a planted outlier loop: the Huber corrector at work
    out["n65_outlier"]["g"]["loop_meas"][2, :3] += [3.0, -2.0, 0.5]
    out["n65_identity_tail"] = _with_identity_tail(graph(n=62, n_loop=4, seed=12))                     # free poses whose step is exactly zero
    neg = graph(n=65, n_loop=6, seed=13, laps=1)                                                       # laps = 1: loops join keyframes of any two headings
    e = m.qmul(m.qconj(neg["g"]["loop_meas"][:, 3:]), m.qmul(m.qconj(neg["g"]["q"][neg["g"]["loop_c"]]), neg["g"]["q"][neg["g"]["loop_i"]]))
    neg["g"]["loop_meas"][e[:, 0] > 0, 3:] *= -1.0                                                     # the same rotations, every error_q.w < 0
    out["n65_negated_q"] = neg
    out["n257_two_sequences"] = graph(n=257, n_loop=16, seed=14, n_fixed_sequence=100)                 # M = 65; sequence 0 constant, loops from sequence 1 into it
    out["n257_128_loops"] = graph(n=257, n_loop=128, seed=15, opt=dict(max_num_iterations=2))          # the cap: 768 capacitance rows, 49 tile columns of panel
    out["all_fixed"] = graph(n=20, n_loop=3, seed=16)
    out["all_fixed"]["g"]["fixed"][:] = 1
    out["max_it_0"] = graph(n=9, seed=17, laps=1, loops=[(0, 8), (2, 5)], opt=dict(max_num_iterations=0))
    out["max_it_1"] = graph(n=9, seed=17, laps=1, loops=[(0, 8), (2, 5)], opt=dict(max_num_iterations=1))
    # a start far off: the sequence edges are formed from the start itself, so "far" means loop measurements that contradict it —
    # rotations off by 175 degrees, translations by hundreds of metres, the loss opened so that they pull at full weight
    far = graph(n=65, n_loop=8, seed=18, throw=1.0, opt=dict(max_num_iterations=12, huber_delta=1e4))
    rng = np.random.default_rng(18)
    for l in range(8):
        a = np.deg2rad(175.0) / 2 * rng.choice([-1, 1])
        turn = np.array([np.cos(a), 0.0, 0.0, np.sin(a)])
        far["g"]["loop_meas"][l, 3:] = m.qmul(far["g"]["loop_meas"][l, 3:], turn)
    far["g"]["loop_meas"][:, :3] += rng.normal(0, 200, (8, 3))
    out["far_start"] = far
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype="ld"):
    """The model's solve of a case (band path), computed once per process and left unchanged."""
    c = cases()[name]
    return m.solve(*args(c), opt=c["opt"], dt=m.LD if dtype == "ld" else np.float64, path="band")


def decisions(res):
    return (res["iterations"], tuple(res["accepted"]), res["termination"], res["status"], res["num_successful"])


def margin_ratio(res):
    """The smallest decision margin of a solve in units of u x the absolute sum behind the quantity compared."""
    return min((mg / (m.U * max(A, 1e-300)) for _, mg, A in res["margins"] if np.isfinite(mg)), default=np.inf)


def solve_ratios(dev, ref):
    """Worst |X_dev - X_ref| / (u A_X) per output array of a solve, against the longdouble model `ref`; dev: dict(t, q, cost_history)."""
    A_pose = max(ref["A_pose"], 1e-300)
    pose = max(float(np.abs(np.asarray(dev["t"], m.LD) - ref["t"]).max()), float(np.abs(np.asarray(dev["q"], m.LD) - ref["q"]).max())) / (m.U * A_pose)
    cost = 0.0
    for k, c in enumerate(ref["cost_history"]):
        A = ref["A_cost"][k] + (ref["g_l1"][k] * A_pose if k else 0.0)
        cost = max(cost, float(abs(m.LD(dev["cost_history"][k]) - c)) / (m.U * max(A, 1e-300)))
    return dict(pose=pose, cost=cost)


def eval_case(name):
    """The edge list gfbe_lc6_eval takes for a case: the model's graph at the input poses, moved off the start by a seeded perturbation
    so that residuals and the corrector are exercised."""
    c = cases()[name]
    G = m.build_graph(*args(c), c["opt"])
    rng = np.random.default_rng(len(name))
    t = np.asarray(c["g"]["t"]) + rng.normal(0, 0.05, c["g"]["t"].shape)
    q, _ = m.plus(np.asarray(c["g"]["q"], np.float64), t, np.concatenate([rng.normal(0, 0.01, (len(t), 3)), np.zeros((len(t), 3))], axis=1), np.float64)
    q /= np.linalg.norm(q, axis=1)[:, None]
    return dict(t=t, q=q, edge_i=G["edge_i"], edge_j=G["edge_j"], kind=G["kind"], meas=G["meas"], opt=c["opt"])


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
# test_lc6_model.py::test_bounds_cover_four_times_the_cpu_ratio, which fails when a K here is not that power of two). Units u A_X.
K = dict(r=16, J=32, eval_cost=4, pose=8, cost=4)      # r_cpu: r 2.30, J 5.08, eval_cost 0.60, pose 1.46, cost 0.57; the device's worst ratios: tests/test_gpu_lc6.py
