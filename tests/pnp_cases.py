"""TEST INFRASTRUCTURE. The cases of the loop verification (include/gfbe_pnp.h) for tests/test_pnp_model.py and tests/test_gpu_pnp.py: planted
poses with a stated share of inliers, built so that no discrete result hangs on a rounding, and the check of that condition.

The case condition (checked on the CPU by test_pnp_model.py for every case the GPU test uses): no (hypothesis, solution, point) has its
squared error within 1e-9 thr^2 of thr^2; the FP64 and the longdouble model agree on the winner, the mask and the decision, with
|relative_yaw| at least 1e-9 from the yaw limit and |relative_t| at least 1e-9 from the translation limit. The planted cases make that
hold by construction: inlier noise is at most thr / 4, outliers are off by at least 4 thr under the planted pose, the inlier share is 0.6."""
import functools

import numpy as np

import pnp_np as m

THR = 10.0 / 460.0
QIC = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # a camera looking along the body's x
TIC = np.array([0.05, -0.02, 0.1])


def rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rot_vec(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = np.asarray(v) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def frame(rng, dyaw=3.0, dt=(0.3, -0.2, 0.1), body_yaw=40.0):
    """The old keyframe's body at a seeded pose with its camera, and the current pose: that body turned by dyaw degrees about z and moved
    by dt in the old body frame. dict(R_wi, T_wi, R_wc, t_wc, pose_cur [12], tic_qic [12])"""
    R_wi = rot_z(body_yaw) @ rot_vec(rng.uniform(-0.05, 0.05, 3))
    T_wi = rng.uniform(-3, 3, 3)
    return dict(R_wi=R_wi, T_wi=T_wi, R_wc=R_wi @ QIC, t_wc=T_wi + R_wi @ TIC, pose_cur=np.concatenate([T_wi + R_wi @ np.asarray(dt, float), (rot_z(dyaw) @ R_wi).ravel()]),
                tic_qic=np.concatenate([TIC, QIC.ravel()]))


def planted(seed, n_inliers, n_outliers, noise=THR / 4, dyaw=3.0, dt=(0.3, -0.2, 0.1), body_yaw=40.0):
    """dict(point_3d [n, 3] float32, pt_norm [n, 2] float32, pose_cur [12], tic_qic [12], inlier [n] bool, R, t (the planted Xc = R Xw + t),
    pnp_pose [12] the planted PnP_T_old, PnP_R_old) around frame()."""
    rng = np.random.default_rng(seed)
    n = n_inliers + n_outliers
    f = frame(rng, dyaw, dt, body_yaw)
    R_wi, T_wi, R_wc, t_wc = f["R_wi"], f["T_wi"], f["R_wc"], f["t_wc"]
    uv = rng.uniform(-0.5, 0.5, (n, 2))
    depth = rng.uniform(2.0, 8.0, n)
    Xc = np.concatenate([uv * depth[:, None], depth[:, None]], 1)
    p3 = (Xc @ R_wc.T + t_wc).astype(np.float32)
    R, t = R_wc.T, -R_wc.T @ t_wc
    Xc = p3.astype(np.float64) @ R.T + t      # (the observations are those of the rounded points)
    obs = Xc[:, :2] / Xc[:, 2:]
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[:n_inliers]] = True
    ang, rad = rng.uniform(0, 2 * np.pi, n), np.where(inl, noise * np.sqrt(rng.uniform(0, 1, n)) * 0.99, rng.uniform(4.0 * THR * 1.01, 0.4, n))
    obs = obs + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    return dict(point_3d=p3, pt_norm=obs.astype(np.float32), pose_cur=f["pose_cur"], tic_qic=f["tic_qic"], inlier=inl, R=R, t=t,
                pnp_pose=np.concatenate([T_wi, R_wi.ravel()]))


def collinear(case, o):
    """The sample of hypothesis 0 forced onto one line (its observations follow the planted pose): zero solutions there."""
    c = dict(case)
    idx, got = m.sample(o["seed"], 0, len(c["point_3d"]))
    assert got == 3
    p3 = c["point_3d"].copy()
    p3[idx[2]] = p3[idx[0]] + np.float32(0.5) * (p3[idx[1]] - p3[idx[0]])
    c["point_3d"] = p3
    return c


# name -> (options of the handle beyond the defaults, the problems of one call)
def build():
    cases = {}
    cases["n25"] = (dict(), [planted(1, 25, 0)])                                   # V1: no PnP
    cases["in26"] = (dict(), [planted(2, 26, 17)])                                 # the least count that is a loop
    cases["in63"] = (dict(), [planted(3, 63, 42)])                                 # V6's lane stride: one short of a wave,
    cases["in64"] = (dict(), [planted(4, 64, 43)])                                 # a whole wave,
    cases["in65"] = (dict(), [planted(5, 65, 43)])                                 # one over
    cases["full"] = (dict(max_points=200), [planted(6, 120, 80)])                  # n = max_points
    cases["tile513"] = (dict(), [planted(18, 308, 205)])                           # one point past k_pnp_score's tile of 512
    cases["tile1025"] = (dict(), [planted(19, 615, 410)])                          # one point past two tiles
    cases["max4096"] = (dict(), [planted(20, 2458, 1638)])                         # n = the default max_points: eight tiles, the whole inlier list
    cases["batch3"] = (dict(), [planted(7, 40, 27), planted(8, 0, 0), planted(9, 90, 60), planted(10, 30, 20)])      # B = 3 and an empty problem
    cases["iter1"] = (dict(iterations=1), [planted(11, 50, 0, noise=0.0)])
    cases["refine0"] = (dict(refine_iterations=0), [planted(12, 45, 30)])
    cases["outliers"] = (dict(), [planted(13, 0, 60)])                             # no loop
    cases["ties"] = (dict(), [planted(14, 48, 32, noise=0.0)])                     # every clean hypothesis has the same count
    cases["collinear"] = (dict(), [collinear(planted(15, 48, 32), m.options())])
    cases["yaw"] = (dict(), [planted(16, 48, 32, dyaw=41.0)])                      # solved, rejected
    cases["far"] = (dict(), [planted(17, 48, 32, dt=(25.0, 3.0, 1.0))])
    cases["turned"] = (dict(max_yaw_deg=50.0, max_translation=30.0), [planted(16, 48, 32, dyaw=41.0), planted(17, 48, 32, dt=(25.0, 3.0, 1.0))])      # the limits are options
    return cases


CASES = build()
YAW_ATOL = 1e-12      # degrees: two atan2 at 2 ulp, the degree conversion and one subtraction stay under 8 ulp of 180 = 2.3e-13; the decade above


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's results of a case's problems, computed once and shared (callers leave them unchanged)."""
    kw, problems = CASES[name]
    return [m.verify_problem(m.options(**kw), p["point_3d"], p["pt_norm"], p["pose_cur"], p["tic_qic"]) for p in problems]


def assert_equals_model(got, offset, wants, diagnostics=True):
    """Every output of a verify against the model's results `wants`: bits, but for relative_yaw (YAW_ATOL)"""
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    for b, want in enumerate(wants):
        assert np.array_equal(got["status"][offset[b]:offset[b + 1]], want["status"]), b
        assert (got["n_inliers"][b], got["has_loop"][b], got["refine_flag"][b]) == (want["n_inliers"], want["has_loop"], want["refine_flag"]), b
        assert np.array_equal(got["best"][b], want["best"]), b
        assert np.array_equal(bits(got["loop_info"][b, :7]), bits(want["loop_info"][:7])), b
        assert abs(got["loop_info"][b, 7] - want["loop_info"][7]) <= YAW_ATOL, b
        assert np.array_equal(bits(got["pnp_pose"][b]), bits(want["pnp_pose"])), b
        if diagnostics:
            assert np.array_equal(got["sample_idx"][b], want["sample_idx"]) and np.array_equal(got["n_solutions"][b], want["n_solutions"]), b
            assert np.array_equal(got["hyp_count"][b], want["hyp_count"]) and np.array_equal(bits(got["hyp_pose"][b]), bits(want["hyp_pose"])), b


def pack(problems):
    """The arguments of one gfbe_pnp_verify: offset, point_3d, pt_norm, pose_cur, tic_qic"""
    off = np.zeros(len(problems) + 1, np.int32)
    off[1:] = np.cumsum([len(p["point_3d"]) for p in problems])
    return (off, np.concatenate([p["point_3d"].reshape(-1, 3) for p in problems]).astype(np.float32), np.concatenate([p["pt_norm"].reshape(-1, 2) for p in problems]).astype(np.float32),
            np.stack([p["pose_cur"] for p in problems]), np.stack([p["tic_qic"] for p in problems]))


def condition(o, problem):
    """The case condition of one problem: (holds, the FP64 result, what failed)"""
    a = m.verify_problem(o, problem["point_3d"], problem["pt_norm"], problem["pose_cur"], problem["tic_qic"], np.float64)
    b = m.verify_problem(o, problem["point_3d"], problem["pt_norm"], problem["pose_cur"], problem["tic_qic"], np.longdouble)
    why = []
    if not min(a["margin"], b["margin"]) >= 1e-9:
        why.append("an error within 1e-9 thr^2 of thr^2")
    if not (np.array_equal(a["best"], b["best"]) and np.array_equal(a["status"], b["status"]) and a["n_inliers"] == b["n_inliers"] and a["refine_flag"] == b["refine_flag"]):
        why.append("the winner or the mask differ")
    if not (np.array_equal(a["n_solutions"], b["n_solutions"]) and np.array_equal(a["hyp_count"], b["hyp_count"])):
        why.append("a hypothesis differs")
    if a["has_loop"] != b["has_loop"]:
        why.append("the decision differs")
    for r in (a, b):
        if r["yaw"] is not None and not (abs(abs(float(r["yaw"])) - o["max_yaw_deg"]) >= 1e-9 and abs(float(r["tnorm"]) - o["max_translation"]) >= 1e-9):
            why.append("a limit of V8 within 1e-9")
    return not why, a, why
