"""The cases shared by tests/test_vreg_model.py (CPU: margins, convergence, r_cpu) and tests/test_gpu_vreg.py (device against the model):
a room map (synth_scan.Room, about 1500 points), a scan of at most 257 keypoints taken at a true pose, and a start pose thrown off it.
Seeds are chosen so that no discrete decision of the loop is nearer to its threshold than 1e3 times the bound of the quantity compared
(asserted on the CPU by test_vreg_model.py); a seed whose margins are too small is replaced, never skipped."""
import numpy as np

from _gfbe_import import gf
import vmap_np as vm
import vreg_np as vr

synth_scan = gf.synth_scan
WG = 256      # workgroup width of k_vr_lin: rows_255 / rows_256 / rows_257 cut the rows around it


def _perturb(pose, rng, trans, deg):
    d = rng.normal(size=3)
    ax = rng.normal(size=3)
    th = np.deg2rad(deg)
    dq = np.concatenate([np.sin(th / 2) * ax / np.linalg.norm(ax), [np.cos(th / 2)]])
    q = vr.qmul(np.asarray(pose[3:], float), dq)
    return np.concatenate([pose[:3] + trans * d / np.linalg.norm(d), q / np.linalg.norm(q)])


def room(seed, n_kp, ct, trans=0.03, deg=0.5, clutter=0.0, n_map=1500, vopt=None, noise=0.001, **o):
    rm = synth_scan.Room(seed=seed, noise=noise)      # (1 mm of plane noise: the floor of the registration stays well under a quarter of the 3 cm start)
    poses = rm.trajectory(3)
    tb, te = poses[0], (poses[1] if ct else poses[0])
    surface = rm.surface(n_map, 0.05)
    sc = rm.scan(tb, te, n_kp, clutter)
    rng = np.random.default_rng(1000 + seed)
    pb = _perturb(tb, rng, trans, deg)
    pe = _perturb(te, rng, trans, deg) if ct else pb.copy()
    o.setdefault("min_num_residuals", 50)
    return dict(vopt=vopt or {}, cap=4096, map=surface, ct=ct, raw=sc["raw"], alpha=sc["alpha"] if ct else None, pb=pb, pe=pe, true_b=tb, true_e=te,
                prev_t=tb[:3].copy() if ct else None, prev_q=tb[3:].copy() if ct else None, o=vr.options(**o), converging=True)


def cases():
    out = {}
    out["ct1_default"] = room(41, 257, 1, min_num_residuals=300)
    out["ct0_default"] = room(42, 120, 0, min_num_residuals=300)
    out["cap"] = room(43, 120, 1, max_num_iteration=2)
    out["cap"]["converging"] = False            # (leaves by the cap)
    out["lm0"] = room(44, 120, 1, lm_max_num_iterations=0, max_num_iteration=2)
    out["lm0"]["converging"] = False
    out["far_start"] = room(45, 120, 1, trans=0.55, deg=45.0)
    out["far_start"]["converging"] = False      # (far enough off that inner steps are rejected; it does not find the pose)
    # clutter: 5 % of the scan lies on no surface, which leaves the model a floor of 5.5 mm whatever the start and the exit thresholds
    # (the same from a 3 cm and a 6 cm start, and with thresholds a hundred times tighter); the start is thrown off by 6 cm and 1 deg
    # so that a quarter of the start error lies above that floor, as it does for the other cases (floors of 3 - 4.5 mm, 3 cm starts)
    out["clutter"] = room(46, 120, 1, clutter=0.05, trans=0.06, deg=1.0)
    out["no_loss"] = room(47, 120, 1, huber_delta=0.0)
    out["betas_zero"] = room(48, 120, 1, beta_location_consistency=0.0, beta_orientation_consistency=0.0, beta_small_velocity=0.0)
    out["betas_mixed"] = room(49, 120, 1, beta_location_consistency=0.5, beta_orientation_consistency=0.5, beta_small_velocity=2.0)
    for cut in (WG - 1, WG, WG + 1):
        out["rows_%d" % cut] = room(50, 257, 1, vopt=dict(num_closest_neighbors=2, max_num_residuals=cut), max_num_iteration=3)
    # one row leaves the 12 unknowns to the LM diagonal: kappa ~ 1e14 makes the pose bound vacuous, so the exit thresholds are set where
    # even that bound decides them (the case is about the single-row reduction)
    out["one_row"] = room(51, 60, 1, vopt=dict(max_num_residuals=1), max_num_iteration=2, min_num_residuals=0, thres_translation_norm=1e5, thres_orientation_norm=1e7)
    out["one_row"]["converging"] = False
    out["empty_map"] = room(52, 30, 1, n_map=0)
    out["empty_map"]["converging"] = False
    out["below_min"] = room(53, 40, 1)
    out["below_min"]["converging"] = False      # (40 keypoints: the loop runs to the cap)
    # ct = 0: the end pose is carried unchanged, its rotation term is acos(1 +- rounding). Seed 103: the unclamped argument of that pose
    # against itself rounds to 1 + 4e-16 in FP64 (asserted by test_vreg_model.py), where the reference's acos gives NaN
    out["equal_rotations"] = room(103, 120, 0)
    return out


def unusable_case():
    """ct = 1 with a non-finite previous translation: H and g are NaN, every factorisation fails, five invalid steps in a row end the
    solve as Ceres' IsSolutionUsable() == false. Not one of cases(): its margins are NaN by construction."""
    c = room(55, 60, 1)
    c["prev_t"] = np.array([np.nan, 0.0, 0.0])
    return c


def build_map(case):
    m = vm.Map(case["cap"], **case["vopt"])
    if len(case["map"]):
        m.add_points(case["map"], 0)
    return m


def pose_error(x, case):
    """The registration error of the poses x = [begin | end]: RMS distance between the scan's points placed at x and placed at the scan's
    true poses. (A sum of pose errors would count the split of one motion between the begin and the end pose, which the scan observes
    only weakly; the points' displacement is what the map sees.)"""
    x = np.asarray(x, np.float64)
    d = []
    for i in range(len(case["raw"])):
        al = np.float64(case["alpha"][i]) if case["ct"] else np.float64(0)
        d.append(vm.world_point(case["ct"], x[:7], x[7:], al, case["raw"][i], np.float64) - vm.world_point(case["ct"], case["true_b"], case["true_e"], al, case["raw"][i], np.float64))
    return float(np.sqrt(np.mean(np.sum(np.square(d), axis=1))))


# K_X: the smallest power of two >= 4 r_cpu, r_cpu = the FP64 model against the longdouble model over one outer iteration from the same
# start, for every outer iteration of every case (measured by test_vreg_model.py::test_bounds_cover_four_times_the_cpu_ratio, which
# fails when a K here is not that power of two). Units u A_X, A_X as vreg_np.outer_iteration returns them.
K = dict(pose=2, cost=4, diff_trans=2, diff_rot=2)      # r_cpu: pose 0.45, cost 0.55, diff_trans 0.28, diff_rot 0.35; device worst: 0.33, 0.56, 0.24, 0.35
