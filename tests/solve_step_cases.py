"""The windows tests/test_solve_step_reference.py (CPU) and tests/test_gpu_solve_step.py (device) check the reduced-system solve on:
one small window per launch shape of csrc/gfbe_solve.hip that changes a code path. n is the number of active dims (the reduced
system has n + 1 rows: the right-hand side rides along as the last row of the augmented matrix), nd the dims outside the eleven
speed-bias blocks (the dense tile columns of the chain kernels). Block sizes: pose 6 (x 11), speed-bias 9 (x 11), camera extrinsic 6,
td 1, wheel extrinsic 6, wheel intrinsics 3, td_wheel 1; the 58 GNSS dims of a gnss_ready window.

  prior, first, all_free, no_imu, partial     the windows of tests/test_gpu_solve_kernels.py (all_free: six dense tile columns)
  edge15 / edge0 / edge1                      n = 175 / 176 / 177: the right-hand side is the last row of a full tile / alone in a new
                                              tile row (the zlast path of the monolithic kernel) / the second row of a tile
                                              (165 + wheel extrinsic 6 + intrinsics 3 + td_wheel 1; + td 1; 165 + both extrinsics 12)
  nd63 / nd64, nd79 / nd80                    nd + 1 = 64, 65 and 80, 81: the last column of the fourth / fifth dense tile column of the
                                              chain kernels and one beyond (Pose[0] constant + intrinsics 3 [+ td_wheel]; both extrinsics +
                                              td [+ td_wheel])
  sb_const                                    SpeedBias[4] constant: identity rows inside the chain
  sb2_prior                                   a prior whose speed-bias block is relabelled SpeedBias[2]: the monolithic fallback
  gnss_a, gnss_b, gnss_prior                  the three GNSS windows of test_gpu_gnss_solve.py (the third carries a ~95-dim prior)
  gnss_nd127 / gnss_nd128, gnss_nd141         nd + 1 = 128, 129 and 142 on the nine-column kernel (wheel extrinsic constant + intrinsics
                                              [+ td_wheel]; every optional block free). nd + 1 = 144 cannot be reached: 141 is every block
                                              there is, and the plane blocks on top (145) leave the nine-column kernel.
  robust, soak_349                            of normal_equations_np (soak_349: the one large window — 3 500 landmarks, LiDAR, partial)

All tile residues n mod 16 in {15, 0, 1} are reached. EXPECTED_N is asserted on the CPU (the oracle's linearisation) and on the device."""
import numpy as np

import gnss_window_cases as gw
import normal_equations_np as ne
from _gfbe_import import gf

abi, synth = gf.abi, gf.synth

NSB = 9 * abi.NFRAMES
# (active dims n, dims outside the speed-bias blocks nd)
EXPECTED_N = {
    "prior": (171, 72), "first": (171, 72), "all_free": (182, 83), "no_imu": (66, 66), "partial": (111, 48),
    "edge15": (175, 76), "edge0": (176, 77), "edge1": (177, 78),
    "nd63": (162, 63), "nd64": (163, 64), "nd79": (178, 79), "nd80": (179, 80),
    "sb_const": (162, 72), "sb2_prior": (171, 72),
    "gnss_a": (229, 130), "gnss_b": (229, 130), "gnss_prior": (229, 130), "gnss_nd127": (226, 127), "gnss_nd128": (227, 128), "gnss_nd141": (240, 141),
    "robust": (171, 72), "soak_349": (126, 54),
}
GNSS = [k for k in EXPECTED_N if k.startswith("gnss")]
PLAIN = [k for k in EXPECTED_N if not k.startswith("gnss")]
_cache = {}


def all_free(snap, masks=True):
    """tests/test_gpu_branches.py::all_free (that module is marked gpu; the CPU half needs the same window)."""
    s = dict(snap)
    s.update(ex_cam_const=0, ex_wheel_const=0, ix_wheel_const=0, td_const=0, td_wheel_const=0)
    if masks:
        s["ex_cam_mask"] = np.array([0, 0, 1, 0, 0, 0], np.uint8)
        s["ex_wheel_mask"] = np.array([0, 0, 1, 1, 1, 0], np.uint8)
    s["ix_wheel"] = np.array([1.01, 0.99, 1.02])
    s["td"], s["td_wheel"] = 0.002, -0.003
    return s


def partial_window(seed=84, L=300, fc=6):
    """A window that is still filling up: the speed-bias blocks beyond frame_count are absent at the tail of the chain."""
    partial = dict(synth.Scenario(seed=seed, n_landmarks=L, use_wheel=True).window(0))
    keep = partial["vis_imu_j"] <= fc
    for k in list(partial):
        if k.startswith("vis_"):
            partial[k] = partial[k][keep]
    partial["frame_count"] = fc
    for k in ("imu", "imu_frame", "wheel", "wheel_frame"):
        partial[k] = partial[k][:fc]
    return partial


def no_imu_window(seed=85, L=300):
    """USE_IMU = 0: no IMU factors, no speed-bias blocks at all, Pose[0] constant."""
    no_imu = dict(synth.Scenario(seed=seed, n_landmarks=L, use_wheel=True).window(0))
    no_imu["imu"], no_imu["imu_frame"] = np.zeros((0, abi.IMU_DOUBLES)), np.zeros(0, np.int32)
    pc = np.zeros(abi.NFRAMES, np.uint8)
    pc[0] = 1
    no_imu["pose_const"] = pc
    return no_imu


def _freed(snap, **const):
    s = dict(snap)
    s.update(const)
    s["ix_wheel"] = np.array([1.01, 0.99, 1.02])
    s["td"], s["td_wheel"] = 0.002, -0.003
    return s


def _pose0_const(snap):
    s = dict(snap)
    pc = np.zeros(abi.NFRAMES, np.uint8)
    pc[0] = 1
    s["pose_const"] = pc
    return s


def build(name, oracle):
    """The window of case `name`. Deterministic; cached per process."""
    if name in _cache:
        return _cache[name]
    plain = lambda seed: synth.Scenario(seed=seed, n_landmarks=200, use_wheel=True).window(0)      # noqa: E731
    if name == "prior":
        snap = ne.window_with_prior(oracle, 81, 300)[1]
    elif name == "first":
        snap = synth.Scenario(seed=82, n_landmarks=300, use_wheel=True).window(0)
    elif name == "all_free":
        snap = all_free(ne.window_with_prior(oracle, 83, 300)[1])
    elif name == "no_imu":
        snap = no_imu_window()
    elif name == "partial":
        snap = partial_window()
    elif name == "edge15":
        snap = _freed(plain(101), ix_wheel_const=0, td_wheel_const=0)
    elif name == "edge0":
        snap = _freed(plain(102), ix_wheel_const=0, td_wheel_const=0, td_const=0)
    elif name == "edge1":
        snap = _freed(plain(103), ex_cam_const=0)
    elif name == "nd63":
        snap = _pose0_const(_freed(plain(104), ex_wheel_const=1, ix_wheel_const=0))
    elif name == "nd64":
        snap = _pose0_const(_freed(plain(105), ex_wheel_const=1, ix_wheel_const=0, td_wheel_const=0))
    elif name == "nd79":
        snap = _freed(plain(106), ex_cam_const=0, td_const=0)
    elif name == "nd80":
        snap = _freed(plain(107), ex_cam_const=0, td_const=0, td_wheel_const=0)
    elif name == "sb_const":
        snap = dict(plain(108))
        sc = np.zeros(abi.NFRAMES, np.uint8)
        sc[4] = 1
        snap["sb_const"] = sc
    elif name == "sb2_prior":
        snap = dict(ne.window_with_prior(oracle, 86, 300)[1])
        pr = dict(snap["prior"])
        ids = pr["block_id"].copy()
        assert abi.BLK_SB0 in ids.tolist()
        ids[ids.tolist().index(abi.BLK_SB0)] = abi.BLK_SB0 + 2
        pr["block_id"] = ids
        snap["prior"] = pr
    elif name == "gnss_a":
        snap = gw.gnss_window(seed=81, L=150, n_per_frame=8)[2]
    elif name == "gnss_b":
        snap = gw.gnss_window(seed=85, L=150, n_per_frame=3, anchor=True)[2]
    elif name == "gnss_prior":
        scn, tru, first = gw.gnss_window(seed=81, L=120, n_per_frame=6)
        snap = gw.next_gnss_window(scn, tru, oracle.solve(first, abi.MARGIN_OLD), seed=81)
    elif name == "gnss_nd127":
        snap = _freed(gw.gnss_window(seed=81, L=150, n_per_frame=8)[2], ex_wheel_const=1, ix_wheel_const=0)
    elif name == "gnss_nd128":
        snap = _freed(gw.gnss_window(seed=81, L=150, n_per_frame=8)[2], ex_wheel_const=1, ix_wheel_const=0, td_wheel_const=0)
    elif name == "gnss_nd141":
        snap = all_free(gw.gnss_window(seed=81, L=150, n_per_frame=8)[2], masks=False)
    elif name in ("robust", "soak_349"):
        snap = ne.build_case(name, oracle)
    else:
        raise KeyError(name)
    _cache[name] = snap
    return snap


def counts_of(act):
    """(n, nd) of an active mask over the ND tangent dims."""
    act = np.asarray(act, bool)
    return int(act.sum()), int(act.sum() - act[ne.T_SB(0):ne.T_SB(0) + NSB].sum())
