"""The cases shared by tests/test_scan_model.py (CPU: the model against its independent restatements, the host build of gfbe_scan.h,
r_cpu) and tests/test_gpu_scan.py (device against the model). The generators ASSERT their own conditions: no p / size of a
sub-sampling case lies within 1e-9 (relative) of an integer, so no rounding can move a point across a voxel face; consecutive states
rotate by exactly 0 or by 1e-3 .. 0.2 rad, and no segment is near the 1e-6 s threshold. A seed that misses a condition is replaced."""
import numpy as np

from _gfbe_import import gf
import scan_np as sn
import vmap_np as vm

synth_scan = gf.synth_scan


def _assert_off_faces(pts, size):
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.asarray(pts, np.float64).reshape(-1, 3) / np.float64(size)
        q = q[np.isfinite(q) & (np.abs(q) < 32767.0)]
    assert (np.abs(q - np.round(q)) > 1e-9 * np.maximum(1.0, np.abs(q))).all()


def subsample_cases():
    """name -> dict(pts [n, 3], size)."""
    rng = np.random.default_rng(3)
    out = {}
    out["empty"] = dict(pts=np.zeros((0, 3)), size=0.2)
    out["one"] = dict(pts=np.array([[0.31, -0.12, 0.07]]), size=0.2)
    # 257 points in ONE voxel: one survivor, index 0, across a workgroup boundary
    out["one_voxel_257"] = dict(pts=np.array([0.41, 0.43, 0.45]) + rng.uniform(0, 0.15, (257, 3)), size=0.2)
    # 1 000 points in 1 000 voxels (voxel centres of a 10 x 10 x 10 block away from the coordinate planes), shuffled
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    out["thousand_voxels"] = dict(pts=(g[rng.permutation(1000)] + 3.5) * 0.2, size=0.2)
    # truncation toward zero: +-0.19 at size 0.2 share the double-width voxel at the origin
    out["origin"] = dict(pts=np.array([[0.19, 0.19, 0.19], [-0.19, -0.19, -0.19], [-0.19, 0.19, -0.19], [0.21, 0.19, 0.19], [-0.21, -0.19, -0.19]]), size=0.2)
    d = rng.uniform(-1, 1, (40, 3))
    out["duplicates"] = dict(pts=np.vstack([d, d[::2], d[5:9], d[5:9]]), size=0.3)
    # out-of-range and NaN points between good ones; a later point of the voxel of no dropped point may be lost to them
    bad = np.array([[7000.0, 0.1, 0.1], [0.1, -6553.5, 0.1], [0.1, 0.1, np.nan], [np.inf, 0.1, 0.1], [0.1, 0.1, 0.1]])
    out["out_of_range"] = dict(pts=np.vstack([bad, d[:10], bad[::-1], [[0.1, 0.1, 0.1]]]), size=0.2)
    # more than 65 536 points: the second level of the scan has more than 256 workgroups to place
    cube = rng.uniform(-10, 10, (70000, 3))
    out["cube_70000"] = dict(pts=cube, size=0.05)
    out["cube_70000_reversed"] = dict(pts=cube[::-1].copy(), size=0.05)
    for c in out.values():
        _assert_off_faces(c["pts"], c["size"])
    return out


def _axis_angle(ax, th):
    ax = np.asarray(ax, float) / np.linalg.norm(ax)
    return np.concatenate([np.sin(th / 2) * ax, [np.cos(th / 2)]])


def _qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def states(seed, n, t0=100.0, dt=0.005, still=(), negate=(), short=(), rot=(2e-3, 0.15)):
    """n nominal states: times t0 + k dt (a segment k in `short` is 5e-7 s long), a random walk of the pose; state k + 1 of a k in `still`
    repeats the quaternion of state k bit for bit; a k in `negate` stores -q (the same rotation, a negative dot product with its
    neighbours). Returns (state_time [n], state_pose [n, 7]) and asserts the generator's conditions."""
    rng = np.random.default_rng(seed)
    t, q, p = [t0], [_axis_angle(rng.normal(size=3), 0.3)], [rng.normal(0, 0.5, 3)]
    for k in range(n - 1):
        t.append(t[-1] + (5e-7 if k in short else dt))
        if k in still:
            q.append(q[-1].copy())
        else:
            qq = _qmul(q[-1], _axis_angle(rng.normal(size=3), rng.uniform(*rot)))
            q.append(qq / np.linalg.norm(qq))
        p.append(p[-1] + rng.normal(0, 0.01, 3))
    for k in negate:
        q[k] = -q[k]
    t, P = np.array(t), np.hstack([np.array(p), np.array(q)])
    for k in range(n - 1):
        d = abs(float(np.dot(P[k, 3:], P[k + 1, 3:])))
        ang = 2 * np.arccos(min(1.0, d))
        assert np.array_equal(np.abs(P[k, 3:]), np.abs(P[k + 1, 3:])) or 1e-3 <= ang <= 0.2, (k, ang)
        seg = t[k + 1] - t[k]
        assert 0 <= seg < 6e-7 or seg > 1e-4, (k, seg)      # (never near the 1e-6 s threshold)
    return t, P


def _cloud(seed, n):
    rng = np.random.default_rng(seed)
    return rng.uniform(-8, 8, (n, 3)), rng.uniform(0, 1, n)


def undistort_cases():
    """name -> dict(pts, alpha, ts, t, poses). `branches` holds one point (at least) for every branch of the time rule; the others vary
    the state count and the interpolation's own branches."""
    out = {}
    # every branch of the time rule in one case: 21 states, segment 7 is 5e-7 s long; 300 points (more than one workgroup)
    t, P = states(1, 21, short=(7,))
    pts, al = _cloud(2, 300)
    rng = np.random.default_rng(4)
    ts = rng.uniform(t[0] + 1e-4, t[-1], 300)
    ts[0] = t[-1] + 0.3            # behind the last state, inside the reference's 0.5 s allowance
    ts[1] = t[-1] + 0.9            # outside it
    ts[2] = t[0]                   # q <= t_0: segment 0, s = 0
    ts[3] = t[0] - 0.002           # in front of the first state: extrapolation, s < 0
    ts[4] = t[8]                   # in (t_7, t_8], the short segment: T_7
    ts[5] = t[12]                  # EQUAL to a state time, the >= side: segment 11 at s = 1
    ts[6] = t[-1]                  # equal to the last time: the last segment at s = 1, not 'behind'
    ts[7] = t[1]                   # segment 0 at s = 1
    ts[8] = np.nextafter(t[12], np.inf)      # just past a state time: segment 12
    out["branches"] = dict(pts=pts, alpha=al, ts=ts, t=t, poses=P)
    have = {sn.branch(t, q) for q in ts}
    assert have == {"behind", "front", "short", "interp"}, have
    assert sn.segment(t, ts[5]) == 11 and sn.segment(t, ts[6]) == 19 and sn.segment(t, ts[8]) == 12 and sn.segment(t, ts[4]) == 7
    for n in (1, 2, 512):
        t, P = states(10 + n, n, dt=0.1 / max(n - 1, 1) if n > 2 else 0.1)
        pts, al = _cloud(20 + n, 40)
        ts = np.random.default_rng(30 + n).uniform(t[0] - 0.01, t[-1] + 0.02, 40)
        out["states_%d" % n] = dict(pts=pts, alpha=al, ts=ts, t=t, poses=P)
    assert sn.branch(out["states_1"]["t"], 100.0) == "single"
    # two equal quaternions (slerp's linear branch) and a pair with a negative dot product
    t, P = states(5, 6, still=(1, 3), negate=(3,))
    assert np.array_equal(P[1, 3:], P[2, 3:]) and np.dot(P[2, 3:], P[3, 3:]) < 0 and np.array_equal(P[3, 3:], -P[4, 3:])
    pts, al = _cloud(6, 60)
    out["slerp_branches"] = dict(pts=pts, alpha=al, ts=np.random.default_rng(7).uniform(t[0] + 1e-4, t[-1], 60), t=t, poses=P)
    segs = {sn.segment(t, q) for q in out["slerp_branches"]["ts"]}
    assert {1, 2, 3} <= segs
    return out


def ratio(got, ref):
    """worst |got - ref| / (u A) over the points of one undistortion (ref: scan_np.undistort in longdouble)."""
    if not len(ref["pts"]):
        return 0.0
    return float((np.abs(np.asarray(got, np.float64).astype(sn.LD) - ref["pts"]).astype(float) / (sn.U * ref["A"])).max())


# K: the smallest power of two >= 4 r_cpu, r_cpu = the FP64 model against the longdouble model over undistort_cases() (measured by
# test_scan_model.py::test_bound_covers_four_times_the_cpu_ratio, which fails when K is not that power of two). Units u A.
K_POINT = 16      # r_cpu 3.47 (states_512; 1.6 .. 2.8 for the other cases); the device's worst ratio: see tests/test_gpu_scan.py


def frame(seed=31, rounds=3, n_scan=900, n_map=9000):
    """The room scene of vmap_cases.room_rounds as a driver would deliver it: per round the scan with time stamps and the nominal
    states of its sweep (21 states over 0.1 s, a small motion on top of the scan's own), the predicted poses and the erase location.
    (options, capacity, first map points, [dict(raw, alpha, ts, t, poses, pb, pe, loc)])."""
    room = synth_scan.Room(seed=seed)
    poses = room.trajectory(rounds + 1)
    steps = []
    for r in range(rounds):
        sc = room.scan(poses[r], poses[r + 1], n_scan, 0.05)
        t, P = states(70 + r, 21, t0=10.0 + 0.1 * r, dt=0.005, rot=(1.1e-3, 2e-3))
        P[:, :3] *= 0.02      # (centimetres of motion inside the sweep)
        steps.append(dict(raw=sc["raw"], alpha=sc["alpha"], ts=t[0] + sc["alpha"] * (t[-1] - t[0]), t=t, poses=P, pb=poses[r], pe=poses[r + 1],
                          loc=poses[r][:3] + [0.9, 0.0, 0.0]))
    return dict(max_distance=1.8), 8192, room.surface(n_map, 0.05), steps
