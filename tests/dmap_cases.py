"""The cases shared by tests/test_dmap_model.py (CPU) and tests/test_gpu_dmap.py (device against the model). A case is a map's
options and capacities and a list of steps, ("add", pose7, pts, rgb) or ("rebuild", poses). The generators ASSERT their own
conditions (check), and build their point lists from points that meet them (_select: a point that misses one is replaced by the
next of the seeded stream), so that no case is left out and every comparison with the model is exact:

  - no FP64 world coordinate lies within K u A of a float32 rounding boundary (A: the absolute sum behind the coordinate);
  - no ((double)pf - origin) / resolution lies within 1e-9 (relative) of an integer;
  - no pw.z lies within K u A of a gate, unless the pose and ex_cam are the identity (the value is then the float itself);
  - the FP64 and the longdouble model take the same decision for every point (test_dmap_model.py replays every case in both).

K = K_WORLD: the smallest power of two >= 4 r_cpu, r_cpu = the FP64 model against the longdouble model over these cases in units of
u A, measured by test_dmap_model.py::test_bound_covers_four_times_the_cpu_ratio (which fails when K is not that power of two)."""
import functools

import numpy as np

from _gfbe_import import gf
import dmap_np as dn

synth_dmap = gf.synth_dmap
K_WORLD = 32      # r_cpu 4.13 (rebuild_40; 1.0 .. 3.7 for the other posed cases) over cases(); see tests/test_dmap_model.py
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
OPEN = dict(z_min=-1e4, z_max=1e4)      # gates that drop nothing


def _is_identity(pose7, ex_cam):
    return np.array_equal(np.asarray(pose7, float), IDENT) and np.array_equal(np.asarray(ex_cam, float), IDENT)


def conditions(pose7, opt, pts, gate):
    """ok [n]: the point meets every condition of the module docstring under this pose (points without a voxel, NaN or outside the
    box by a wide margin, meet them when they are far from the box's faces)."""
    o = dict(dn.DEFAULTS, **opt)
    pw, A = dn.world(pose7, o["ex_cam"], pts, np.float64)
    pf = dn.to_float(pw)
    fin = np.isfinite(pw).all(1) & np.isfinite(pf).all(1)
    ok = np.ones(len(pw), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = np.nextafter(pf, np.float32(-np.inf)).astype(np.float64), np.nextafter(pf, np.float32(np.inf)).astype(np.float64)
        p64 = pf.astype(np.float64)
        edge = np.minimum(np.abs(pw - (p64 + lo) / 2), np.abs(pw - (p64 + hi) / 2))
        ok &= ~fin | (edge > K_WORLD * dn.U * A).all(1)
        q = dn.axis_q(pf, o["origin"], o["resolution"])
        near = (q > -1.0) & (q < 2.0 ** dn.KEY_BITS + 1.0)      # (an axis far outside the box has no face to cross)
        ok &= ~fin | (~near | (np.abs(q - np.round(q)) > 1e-9 * np.maximum(1.0, np.abs(q)))).all(1)
        if gate and not _is_identity(pose7, o["ex_cam"]):
            z = pw[:, 2]
            ok &= ~fin | ((np.abs(z - o["z_min"]) > K_WORLD * dn.U * A[:, 2]) & (np.abs(z - o["z_max"]) > K_WORLD * dn.U * A[:, 2]))
    return ok


def _select(n, draw, poses, opt, gate=True):
    """n points of the stream draw(m) -> (pts [m, 3], rgb [m, 3]) that meet the conditions under every pose of `poses`."""
    pts, rgb = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)
    while len(pts) < n:
        p, c = draw(max(64, 2 * (n - len(pts))))
        p = np.asarray(p, np.float32)
        ok = np.ones(len(p), bool)
        for pose in poses:
            ok &= conditions(pose, opt, p, gate)
        pts, rgb = np.vstack([pts, p[ok]]), np.vstack([rgb, np.asarray(c, np.uint8)[ok]])
    return pts[:n], rgb[:n]


def _pose(rng, t_scale=2.0, angle=0.6):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0.1, angle)
    return np.concatenate([rng.normal(0, t_scale, 3), np.sin(th / 2) * ax, [np.cos(th / 2)]])


def _in_voxels(rng, idx, frac=0.3):
    """float32 points inside the voxels idx [n, 3] (integers, voxel 0 at the coordinate 0), at most frac voxels off the centre."""
    return ((np.asarray(idx, float) + 0.5 + rng.uniform(-frac, frac, np.shape(idx))) * 0.01).astype(np.float32)


def _rgb(rng, n):
    return rng.integers(0, 256, (n, 3), dtype=np.uint8)


def _case(steps, pcap=None, kcap=None, **opt):
    total = sum(len(s[2]) for s in steps if s[0] == "add")
    kfs = sum(1 for s in steps if s[0] == "add")
    return dict(opt=opt, pcap=pcap or max(total, 1), kcap=kcap or max(kfs, 1), steps=steps)


EX = np.array([0.08, 0.02, 0.25, -0.5, 0.5, -0.5, 0.5])      # the camera of synth_dmap.DenseScene (looks along the body's x axis)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case. Small on purpose; chunk_* are the only large ones (the second-level scan's chunk boundary)."""
    rng = np.random.default_rng(5)
    out = {}
    out["n0"] = _case([("add", IDENT, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))])
    out["n1"] = _case([("add", IDENT, _in_voxels(rng, [[3, 4, 5]]), _rgb(rng, 1))])
    # 7 points in ONE voxel: the first 3 are kept
    out["seven_in_one_voxel"] = _case([("add", IDENT, _in_voxels(rng, np.tile([[10, -20, 30]], (7, 1))), _rgb(rng, 7))])
    # a voxel filled to 2 by an earlier keyframe (between other voxels), then 3 more candidates: one is kept
    a = _in_voxels(rng, [[1, 1, 1], [7, 7, 7], [2, 2, 2], [7, 7, 7], [3, 3, 3]])
    b = _in_voxels(rng, [[7, 7, 7], [4, 4, 4], [7, 7, 7], [7, 7, 7], [1, 1, 1]])
    out["base2_then3"] = _case([("add", IDENT, a, _rgb(rng, 5)), ("add", IDENT, b, _rgb(rng, 5))])
    # workgroup boundaries of the scan, under a pose and the camera extrinsics; a few voxels wide, so the cap decides
    for n in (255, 256, 257, 513):
        pose = _pose(rng)
        opt = dict(ex_cam=tuple(EX), **OPEN)
        pts, rgb = _select(n, lambda m: (rng.uniform(-0.03, 0.03, (m, 3)) + [0.5, 0.1, 1.0], _rgb(rng, m)), [pose], opt)
        out["wg_%d" % n] = _case([("add", pose, pts, rgb)], **opt)
    # second-level chunk boundary: 256 * 1024 + 1 points over about 64 000 voxels (4 per voxel: the cap decides), and reversed
    n = 256 * 1024 + 1
    pts, rgb = _in_voxels(rng, rng.integers(-20, 20, (n, 3))), _rgb(rng, n)
    out["chunk_262145"] = _case([("add", IDENT, pts, rgb)], **OPEN)
    out["chunk_262145_reversed"] = _case([("add", IDENT, pts[::-1].copy(), rgb[::-1].copy())], **OPEN)
    # the gates under the identity: exactly on z_min / z_max is kept, one float beyond is gated. The gates are floats off the voxel
    # faces (the defaults 2 and -0.5 ARE voxel faces, where FP64 and longdouble floor differently: 10002 / 0.01 rounds up to 1000200)
    f = np.float32
    zl, zh = f(-0.5037), f(2.0037)
    z = [zh, np.nextafter(zh, f(3)), zl, np.nextafter(zl, f(-1)), f(1.995), np.nextafter(zh, f(0)), np.nextafter(zl, f(0))]
    g = _in_voxels(rng, np.arange(21).reshape(7, 3))
    g[:, 2] = z
    out["gates"] = _case([("add", IDENT, g, _rgb(rng, 7))], z_min=float(zl), z_max=float(zh))
    # gates under a pose: points on both sides of both gates
    pose = _pose(rng, 0.3, 0.3)
    opt = dict(ex_cam=tuple(EX))
    pts, rgb = _select(300, lambda m: (rng.uniform(-2.5, 2.5, (m, 3)), _rgb(rng, m)), [pose], opt)
    out["gates_posed"] = _case([("add", pose, pts, rgb)], **opt)
    zz = dn.world(pose, EX, pts)[0][:, 2]
    assert (zz > 2).any() and (zz < -0.5).any() and ((zz < 2) & (zz > -0.5)).any()
    # NaN, infinite and outside-the-box points between good ones (their repeats fill the good points' voxels)
    good = _in_voxels(rng, [[5, 5, 5], [6, 6, 6], [5, 5, 5], [5, 5, 5], [5, 5, 5], [6, 6, 6]])
    bad = np.array([[np.nan, 0.105, 0.105], [0.105, np.inf, 0.105], [-np.inf, 0.105, 0.105], [10972.123, 0.055, 0.055], [0.055, -10000.507, 0.055], [0.055, 0.055, 3e38]], np.float32)
    mix = np.empty((12, 3), np.float32)
    mix[0::2], mix[1::2] = bad, good
    out["bad_points"] = _case([("add", IDENT, mix, _rgb(rng, 12))], **OPEN)
    # negative coordinates on every axis, under a pose
    pose = np.concatenate([[-3.0, -2.0, -1.0], _pose(rng)[3:]])
    pts, rgb = _select(200, lambda m: (rng.uniform(-0.05, 0.05, (m, 3)), _rgb(rng, m)), [pose], OPEN)
    out["negative"] = _case([("add", pose, pts, rgb)], **OPEN)
    assert (dn.world(pose, IDENT, pts)[0] < 0).all()
    # rebuilds: three keyframes by hand and 40 of the synthetic scene; the corrected poses move points into each other's voxels;
    # afterwards an insert that meets full voxels
    out["rebuild_3"] = _rebuild_case(rng, 3, 30)
    out["rebuild_40"] = _rebuild_case(rng, 40, 20)
    for name, c in out.items():
        check(c, name)
    return out


def _rebuild_case(rng, n_kf, depth_dist):
    scene = synth_dmap.DenseScene(seed=11 + n_kf, depth_dist=depth_dist)
    poses = scene.poses(n_kf + 1, dwell=8)
    fixed = scene.corrected(poses[:n_kf], yaw_drift=0.004, t_drift=(0.012, -0.008, 0.0))
    opt = dict(ex_cam=tuple(scene.ex_cam))
    steps = []
    for k in range(n_kf):
        raw = scene.keyframe(poses[k])
        ok = conditions(poses[k], opt, raw[0], True) & conditions(fixed[k], opt, raw[0], False)
        steps.append(("add", poses[k], raw[0][ok], raw[1][ok]))
    steps.append(("rebuild", fixed))
    raw = scene.keyframe(poses[n_kf])
    ok = conditions(poses[n_kf], opt, raw[0], True)
    steps.append(("add", poses[n_kf], raw[0][ok], raw[1][ok]))
    return _case(steps, **opt)


def replay(case, model):
    """Runs the steps on a dmap_np.DenseMapModel (or anything with add_keyframe / rebuild); returns the model."""
    for s in case["steps"]:
        if s[0] == "add":
            model.add_keyframe(s[1], s[2], s[3])
        else:
            model.rebuild(s[1])
    return model


def model_for(case, **kw):
    return dn.DenseMapModel(case["pcap"], case["kcap"], **dict(case["opt"], **kw))


def check(case, name=""):
    """The conditions of the module docstring at every pose a point is taken at."""
    lists = []
    for s in case["steps"]:
        if s[0] == "add":
            assert conditions(s[1], case["opt"], s[2], True).all(), name
            lists.append(s[2])
        else:
            # (a rebuild takes the lists as the inserts left them; the condition is asserted on the whole input lists, a superset)
            for pose, pts in zip(s[1], lists):
                assert conditions(pose, case["opt"], pts, False).all(), name


def world_ratio(case):
    """r of one case: the worst |FP64 model - longdouble model| / (u A) over every world coordinate the case forms."""
    o = dict(dn.DEFAULTS, **case["opt"])
    worst, lists = 0.0, []

    def one(pose, pts):
        a, A = dn.world(pose, o["ex_cam"], pts, np.float64)
        b, _ = dn.world(pose, o["ex_cam"], pts, dn.LD)
        fin = np.isfinite(a) & (A > 0)
        return float((np.abs(a.astype(dn.LD) - b).astype(float)[fin] / (dn.U * A[fin])).max()) if fin.any() else 0.0
    for s in case["steps"]:
        if s[0] == "add":
            worst = max(worst, one(s[1], s[2]))
            lists.append(s[2])
        else:
            for pose, pts in zip(s[1], lists):
                worst = max(worst, one(pose, pts))
    return worst


@functools.lru_cache(maxsize=None)
def filter_cases():
    """name -> dict(opt, pts [n, 3] float32, rgb): clouds for the radius filter, inserted under the identity with open gates and
    add_cap 8 (no voxel holds more), so the cloud is the list."""
    rng = np.random.default_rng(9)
    out = {}

    def blob(centre, n, spread):
        idx = np.round(np.asarray(centre) * 100 + rng.uniform(-spread, spread, (n, 3)) * 100).astype(int)
        return _in_voxels(rng, idx)
    # an isolated point; clusters of exactly min_neighbors and min_neighbors + 1 points; a dense cell (fast path) with sparse points
    # around it that are kept only through the dense cell's points (walk path); clusters across cell faces and the coordinate planes
    parts = [blob([20.0, 20.0, 1.0], 1, 0.0), blob([30.0, -5.0, 0.5], 10, 0.1), blob([40.0, 5.0, 0.5], 11, 0.1), blob([1.2, 1.2, 1.2], 60, 0.05),
             blob([1.2, 1.2, 1.2], 12, 0.7), blob([0.0, 0.0, 0.0], 11, 0.2), blob([0.0, 8.0, 0.0], 10, 0.2), blob([-0.4571, -3.0, 0.9142], 14, 0.15)]
    pts = np.vstack(parts)
    out["hand"] = dict(opt=dict(add_cap=8, **OPEN), pts=pts, rgb=_rgb(rng, len(pts)))
    # two points exactly `radius` apart on dyadic coordinates (radius 0.5, min_neighbors 1): kept; one float further: dropped
    f = np.float32
    pts = np.array([[0.125, 0.125, 0.125], [0.625, 0.125, 0.125], [8.125, 0.125, 0.125], [np.nextafter(f(8.625), f(9)), 0.125, 0.125],
                    [0.125, 16.125, -0.375], [0.125, 16.125, 0.125]], np.float32)
    out["exact_radius"] = dict(opt=dict(add_cap=8, filter_radius=0.5, filter_min_neighbors=1, **OPEN), pts=pts, rgb=_rgb(rng, len(pts)))
    # 5 000 random points, about 7 neighbours on average: both outcomes, mostly the walk path; dense patches take the fast path
    p = np.vstack([rng.uniform([-10, -10, -1], [10, 10, 3], (4400, 3)), rng.uniform(-0.2, 0.2, (600, 3)) + rng.integers(-8, 8, (600, 1)) * [1.0, 0.7, 0.1]])
    pts = _in_voxels(rng, np.floor(p[rng.permutation(5000)] * 100).astype(int))
    out["random_5000"] = dict(opt=dict(add_cap=8, **OPEN), pts=pts, rgb=_rgb(rng, 5000))
    for name, c in out.items():
        assert conditions(IDENT, c["opt"], c["pts"], True).all(), name
        m = dn.DenseMapModel(**c["opt"])
        assert len(m.add_keyframe(IDENT, c["pts"], c["rgb"])) == len(c["pts"]), name      # (the cloud is the list)
    return out
