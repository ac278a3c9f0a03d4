"""The cases shared by tests/test_vmap_model.py (CPU: margins, r_cpu) and tests/test_gpu_vmap.py (device against the model): each case
is a list of operations on a map followed by one association. Seeds are chosen so that no discrete decision is nearer than 1e-9
relative to its threshold and no eigen-gap is below 1e-3 relative (asserted on the CPU by test_vmap_model.py)."""
import numpy as np

from _gfbe_import import gf
import vmap_np as vm

synth_scan = gf.synth_scan
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _plane_patch(rng, centre, n, spread=0.25, noise=0.003, normal_axis=2):
    p = rng.uniform(-spread, spread, (n, 3))
    p[:, normal_axis] = rng.normal(0, noise, n)
    return p + np.asarray(centre, float)


def room_case(seed, n_map, n_kp, ct, **opt):
    room = synth_scan.Room(seed=seed)
    poses = room.trajectory(3)
    sc = room.scan(poses[0], poses[1] if ct else poses[0], n_kp, 0.05)
    return dict(opt=opt, cap=4096, ops=[("add", room.surface(n_map, 0.05), 0)], ct=ct, raw=sc["raw"], alpha=sc["alpha"],
                pb=poses[0], pe=poses[1] if ct else poses[0], frame_init=False)


def cases():
    """name -> case. Small shapes, one per path of the kernels."""
    rng = np.random.default_rng(11)
    out = {}
    small = dict(min_number_neighbors=5, max_number_neighbors=8)
    out["empty_map"] = dict(opt={}, cap=64, ops=[], ct=0, raw=rng.uniform(-1, 1, (3, 3)), alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    out["one_point"] = dict(opt=dict(min_number_neighbors=1), cap=64, ops=[("add", [[0.31, 0.12, -0.07]], 0)], ct=0, raw=[[0.3, 0.1, -0.05]], alpha=None,
                            pb=IDENT, pe=IDENT, frame_init=False)
    # points straddling all three coordinate planes: truncation toward zero puts +-0.1 into voxel 0
    strad = _plane_patch(rng, (0.0, 0.0, 0.02), 60, spread=0.35)
    out["straddle"] = dict(opt=small, cap=256, ops=[("add", strad, 0)], ct=0, raw=[[0.05, -0.05, 0.3], [-0.15, 0.1, 0.25], [0.1, 0.15, -0.2]], alpha=None,
                           pb=np.array([0.01, 0.02, 0.0, 0, 0, 0, 1.0]), pe=IDENT, frame_init=False)
    # a voxel filled to exactly max_num_points_in_voxel, then offered one more; two close points of one voxel in one scan (order matters)
    full = np.array([[0.41 + 0.012 * (i % 4), 0.41 + 0.012 * (i // 4), 0.45 + 0.004 * (i % 3)] for i in range(6)])
    out["full_voxel"] = dict(opt=dict(max_num_points_in_voxel=6, min_distance_points=0.01, min_number_neighbors=3, max_number_neighbors=6), cap=64,
                             ops=[("add", full, 0), ("add", [[0.47, 0.47, 0.47]], 0)], ct=0, raw=[[0.437, 0.421, 0.5]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    close = np.array([[0.45, 0.45, 0.45], [0.46, 0.45, 0.45], [0.55, 0.5, 0.45], [0.452, 0.49, 0.45], [0.5, 0.55, 0.452]])
    out["close_pair"] = dict(opt=dict(min_distance_points=0.05, min_number_neighbors=3, max_number_neighbors=6), cap=64,
                             ops=[("add", close, 0), ("add", close[::-1] + 0.2, 0)], ct=0, raw=[[0.5, 0.5, 0.5]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    out["out_of_range"] = dict(opt=small, cap=256, ops=[("add", np.vstack([strad[:30], [[7000.0, 0, 0], [0, -6553.4, 0], [0.1, 0.1, np.nan]]]), 0)], ct=0,
                               raw=[[0.05, -0.05, 0.3], [9000.0, 0, 0]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    out["overflow"] = dict(opt=small, cap=8, ops=[("add", strad[:6] * 0.3, 0), ("add", strad * 3.0, 0), ("add", strad[:2] * 0.3 + 0.011, 0)], ct=0,
                           raw=[[0.0, 0.0, 0.1]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False, expect_overflow=True)
    out["min_num_points"] = dict(opt=small, cap=256, ops=[("add", strad[:30], 0), ("add", strad[30:] + [0.0, 0.0, 1.0], 3), ("add", strad[30:], 3)], ct=0,
                                 raw=[[0.05, -0.05, 0.3]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    # exactly max_number_neighbors candidates, one more, one fewer than min_number_neighbors
    for name, n in (("exact_k", 8), ("k_plus_one", 9), ("below_min", 4)):
        pts = _plane_patch(np.random.default_rng(5), (0.5, 0.5, 0.5), n, spread=0.09)
        out[name] = dict(opt=dict(small, min_distance_points=0.001), cap=64, ops=[("add", pts, 0)], ct=0, raw=[[0.5, 0.5, 0.56]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    dense = _plane_patch(np.random.default_rng(6), (0.5, 0.5, 0.5), 400, spread=0.7)
    for v in (0, 1, 2):
        out["neighborhood_%d" % v] = dict(opt=dict(voxel_neighborhood=v, min_number_neighbors=3, max_number_neighbors=20), cap=1024, ops=[("add", dense, 0)], ct=0,
                                          raw=[[0.5, 0.5, 0.56], [0.21, 0.79, 0.45], [0.9, 0.3, 0.52]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    out["frame_init"] = dict(opt=dict(voxel_neighborhood=0, threshold_voxel_occupancy=3), cap=1024, ops=[("add", dense, 0)], ct=0,
                             raw=[[0.5, 0.5, 0.56], [0.21, 0.79, 0.45]], alpha=None, pb=IDENT, pe=IDENT, frame_init=True)
    out["occupancy"] = dict(opt=dict(threshold_voxel_occupancy=4, min_number_neighbors=5), cap=1024, ops=[("add", dense, 0)], ct=0,
                            raw=[[0.5, 0.5, 0.56], [0.21, 0.79, 0.45]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    out["past_plane"] = dict(opt=dict(max_dist_to_plane_icp=0.05, num_closest_neighbors=2), cap=1024, ops=[("add", dense, 0)], ct=0,
                             raw=[[0.5, 0.5, 0.56], [0.3, 0.6, 0.53]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    # the pose below the plane: the eigenvector's sign must follow translation_begin, whichever way the solver returned it
    out["flip"] = dict(opt={}, cap=1024, ops=[("add", dense, 0)], ct=0, raw=[[0.2, 0.1, 0.3], [0.2, 0.1, -0.3]], alpha=None,
                       pb=np.array([0.3, 0.4, 0.26, 0, 0, 0, 1.0]), pe=IDENT, frame_init=False)
    out["two_closest"] = dict(opt=dict(num_closest_neighbors=2), cap=1024, ops=[("add", dense, 0)], ct=0,
                              raw=[[0.5, 0.5, 0.56], [0.3, 0.6, 0.53], [0.7, 0.2, 0.47]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    out["residual_cap"] = dict(opt=dict(num_closest_neighbors=2, max_num_residuals=4), cap=1024, ops=[("add", dense, 0)], ct=0,
                               raw=[[0.5, 0.5, 0.56], [0.3, 0.6, 0.53], [0.7, 0.2, 0.47], [0.4, 0.4, 0.5]], alpha=None, pb=IDENT, pe=IDENT, frame_init=False)
    out["residual_cap"]["opt"]["max_num_residuals"] = 3      # (cuts between the two neighbours of the second keypoint)
    for n in (1, 63, 64, 65, 257):
        out["scan_%d" % n] = room_case(20 + n, 1500, n, ct=1)
    out["room_ct0"] = room_case(7, 1500, 40, ct=0)
    return out


def run_model(case, dtype=np.float64):
    m = vm.Map(case["cap"], **case["opt"])
    for op in case["ops"]:
        if op[0] == "add":
            m.add_points(op[1], op[2])
        else:
            m.erase_far(op[1])
    return m, vm.associate(m, case["ct"], case["raw"], case["alpha"], case["pb"], case["pe"], case["frame_init"], dtype)


def ratios(got, ref):
    """worst |got - ref| / (u A) per quantity (ref: the longdouble model with its A_X)."""
    out = {}
    LD = vm.LD
    if ref["n_res"]:
        out["normals"] = float((np.abs(got["normals"].astype(LD) - ref["normals"]).astype(float) / (vm.U * ref["A_normal"][:, None])).max())
        out["offsets"] = float((np.abs(got["offsets"].astype(LD) - ref["offsets"]).astype(float) / (vm.U * ref["A_offset"])).max())
        out["weights"] = float((np.abs(got["weights"].astype(LD) - ref["weights"]).astype(float) / (vm.U * ref["A_weight"])).max())
    ok = ref["A_a2D"] > 0
    if ok.any():
        out["a2D"] = float((np.abs(np.asarray(got["a2D"])[ok].astype(LD) - ref["a2D"][ok]).astype(float) / (vm.U * ref["A_a2D"][ok])).max())
    return out


# K_X: the smallest power of two >= 4 r_cpu, r_cpu = the FP64 model against the longdouble model over cases() (measured by
# test_vmap_model.py::test_bounds_cover_four_times_the_cpu_ratio, which fails when a K here is not that power of two)
K = dict(normals=8, offsets=4, weights=4, a2D=8, sv=2)


def room_rounds(seed=31, n_map=9000, n_kp=600, rounds=3):
    """One room scene run through `rounds` add / erase / associate rounds: (options, capacity, [(add points, erase location, scan, pb, pe)])."""
    room = synth_scan.Room(seed=seed)
    poses = room.trajectory(rounds + 1)
    steps = []
    for r in range(rounds):
        sc = room.scan(poses[r], poses[r + 1], n_kp // rounds, 0.05)
        steps.append((room.surface(n_map if r == 0 else n_map // 8, 0.05), poses[r][:3] + [0.9, 0.0, 0.0], sc, poses[r], poses[r + 1]))
    return dict(max_distance=1.8), 8192, steps      # (about 4 000 map points survive min_distance_points; every erase removes some voxels)
