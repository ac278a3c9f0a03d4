"""gfbe_scan_* and the hand-over (gfbe_vmap_register_scan, gfbe_vmap_add_scan_handle) on the device against the numpy model
(tests/scan_np.py). Everything integer is compared for equality (kept indices, counts, n_skipped); points that no step rewrites,
alpha and the time stamps bit for bit; the undistorted points within K u A of the longdouble model, K = scan_cases.K_POINT = 16:
the smallest power of two >= 4 r_cpu, r_cpu = 3.47 measured on the CPU by tests/test_scan_model.py. The hand-over is the same
computation as the host-fed calls on the downloaded rows: poses, every field of gfbe_vreg_summary and the maps are bit-identical.

Worst ratio |device - longdouble model| / (u A) of the undistorted points measured on the MI355X over scan_cases.undistort_cases():
3.47 (states_512), the FP64 model's own figure; per case in test_undistort's docstring."""
import numpy as np
import pytest

from _gfbe_import import gf
import scan_cases as sc
import scan_np as sn
import vmap_cases
import vmap_np as vm
import vreg_cases as vc
import vreg_np as vr

pytestmark = pytest.mark.gpu
abi = gf.abi
SUB = sc.subsample_cases()
UND = sc.undistort_cases()
VREG = vc.cases()


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def big(be):
    s = be.scan(70000)
    yield s
    s.close()


def _same_rows(got, pts, alpha, ts, kept):
    assert np.array_equal(got["src"], kept)
    assert np.array_equal(got["pts"], np.asarray(pts, np.float64).reshape(-1, 3)[kept], equal_nan=True)
    assert np.array_equal(got["alpha"], alpha[kept]) and np.array_equal(got["timestamp"], ts[kept])


@pytest.mark.parametrize("name", list(SUB))
def test_subsample(be, big, name):
    c = SUB[name]
    n = len(c["pts"])
    rng = np.random.default_rng(1)
    alpha, ts = rng.uniform(0, 1, n), rng.uniform(5, 6, n)
    kept, skipped = sn.subsample(c["pts"], c["size"])
    big.upload(c["pts"], alpha, ts)
    assert big.size() == dict(n_points=n, n_keypoints=0, n_skipped=0)
    big.subsample(c["size"])
    assert big.size() == dict(n_points=len(kept), n_keypoints=0, n_skipped=skipped)
    _same_rows(big.download(0), c["pts"], alpha, ts, kept)
    # a second pass at the same size keeps everything; nothing more is dropped
    big.subsample(c["size"])
    assert big.size() == dict(n_points=len(kept), n_keypoints=0, n_skipped=skipped)
    _same_rows(big.download(0), c["pts"], alpha, ts, kept)


def test_subsample_reversed_keeps_the_other_point(be, big):
    """The same cloud reversed keeps, of every voxel that holds several points, its LAST point of the forward order."""
    pts = SUB["cube_70000"]["pts"]
    n = len(pts)
    al = np.zeros(n)
    big.upload(pts, al)
    big.subsample(0.05)
    fwd = big.download(0)["src"]
    big.upload(pts[::-1].copy(), al)
    big.subsample(0.05)
    rev = np.sort(n - 1 - big.download(0)["src"])
    assert len(fwd) == len(rev) < n and not np.array_equal(fwd, rev)
    assert np.array_equal(rev, np.sort(n - 1 - sn.subsample(pts[::-1], 0.05)[0]))
    assert (rev >= fwd).all()      # (the k-th smallest of the voxels' last indices is not below the k-th smallest of their first ones)


@pytest.mark.parametrize("name", list(UND))
def test_undistort(be, name):
    """Worst ratio |device - longdouble model| / (u A) measured on the MI355X: branches 2.84, states_1 1.83, states_2 2.10,
    states_512 3.47, slerp_branches 1.58 (bound: K = 16)."""
    c = UND[name]
    s = be.scan(512)
    try:
        s.upload(c["pts"], c["alpha"], c["ts"])
        s.undistort(c["t"], c["poses"])
        got = s.download(0)
        ref = sn.undistort(c["pts"], c["ts"], c["t"], c["poses"], sn.LD)
        r = sc.ratio(got["pts"], ref)
        print(name, "n_states", len(c["t"]), "worst ratio", r)
        assert r <= sc.K_POINT
        assert np.array_equal(got["src"], np.arange(len(c["pts"]))) and np.array_equal(got["alpha"], c["alpha"]) and np.array_equal(got["timestamp"], c["ts"])
    finally:
        s.close()


def test_undistort_21_states_after_a_subsample(be):
    """The frame's order: the survivors of a sub-sampling are undistorted with their own time stamps."""
    c = UND["branches"]
    s = be.scan(512)
    try:
        s.upload(c["pts"], c["alpha"], c["ts"])
        s.subsample(2.0)
        kept, _ = sn.subsample(c["pts"], 2.0)
        assert 1 < len(kept) < len(c["pts"])
        s.undistort(c["t"], c["poses"])
        got = s.download(0)
        ref = sn.undistort(c["pts"][kept], c["ts"][kept], c["t"], c["poses"], sn.LD)
        assert np.array_equal(got["src"], kept) and sc.ratio(got["pts"], ref) <= sc.K_POINT
    finally:
        s.close()


def test_til_at_upload(be):
    til = np.array([0.05, -0.02, 0.1, *sc._axis_angle([1, 2, 3], 0.4)])
    pts = UND["branches"]["pts"]
    s = be.scan(512)
    try:
        s.upload(pts, np.zeros(len(pts)), None, til)
        got = s.download(0)["pts"]
        ref = np.array([sn.til_point(til, p, sn.LD) for p in pts])
        # u (|R| |p| + |t|) per rounding of the rotation, the product and the sum, as the world points of tests/test_gpu_vreg.py
        bound = 8 * sn.U * (np.abs(pts).sum(axis=1) + np.abs(til[:3]).sum() + 1)
        assert (np.abs(got.astype(sn.LD) - ref).astype(float).max(axis=1) <= bound).all()
        s.upload(pts, np.zeros(len(pts)))      # no til: the points as they are
        assert np.array_equal(s.download(0)["pts"], pts)
    finally:
        s.close()


@pytest.mark.parametrize("ct", [0, 1])
def test_keypoints(be, ct):
    c = VREG["ct1_default" if ct else "ct0_default"]
    n = len(c["raw"])
    alpha = c["alpha"] if ct else np.zeros(n)
    s = be.scan(1024)
    v = be.voxel_map(c["cap"], **c["vopt"])
    try:
        s.upload(c["raw"], alpha)
        nkp = s.keypoints(ct, c["true_b"], c["true_e"], 0.3)
        world = v.add_scan(ct, c["raw"], alpha, c["true_b"], c["true_e"], 0, want_world=True)
        kept, skipped, _ = sn.keypoints(ct, c["true_b"], c["true_e"], alpha, c["raw"], 0.3, world=world)
        assert 1 < len(kept) < n and nkp == len(kept)
        assert s.size() == dict(n_points=n, n_keypoints=len(kept), n_skipped=skipped)
        kp = s.download(1)
        _same_rows(kp, c["raw"], alpha, np.zeros(n), kept)
        # the world points the keypoints were keyed on are add_scan's, bit for bit: a scan of the keypoints alone gives world[kept]
        w2 = v.add_scan(ct, kp["pts"], kp["alpha"], c["true_b"], c["true_e"], 0, want_world=True)
        assert np.array_equal(w2, world[kept])
        # ... and a voxel size that separates every point keeps them all, one that joins them all keeps the first
        assert s.keypoints(ct, c["true_b"], c["true_e"], 1e-3) == len(sn.subsample(world, 1e-3)[0]) > len(kept)
        assert s.keypoints(ct, c["true_b"], c["true_e"], 100.0) == len(sn.subsample(world, 100.0)[0])
        _same_rows(s.download(0), c["raw"], alpha, np.zeros(n), np.arange(n))      # the points stay
    finally:
        s.close()
        v.close()


def test_keypoints_drop_points_without_a_world_voxel(be):
    pb = np.array([6000.0, 0, 0, 0, 0, 0, 1.0])      # 6000 / 0.2 = 30000: points with x > 553.4 have no voxel
    pts = np.array([[1.05, 0.3, 0.25], [600.0, 0.3, 0.25], [1.06, 0.31, 0.27], [np.nan, 0, 0], [2.5, 0.3, 0.25]])
    s = be.scan(16)
    try:
        s.upload(pts, np.zeros(5))
        assert s.keypoints(0, pb, pb, 0.2) == 2
        assert s.size() == dict(n_points=5, n_keypoints=2, n_skipped=2)
        assert s.download(1)["src"].tolist() == [0, 4]
    finally:
        s.close()


def _maps(be, c, k=2):
    first = be.voxel_map(c["cap"], **c["vopt"])
    if len(c["map"]):
        first.add_points(c["map"], 0)
    out = [first]
    d = first.download()
    for _ in range(k - 1):
        v = be.voxel_map(c["cap"], **c["vopt"])
        v.upload(d["keys"], d["counts"], d["points"])
        out.append(v)
    return out


def _same_registration(a, b):
    (rc1, ob1, oe1, s1), (rc2, ob2, oe2, s2) = a, b
    assert rc1 == rc2 == abi.OK and np.array_equal(ob1, ob2) and np.array_equal(oe1, oe2, equal_nan=True)
    assert set(s1) == set(s2)
    for k in s1:
        assert np.array_equal(np.asarray(s1[k]), np.asarray(s2[k]), equal_nan=True), k


def _same_map(a, b):
    da, db = a.download(), b.download()
    for k in ("keys", "counts", "points"):
        assert np.array_equal(da[k], db[k]), k
    assert a.size() == b.size()


@pytest.mark.parametrize("name,frame_init", [("ct1_default", 0), ("ct1_default", 1), ("ct0_default", 0), ("ct0_default", 1)])
def test_hand_over_is_the_same_computation(be, name, frame_init):
    c = VREG[name]
    ct = c["ct"]
    alpha = c["alpha"] if ct else np.zeros(len(c["raw"]))
    s = be.scan(1024)
    va, vb = _maps(be, c)
    try:
        s.upload(c["raw"], alpha)
        nkp = s.keypoints(ct, c["pb"], c["pe"], 0.25)
        kp, pts = s.download(1), s.download(0)
        assert 1 < nkp < len(c["raw"]) and len(kp["src"]) == nkp
        a = va.register_scan_raw(ct, s, c["pb"], c["pe"], c["prev_t"], c["prev_q"], frame_init, **c["o"])
        b = vb.register_raw(ct, kp["pts"], kp["alpha"], c["pb"], c["pe"], c["prev_t"], c["prev_q"], frame_init, **c["o"])
        _same_registration(a, b)
        assert a[3]["outer_iterations"] >= 1 and a[3]["n_res"][0] > 0
        before = va.size()["n_points"]
        va.add_scan_handle(ct, s, a[1], a[2], 0)
        vb.add_scan(ct, pts["pts"], pts["alpha"], b[1], b[2], 0)
        _same_map(va, vb)
        assert va.size()["n_points"] > before
    finally:
        s.close()
        va.close()
        vb.close()


def test_frame_loop(be):
    """Three rounds of the room through the handle (upload, subsample, undistort, keypoints, register_scan, add_scan_handle, erase_far)
    against the same rounds with every step done by the numpy model and the host-fed calls. The undistorted points of the host side
    are the handle's downloaded ones (the model's differ from them in rounding; they are checked within K u A), the world points the
    keypoints are keyed on come from gfbe_vmap_add_scan on a scratch map. Maps and poses bit-identical after every round."""
    vopt, cap, first, steps = sc.frame()
    s = be.scan(2048)
    va, vb, scratch = be.voxel_map(cap, **vopt), be.voxel_map(cap, **vopt), be.voxel_map(cap, **vopt)
    o = vr.options(min_num_residuals=50, max_num_iteration=3)
    try:
        va.add_points(first, 0)
        vb.add_points(first, 0)
        for r, f in enumerate(steps):
            rng = np.random.default_rng(5 + r)
            pb, pe = vc._perturb(f["pb"], rng, 0.02, 0.3), vc._perturb(f["pe"], rng, 0.02, 0.3)
            # the handle
            s.upload(f["raw"], f["alpha"], f["ts"])
            s.subsample(0.05)
            s.undistort(f["t"], f["poses"])
            nkp = s.keypoints(1, pb, pe, 0.1)
            a = va.register_scan_raw(1, s, pb, pe, f["pb"][:3], f["pb"][3:], False, **o)
            va.add_scan_handle(1, s, a[1], a[2], 0)
            va.erase_far(f["loc"])
            # the model and the host-fed calls
            kept, skipped = sn.subsample(f["raw"], 0.05)
            pts = s.download(0)
            assert np.array_equal(pts["src"], kept) and len(kept) < len(f["raw"])
            ref = sn.undistort(f["raw"][kept], f["ts"][kept], f["t"], f["poses"], sn.LD)
            assert sc.ratio(pts["pts"], ref) <= sc.K_POINT
            assert np.array_equal(pts["alpha"], f["alpha"][kept]) and np.array_equal(pts["timestamp"], f["ts"][kept])
            world = scratch.add_scan(1, pts["pts"], pts["alpha"], pb, pe, 0, want_world=True)
            kp_idx, kp_skipped, _ = sn.keypoints(1, pb, pe, pts["alpha"], pts["pts"], 0.1, world=world)
            assert nkp == len(kp_idx) and 100 < nkp < len(kept)
            assert np.array_equal(s.download(1)["src"], kept[kp_idx])
            assert s.size() == dict(n_points=len(kept), n_keypoints=nkp, n_skipped=skipped + kp_skipped)
            b = vb.register_raw(1, pts["pts"][kp_idx], pts["alpha"][kp_idx], pb, pe, f["pb"][:3], f["pb"][3:], False, **o)
            vb.add_scan(1, pts["pts"], pts["alpha"], b[1], b[2], 0)
            vb.erase_far(f["loc"])
            _same_registration(a, b)
            _same_map(va, vb)
            assert a[3]["n_res"][0] >= 50
    finally:
        s.close()
        for v in (va, vb, scratch):
            v.close()


def test_contracts(be):
    c = VREG["ct1_default"]
    n = len(c["raw"])
    ts = np.linspace(1.0, 1.1, n)
    t, P = sc.states(3, 5, t0=1.0, dt=0.025)
    s, s2 = be.scan(n), be.scan(n)
    v, = _maps(be, c, 1)
    other = gf.Backend(device=0)
    try:
        # n > capacity is refused and leaves the handle as it was
        s.upload(c["raw"][:10], c["alpha"][:10], ts[:10])
        assert s.upload_raw(np.vstack([c["raw"], c["raw"][:1]]), np.zeros(n + 1)) == abi.BAD_INPUT
        assert "capacity" in be._err()
        assert s.size()["n_points"] == 10 and np.array_equal(s.download(0)["pts"], c["raw"][:10])
        for bad in (0.0, -0.2, np.nan, np.inf):
            assert s.subsample_raw(bad) == abi.BAD_INPUT and s.keypoints_raw(1, c["pb"], c["pe"], bad)[0] == abi.BAD_INPUT
        assert s.undistort_raw(t[::-1].copy(), P) == abi.BAD_INPUT and s.undistort_raw(np.zeros(0), np.zeros((0, 7))) == abi.BAD_INPUT
        assert s.undistort_raw(np.arange(513.0), np.tile(P[0], (513, 1))) == abi.BAD_INPUT
        assert np.array_equal(s.download(0)["pts"], c["raw"][:10])
        # undistort without time stamps is refused
        s.upload(c["raw"], c["alpha"])
        assert s.undistort_raw(t, P) == abi.BAD_INPUT and "time stamps" in be._err()
        # register_scan before keypoints, and with keypoints a later upload / subsample / undistort made stale
        reg = lambda h=s, vv=v: vv.register_scan_raw(1, h, c["pb"], c["pe"], c["prev_t"], c["prev_q"], False, **c["o"])
        rc, ob, oe, sm = reg()
        assert rc == abi.BAD_INPUT and np.isnan(ob).all() and sm["outer_iterations"] == 0 and "keypoints" in be._err()
        s.upload(c["raw"], c["alpha"], ts)      # a second upload reuses the handle
        assert s.keypoints(1, c["pb"], c["pe"], 0.12) > 50
        ok = reg()
        assert ok[0] == abi.OK
        for stale in (lambda: s.subsample(0.01), lambda: s.undistort(t, P), lambda: s.upload(c["raw"], c["alpha"], ts)):
            s.keypoints(1, c["pb"], c["pe"], 0.12)
            stale()
            assert reg()[0] == abi.BAD_INPUT
            assert s.size()["n_keypoints"] == 0 and len(s.download(1)["src"]) == 0
        # two handles on one context do not disturb each other
        s.upload(c["raw"], c["alpha"], ts)
        s2.upload(c["raw"][::-1].copy(), c["alpha"][::-1].copy(), ts)
        s.keypoints(1, c["pb"], c["pe"], 0.12)
        s2.subsample(0.5)
        s2.keypoints(1, c["pb"], c["pe"], 0.3)
        _same_registration(reg(), ok)
        assert np.array_equal(s.download(0)["pts"], c["raw"]) and np.array_equal(s2.download(0)["src"], sn.subsample(c["raw"][::-1], 0.5)[0])
        # a handle of another context
        s3 = other.scan(n)
        try:
            s3.upload(c["raw"], c["alpha"])
            s3.keypoints(1, c["pb"], c["pe"], 0.12)
            assert reg(s3)[0] == abi.BAD_INPUT and "another context" in be._err()
            assert v.add_scan_handle_raw(1, s3, c["pb"], c["pe"]) == abi.BAD_INPUT
        finally:
            s3.close()
        # add_scan_handle reads the count back itself when no keypoints call did
        before = v.size()["n_points"]
        s.subsample(0.2)
        v.add_scan_handle(1, s, c["true_b"], c["true_e"])
        assert v.size()["n_points"] > before
    finally:
        s.close()
        s2.close()
        v.close()
        other.close()
