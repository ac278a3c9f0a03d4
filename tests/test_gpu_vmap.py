"""The device voxel map and the scan-to-map association (gfbe_vmap_*) against the numpy model (tests/vmap_np.py) on the cases of
tests/vmap_cases.py. Integers, kept sets, neighbour counts and identities (neighbor_visit: the visit index of
every neighbour, in order), map contents and pts: equal / bit for bit. normals, offsets, weights, a2D
and sv: |X_dev - X_ref| <= K_X u A_X against the model in longdouble, A_X the absolute sum behind the entry (vmap_np.associate), for
the normal divided by the relative eigen-gap; K_X = the smallest power of two >= 4 r_cpu, r_cpu measured by
tests/test_vmap_model.py: normals 1.17, offsets 0.92, weights 0.80, a2D 1.27, sv 0.37 -> K = 8, 4, 4, 8, 2.
Worst device ratios of the recorded MI355X run (each test prints its own): normals 1.17, offsets 0.92, weights 0.93, a2D 1.27, sv 0.71."""
import numpy as np
import pytest

from _gfbe_import import gf
import vmap_cases as vc
import vmap_np as vm

abi = gf.abi
pytestmark = pytest.mark.gpu
CASES = vc.cases()


@pytest.fixture(scope="module")
def be():
    return gf.Backend(device=0)


def _build(be, case, cap=None):
    dm = be.voxel_map(cap or case["cap"], **case["opt"])
    for op in case["ops"]:
        dm.add_points(op[1], op[2])
    return dm


def _check_map(dm, m):
    assert dm.size() == m.size()
    d, r = dm.download(), m.download()
    for k in ("keys", "counts", "points"):
        assert np.array_equal(d[k], r[k], equal_nan=True), k


def _check_assoc(got, ref64, ref, name):
    assert got["n_res"] == ref["n_res"] and got["n_nan"] == ref["n_nan"], name
    assert np.array_equal(got["src"], ref["src"]) and np.array_equal(got["neighbor_count"][:ref["reached"]], ref["neighbor_count"][:ref["reached"]]), name
    assert np.array_equal(got["neighbor_visit"][:ref["reached"]], ref["visit"][:ref["reached"]]), name      # neighbour identities, in order
    assert np.array_equal(got["pts"], ref64["pts"]) and np.array_equal(got["alpha"], ref64["alpha"]), name
    r = vc.ratios(got, ref)
    print(name, "device ratios", {k: round(v, 3) for k, v in r.items()})
    for k, v in r.items():
        assert v <= vc.K[k], (name, k, v)
    return r


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_the_model(be, name):
    case = CASES[name]
    dm = _build(be, case)
    m, ref64 = vc.run_model(case)
    _, ref = vc.run_model(case, vm.LD)
    _check_map(dm, m)
    if case.get("expect_overflow"):
        assert dm.size()["overflow"] == 1
        with pytest.raises(RuntimeError):      # sticky: the association is refused from then on
            dm.associate(case["ct"], case["raw"], case["alpha"], case["pb"], case["pe"], case["frame_init"])
        dm.close()
        return
    got = dm.associate(case["ct"], case["raw"], case["alpha"], case["pb"], case["pe"], case["frame_init"])
    _check_assoc(got, ref64, ref, name)
    if ref["n_res"]:
        sv, deg = dm.localizability()
        svr, degr, A = vm.localizability(ref["normals"], ref["relgap_res"], vm.LD)
        ratio = float((np.abs(sv.astype(vm.LD) - svr).astype(float) / (vm.U * A)).max())
        print(name, "sv ratio", ratio)
        assert deg == degr and ratio <= vc.K["sv"]
    dm.close()


def test_room_through_three_rounds(be):
    opt, cap, steps = vc.room_rounds()
    dm, m, ml = be.voxel_map(cap, **opt), vm.Map(cap, **opt), None
    worst = {}
    for r, (add, loc, sc, pb, pe) in enumerate(steps):
        dm.add_points(add)
        dm.erase_far(loc)
        m.add_points(add)
        before = m.size()["n_voxels"]
        m.erase_far(loc)
        _check_map(dm, m)
        got = dm.associate(1, sc["raw"], sc["alpha"], pb, pe)
        ref64, ref = vm.associate(m, 1, sc["raw"], sc["alpha"], pb, pe), vm.associate(m, 1, sc["raw"], sc["alpha"], pb, pe, dtype=vm.LD)
        # the scene itself (the model's figures): the erase removes voxels, about 4 000 points stay, most keypoints find their plane
        assert m.size()["n_voxels"] < before and m.size()["n_points"] > 3000 and ref["n_res"] > len(sc["raw"]) // 2, (r, before, m.size(), ref["n_res"])
        rr = _check_assoc(got, ref64, ref, "round %d" % r)
        for k, v in rr.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("room: worst device ratios", worst)
    dm.close()


def test_a_scan_alone_equals_the_same_keypoints_inside_a_larger_scan(be):
    case = vc.room_case(41, 1500, 150, ct=1)
    dm = _build(be, case)
    rng = np.random.default_rng(9)
    pick = np.sort(rng.choice(150, 40, replace=False))
    perm = rng.permutation(150)
    big = dm.associate(1, case["raw"][perm], case["alpha"][perm], case["pb"], case["pe"])
    alone = dm.associate(1, case["raw"][pick], case["alpha"][pick], case["pb"], case["pe"])
    where = {int(perm[j]): j for j in range(150)}      # original keypoint -> place in the larger scan
    rows = {int(s): i for i, s in enumerate(big["src"])}
    assert alone["n_res"] > 20
    for i, s in enumerate(alone["src"]):
        j = rows[where[int(pick[s])]]
        for k in ("pts", "normals", "offsets", "alpha", "weights"):
            assert np.array_equal(alone[k][i], big[k][j]), k
    dm.close()


def test_layout_and_order_across_voxels_do_not_reach_the_bits(be):
    case = vc.room_case(43, 1500, 80, ct=1)
    pts = case["ops"][0][1]
    keys = [vm.point_key(p, 0.2) for p in pts]
    order = sorted(range(len(pts)), key=lambda i: (hash(keys[i]) % 97, i))      # permuted across voxels, input order inside each
    a, b = _build(be, case, cap=2048), be.voxel_map(50000, **case["opt"])
    b.add_points(pts[order])
    da, db = a.download(), b.download()
    for k in ("keys", "counts", "points"):
        assert np.array_equal(da[k], db[k]), k
    ra = a.associate(1, case["raw"], case["alpha"], case["pb"], case["pe"])
    rb = b.associate(1, case["raw"], case["alpha"], case["pb"], case["pe"])
    assert ra["n_res"] == rb["n_res"] > 40
    for k in ("src", "pts", "normals", "offsets", "alpha", "weights", "neighbor_count", "a2D"):
        assert np.array_equal(ra[k], rb[k]), k
    c = be.voxel_map(4096, **case["opt"])      # a map seeded through upload associates to the same bits
    c.upload(da["keys"], da["counts"], da["points"])
    rc = c.associate(1, case["raw"], case["alpha"], case["pb"], case["pe"])
    for k in ("src", "normals", "offsets", "weights"):
        assert np.array_equal(ra[k], rc[k]), k
    for t in (a, b, c):
        t.close()


@pytest.mark.parametrize("ct", [0, 1])
def test_linearize_equals_lio_linearize_on_the_downloaded_rows(be, ct):
    case = vc.room_case(45, 1500, 120, ct=ct)
    dm = _build(be, case)
    got = dm.associate(ct, case["raw"], case["alpha"], case["pb"], case["pe"])
    assert got["n_res"] > 50
    pb = case["pb"] + np.array([0.004, -0.003, 0.002, 0, 0, 0, 0])
    dev = dm.linearize(ct, 10.0, pb, case["pe"])
    host = abi.lio_linearize(be.lib, "gfbe_", be.ctx, ct, got["pts"], got["normals"], got["offsets"], got["alpha"], got["weights"], 10.0, pb, case["pe"], blocks=False)
    assert np.array_equal(dev["H"], host["H"]) and np.array_equal(dev["g"], host["g"]) and dev["cost"] == host["cost"]
    assert dev["cost"] > 0
    # the map changed: the held association no longer describes it
    dm.add_points([[0.31, 0.32, 0.33]])
    rc, _ = dm.linearize_raw(ct, 10.0, pb, case["pe"])
    assert rc == abi.BAD_INPUT
    with pytest.raises(RuntimeError):
        dm.localizability()
    dm.associate(ct, case["raw"], case["alpha"], case["pb"], case["pe"])
    assert dm.linearize_raw(ct, 10.0, pb, case["pe"])[0] == abi.OK
    dm.close()
