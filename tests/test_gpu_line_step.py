"""gfbe_line_step / gfbe_ltab_keep_records / gfbe_ltab_step / gfbe_ltab_commit on the GPU against the numpy checker evaluated in
numpy.longdouble (tests/line_step_np.py), entry by entry:

    |X_dev - X_ref| <= K_X u A_X,   exactly equal where A_X is zero

The records the step reads are the device's own (gfbe_line_reduce with the member V): the checker takes them as exact inputs, so the
comparison is of the step alone; the new record V is compared with the checker's V_l under its own K_V. A_X and the rule for K_X (the
smallest power of two >= 4 r_cpu, r_cpu measured on the CPU and asserted by tests/test_line_step_host.py): tests/line_step_np.py.
%(K)s

Cases: those of line_reduce_np.case_names() plus the NaN-observation window (one failed line) and sqrt_info = 0 (every line fails at
mu = 0; at mu = 1 every V' is the clamp alone), each at mu = 0 and mu = 1 and at three radii, one per dogleg branch (the caller's side -
the rest of the window P, its gradient, y_p, v_p, rest - by line_step_np.prepare from the device's reduce). The branch (read from c1, c2)
and the invalid flag must equal the checker's, and no case may sit within 1e-9 relative of a branch boundary. Bit for bit: a window
alone against the same window at shuffled places of a batch of 257; table-fed against host-fed on the downloaded list;
gfbe_ltab_reduce with records kept against the same call without. A failed line has y_l = v_l = 0 and its candidate is its input.
gfbe_ltab_commit: accept = 1 leaves exactly plucker_cand on the entering lines and every other byte of the download unchanged, accept = 0
the whole table. gfbe_ltab_step is refused after any gfbe_ltab_* mutation, after a commit and with other pose bits. The closed loop
(reduce, the checker's 72-dim solve on the host, step, commit per iteration) follows the checker's loop: the same accept / reject
sequence and iteration count, the final total cost within 1e-9 relative (the settled-solve bound of tests/test_gpu_parity.py).

Measured on an MI355X (worst |X_dev - X_ref| / (u A_X) per array over all cases, mu and radii):
%(MEASURED)s
"""
import numpy as np
import pytest

import line_reduce_np as lr
import line_step_np as ls
from _gfbe_import import gf

abi = gf.abi
pytestmark = pytest.mark.gpu

MEASURED = """  (not yet measured)"""
__doc__ = __doc__ % dict(K="  r_cpu %s\n  K     %s" % (ls.R_CPU, ls.K), MEASURED=MEASURED)
BITS = ("gram", "total", "coef", "invalid", "y_l", "v_l", "orth_cand", "plucker_cand", "pose_cand", "ex_cand", "cost_cand")
RBITS = ("H", "g", "U", "bp", "cost", "n_eligible", "n_failed", "Vinv", "bl", "W", "failed", "V")


@pytest.fixture(scope="module")
def be():
    if np.finfo(ls.LD).nmant < 63:
        pytest.skip("numpy.longdouble has no extended precision on this host")
    b = gf.Backend(device=0)
    yield b
    b.close()


_cache = {}


def device_case(be, name, mu):
    """(lw, par, the device's reduce of the window, y_p, v_p, rest, the three radii)."""
    if (name, mu) not in _cache:
        lw, par = ls.build_case(name)
        red = be.line_reduce_v([lw], lr.SOLVE, par["sqrt_info"], par["width"], mu)[0]
        y, v, rest, radii, _ = ls.prepare(name, lw, red, red, mu, par["sqrt_info"], par["width"])
        _cache[(name, mu)] = (lw, par, red, y, v, rest, radii)
    return _cache[(name, mu)]


def branch_of(coef):
    return 0 if (coef[0] == 0.0 and coef[1] == -1.0) else (1 if coef[1] == 0.0 else 2)


def compare(got, ref, label, worst):
    fails = []
    if int(got["invalid"]) != ref["invalid"]:
        fails.append("%s: invalid %d, expected %d" % (label, got["invalid"], ref["invalid"]))
    if not ref["invalid"] and branch_of(got["coef"]) != ref["branch"]:
        fails.append("%s: branch %d, expected %d" % (label, branch_of(got["coef"]), ref["branch"]))
    if not ref["margin"] > 1e-9:
        fails.append("%s: within %.1e of a branch boundary" % (label, ref["margin"]))
    rat = ls.ratios(got, ref)
    for k, (r, nz) in rat.items():
        worst[k] = max(worst.get(k, 0.0), r)
        if not r <= ls.K[k]:
            fails.append("%s: %s off by %.3g u A (K = %g)" % (label, k, r, ls.K[k]))
        if nz:
            fails.append("%s: %s differs in %d entries where the reference's allowance is zero" % (label, k, nz))
    print("%-34s " % label + "  ".join("%s %.3g" % (k, v[0]) for k, v in rat.items()))
    return fails


def same_bits(a, b, keys=BITS):
    return [k for k in keys if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]


@pytest.mark.parametrize("mu", ls.MUS)
@pytest.mark.parametrize("name", ls.case_names())
def test_one_window_alone(be, name, mu):
    lw, par, red, y, v, rest, radii = device_case(be, name, mu)
    fails, worst = [], {}
    # the new record V against the checker's V_l
    _, Vl, A_Vl = ls.line_blocks(lw, par["sqrt_info"], par["width"], ls.LD)
    ok = red["failed"] == 0
    A = ls.full_to_tri(A_Vl)[ok]
    d = np.abs(np.asarray(red["V"], ls.LD)[ok] - ls.full_to_tri(Vl)[ok])
    rv = float((d[A > 0] / (ls.UNIT * A[A > 0])).max()) if (A > 0).any() else 0.0
    assert rv <= ls.K["V"] and not d[A == 0].any(), rv
    assert not np.asarray(red["V"])[~ok].any()
    el = np.flatnonzero(lr.entering(lw, lr.SOLVE))
    for want, radius in enumerate(radii):
        got = be.line_step([lw], [red], y, v, rest, [radius], par["sqrt_info"], par["width"], mu)[0]
        ref = ls.step(lw, red, y, v, rest, radius, par["sqrt_info"], par["width"], ls.LD)
        assert ref["branch"] == want and ref["invalid"] == 0
        fails += compare(got, ref, "%s mu %g branch %d" % (name, mu, want), worst)
        bad = ~ok
        if bad.any():      # a failed line takes part in nothing; its candidate is its input, bit for bit
            assert not got["y_l"][bad].any() and not got["v_l"][bad].any()
            assert np.array_equal(got["plucker_cand"][bad], np.asarray(lw["line_plucker"], float).reshape(-1, 6)[el][bad])
        if len(el) == 0 or not ok.any():
            assert not got["gram"].any() and np.array_equal(got["total"], rest)
    print("V %.3g  worst %s" % (rv, {k: float("%.3g" % x) for k, x in worst.items()}))
    assert not fails, "\n".join(fails)


def test_failed_line_orth_candidate_is_the_line_itself(be):
    """The NaN window: the failed line's orth_cand equals the orth_cand an invalid step (no candidate formed) reports for it: x_l."""
    lw, par, red, y, v, rest, radii = device_case(be, "nan_obs", 0.0)
    bad = red["failed"] != 0
    assert bad.sum() == 1
    a = be.line_step([lw], [red], y, v, rest, [radii[0]])[0]
    # an invalid step: on the Gauss-Newton branch model_change = gy - yHy / 2, made negative through the rest's yHy
    rest_bad = rest.copy()
    rest_bad[5] = 1e30
    b = be.line_step([lw], [red], y, v, rest_bad, [radii[0]])[0]
    assert int(b["invalid"]) == 1 and b["cost_cand"] == ls.COST_INVALID
    assert np.array_equal(b["pose_cand"], np.asarray(lw["pose"], float)) and np.array_equal(b["ex_cand"], np.asarray(lw["ex_cam"], float))
    el = np.flatnonzero(lr.entering(lw, lr.SOLVE))
    assert np.array_equal(b["plucker_cand"], np.asarray(lw["line_plucker"], float).reshape(-1, 6)[el])
    assert np.array_equal(a["orth_cand"][bad], b["orth_cand"][bad])
    ref = ls.step(lw, red, y, v, rest_bad, radii[0], dtype=ls.LD)
    assert ref["invalid"] == 1
    assert not compare(b, ref, "invalid step", {})


@pytest.mark.parametrize("mu", ls.MUS)
def test_batch_of_257(be, mu):
    """Every case at shuffled places of one batch (sqrt_info, width and mu are per call: one batch per parameter set), the radii
    cycling through the three branches; each place against the same window alone, bit for bit."""
    names = ls.case_names()
    fails = []
    for key in sorted({(ls.build_case(n)[1]["sqrt_info"], ls.build_case(n)[1]["width"]) for n in names}):
        mine = [n for n in names if (ls.build_case(n)[1]["sqrt_info"], ls.build_case(n)[1]["width"]) == key]
        rng = np.random.default_rng(257 + int(mu))
        order = np.concatenate([rng.permutation(len(mine)) for _ in range(257 // len(mine) + 1)])[:257]
        cases = {n: device_case(be, n, mu) for n in mine}
        holders = {n: abi.LineWindowHolder(cases[n][0]) for n in mine}
        pick = [(mine[q], w % 3) for w, q in enumerate(order)]
        res = be.line_step([holders[n] for n, _ in pick], [cases[n][2] for n, _ in pick], np.array([cases[n][3] for n, _ in pick]),
                           np.array([cases[n][4] for n, _ in pick]), np.array([cases[n][5] for n, _ in pick]),
                           np.array([cases[n][6][b] for n, b in pick]), key[0], key[1], mu)
        alone = {}
        for w, (n, b) in enumerate(pick):
            if (n, b) not in alone:
                c = cases[n]
                alone[(n, b)] = be.line_step([holders[n]], [c[2]], c[3], c[4], c[5], [c[6][b]], key[0], key[1], mu)[0]
            d = same_bits(alone[(n, b)], res[w])
            if d:
                fails.append("%s branch %d: %s differ between alone and place %d of the batch" % (n, b, d, w))
    assert not fails, "\n".join(fails)


def test_batch_of_1025_walks_a_workgroup_to_a_second_window(be):
    """k_line_step runs at most 1024 workgroups: in a batch of 1025 the workgroup of window 0 goes on to window 1024. Small windows
    (8 lines, 5 of them entering) with distinct seeds, the radii cycling through a small, a middle and a large one; windows 0, 1, 1023
    and 1024 of the batch against the same windows stepped alone, bit for bit on every output."""
    W = 1025
    lws = [gf.synth_line.line_window(seed=7000 + k, n_ok=5, n_short=1, n_late=1, n_untri=1, n_behind=0, n_long=0, n_outlier=0) for k in range(W)]
    assert all(len(lw["n_obs"]) == 8 and int(lr.entering(lw, lr.SOLVE).sum()) >= 5 for lw in lws)
    holders = [abi.LineWindowHolder(lw) for lw in lws]
    keys = ("n_eligible", "n_failed") + abi.LINE_RECORD_KEYS
    reds = be.line_reduce_v(holders, lr.SOLVE, 400.0, 1.0, 0.0, keys)
    assert all(int(r["n_eligible"]) >= 5 and int(r["n_failed"]) == 0 for r in reds)
    rng = np.random.default_rng(1025)
    y, v = rng.normal(0, 1e-3, (W, 72)), rng.normal(0, 1e-3, (W, 72))
    rest = np.abs(rng.normal(1, 0.1, (W, 8)))
    radius = np.array([1e-3, 1.0, 1e4])[np.arange(W) % 3]
    res = be.line_step(holders, reds, y, v, rest, radius)
    assert not all(int(r["invalid"]) for r in res)
    for w in (0, 1, 1023, 1024):
        alone = be.line_step([holders[w]], [reds[w]], y[w], v[w], rest[w], radius[w:w + 1])[0]
        assert len(alone["y_l"]) == int(reds[w]["n_eligible"]) and np.isfinite(alone["cost_cand"])
        assert not same_bits(alone, res[w]), (w, same_bits(alone, res[w]))
    assert same_bits(res[0], res[1024])      # (distinct windows: the comparison above is not of one window with itself)


def _upload(tabs, w, lw):
    n = len(lw["n_obs"])
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
    obs4 = np.zeros((n, abi.NFRAMES, 4))
    for i in range(n):
        obs4[i, :lw["n_obs"][i]] = lw["obs"][off[i]:off[i + 1]]
    tabs.upload(w, dict(line_id=np.arange(n, dtype=np.int32), start_frame=lw["start_frame"], n_obs=lw["n_obs"], obs4=obs4,
                        is_triangulation=lw["is_triangulation"], line_plucker=lw["line_plucker"]))


TAB_NAMES = ["default", "lines_257", "no_eligible", "obs_11", "nan_obs"]


def _tables(be):
    lws = [ls.build_case(n)[0] for n in TAB_NAMES]
    tabs = be.line_tables(len(lws), 320)
    for w, lw in enumerate(lws):
        _upload(tabs, w, lw)
    pose7 = np.ascontiguousarray([lw["pose"] for lw in lws], float)
    ex = np.ascontiguousarray([lw["ex_cam"] for lw in lws], float)
    return lws, tabs, pose7, ex


def _caller(reds, lws, mu):
    out = [ls.prepare(TAB_NAMES[w], lws[w], reds[w], reds[w], mu, 400.0, 1.0) for w in range(len(lws))]
    y, v, rest = (np.array([o[k] for o in out]) for k in range(3))
    radius = np.array([o[3][w % 3] for w, o in enumerate(out)])
    return y, v, rest, radius


@pytest.mark.parametrize("mu", ls.MUS)
def test_table_fed_equals_host_fed_and_commit(be, mu):
    lws, tabs, pose7, ex = _tables(be)
    W = len(lws)
    try:
        plain = tabs.reduce_v(pose7, ex, lr.SOLVE, 400.0, 1.0, mu)
        with pytest.raises(RuntimeError):          # no records are held
            tabs.step(pose7, ex, np.zeros((W, 72)), np.zeros((W, 72)), np.zeros((W, 8)), np.ones(W), [p["n_eligible"] for p in plain])
        tabs.keep_records(True)
        kept = tabs.reduce_v(pose7, ex, lr.SOLVE, 400.0, 1.0, mu)
        for w in range(W):                          # records kept: the call's outputs keep their bits
            assert not same_bits(plain[w], kept[w], RBITS), (TAB_NAMES[w], same_bits(plain[w], kept[w], RBITS))
        old = tabs.reduce(pose7, ex, lr.SOLVE, 400.0, 1.0, mu)      # (the structure without V: the same bits again)
        for w in range(W):
            assert not same_bits(plain[w], old[w], [k for k in RBITS if k != "V"])
        before = [tabs.download(w) for w in range(W)]
        y, v, rest, radius = _caller(kept, lws, mu)
        ne = np.array([int(k["n_eligible"]) for k in kept])
        got = tabs.step(pose7, ex, y, v, rest, radius, ne)
        host = be.line_step([abi.ltab_to_line_window(before[w], pose7[w], ex[w]) for w in range(W)], kept, y, v, rest, radius, 400.0, 1.0, mu)
        for w in range(W):
            assert not same_bits(host[w], got[w]), (TAB_NAMES[w], same_bits(host[w], got[w]))
            assert int(got[w]["invalid"]) == 0
        mid = [tabs.download(w) for w in range(W)]
        for a, b in zip(before, mid):               # the step leaves the tables alone
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), k
        # other pose bits: refused; the records stay
        p2 = pose7.copy()
        p2[1, 3, 0] = np.nextafter(p2[1, 3, 0], 1e9)
        with pytest.raises(RuntimeError):
            tabs.step(p2, ex, y, v, rest, radius, ne)
        again = tabs.step(pose7, ex, y, v, rest, radius, ne)
        for w in range(W):
            assert not same_bits(again[w], got[w])
        # commit
        accept = np.array([1, 0, 1, 0, 1], np.uint8)
        tabs.commit(accept)
        after = [tabs.download(w) for w in range(W)]
        for w in range(W):
            want = {k: a.copy() for k, a in before[w].items()}
            if accept[w]:
                el = np.flatnonzero(lr.entering(lws[w], lr.SOLVE))
                okl = kept[w]["failed"] == 0
                want["line_plucker"][el[okl]] = got[w]["plucker_cand"][okl]
                assert np.array_equal(got[w]["plucker_cand"][~okl], before[w]["line_plucker"][el[~okl]])
            for k in want:
                assert want[k].tobytes() == after[w][k].tobytes(), (TAB_NAMES[w], k)
        assert not np.array_equal(after[0]["line_plucker"], before[0]["line_plucker"])
        with pytest.raises(RuntimeError):          # after a commit: the records and the candidates are gone
            tabs.step(pose7, ex, y, v, rest, radius, ne)
        with pytest.raises(RuntimeError):
            tabs.commit(accept)
    finally:
        tabs.close()


def test_step_is_refused_after_any_table_mutation(be):
    lws, tabs, pose7, ex = _tables(be)
    W = len(lws)
    try:
        tabs.keep_records(True)
        PR = np.tile(np.concatenate([np.zeros(3), np.eye(3).reshape(-1)]), (W, 1))
        muts = [("upload", lambda: _upload(tabs, 2, lws[2])),
                ("add_frame", lambda: tabs.add_frame([10] * W, [[100000]] * W, [np.zeros((1, 4))] * W)),
                ("triangulate", lambda: tabs.triangulate(np.tile(PR[:, None, :], (1, 11, 1)), PR)),
                ("remove_front", lambda: tabs.remove_front([10] * W)),
                ("remove_back", lambda: tabs.remove_back()),
                ("remove_back_shift", lambda: tabs.remove_back_shift(PR, PR)),
                ("refine", lambda: tabs.refine(pose7, ex, max_num_iterations=1))]
        for label, mutate in muts:
            kept = tabs.reduce_v(pose7, ex, lr.SOLVE, 400.0, 1.0, 1.0)
            ne = np.array([int(k["n_eligible"]) for k in kept])
            args = (pose7, ex, np.zeros((W, 72)), np.zeros((W, 72)), np.ones((W, 8)), np.ones(W), ne)
            tabs.step(*args)
            mutate()
            with pytest.raises(RuntimeError):
                tabs.step(*args)
            with pytest.raises(RuntimeError):
                tabs.commit(np.ones(W, np.uint8))
            print("refused after", label)
        # accept = 0 everywhere leaves the whole table unchanged
        kept = tabs.reduce_v(pose7, ex, lr.SOLVE, 400.0, 1.0, 1.0)
        ne = np.array([int(k["n_eligible"]) for k in kept])
        before = [tabs.download(w) for w in range(W)]
        tabs.step(pose7, ex, np.zeros((W, 72)), np.zeros((W, 72)), np.ones((W, 8)), np.ones(W), ne)
        tabs.commit(np.zeros(W, np.uint8))
        for w in range(W):
            b = tabs.download(w)
            for k in b:
                assert b[k].tobytes() == before[w][k].tobytes(), k
        tabs.keep_records(False)
        tabs.reduce_v(pose7, ex, lr.SOLVE, 400.0, 1.0, 1.0)
        with pytest.raises(RuntimeError):
            tabs.step(pose7, ex, np.zeros((W, 72)), np.zeros((W, 72)), np.ones((W, 8)), np.ones(W), ne)
    finally:
        tabs.close()


class DeviceOps:
    """reduce / step / commit of line_step_np.closed_loop on one device table."""

    def __init__(self, be, lw, sqrt_info=400.0, width=1.0):
        self.tabs = be.line_tables(1, 64)
        _upload(self.tabs, 0, lw)
        self.tabs.keep_records(True)
        self.pose, self.ex = np.array(lw["pose"], float).reshape(1, 11, 7), np.array(lw["ex_cam"], float).reshape(1, 7)
        self.si, self.width = sqrt_info, width

    def reduce(self, mu):
        self.red = self.tabs.reduce_v(self.pose, self.ex, lr.SOLVE, self.si, self.width, mu)[0]
        return self.red

    def step(self, y, v, rest, radius):
        self.last = self.tabs.step(self.pose, self.ex, y, v, rest, [radius], [int(self.red["n_eligible"])], self.si, self.width)[0]
        return self.last

    def commit(self, accept):
        self.tabs.commit([1 if accept else 0])
        if accept:
            self.pose, self.ex = self.last["pose_cand"].reshape(1, 11, 7).copy(), self.last["ex_cand"].reshape(1, 7).copy()


def test_closed_loop_on_the_device_follows_the_checker(be):
    import test_line_step_host as host
    lw, quad = host._perturbed()
    ref = ls.closed_loop(ls.NumpyOps(lw), quad, lw["pose"], lw["ex_cam"])
    ops = DeviceOps(be, lw)
    try:
        got = ls.closed_loop(ops, quad, lw["pose"], lw["ex_cam"])
        tab = ops.tabs.download(0)
    finally:
        ops.tabs.close()
    print("checker", ref["trace"], "%.15g" % ref["cost"])
    print("device ", got["trace"], "%.15g" % got["cost"])
    assert got["trace"] == ref["trace"] and got["iterations"] == ref["iterations"]
    assert abs(got["cost"] - ref["cost"]) <= 1e-9 * ref["cost"]
    assert all(b < a for a, b in zip(got["costs"], got["costs"][1:]))
    # the committed table reproduces the loop's final line cost
    final = lr.reduce(abi.ltab_to_line_window(tab, got["pose"], got["ex"]), lr.SOLVE)
    assert abs(float(final["cost"]) + quad.at(got["pose"], got["ex"])[0] - got["cost"]) <= 1e-9 * got["cost"]
