"""Device line tables (gfbe_ltab_*, csrc/gfbe_ltab.hip) against the list model tests/ltab_np.py, and the table-fed line refinement
against the host-fed gfbe_line_refine, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import ltab_np as lt
from _gfbe_import import gf

abi, synth_line = gf.abi, gf.synth_line
pytestmark = pytest.mark.gpu
U = 2.0 ** -53
K_PLUCKER = 1024.0      # the multiple of tests/test_gpu_normal_equations.py (normal_equations_np.K); measured ratios in the docstrings below
DECISION_MARGIN = 1e-9
INT_KEYS = ("line_id", "start_frame", "n_obs", "is_triangulation")


@pytest.fixture(scope="module")
def be():
    return gf.Backend(device=0)


def _same_table(got, want, what, plucker=False):
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))
    assert got["obs4"].tobytes() == np.asarray(want["obs4"], float).tobytes(), "%s: obs4" % what
    if plucker:
        assert got["line_plucker"].tobytes() == np.asarray(want["line_plucker"], float).tobytes(), "%s: line_plucker" % what


def _window_pose7(stream, frames):
    p = [stream.pose7(g) for g in frames]
    return np.array(p + [p[-1]] * (lt.NFRAMES - len(p)))


def _margin_kind(g):
    return "front" if g % 3 == 1 else ("back" if g % 5 == 0 else "shift")


class Loop:
    """W streams through W tables in lockstep, the frame loop of a use_line caller; the model (if kept) runs beside it and takes the
    device's refined lines after every refine. check: compare after every operation."""

    def __init__(self, be, seeds, capacity=256, model=True, check=True, noise=0.5 / 460.0):
        self.W = len(seeds)
        made = {s: synth_line.LineStream(seed=s, noise=noise, n_frames=34) for s in set(seeds)}
        self.streams, self._frames = [made[s] for s in seeds], {}
        self.tabs = be.line_tables(self.W, capacity)
        self.models = [lt.LineTable() for _ in seeds] if model else None
        self.check, self.frames, self.fc = check, [[] for _ in seeds], 0
        self.tic_ric = np.array([abi.pose_rows(s.ex_cam[None])[0] for s in self.streams])
        self.ex = np.array([s.ex_cam for s in self.streams])
        self.min_gate_margin = np.inf
        self.n_refined = self.n_culled = self.n_triangulated = 0

    def compare(self, what, counters=None):
        if not (self.check and self.models):
            return
        np.testing.assert_array_equal(self.tabs.size(), [m.size() for m in self.models], err_msg=what)
        np.testing.assert_array_equal(self.tabs.line_count(), [m.line_count() for m in self.models], err_msg=what)
        for w, m in enumerate(self.models):
            _same_table(self.tabs.download(w), m.snapshot(), "%s, table %d" % (what, w))

    def frame(self, g):
        W, fc = self.W, self.fc
        for s in set(self.streams):
            self._frames[s] = s.frame(g)
        inc = [self._frames[s] for s in self.streams]
        cnt = self.tabs.add_frame([fc] * W, [i for i, _ in inc], [o for _, o in inc])
        for w in range(W):
            self.frames[w].append(g)
        if self.models:
            np.testing.assert_array_equal(cnt, [m.add_frame(fc, *inc[w]) for w, m in enumerate(self.models)], err_msg="counters, frame %d" % g)
        self.compare("add_frame %d" % g)
        pose7 = np.array([_window_pose7(s, self.frames[w]) for w, s in enumerate(self.streams)])
        pr = np.array([abi.pose_rows(p) for p in pose7])
        self.tabs.triangulate(pr, self.tic_ric)
        if self.models:
            for w, m in enumerate(self.models):
                for _, gate, _, done in m.triangulate(pr[w], self.tic_ric[w]):
                    self.min_gate_margin = min(self.min_gate_margin, gate)
                    self.n_triangulated += done
        self.compare("triangulate %d" % g)
        before = [self.tabs.download(w) for w in range(W)] if self.models else None
        out = self.tabs.refine(pose7, self.ex)
        if self.models:
            for w, m in enumerate(self.models):      # the model takes the device's refined lines and keep flags
                after = self.tabs.download(w)
                keep = np.isin(before[w]["line_id"], after["line_id"])
                plk = before[w]["line_plucker"].copy()
                plk[keep] = after["line_plucker"]
                m.apply_refine(plk, keep)
                self.n_culled += int((~keep).sum())
                self.n_refined += out[w]["summary"]["termination"] != 5
        self.compare("refine %d" % g)
        if fc < lt.WINDOW_SIZE:
            self.fc += 1
            return
        kind = _margin_kind(g)
        if kind == "front":
            self.tabs.remove_front([fc] * W)
            for w in range(W):
                self.frames[w].pop(lt.WINDOW_SIZE - 1)
                if self.models:
                    self.models[w].remove_front(fc)
        else:
            marg = np.array([lt.cam_pr(pose7[w][0], self.ex[w]) for w in range(W)])
            new = np.array([lt.cam_pr(pose7[w][1], self.ex[w]) for w in range(W)])
            if kind == "shift":
                self.tabs.remove_back_shift(marg, new)
            else:
                self.tabs.remove_back()
            for w in range(W):
                self.frames[w].pop(0)
                if self.models:
                    self.models[w].remove_back_shift(marg[w], new[w]) if kind == "shift" else self.models[w].remove_back()
        self.compare("slide (%s) %d" % (kind, g))

    def snapshots(self):
        return [self.tabs.download(w) for w in range(self.W)]


def test_frame_loop_parity(be):
    """32 frames of three streams, every operation every frame, all three slide kinds: ids, start frames, observation counts, triangulation
    flags, sizes, line counts and counters equal to the list model, observations bit for bit. The triangulation gate is a floating-point
    comparison: no line of these streams comes nearer to it than DECISION_MARGIN (asserted)."""
    loop = Loop(be, seeds=[41, 42, 43])
    kinds = set()
    for g in range(32):
        loop.frame(g)
        if g >= lt.WINDOW_SIZE:
            kinds.add(_margin_kind(g))
    assert kinds == {"front", "back", "shift"}
    assert loop.min_gate_margin >= DECISION_MARGIN
    print("triangulated %d, refines that solved %d, culled %d, final sizes %s" % (loop.n_triangulated, loop.n_refined, loop.n_culled, loop.tabs.size()))
    assert loop.n_triangulated >= 30 and loop.n_refined >= 10
    loop.tabs.close()


PLUCKER_SEEDS = (51, 52, 53, 54, 55, 56)


def test_triangulated_and_shifted_plucker_against_longdouble(be):
    """Every component of the triangulated and of the shifted Plücker vectors against the list model evaluated in numpy.longdouble:
    |x_dev - x_ref| <= K u A(x), A(x) the component's absolute sum as the model carries it, K = 1024 (the multiple of
    tests/test_gpu_normal_equations.py); exactly zero where A is zero. The shift is checked from the device's own triangulated
    values (exact inputs of that step). Both discrete decisions are conditions: no line of these seeds has min_cos_theta nearer
    than 1e-9 to 0.998, or its two smallest cos_theta nearer than 1e-9 to each other.
    Measured on an MI355X (worst |x_dev - x_ref| / (u A) over the seeds): triangulate %(TRI)s, shift %(SHIFT)s."""
    W = len(PLUCKER_SEEDS)
    streams = [synth_line.LineStream(seed=s) for s in PLUCKER_SEEDS]
    tabs = be.line_tables(W, 256)
    models = [lt.LineTable(np.longdouble) for _ in streams]
    for g in range(lt.NFRAMES):
        inc = [s.frame(g) for s in streams]
        tabs.add_frame([g] * W, [i for i, _ in inc], [o for _, o in inc])
        for w, m in enumerate(models):
            m.add_frame(g, *inc[w])
    pose7 = np.array([[s.pose7(g) for g in range(lt.NFRAMES)] for s in streams])
    pr = np.array([abi.pose_rows(p) for p in pose7])
    tic_ric = np.array([abi.pose_rows(s.ex_cam[None])[0] for s in streams])
    tabs.triangulate(pr, tic_ric)
    n_lines = 0
    for w, m in enumerate(models):
        for lid, gate, gap, _ in m.triangulate(pr[w], tic_ric[w]):
            assert gate >= DECISION_MARGIN and gap >= DECISION_MARGIN, (PLUCKER_SEEDS[w], lid, gate, gap)
            n_lines += 1

    def worst(what):
        r = 0.0
        for w, m in enumerate(models):
            got, ref = tabs.download(w), m.snapshot()
            np.testing.assert_array_equal(got["is_triangulation"], ref["is_triangulation"])
            A = np.asarray(ref["plucker_abs"], np.longdouble)
            err = np.abs(got["line_plucker"].astype(np.longdouble) - ref["line_plucker"])
            assert (got["line_plucker"][A == 0] == 0.0).all(), what
            ratio = np.where(A > 0, err / np.where(A > 0, U * A, 1), 0)
            r = max(r, float(ratio.max()) if ratio.size else 0.0)
        return r
    r_tri = worst("triangulate")
    print("triangulate: %d lines visited, worst ratio %.3g" % (n_lines, r_tri))
    assert n_lines >= 60
    assert r_tri <= K_PLUCKER
    # the shift, from the device's own values
    for w, m in enumerate(models):
        m.load(tabs.download(w))
    marg = np.array([lt.cam_pr(pose7[w][0], streams[w].ex_cam) for w in range(W)])
    new = np.array([lt.cam_pr(pose7[w][1], streams[w].ex_cam) for w in range(W)])
    tabs.remove_back_shift(marg, new)
    for w, m in enumerate(models):
        m.remove_back_shift(marg[w], new[w])
        _same_table(tabs.download(w), m.snapshot(), "shift, table %d" % w)
    r_shift = worst("shift")
    print("shift: worst ratio %.3g" % r_shift)
    assert r_shift <= K_PLUCKER
    tabs.close()


test_triangulated_and_shifted_plucker_against_longdouble.__doc__ %= dict(TRI="0.009 (the absolute sums carry the window positions, |P| ~ 10, through (R p + t) - t and two cross products: A ~ 1e4 |x|)", SHIFT="2.1")


def _seed_tables(be, W):
    """W tables seeded from synthetic line windows (upload): table 1 (if any) has fewer than 4 eligible lines, the last one is empty."""
    tabs = be.line_tables(W, 96)
    wins, made = [], {}
    for w in range(W):
        if W > 1 and w == 1:
            lw = synth_line.line_window(seed=700, n_ok=3, n_behind=0, n_long=0, n_outlier=0)
        elif W > 1 and w == W - 1:
            lw = synth_line.line_window(seed=701, n_ok=0, n_short=0, n_late=0, n_untri=0, n_behind=0, n_long=0, n_outlier=0)
        else:
            if w % 12 not in made:
                made[w % 12] = synth_line.line_window(seed=710 + w % 12, n_ok=20 + 5 * (w % 7), init_sigma=0.02)
            lw = made[w % 12]
        n = len(lw["start_frame"])
        off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
        obs4 = np.zeros((n, lt.NFRAMES, 4))
        for i in range(n):
            obs4[i, :lw["n_obs"][i]] = lw["obs"][off[i]:off[i + 1]]
        tabs.upload(w, dict(line_id=np.arange(n) + 1000 * w, start_frame=lw["start_frame"], n_obs=lw["n_obs"], obs4=obs4,
                            is_triangulation=lw["is_triangulation"], line_plucker=lw["line_plucker"]))
        wins.append(lw)
    return tabs, wins


@pytest.mark.parametrize("W", [1, 257])
def test_table_fed_refine_equals_host_fed_bit_for_bit(be, W):
    tabs, wins = _seed_tables(be, W)
    pose7, ex = np.array([lw["pose"] for lw in wins]), np.array([lw["ex_cam"] for lw in wins])
    before = [tabs.download(w) for w in range(W)]
    for w in range(W):          # upload -> download round-trips
        assert before[w]["line_plucker"].tobytes() == np.ascontiguousarray(wins[w]["line_plucker"], float).tobytes()
    holders = [abi.LineWindowHolder(abi.ltab_to_line_window(before[w], pose7[w], ex[w])) for w in range(W)]
    rc_h, plk, keep, sums_h = abi.line_refine_raw(be.lib, "gfbe_", be.ctx, holders)
    rc_t, sums_t = tabs.refine_raw(np.ascontiguousarray(pose7), np.ascontiguousarray(ex))
    assert rc_h == rc_t and rc_h in (abi.OK, abi.NO_CONVERGENCE)
    o = n_culled = 0
    for w in range(W):
        n = holders[w].n
        k = keep[o:o + n] != 0
        after = tabs.download(w)
        for key in INT_KEYS:
            np.testing.assert_array_equal(after[key], before[w][key][k], err_msg="table %d: %s" % (w, key))
        assert after["obs4"].tobytes() == before[w]["obs4"][k].tobytes()
        assert after["line_plucker"].tobytes() == np.ascontiguousarray(plk[o:o + n][k]).tobytes(), "table %d" % w
        for f, _ in abi.Summary._fields_:
            if f == "ms_solve":
                continue
            a, b = getattr(sums_h[w], f), getattr(sums_t[w], f)
            assert (bytes(a) == bytes(b)) if hasattr(a, "__len__") else (a == b), (w, f)
        n_culled += int((~k).sum())
        o += n
    assert n_culled >= 1
    if W > 1:
        assert sums_t[1].termination == 5 and tabs.download(1)["line_plucker"].tobytes() == before[1]["line_plucker"].tobytes()
        assert sums_t[W - 1].termination == 5 and tabs.size()[W - 1] == 0
    tabs.close()


def _run_frames(be, seeds, n_frames):
    loop = Loop(be, seeds, capacity=192, model=False, check=False)
    for g in range(n_frames):
        loop.frame(g)
    snaps = loop.snapshots()
    loop.tabs.close()
    return snaps


def test_tables_are_independent_and_deterministic(be):
    """Table 0 of a 257-table run equals the same table run alone, bit for bit, after 13 full frames (all operations, slides of
    every kind among frames 10-12); two runs of the same script give the same bits."""
    seeds = [60 + (w % 9) for w in range(257)]
    many = _run_frames(be, seeds, 13)
    alone = _run_frames(be, seeds[:1], 13)
    again = _run_frames(be, seeds[:1], 13)
    assert len(many[0]["line_id"]) > 10
    _same_table(many[0], alone[0], "table 0 of 257 against alone", plucker=True)
    _same_table(again[0], alone[0], "second run", plucker=True)
    _same_table(many[9], many[0], "the same stream in another table", plucker=True)


def test_contract(be):
    eye = np.concatenate([np.zeros(3), np.eye(3).ravel()])
    ob = lambda *ids: np.array([[i, 1.0, i + 0.5, 2.0] for i in ids], float).reshape(-1, 4)      # noqa: E731
    # remove_back erases at 0 observations left, remove_back_shift at fewer than 2
    for op, want in (("remove_back", [(1, 0, 1), (2, 0, 2)]), ("remove_back_shift", [(2, 0, 2)])):
        tabs = be.line_tables(1, 8)
        tabs.add_frame([0], [[0, 1, 2]], [ob(0, 1, 2)])
        tabs.add_frame([1], [[1, 2]], [ob(1, 2)])
        tabs.add_frame([2], [[2]], [ob(2)])
        tabs.remove_back() if op == "remove_back" else tabs.remove_back_shift([eye], [eye])
        d = tabs.download(0)
        assert list(zip(d["line_id"], d["start_frame"], d["n_obs"])) == want, op
        tabs.close()
    # upload -> download round-trips bit for bit (rows past n_obs come back zero)
    rng = np.random.default_rng(5)
    tab = dict(line_id=np.array([7, 3, 9], np.int32), start_frame=np.array([0, 2, 10], np.int32), n_obs=np.array([11, 5, 1], np.int32),
               obs4=rng.normal(size=(3, 11, 4)), is_triangulation=np.array([1, 0, 1], np.uint8), line_plucker=rng.normal(size=(3, 6)))
    for i in range(3):
        tab["obs4"][i, tab["n_obs"][i]:] = 0.0
    tabs = be.line_tables(2, 4)
    tabs.upload(1, tab)
    _same_table(tabs.download(1), tab, "round trip", plucker=True)
    assert tabs.size().tolist() == [0, 3] and tabs.line_count().tolist() == [0, 1]
    # a 12th observation: GFBE_BAD_INPUT, sticky
    with pytest.raises(RuntimeError, match="status %d" % abi.BAD_INPUT):
        tabs.add_frame([10, 10], [[], [7]], [ob(), ob(7)])
    with pytest.raises(RuntimeError, match="status %d" % abi.BAD_INPUT):
        tabs.add_frame([10, 10], [[], []], [ob(), ob()])
    tabs.close()
    # capacity overflow: GFBE_BAD_INPUT, sticky
    tabs = be.line_tables(1, 4)
    tabs.add_frame([0], [[1, 2, 3]], [ob(1, 2, 3)])
    with pytest.raises(RuntimeError, match="status %d" % abi.BAD_INPUT):
        tabs.add_frame([1], [[3, 4, 5]], [ob(3, 4, 5)])
    with pytest.raises(RuntimeError, match="status %d" % abi.BAD_INPUT):
        tabs.add_frame([2], [[]], [ob()])
    tabs.close()
    # bad arguments
    with pytest.raises(gf.BackendError):
        be.line_tables(1, 16385)
