"""The sensor gate on the device (gfbe_gate_*, include/gfbe_gate.h) against the model (tests/gate_np.py) on the cases of tests/gate_cases.py,
whose case condition tests/test_gate_model.py checks on the CPU: gfbe_gate_frame, gfbe_gate_pair_stats in both modes and
gfbe_gate_corresponding in both modes for several (l, r) equal the model, integers exactly and doubles as bytes; the tables are byte-identical
before and after; too little room reports the count; and every refusal of the failure contract leaves sentinel-filled outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import ftab_model
import gate_cases as gc
import gate_np as m

pytestmark = pytest.mark.gpu
abi = gf.abi
PI, PD = C.POINTER(C.c_int32), C.POINTER(C.c_double)
FRAME_OUT = ("flags", "l_still", "l_init", "pair_count", "pair_sum", "dP_imu", "dP_wheel", "dis", "var", "pose_out", "vel_out")


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def world(be):
    """name -> (FeatureTables filled by the case's script, SensorGate with the case's options), built once"""
    made = {}

    def get(name):
        if name not in made:
            kw, script, robots = gc.CASES[name]
            ft = abi.FeatureTables(be.lib, "gfbe_", be.ctx, len(robots), gc.CAPACITY)
            gc.run_script_device(script, ft)
            made[name] = (ft, be.sensor_gate(len(robots), **kw))
        return made[name]
    yield get
    for ft, g in made.values():
        g.close()
        ft.close()


def _downloads(ft):
    return [ft.download(w) for w in range(ft.W)]


def _table_bytes(snaps):
    return [np.ascontiguousarray(s[k]).tobytes() for s in snaps for k in sorted(s)]


@pytest.mark.parametrize("name", gc.GPU_CASES)
def test_cases_against_the_model(world, name):
    """Three tables in one handle (empty, 30 and 1100 features: chunks of 2 with a ragged tail and idle threads) and one; tracks of every
    start and length; a table rebuilt after remove_back (the other ping-pong half); frame_count below WINDOW_SIZE and 0; 0, 1 and 20 IMU
    samples, 0, 1 and 5 wheel samples, stationary_prev 0 and 1, use_wheel 0, wdetect 0, depth_mode 0; frame lists of 1 and 12 and one with
    a zero sum_dt; the count, parallax and depth thresholds from both sides."""
    ft, g = world(name)
    want, robots = gc.expected(name), gc.CASES[name][2]
    before = _downloads(ft)
    for got, w in zip(before, gc.tables(name)):
        ftab_model.assert_same_tables(got, w)      # the device's tables are the model's
    frame = g.frame(ft, *gc.frame_args(robots))
    gc.assert_same(frame, want["frame"], (name, "frame"))
    for mode in (0, 1):
        st = g.pair_stats(ft, mode)
        gc.assert_same(st, want["stats"][mode], (name, "pair_stats", mode))
        if mode == g.opt.depth_mode:
            gc.assert_same(frame, st, (name, "frame against pair_stats"))
        for l, r in gc.LR:
            exp = want["corres"][mode, l, r]
            counts = np.array([len(a) for a, _ in exp], np.int32)
            rc, cnt, _, _, _ = g.corresponding_raw(ft, mode, [l] * g.B, [r] * g.B, np.zeros(g.B, np.int32))
            assert rc == (abi.BAD_INPUT if counts.any() else abi.OK) and np.array_equal(cnt, counts), (name, mode, l, r, cnt, counts)
            rc, cnt, a, b, off = g.corresponding_raw(ft, mode, [l] * g.B, [r] * g.B, counts)
            assert rc == abi.OK and np.array_equal(cnt, counts)
            for q, (wa, wb) in enumerate(exp):
                assert np.array_equal(gc.bits(a[off[q]:off[q + 1]]), gc.bits(wa)) and np.array_equal(gc.bits(b[off[q]:off[q + 1]]), gc.bits(wb)), (name, mode, l, r, q)
    assert _table_bytes(_downloads(ft)) == _table_bytes(before)      # the calls never modify the tables


def test_per_table_l_and_r_and_the_list_form(world):
    ft, g = world("mix3")
    o, tabs = m.options(), gc.tables("mix3")
    l, r = [0, 9, 2], [10, 10, 6]
    for mode in (0, 1):
        got = g.corresponding(ft, mode, l, r)
        for q in range(3):
            wa, wb = m.corresponding(o, mode, tabs[q], l[q], r[q])
            assert np.array_equal(gc.bits(got[q][0]), gc.bits(wa)) and np.array_equal(gc.bits(got[q][1]), gc.bits(wb))


def test_too_little_room_reports_the_count(world):
    ft, g = world("thresholds")
    counts = np.array([20, 24, 25], np.int32)      # pair (0, 10) in mode 1 (tests/test_gate_model.py)
    rc, cnt, a, b, _ = g.corresponding_raw(ft, 1, [0] * 3, [10] * 3, [20, 23, 25])
    assert rc == abi.BAD_INPUT and np.array_equal(cnt, counts) and (a == -7.0).all() and (b == -7.0).all()      # nothing but count is written
    assert b"more pairs than room" in g.lib.gfbe_last_error(g.ctx)
    rc, cnt, a, b, off = g.corresponding_raw(ft, 1, [0] * 3, [10] * 3, cnt)
    assert rc == abi.OK and np.array_equal(cnt, counts) and not (a == -7.0).any()
    # more room than pairs: the rows past a table's count stay the caller's
    rc, cnt2, a2, b2, off2 = g.corresponding_raw(ft, 1, [0] * 3, [10] * 3, counts + 3)
    assert rc == abi.OK and np.array_equal(cnt2, counts)
    for q in range(3):
        assert np.array_equal(gc.bits(a2[off2[q]:off2[q] + counts[q]]), gc.bits(a[off[q]:off[q + 1]])) and (a2[off2[q] + counts[q]:off2[q + 1]] == -7.0).all()
        assert np.array_equal(gc.bits(b2[off2[q]:off2[q] + counts[q]]), gc.bits(b[off[q]:off[q + 1]])) and (b2[off2[q] + counts[q]:off2[q + 1]] == -7.0).all()


def _p(a):
    return None if a is None else a.ctypes.data_as(PI if a.dtype == np.int32 else PD)


def _frame_call(g, ft_h, p, outs, ctx=None):
    """gfbe_gate_frame with the packed arguments p (tests/gate_cases.py pack_robots; a value may be None) and the output arrays outs"""
    return g.lib.gfbe_gate_frame(ctx or g.ctx, g.h, ft_h, _p(p["frame_count"]), _p(p["imu_off"]), _p(p["imu"]), _p(p["imu_first"]), _p(p["wheel_off"]), _p(p["wheel"]),
                                 _p(p["wheel_first"]), _p(p["pose"]), _p(p["vel_ba"]), p["g_norm"], _p(p["stationary_prev"]), _p(p["frames_off"]), _p(p["frames"]),
                                 *[_p(outs[k]) if outs is not None else None for k in FRAME_OUT])


def _sentinels(B):
    o = dict(flags=np.full(B, -7, np.int32), l_still=np.full(B, -7, np.int32), l_init=np.full(B, -7, np.int32), pair_count=np.full((B, 10), -7, np.int32),
             pair_sum=np.full((B, 10), -7.0), dP_imu=np.full((B, 3), -7.0), dP_wheel=np.full((B, 3), -7.0), dis=np.full(B, -7.0), var=np.full(B, -7.0),
             pose_out=np.full((B, 12), -7.0), vel_out=np.full((B, 3), -7.0))
    return o


def _untouched(o):
    return all((v == -7).all() for v in o.values())


def test_outputs_may_be_null(world):
    ft, g = world("mix3")
    p = gc.pack_robots(gc.CASES["mix3"][2])
    assert _frame_call(g, ft.h, p, None) == abi.OK
    assert g.lib.gfbe_gate_pair_stats(g.ctx, g.h, ft.h, 1, None, None, None, None) == abi.OK
    outs = _sentinels(3)
    for k in ("pair_sum", "dis", "pose_out"):
        outs[k] = None
    assert _frame_call(g, ft.h, p, outs) == abi.OK
    gc.assert_same(outs, {k: v for k, v in gc.expected("mix3")["frame"].items() if outs[k] is not None}, "some outputs null")


def test_refusals_leave_the_outputs_untouched(be, world):
    ft, g = world("mix3")
    robots = gc.CASES["mix3"][2]
    good = gc.pack_robots(robots)

    def refused(what, gate=g, tables_h=ft.h, ctx=None, **change):
        p = dict(good)
        p.update(change)
        outs = _sentinels(3)
        rc = _frame_call(gate, tables_h, p, outs, ctx)
        assert rc == abi.BAD_INPUT and _untouched(outs), (what, rc)
    bad_off = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(np.int32)
    refused("imu offsets from 1", imu_off=bad_off(good["imu_off"], 0, 1))
    refused("imu offsets descend", imu_off=bad_off(good["imu_off"], 1, 5))
    refused("wheel offsets descend", wheel_off=bad_off(good["wheel_off"], 2, 7))
    refused("frame offsets from -1", frames_off=bad_off(good["frames_off"], 0, -1))
    for k in ("frame_count", "imu_off", "imu", "imu_first", "wheel_off", "wheel", "wheel_first", "pose", "vel_ba", "stationary_prev", "frames_off", "frames"):
        refused(k + " NULL", **{k: None})
    refused("ftab NULL", tables_h=None)
    # B equal to the handle's n_robots but unequal to the table count
    ft1, _ = world("rest1")
    refused("table count", tables_h=ft1.h)
    # an interval above max_samples, a frame list above max_frames
    small = be.sensor_gate(3, max_samples=19, max_frames=64)
    refused("max_samples", gate=small)
    small.close()
    small = be.sensor_gate(3, max_samples=20, max_frames=11)
    refused("max_frames", gate=small)
    small.close()
    # the table half and G8
    st = {k: v for k, v in _sentinels(3).items() if k in ("pair_count", "pair_sum", "l_still", "l_init")}
    for mode in (-1, 2):
        assert g.lib.gfbe_gate_pair_stats(g.ctx, g.h, ft.h, mode, _p(st["pair_count"]), _p(st["pair_sum"]), _p(st["l_still"]), _p(st["l_init"])) == abi.BAD_INPUT and _untouched(st)
        rc, cnt, a, b, _ = g.corresponding_raw(ft, mode, [0] * 3, [10] * 3, [5] * 3)
        assert rc == abi.BAD_INPUT and (cnt == -7).all() and (a == -7.0).all() and (b == -7.0).all()
    assert g.lib.gfbe_gate_pair_stats(g.ctx, g.h, ft1.h, 1, _p(st["pair_count"]), _p(st["pair_sum"]), _p(st["l_still"]), _p(st["l_init"])) == abi.BAD_INPUT and _untouched(st)
    for l, r in (([0, 0, -1], [10] * 3), ([0, 5, 5], [10, 5, 10]), ([0, 0, 0], [10, 11, 10]), ([3, 2, 1], [2, 3, 4])):
        rc, cnt, a, b, _ = g.corresponding_raw(ft, 1, l, r, [5] * 3)
        assert rc == abi.BAD_INPUT and (cnt == -7).all() and (a == -7.0).all() and (b == -7.0).all(), (l, r)
    cnt, a = np.full(3, -7, np.int32), np.full((15, 3), -7.0)
    for off in ([1, 5, 10, 15], [0, 5, 4, 15]):
        assert g.lib.gfbe_gate_corresponding(g.ctx, g.h, ft.h, 1, _p(np.zeros(3, np.int32)), _p(np.full(3, 10, np.int32)), _p(np.array(off, np.int32)), _p(a), _p(a), _p(cnt)) == abi.BAD_INPUT
    assert g.lib.gfbe_gate_corresponding(g.ctx, g.h, ft.h, 1, None, _p(np.full(3, 10, np.int32)), _p(np.array([0, 5, 10, 15], np.int32)), _p(a), _p(a), _p(cnt)) == abi.BAD_INPUT
    assert g.lib.gfbe_gate_corresponding(g.ctx, g.h, ft.h, 1, _p(np.zeros(3, np.int32)), _p(np.full(3, 10, np.int32)), _p(np.array([0, 5, 10, 15], np.int32)), None, _p(a), _p(cnt)) == abi.BAD_INPUT
    assert (cnt == -7).all() and (a == -7.0).all()
    # a handle of another context, tables of another context
    other = gf.Backend(device=0)
    try:
        refused("the handle's context", ctx=other.ctx)
        ft_other = abi.FeatureTables(other.lib, "gfbe_", other.ctx, 3, 64)
        refused("the tables' context", tables_h=ft_other.h)
        ft_other.close()
    finally:
        other.close()
    # a table whose sticky error flag is set
    full = abi.FeatureTables(be.lib, "gfbe_", be.ctx, 3, 4)
    with pytest.raises(RuntimeError):
        full.add_frame([0] * 3, [[1, 2], [], [1, 2, 3, 4, 5, 6]], [np.zeros((2, 8)), np.zeros((0, 8)), np.zeros((6, 8))], [0.0] * 3)
    refused("sticky error flag", tables_h=full.h)
    full.close()
    # ... and the handle still answers
    gc.assert_same(g.frame(ft, *gc.frame_args(robots)), gc.expected("mix3")["frame"], "after the refusals")
