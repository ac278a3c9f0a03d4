"""The validation of gfbe_line_window[] is one piece of code behind gfbe_line_refine, gfbe_line_reduce and gfbe_line_step: the same
malformed windows must be refused by all three in the same way — GFBE_BAD_INPUT before the device check, every output buffer left at
its sentinel, and an error text (where one is set) that names the function that was called. Runs on a context without a device."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf

abi, synth_line = gf.abi, gf.synth_line
FUNCS = ("gfbe_line_refine", "gfbe_line_reduce", "gfbe_line_step")


@pytest.fixture(scope="module")
def lib():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    lib.gfbe_create.restype = abi.c_i
    lib.gfbe_last_error.restype = C.c_char_p
    lib.gfbe_last_error.argtypes = [C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def windows():
    return [synth_line.line_window(seed=s, n_ok=8, n_short=1, n_late=1, n_untri=1) for s in (11, 12)]


def _holders(windows):
    """Fresh holders over private copies of the arrays (a case edits them in place)."""
    return [abi.LineWindowHolder({k: np.array(v, copy=True) for k, v in w.items()}) for w in windows]


class _Calls:
    """The three entry points over one list of holders, each with sentinel-filled outputs of its own."""

    def __init__(self, lib, ctx, windows):
        self.lib, self.ctx = lib, ctx
        n = sum(len(w["n_obs"]) for w in windows)
        nw = len(windows)
        ne = np.array([int(synth_line.eligible(w).sum()) for w in windows], np.int32)
        N = max(int(ne.sum()), 1)
        # (the step's records: only their sizes and n_eligible are looked at before the device check)
        self.rec = dict(n_eligible=ne, Vinv=np.zeros((N, 4, 4)), bl=np.zeros((N, 4)), W=np.zeros((N, 72, 4)), V=np.zeros((N, 10)),
                        failed=np.zeros(N, np.uint8))
        self.red_in = abi.line_reduced_struct_v(self.rec)
        self.plk, self.keep = np.full((n, 6), 7.25), np.full(n, 9, np.uint8)
        self.sums = (abi.Summary * nw)()
        for s in self.sums:
            s.iterations = 77
        self.rbuf = abi.line_reduced_buffers_v(nw, n, fill=7)
        self.rs = abi.line_reduced_struct_v(self.rbuf)
        self.sbuf = abi.line_stepped_buffers(nw, N, fill=7)
        self.ss = abi.line_stepped_struct(self.sbuf)
        self.y, self.rest, self.radius = np.ones((nw, 72)), np.ones((nw, 8)), np.ones(nw)

    def call(self, name, holders):
        """`name` over the holders' windows; a holder that is None goes in as a NULL window pointer."""
        PP, PD, PU8 = C.POINTER(C.POINTER(abi.LineWindow)), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        arr = (C.POINTER(abi.LineWindow) * len(holders))(*[C.pointer(h.c) if h is not None else None for h in holders])
        f = getattr(self.lib, name)
        f.restype = abi.c_i

        def pd(a):
            return a.ctypes.data_as(PD)
        if name == "gfbe_line_refine":
            f.argtypes = [C.c_void_p, abi.c_i, PP, abi.c_d, abi.c_d, abi.c_i, PD, PU8, C.POINTER(abi.Summary)]
            return f(self.ctx, len(holders), arr, 400.0, 1.0, 8, pd(self.plk), self.keep.ctypes.data_as(PU8), self.sums)
        if name == "gfbe_line_reduce":
            f.argtypes = [C.c_void_p, abi.c_i, PP, abi.c_i, abi.c_d, abi.c_d, abi.c_d, C.c_void_p]
            return f(self.ctx, len(holders), arr, abi.LINE_REDUCE_SOLVE, 400.0, 1.0, 0.0, C.byref(self.rs))
        f.argtypes = [C.c_void_p, abi.c_i, PP, C.c_void_p, abi.c_d, abi.c_d, abi.c_d, PD, PD, PD, PD, C.c_void_p]
        return f(self.ctx, len(holders), arr, C.byref(self.red_in), 400.0, 1.0, 0.0, pd(self.y), pd(self.y), pd(self.rest), pd(self.radius),
                 C.byref(self.ss))

    def untouched(self):
        return ((self.plk == 7.25).all() and (self.keep == 9).all() and all(s.iterations == 77 for s in self.sums)
                and all((a == 7).all() for a in self.rbuf.values()) and all((a == 7).all() for a in self.sbuf.values()))


def _null_window(hs):
    hs[1] = None


def _set(field, value):
    def edit(hs):
        setattr(hs[1].c, field, value)
    return edit


def _first(array, value):
    def edit(hs):
        a = getattr(hs[1], array)
        a[0] = value(hs[1]) if callable(value) else value
    return edit


# (name, the edit, whether the library sets an error text for it)
CASES = [
    ("struct_size", _set("struct_size", C.sizeof(abi.LineWindow) - 8), True),
    ("null window", _null_window, True),
    ("n_lines < 0", _set("n_lines", -1), False),
    ("null start_frame", _set("start_frame", None), False),
    ("null n_obs", _set("n_obs", None), False),
    ("null is_triangulation", _set("is_triangulation", None), False),
    ("null line_plucker", _set("line_plucker", None), False),
    ("start_frame < 0", _first("sf", -1), True),
    ("n_obs < 0", _first("no", -1), True),
    ("start_frame + n_obs = 12", _first("sf", lambda h: 12 - int(h.no[0])), True),
    ("obs == NULL", _set("obs", None), False),
]


@pytest.mark.parametrize("name,edit,has_text", CASES, ids=[c[0] for c in CASES])
def test_malformed_windows_are_refused_alike(lib, windows, name, edit, has_text):
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    try:
        calls = _Calls(lib, ctx, windows)
        for fn in FUNCS:
            hs = _holders(windows)
            edit(hs)
            rc = calls.call(fn, hs)
            assert rc == abi.BAD_INPUT, (fn, rc)
            assert calls.untouched(), fn
            if has_text:      # (the previous text in the context is another function's: the three are called in turn)
                assert lib.gfbe_last_error(ctx).startswith(fn.encode() + b":"), (fn, lib.gfbe_last_error(ctx))
    finally:
        lib.gfbe_destroy(ctx)


def test_well_formed_windows_reach_the_device_check(lib, windows):
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    try:
        calls = _Calls(lib, ctx, windows)
        for fn in FUNCS:
            assert calls.call(fn, _holders(windows)) == abi.NO_DEVICE, fn
            assert calls.untouched(), fn
            msg = lib.gfbe_last_error(ctx)
            assert msg.startswith(fn.encode() + b":") and b"no CPU fallback" in msg, (fn, msg)
    finally:
        lib.gfbe_destroy(ctx)
