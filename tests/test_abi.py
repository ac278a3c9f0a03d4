"""CPU-side checks of the drop-in boundary: the HIP library loads without a GPU, exports every
symbol include/gfbe.h declares, the integer landmark bookkeeping (a13) is bit-exact against the
oracle, and compute entry points fail loudly (no CPU fallback) when no device is given."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _gfbe_import import gf

abi, synth = gf.abi, gf.synth
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    gf.build_native()
    return abi.bind(C.CDLL(gf.lib_path()), "gfbe_")


def test_header_symbols_all_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gfbe.h")).read()
    declared = sorted(set(re.findall(r"\b(gfbe_[a-z_0-9]+)\s*\(", hdr)))
    declared = [d for d in declared if d not in ("gfbe_allreduce_fn",)]
    table = {"gfbe_" + name for name in gf.signatures.GFBE}
    assert set(declared) == table == set(gf.backend.EXPORTS), set(declared) ^ table
    for name in declared:
        assert hasattr(lib, name), name


def test_struct_layouts_match_header(lib):
    assert C.sizeof(abi.State) == 259 * 8
    assert C.sizeof(abi.GnssObs) == 19 * 8 and C.sizeof(abi.Window) == 2536
    assert C.sizeof(abi.ImuPreint) == 467 * 8
    assert C.sizeof(abi.WheelPreint) == 78 * 8
    o = abi.Options()
    lib.gfbe_default_options(C.byref(o))
    d = abi.default_options()
    for f, _ in abi.Options._fields_:
        assert getattr(o, f) == getattr(d, f), f


def test_options_struct_size_is_checked(lib):
    """gfbe_options.struct_size: gfbe_default_options writes the library's sizeof, gfbe_options_size returns it, and
    gfbe_create refuses a struct of another size instead of reading past it."""
    assert lib.gfbe_options_size() == C.sizeof(abi.Options)
    o = abi.Options()
    lib.gfbe_default_options(C.byref(o))
    assert o.struct_size == C.sizeof(abi.Options) == abi.default_options().struct_size
    for size, want in ((o.struct_size, abi.OK), (o.struct_size - 4, abi.BAD_INPUT), (0, abi.BAD_INPUT)):
        o.struct_size = size
        ctx = C.c_void_p()
        assert lib.gfbe_create(C.byref(ctx), -1, C.byref(o)) == want
        if want != abi.OK:
            assert b"ABI mismatch" in lib.gfbe_last_error(ctx)
        lib.gfbe_destroy(ctx)


class HostOnly(abi.CApi):
    prefix = "gfbe_"

    def __init__(self, lib):
        self.lib = abi.bind(lib, "gfbe_")
        self.ctx = C.c_void_p()
        assert lib.gfbe_create(C.byref(self.ctx), -1, None) == abi.OK
        self.head = self.ctx


def test_bookkeeping_bit_exact_vs_oracle(lib, oracle):
    host = HostOnly(lib)
    for seed, extra in ((1, 0), (2, 30), (3, 100)):
        scn = synth.Scenario(seed=seed, n_landmarks=80)
        fl = scn.feature_list(0, extra_short=extra)
        fl["estimate_flag"][::5] = 1
        for only0 in (False, True):
            a, b = host.build_visual_factors(fl, only0), oracle.build_visual_factors(fl, only0)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        lam = a["para_feature"].copy()
        lam[::9] *= -1
        ea, fa = host.set_depth(fl, lam)
        eb, fb = oracle.set_depth(fl, lam)
        np.testing.assert_array_equal(ea, eb)
        np.testing.assert_array_equal(fa, fb)


def test_empty_and_ragged_feature_lists(lib, oracle):
    host = HostOnly(lib)
    empty = dict(start_frame=np.zeros(0, np.int32), n_obs=np.zeros(0, np.int32), obs=np.zeros((0, 7)),
                 obs_td=np.zeros(0), estimated_depth=np.zeros(0), estimate_flag=np.zeros(0, np.int32))
    out = host.build_visual_factors(empty)
    assert len(out["vis_imu_i"]) == 0 and len(out["para_feature"]) == 0
    # only short tracks: nothing survives the used_num >= 4 filter (feature_manager.cpp:49)
    short = dict(start_frame=np.array([0, 3, 8], np.int32), n_obs=np.array([3, 1, 2], np.int32),
                 obs=np.random.default_rng(0).normal(size=(6, 7)), obs_td=np.zeros(6),
                 estimated_depth=np.ones(3), estimate_flag=np.zeros(3, np.int32))
    out = host.build_visual_factors(short)
    assert len(out["vis_imu_i"]) == 0 and len(out["para_feature"]) == 0
    # maximum track: 11 observations from frame 0 -> 10 factors, imu_j = 1..10
    full = dict(start_frame=np.array([0], np.int32), n_obs=np.array([11], np.int32),
                obs=np.random.default_rng(1).normal(size=(11, 7)), obs_td=np.arange(11.0),
                estimated_depth=np.array([2.0]), estimate_flag=np.array([1], np.int32))
    a, b = host.build_visual_factors(full), oracle.build_visual_factors(full)
    assert a["vis_imu_j"].tolist() == list(range(1, 11)) and a["feature_const"].tolist() == [1]
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_compute_fails_loudly_without_device(lib):
    host = HostOnly(lib)
    scn = synth.Scenario(seed=4, n_landmarks=10)
    wh = abi.WindowHolder(scn.window(0))
    st, sm = abi.State(), abi.Summary()
    feat = np.zeros(wh.n_feature)
    rc = lib.gfbe_solve_window(host.ctx, C.byref(wh.c), abi.MARGIN_NONE, C.byref(st), abi._pd(feat), None, C.byref(sm))
    assert rc == abi.NO_DEVICE
    assert b"no CPU fallback" in lib.gfbe_last_error(host.ctx)


def test_backend_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(gf.BackendError):
        gf.Backend(device=0)


# The 23 public structs of include/gfbe.h and their ctypes mirrors
STRUCTS = [("gfbe_state", abi.State), ("gfbe_imu_preint", abi.ImuPreint), ("gfbe_wheel_preint", abi.WheelPreint),
           ("gfbe_visual", abi.Visual), ("gfbe_prior", abi.Prior), ("gfbe_lio_block", abi.LioBlock), ("gfbe_window", abi.Window),
           ("gfbe_options", abi.Options), ("gfbe_summary", abi.Summary), ("gfbe_feature_list", abi.FeatureList),
           ("gfbe_ftab_options", abi.FtabOptions), ("gfbe_gnss_obs", abi.GnssObs), ("gfbe_gnss_state", abi.GnssState),
           ("gfbe_lc4_options", abi.Lc4Options), ("gfbe_dmap_options", abi.DmapOptions), ("gfbe_ldb_vocab", abi.LdbVocab),
           ("gfbe_ldb_options", abi.LdbOptions), ("gfbe_vmap_options", abi.VmapOptions), ("gfbe_vreg_options", abi.VregOptions),
           ("gfbe_vreg_summary", abi.VregSummary), ("gfbe_line_window", abi.LineWindow), ("gfbe_line_reduced", abi.LineReducedV),
           ("gfbe_line_stepped", abi.LineStepped)]


def test_every_public_struct_matches_the_c_header(tmp_path):
    """sizeof and every field offset of the ctypes mirrors (abi.py) against what a C compiler makes of include/gfbe.h."""
    import subprocess
    pairs = STRUCTS
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gfbe.h")).read(), flags=re.S)
    assert sorted(c for c, _ in pairs) == sorted(re.findall(r"typedef struct (\w+) \{", hdr))       # all 23 public structs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, "%s.%s" % (cname, f)


# ---------------------------------------------------------------------------------------------
# The signature tables (signatures.py) against the prototypes of the two headers
# ---------------------------------------------------------------------------------------------
SCALARS = {"double": C.c_double, "float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint64_t": C.c_uint64,
           "int16_t": C.c_int16}
OPAQUE = ("gfbe_ctx", "gfbe_ftab", "gfbe_ltab", "gfbe_vmap", "gfbe_scan", "gfbe_dmap", "gfbe_ldb", "gfbe_batch", "gfbe_rccl")


def _vocabulary():
    """Every spelling a parameter / a return of the two headers has (pointer stars without blanks, `struct` dropped, an array in
    parameter position spelt as a pointer) -> the ctypes type the table must hold for it."""
    P = C.POINTER
    par = {"double": C.c_double, "int32_t": C.c_int32, "int": C.c_int32, "gfbe_status": C.c_int32, "int64_t": C.c_int64,
           "void*": C.c_void_p, "char*": P(C.c_char), "const char*": P(C.c_char), "const char**": P(C.c_char_p),
           "double*const*": P(P(C.c_double)), "gfbe_prior*const*": P(P(abi.Prior)),
           "const gfbe_window*const*": P(P(abi.Window)), "const gfbe_line_window*const*": P(P(abi.LineWindow)),
           "gfbe_allreduce_fn": gf.signatures.ALLREDUCE_FN}
    for name, ct in SCALARS.items():
        par[name + "*"] = par["const " + name + "*"] = P(ct)
    for cname, cls in STRUCTS:
        par[cname + "*"] = par["const " + cname + "*"] = P(cls)
    for name in OPAQUE:
        par[name + "*"] = par["const " + name + "*"] = C.c_void_p
        par[name + "**"] = P(C.c_void_p)
    ret = {"void": None, "const char*": C.c_char_p, "int32_t": C.c_int32, "gfbe_status": C.c_int32, "int64_t": C.c_int64}
    return par, ret


def _spell(t):
    return re.sub(r"\s*\*\s*", "*", " ".join(t.replace("struct ", "").split()))


def _prototypes(header, prefix):
    """[(return spelling, name, [parameter spellings])] of every `ret name(args);` of the header, comments stripped."""
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    src = re.sub(r"//[^\n]*|^\s*#.*$", " ", src, flags=re.M)
    out = []
    for ret, name, args in re.findall(r"([A-Za-z_][\w \*]*?)\b(%s\w+)\s*\(([^()]*)\)\s*;" % prefix, src):
        if "typedef" in ret:
            continue
        params = []
        for a in ([] if args.strip() in ("", "void") else args.split(",")):
            t, _, dims = re.fullmatch(r"\s*(.*?)(\w+)\s*(\[\w*\])?\s*", a, flags=re.S).groups()
            params.append(_spell(t + ("*" if dims else "")))
        out.append((_spell(ret), name, params))
    return out


@pytest.mark.parametrize("header,prefix,table,count", [("gfbe.h", "gfbe_", "GFBE", 120), ("gfbe_rccl.h", "gfbe_rccl_", "RCCL", 8)])
def test_signature_table_matches_the_header(header, prefix, table, count):
    """Every prototype of the header has a table entry with the same number of parameters, each of the ctypes type its C spelling
    stands for; a spelling the vocabulary does not list fails."""
    table = getattr(gf.signatures, table)
    protos = _prototypes(header, prefix)
    assert len(protos) == count and len({p[1] for p in protos}) == count
    assert {p[1] for p in protos} == {prefix + k for k in table}
    par, ret = _vocabulary()
    bad = []
    for r, name, params in protos:
        res, args = table[name[len(prefix):]]
        assert r in ret, "unknown return spelling %r of %s" % (r, name)
        if res is not ret[r]:
            bad.append("%s returns %s: table has %s" % (name, r, res))
        if len(args) != len(params):
            bad.append("%s takes %d parameters: table has %d" % (name, len(params), len(args)))
            continue
        for k, (p, a) in enumerate(zip(params, args)):
            assert p in par, "unknown parameter spelling %r of %s" % (p, name)
            if a is not par[p]:
                bad.append("%s parameter %d is %s: table has %s" % (name, k, p, a))
    assert not bad, "\n".join(bad)
    fn = gf.signatures.ALLREDUCE_FN                        # typedef int32_t (*gfbe_allreduce_fn)(void *, void *, int64_t, void *)
    assert fn._restype_ is C.c_int32 and tuple(fn._argtypes_) == (C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


def test_oracle_table_differs_only_where_the_oracle_does():
    s, P = gf.signatures, C.POINTER
    for name, (res, args) in s.GFBE.items():
        ores, oargs = s.GFO[name]
        assert ores is res
        if name in ("eval_factors", "solve_window"):
            assert oargs == [P(abi.Options)] + args[1:]
        elif name in ("preintegrate_imu", "preintegrate_wheel"):
            assert oargs == args[1:]
        else:
            assert oargs == args


def test_bind_types_what_a_partial_library_exports(tmp_path):
    """abi.bind on a library with two of the 120 symbols: they get their types, the others are skipped, a second bind is harmless, and
    a float where an int32_t is declared raises instead of being passed as garbage."""
    import subprocess
    src = tmp_path / "partial.c"
    src.write_text("#include <stdint.h>\n"
                   "int32_t gfbe_visual_factor_count(const void *fl, int32_t only_start_frame0) { return fl ? -1 : only_start_frame0 + 40; }\n"
                   "int32_t gfbe_options_size(void) { return 7; }\n")
    so = tmp_path / "libpartial.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    raw = C.CDLL(str(so))
    lib = abi.bind(raw, "gfbe_")
    assert lib is raw and abi.bind(lib, "gfbe_") is raw
    f = lib.gfbe_visual_factor_count
    assert f.restype is C.c_int32 and list(f.argtypes) == [C.POINTER(abi.FeatureList), C.c_int32]
    assert lib.gfbe_options_size.restype is C.c_int32 and list(lib.gfbe_options_size.argtypes) == []
    assert not hasattr(lib, "gfbe_create")
    assert f(None, 2) == 42 and lib.gfbe_options_size() == 7
    with pytest.raises(C.ArgumentError):
        f(None, 2.0)
    with pytest.raises(C.ArgumentError):
        f(C.byref(abi.State()), 2)


def test_no_signature_is_declared_outside_the_table():
    """Plain text: no .restype / .argtypes assignment in the package outside signatures.py (abi.bind applies the table through it)."""
    pkg = os.path.join(ROOT, "ground-fusion2_amd")
    stray = []
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py") and name != "signatures.py":
            for k, line in enumerate(open(os.path.join(pkg, name)), 1):
                if re.search(r"\.(restype|argtypes)\s*(,[^=\n]*)?=(?!=)", line):
                    stray.append("%s:%d: %s" % (name, k, line.strip()))
    assert not stray, "\n".join(stray)
    assert len(re.findall(r"\.(restype|argtypes)\s*(,[^=\n]*)?=(?!=)", open(os.path.join(pkg, "signatures.py")).read())) == 1
