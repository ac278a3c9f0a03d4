"""The new prior of the device's marginalisation (csrc/gfbe_marg.hip: k_marg, k_marg_ldlt<4 / 6 / 8>, k_marg_ldlt_tp, tridiag_dc,
tridiag_ql_eig) against the extended-precision model of tests/prior_np.py, at every size at which the launch logic takes another
path, with the checker and the bounds of tests/test_prior_reference.py (K = smallest power of two >= 4 r_cpu, in units of
u = 2^-53: rA %(KA)g, rb %(Kb)g, ro %(Ko)g; block table, x0 and the number of rows exact).

What these cases do not pin. Every case has full rank (prior_np's docstring: the gap condition admits no other), so the new prior
keeps all n rows at every size: the rank decision at marg_eps and the zero rows of a thresholded prior are NOT exercised here; they
stay with tests/test_gpu_parity.py::test_prior_square_root_modes and the check_prior calls against the oracle. And rb has teeth
only in the gnss and nowheel cases: its scale is max(b_scale, 1e-2 a_scale), and for the windows with a grown prior (85 .. 177, both
MARGIN_SECOND_NEW cases) b_scale is ~1e4 against 1e-2 a_scale = 6.7e9 — the device measures 1.2e-4 u there, an error of r0 would
have to be ~1e7 roundings to show. J0 of those cases is held by rA and ro.

The prior comes from Backend.solve / solve_batch with max_num_iterations = 0: no step is taken, but the re-anchoring rewrites
every quaternion through a rotation matrix, so the state the device marginalises at differs from the window's in the last bits
(asserted: within 1e-14, the inverse depths unchanged). The model is built at the state the device returns (x0 of the prior is
compared exactly with it), not at the window's: no A' dx term is left to allow for.

Launch shapes, both marg_sqrt modes:
  alone                  k_marg on 1024 threads; k_marg_ldlt<4> (n <= 88), <6> (<= 132), <8> (<= 176); n = 177: the eigen path under
                         marg_sqrt = 1; eigen mode: tridiag_dc in LDS up to n = 90, the global-memory QL above
  batch of 13            B < 32: <4>, <6> and <8> launched into one batch, each leaving the other kinds' windows alone
  batch of 33, all       every MARGIN_OLD case at shuffled places, each at least twice: k_marg on 512 threads (n = 89, 90: two passes
                         of tridiag_dc's M8), k_marg_ldlt_tp + <6> + <8> launched into one batch
  batch of 33, <= 88     prior_np.WITHIN_88 only — the cases whose HOST bound (the larger of the incoming prior's n and the
                         MARGIN_OLD bound, csrc/gfbe_upload.h) is <= 88: marg_nmax keeps <6> and <8> unlaunched, k_marg_ldlt_tp alone
  MARGIN_SECOND_NEW      alone, as a batch of 2 and as a batch of 33 of its own
Across shapes: a case that occurs twice in a batch is bit-identical to itself. Inside one kernel set a window does not depend on
its batch, in bits, in both modes: alone against the batch of 13, and the batch of 33 with every size against the one within 88
(B >= 32). ACROSS the two sets (alone against a batch of 33) the prior is not the same bits in either mode: the Householder phase
of the eigen path sums blockDim / 128 partial products per row (1024 against 512 threads), k_marg_ldlt<4> and k_marg_ldlt_tp
differ by design, and the partials k_marg sums come from other kernels (k_lin_small against k_vis / k_pairsum / k_schur / k_dense).
What holds across the sets, and is asserted in both modes: the same state, the same number of rows, and J0^T J0, J0^T r0 within
2 K of each other.

MEASURED on an MI355X (worst ratio over the cases of a shape, in units of u; bounds rA 512, rb 1024, ro 32):
  launch shape                          marg_sqrt 0 (eigen)            marg_sqrt 1 (LDL^T)      worst case
                                        rA      rb      ro             rA      rb
  alone, B = 13                       6.91    2.92    15.2           6.91    2.92             rA: old_177   rb: gnss   ro: old_132
  B = 33, every size                  6.91    2.92    11.7           6.91    2.92             ro: old_176
  B = 33, within 88                   5.88  1.2e-4    2.30           5.88  1.2e-4             rA: old_87
  MARGIN_SECOND_NEW alone / B = 2     0.20    0.20    1.15           0       0.18
  MARGIN_SECOND_NEW, B = 33           1.47    0.29    2.50           0       0.18
The two kernel sets against each other (alone against B = 33; bound 2 K): LDL^T, k_marg_ldlt<4> against k_marg_ldlt_tp (n <= 88):
rA 1.7e-5, rb 5.8e-7; MARGIN_SECOND_NEW rA 0.14, rb 0.017; n = 177 (the eigen path in both) rA 1.4e-3. Eigen mode: rA 1.4e-3,
rb 2.1e-5; MARGIN_SECOND_NEW rA 12.2 (new_90), rb 0.14. (The LDL^T priors of 89 .. 176 dims and new_90, which both shapes hand to
the same <6> / <8> kernel, came out identical in bits — A' itself agreed in these small windows; nothing promises that, and it is
not asserted.) ro is the quantity with the least room: 15.2 of 32 (old_132 alone, the global-memory QL path).
"""
import numpy as np
import pytest

import normal_equations_np as ne
import prior_np as pn
from _gfbe_import import gf

abi = gf.abi
pytestmark = pytest.mark.gpu
__doc__ = __doc__ % dict(KA=pn.K["rA"], Kb=pn.K["rb"], Ko=pn.K["ro"])

ITERATIONS = 0
OLD = [n for n, c in pn.CASES.items() if c[4] == abi.MARGIN_OLD]
NEW = [n for n, c in pn.CASES.items() if c[4] == abi.MARGIN_SECOND_NEW]
STATE_KEYS = ("pose", "speed_bias", "ex_pose", "ex_pose_wheel", "ix_wheel", "td", "td_wheel", "plane_R", "plane_Z", "gnss_state")


@pytest.fixture(scope="module")
def backends():
    ne.require_extended_precision()
    made = {}

    def get(mode):
        if mode not in made:
            o = abi.default_options()
            o.max_num_iterations, o.marg_sqrt = ITERATIONS, mode
            made[mode] = gf.Backend(device=0, options=o)
        return made[mode]
    yield get
    for b in made.values():
        b.close()


_models, _alone = {}, {}


def model_at(oracle, name, res):
    """The model of case `name` at the state the device marginalised at (cached by that state's bits)."""
    snap, flag = pn.build_case(name, oracle)
    st = res["state"]
    # no iteration ran: the state is the window's up to the re-anchoring's rewrite of the quaternions, the inverse depths are the window's
    want, got = abi.flat_state(abi.state_to_dict(abi.state_from_snapshot(snap))), abi.flat_state(st)
    for k in want:
        a, b = np.array(got[k], float), np.array(want[k], float)
        if k in ("pose", "ex_pose", "ex_pose_wheel"):      # (the rewrite may return -q for q: the same rotation)
            qa, qb = a[..., 3:], b[..., 3:]
            qa *= np.where((qa * qb).sum(axis=-1, keepdims=True) < 0, -1.0, 1.0)
        assert np.allclose(a, b, rtol=1e-14, atol=1e-14), (name, k, float(np.abs(a - b).max()))
    assert np.array_equal(res["feature"], np.asarray(snap["para_feature"], float)), (name, "inverse depths")
    key = (name,) + tuple(np.asarray(v, float).tobytes() for v in abi.flat_state(st).values()) + (res["feature"].tobytes(),)
    if key not in _models:
        at = dict(snap, para_feature=res["feature"].copy(), **{k: st[k] for k in STATE_KEYS})
        _models[key] = pn.reference_prior(oracle, at, flag)
    return _models[key]


def check(oracle, name, mode, res, label, worst):
    ref = model_at(oracle, name, res)
    got = pn.check_prior(res["prior"], ref, mode, "%s %s marg_sqrt %d" % (label, name, mode))
    for q, v in got.items():
        if v >= worst.get(q, (-1.0, ""))[0]:
            worst[q] = (v, name)
    return ref, got


def report_and_assert(label, mode, worst):
    print("%s marg_sqrt %d: " % (label, mode) + "  ".join("%s %.3g (%s)" % (q, v, n) for q, (v, n) in sorted(worst.items())))
    for q, (v, n) in worst.items():
        assert v <= pn.K[q], (label, mode, q, n, v, pn.K[q])


def alone(backends, oracle, name, mode):
    if (name, mode) not in _alone:
        snap, flag = pn.build_case(name, oracle)
        _alone[(name, mode)] = backends(mode).solve(snap, flag)
    return _alone[(name, mode)]


def same_bits(a, b):
    return all(np.array_equal(a["prior"][k], b["prior"][k]) for k in ("J0", "r0", "x0", "block_id", "block_size", "block_idx"))


def batch_of_33(names, seed):
    """33 places: every case at least twice, the rest dealt round-robin, shuffled."""
    order = [names[q % len(names)] for q in range(33)]
    assert all(order.count(n) >= 2 for n in names)
    return [order[q] for q in np.random.default_rng(seed).permutation(33)]


_batches = {}


def run_batch(backends, oracle, mode, flag, names, label):
    """The batch `names` under `flag` (run once per mode): every window against the model, a case that occurs twice bit-identical to
    itself. Returns {case: result of its first place}."""
    if (label, mode) in _batches:
        return _batches[(label, mode)]
    snaps = [pn.build_case(n, oracle)[0] for n in names]
    assert all(pn.build_case(n, oracle)[1] == flag for n in names)
    out = backends(mode).solve_batch(snaps, flag)
    worst, first = {}, {}
    for n, res in zip(names, out):
        check(oracle, n, mode, res, label, worst)
        if n in first:
            assert same_bits(first[n], res), (label, mode, n, "differs between two places of one batch")
        first.setdefault(n, res)
    report_and_assert(label, mode, worst)
    _batches[(label, mode)] = first
    return first


def compare_kernel_sets(backends, oracle, mode, first, label):
    """A case alone (B < 32: the small-batch kernels, k_marg on 1024 threads, k_marg_ldlt<4>) and in a batch of 33 (the throughput
    kernels, 512 threads, k_marg_ldlt_tp): the same state, the same rows kept, J0^T J0 and J0^T r0 within 2 K of each other."""
    apart, bits = dict(rA=(0.0, ""), rb=(0.0, "")), []
    for n, res in first.items():
        one = alone(backends, oracle, n, mode)
        assert np.array_equal(one["state"]["pose"], res["state"]["pose"]) and np.array_equal(one["feature"], res["feature"]), (label, n, "the state differs")
        if same_bits(one, res):
            bits.append(n)
        ref = model_at(oracle, n, res)
        Ja, Jb = np.asarray(one["prior"]["J0"], pn.LD), np.asarray(res["prior"]["J0"], pn.LD)
        ra, rb_ = np.asarray(one["prior"]["r0"], pn.LD), np.asarray(res["prior"]["r0"], pn.LD)
        assert (np.abs(one["prior"]["J0"]).sum(axis=1) > 0).sum() == (np.abs(res["prior"]["J0"]).sum(axis=1) > 0).sum(), (label, mode, n)
        dA = float(np.abs(Ja.T @ Ja - Jb.T @ Jb).max() / (pn.U * ref["a_scale"]))
        db = float(np.abs(Ja.T @ ra - Jb.T @ rb_).max() / (pn.U * max(ref["b_scale"], 1e-2 * ref["a_scale"])))
        apart["rA"], apart["rb"] = max(apart["rA"], (dA, n)), max(apart["rb"], (db, n))
    print("%s marg_sqrt %d, alone against the batch: rA %.3g (%s)  rb %.3g (%s); identical in bits: %s"
          % (label, mode, apart["rA"][0], apart["rA"][1], apart["rb"][0], apart["rb"][1], ", ".join(bits) or "none"))
    assert apart["rA"][0] <= 2 * pn.K["rA"] and apart["rb"][0] <= 2 * pn.K["rb"], (label, mode, apart)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(pn.CASES))
def test_alone(backends, oracle, name, mode):
    res = alone(backends, oracle, name, mode)
    worst = {}
    check(oracle, name, mode, res, "alone", worst)
    report_and_assert("alone " + name, mode, worst)


@pytest.mark.parametrize("mode", [0, 1])
def test_small_batch_is_bit_identical_to_alone(backends, oracle, mode):
    """B = 13 < 32: the kernel set of a single window; k_marg_ldlt<4>, <6> and <8> launched into one batch, each leaving the other
    kinds' windows alone."""
    order = [OLD[q] for q in np.random.default_rng(4).permutation(len(OLD))]
    first = run_batch(backends, oracle, mode, abi.MARGIN_OLD, order, "B = 13")
    for n, res in first.items():
        assert same_bits(alone(backends, oracle, n, mode), res), (mode, n, "alone and in a batch of 13 differ in bits")
    both = run_batch(backends, oracle, mode, abi.MARGIN_SECOND_NEW, NEW, "B = 2, MARGIN_SECOND_NEW")
    for n, res in both.items():
        assert same_bits(alone(backends, oracle, n, mode), res), (mode, n, "alone and in a batch of 2 differ in bits")


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_of_33_with_every_size(backends, oracle, mode):
    first = run_batch(backends, oracle, mode, abi.MARGIN_OLD, batch_of_33(OLD, 1), "B = 33, every size")
    compare_kernel_sets(backends, oracle, mode, first, "B = 33, every size")


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_of_33_within_88_dims(backends, oracle, mode):
    """marg_nmax <= 88: k_marg_ldlt<6> and <8> are not launched, k_marg_ldlt_tp is the only LDL^T kernel of the batch. marg_nmax is the
    batch maximum of the HOST's bound per window — the larger of the incoming prior's n and the MARGIN_OLD bound —, not of n_out.
    Inside the throughput kernel set a window does not depend on its batch: bit-identical to the same case in the batch with every
    size (where <6> and <8> are launched and must leave these windows alone)."""
    assert max(pn.host_marg_bound(pn.build_case(n, oracle)[0]) for n in pn.WITHIN_88) <= 88
    assert max(pn.host_marg_bound(pn.build_case(n, oracle)[0]) for n in OLD) > 132
    first = run_batch(backends, oracle, mode, abi.MARGIN_OLD, batch_of_33(pn.WITHIN_88, 2), "B = 33, within 88")
    compare_kernel_sets(backends, oracle, mode, first, "B = 33, within 88")
    every = run_batch(backends, oracle, mode, abi.MARGIN_OLD, batch_of_33(OLD, 1), "B = 33, every size")
    for n, res in first.items():
        assert same_bits(every[n], res), (mode, n, "differs between two batches of 33")


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_of_33_second_new(backends, oracle, mode):
    first = run_batch(backends, oracle, mode, abi.MARGIN_SECOND_NEW, batch_of_33(NEW, 3), "B = 33, MARGIN_SECOND_NEW")
    compare_kernel_sets(backends, oracle, mode, first, "B = 33, MARGIN_SECOND_NEW")
