"""CPU checks of the extended-precision reference of the normal equations (tests/normal_equations_np.py) and of the windows the GPU
comparison runs on (tests/test_gpu_normal_equations.py): the windows have the prescribed landmark layout and the oracle takes them;
the oracle's plain FP64 linearisation is within the measured K_MEASURED u A of the reference, entry by entry — the measurement the
GPU bound K is derived from, asserted so that it cannot drift —; the Schur term contracts to dist.reduced_system's; the structural
zeros are where the constant blocks are."""
import numpy as np
import pytest

import normal_equations_np as ne
from _gfbe_import import gf

abi, synth, dist = gf.abi, gf.synth, gf.dist


@pytest.fixture(autouse=True)
def _extended_precision():
    ne.require_extended_precision()


def test_bound_constants_follow_from_the_measurement():
    top = ne.K_MARGIN * max(ne.K_MEASURED.values())
    assert ne.K == 2.0 ** np.ceil(np.log2(top)) and ne.K_MARGIN == 8.0


def test_factor_rows_of_any_length_equal_the_bookkeeping_for_long_tracks():
    fl = synth.Scenario(seed=38, n_landmarks=60).feature_list(0)
    fl["estimate_flag"][::7] = 1
    want, got = synth.build_visual_factors_np(fl), ne.visual_factors_any_length(fl)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("name", ne.case_names())
def test_case_window_has_the_prescribed_layout(oracle, name):
    snap = ne.build_case(name, oracle)
    counts = ne.layout_counts(snap)
    L, fc = len(snap["para_feature"]), snap["frame_count"]
    assert sum(counts.values()) == L
    if name in ne.CASE_PER_START:
        want = ne.case_counts(name)
        assert counts == want and ne.per_start_frame(counts) == ne.CASE_PER_START[name]
    if name == "tile_edges":      # the longest possible track in every occupied start frame, two- and one-factor tracks in start frames 8 and 9
        assert all((s, 10 - s) in counts for s in (0, 1, 2, 3, 5, 6, 8, 9)) and counts[(8, 2)] == counts[(8, 1)] == counts[(9, 1)] == 1
    if name == "chunk_edges":
        assert sorted(ne.per_start_frame(counts))[-3:] == [256, 257, 513]
    if name == "short_tracks":
        assert set(m for _, m in counts) == {1} and set(s for s, _ in counts) == set(range(10))
    if name == "no_landmarks":
        assert L == 0 and len(snap["vis_imu_i"]) == 0
    if name == "idle_landmarks":
        m = np.bincount(snap["vis_feature_index"], minlength=L)
        assert (m[4::5] == 0).all() and (np.delete(m, np.arange(4, L, 5)) > 0).all() and snap["feature_const"].tolist() == [int(l % 3 == 0) for l in range(L)]
        assert ne.idle_landmarks(snap).sum() == len(set(range(0, L, 3)) | set(range(4, L, 5)))
    if name == "full_columns":
        assert snap["ex_cam_const"] == 0 and snap["td_const"] == 0 and np.abs(snap["td"] - snap["vis_td_j"]).min() > 0
    if name == "robust":          # on the reference: the Huber corrector is active on a few per cent of the factors, not on none and not on most
        r = oracle.eval_factors(snap, robustify=False)["vis_r"]
        past = (np.sqrt((r * r).sum(axis=1)) > abi.default_options().huber_delta).mean()
        assert 0.02 < past < 0.20, past
    if name in ("partial", "soak_349"):
        assert fc < abi.WINDOW_SIZE and snap["vis_imu_j"].max() <= fc and len(snap["imu_frame"]) == fc
    if name == "prior_wheel_2k":
        assert L == 2000 and snap["prior"] is not None and "wheel" in snap
    if name == "soak_349":
        assert L == 3500 and len(snap["lio"]["pts"]) > 0 and snap["feature_const"].sum() == 1167 and counts.get((0, 0), 0) > 0
    lin = oracle.linearize(snap)                       # the oracle accepts the window
    assert np.isfinite(lin["H"]).all() and np.isfinite(lin["Hpl"]).all() and lin["cost"] > 0


@pytest.mark.parametrize("name", ne.case_names())
def test_fp64_linearisation_is_within_the_measured_ratio(oracle, name):
    """|X_fp64 - X_ref| <= K_MEASURED[X] u A_X for every entry of every array (the measurement of K); structural zeros exact."""
    snap, ev, ref = ne.case_reference(name, oracle)
    got = ne.fp64_system(oracle, snap)
    for key in ("H", "g", "Hll", "gl", "Hpl", "E", "eg"):
        ratio, where, n0, first0 = ne.worst_ratio(key, got[key], ref[key], ref["A_" + key])
        print("%s %s: %.2f u A" % (name, key, ratio))
        assert n0 == 0, first0
        assert ratio <= ne.K_MEASURED[key], where


@pytest.mark.parametrize("name", ne.case_names())
def test_schur_term_contracts_to_the_reduced_system(oracle, name):
    """With s_l = 1 and no clamp, H[:73, :73] - E and g[:73] - eg are dist.reduced_system(lin, mu): an independent statement of the
    same contraction (FP64 rounding: K_MEASURED of E on the reference's own scales)."""
    snap, ev, ref = ne.case_reference(name, oracle)
    mu = 0.125
    E, eg, A_E, A_eg = ne.schur_reference(ref["Hll"], ref["gl"], ref["Hpl"], mu, False, ref["idle"], ref["A_Hpl"], ref["A_gl"], clamp=False)
    lin = oracle.linearize(snap)
    packed = dist.reduced_system(lin, mu)
    S, gs = packed[:ne.ND * ne.ND].reshape(ne.ND, ne.ND), packed[ne.ND * ne.ND:ne.ND * ne.ND + ne.ND]
    k = max(ne.K_MEASURED.values())
    dS = np.abs(np.asarray(ref["H"][:73, :73] - E, float) - S[:73, :73])
    dg = np.abs(np.asarray(ref["g"][:73] - eg, float) - gs[:73])
    assert (dS <= k * ne.U * np.asarray(ref["A_H"][:73, :73] + A_E, float)).all()
    assert (dg <= k * ne.U * np.asarray(ref["A_g"][:73] + A_eg, float)).all()
    if len(snap["para_feature"]):
        assert np.abs(np.asarray(E, float)).max() > 0


def test_structural_zeros_are_the_constant_blocks(oracle):
    """The reference removes what test_oracle_solver.py::test_constant_blocks_are_removed sees removed in the oracle — and nothing else."""
    scn = synth.Scenario(seed=32, n_landmarks=30, use_wheel=True)
    snap = scn.window(0)
    ref = ne.reference_system(snap, oracle.eval_factors(snap, robustify=True))
    lin = oracle.linearize(snap)
    gone = list(range(ne.T_EX, ne.T_EX + 6)) + [ne.T_TD, ne.T_SX, ne.T_SY, ne.T_SW, ne.T_TDW] + list(range(182, ne.ND))
    assert sorted(np.where(~ref["act"])[0].tolist()) == gone
    for a in gone:
        assert not ref["A_H"][a].any() and not ref["A_H"][:, a].any() and ref["A_g"][a] == 0 and not ref["H"][a].any() and ref["g"][a] == 0
    assert not ref["A_Hpl"][:, ne.T_EX:ne.T_EX + 7].any() and not ref["A_E"][ne.T_EX:ne.T_EX + 7].any() and not ref["A_eg"][ne.T_EX:ne.T_EX + 7].any()
    assert ((np.asarray(ref["A_H"], float) == 0) == (lin["H"] == 0)).all() and ((np.asarray(ref["A_Hpl"], float) == 0) == (lin["Hpl"] == 0)).all()
    for name in ("partial", "no_landmarks", "full_columns"):
        snap, ev, ref = ne.case_reference(name, oracle)
        lin = oracle.linearize(snap)
        assert ((np.asarray(ref["A_H"], float) == 0) == (lin["H"] == 0)).all(), name
        assert (ref["act"][:ne.DIMS_IN_USE] == (np.diag(lin["H"])[:ne.DIMS_IN_USE] != 0)).all(), name
    assert not ne.case_reference("no_landmarks", oracle)[2]["A_E"].any()
    assert ne.case_reference("full_columns", oracle)[2]["A_E"][ne.T_TD, ne.T_EX] > 0
