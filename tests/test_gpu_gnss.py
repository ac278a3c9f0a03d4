"""The GNSS factors on the device (csrc/gfbe_gnss.hip: gfbe_gnss_eval) against the extended-precision model of the operation it
performs (tests/gnss_np.py), entry by entry, through the C ABI:

    |r_dev - r| <= K_R u A_r      |J_dev - J| <= K_J u A_J      |r_clk_dev - r_clk| <= K_CLK u A_clk      (u = 2^-53)

with the absolute sums A of that module (the weights' conditioning on the elevation, 1 + 2 |cot el|, is in the scale), exactly 0.0
where A is zero (the pseudo-range row at the velocities and the clock drift, the Doppler row at the clock bias and the anchor, the
columns of a pose whose interpolation weight is exactly 0), and the cost against the model's longdouble sum on the scale sum r^2 / 2
with the first-order allowance sum |r| K_R u A_r. K_R = %(K_R)g, K_J = %(K_J)g, K_CLK = %(K_CLK)g are 8 x what plain FP64 implementations measure on the
CPU (tests/test_gnss_reference.py; nothing is derived from the device), and the same comparison runs on the oracle. These bounds
replace |dr| < 1e-5, |dJ| < 1e-9 max |J|, 1e-9 and 1e-12 on the clock residuals: K_R u A_r is 1e-6 at most (a pseudo-range of
2.5e7 m, weight 5), K_J u A_J 1e-11, K_CLK u A_clk 1e-12 and less. The device-against-oracle cost check (1e-9 relative) stays.

Cases (gnss_np.MODEL_CASES): latitudes 4, 22.3, 40, 52, 68, 80 degrees (every interval of the Niell table and outside both ends; phi
clamps at 0.416 at 80) and -33.9 (the half-year shift), heights -20 m and 900 m, elevations 8 .. 88 degrees and one satellite below
the horizon, day and night Klobuchar and iono = None, ratio exactly 0 and exactly 1, all four constellations, 1 / 63 / 64 / 65 / 127 /
128 / 129 observations (the edges of the 128-thread grid with the 50 clock threads behind them); and the cases this file had before
(gnss_np.PLAIN_CASES: 88, 33, 440 observations; the horizon and clock-only edge cases). Every observation of every case is compared:
that each keeps its distance from every branch of the arithmetic is asserted on the CPU, not filtered here.

Measured on an MI355X (worst |X_dev - X| / (u A_X) over all cases and both ionosphere settings):
%(MEASURED)s
"""
import numpy as np
import pytest

from _gfbe_import import gf
import gnss_cases as gc
import gnss_np as gn

abi = gf.abi
pytestmark = pytest.mark.gpu

MEASURED = """                 r      J    clock residuals    cost (in u sum r^2 / 2, inside the allowance)
  device      2.41   4.28      0.593             4.7e5        worst case r: plain_23   J: lat80_n128   cost: plain_22
  oracle      2.41   5.47      0.593             4.6e5
The device is where a plain FP64 loop on the CPU is: an eighth of each bound is used. The cost's 4.7e5 u (5e-11 relative) is the
residuals' own rounding, 1e-9 of a residual of 10 that is the difference of numbers of 2.5e7, which the allowance states."""
__doc__ = __doc__ % dict(K_R=gn.K_R, K_J=gn.K_J, K_CLK=gn.K_CLK, MEASURED=MEASURED)


@pytest.fixture(scope="module")
def be():
    gn.require_extended_precision()
    return gf.Backend(device=0)


def check_case(be, oracle, name, iono):
    """Device and oracle against the model on every entry; device against oracle on the cost, as before. Returns the device's output."""
    c, ref = gn.gnss_model_cases()[name], gn.case_reference(name, iono)
    a = gc.eval_case(abi, oracle.lib, "gfo_", None, c, iono=iono)
    b = gc.eval_case(abi, be.lib, "gfbe_", be.ctx, c, iono=iono)
    fails = []
    for label, got in (("oracle", a), ("device", b)):
        ratios, f = gn.compare(got, ref, "%s %s %s:" % (name, "iono" if iono else "no iono", label))
        print("%-20s %-5s %-7s " % (name, "iono" if iono else "none", label) + "  ".join("%s %.3g" % kv for kv in ratios.items()))
        fails += f
    assert not fails, "\n".join(fails)
    assert abs(a["cost"] - b["cost"]) < 1e-9 * a["cost"]
    return b


@pytest.mark.parametrize("name", list(gn.MODEL_CASES))
def test_gnss_factors_match_the_model(be, oracle, name):
    for iono in ("case", None):
        check_case(be, oracle, name, iono)


@pytest.mark.parametrize("seed,lat,lon,h,n_per_frame", [(21, 22.3, 114.17, 30.0, 8), (22, -33.9, 151.2, 900.0, 3), (23, 68.0, -20.0, 5.0, 40)])
def test_gnss_factors_match_oracle(be, oracle, seed, lat, lon, h, n_per_frame):
    name = "plain_%d" % seed
    assert gn.PLAIN_CASES[name] == (seed, n_per_frame, lat, lon, h)
    for iono in ("case", None):
        check_case(be, oracle, name, iono)
    c = gn.gnss_model_cases()[name]
    again = gc.eval_case(abi, be.lib, "gfbe_", be.ctx, c)
    first = gc.eval_case(abi, be.lib, "gfbe_", be.ctx, c)
    assert again["cost"] == first["cost"] and np.array_equal(again["J"], first["J"])        # deterministic
    assert np.array_equal(again["r"], first["r"]) and np.array_equal(again["r_dt_ddt"], first["r_dt_ddt"]) and np.array_equal(again["r_smooth"], first["r_smooth"])


def test_gnss_edge_cases(be, oracle):
    # no observations: the clock chain alone
    empty = gn.gnss_model_cases()["edge_24_clock_only"]
    b = check_case(be, oracle, "edge_24_clock_only", "case")
    a = gc.eval_case(abi, oracle.lib, "gfo_", None, empty)
    assert b["r"].shape == (0, 2) and abs(a["cost"] - b["cost"]) < 1e-12 * a["cost"] and a["cost"] > 0
    # a satellite below the horizon: no atmosphere terms, finite residuals, inside the model's bounds like any other
    c = gn.gnss_model_cases()["edge_24"]
    b = check_case(be, oracle, "edge_24", "case")
    assert np.isfinite(b["r"]).all() and np.array_equal(b["r"][0], check_case(be, oracle, "edge_24", None)["r"][0])
    # indices out of range are refused before anything is launched
    bad = dict(c, obs=[dict(c["obs"][0], lower_idx=10)])
    with pytest.raises(RuntimeError):
        gc.eval_case(abi, be.lib, "gfbe_", be.ctx, bad)
    bad = dict(c, obs=[dict(c["obs"][0], pr_uura=0.0)])
    with pytest.raises(RuntimeError):
        gc.eval_case(abi, be.lib, "gfbe_", be.ctx, bad)
