"""Which form of k_schur the solve pass of a batch takes (schur_lean_form, csrc/gfbe_device.h; launch_schur asks it): the lean form
addresses a landmark's rows as [row base + 32-bit BYTE offset of its slot], so it needs 8 tot_lm < 2^32 on top of what chose it before
(a throughput batch, SCHUR_GROUPS groups, with constant extrinsic and td). Evaluated without a GPU and without allocating anything:
tests/schur_form_shim.cpp, built and loaded the way tests/test_upload_host.py builds the upload's host half, and on the plans of real
(small) batches through that file's shim."""
import ctypes as C
import os

import pytest

import test_upload_host as uh
from test_upload_host import shim      # noqa: F401  (the fixture that builds the upload's host half)

LIMIT = 2 ** 32 // 8        # slots: the first tot_lm whose last byte offset does not fit


@pytest.fixture(scope="module")
def form():
    lib = C.CDLL(uh._build(os.path.join(uh.ROOT, "tests", "schur_form_shim.cpp"), os.path.join(uh.BUILD, "libschur_form_shim.so"), ["-fPIC", "-shared"]))
    lib.sf_lean.argtypes = [C.c_int, C.c_int, C.c_longlong]
    lib.sf_lean_of_plan.argtypes = [C.c_int] * 4
    return lib


def test_byte_offset_bound(form):
    g = form.sf_groups()
    assert g == 4
    # a landmark slot is 64-aligned: the largest batch below the bound and the first one at it
    assert form.sf_lean(g, 0, LIMIT - 64) == 1 and form.sf_lean(g, 0, LIMIT - 1) == 1
    assert form.sf_lean(g, 0, LIMIT) == 0 and form.sf_lean(g, 0, LIMIT + 64) == 0 and form.sf_lean(g, 0, 2 ** 31 - 64) == 0
    assert form.sf_lean(g, 0, 0) == 1 and form.sf_lean(g, 0, 64) == 1
    # the conditions from before: the number of groups and the constant extrinsic / td
    for tot in (64, LIMIT - 64):
        assert form.sf_lean(g, 1, tot) == 0 and form.sf_lean(11, 0, tot) == 0 and form.sf_lean(22, 0, tot) == 0


def test_as_a_plan_leaves_it_in_the_batch(form):
    """Through plan_to_batch: the members launch_schur reads (BatchDev::tot_lm is an int, the bound lies inside its range)."""
    assert form.sf_lean_of_plan(32, 0, 0, LIMIT - 64) == 1 and form.sf_lean_of_plan(32, 0, 0, LIMIT) == 0
    assert form.sf_lean_of_plan(8192, 0, 0, LIMIT - 64) == 1 and form.sf_lean_of_plan(8192, 0, 0, LIMIT) == 0
    assert form.sf_lean_of_plan(31, 0, 0, 64) == 0 and form.sf_lean_of_plan(31, 1, 0, 64) == 0       # small batches: 22 / 11 groups
    assert form.sf_lean_of_plan(32, 1, 0, 64) == 1                                                   # (sharded throughput batches had the lean form before)
    assert form.sf_lean_of_plan(32, 0, 1, 64) == 0


def test_real_plans(form, shim):
    for snaps, want in ((uh._many(33), 1), (uh._many(33, ex_cam_const=0), 0), ([uh.CASES["no_prior"]], 0)):
        p = uh.Packed(shim, snaps)
        try:
            assert p.status == uh.abi.OK, p.err
            assert form.sf_lean(p.info["schur_groups"], p.info["vis_full"], p.info["tot_lm"]) == want
        finally:
            p.close()
