"""Source-level invariants of the product's host / device headers that no runtime test on a CPU box can see (no GPU here).

Speculative linearisation keeps a SECOND set of the linearisation's outputs: BatchDev::lin2, a LinSet like the batch's own
(csrc/gfbe_device.h). That every member of it is carved from the slab and swapped by lin_view is checked by RUNNING carve_slab and
lin_view (tests/test_upload_host.py); what stays here is that no hand-kept `<member>2` twin of a LinSet member comes back.
"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ground-fusion2_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _lin_set_members():
    dev = _read("gfbe_device.h")
    body = dev[dev.index("struct LinSet {"):]
    body = re.sub(r"//[^\n]*", "", body[:body.index("\n};")])
    return sorted(set(re.findall(r"\*\s*([A-Za-z_][A-Za-z_0-9]*)\b", body)))


def test_no_second_set_member_is_kept_by_hand():
    members = _lin_set_members()
    assert len(members) >= 16 and "lm_hP" in members and "gnss_cost" in members and "schur_part" in members, members
    for name in ("gfbe_device.h", "gfbe_host.cpp"):
        text = re.sub(r"//[^\n]*", "", _read(name))
        for m in members:
            assert not re.search(r"(?<![A-Za-z_0-9\"])%s2\b" % m, text), "%s declares or assigns %s2" % (name, m)


def test_options_default_and_binding_agree_on_the_speculative_pass():
    host = _read("gfbe_host.cpp")
    assert re.search(r"speculative_linearization\s*=\s*1\s*;", host)
    from importlib import import_module
    abi = import_module("ground-fusion2_amd.abi")
    assert abi.default_options().speculative_linearization == 1
