"""The grouped BatchNorm entry points of csrc/rows.hip leave the bits they left before their partial-sum kernels became one templated
body: SHA-256 digests of the raw outputs on fixed inputs (profiles/bn_parent_bits.py), recorded on the commit before that change in
tests/bn_parent_bits.json.  A changed order of additions moves a digest; the entry-point-against-entry-point tests cannot see one."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_outputs_have_the_recorded_digests():
    spec = importlib.util.spec_from_file_location("bn_parent_bits", os.path.join(ROOT, "profiles", "bn_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "tests", "bn_parent_bits.json")) as f:
        recorded = json.load(f)
    assert recorded["seed"] == mod.SEED
    got = mod.digests()
    assert set(got) == set(recorded["digests"]) and len(got) == 12 * 8 + 6
    differ = sorted(k for k in got if got[k] != recorded["digests"][k])
    assert not differ, differ
