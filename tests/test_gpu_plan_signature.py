"""The native plan's launch grouping, kernel choice and workspace placement against tests/golden/plan_signature.json
(tests/golden/make_plan_signature.py): host-side refactors of plan.hip must leave all three exactly as they are."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def _load(golden_dir):
    sys.path.insert(0, golden_dir)
    try:
        import make_plan_signature as mps
    finally:
        sys.path.remove(golden_dir)
    with open(os.path.join(golden_dir, "plan_signature.json")) as f:
        return mps, json.load(f)


def test_plan_signature_is_unchanged(golden_dir):
    mps, want = _load(golden_dir)
    assert sorted(want) == sorted(mps.config_key(name, env) for name, env in mps.CONFIGS)
    for name, env in mps.CONFIGS:
        key = mps.config_key(name, env)
        got = mps.signature(name, env)
        for part in ("ws", "tensors", "ops"):
            assert got[part] == want[key][part], f"{key}: {part} differs from the pinned plan"
