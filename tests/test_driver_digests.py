"""The Python rollout drivers against what they computed, and the host work they did, at the commit tools/gen_driver_digests.py was last run at
(tests/golden/driver_digests.json): every output and gradient bit, the same entry points in the same order, and no more aten operators or
synchronising calls on a warm call."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("gen_driver_digests", os.path.join(ROOT, "tools", "gen_driver_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "driver_digests.json")) as f:
    FIXTURE = json.load(f)


@pytest.fixture
def exact_chains():
    with gen.exact_chains():
        yield


def test_the_fixture_holds_exactly_the_generators_cases():
    assert sorted(FIXTURE["cases"]) == sorted(gen.CASES)


@pytest.mark.parametrize("cid", list(gen.CASES))
def test_driver_bits_and_work_are_the_recorded_ones(exact_chains, cid):
    case, want = gen.CASES[cid], FIXTURE["cases"][cid]
    got = gen.run_case(case)
    print(cid, {k: v for k, v in got.items() if k in ("non_view_ops", "sync_warnings")}, "recorded",
          {k: v for k, v in want.items() if k in ("non_view_ops", "sync_warnings")})
    assert set(got) == set(want)
    for key in want:
        if key in ("non_view_ops", "sync_warnings"):
            assert got[key] <= want[key], (key, got[key], want[key])
        else:
            assert got[key] == want[key], key
    if case.get("too_long"):      # the plain-call fallback of a ragged column: the bits of the call with the attribute off
        twin = FIXTURE["cases"][gen.plain_twin(case)]
        assert (got["state_seqs"], got["action_seqs"]) == (twin["state_seqs"], twin["action_seqs"])
