"""The C ABI layer refuses what it refused when tests/golden/capi_refusals.json was recorded: every single-fault case of
tests/capi_refusal_cases.py comes back with the recorded code, and the pure host queries with the recorded values.

CPU only.  After a deliberate change of a refusal: `python tests/capi_refusal_cases.py --record` on a machine without a
GPU, and the diff of the JSON goes into the review with the change."""
import json

import pytest
import torch

pytestmark = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="replayed on machines without a GPU only: the cases hand the library HOST pointers, and a refusal that had "
           "regressed would launch a kernel on them -- never on a shared card")


@pytest.fixture(scope="module")
def table():
    import capi_refusal_cases as cases
    with open(cases.GOLDEN) as f:
        return cases, json.load(f)


def test_every_entry_point_has_a_case(table):
    cases, golden = table
    missing, unknown = cases.coverage_gaps()
    assert not missing, f"entry points without a recipe: {missing}"
    assert not unknown, f"recipes for names miso_hip.h does not declare: {unknown}"
    per_entry = {k.split(":")[0].split("/")[0] for k in golden}
    from miso_amd import _lib
    assert per_entry == set(_lib.SIGNATURES) and len(per_entry) == 88
    assert set(cases.cases()) == set(golden), "the cases and the recording name different cases: record again"


def test_cases_of_launching_entry_points_are_recorded_refusals(table):
    cases, golden = table
    bad = {k: v for k, v in golden.items() if cases.launching(k) and v not in cases.REFUSALS}
    assert not bad, f"recorded as something other than a refusal: {bad}"


def test_refusals_and_host_values_are_as_recorded(table):
    cases, golden = table
    from miso_amd import _lib
    lib = _lib.load()
    diff = {}
    for key, thunk in cases.cases().items():
        want = golden[key]
        if cases.launching(key):
            assert want in cases.REFUSALS, key         # (checked above: nothing below can reach a launcher by the record)
        got = thunk(lib)
        if got != want:
            diff[key] = (want, got)
            if cases.launching(key) and got not in cases.REFUSALS:
                break                                   # no longer a refusal: stop before anything else is tried
    assert not diff, "recorded -> now: " + "; ".join(f"{k}: {w} -> {g}" for k, (w, g) in sorted(diff.items()))
