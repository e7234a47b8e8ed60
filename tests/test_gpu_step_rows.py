"""atm_srk3 makes the launches, and the option calls give the answers, that were recorded from the
driver before its refactor into step form / run state / stage functions.

tests/golden/srk3_rows_x1.2562.json was written by tools/record_step_rows.py on the parent build: per
configuration the timing rows (key, calls) of four consecutive steps -- a full step, generations 1 and 2
and a second kept step -- at L = 5 and L = 56, and per option name the return codes, error texts and
values of set_option / get_option over a fixed list of values.  The same two functions run here and
must give the same data.  (Rows and counts do not pin the order of launches within a step: the
bit-identity suites do.)"""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import record_step_rows as R  # noqa: E402

pytestmark = pytest.mark.gpu

with open(R.FIXTURE) as _f:
    FX = json.load(_f)


def test_fixture_covers_the_matrix():
    assert sorted(FX["configs"]) == sorted(R.CONFIGS)
    assert FX["option_names"] == R.OPTION_NAMES and sorted(FX["options"]) == sorted(R.OPTION_NAMES)
    assert FX["values"] == list(R.VALUES) and FX["steps"] == R.STEPS


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_step_rows(name):
    want = R.unpack_steps(FX, name)
    got = R.step_rows(R.CONFIGS[name])
    if isinstance(want, dict) or isinstance(got, dict):
        assert got == want
        return
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"step {i}: rows differ\n got  {g}\n want {w}"
    assert len(got) == len(want)


@pytest.mark.parametrize("name", R.OPTION_NAMES)
def test_option_surface(name):
    got = R.option_rows(name)
    want = FX["options"][name]
    for g, w in zip(got, want):
        assert g == w, f"{name} = {w[0]}: [value, set rc, set error, get rc, got] {g}, recorded {w}"
    assert len(got) == len(want)
