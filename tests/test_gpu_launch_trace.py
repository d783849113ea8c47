"""The train path issues exactly the native launches it issued when
tests/golden/launch_traces.json was recorded: same launchers, same order,
same shapes, same integers (tests/_launch_trace.py; the file is written by
scripts/record_launch_trace.py).  A refactor of the host layer must leave
every scenario's trace equal element for element."""
import pytest

from tests import _launch_trace as LT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return LT.load_golden()


def test_golden_covers_every_scenario(golden):
    assert sorted(golden) == sorted(LT.SCENARIOS)
    for name, need in LT.REQUIRED.items():
        issued = {rec[0] for rec in golden[name]}
        assert not [n for n in need if n not in issued], name


@pytest.mark.parametrize("name", list(LT.SCENARIOS))
def test_launch_trace_matches_golden(name, golden):
    import json
    got = json.loads(json.dumps(LT.run_scenario(name)))  # tuples -> lists, as the file holds them
    want = golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: launch {i} differs\n  now:    {g}\n  golden: {w}"
    assert len(got) == len(want), (name, len(got), len(want))
