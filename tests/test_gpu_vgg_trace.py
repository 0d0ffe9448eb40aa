"""VggEngine's launch trace against the recorded one (tests/golden/vgg_launch_trace.json, made with tests/launch_trace.py on the commit
before the per-shape plan of vgg_plan.conv_plan): every library launch of one forward + backward keeps its entry, its scalar
arguments, its stream and its place among the stream waits and event records."""
import json
import os

import pytest

from . import launch_trace

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vgg_launch_trace.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(launch_trace.CASES))
def test_launch_trace_equals_the_recorded_one(lib, golden, monkeypatch, case):
    got = json.loads(json.dumps(launch_trace.trace_case(lib, case, monkeypatch.setenv)))   # (tuples -> lists, as stored)
    want = golden[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (case, i, got[max(i - 2, 0):i + 1], want[max(i - 2, 0):i + 1])
    assert len(got) == len(want), (case, len(got), len(want))
