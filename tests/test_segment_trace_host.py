"""The residual-block walk of ``RingSegment`` / ``RingSegmentH`` makes exactly the wrapper calls, with the same operands in the same
order, that the two hand-written walks made before they became one: record for record against tests/golden/segment_traces.json, which
tests/segment_trace.py wrote at that earlier commit (never regenerate it from the code under test).  Host logic, no GPU, no library:
the kernels and the C dispatch being deterministic, identical calls on identical operands in identical order give identical bits."""
import json
import os

import pytest

from tests import segment_trace

CASES = segment_trace.cases()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "segment_traces.json")) as f:
        return json.load(f)


def test_golden_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)
    assert len(CASES) >= 24 + 5


@pytest.mark.parametrize("cid", sorted(CASES))
def test_segment_makes_the_recorded_calls(golden, cid):
    want = golden[cid]
    got = json.loads(json.dumps(segment_trace.record(**CASES[cid])))
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f"{cid}: first differing record, number {i}\n  recorded then: {json.dumps(w)}\n  made now:      {json.dumps(g)}")
        assert g == w, f"record {i} of {cid} differs"
    longer = got if len(got) > len(want) else want
    assert len(got) == len(want), f"{cid}: {len(got)} records now, {len(want)} then; first unmatched: {json.dumps(longer[min(len(got), len(want))])}"
