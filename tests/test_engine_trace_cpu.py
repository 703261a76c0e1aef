"""The launch sequence of Engine.network and Engine.transformer against the one recorded from the parent of the engine's per-forward
context (tests/golden/engine_trace_parent.json, written by `tools/engine_trace.py --record` on that revision): every library call with its
label, its scalar arguments and the data flow between its buffers, for 57 configurations of model, precision, batch and switches.  The
library is a recording stub (tools/engine_trace.py): no device is needed.  A routing change that is meant re-records the file with the tool
on the revision BEFORE a refactor, never from the code under test; `python tools/engine_trace.py --dump KEY` prints one configuration in full."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def golden():
    import engine_trace as et
    with open(et.GOLDEN) as f:
        return json.load(f)


def test_launch_trace_equals_the_recorded_parent(golden, monkeypatch):
    import engine_trace as et
    from omnifusion_amd.model._engine import Engine
    configs = et.configurations()
    assert set(configs) == set(golden["digests"]) and len(configs) == 57
    assert set(golden["anchors"]) == set(et.ANCHORS)
    tracer = et.Tracer(monkeypatch.setattr)
    bad = []
    for key, cfg in configs.items():
        lines = tracer.run(cfg)
        if et.digest(lines) == golden["digests"][key]:
            continue
        bad.append(key)
        if key in golden["anchors"]:
            want = [golden["calls"][i] for i in golden["anchors"][key]]
            k = next((i for i, (a, b) in enumerate(zip(lines, want)) if a != b), min(len(lines), len(want)))
            print(f"{key}: {len(lines)} calls, recorded {len(want)}; first difference at call {k}:\n  now      {lines[k] if k < len(lines) else '(none)'}"
                  f"\n  recorded {want[k] if k < len(want) else '(none)'}")
    assert not bad, f"the launch trace moved in {len(bad)} of {len(configs)} configurations (from {golden['recorded_from']}): {bad}"
    assert all(getattr(Engine, k) == v for k, v in et.DEFAULTS.items())                  # every switch is back at its default


def test_anchor_lists_match_their_digests(golden):
    """the file is consistent with itself: an anchor's full call list hashes to its digest"""
    import engine_trace as et
    for key, idx in golden["anchors"].items():
        assert et.digest([golden["calls"][i] for i in idx]) == golden["digests"][key], key
