"""What the three circuit layouts of synthesis.py decide -- regions, fixed columns, copies -- and the advice columns they assign for
seeded inputs, against sha256 digests recorded before the layouts were rebuilt on one Pow5 base (tests/golden/layout_digests.json,
written by tests/golden/gen_golden.py: layout_vectors).  The other witness tests compare the kernels' code with assign_ints; this
one pins assign_ints and the layouts themselves."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_layouts_reproduce_the_recorded_digests():
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "golden", "gen_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(HERE, "golden", "layout_digests.json")) as f:
        recorded = json.load(f)
    got = gen.layout_digests()
    assert sorted(got) == sorted(recorded) and len(got) == 10
    assert {name: d for name, d in got.items() if d != recorded[name]} == {}
