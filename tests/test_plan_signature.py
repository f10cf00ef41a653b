"""Guard on the host-side plan builders: every description of tools/plan_signature.py is built host-only (no GPU) and its
integer signature -- path, tiles, workspace_bytes, kernel and exchange counts, exchange sizes, the names and lengths of its
tables, which dimensions take the neighbour form -- is compared with tests/golden/plan_signature.json.  A change that moves
one of these on purpose regenerates the file: python tools/plan_signature.py --golden > tests/golden/plan_signature.json"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import plan_signature as ps     # noqa: E402

with open(os.path.join(HERE, "golden", "plan_signature.json")) as f:
    GOLDEN = json.load(f)


def test_the_golden_file_covers_the_case_list():
    assert sorted(GOLDEN) == sorted(name for name, _ in ps.CASES)
    assert len(GOLDEN) >= 320


@pytest.mark.parametrize("name,kw", ps.CASES, ids=[name for name, _ in ps.CASES])
def test_plan_signature(name, kw):
    got = json.loads(json.dumps(ps.golden_record(kw)))     # (tuples -> lists, as the file holds them)
    assert got == GOLDEN[name]
