"""Guard on which instance of the final pass of the fused path runs (recfilter_amd/csrc/pass2_select.h).

Every instance of fused_pass2_kernel / fused_pass2_tall_kernel computes the same pixels, so no parity, footprint or golden test sees
a wrong pick; only a timing would.  tests/cpp/pass2_choice_table.cpp -- a host program, no HIP -- prints select_pass2 over a fixed
lattice of queries, and tests/golden/pass2_choices.json holds the row count of that table, its SHA-256 and, per distinct instance,
the number of rows that reach it (so a mismatch names the instances that gained or lost rows).  The table was recorded when it
equalled, line for line, the table of the launchers that had the rule in their RF_CASE ladders.  A change that moves a choice on
purpose regenerates the file from the program's two outputs.

The instance list the launchers walk (kPass2Instances under its guard pass2_has) is checked against
the table both ways: every chosen instance is listed, and every listed instance is reached by a row or matches one of the file's
"unreachable" patterns, each with its reason."""
import hashlib
import json
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "pass2_choices.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pass2") / "pass2_choice_table")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-Werror", "-x", "c++", os.path.join(HERE, "cpp", "pass2_choice_table.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def summary(program):
    """(rows, {instance: rows that reach it}, unlisted instances, unreached instances)"""
    run = subprocess.run([program, "--summary"], capture_output=True, text=True)
    rows, reach, unlisted, unreached = None, {}, [], []
    for line in run.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        if kind == "rows":
            rows = int(rest)
        elif kind == "reach":
            count, label = rest.split(" ", 1)
            reach[label] = int(count)
        else:
            {"unlisted": unlisted, "unreached": unreached}[kind].append(rest)
    assert run.returncode == (1 if unlisted else 0)
    return rows, reach, unlisted, unreached


def test_the_table_is_the_recorded_one(program):
    sha, rows = hashlib.sha256(), 0
    with subprocess.Popen([program], stdout=subprocess.PIPE) as run:
        for chunk in iter(lambda: run.stdout.read(1 << 20), b""):
            sha.update(chunk)
            rows += chunk.count(b"\n")
    assert run.returncode == 0
    assert rows == GOLDEN["rows"]
    assert sha.hexdigest() == GOLDEN["sha256"]


def test_every_instance_is_reached_by_the_recorded_number_of_rows(summary):
    rows, reach, _, _ = summary
    assert rows == GOLDEN["rows"]
    want = GOLDEN["rows_per_instance"]
    moved = {label: (want.get(label, 0), reach.get(label, 0)) for label in sorted(set(want) | set(reach)) if want.get(label, 0) != reach.get(label, 0)}
    assert not moved, f"rows per instance (recorded, now): {moved}"


def test_every_chosen_instance_is_in_the_launchers_lists(summary):
    assert summary[2] == []


def test_every_listed_instance_is_reached_or_known_unreachable(summary):
    unreached = summary[3]
    patterns = [re.compile(entry["pattern"]) for entry in GOLDEN["unreachable"]]
    assert all(entry["reason"] for entry in GOLDEN["unreachable"])
    unexplained = [label for label in unreached if not any(p.search(label) for p in patterns)]
    assert unexplained == []
    idle = [p.pattern for p in patterns if not any(p.search(label) for label in unreached)]
    assert idle == [], "patterns that excuse nothing"
