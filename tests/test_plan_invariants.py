"""Host-side planning of the engine (msm_plan.h make_plan): invariants over the whole supported size range,
including pair counts far beyond what the GPU tests run (up to 2^31 - 1)."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_dump_row_digests.txt")

# SHA-256 and row count of `t_plan --dump`, recorded from the library BEFORE planning moved into msm_plan.h (msm_pipeline.h of commit
# bc26225, the sort's argument fill and buffer sizes as accumulate_pairs had them): a refactoring of the planning leaves every row alone.
PLAN_DUMP_SHA256 = "9c87d68f49918870f59324138b3e54d1bedd1f5d754ced2f3935413a93e03917"
PLAN_DUMP_ROWS = 10551


@pytest.fixture(scope="module")
def t_plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("t_plan") / "t_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "constantine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_api", "t_plan.cpp"), "-o", exe])
    return exe


def test_plan_invariants(t_plan):
    out = subprocess.run([t_plan], capture_output=True, text=True)
    assert out.returncode == 0 and "plans ok" in out.stdout, out.stdout[-2000:]


def test_plans_are_what_they_were(t_plan):
    """Every MsmPlan field, the sort's sizing and six buffer sizes, both window choosers and host_slices over the grid of t_plan.cpp's dump."""
    out = subprocess.run([t_plan, "--dump"], capture_output=True, check=True).stdout
    if hashlib.sha256(out).hexdigest() == PLAN_DUMP_SHA256:
        return
    rows = out.decode().splitlines()
    # the digest cannot say where: the recorded rows' own digests (8 hex digits each, same order) can
    with open(GOLDEN) as f:
        want = f.read().split()
    assert len(want) == PLAN_DUMP_ROWS
    for i, (row, w) in enumerate(zip(rows, want)):
        assert hashlib.sha256(row.encode()).hexdigest()[:8] == w, f"row {i + 1} of the plan dump differs from the recorded one (only its digest is kept, not its text); it is now: {row}"
    assert len(rows) == PLAN_DUMP_ROWS, f"{len(rows)} rows, {PLAN_DUMP_ROWS} recorded"
    raise AssertionError("the plan dump differs from the recorded one in a way its rows do not show (line ends?)")
