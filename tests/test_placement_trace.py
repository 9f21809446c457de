"""Where and when the MSM pipeline runs each stage (msm_pipeline.h MsmEngine over a backend that only writes down what it is asked to
do: tests/c_api/t_place.cpp), over curves, lane counts, sizes, pipeline depths, options, backend shapes and the environment knobs.
No GPU, no kernels: the text of every row is pinned, as tests/test_plan_invariants.py pins the plans."""
import hashlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "placement_trace_row_digests.txt")
SOURCE = os.path.join(ROOT, "tests", "c_api", "t_place.cpp")

# The dumps: the full grid with no knob set, and the small grid (t_place --small) once with no knob set and once per environment knob at
# a value that is not its default -- a knob is read once per process.  (TAIL_MIN_FREE = 40: what BLS12-381 G1 leaves free at 2^20 pairs,
# the one size of the small grid where the comparison is between equals.)
KNOBS = ["", "WIDE_EARLY=0", "TAIL_MIN_FREE=40", "TAIL_FREE_RATIO=0.1", "SMALL_FREE_32NDS=5", "FRONT=0", "FRONT=2", "EARLY_TAIL=0",
         "EARLY_TAIL=2", "LATE_POINTS=0"]
DUMP_NAMES = ["full"] + ["small " + k if k else "small" for k in KNOBS]

# SHA-256 and row count of each dump, recorded from the pipeline BEFORE its placement decisions moved into msm_place.h (msm_pipeline.h of
# commit 82abdc3) by `python tests/test_placement_trace.py --record`: a refactoring of the placement leaves every row alone.
TRACE = {
    "full": ("d200516b18a4a674f4a8778cc27e210b1fad0329123d007e35c82363ba691a63", 9152),
    "small": ("c473333bae61ab817fba1c470a67e173413fb08f4280d9f6c0262cde40bd9a88", 111),
    "small WIDE_EARLY=0": ("a2f259a55d1d7fb6ab9631726f55dc94fd447776d5a45a6a0e3c12f6ab2cda53", 111),
    "small TAIL_MIN_FREE=40": ("d683f469bdbe98c3bebee2e2830f7bacf3bd2f5bb3e98a6a3feaa7bddf2bfbe1", 111),
    "small TAIL_FREE_RATIO=0.1": ("2285527c9a34cbeb9d0e693f000424560d08d8e87d3bc853ea0ed4a6775f0adf", 111),
    "small SMALL_FREE_32NDS=5": ("8dfc141e694df0085f72f901107c48cffe394409f96e84f4981bbb49caf3f616", 111),
    "small FRONT=0": ("4d56332bbae813164b04c8812be7053eb49bb51d3b72af4a54ad88cd06c9268a", 111),
    "small FRONT=2": ("c83de0024a129b0dbdedc7194e1de6984eb17d68bd73911bb3500f3cb6dc97ea", 111),
    "small EARLY_TAIL=0": ("e1185a3581202ca0c1daca49db54f23b26daab793c35e8664a4580cde8eb024c", 111),
    "small EARLY_TAIL=2": ("3bb9c26503f49b519f79d0de1d0565a7a7bef5918d77ec9ea73d4741d128d086", 111),
    "small LATE_POINTS=0": ("9e6a1277186ae48ef054dd1534047320f0794f23bfe54023b992f92eb3fc0536", 111),
}


def build(exe):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "constantine_amd", "csrc"), SOURCE, "-o", exe])


def dump(exe, name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTT_")}
    args = [exe]
    if name != "full":
        args.append("--small")
        knob = name[len("small "):]
        if knob:
            key, value = knob.split("=")
            env["CTT_HIP_MSM_" + key] = value
    return subprocess.run(args, env=env, capture_output=True, check=True).stdout


def row_digest(row):
    return hashlib.sha256(row.encode()).hexdigest()[:8]


def golden_rows():
    """{dump name: [8 hex digits per row]} -- sections '# <name>' of the golden file"""
    out, cur = {}, None
    with open(GOLDEN) as f:
        for line in f:
            line = line.strip()
            if line.startswith("# "):
                cur = out.setdefault(line[2:], [])
            elif line:
                cur.append(line)
    return out


@pytest.fixture(scope="module")
def t_place(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("t_place") / "t_place")
    build(exe)
    return exe


def test_every_knob_moves_a_row():
    """the recorded dumps of the small grid differ from one another: each knob's value shows in at least one row"""
    small = [TRACE[n][0] for n in DUMP_NAMES[1:]]
    assert len(set(small)) == len(small)


@pytest.mark.parametrize("name", DUMP_NAMES)
def test_placements_are_what_they_were(t_place, name):
    """Every launch, wait and mark of every submit of the grid, in order, with the plan fields the placement feeds."""
    out = dump(t_place, name)
    sha, nrows = TRACE[name]
    if hashlib.sha256(out).hexdigest() == sha:
        return
    rows = out.decode().splitlines()
    # the digest cannot say where: the recorded rows' own digests (8 hex digits each, same order) can
    want = golden_rows()[name]
    assert len(want) == nrows
    for i, (row, w) in enumerate(zip(rows, want)):
        assert row_digest(row) == w, f"row {i + 1} of the placement trace '{name}' differs from the recorded one (only its digest is kept, not its text); it is now: {row}"
    assert len(rows) == nrows, f"{len(rows)} rows, {nrows} recorded"
    raise AssertionError("the placement trace differs from the recorded one in a way its rows do not show (line ends?)")


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "t_place")
        build(exe)
        with open(GOLDEN, "w") as g:
            print("TRACE = {")
            for name in DUMP_NAMES:
                out = dump(exe, name)
                rows = out.decode().splitlines()
                g.write(f"# {name}\n" + "".join(row_digest(r) + "\n" for r in rows))
                print(f'    "{name}": ("{hashlib.sha256(out).hexdigest()}", {len(rows)}),')
            print("}")
