"""Every nova_pointset_* entry point answers bad arguments as tests/golden/pointset_errors.json recorded it: the same return
code and the same nova_last_error() text, call by call (CPU: every call of the table returns before any HIP call).

The table (tests/golden/make_golden_pointset_errors.py) holds one call per argument check and per early `return 0`, and for
the entry points whose checks once sat in two files, calls that break two checks at once, which pins their order. It must
keep up with the source: each set_error / NOVA_REQUIRE site of the point-set files needs a recorded message that its format
string produces: as many different recorded answers of a form as there are sites that say it."""
import json
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nova_pointcloud_amd", "csrc")
POINTSET_SOURCES = ["pointset.hip", "nearest_match.hip", "matched.hip", "chamfer.hip", "emd.hip", "occupancy.hip", "fps.hip", "knn.hip",
                    "neighbor.hip", "interp.hip", "interp_bwd.hip", "soft_cluster.hip", "assign.hip", "interp_common.h", "pointset_common.h"]
# format string of a site -> why no call of the table can reach it
EXEMPT = {
    # only in the sources of the commit the table was recorded from (this test passes on them too); emd.hip no longer says it
    "pointset_emd_matrix: N %d outside 1 .. %d (the maximum point count)":
        "a second statement of the N range behind the first one (which ends in NOVA_EMD_MAX_POINTS): no argument gets to it",
}

STRING = r'"((?:[^"\\]|\\.)*)"'
SITE = re.compile(r"\bset_error\(\s*NOVA_ERR_\w+,\s*" + STRING + r"|\bNOVA_REQUIRE\((?:[^;]|\n)*?,\s*NOVA_ERR_\w+,\s*" + STRING)


def table():
    with open(os.path.join(ROOT, "tests", "golden", "pointset_errors.json")) as f:
        return json.load(f)


def sites():
    """The format string of every argument check of the point-set entry points, one per site."""
    found = []
    for name in POINTSET_SOURCES + ["capi.hip"]:
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for m in SITE.finditer(text):
            fmt = m.group(1) if m.group(1) is not None else m.group(2)
            if name != "capi.hip" or fmt.startswith("pointset_"):  # capi.hip: only what it says about these entry points
                found.append(fmt)
    return found


def as_regex(fmt):
    """A printf format of these files as the pattern of the messages it produces."""
    parts = re.split(r"(%ld|%d|%g|%s|%%)", fmt)
    conv = {"%d": r"-?\d+", "%ld": r"-?\d+", "%g": r"[-+.\w]+", "%s": r"\w+", "%%": "%"}
    return re.compile("".join(conv.get(p, re.escape(p)) for p in parts) + r"\Z")


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_table_covers_every_check_in_the_source():
    t = table()
    messages = [c["message"] for c in t["cases"] if c["rc"] != 0]
    fmts = [f for f in sites() if f not in EXEMPT]
    assert len(fmts) >= 70, fmts  # the scan itself: about 75 sites exist
    # format by format: n sites that say the same thing (the `%s: ...` checks of several entry points, an entry point's null
    # checks in two statements) need n recorded calls answered so, so a new site is seen even where its text is an old one
    for fmt in sorted(set(fmts)):
        reached = sum(1 for m in messages if as_regex(fmt).match(m))
        assert reached >= fmts.count(fmt), f"{fmts.count(fmt)} check(s) say, but only {reached} recorded call(s) are answered: {fmt}"
    assert len(messages) >= len(fmts), (len(messages), len(fmts))
    # one early return at least for every entry point that has one (nova_pointset_assignment launches even with B <= 0)
    early = {c["entry"] for c in t["cases"] if c["rc"] == 0}
    assert early == {c["entry"] for c in t["cases"]} - {"assignment"}, early


def test_generator_and_table_agree():
    """The committed table is the generator's list of calls, in its order (the answers are the recorded commit's)."""
    from golden.make_golden_pointset_errors import STATE_BYTES, cases

    t = table()
    assert re.fullmatch(r"[0-9a-f]{40}", t["commit"])
    got = [(c["entry"], c["args"]) for c in t["cases"]]
    want = cases()
    assert len(got) == len(want)
    for (ge, ga), (we, wa) in zip(got, want):
        assert ge == we and len(ga) == len(wa) and all(same(a, b) for a, b in zip(ga, wa)), (ge, ga, we, wa)
    assert [n for n, _ in t["state_bytes"]] == STATE_BYTES


def test_current_build_answers_as_recorded():
    """The replay (hip.load(check_device=False), every call of the table, code and text compared exactly) in a child process
    that sees no GPU: the calls carry addresses of nothing, and a build that lost a check would launch on them. Without a
    device that launch fails with a return code, which is a failed comparison here and not a fault on a device."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_pointset_errors.py"), "--replay"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.strip().endswith(f"replayed {len(table()['cases'])} cases"), out.stdout[-2000:]
