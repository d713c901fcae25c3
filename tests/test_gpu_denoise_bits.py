"""Bitwise guard of the denoising loop (csrc/denoise.hip and every kernel it launches: rowops.hip, rownorm.h, gemm.hip,
skinny.hip): x, the echo energy, the echo rows and all workspaces of the calls in tests/golden/make_golden_denoise_bits.py's
CASES must hash to what tests/golden/denoise_bits.json records. The fixture was written by that generator on an MI355X from
the library built at the commit it names (meta.commit); it holds SHA-256 digests only, of the inputs too, so that a drift
of the seeded CPU generators shows as an input mismatch rather than as a kernel failure.

The recorded bits pin the PRESENT launch sequence and arithmetic: which kernel runs a step's GEMMs and row passes and in which
order, the offsets each launch is given, the sampler step, and the summation order of the guidance-renorm ratio (wave sum, then
(r0 + r1) + (r2 + r3), then the echo term). Graph capture and graph replay must give the direct call's recorded digests. A pull
request that changes an order on purpose regenerates the fixture with the generator and says so."""
import json
import os
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_GENERATOR = os.path.join(HERE, "golden", "make_golden_denoise_bits.py")
G = types.ModuleType("make_golden_denoise_bits")  # the generator's CASES and run_case, loaded without a bytecode cache beside the fixtures
G.__file__ = _GENERATOR
with open(_GENERATOR) as _f:
    exec(compile(_f.read(), _GENERATOR, "exec"), G.__dict__)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "denoise_bits.json")) as f:
        return json.load(f)


def test_fixture_records_every_case_and_its_commit(golden):
    assert sorted(golden["cases"]) == sorted(G.CASES)
    assert len(golden["meta"]["commit"]) == 40 and int(golden["meta"]["commit"], 16) >= 0
    for name, rec in golden["cases"].items():
        assert rec["inputs"] and rec["outputs"], name
        for sha in list(rec["inputs"].values()) + list(rec["outputs"].values()):
            assert len(sha) == 64 and int(sha, 16) >= 0, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_same_bits_as_recorded(hip, golden, name):
    ins, outs = G.run_case(name, hip.load())
    want = golden["cases"][name]
    assert ins == want["inputs"], f"{name}: the seeded inputs are not the recorded ones (generator drift, not a kernel failure)"
    assert sorted(outs) == sorted(want["outputs"])
    differ = [k for k in sorted(outs) if outs[k] != want["outputs"][k]]
    assert not differ, f"{name}: {differ} differ from the build at {golden['meta']['commit']}"
    if name.startswith("graph/"):  # capture and replay against the DIRECT call's record
        direct = golden["cases"][G.direct_case_of(name)]["outputs"]
        differ = [f"{tag}/{k}" for tag in ("capture", "replay") for k in sorted(direct) if outs[f"{tag}/{k}"] != direct[k]]
        assert not differ, f"{name}: {differ} differ from the direct launches of the build at {golden['meta']['commit']}"
