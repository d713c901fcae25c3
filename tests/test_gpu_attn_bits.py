"""Bitwise guard of the attention forward kernels (csrc/attn.hip, attn16.hip, attn_tile.h): every output buffer of the calls
in tests/golden/make_golden_attn_bits.py's CASES must hash to what tests/golden/attn_fwd_bits.json records. The fixture
was written by that generator on an MI355X from the library built at the commit it names (meta.commit); it holds SHA-256
digests only, of the inputs too, so that a drift of the seeded CPU generators shows as an input mismatch rather than as a
kernel failure. The generator's vit* cases pin whole block stacks the same way (csrc/capi.hip: the plain, the fp8 and the
KV-cached stack, each launch's walk direction and arguments included).

The recorded bits pin the PRESENT summation order of the kernels: the K/V tile order, the deferred rescale, the MFMA
contraction order and the row-sum form of each structure. A pull request that changes an order on purpose regenerates the
fixture with the generator and says so."""
import json
import os
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_GENERATOR = os.path.join(HERE, "golden", "make_golden_attn_bits.py")
G = types.ModuleType("make_golden_attn_bits")  # the generator's CASES and run_case, loaded without a bytecode cache beside the fixtures
G.__file__ = _GENERATOR
with open(_GENERATOR) as _f:
    exec(compile(_f.read(), _GENERATOR, "exec"), G.__dict__)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "attn_fwd_bits.json")) as f:
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
