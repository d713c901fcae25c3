"""Bitwise guard of the point-set kernels (pointset, chamfer, emd, occupancy, fps, assign, knn): every output of the calls
recorded in tests/golden/pointset_bits.npz must come back bit for bit from the current build. The file was written by
tests/golden/make_golden_pointset_bits.py on an MI355X from the library built at the commit it names (meta["commit"]);
it holds the inputs themselves, and that generator's CASES says what each case calls and which code path it reaches.

What the recorded bits mean:
  - integer outputs (kNN and FPS indices, the assignment and its rounds, occupancy counters, nodes and the outside
    count) and floats defined element by element (kNN d2, FPS distances, nn_dist, pairwise_dist) are permanent facts of
    the contract in include/nova_hip.h: no later change may move them;
  - summed floats (the Chamfer and EMD matrix entries, the assignment's mean cost) pin the PRESENT summation order. A
    pull request that changes an order on purpose regenerates the file with the generator and says so.

An output above the generator's DIGEST_ABOVE bytes is held as its SHA-256; the 512-cloud kNN case is 8 distinct cloud pairs
repeated 64 times, stored once, and every repetition must equal the stored result."""
import json
import os
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_GENERATOR = os.path.join(HERE, "golden", "make_golden_pointset_bits.py")
G = types.ModuleType("make_golden_pointset_bits")  # the generator's CASES and run_case, loaded without a bytecode cache beside the fixtures
G.__file__ = _GENERATOR
with open(_GENERATOR) as _f:
    exec(compile(_f.read(), _GENERATOR, "exec"), G.__dict__)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "pointset_bits.npz")) as f:
        arrays = {k: f[k] for k in f.files}
    return arrays, json.loads(str(arrays["meta"]))


def test_fixture_records_every_case_and_its_commit():
    with np.load(os.path.join(HERE, "golden", "pointset_bits.npz")) as f:
        meta = json.loads(str(f["meta"]))
        assert sorted(meta["outputs"]) == sorted(G.CASES)
        assert len(meta["commit"]) == 40 and int(meta["commit"], 16) >= 0
        for name, outs in meta["outputs"].items():
            for e in outs:
                assert ("sha256" in e) != (f"{name}/{e['name']}" in f.files), (name, e)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_same_bits_as_recorded(hip, golden, name):
    arrays, meta = golden
    got = G.run_case(name, arrays)
    want = meta["outputs"][name]
    assert [k for k, _ in got] == [e["name"] for e in want]
    for (k, v), e in zip(got, want):
        assert str(v.dtype) == e["dtype"] and list(v.shape) == e["shape"], (name, k, v.dtype, v.shape, e)
        if "sha256" in e:
            assert G.digest(v) == e["sha256"], f"{name}/{k}: bits differ from the build at {meta['commit']}"
        else:
            ref = arrays[f"{name}/{k}"]
            differ = np.frombuffer(v.tobytes(), np.uint8) != np.frombuffer(ref.tobytes(), np.uint8)
            assert not differ.any(), f"{name}/{k}: {int(differ.sum())} bytes of {differ.size} differ from the build at {meta['commit']}"
