"""The launch sequence of the region paths, without a GPU: FpnRegionPath / C4RegionPath are built on the CPU against a recording
stand-in for the native library (tests/golden/make_region_path_launches.py) and every dtc_* call they issue -- entry point, order,
each argument with pointers named by the path attribute they belong to -- must equal tests/golden/region_path_launches.json, which
was generated before the two classes were rebuilt on one base.  The fixture also pins the name, dtype and shape of every public tensor
attribute after construction + bind."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN


def _recorder():
    spec = importlib.util.spec_from_file_location("make_region_path_launches", os.path.join(GOLDEN, "make_region_path_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "region_path_launches.json")) as f:
        return json.load(f)


@pytest.fixture()
def got(monkeypatch):
    rec = _recorder()
    return json.loads(rec.dumps(rec.record(monkeypatch.setattr)))          # through JSON: tuples -> lists, as in the fixture


def test_same_configurations(got, want):
    assert sorted(got) == sorted(want) and len(want) == 12


def test_launches_equal_fixture(got, want):
    for cfg in want:
        g, w = got[cfg]["phases"], want[cfg]["phases"]
        assert [p["phase"] for p in g] == [p["phase"] for p in w], cfg
        for pg, pw in zip(g, w):
            assert [c[0] for c in pg["calls"]] == [c[0] for c in pw["calls"]], (cfg, pw["phase"])
            for cg, cw in zip(pg["calls"], pw["calls"]):
                assert cg == cw, (cfg, pw["phase"], cw[0])


def test_public_tensor_attributes_kept(got, want):
    for cfg in want:
        g, w = got[cfg]["tensors"], want[cfg]["tensors"]
        for name, sig in w.items():
            assert g.get(name) == sig, (cfg, name)
        assert ("mask_feats" in g) == ("mask_feats" in w), cfg
    assert "mask_feats" not in want["c4_default"]["tensors"] and "mask_feats" in want["c4_masks_rle"]["tensors"]


def test_stand_ins_are_restored():
    from detectorch_amd import hip
    assert not type(hip._lib).__name__ == "RecordingLib" and hip.stream_ptr.__name__ == "stream_ptr"
