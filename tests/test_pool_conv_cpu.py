"""match_pool_conv without a GPU: where it is asked to (TRTX_POOL_CONV=2: the one launch measured slower at every shape of profiles/pool_conv_time.jsonl, so the
unset switch admits none) YOLOv9's AConv / ADown lower to one "pool_conv" op per convolution and no average pool; fp32 and kINT8 engines, the unset and the
cleared switch and near misses keep the pool ops."""
import collections

import pytest

from tensorrtx_amd import engine
from tests import pool_conv_cases as pc
from tests.test_yolov9_cpu import lowered

# host/yolov9.cpp, spec_of() and buildEngineYolov9(): (downsampling blocks the builder connects, convolutions per block: AConv 1, ADown 2).  t and gelan-c: L3, L5,
# L7, L16, L19; c: L3, L5, L7 and the auxiliary branch's three (model.28, 31, 34)
DOWNS = {"yolov9t": (5, 1), "gelanc": (5, 2), "yolov9c": (6, 2)}


def _kinds(low):
    return collections.Counter(o["kind"] for o in low["ops"])


def _avg_pools(low):
    return [o for o in low["ops"] if o["kind"] == "pool" and o["k"] == [2, 2] and o["stride"] == [1, 1]]


@pytest.mark.parametrize("name", list(DOWNS))
def test_yolov9_downsamplers_become_pool_conv_ops(name, monkeypatch):
    blocks, per = DOWNS[name]
    monkeypatch.setenv("TRTX_POOL_CONV", "2")
    low = lowered(name, batch=1, h=64, w=64, fp16=1)[1]
    fused = [o for o in low["ops"] if o["kind"] == "pool_conv"]
    assert len(fused) == blocks * per and not _avg_pools(low), _kinds(low)
    assert [o["mode"] for o in fused].count("avgmax_c1") == (blocks if per == 2 else 0)
    assert all(o["bn_folded"] and o["act1"] == 3 and o["ld_in"] % 8 == 0 and o["ld_out"] % 8 == 0 and o["hw_out"] == [o["hw_in"][0] // 2, o["hw_in"][1] // 2] for o in fused), fused
    # an fp32 engine, the admission rule (no shape measured faster) and the switch keep today's ops: one average pool per block
    for kw, env in ((dict(fp16=0), "2"), (dict(fp16=1), "1"), (dict(fp16=1), "0")):
        monkeypatch.setenv("TRTX_POOL_CONV", env)
        low0 = lowered(name, batch=1, h=64, w=64, **kw)[1]
        assert _kinds(low0)["pool_conv"] == 0 and len(_avg_pools(low0)) == blocks, _kinds(low0)


@pytest.mark.parametrize("kind,kw,want", [("adown", {}, 2), ("aconv", {}, 1), ("adown", dict(miss="reader"), 0), ("aconv", dict(miss="output"), 0),
                                          ("adown", dict(int8=True), 0), ("aconv", dict(fp16=False), 0), ("adown", dict(C=24), 0)])   # C 24: halves of 12 channels
def test_matcher_takes_whole_blocks_or_nothing(kind, kw, want, monkeypatch):
    monkeypatch.setenv("TRTX_POOL_CONV", "2")
    plan, layers = pc.down_net(kind, **{**dict(B=2, C=32, H=12, W=14, cout=48), **kw})
    k = _kinds(engine.describe_plan(plan, lowered=True))
    assert k["pool_conv"] == want and k["conv"] == len(layers) - want and (k["pool"] == 0) == (want > 0), k
