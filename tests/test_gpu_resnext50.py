"""The resnext50_32x4d fp16 engine at 64 x 64, batch 2, against the fp64 torch twin: the sixteen grouped layers on kernels/conv_slab.hip, and on the direct
kernel under TRTX_CONV_SLAB=0.  Bound: fp16_walk(107, ref_max), resnet50_64's (tests/parity.py): the same 53 convolutions + fc, 54 weight and 53 activation sites."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import engine
from tests import conv_slab_cases as sc
from tests import parity, util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    sd, path = sc.resnext50_wts(tmp_path_factory.mktemp("resnext"))
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    with torch.inference_mode():
        return engine.build_plan("resnext50_32x4d", path, batch=2, fp16=1, h=64, w=64), x, sc.resnext50_twin(sd, x.double())


@pytest.mark.parametrize("slab", [True, False], ids=["slab", "direct"])
def test_fp16_engine_matches_the_fp64_twin(gpu, model, slab, monkeypatch):
    plan, x, ref = model
    if not slab:
        monkeypatch.setenv("TRTX_CONV_SLAB", "0")
    grouped = [o for o in engine.describe_plan(plan, lowered=True)["ops"] if o["kind"] == "conv" and not o["igemm"] and not o["stem"]]
    assert len(grouped) == 16 and all((o.get("slab") is True) == slab for o in grouped), grouped
    e = engine.Engine(plan)
    try:
        bufs = [x.to(gpu) if e.is_input[i] else torch.full((2 * int(np.prod(e.dims[i])),), float("nan"), device=gpu) for i in range(e.nb_bindings)]
        with util.time_limit():
            e.enqueue(2, bufs)
            util.sync("resnext50_32x4d")
        out = bufs[e.names.index("prob")].cpu().reshape(2, 1000).double()
    finally:
        e.close()
    err, ref_max = (out - ref).abs().max().item(), ref.abs().max().item()
    print(f"resnext50_32x4d fp16 64x64 {'slab' if slab else 'direct'}: max err {err:.4f}, bound {parity.fp16_walk(107, ref_max):.4f}, ref max {ref_max:.1f}")
    assert err <= parity.fp16_walk(107, ref_max)
