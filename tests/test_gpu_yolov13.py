"""YOLOv13's additions to the runtime on the device (tests/yolov13_cases.py): kEXP in both layouts, the spelled-out softmax chain (fused
into the softmax op, and its near-misses on the generic ops), and the gated add (scalar and per-channel gates, dense and concat-slice
destinations, both operand orders, the switch-off route) - every case through engine.Engine as an fp32 and as an fp16 plan against its own
torch fp64 reference, with tests/test_gpu_layers.py's checker and error model: every element of every binding, NaN-prefilled outputs, the
concat neighbour's channels bit for bit.  The checker prints max err / bound per binding."""
import pytest

from tests import test_gpu_layers as layers
from tests import yolov13_cases as yc

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", yc.EXP_CASES, ids=_ids(yc.EXP_CASES))
def test_exp_matches_fp64_reference(case, fp16, gpu):
    layers.test_layer_matches_fp64_reference(case, fp16, gpu)


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", yc.CHAIN_CASES + yc.CHAIN_NEAR_MISSES, ids=_ids(yc.CHAIN_CASES + yc.CHAIN_NEAR_MISSES))
def test_softmax_chain_matches_fp64_reference(case, fp16, gpu):
    layers.test_layer_matches_fp64_reference(case, fp16, gpu)


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", yc.GATED_CASES + yc.GATED_NEAR_MISSES, ids=_ids(yc.GATED_CASES + yc.GATED_NEAR_MISSES))
def test_gated_add_matches_fp64_reference(case, fp16, gpu):
    layers.test_layer_matches_fp64_reference(case, fp16, gpu)


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", yc.GATED_GENERIC, ids=_ids(yc.GATED_GENERIC))
def test_gated_add_switch_off_route_matches_fp64_reference(case, fp16, gpu, monkeypatch):
    """TRTX_GATED_ADD=0: the same networks on the generic ops, against the same references with the second rounding site that route has - so the
    two routes agree within the sum of their bounds"""
    monkeypatch.setenv("TRTX_GATED_ADD", "0")
    layers.test_layer_matches_fp64_reference(case, fp16, gpu)
