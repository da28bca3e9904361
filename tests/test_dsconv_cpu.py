"""match_dsconv without a GPU: a DSBottleneck as the reference spells it lowers to one "dsconv" op per DSConv; every near miss keeps two "conv" ops."""
import pytest

from tensorrtx_amd import engine
from tests import dsconv_cases as dc

GEOM = dict(B=2, C=16, H=12, W=10, k1=3, k2=7, shortcut=True, stride=1)
# (arguments of dsbottleneck_net, TRTX_DSCONV (1 is what unset means), which of the DSConvs become "dsconv" ops)
VARIANTS = {"reference_spelling": ({}, "1", [0, 1]), "stride2_single_cin_ne_cout": (dict(stride=2, single=True, cout=24, shortcut=False), "1", [0]),
            "scale_behind_dw": (dict(miss="scale"), "1", [1]), "activation_behind_dw": (dict(miss="act"), "1", [1]), "bias_on_dw": (dict(miss="bias"), "1", [1]),
            "second_reader": (dict(miss="reader"), "1", [1]), "dw_is_network_output": (dict(miss="output"), "1", [1]), "dilation2": (dict(miss="dilation"), "1", [1]),
            "fp32_engine": (dict(fp16=False), "1", []), "int8_engine": (dict(int8=True), "1", []), "switch_off": ({}, "0", [])}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_matcher_claims_the_reference_spelling_and_declines_near_misses(name, monkeypatch):
    kw, switch, want = VARIANTS[name]
    monkeypatch.setenv("TRTX_DSCONV", switch)
    g = {**GEOM, **kw}
    plan, layers = dc.dsbottleneck_net(**g)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    fused = [o for o in ops if o["kind"] == "dsconv"]
    assert len(fused) == len(want) and sum(o["kind"] == "conv" for o in ops) == 2 * (len(layers) - len(want)), [o["kind"] for o in ops]
    for j, o in zip(want, fused):   # the whole block in the op: the folded BatchNorm, the SiLU, the bottleneck's sum on the last one; and the fused route
        assert (o["bn_folded"] and o["act1"] == 3 and (o["cin"], o["dw_k"], o["dw_stride"]) == (g["C"], *layers[j][3:]) and o["fused"] and o["ws_bytes"] > 0 and
                o["residual"] == (g["shortcut"] and j == len(layers) - 1)), o
