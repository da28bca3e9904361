"""PSA attention on the matrix pipe as the host sees it: the lowered plans carry "mfma" on their attention op - heads of 72 unless TRTX_PSA_MFMA=0, heads of
64 with TRTX_PSA_MFMA=2 (their default lowering is pinned by tests/test_yolo12_cpu.py) - and the C entry is declared, exported and bound."""
import os
import re

import pytest

from tensorrtx_amd import capi, engine, synth, wts


# yolo11n as tests/test_yolo11_cpu.py lowers it (kd 32 / hd 64); yolov10m has the heads of 72
@pytest.mark.parametrize("model,state,kw,shape,on", [("yolo11n", lambda: synth.yolo11_state("n"), dict(batch=32, h=640, w=640), (32, 64), "2"),
                                                     ("yolov10m", lambda: synth.yolov10_state("yolov10m"), dict(batch=1, h=64, w=64), (36, 72), None)])
def test_lowered_plans_route_psa_to_the_mfma_kernel(model, state, kw, shape, on, monkeypatch, tmp_path):
    path = str(tmp_path / f"{model}.wts")
    wts.write_wts(path, state(), dialect="double")
    for switch, flag in ((None, True if on is None else None), ("2", True), ("0", None)):   # the switch is read at every lowering
        monkeypatch.delenv("TRTX_PSA_MFMA", raising=False) if switch is None else monkeypatch.setenv("TRTX_PSA_MFMA", switch)
        low = engine.describe_plan(engine.build_plan(model, path, fp16=1, **kw), lowered=True)
        (att,) = [o for o in low["ops"] if o["kind"] == "attention"]
        assert (att["kd"], att["hd"], att.get("mfma")) == (*shape, flag) and "area" not in att


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trtx_hip.h")).read()
    assert re.search(r"\btrtx_op_psa_attention_mfma_f16\(", header)
    assert hasattr(capi.lib(), "trtx_op_psa_attention_mfma_f16") and callable(capi.psa_attention_mfma)
