"""YOLOv13's additions to the runtime, on the host (tests/yolov13_cases.py): IUnaryLayer through the C ABI, the shim and builder.Network,
the lowering of kEXP, of the spelled-out softmax chain and of the gated add, their near-misses and switch, and the oracle's interpreter
(which is handed an equivalent description: it does not know the unary kind) against each case's own fp64 reference."""
import ctypes
import dataclasses
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from tensorrtx_amd import builder, capi, engine
from tests import layer_cases as lc
from tests import yolov13_cases as yc
from tests.test_layers_cpu import _is_vec, instantiations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = yc.EXP_CASES + yc.CHAIN_CASES + yc.CHAIN_NEAR_MISSES + yc.GATED_CASES + yc.GATED_NEAR_MISSES
IDS = [c.name for c in ALL]


def _ops(plan):
    return engine.describe_plan(plan, lowered=True)["ops"]


# ---- IUnaryLayer: the ABI, the shim, the builder ---------------------------------------------------------------------------------------------
def test_unary_entry_is_exported_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    assert re.search(r"int32_t\s+trtx_network_add_unary\s*\(trtx_network\* n, int32_t input, int32_t op\);", src)
    assert "yolov13/src/block.cpp:389" in src
    assert hasattr(capi.lib(), "trtx_network_add_unary")
    shim = open(os.path.join(ROOT, "include", "NvInfer.h")).read()
    ops = re.search(r"enum class UnaryOperation : int32_t \{(.*?)\};", shim, re.S).group(1)
    got = {k: int(v) for k, v in re.findall(r"(k[A-Z]+) = (\d+)", ops)}
    want = ["kEXP", "kLOG", "kSQRT", "kRECIP", "kABS", "kNEG", "kSIN", "kCOS", "kTAN", "kSINH", "kCOSH", "kASIN", "kACOS", "kATAN", "kASINH", "kACOSH",
            "kATANH", "kCEIL", "kFLOOR", "kERF", "kNOT", "kSIGN", "kROUND", "kISINF"]     # TensorRT's enumerators, in TensorRT's order
    assert got == {k: i for i, k in enumerate(want)}
    assert "class IUnaryLayer" in shim and re.search(r"IUnaryLayer\* addUnary\(ITensor& in, UnaryOperation op\)", shim)
    assert callable(builder.Network.unary)


def test_bad_arguments_to_add_unary_are_refused():
    net = builder.Network()
    try:
        x = net.input("x", (4, 5))
        fn = net.L.trtx_network_add_unary
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
        assert fn(None, x, 0) == -1
        assert fn(net.n, -1, 0) == -1 and fn(net.n, 99, 0) == -1
        for op in (-1, 24, 1000):
            with pytest.raises(RuntimeError, match=f"{op} is no UnaryOperation"):
                net.unary(x, op)
        assert net.unary(x, 0) >= 0 and net.unary(x, 23) >= 0       # every enumerator is a layer; which of them has a kernel is the build's business
    finally:
        net.close()


def test_unary_layer_is_inferred_serialized_and_described():
    net = builder.Network(max_batch=2)
    try:
        x = net.input("x", (3, 4, 5))
        l = net.unary(x, "exp")
        d = builder.Dims()
        assert net.L.trtx_tensor_get_dims(net.n, net.out(l), ctypes.byref(d)) == 0 and list(d.d[:d.nb]) == [3, 4, 5]     # while the network is being built
        net.mark_output(net.out(l), "y")
        plan = net.build()
    finally:
        net.close()
    desc = engine.describe_plan(plan)        # the plan bytes, deserialized
    (u,) = [l for l in desc["layers"] if l["kind"] == yc.L_UNARY]
    assert u["op"] == 0 and desc["tensors"][u["outputs"][0]]["dims"] == [3, 4, 5] and desc["tensors"][u["outputs"][0]]["name"] == "y"
    assert [l["kind"] for l in desc["layers"]] == [yc.L_UNARY]
    assert gi.L_IDENTITY == 17 and yc.L_UNARY == 18      # appended: plans written before it read as before (the golden plan hashes pin those)


@pytest.mark.parametrize("op,name", [(1, "kLOG"), (2, "kSQRT"), (4, "kABS"), (19, "kERF"), (23, "kISINF")])
def test_another_unary_operation_is_a_build_error_that_names_it(op, name, capfd):
    net = builder.Network()
    try:
        net.mark_output(net.out(net.unary(net.input("x", (4, 5)), op)), "y")
        with pytest.raises(Exception):
            net.build()
    finally:
        net.close()
    assert f"unary operation {name} is not implemented" in capfd.readouterr().err


def test_the_shim_compiles_add_unary(tmp_path):
    """include/NvInfer.h as the reference's builder uses it (block.cpp:389), compiled and run against the library: the plan holds a kEXP layer"""
    src = tmp_path / "unary.cpp"
    src.write_text('#include <cstdio>\n#include "NvInfer.h"\nusing namespace nvinfer1;\n'
                   'struct Log : ILogger { void log(Severity, const char*) noexcept override {} } gLog;\n'
                   'int main() {\n'
                   '    IBuilder* b = createInferBuilder(gLog);\n'
                   '    INetworkDefinition* n = b->createNetworkV2(1U);\n'
                   '    ITensor* x = n->addInput("x", DataType::kFLOAT, Dims4{1, 8, 4, 4});\n'
                   '    IUnaryLayer* e = n->addUnary(*x, UnaryOperation::kEXP);\n'
                   '    if (!e || e->getOutput(0)->getDimensions().d[1] != 8) return 2;\n'
                   '    e->getOutput(0)->setName("y");\n'
                   '    n->markOutput(*e->getOutput(0));\n'
                   '    IBuilderConfig* c = b->createBuilderConfig();\n'
                   '    IHostMemory* m = b->buildSerializedNetwork(*n, *c);\n'
                   '    if (!m || m->size() == 0) return 3;\n'
                   '    std::printf("%zu\\n", (size_t)m->size());\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "unary"
    libdir = os.path.dirname(capi.lib_path())
    cmd = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-ltrtx_hip", f"-Wl,-rpath,{libdir}"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert int(out) > 0


# ---- the lowering ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans():
    cache = {}

    def get(case, fp16):
        if (case.name, fp16) not in cache:
            cache[(case.name, fp16)] = lc.build_plan(case, fp16)
        return cache[(case.name, fp16)]
    return get


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_plan_lowers_to_the_intended_ops(case, fp16, plans):
    desc = engine.describe_plan(plans(case, fp16), lowered=True)
    kinds = {o["kind"] for o in desc["ops"]}
    assert case.kinds_for(fp16) <= kinds, (sorted(kinds), case.kinds_for(fp16))
    assert not case.absent_for(fp16) & kinds, sorted(kinds)
    if case.inst:
        kind, want32, want16 = case.inst
        got = [i.split()[-1] for k, _, i in instantiations(desc, fp16) if k == kind]
        assert got and got[-1] == (want16 if fp16 else want32), (kind, got)


@pytest.mark.parametrize("fp16", [0, 1])
def test_exp_is_one_activation_op_in_the_layout_of_its_input(fp16, plans):
    for case in yc.EXP_CASES:
        acts = [o for o in _ops(plans(case, fp16)) if o["kind"] in ("act_nhwc", "act_lin")]
        assert [o["act"] for o in acts] == [yc.ACT_EXP], case.name
        assert acts[0]["kind"] == ("act_nhwc" if case.family == "exp_nhwc" else "act_lin")


@pytest.mark.parametrize("fp16", [0, 1])
def test_a_lone_softmax_chain_is_exactly_one_softmax_op(fp16, plans):
    for case in yc.CHAIN_CASES:
        ops = _ops(plans(case, fp16))
        assert [o["kind"] for o in ops] == ["softmax"], (case.name, [o["kind"] for o in ops])
        assert "max / sub / exp / sum / div" in ops[0]["name"]
    for case in yc.CHAIN_NEAR_MISSES:      # one broken condition each: every layer of the chain is an op of its own
        kinds = [o["kind"] for o in _ops(plans(case, fp16))]
        assert kinds.count("reduce_lin") == 2 and kinds.count("ew_lin") == 2 and "softmax" not in kinds, (case.name, kinds)
        assert [o["act"] for o in _ops(plans(case, fp16)) if o["kind"] == "act_lin"][0] == yc.ACT_EXP


@pytest.mark.parametrize("fp16", [0, 1])
def test_gated_add_is_one_op_and_its_switch_brings_the_generic_ops_back(fp16, plans, monkeypatch):
    v = 8 if fp16 else 4
    for case in yc.GATED_CASES:
        desc = engine.describe_plan(plans(case, fp16), lowered=True)
        kinds = [o["kind"] for o in desc["ops"]]
        assert kinds.count("gated_add") == 1 and "ew_lin" not in kinds and "ew_nhwc" not in kinds, (case.name, kinds)
        assert kinds.count("to_nhwc") == len(case.inputs) and kinds.count("to_linear") == 1     # the only layout passes are those of the bindings
        (op,) = [o for o in desc["ops"] if o["kind"] == "gated_add"]
        C = desc["tensors"][op["out"][0]]["dims"][-3]
        aligned = "concat12" not in case.name or not fp16                  # channel offset 12: 24 bytes in fp16, 48 in fp32
        assert _is_vec(desc, op, fp16) == (C % v == 0 and aligned), case.name
        if "concat" in case.name:                                         # it writes into the concat's buffer at that buffer's pixel stride: no copy
            to = desc["tensors"][op["out"][0]]
            assert "copy_nhwc" not in kinds and to["view"] and to["coff"] == (16 if "concat16" in case.name else 12) and to["ld"] >= to["coff"] + C
    monkeypatch.setenv("TRTX_GATED_ADD", "0")
    for case in yc.GATED_CASES:
        kinds = [o["kind"] for o in _ops(plans(case, fp16))]
        assert "gated_add" not in kinds and yc.GATED_GENERIC_KINDS <= set(kinds), (case.name, kinds)
        assert kinds.count("ew_lin") == 1 and kinds.count("ew_nhwc") == 1 and kinds.count("to_linear") == 2       # the product's operand, and the output binding
    for case in yc.GATED_GENERIC:
        assert case.kinds_for(fp16) <= {o["kind"] for o in _ops(plans(case, fp16))}
    monkeypatch.delenv("TRTX_GATED_ADD")
    for case in yc.GATED_NEAR_MISSES:
        kinds = [o["kind"] for o in _ops(plans(case, fp16))]
        assert "gated_add" not in kinds and "ew_nhwc" in kinds, (case.name, kinds)


def test_a_gated_add_behind_a_convolution_is_not_taken_as_that_convolutions_residual():
    """FullPad_Tunnel's first operand is usually a convolution's output with the sum as its only reader: the sum belongs to the gated add (one op that
    reads the product's operand in place), not to the convolution's residual epilogue behind a product on the LINEAR path"""
    rng = np.random.default_rng(5)
    net = builder.Network(fp16=True, explicit_batch=True)
    try:
        x, b = net.input("x", (2, 16, 6, 6)), net.input("b", (2, 16, 6, 6))
        a = net.out(net.conv(x, rng.standard_normal((16, 16, 3, 3)).astype(np.float32) * 0.1, None, 1, 1))
        _, y = yc.gated_add(net, a, lc.nhwc(net, b), np.float32([0.37]), True)
        net.mark_output(y, "y")
        ops = _ops(net.build())
    finally:
        net.close()
    kinds = [o["kind"] for o in ops]
    assert kinds.count("gated_add") == 1 and "ew_lin" not in kinds and "ew_nhwc" not in kinds, kinds
    assert not [o for o in ops if o["kind"] == "conv" and o["residual"]]


# ---- the interpreter against the fp64 references ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_interpreter_matches_the_fp64_reference(case, plans):
    plan = plans(case, 0)
    inputs = lc.gen_inputs(case)
    for fp16 in (0, 1):
        for name, outs in lc.outs_of(case, lc.ref_inputs(case, inputs, fp16), fp16).items():
            for o in outs:
                assert torch.isfinite(o.ref).all() and o.ref.abs().max() <= lc.F16_MAX, name     # every result fits fp16
                if o.mag is not None:
                    assert (o.mag >= o.ref.abs() * (1 - 1e-12)).all(), name
    desc, plan2 = yc.exp_as_pow(engine.describe_plan(plan), plan)
    assert not [l for l in desc["layers"] if l["kind"] == yc.L_UNARY]
    got = gi.run(desc, plan2, inputs, batch=case.batch)
    for name, outs in lc.outs_of(case, lc.ref_inputs(case, inputs, 0), 0).items():
        g = got[name].double()
        for o in outs:
            part = g if o.ch is None else g[:, o.ch]
            assert part.shape == o.ref.shape, (name, part.shape, o.ref.shape)
            if o.mag is None:
                assert torch.equal(part, o.ref), name
            else:
                err = (part - o.ref).abs()
                assert (err <= lc.fp32_bound(o)).all(), (name, (err / lc.fp32_bound(o)).max().item())


def test_the_gates_of_the_cases_are_neither_0_nor_1():
    for case in yc.GATED_CASES:
        plan = lc.build_plan(case, 0)
        desc = engine.describe_plan(plan)
        (c,) = [l for l in desc["layers"] if l["kind"] == gi.L_CONSTANT]
        g = np.frombuffer(plan, np.float32, c["w"][0][1], c["w"][0][0])
        assert g.size in (1, desc["tensors"][c["outputs"][0]]["dims"][-3]) and (np.abs(g) >= 0.2).all() and (np.abs(g) <= 0.8).all()


def test_new_cases_leave_the_layer_table_alone():
    names = [c.name for c in lc.CASES]
    assert not set(names) & set(IDS) and len(set(IDS)) == len(IDS)
    assert dataclasses.is_dataclass(lc.Case)


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-q"]))
