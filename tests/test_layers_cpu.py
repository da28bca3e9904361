"""The layer conformance table (tests/layer_cases.py) on the host: every case's plan builds and lowers to the op kinds it is meant to
exercise, takes the kernel instantiation it is meant to take, and the oracle's fp32 interpreter of the unlowered graph agrees with the
case's own fp64 reference - so that a failure of tests/test_gpu_layers.py points at the lowering or at a kernel.

Instantiations are derived from describe_plan(lowered=True), restating the launchers' dispatch conditions:
  * pool / resize / ew_nhwc / act_nhwc / scale_nhwc / copy_nhwc: can_vec() (kernels/nhwc_ops.hip:445-453) - C % v == 0, every ld % v == 0
    and every pointer 16-byte aligned, v = 8 (fp16) / 4 (fp32).  The base address of a storage is not part of the description (the arena
    hands out offsets at 256-byte granularity); what is visible, and asserted, is the channel offset of the view: coff % v == 0;
  * to_nhwc: nchw_f32_to_nhwc() (nhwc_ops.hip:466-482) - the tiled fp16 kernel iff fp16, ld % 8 == 0, C >= 16 (and an aligned view);
  * reduce_hw: nhwc_reduce_hw_avg() (nhwc_ops.hip:606-619) - the x8 kernel iff fp16 and can_vec(), one scalar kernel per type otherwise;
  * pool_chain: x8 (fp16) / x4 (fp32) only (nhwc_ops.hip:508-521); depth_to_space: fp16 x8 only (nhwc_ops.hip:542-549);
  * conv / deconv with igemm, dw and stem false: conv_direct() / deconv_direct() (nhwc_ops.hip:621-637), one kernel per type;
  * the LINEAR kernels have one fp32 instantiation each (kernels/linear_ops.hip:174-226)."""
import collections

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from tensorrtx_amd import builder, engine
from tests import layer_cases as lc

IDS = [c.name for c in lc.CASES]
LINEAR_KERNELS = {"gather": "gather_kernel", "scatter": "scatter_kernel", "ew_lin": "ew_kernel", "act_lin": "act_kernel", "softmax": "softmax_kernel",
                  "matmul": "matmul_kernel", "reduce_lin": "reduce_kernel", "scale_lin": "scale_kernel(linear)"}
VEC_KERNELS = {"pool": "pool_kernel", "resize": "resize_nearest_kernel", "ew_nhwc": "elementwise_kernel", "act_nhwc": "activation_kernel",
               "scale_nhwc": "scale_kernel", "copy_nhwc": "copy_kernel"}
REQUIRED = ([(k, i) for k in VEC_KERNELS.values() for i in ("f16 x8", "f16 x1", "f32 x4", "f32 x1")]
            + [("nchw_to_nhwc_f16_tiled_kernel", "f16"), ("nchw_to_nhwc_kernel", "f16"), ("nchw_to_nhwc_kernel", "f32"), ("nhwc_to_nchw_kernel", "f16"),
               ("nhwc_to_nchw_kernel", "f32"), ("reduce_hw_avg_f16x8_kernel", "f16 x8"), ("reduce_hw_avg_kernel", "f16 x1"), ("reduce_hw_avg_kernel", "f32 x1"),
               ("maxpool_chain3_kernel", "f16 x8"), ("maxpool_chain3_kernel", "f32 x4"), ("depth_to_space_f16_kernel", "f16 x8"), ("conv_direct_kernel", "f16"),
               ("conv_direct_kernel", "f32"), ("deconv_direct_kernel", "f16"), ("deconv_direct_kernel", "f32")]
            + [(k, "f32") for k in LINEAR_KERNELS.values()])


def _is_vec(desc, op, fp16):
    v = 8 if fp16 else 4
    T = desc["tensors"]
    ts = [T[i] for i in op["in"] + op["out"] if T[i]["layout"] == "nhwc"]
    return T[op["in"][0]]["dims"][-3] % v == 0 and all(t["ld"] % v == 0 and t["coff"] % v == 0 for t in ts)


def instantiations(desc, fp16):
    """[(op kind, kernel, instantiation)] of a lowered plan"""
    ty = "f16" if fp16 else "f32"
    out = []
    for op in desc["ops"]:
        k = op["kind"]
        T = desc["tensors"]
        if k in VEC_KERNELS:
            out.append((k, VEC_KERNELS[k], f"{ty} x{(8 if fp16 else 4) if _is_vec(desc, op, fp16) else 1}"))
        elif k == "to_nhwc":
            to = T[op["out"][0]]
            tiled = fp16 and to["ld"] % 8 == 0 and to["coff"] % 8 == 0 and to["dims"][-3] >= 16
            out.append((k, "nchw_to_nhwc_f16_tiled_kernel" if tiled else "nchw_to_nhwc_kernel", ty))
        elif k == "to_linear":
            out.append((k, "nhwc_to_nchw_kernel", ty))
        elif k == "reduce_hw":
            x8 = fp16 and _is_vec(desc, op, fp16)
            out.append((k, "reduce_hw_avg_f16x8_kernel" if x8 else "reduce_hw_avg_kernel", f"{ty} x{8 if x8 else 1}"))
        elif k == "pool_chain":
            assert _is_vec(desc, op, fp16)
            out.append((k, "maxpool_chain3_kernel", f"{ty} x{8 if fp16 else 4}"))
        elif k == "depth_to_space":
            assert fp16 and _is_vec(desc, op, fp16)
            out.append((k, "depth_to_space_f16_kernel", "f16 x8"))
        elif k in ("conv", "deconv") and not (op["igemm"] or op["stem"] or op.get("dw")):
            out.append((k, k + "_direct_kernel", ty))
        elif k in LINEAR_KERNELS:
            out.append((k, LINEAR_KERNELS[k], "f32"))
    return out


@pytest.fixture(scope="module")
def plans():
    cache = {}

    def get(case, fp16):
        if (case.name, fp16) not in cache:
            cache[(case.name, fp16)] = lc.build_plan(case, fp16)
        return cache[(case.name, fp16)]
    return get


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_plan_lowers_to_the_intended_kernels(case, fp16, plans):
    desc = engine.describe_plan(plans(case, fp16), lowered=True)
    kinds = {o["kind"] for o in desc["ops"]}
    assert case.kinds_for(fp16) <= kinds, (sorted(kinds), case.kinds_for(fp16))
    assert not case.absent_for(fp16) & kinds, sorted(kinds)
    convs = [o for o in desc["ops"] if o["kind"] in ("conv", "deconv")]
    if case.direct:
        assert convs and not any(o["igemm"] or o["stem"] or o.get("dw") for o in convs)
    if case.igemm:
        assert convs and convs[-1]["igemm"] and not convs[-1]["stem"], convs[-1]
    if case.stem:
        assert convs and convs[-1]["stem"], convs[-1]
    if case.fused:
        (o,) = convs
        assert {k: o[k] for k in case.fused} == case.fused   # bias, activation, shortcut and second activation live in the one conv op
    if case.inst:
        kind, want32, want16 = case.inst
        got = [i.split()[-1] for k, _, i in instantiations(desc, fp16) if k == kind]
        assert got and got[-1] == (want16 if fp16 else want32), (kind, got)   # the last op of the kind: the one under test (helpers come first)


def test_every_kernel_instantiation_is_reached(plans):
    table = collections.Counter()
    for case in lc.CASES:
        for fp16 in (0, 1):
            for _, kernel, inst in set(instantiations(engine.describe_plan(plans(case, fp16), lowered=True), fp16)):
                table[(kernel, inst)] += 1
    empty = [cell for cell in REQUIRED if table[cell] == 0]
    print("\n".join(f"{k:34s} {i:8s} {n}" for (k, i), n in sorted(table.items())))
    assert not empty, empty


def test_the_table_covers_the_common_axes():
    """per family: a batch-1 enqueue on a max_batch-3 plan and a work count above one grid (2048 blocks of 256 threads).  pool_chain and
    reduce_hw launch one workgroup per (image, channel chunk) and have no grid-stride loop; fc is a convolution"""
    for fam in {c.family for c in lc.CASES} - {"fc", "pool_chain"}:
        names = [c.name for c in lc.CASES if c.family == fam]
        assert any(c.family == fam and c.batch == 1 and c.max_batch == 3 for c in lc.CASES), fam
        assert fam == "reduce_hw" or any(n.endswith("_big") for n in names), fam


@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_interpreter_matches_the_fp64_reference(case, plans):
    """oracle.graph_interp (fp32 torch on the unlowered layer list) against the case's own fp64 reference, and the conditioning of that reference"""
    plan = plans(case, 0)
    inputs = lc.gen_inputs(case)
    for fp16 in (0, 1):
        x = lc.ref_inputs(case, inputs, fp16)
        if case.cond:
            case.cond(x)
        for name, outs in lc.outs_of(case, x, fp16).items():
            for o in outs:
                assert torch.isfinite(o.ref).all() and o.ref.abs().max() <= lc.F16_MAX, name   # every result fits fp16
                if o.mag is not None:
                    assert (o.mag >= o.ref.abs() * (1 - 1e-12)).all(), name   # the magnitude bounds the value it belongs to
    got = gi.run(engine.describe_plan(plan), plan, inputs, batch=case.batch)
    for name, outs in lc.outs_of(case, lc.ref_inputs(case, inputs, 0), 0).items():
        g = got[name].double()
        for o in outs:
            part = g if o.ch is None else g[:, o.ch]
            assert part.shape == o.ref.shape, (name, part.shape, o.ref.shape)
            if o.mag is None:
                assert torch.equal(part, o.ref), name
            else:
                err = (part - o.ref).abs()
                assert (err <= lc.fp32_bound(o)).all(), (name, (err - lc.fp32_bound(o)).max().item())


def test_matmul_with_three_broadcast_patterns_is_refused_at_build_time(capfd):
    """the lowering merges the leading dims of a matmul into at most two (outer, inner) runs per operand; a third pattern is unsupported by
    design and must be refused with a message, not run wrongly"""
    net = builder.Network(explicit_batch=True)
    try:
        y = net.out(net.matmul(net.input("a", (2, 3, 2, 5, 7)), net.input("b", (2, 1, 2, 7, 4))))
        net.mark_output(y, "y")
        with pytest.raises(Exception, match="unsupported"):
            net.build()
    finally:
        net.close()
    assert "matmul with more than two independent broadcast patterns in its leading dims" in capfd.readouterr().err


def test_grouped_deconvolution_builds():
    """Network.conv(deconv=True, groups=g) takes CKRS weights with K = Cout / g: nb_out is K * g"""
    net = builder.Network()
    try:
        x = net.input("x", (6, 5, 5))
        y = net.out(net.conv(x, np.ones((6, 2, 4, 4), np.float32), None, 2, 1, deconv=True, groups=2))
        net.mark_output(y, "y")
        desc = engine.describe_plan(net.build())
    finally:
        net.close()
    assert [t["dims"] for t in desc["tensors"] if t["is_output"]] == [[4, 10, 10]]
