"""Small networks for the pieces of YOLOv13 that the runtime has beyond YOLOv12's: IUnaryLayer kEXP (AAttn's spelled-out softmax,
yolov13/src/block.cpp:384-394), that softmax chain standing alone, and the gated add a + gate * b of FullPad_Tunnel (block.cpp:889-900) and of
A2C2f's gamma residual (block.cpp:473-484).  Shared by tests/test_yolov13_cpu.py (plans, the interpreter) and tests/test_gpu_yolov13.py (engines).

The cases are tests/layer_cases.py `Case` records - same fields, same error model, same checker - kept in a list of their own: the layer table
stays what it is.

Error model of the new ops (per element, on inputs already rounded to the engine's storage type):
  * exp: the accurate expf in fp32 (covered by the 1e-5 relative term of layer_cases.fp32_bound), one fp16 store on the NHWC path (1 site);
  * the softmax chain lowers to the softmax op: layer_cases' softmax model (n = the axis length, U32 * |x - max| from the rounded subtraction);
  * gated add: one fp32 product, one fp32 sum (n = 2 terms of magnitude |a| + |gate b|), one rounding to the storage type (1 site).  The gate is
    an fp32 weight in both engines: no site."""
import copy
import zlib

import numpy as np
import torch

from oracle import graph_interp as gi
from tests import layer_cases as lc
from tests.layer_cases import Out, U32, nhwc, select_conv

L_UNARY = 18       # runtime/graph.h: appended after L_IDENTITY
ACT_EXP = 8        # kernels/kernels.h
E32 = np.float32(np.e)


def _own(fn, *a, **kw):
    """a case built by a layer_cases constructor, taken back out of its table"""
    c = fn(*a, **kw)
    lc.CASES.remove(c)
    return c


# ---- the interpreter does not know the unary kind: hand it an equivalent description -------------------------------------------------------
def exp_as_pow(desc, plan):
    """(desc', plan'): every kEXP layer becomes kPOW(e, x), e a one-element constant whose value is appended to a copy of the plan bytes"""
    d = copy.deepcopy(desc)
    plan = bytes(plan) + b"\0" * (-len(plan) % 16)
    layers = []
    for l in d["layers"]:
        if l["kind"] != L_UNARY:
            layers.append(l)
            continue
        assert l["op"] == 0, "only kEXP has an equivalent here"
        rank = len(d["tensors"][l["inputs"][0]]["dims"])
        tid = len(d["tensors"])
        d["tensors"].append({"id": tid, "name": f"e:{l['name']}", "dims": [1] * rank, "is_input": False, "is_output": False})
        c = copy.deepcopy(l)
        c.update(kind=gi.L_CONSTANT, name=f"e:{l['name']}", inputs=[], outputs=[tid], out_dims=[1] * rank, w=[[len(plan), 1], [0, 0], [0, 0]])
        plan += E32.tobytes() + b"\0" * 12
        layers.append(c)
        l.update(kind=gi.L_ELEMENTWISE, op=6, inputs=[tid, l["inputs"][0]])
        layers.append(l)
    d["layers"] = layers
    return d, plan


# ---- 1. exp --------------------------------------------------------------------------------------------------------------------------------
EXP_SPECIAL = [0.0, 11.0, -11.0, -17.0, 1.0, -1.0, 0.5, 11.0625, -30.0, -88.0]   # e^11.0625 = 63 736 fits fp16; e^-17 and below round to 0 there


def _exp_gen(rng, shape):
    a = rng.uniform(-12.0, 11.0, shape).astype(np.float32)
    flat = a.reshape(-1)
    n = min(len(EXP_SPECIAL), flat.size)
    flat[:n] = EXP_SPECIAL[:n]
    if flat.size >= 2 * len(EXP_SPECIAL):
        flat[-len(EXP_SPECIAL):] = EXP_SPECIAL
    return a


def _exp_op(net, t, chw):
    return net.out(net.unary(t, "exp"))


def _exp_ref(sites):
    def ref(x):
        r = torch.exp(x)
        return Out(r, r, sites=sites)
    return ref


EXP_CASES = []
for C, H, W, B in ((5, 13, 17, 3), (8, 1, 9, 1), (12, 13, 17, 3), (72, 13, 17, 3)):     # fp16 x1 / x8 / x1 / x8, fp32 x1 / x4 / x4 / x4
    EXP_CASES.append(_own(lc.unary_nhwc, f"exp_nhwc_c{C}_{H}x{W}_b{B}", "exp_nhwc", C, H, W, B, _exp_op, _exp_ref(1), "act_nhwc", gen=_exp_gen, via_pool=True,
                          kinds={"act_nhwc", "pool"}, absent={"act_lin"}))
for wrap in ("slice", "concat"):
    EXP_CASES.append(_own(lc.unary_nhwc, f"exp_nhwc_c8_13x17_b3_{wrap}", "exp_nhwc", 8, 13, 17, 3, _exp_op, _exp_ref(1), "act_nhwc", gen=_exp_gen, via_pool=True,
                          wrap=wrap, kinds={"act_nhwc", "pool"}, absent={"act_lin"}))
EXP_CASES.append(_own(lc.unary_nhwc, "exp_nhwc_c12_13x17_b1_of3", "exp_nhwc", 12, 13, 17, 1, _exp_op, _exp_ref(1), "act_nhwc", gen=_exp_gen, via_pool=True,
                      max_batch=3, kinds={"act_nhwc", "pool"}))
EXP_CASES.append(_own(lc.unary_nhwc, "exp_nhwc_c12_128x128_b3_big", "exp_nhwc", 12, 128, 128, 3, _exp_op, _exp_ref(1), "act_nhwc", gen=_exp_gen, via_pool=True,
                      kinds={"act_nhwc", "pool"}))      # 589 824 items on the fp16 scalar path: the grid-stride loop iterates
for dims, B, mb in (((5, 13, 17), 3, 3), ((7,), 1, 1), ((3, 4, 5, 6), 2, 2), ((5, 13, 17), 1, 3)):
    EXP_CASES.append(lc.Case(name=f"exp_lin_{'x'.join(map(str, dims))}_b{B}_of{mb}", family="exp_lin", inputs={"x": (dims, _exp_gen)},
                             build=lambda net, t: {"y": net.out(net.unary(t["x"], "exp"))}, ref=lambda x: {"y": _exp_ref(0)(x["x"])},
                             kinds={"act_lin"}, absent={"act_nhwc"}, half=(), batch=B, max_batch=mb))


# ---- 2. the spelled-out softmax ------------------------------------------------------------------------------------------------------------
def softmax_chain(net, x, ax_max, ax_sum=None, extra_reader=False):
    """block.cpp:384-394 on tensor x: reduce-max (keepDims), sub, exp, reduce-sum (keepDims), div -> {output name: tensor id}"""
    ax_sum = ax_max if ax_sum is None else ax_sum
    m = net.out(net.reduce(x, "max", 1 << ax_max, True))
    e = net.out(net.unary(net.out(net.elementwise(x, m, "sub")), "exp"))
    s = net.out(net.reduce(e, "sum", 1 << ax_sum, True))
    outs = {"y": net.out(net.elementwise(e, s, "div"))}
    if extra_reader:
        outs["e"] = net.out(net.activation(e, "relu"))    # e >= 0: the same values, read a second time
    return outs


def _chain_ref(dims, ax_max, ax_sum=None, extra_reader=False):
    ax_sum = ax_max if ax_sum is None else ax_sum

    def ref(x):
        v = x["x"]
        spread = (v - v.amax(ax_max + 1, keepdim=True)).abs()
        e = torch.exp(v - v.amax(ax_max + 1, keepdim=True))
        r = e / e.sum(ax_sum + 1, keepdim=True)
        outs = {"y": Out(r, r, n=dims[ax_sum], amp=U32 * spread)}
        if extra_reader:
            outs["e"] = Out(e, e, amp=U32 * spread)
        return outs
    return ref


def _chain_case(dims, B, ax, gen="logits", ax_sum=None, extra_reader=False, max_batch=None, tag=""):
    fused = ax_sum is None and not extra_reader
    generic = {"reduce_lin", "ew_lin", "act_lin"}
    return lc.Case(name=f"softmax_chain_{'x'.join(map(str, dims))}_ax{ax}_{gen}_b{B}{tag}", family="softmax_chain", inputs={"x": (dims, gen)},
                   build=lambda net, t: softmax_chain(net, t["x"], ax, ax_sum, extra_reader), ref=_chain_ref(dims, ax, ax_sum, extra_reader),
                   kinds={"softmax"} if fused else generic, absent=generic if fused else {"softmax"}, half=(), batch=B, max_batch=max_batch)


CHAIN_CASES = [_chain_case(dims, 2, ax) for dims in ((16, 5), (2, 80, 3), (2, 3, 16, 2)) for ax in range(len(dims))]
CHAIN_CASES += [_chain_case((4, 25, 25), 3, 2), _chain_case((6, 80), 3, 1, gen="logits80"), _chain_case((6, 80), 3, 1, gen="equal"),
                _chain_case((6, 80), 1, 1, max_batch=3, tag="_of3"), _chain_case((2, 450, 450), 3, 2, tag="_big")]
CHAIN_NEAR_MISSES = [_chain_case((4, 6, 9), 2, 2, ax_sum=1, tag="_sum_over_another_axis"), _chain_case((4, 6, 9), 2, 2, extra_reader=True, tag="_exp_read_twice")]


# ---- 3. gated add --------------------------------------------------------------------------------------------------------------------------
def _gate(name, C, per_channel):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return (rng.uniform(0.2, 0.8, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32) if per_channel else np.float32([0.37])   # not 0, not 1


def gated_add(net, a, b, gate, explicit, order=0):
    """a + gate * b with the constant shaped as the reference shapes it; order bit 0: the product's operands swapped, bit 1: the sum's"""
    g = net.out(net.constant(gate.reshape(([1] if explicit else []) + [gate.size, 1, 1])))
    p = net.out(net.elementwise(b, g, "prod") if order & 1 else net.elementwise(g, b, "prod"))
    return p, net.out(net.elementwise(p, a, "sum") if order & 2 else net.elementwise(a, p, "sum"))


def _gated_case(C, per_channel, dest, explicit=True, order=0, B=3, H=5, W=7, max_batch=None, near=None, generic=False):
    """dest: "dense"; "concat12" / "concat16": the op writes behind a 12- / 16-channel convolution in a concat (channel offset 12: no 16-byte
    access in fp16; 16: aligned in both).  near: None, "gate2" (a two-element gate along W) "reader" (the product is read a second time) or "tokens" (a 1 x 1 map).
    generic: the case as TRTX_GATED_ADD=0 lowers it, as a near-miss does: the product is stored (fp16 in an fp16 engine) before the sum - 2 sites"""
    generic = generic or bool(near)
    name = f"gated_add_c{C}_{'chan' if per_channel else 'one'}_{dest}_{'eb' if explicit else 'ib'}_o{order}_{H}x{W}_b{B}" + (f"_of{max_batch}" if max_batch else "") + (f"_{near}" if near else "") + ("_generic" if generic and not near else "")
    gate = _gate(name, C, per_channel)
    nb = 16 if dest == "concat16" else 12
    pick = (lc.NEIGHBOUR + lc.NEIGHBOUR)[:nb]
    lead = (B,) if explicit else ()

    def build(net, t):
        a, b = nhwc(net, t["a"]), nhwc(net, t["b"])
        if near == "gate2":
            g = net.out(net.constant(np.float32([0.37, -0.61]).reshape(([1] if explicit else []) + [1, 1, 2])))
            p = net.out(net.elementwise(g, b, "prod"))
            y = net.out(net.elementwise(a, p, "sum"))
        else:
            p, y = gated_add(net, a, b, gate, explicit, order)
        outs = {}
        if near == "reader":
            outs["p"] = net.out(net.pooling(p, 1, 1))
        if dest != "dense":
            y = net.out(net.concat([select_conv(net, nhwc(net, t["z"]), 8, pick), y]))
        outs["y"] = y
        return outs

    def ref(x):
        g = torch.tensor([0.37, -0.61], dtype=torch.float64).reshape(1, 1, 1, 2) if near == "gate2" else torch.from_numpy(gate).double().reshape(1, -1, 1, 1)
        prod = g * x["b"]
        o = Out(x["a"] + prod, x["a"].abs() + prod.abs(), n=2, sites=2 if generic else 1)
        outs = {}
        if near == "reader":
            outs["p"] = Out(prod, prod.abs(), sites=1)
        if dest != "dense":
            o.ch = slice(nb, None)
            outs["y"] = [Out(x["z"][:, pick], ch=slice(0, nb)), o]
        else:
            outs["y"] = o
        return outs
    inputs = {"a": (lead + (C, H, W), "n"), "b": (lead + (C, H, W), "n")}
    if dest != "dense":
        inputs["z"] = (lead + (8, H, W), "n")
    kinds = {"pool"} | ({"ew_nhwc"} if generic else {"gated_add"}) | ({"conv"} if dest != "dense" else set())
    absent = {"gated_add"} if generic else {"ew_nhwc", "ew_lin"}
    return lc.Case(name=name, family="gated_add", inputs=inputs, build=build, ref=ref, kinds=kinds, absent=absent, batch=1 if explicit else B,
                   max_batch=None if explicit else max_batch, explicit=explicit)


GATED_CASES = [_gated_case(C, pc, dest) for C in (16, 24, 64) for pc in (False, True) for dest in ("dense", "concat12", "concat16")]
GATED_CASES += [_gated_case(16, True, "dense", order=o) for o in (1, 2, 3)]
GATED_CASES += [_gated_case(12, True, "dense"), _gated_case(5, False, "dense"),                    # no 16-byte access in fp16 / in either type
                _gated_case(16, True, "dense", explicit=False), _gated_case(16, False, "concat16", explicit=False, B=1, max_batch=3),
                _gated_case(72, True, "dense", B=4, H=128, W=128)]                                   # above one grid of 2048 x 256 lanes
GATED_NEAR_MISSES = [_gated_case(16, False, "dense", W=2, near="gate2"), _gated_case(16, True, "dense", near="reader"),
                     _gated_case(16, False, "dense", H=1, W=1, near="tokens")]      # a 1 x 1 map is a token matrix: it keeps its element-wise ops

# the switch-off route (TRTX_GATED_ADD=0) of the first cases: the broadcast product on the LINEAR path (two layout passes), the sum on NHWC
GATED_GENERIC = [_gated_case(C, pc, dest, generic=True) for C, pc, dest in ((16, False, "dense"), (24, True, "concat12"), (64, True, "concat16"))]
GATED_GENERIC_KINDS = {"to_linear", "ew_lin", "to_nhwc", "ew_nhwc"}
