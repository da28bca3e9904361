"""YOLOv13's hypergraph convolution without a GPU (tests/hgconv_cases.py): the table covers what it claims, its inputs are conditioned, the NumPy fp32
emulation of the kernel's folded order lies within the derived bound on every case while eight restated bugs leave it, the subgraph lowers to one
`hgconv` op (and near-misses do not), the oracle's interpreter agrees with the table's reference, and the C entry refuses bad arguments on the host."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from tensorrtx_amd import capi, engine
from tests import hgconv_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC = {"matmul", "softmax", "reduce_lin", "gather", "scatter", "copy_nhwc", "copy_lin"}
NOT_TIED = [c for c in hc.CASES if c.data != "tied"]


# ---- coverage -------------------------------------------------------------------------------------------------------------------------------------------
def test_table_covers_the_axes_and_every_tile_edge():
    assert len(set(hc.IDS)) == len(hc.CASES)
    tiles = capi.hgconv_geometry()
    assert tuple(tiles) == hc.TILES, "the table's node maps were chosen for these tile sizes"
    nodes = {c.H * c.W for c in hc.CASES}
    for T in tiles:
        assert {T - 1, T, T + 1, 2 * T + 1} <= nodes, T
    assert {1, 35, 64, 65, 400, 1600} <= nodes
    assert {(c.D, c.E) for c in hc.CASES} == set(hc.MODEL_DE + hc.OFF_MODEL_DE)
    assert {c.B for c in hc.CASES} == {1, 3}
    assert {c.data for c in hc.CASES} == set(hc.DATA)
    assert any(c.B == 3 and c.data == "ctx" for c in hc.CASES)
    for c in hc.CASES:      # small: the whole table is a few seconds on the device
        assert c.B * c.H * c.W * c.D <= 1600 * 384 * 1, c.name
        if c.data in ("rising", "falling"):
            assert (c.H * c.W) > 2 * tiles[1]      # at least three tiles: the running maximum moves inside a tile and between tiles
        if c.data == "negative":
            assert (c.H * c.W) % tiles[0]          # a partial sub-tile: rows a careless kernel would zero-fill
    for D, E in hc.MODEL_DE + hc.OFF_MODEL_DE:
        assert capi.hgconv_workspace_bytes(3, 35, D, E) > 0
    for D, E in [(24, 4), (400, 4), (64, 0), (64, 17), (0, 4)]:
        assert capi.hgconv_workspace_bytes(3, 35, D, E) == 0
    # a pure function of (B, N, D, E): the same number again, growing with each of the four
    base = capi.hgconv_workspace_bytes(3, 257, 128, 8)
    assert base == capi.hgconv_workspace_bytes(3, 257, 128, 8) and base % 256 == 0
    assert all(capi.hgconv_workspace_bytes(*a) > base for a in [(4, 257, 128, 8), (3, 400, 128, 8), (3, 257, 144, 8), (3, 257, 128, 9)])


# ---- the special data is what it is said to be ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in hc.CASES if c.data != "gauss"])
def test_data_has_the_stated_shape(name):
    c = hc.BY_NAME[name]
    ref = hc.reference(name)
    x, w = hc.gen(name)
    N = c.H * c.W
    lg = ref.logits
    if c.data == "large":
        assert lg.max().item() > 100
    elif c.data == "tied":
        assert torch.allclose(ref.A, torch.full_like(ref.A, 1.0 / N), rtol=1e-12, atol=0) and np.abs(w["b_pre"]).max() > 0.5
    elif c.data == "dominant":
        top = ref.A.max(1)
        assert (top.values > 0.99).all() and (top.indices == torch.tensor([17 * e + 3 for e in range(c.E)])[None]).all()
    elif c.data == "rising":
        assert (lg[:, 1:] > lg[:, :-1]).all() and (lg[:, -1] - lg[:, 0]).min().item() > 40
    elif c.data == "falling":
        assert (lg[:, 1:] < lg[:, :-1]).all() and (lg[:, 0] - lg[:, -1]).min().item() > 40
    elif c.data == "negative":
        assert x.max().item() < 0
    elif c.data == "ctx":
        m = x.double().mean((1, 2))
        assert abs(m[0].item()) < 0.2 and abs(m[1].item() - 2) < 0.2 and abs(m[2].item() + 2) < 0.2
        P = [ref.A[b] for b in range(c.B)]
        assert not torch.allclose(P[0], P[1], atol=1e-3)
    elif c.data == "bpre":      # b_pre (here 100 x) is constant over the nodes: the same result without it, to fp64 round-off
        w0 = dict(w, b_pre=np.zeros_like(w["b_pre"]))
        assert np.abs(w["b_pre"]).max() > 100
        ref0 = hc.reference_of(x, w0, c.D, c.E)
        assert (ref0.out - ref.out).abs().max().item() < 1e-9 * max(1.0, ref.out.abs().max().item())


# ---- conditioning: a condition on the inputs, not a tolerance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in NOT_TIED if c.H * c.W >= 16])
def test_inputs_are_conditioned(name):
    """Some hyperedge's largest participation is at least 4 / N (A is not near-uniform), and out - X is not negligible against the bound: its median
    magnitude is at least 5 x the median bound, so a wrong A, He or G moves the output by far more than the bound allows"""
    c = hc.BY_NAME[name]
    ref = hc.reference(name)
    N = c.H * c.W
    peak = ref.A.max(1).values.max().item()
    ratio = (ref.delta.abs().median() / ref.bound.median()).item()
    print(f"{name}: largest participation {peak:.4f} = {peak * N:.1f} / N, median |out - X| / median bound {ratio:.0f}")
    assert peak >= 4.0 / N
    assert ratio >= 5


# ---- the bound -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.IDS)
def test_emulation_within_the_bound(name):
    ref = hc.reference(name)
    got = hc.emulate(name)
    err = (got.double() - ref.out).abs()
    print(f"{name}: max err {err.max().item():.3e}, max err / bound {(err / ref.bound).max().item():.3f}, "
          f"fp16 rounding share of the bound (median) {(hc.U16 * ref.out.abs() / ref.bound).median().item():.2f}")
    assert torch.isfinite(got).all() and torch.isfinite(ref.bound).all()
    assert (err <= ref.bound).all(), ((err / ref.bound).max().item(), int((err > ref.bound).sum()))


def _caught(bug, cases):
    caught = []
    for c in cases:
        ref = hc.reference(c.name)
        got = hc.emulate(c.name, bug).double()
        if not torch.isfinite(got).all() or ((got - ref.out).abs() > ref.bound).any():
            caught.append(c.name)
    return caught


SMALL = [c for c in hc.CASES if c.B * c.H * c.W * c.D <= 3 * 257 * 128]


@pytest.mark.parametrize("bug", hc.BUGS)
def test_restated_bug_leaves_the_bound(bug):
    caught = _caught(bug, SMALL)
    print(f"{bug}: caught on {len(caught)} of {len(SMALL)} cases")
    assert caught, bug
    names = set(caught)
    if bug == "pad_max":       # the all-negative cases are the ones that show a zero fill in the column maximum
        assert names >= {c.name for c in SMALL if c.data == "negative"}
    if bug in ("pad_max", "pad_sum"):   # whole tiles: nothing is padded, the mutation changes nothing
        T = hc.TILES[0] if bug == "pad_max" else hc.TILES[1]
        assert not names & {c.name for c in SMALL if (c.H * c.W) % T == 0}
    if bug in ("no_residual", "swap_ctx", "no_heads"):
        assert len(caught) >= len(SMALL) // 2


# ---- lowering ------------------------------------------------------------------------------------------------------------------------------------------------
def _net(B, D, E, H, W, seed=0, **kw):
    c = hc._c(D, E, (5, 7), 3) if (D, E) in set(hc.MODEL_DE + hc.OFF_MODEL_DE) else None
    if c is not None:
        _, w = hc.gen(c.name)
    else:       # an off-table width (the D = 24 near-miss): weights of the right shapes
        rng = np.random.default_rng(seed)
        shapes = {"w_ctx": (E * D, 2 * D), "b_ctx": (E * D,), "proto": (E, D), "w_pre": (D, D), "b_pre": (D,), "w_edge": (D, D), "b_edge": (D,),
                  "w_node": (D, D), "b_node": (D,)}
        w = {k: (rng.standard_normal(s) / 8).astype(np.float32) for k, s in shapes.items()}
    return hc.subgraph_net(B, D, E, H, W, w, hc.c3ah_weights(D, seed=seed), **kw)


def _ops(plan):
    return engine.describe_plan(plan, lowered=True)["ops"]


def _kinds(plan):
    """op kinds with the members of a grouped convolution launch counted as the convolutions they are"""
    out = []
    for o in _ops(plan):
        out += ["conv"] * len(o["members"]) if o["kind"] == "conv_group" else [o["kind"]]
    return out


@pytest.mark.parametrize("spelling,B", [("a", 1), ("a", 3), ("b", 1)])
def test_subgraph_lowers_to_conv_conv_hgconv_conv(spelling, B):
    """cv1, cv2, the hypergraph convolution, cv3 - and nothing else but the layout pass of the fp32 output binding (every network output is a linear
    fp32 tensor; the 3-channel input is read by the two stem convolutions directly)"""
    plan = _net(B, 64, 4, 6, 7, spelling=spelling)
    ops = _ops(plan)
    kinds = _kinds(plan)
    assert kinds == ["conv", "conv", "hgconv", "conv", "to_linear"], kinds
    assert ops[-1]["name"].endswith("y") or "y" in ops[-1]["name"]
    (hg,) = [o for o in ops if o["kind"] == "hgconv"]
    assert (hg["n"], hg["d"], hg["e"]) == (42, 64, 4)
    assert hg["logit_scale"] == pytest.approx(1.0 / (4 * 4.0), rel=1e-6)          # heads = 4, scaling = sqrt(16)
    assert hg["ws_bytes"] == capi.hgconv_workspace_bytes(B, 42, 64, 4) > 0
    assert hg["ld"] == [64, 128], "reads cv1's tensor in place, writes its slice of the concat that feeds cv3"
    assert hg["flops"] > 0 and hg["bytes"] > 0


@pytest.mark.parametrize("D,E", [(128, 8), (384, 12)])
def test_wider_subgraphs_lower_to_one_op(D, E):
    kinds = collections.Counter(_kinds(_net(3, D, E, 6, 6)))
    assert kinds["hgconv"] == 1 and kinds["conv"] == 3 and not set(kinds) & GENERIC, kinds


MISSES = ["softmax_e", "gelu_const", "mean_only", "a_output", "he_reader", "b_at_2", "fp32", "option", "d24"]


@pytest.mark.parametrize("miss", MISSES)
def test_near_miss_graphs_lower_generically(miss, monkeypatch):
    """One matcher condition broken at a time: no hgconv op, and the network still builds and lowers on the generic path"""
    kw = dict(miss=miss) if miss in ("softmax_e", "gelu_const", "mean_only", "a_output", "he_reader") else {}
    B, D, E = 2, 64, 4
    if miss == "b_at_2":
        kw["spelling"] = "b2"
    elif miss == "fp32":
        kw["fp16"] = False
    elif miss == "d24":
        D = 24
    plan = _net(B, D, E, 5, 6, **kw)
    if miss == "option":
        assert "hgconv" in _kinds(plan)
        monkeypatch.setenv("TRTX_HGCONV", "0")
    kinds = collections.Counter(_kinds(plan))
    assert kinds["hgconv"] == 0 and kinds["matmul"] == 3 and kinds["softmax"] == 1, kinds
    # the GELU chains: one activation op each where the chain is the reference's; with the changed constant the edge chain keeps its eight
    # element-wise layers and its tanh (besides the prototype sum, the division and the residual add every variant has)
    assert kinds["act_nhwc"] + kinds["act_lin"] == 2, kinds
    assert kinds["ew_nhwc"] + kinds["ew_lin"] == (3 + 8 if miss == "gelu_const" else 3), kinds


def test_lone_gelu_chain_lowers_to_one_activation_op():
    from tensorrtx_amd import builder
    for fp16 in (True, False):
        net = builder.Network(explicit_batch=True, fp16=fp16)
        try:
            xi = net.input("x", (2, 3, 5, 6))
            t = net.out(net.conv(xi, np.ones((16, 3, 1, 1), np.float32)))
            t = net.out(net.pooling(t, 1, 1))      # a layer between the convolution and the chain
            net.mark_output(net.out(hc.gelu_chain(net, t, 4)), "y")
            plan = net.build()
        finally:
            net.close()
        kinds = _kinds(plan)
        assert kinds == ["conv", "pool", "act_nhwc", "to_linear"], kinds
        x = np.random.default_rng(0).standard_normal((2, 3, 5, 6)).astype(np.float32)
        y = gi.run(engine.describe_plan(plan), plan, {"x": x}, batch=2)["y"]
        v = torch.from_numpy(x).sum(1, keepdim=True).expand(2, 16, 5, 6).double()
        assert (y.double() - hc.gelu64(v)).abs().max().item() < 1e-5


def test_golden_plans_of_other_models_do_not_contain_the_new_ops():
    """No network built before this op contains the GELU chain: the yolo11 / yolo12 golden hashes (tests/test_golden.py, test_yolo12_cpu.py) are
    untouched; here only that a YOLOv12 plan, the nearest relative, has neither op"""
    from test_yolo12_cpu import lowered
    _, low = lowered("n", batch=1, h=96, w=96, fp16=1)
    kinds = {o["kind"] for o in low["ops"]}
    assert "hgconv" not in kinds and "attention" in kinds
    assert not any("GELU" in o["name"] for o in low["ops"])


# ---- the interpreter pins the builder helper -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spelling,B,D,E", [("a", 3, 64, 4), ("b", 1, 64, 4), ("a", 2, 48, 3)])
def test_interpreter_agrees_with_the_tables_reference(spelling, B, D, E):
    H, W = 5, 7
    _, w = hc.gen(hc._c(D, E, (5, 7), 3).name)
    plan = hc.subgraph_net(B, D, E, H, W, w, hc.c3ah_weights(D, seed=3), spelling=spelling, fp16=False, mark_inner=True)
    x = np.random.default_rng(5).standard_normal((B, 3, H, W)).astype(np.float32)
    out = gi.run(engine.describe_plan(plan), plan, {"x": x}, batch=B)
    x1 = out["x1"].reshape(B, D, H * W).transpose(1, 2)            # the tokens the subgraph saw, fp32 as the interpreter holds them
    ref = hc.reference_of(x1, w, D, E)
    got = out["m"].reshape(B, D, H * W).transpose(1, 2).double()
    err = (got - ref.out).abs().max().item()
    print(f"{spelling} B{B} D{D}: interpreter vs fp64 reference {err:.3g}, |out| {ref.out.abs().max().item():.3g}")
    assert err <= 2e-5 * max(1.0, ref.out.abs().max().item())


# ---- the C entry: arguments, exports -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_on_the_host():
    L = capi.lib()
    fn = L.trtx_op_hgconv_f16
    fn.argtypes = ([ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 4 + [ctypes.c_float] + [ctypes.c_void_p] * 9 +
                   [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p])
    B, N, D, E = 2, 35, 64, 4
    need = capi.hgconv_workspace_bytes(B, N, D, E)
    p = 0x10000     # never dereferenced: every call below returns before a launch (there is no device here to launch on)

    def call(x=p, ld_x=D, out=p, ld_out=D, B=B, N=N, D=D, E=E, w=None, ws=p, ws_bytes=need):
        w = [p] * 9 if w is None else w
        return fn(x, ld_x, out, ld_out, B, N, D, E, 0.0625, *w, ws, ws_bytes, None)

    INVALID, UNSUPPORTED = 1, 4     # TRTX_ERR_INVALID, TRTX_ERR_UNSUPPORTED
    assert call(x=None) == INVALID and call(out=None) == INVALID and call(ws=None) == INVALID
    for k in range(9):
        assert call(w=[None if j == k else p for j in range(9)]) == INVALID, hc.WEIGHTS[k]
    assert call(ld_x=D - 8) == INVALID and call(ld_out=D - 8) == INVALID
    assert call(ws_bytes=need - 1) == INVALID and call(ws_bytes=0) == INVALID
    assert call(B=0) == INVALID and call(N=0) == INVALID
    assert call(E=17) == UNSUPPORTED and call(D=24, ld_x=24, ld_out=24) == UNSUPPORTED and call(D=400, ld_x=400, ld_out=400) == UNSUPPORTED
    assert call(x=p + 2) == UNSUPPORTED and call(ld_out=D + 4) == UNSUPPORTED      # no 16-byte accesses: refused, not run element-wise
    n = ctypes.c_int32()
    assert L.trtx_op_hgconv_geometry(None, 4, ctypes.byref(n)) == INVALID


def test_header_exports_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "trtx_hip.h")).read()
    L = capi.lib()
    for sym in ("trtx_op_hgconv_workspace_bytes", "trtx_op_hgconv_geometry", "trtx_op_hgconv_f16"):
        assert re.search(r"\b%s\s*\(" % sym, src), sym
        assert hasattr(L, sym), sym
    proto = re.search(r"trtx_op_hgconv_f16\((.*?)\);", src, re.S).group(1)
    names = re.findall(r"const float\* (\w+)", proto)
    assert tuple(names) == capi.HGCONV_WEIGHTS == hc.WEIGHTS
    assert "block.cpp:607-700" in src and "block.cpp:746-790" in src and "block.cpp:702-744" in src
    assert L.trtx_abi_version() == 1
