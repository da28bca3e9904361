"""YOLOv12 on the GPU: the MFMA area-attention op against torch in fp64 and against the generic lowering of the same graph, its batch
invariance, and YOLOv12 engines against the oracle's interpreter (fp32) and against the fp32 engine (fp16).

Rounding sites of the attention op (kernels/attention_mfma.hip), u = 2^-11.  The reference is computed from the qkv tensor rounded to fp16
(the storage site the engine has by design).  The kernel's scores are fp32 MFMA sums of exact fp16 products, scaled in fp32; max, exp
and the denominator are fp32; then
  * p is rounded to fp16 as the P.V operand: each p_m carries a relative error <= u and the fp32 denominator none, so
    |dO| <= u * sum_m p_m |v_m| / l; the bound takes 2u * (softmax @ |v|);
  * O is rounded once at its store and the sum O + V once more: fp16_walk(2, |O| + |V|);
  * a one-ulp disagreement between the fp32 and the fp64 rounding of q / k moves a score by at most 2u * s_abs (s_abs = the largest
    scale * sum_j |q_j k_j|), the output by that times max |v|; and a floor of 1e-4 * max |v| for the fp32 arithmetic in between.
The generic lowering of the same fp16 graph has fewer sites (fp32 linear tensors between the qkv image and the sum), so the same bound
holds for it against fp64, and twice the bound between the two.
Engines: every convolution's packed weights and stored output is a site, and each attention op has two (its O store, its P rounding)."""
import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from oracle import yolo_post as yp
from tensorrtx_amd import engine, synth
from test_yolo12_cpu import aattn_net, aattn_reference, yolo12_wts
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk

pytestmark = pytest.mark.gpu
U16 = 2.0 ** -11


def _run(plan, inputs, gpu):
    e = engine.Engine(plan)
    batch = next(iter(inputs.values())).shape[0]
    bufs = []
    for i in range(e.nb_bindings):
        if e.is_input[i]:
            bufs.append(torch.from_numpy(np.ascontiguousarray(inputs[e.names[i]], dtype=np.float32)).to(gpu))
        else:
            bufs.append(torch.full((int(np.prod(e.dims[i])),), float("nan"), dtype=torch.float32, device=gpu))
    e.enqueue(batch, bufs)
    torch.cuda.synchronize()
    out = {e.names[i]: bufs[i].cpu() for i in range(e.nb_bindings) if not e.is_input[i]}
    e.close()
    return out


def _kinds(plan):
    return [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]]


def _bound(x, wq, heads, area, gain):
    o, v, scores, pv_abs, s_abs = aattn_reference(x, wq, heads, area)
    if gain > 1:
        assert scores.abs().max().item() > 40   # the large-score case: softmax without max subtraction overflows
        assert (scores.softmax(-1).max(-1).values > 0.99).float().mean().item() > 0.3   # rows one key dominates
    vmax = v.abs().max().item()
    return o + v, fp16_walk(2, o.abs() + v.abs()) + 2 * U16 * pv_abs + 2 * U16 * s_abs * vmax + 1e-4 * vmax


# heads, (H, W), area, B, q / k gain.  Keys per query: 8 (less than one tile), 100, 25, 42 (a partial tile), 168, 400, 100, 400, 1600, 400, 1600
OP_CASES = [(1, (4, 8), 4, 1, 1.0), (2, (10, 10), 1, 3, 1.0), (2, (10, 10), 4, 3, 1.0), (4, (12, 14), 4, 3, 1.0), (6, (12, 14), 1, 1, 1.0),
            (4, (20, 20), 1, 3, 1.0), (2, (20, 20), 4, 32, 1.0), (4, (20, 20), 1, 32, 1.0), (1, (40, 40), 1, 1, 1.0), (2, (40, 40), 4, 3, 1.0),
            (2, (80, 80), 4, 1, 1.0), (6, (20, 20), 4, 1, 1.0), (2, (10, 10), 1, 1, 6.0), (2, (12, 14), 4, 3, 6.0)]


@pytest.mark.parametrize("heads,hw,area,B,gain", OP_CASES)
def test_area_attention_op_matches_torch(heads, hw, area, B, gain, gpu):
    H, W = hw
    plan, x, wq = aattn_net(B, heads, H, W, area, gain=gain, seed=heads * 7 + H + area)
    kinds = _kinds(plan)
    assert kinds.count("attention") == 1 and not {"matmul", "softmax", "gather"} & set(kinds)
    got = _run(plan, {"x": x}, gpu)["y"].reshape(B, heads * 32, H, W).double()
    ref, bound = _bound(x, wq, heads, area, gain)
    err = (got - ref).abs()
    print(f"heads {heads} {H}x{W} area {area} B {B} gain {gain}: max err {err.max().item():.3g}, max err / bound {(err / bound).max().item():.3g}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.mark.parametrize("heads,hw,area,B,gain", [(2, (12, 14), 4, 3, 1.0), (4, (20, 20), 1, 3, 1.0), (2, (40, 40), 4, 3, 1.0), (2, (12, 14), 4, 3, 6.0)])
def test_fused_area_attention_agrees_with_generic_lowering(heads, hw, area, B, gain, gpu, monkeypatch):
    H, W = hw
    plan, x, wq = aattn_net(B, heads, H, W, area, gain=gain, seed=heads * 7 + H + area)
    fused = _run(plan, {"x": x}, gpu)["y"].reshape(B, heads * 32, H, W).double()
    monkeypatch.setenv("TRTX_AREA_ATTENTION", "0")
    kinds = _kinds(plan)
    assert kinds.count("attention") == 0 and kinds.count("matmul") == 2 and kinds.count("softmax") == 1
    generic = _run(plan, {"x": x}, gpu)["y"].reshape(B, heads * 32, H, W).double()
    ref, bound = _bound(x, wq, heads, area, gain)
    print(f"generic vs fp64 / bound {((generic - ref).abs() / bound).max().item():.3g}, fused vs generic / bound "
          f"{((fused - generic).abs() / bound).max().item():.3g}")
    assert ((generic - ref).abs() <= bound).all()
    assert ((fused - generic).abs() <= 2 * bound).all()


def test_area_attention_is_batch_invariant(gpu):
    """Image 0 of a B = 32 run is bit-equal to the same image run alone: the kernel's reduction order does not depend on B (and the 1x1
    qkv convolution on 16 channels takes the same tactic for both)"""
    p32, x, wq = aattn_net(32, 2, 20, 20, 4, seed=3)
    p1, _, _ = aattn_net(1, 2, 20, 20, 4, x=x[:1], wq=wq)
    a = _run(p32, {"x": x}, gpu)["y"].reshape(32, -1)[0]
    b = _run(p1, {"x": x[:1]}, gpu)["y"].reshape(-1)
    assert torch.equal(a, b)


@pytest.fixture(scope="module")
def y12n_fp32_640_b8():
    path, _ = yolo12_wts("n")
    B, S = 8, 640
    plan = engine.build_plan("yolo12n", path, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=MAX_OUT[("n", 640)])
    return plan, synth.images(B, S, S, seed=11)


# The synthetic class head passes most cells of these backbones (synth.yolo12_state).  Largest per-image candidate count of the reference
# alone - the fp32 twin (tests/yolo12_twin.py) on the CPU at the engine tests' seed (12) and sizes - next to the plugin's max_out:
#   n, 32 x 640^2: 6550 of 8400 cells;  s, 8 x 640^2: 8400 of 8400;  n, 2 x 1280^2: 26633 of 33600
MAX_OUT = {("n", 640): 8500, ("s", 640): 8500, ("n", 1280): 34000}   # above the cell count: no image can reach it


def test_yolo12n_fp32_engine_matches_interpreter(y12n_fp32_640_b8, gpu):
    plan, x = y12n_fp32_640_b8
    B, mo = x.shape[0], MAX_OUT[("n", 640)]
    got = _run(plan, {"images": x}, gpu)
    ref = gi.run(engine.describe_plan(plan), plan, {"images": x}, batch=B)
    for i in range(3):
        h = ref[f"head{i}"]
        err = (got[f"head{i}"].reshape(h.shape) - h).abs().max().item()
        print(f"head{i}: err {err:.3g}, |head| {h.abs().max().item():.3g}")
        assert err <= 1e-4 * max(1.0, h.abs().max().item()), (i, err)
    dec = yp.decode_c([got[f"head{i}"].reshape(ref[f"head{i}"].shape).numpy() for i in range(3)], 80, 640, 640, [8, 16, 32], max_out=mo)
    out = got["output"].reshape(B, -1).numpy()
    for b in range(B):   # the plugin writes the count and that many detections; the rest of the binding is not its output
        n = int(out[b, 0])
        assert 0 < n < mo and out[b, 0] == dec[b, 0], b
        got_d = out[b, 1:1 + n * yp.DET_FLOATS].reshape(n, yp.DET_FLOATS)[:, :6]
        ref_d = dec[b, 1:1 + n * yp.DET_FLOATS].reshape(n, yp.DET_FLOATS)[:, :6]
        rows = lambda a: a[np.lexsort(np.round(a[:, [3, 2, 1, 0, 5]], 2).T)]  # noqa: E731  (slot order is not fixed: sort)
        g_, r_ = rows(got_d), rows(ref_d)
        assert np.array_equal(g_[:, 5], r_[:, 5]), b
        assert np.allclose(g_, r_, rtol=1e-5, atol=1e-4), (b, np.abs(g_ - r_).max())


def _match_detections(dec, dec_ref, max_out, conf_margin=0.02):
    """tests/test_gpu_yolo11.py's matching, with one difference: no image may be left out (every count is below max_out)"""
    st = dict(ref=0, matched=0, min_iou=1.0)
    for b in range(dec_ref.shape[0]):
        nr, ng = int(dec_ref[b, 0]), int(dec[b, 0])
        assert nr < max_out and ng < max_out, (b, nr, ng, max_out)
        R = dec_ref[b, 1:1 + nr * yp.DET_FLOATS].reshape(nr, yp.DET_FLOATS)[:, :6]
        G = dec[b, 1:1 + ng * yp.DET_FLOATS].reshape(ng, yp.DET_FLOATS)[:, :6]
        for r in R:
            if abs(r[4] - 0.1) < conf_margin:
                continue
            st["ref"] += 1
            same = np.nonzero(G[:, 5] == r[5])[0]
            if len(same) == 0:
                continue
            c = np.abs((G[same, 0] + G[same, 2]) - (r[0] + r[2])) + np.abs((G[same, 1] + G[same, 3]) - (r[1] + r[3]))
            g = G[same[np.argmin(c)]]
            ix = max(0.0, min(r[2], g[2]) - max(r[0], g[0])) * max(0.0, min(r[3], g[3]) - max(r[1], g[1]))
            ua = (r[2] - r[0]) * (r[3] - r[1]) + (g[2] - g[0]) * (g[3] - g[1]) - ix
            iou = ix / ua if ua > 0 else 0.0
            if iou > 0.9:
                st["matched"] += 1
                st["min_iou"] = min(st["min_iou"], float(iou))
    return st


def _sites(plan):
    """fp16 rounding sites of a plan: every convolution's packed weights and stored output; per attention op its O store and its P rounding"""
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    convs = [o for o in ops if o["kind"] == "conv"] + [m for o in ops if o["kind"] == "conv_group" for m in o["members"]]
    return 2 * len(convs) + 2 * sum(o["kind"] == "attention" for o in ops)


@pytest.mark.parametrize("scale,B,S", [("n", 32, 640), ("s", 8, 640), ("n", 2, 1280)])
def test_yolo12_fp16_engine_tracks_fp32_engine(scale, B, S, gpu):
    """fp16 storage, fp32 accumulation, against the fp32 engine (pinned on the interpreter above, within 1e-4): head values within
    fp16_walk(sites, max |head|), detections of the fused head (no marked heads) matched as parity.py asks, no image left out"""
    path, _ = yolo12_wts(scale)
    x = synth.images(B, S, S, seed=12)
    mo = MAX_OUT[(scale, S)]
    name = "yolo12" + scale
    p16 = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, max_out=mo)
    p16h = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, mark_heads=1, max_out=mo)
    p32h = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=0, mark_heads=1, max_out=mo)
    kinds = _kinds(p16)
    assert kinds.count("attention") == 8 and kinds.count("yolo_head") == 1
    sites = _sites(p16)
    g16, g16h, g32 = _run(p16, {"images": x}, gpu), _run(p16h, {"images": x}, gpu), _run(p32h, {"images": x}, gpu)
    for i in range(3):
        h16, h32 = g16h[f"head{i}"], g32[f"head{i}"]
        assert torch.isfinite(h16).all()
        err, lim = (h16 - h32).abs().max().item(), fp16_walk(sites, h32.abs().max().item())
        print(f"{name} B{B} {S}: head{i} err {err:.3g}, bound {lim:.3g} ({sites} sites)")
        assert err <= lim, i
    st = _match_detections(g16["output"].reshape(B, -1).numpy(), g32["output"].reshape(B, -1).numpy(), mo)
    print(st)
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st
