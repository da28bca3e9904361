"""YOLOv10 on the GPU.

Kernels: every case of tests/yolov10_cases.py through trtx_yolov10_decode (fp32 planes) and trtx_yolov10_head_decode_nhwc{,_f32} (the head
convolutions' NHWC layout at three pixel strides per class count, NaN / 60000 in the padding channels) against the NumPy restatement of the
reference's CalDetection.  Outputs are pre-filled with a sentinel and carry one row more than the batch.  Exact: counts, class ids, slot
order, every float behind a row's records and the extra row.  conf within 2e-7.  Boxes: the planar decode bit for bit, the fused head under
the DFL bound of tests/test_gpu_yolo_head.py (yolov10_cases.box_bound: yolo_head_cases.bound_of on this table's data), printed as
max err / bound.  The fused head and the planar decode agree bit for bit in count, conf and class on the same fp32 values, and the head's
result does not depend on the pixel stride.  trtx_yolov10_topk is bit for bit the restatement of get_topk on every case, into pre-filled
outputs.  RepVGGDW runs as single-layer networks through tests/test_gpu_layers.py's checker and error model, folded and with
TRTX_REPVGGDW_FOLD=0, fp32 and fp16, 8 / 24 / 40 channels, maps of 2 x 2, 7 x 9 and 20 x 20, into a tensor of its own and into a concat slice.

Engines (explicit batch, as the reference builds: a plan serves exactly its batch, so the issue's "3 of 4" partial batch has no enqueue to
run on and a plan of batch 3 stands in): fp32 heads against the fp64 twin (tests/yolov10_twin.py), "output" against the restatement's decode
of the engine's own heads, fp16 against fp32, the fused head against TRTX_YOLO10_HEAD=0, folded against unfolded.

Candidates the synthetic models keep (synth.yolov10_state, seed 0, 80 classes), measured with the fp64 twin on the CPU at the engine tests'
image seeds and sizes, per image, next to the cell count (max_out is 1000, out of reach of these nets):
  yolov10n, 1 x 64 x 64 (seed 5): 24 of 84              yolov10n, 2 x 64 x 64 (seed 5): 31, 26 of 84
  yolov10n, 3 x 64 x 64 (seed 5): 30, 30, 31 of 84      yolov10m, 1 x 64 x 64 (seed 5): 31 of 84
  yolov10n, 1 x 96 x 64 (seed 5): 41 of 126             yolov10n, 4 x 64 x 64 (seed 12): 33, 34, 34, 29 of 84
  yolov10m, 1 x 64 x 64 (seed 12): 34 of 84
(test_fp32_engine_matches_twin asserts at least 8, fewer than the cells and fewer than max_out on what the engine itself keeps.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_layers as tgl
from tensorrtx_amd import capi, engine, synth
from test_gpu_yolov5 import kinds, run
from test_yolov10_cpu import convs_of, yolov10_wts
from tests import layer_cases as lc
from tests import yolo_head_cases as hc
from tests import yolov10_cases as yc
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk
from tests.util import SENTINEL, sync, time_limit
from yolov10_twin import Yolov10

pytestmark = pytest.mark.gpu
REC = yc.REC
MAX_OUT = 1000


def framed(batch, max_out, gpu):
    """an output buffer one row longer than the batch, filled with a sentinel"""
    return torch.full((batch + 1, 1 + max_out * REC), SENTINEL, dtype=torch.float32, device=gpu)


def check_frame(got, ref, what):
    """exact: the counts, the row behind the batch and the floats behind every row's records"""
    B = ref.shape[0]
    assert (got[B:] == SENTINEL).all(), f"{what}: a row behind the batch was written"
    assert np.array_equal(got[:B, 0], ref[:, 0]), (what, got[:B, 0], ref[:, 0])
    for b in range(B):
        n = int(ref[b, 0])
        assert (got[b, 1 + n * REC:] == SENTINEL).all(), f"{what}: image {b}: written behind its {n} records"


# ---- the decode and head kernels -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", yc.DTYPES)
@pytest.mark.parametrize("case", yc.DECODE_CASES, ids=lambda c: c.name)
def test_decode_and_head_kernels(gpu, case, dt):
    H, W, strides = case.net
    ref = yc.reference(case.name, dt)
    kept = yc.kept_cells(case.name, dt)
    # the planar plugin kernel on the restatement's own inputs
    ins = [torch.from_numpy(x).to(gpu) for x in yc.planar(case.name, dt)]
    out = framed(case.B, case.max_out, gpu)
    with time_limit():
        capi.yolov10_decode(ins, case.classes, H, W, list(strides), case.max_out, out=out)
        sync(f"{case.name} planar")
    planar = out.cpu().numpy()
    check_frame(planar, ref, f"{case.name} {dt} planar")
    for b in range(case.B):
        G, R = yc.records(planar, b), yc.records(ref, b)
        assert np.array_equal(G[:, 5], R[:, 5]), f"planar: class ids / slot order, image {b}"
        assert (np.abs(G[:, 4] - R[:, 4]) <= hc.CONF_ATOL).all()
        assert np.array_equal(G[:, :4], R[:, :4], equal_nan=True), f"planar: the boxes are two exact fp32 operations, image {b}"
    # the fused head at every pixel stride
    w = torch.from_numpy(yc.build(case.name, dt).dfl_w).to(gpu)
    first = None
    for ld in yc.head_lds(case, dt):
        heads = [h.to(gpu) for h in yc.head_tensors(case.name, dt, ld)]
        assert torch.isnan(heads[0][..., 64 + case.classes:]).any() or ld == 64 + case.classes
        out = framed(case.B, case.max_out, gpu)
        with time_limit():
            capi.yolov10_head_decode_nhwc(heads, case.classes, H, W, list(strides), w, case.max_out, out=out)
            sync(f"{case.name} {dt} ld {ld}")
        got = out.cpu().numpy()
        check_frame(got, ref, f"{case.name} {dt} ld {ld}")
        worst = 0.0
        for b in range(case.B):
            G, R, P = yc.records(got, b), yc.records(ref, b), yc.records(planar, b)
            assert np.array_equal(G[:, 5], R[:, 5]), f"class ids / slot order, image {b}"
            assert np.array_equal(G[:, 4:6], P[:, 4:6]), "the fused head and the planar decode: conf and class bit for bit"
            assert np.array_equal(np.isnan(G[:, :4]), np.isnan(R[:, :4]))
            if len(G):
                bound = yc.box_bound(case.name, dt, b, kept[b][:len(G)], R)
                ok = ~np.isnan(R[:, :4])
                frac = np.abs(G[:, :4].astype(np.float64) - R[:, :4])[ok] / bound[ok]
                worst = max(worst, float(frac.max()) if frac.size else 0.0)
        print(f"{case.name} {dt} ld {ld}: records {ref[:, 0].astype(int).tolist()} of {case.cells}, max err / bound {worst:.3f}")
        assert worst <= 1.0, (case.name, dt, ld, worst)
        if first is None:
            first = got
        else:
            assert np.array_equal(got, first, equal_nan=True), f"ld {ld}: the pixel stride changes the result"


@pytest.mark.parametrize("dt", yc.DTYPES)
def test_head_with_a_batch_below_the_tensors_and_a_filled_workspace(gpu, dt):
    """three images in the tensors, batch 2 in the call, a workspace pre-filled with 0x5A: rows 2 and 3 keep the sentinel"""
    case = yc.DECODE_BY_NAME["full_126_nc8_b3"]
    H, W, strides = case.net
    ref = yc.reference(case.name, dt)
    heads = [h.to(gpu) for h in yc.head_tensors(case.name, dt, yc.head_lds(case, dt)[1])]
    w = torch.from_numpy(yc.build(case.name, dt).dfl_w).to(gpu)
    ws = torch.full((capi.yolov10_head_decode_workspace(3, H, W, list(strides)),), 0x5A, dtype=torch.uint8, device=gpu)
    out = torch.full((4, 1 + case.max_out * REC), SENTINEL, dtype=torch.float32, device=gpu)
    with time_limit():
        capi.yolov10_head_decode_nhwc(heads, case.classes, H, W, list(strides), w, case.max_out, out=out, ws=ws, batch=2)
        sync("batch 2 of 3")
    check_frame(out.cpu().numpy(), ref[:2], "batch 2 of 3")


# ---- top-k -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", yc.TOPK_CASES, ids=lambda c: c.name)
def test_topk_is_the_restatement(gpu, case):
    dec = yc.topk_input(case.name)
    B = dec.shape[0]
    ref = yc.topk_ref(dec, case.max_out, case.thresh, case.topk)
    out = framed(B, case.max_out, gpu)
    with time_limit():
        capi.yolov10_topk(torch.from_numpy(dec.copy()).to(gpu), case.max_out, case.thresh, case.topk, out=out, batch=B)
        sync(case.name)
    got = out.cpu().numpy()
    check_frame(got, ref, case.name)
    print(f"{case.name}: headers {dec[:, 0].astype(int).tolist()} -> kept {ref[:, 0].astype(int).tolist()}")
    for b in range(B):
        assert np.array_equal(yc.records(got, b).view(np.int32), yc.records(ref, b).view(np.int32)), f"image {b}"


# ---- RepVGGDW as a single layer --------------------------------------------------------------------------------------------------------

def repdw_case(C, H, W, B, wrap, folded):
    """SiLU(dw7x7 + BN + dw3x3 + BN) of one NHWC tensor (yolov10/src/block.cpp:388-403).  Error model: 49 + 9 products and the two shifts
    accumulated in fp32 (n), magnitude = the same sums over absolute values, times 1.1 for SiLU's slope; an fp16 plan stores the result once
    (folded: one site) or the 3x3 branch, the sum, the sigmoid and the product (unfolded: four sites).  The folded filter is one fp32 rounding of
    the exact sum of two products, covered by the two terms n counts beyond the 58 products."""
    rng = np.random.default_rng(1000 * C + 10 * H + W)
    w7 = (rng.standard_normal((C, 1, 7, 7)) / 7).astype(np.float32)
    w3 = (rng.standard_normal((C, 1, 3, 3)) / 3).astype(np.float32)
    s7, s3 = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32)
    h7, h3 = (0.1 * rng.standard_normal(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    d = lambda a: torch.from_numpy(a).double()  # noqa: E731

    def pre(x, absolute=False):
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        a = F.conv2d(f(x), f(d(w7)), None, 1, 3, 1, C) * f(d(s7))[:, None, None] + f(d(h7))[:, None, None]
        b = F.conv2d(f(x), f(d(w3)), None, 1, 1, 1, C) * f(d(s3))[:, None, None] + f(d(h3))[:, None, None]
        return a + b

    def build(net, t):
        x = lc.nhwc(net, t["x"])
        a = net.out(net.scale(net.out(net.conv(x, w7, padding=3, groups=C)), h7, s7))
        b = net.out(net.scale(net.out(net.conv(x, w3, padding=1, groups=C)), h3, s3))
        s = net.out(net.elementwise(a, b, "sum"))
        y = net.out(net.elementwise(s, net.out(net.activation(s, "sigmoid")), "prod"))
        if wrap == "concat":
            y = net.out(net.concat([lc.select_conv(net, lc.nhwc(net, t["z"]), 8, lc.NEIGHBOUR), y]))
        return {"y": y}

    def ref(x):
        o = lc.Out(F.silu(pre(x["x"])), 1.1 * pre(x["x"], True), n=49 + 9 + 4, sites=1 if folded else 4)
        if wrap == "concat":
            o.ch = slice(12, None)
            return {"y": [lc.Out(x["z"][:, lc.NEIGHBOUR], ch=slice(0, 12)), o]}
        return {"y": o}
    inputs = {"x": ((C, H, W), "n")}
    if wrap == "concat":
        inputs["z"] = ((8, H, W), "n")
    want = {"conv"}
    return lc.Case(name=f"repvggdw_c{C}_{H}x{W}_b{B}_{wrap}_{'folded' if folded else 'unfolded'}", family="repvggdw", inputs=inputs, build=build, ref=ref,
                   kinds=want, absent={"act_nhwc", "ew_nhwc"} if folded else frozenset(), batch=B)


REPDW = [(8, 2, 2, 2, "plain"), (24, 7, 9, 1, "plain"), (40, 20, 20, 2, "plain"), (8, 7, 9, 2, "concat"), (24, 2, 2, 1, "concat"), (40, 7, 9, 1, "concat")]


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("folded", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("shape", REPDW, ids=lambda s: f"c{s[0]}_{s[1]}x{s[2]}_b{s[3]}_{s[4]}")
def test_repvggdw_layer(shape, folded, fp16, gpu, monkeypatch):
    if not folded:
        monkeypatch.setenv("TRTX_REPVGGDW_FOLD", "0")
    case = repdw_case(*shape, folded)
    low = engine.describe_plan(lc.build_plan(case, fp16), lowered=True)
    dw = [o for o in convs_of(low) if o.get("dw")]
    assert len(dw) == (1 if folded else 2) and bool(dw[0].get("repvggdw_fold")) == folded, [o["name"] for o in convs_of(low)]
    tgl.test_layer_matches_fp64_reference(case, fp16, gpu)


# ---- engines ---------------------------------------------------------------------------------------------------------------------------

def match_detections(dec, dec_ref, skip_margin=None):
    """every reference record (those with conf within skip_margin of the 0.1 gate left out, if given) must appear with the same class and a
    box of IoU > 0.9; candidates come from distinct cells, so they are matched on the box centre.  No image is left out."""
    st = dict(ref=0, matched=0, min_iou=1.0, skipped=0)
    for b in range(dec_ref.shape[0]):
        assert dec_ref[b, 0] < MAX_OUT and dec[b, 0] < MAX_OUT
        R, G = yc.records(dec_ref, b), yc.records(dec, b)
        for r in R:
            if skip_margin is not None and abs(r[4] - 0.1) < skip_margin:
                st["skipped"] += 1
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


def sites_of(plan):
    """fp16 rounding sites of a plan: every convolution's packed weights and stored output, the attention's O, and every stored element-wise result"""
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    return 2 * len(convs_of({"ops": ops})) + sum(o["kind"] in ("attention", "act_nhwc", "ew_nhwc") for o in ops)


@pytest.mark.parametrize("name,B,H,W", [("yolov10n", 1, 64, 64), ("yolov10n", 2, 64, 64), ("yolov10n", 3, 64, 64), ("yolov10m", 1, 64, 64),
                                        ("yolov10n", 1, 96, 64)])
def test_fp32_engine_matches_twin(gpu, name, B, H, W):
    """heads within 1e-4 * max(1, |head|) of the fp64 twin (the bound of the other families' twin tests); "output" is the restatement's decode
    of the engine's own heads: counts, classes and order exact, conf within 2e-7, boxes bit for bit (the plugin route is the planar kernel)"""
    path, sd = yolov10_wts(name)
    plan = engine.build_plan(name, path, batch=B, h=H, w=W, fp16=0, mark_heads=1)
    assert kinds(plan).count("plugin") == 1
    x = synth.images(B, H, W, seed=5)
    got = run(plan, x, gpu)
    with torch.inference_mode():
        heads, strides = Yolov10(sd, name).heads(torch.from_numpy(x))
    assert strides == [8, 16, 32]
    mine = []
    for i, h in enumerate(heads):
        g = got[f"head{i}"].reshape(h.shape)
        err = (g.double() - h).abs().max().item()
        print(f"{name} {B}x{H}x{W} head{i}: err {err:.3g}, |head| {h.abs().max().item():.3g}")
        assert err <= 1e-4 * max(1.0, h.abs().max().item()), (i, err)
        mine.append(g.numpy())
    out = got["output"].reshape(B, -1).numpy()
    cells = sum(h.shape[2] for h in heads)
    print(f"{name}: candidates {out[:, 0].astype(int).tolist()} of {cells} cells")
    assert (out[:, 0] >= 8).all() and (out[:, 0] < cells).all() and (out[:, 0] < MAX_OUT).all()
    ref = yc.decode_ref(mine, 80, H, W, strides, MAX_OUT)
    assert np.array_equal(out[:, 0], ref[:, 0])
    for b in range(B):
        G, R = yc.records(out, b), yc.records(ref, b)
        assert np.isnan(out[b, 1 + len(G) * REC:]).all(), "written behind the records"
        assert np.array_equal(G[:, 5], R[:, 5]) and (np.abs(G[:, 4] - R[:, 4]) <= hc.CONF_ATOL).all()
        assert np.array_equal(G[:, :4], R[:, :4])
    # the same engine without marked heads runs the fused head: another plan, matched against the plugin route's records
    fused = engine.build_plan(name, path, batch=B, h=H, w=W, fp16=0)
    k = kinds(fused)
    # (fp32 engines keep the generic attention path, as YOLO11's do: its softmax is the only one left)
    assert k.count("yolo10_head") == 1 and "plugin" not in k and k.count("softmax") == 1 and k.count("matmul") == 2
    fout = run(fused, x, gpu)["output"].reshape(B, -1).numpy()
    st = match_detections(fout, out)
    print(f"{name} fp32 fused head: counts {fout[:, 0].astype(int).tolist()}", st)
    assert np.array_equal(fout[:, 0], out[:, 0]) and st["matched"] == st["ref"] > 0 and st["min_iou"] >= 0.999, st


@pytest.mark.parametrize("name,B", [("yolov10n", 4), ("yolov10m", 1)])
def test_fp16_engine_tracks_fp32_engine(name, B, gpu):
    """fp16 storage, fp32 accumulation, against the fp32 engine: head values within fp16_walk(sites, max |head|); detections of the fused head
    matched under FP16_MATCH / FP16_IOU, candidates within 0.02 of the gate skipped"""
    path, _ = yolov10_wts(name)
    S = 64
    x = synth.images(B, S, S, seed=12)
    p16 = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1)
    p16h = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    p32h = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=0, mark_heads=1)
    k = kinds(p16)
    assert k.count("yolo10_head") == 1 and k.count("attention") == 1 and "plugin" not in k
    sites = sites_of(p16)
    g16, g16h, g32 = run(p16, x, gpu), run(p16h, x, gpu), run(p32h, x, gpu)
    for i in range(3):
        a, r = g16h[f"head{i}"], g32[f"head{i}"]
        assert torch.isfinite(a).all()
        err, lim = (a - r).abs().max().item(), fp16_walk(sites, r.abs().max().item())
        print(f"{name} B{B}: head{i} err {err:.3g}, bound {lim:.3g} ({sites} sites)")
        assert err <= lim, i
    ref = g32["output"].reshape(B, -1).numpy()
    st = match_detections(g16["output"].reshape(B, -1).numpy(), ref, skip_margin=0.02)
    print(st, "counts", ref[:, 0].astype(int).tolist())
    assert (ref[:, 0] > 0).all() and st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st


def test_fused_head_engine_agrees_with_the_plugin_route(gpu, monkeypatch):
    """the fused fp16 plan against the plan the same build makes with TRTX_YOLO10_HEAD=0: the same heads in both (the switch changes nothing in
    front of them), so the same counts, order and classes and conf within 2e-7.  Boxes: the fused head keeps the DFL in fp32 registers, the
    plugin route's DFL convolution may read the softmax from and store the distance to fp16 tensors - two roundings of relative 2^-11 on a
    distance below 15 (dfl_w = arange(16)) - so stride * 15 * 2^-10 at the coarsest stride, 32"""
    path, _ = yolov10_wts("yolov10n")
    B, S = 4, 64
    x = synth.images(B, S, S, seed=12)
    fused = engine.build_plan("yolov10n", path, batch=B, h=S, w=S, fp16=1)
    assert kinds(fused).count("yolo10_head") == 1
    a = run(fused, x, gpu)["output"].reshape(B, -1).numpy()
    monkeypatch.setenv("TRTX_YOLO10_HEAD", "0")
    route = engine.build_plan("yolov10n", path, batch=B, h=S, w=S, fp16=1)
    k = kinds(route)
    assert k.count("plugin") == 1 and k.count("yolo10_head") == 0 and k.count("softmax") == 3
    r = run(route, x, gpu)["output"].reshape(B, -1).numpy()
    print("counts fused", a[:, 0], "plugin route", r[:, 0])
    assert np.array_equal(a[:, 0], r[:, 0]) and (a[:, 0] >= 8).all()
    for b in range(B):
        G, R = yc.records(a, b), yc.records(r, b)
        assert np.array_equal(G[:, 5], R[:, 5]) and (np.abs(G[:, 4] - R[:, 4]) <= hc.CONF_ATOL).all()
        err = np.abs(G[:, :4] - R[:, :4]).max()
        print(f"image {b}: max box difference {err:.3g}")
        assert err <= 32 * 15 * 2.0 ** -10, (b, err)


def test_folded_engine_tracks_the_unfolded_one(gpu, monkeypatch):
    """yolov10s (two lk CIB blocks) in fp16, heads marked: folded against TRTX_REPVGGDW_FOLD=0 within the sum of the two routes' bounds,
    fp16_walk over each plan's own rounding sites"""
    name, B, S = "yolov10s", 2, 64
    path, _ = yolov10_wts(name)
    x = synth.images(B, S, S, seed=12)
    fold = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    assert sum(bool(o.get("repvggdw_fold")) for o in convs_of(engine.describe_plan(fold, lowered=True))) == 2
    a = run(fold, x, gpu)
    monkeypatch.setenv("TRTX_REPVGGDW_FOLD", "0")
    plain = engine.build_plan(name, path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    assert not any(o.get("repvggdw_fold") for o in convs_of(engine.describe_plan(plain, lowered=True)))
    r = run(plain, x, gpu)
    for i in range(3):
        mag = r[f"head{i}"].abs().max().item()
        err, lim = (a[f"head{i}"] - r[f"head{i}"]).abs().max().item(), fp16_walk(sites_of(fold), mag) + fp16_walk(sites_of(plain), mag)
        print(f"head{i}: folded - unfolded {err:.3g}, bound {lim:.3g}")
        assert torch.isfinite(a[f"head{i}"]).all() and err <= lim
