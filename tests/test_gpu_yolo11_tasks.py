"""YOLO11 seg / pose / obb / cls on the GPU: the fused task head (trtx_yolo_task_head_decode_nhwc{,_f32}) in isolation against the det
head and the C oracle of the plugin's decode, the task engines with the plugin (marked heads) against the twin, the production plans
(fused task head) against those engines, the batch-32 seg plan's per-image addressing, and the classifier."""
import numpy as np
import pytest
import torch

from oracle import yolo_post as yp
from tensorrtx_amd import capi, engine, synth
from test_gpu_yolo11 import _match_detections, _run, _sites
from test_yolo11_tasks_cpu import TASKS, task_wts
from tests.parity import FP16_IOU, FP16_MATCH, fp16_walk
from yolo11_task_twin import Yolo11Task

pytestmark = pytest.mark.gpu
STRIDES = [8, 16, 32]


def _rows(dec, b):
    n = int(dec[b, 0])
    return dec[b, 1:1 + n * yp.DET_FLOATS].reshape(n, yp.DET_FLOATS)


# ------------------------------------------------------------------------------------------------------------- the kernel in isolation
def _heads(task, classes, fp16, B=3, S=640, seed=0, nk=17, odd_ld=False):
    """Seeded NHWC head [B, gh, gw, ld] and branch [B, gh, gw, bld] tensors with padded strides (the padding channels hold +20, which would
    win the argmax and pass the gate if they were read), and the equivalent CHW plugin inputs [B, 4 + classes + extra, g] with the DFL
    done in float64.  odd_ld: an odd branch stride, which rules out the branch's 16-byte loads (the kernel's scalar path)"""
    rng = np.random.default_rng(seed + 17 * classes)
    extra = TASKS[task][2] if task != "pose" else 3 * nk
    dt = np.float16 if fp16 else np.float32
    vec = 8 if fp16 else 4
    mean = {1: -5.0, 8: -6.0, 15: -6.5, 80: -7.2}[classes]   # about 3 % of the cells pass the 0.1 gate
    heads, branches, chw = [], [], []
    for s in STRIDES:
        gh = gw = S // s
        x = rng.normal(0, 1.5, size=(B, 64 + classes, gh, gw))
        x[:, 64:] = rng.normal(mean, 1.5, size=(B, classes, gh, gw))
        if task == "pose":
            br = rng.normal(0, 1.5, size=(B, extra, gh, gw))
            br[:, 2::3] = rng.normal(0.5, 2.0, size=(B, nk, gh, gw))
        else:
            br = rng.normal(0, 1.0 if task == "seg" else 2.0, size=(B, extra, gh, gw))
        x, br = x.astype(dt).astype(np.float32), br.astype(dt).astype(np.float32)   # the values the tensors hold
        ld = -(-(64 + classes) // vec) * vec + vec
        bld = extra + (1 if extra % 2 == 0 else 2) if odd_ld else -(-extra // vec) * vec + vec
        hn = np.full((B, gh, gw, ld), 20.0, dtype=np.float32)
        hn[..., :64 + classes] = x.transpose(0, 2, 3, 1)
        bn = np.full((B, gh, gw, bld), 20.0, dtype=np.float32)
        bn[..., :extra] = br.transpose(0, 2, 3, 1)
        heads.append(torch.from_numpy(hn).to(torch.float16 if fp16 else torch.float32))
        branches.append(torch.from_numpy(bn).to(torch.float16 if fp16 else torch.float32))
        bins = torch.from_numpy(x[:, :64].reshape(B, 4, 16, gh * gw)).double().softmax(2)
        box = (bins * torch.arange(16.0, dtype=torch.float64)[None, None, :, None]).sum(2).float().numpy()
        chw.append(np.concatenate([box, x[:, 64:].reshape(B, classes, -1), br.reshape(B, extra, -1)], 1))
    return heads, branches, chw


@pytest.mark.parametrize("task,classes,odd_ld", [("seg", 80, False), ("pose", 1, False), ("obb", 15, False), ("pose", 8, False),
                                                  ("seg", 80, True), ("pose", 1, True)])
@pytest.mark.parametrize("fp16", [1, 0])
def test_task_head_kernel_matches_plugin_decode(task, classes, odd_ld, fp16, gpu):
    B, S, mo = 3, 640, 2000
    heads, branches, chw = _heads(task, classes, fp16, B, S, odd_ld=odd_ld)
    assert all((b.shape[-1] % 2 == 1) == odd_ld for b in branches)
    dfl = torch.arange(16.0).to(gpu)
    hs, bs = [h.to(gpu) for h in heads], [b.to(gpu) for b in branches]
    kpt_conf = 0.5 if task == "pose" else 0.0
    out = capi.yolo_task_head_decode_nhwc(hs, bs, classes, S, S, STRIDES, dfl, max_out=mo, nk=17, kpt_conf=kpt_conf, **{task: True})
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = yp.decode_ex_c(chw, classes, S, S, STRIDES, mo, nk=17, kpt_conf=kpt_conf, **{task: True})
    assert np.array_equal(got[:, 0], ref[:, 0]) and ref[:, 0].min() >= 20 and ref[:, 0].max() < mo
    for b in range(B):
        G, R = _rows(got, b), _rows(ref, b)
        assert np.array_equal(G[:, 5], R[:, 5])
        assert np.allclose(G[:, 4], R[:, 4], rtol=0, atol=2e-7)
        # boxes: the kernel's fp32 DFL against the float64 one of the test
        assert np.allclose(G[:, :4], R[:, :4], rtol=1e-5, atol=1e-4)
        if task == "seg":
            assert np.array_equal(G[:, 6:38], R[:, 6:38]), "mask coefficients are copied"
        if task == "pose":
            gk, rk = G[:, 38:89], R[:, 38:89]
            assert np.array_equal(gk == -1, rk == -1) and np.allclose(gk, rk, rtol=1e-6, atol=1e-4)
            assert (gk == -1).any() and (gk != -1).any()
        if task == "obb":
            assert np.allclose(G[:, 89], R[:, 89], rtol=1e-6, atol=1e-7)
    if classes % 8 == 0:
        # the det head on the same head tensors: the same candidates, and box / conf / class to the bit (seg and pose keep the box)
        det = capi.yolo_head_decode_nhwc(hs, classes, S, S, STRIDES, dfl, max_out=mo)
        torch.cuda.synchronize()
        det = det.cpu().numpy()
        assert np.array_equal(got[:, 0], det[:, 0])
        for b in range(B):
            cols = slice(0, 6) if task != "obb" else slice(4, 6)
            assert np.array_equal(_rows(got, b)[:, cols], _rows(det, b)[:, cols])


# ------------------------------------------------------------------------------------------------------------- engines
def _engine_case(task, fp16, gpu, B, S, mark_heads, seed=7, max_out=1000):
    tid, nc, _ = TASKS[task]
    path, sd = task_wts("n", task)
    plan = engine.build_plan("yolo11n", path, batch=B, h=S, w=S, fp16=fp16, task=tid, mark_heads=mark_heads, max_out=max_out)
    x = synth.images(B, S, S, seed=seed)
    return plan, _run(plan, {"images": x}, gpu), x, sd, nc


@pytest.mark.parametrize("task", ["seg", "pose", "obb"])
def test_task_engine_fp32_plugin_path_matches_twin(task, gpu):
    B, S = 2, 128
    plan, out, x, sd, nc = _engine_case(task, 0, gpu, B, S, 1)
    kinds = [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]]
    assert kinds.count("plugin") == 1 and kinds.count("yolo_task_head") == 0
    with torch.inference_mode():
        heads, strides, proto = Yolo11Task(sd, "n", nc, task).task_heads(torch.from_numpy(x))
    worst = max((out[f"head{i}"].reshape(h.shape) - h).abs().max().item() for i, h in enumerate(heads))
    assert worst < 1e-3, worst
    got_heads = [out[f"head{i}"].reshape(h.shape).numpy() for i, h in enumerate(heads)]
    dec_ref = yp.decode_ex_c(got_heads, nc, S, S, strides, kpt_conf=0.0, **{task: True})
    dec = out["output"].reshape(dec_ref.shape).numpy()
    assert dec_ref[:, 0].min() >= 5
    assert np.array_equal(dec[:, 0], dec_ref[:, 0])
    for b in range(B):
        G, R = _rows(dec, b), _rows(dec_ref, b)
        assert np.array_equal(G[:, 5], R[:, 5])
        assert np.allclose(G[:, 4], R[:, 4], rtol=0, atol=2e-7)
        if task == "obb":
            assert np.allclose(G[:, :4], R[:, :4], rtol=1e-6, atol=1e-4) and np.allclose(G[:, 89], R[:, 89], rtol=1e-6, atol=1e-7)
        else:
            assert np.array_equal(G[:, :4], R[:, :4])
        if task == "seg":
            assert np.array_equal(G[:, 6:38], R[:, 6:38])
        if task == "pose":
            assert np.array_equal(G[:, 38:89] == -1, R[:, 38:89] == -1) and np.allclose(G[:, 38:89], R[:, 38:89], rtol=1e-6, atol=1e-4)
    if task == "seg":
        err = (out["proto"].reshape(proto.shape) - proto).abs().max().item()
        assert err < 1e-3 * max(1.0, proto.abs().max().item()), err


def _xyxy(dec, obb):
    """records with the box as x1 y1 x2 y2 (obb records hold cx cy w h and the angle: the axis-aligned box of the same centre and size)"""
    d = dec.copy()
    if obb:
        for b in range(d.shape[0]):
            n = int(d[b, 0])
            r = d[b, 1:1 + n * yp.DET_FLOATS].reshape(n, yp.DET_FLOATS)
            cx, cy, w, h = r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), r[:, 3].copy()
            r[:, 0], r[:, 1], r[:, 2], r[:, 3] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
            d[b, 1:1 + n * yp.DET_FLOATS] = r.reshape(-1)
    return d


@pytest.mark.parametrize("task", ["seg", "pose", "obb"])
@pytest.mark.parametrize("fp16", [0, 1])
def test_task_engine_fused_head_tracks_plugin_engine(task, fp16, gpu):
    """The production plan (one yolo_task_head) against the fp32 marked-heads engine's records (plugin path, pinned on the twin above):
    the matching rule and ceilings test_gpu_yolo11.py applies to det.  Matched records (same class, centres within 1 px) carry the same task
    fields within the bound of the branch values they come from, bv = fp16_walk(sites, max |head|) (fp32 plans: 1e-4 max |head|):
    seg coefficients within bv; keypoints (2 v + col) * stride within 2 * 32 * bv, their sigmoid confidence within bv / 4, and a keypoint
    kept on one side only lies within that bound (plus the two boxes' difference) of the other record's box edge; the obb angle
    (sigmoid(a) - 1/4) * pi within pi / 4 * bv"""
    B, S, mo = 4, 256, 10000
    obb = task == "obb"
    p, out, _, _, nc = _engine_case(task, fp16, gpu, B, S, 0, max_out=mo)
    _, ref, _, _, _ = _engine_case(task, 0, gpu, B, S, 1, max_out=mo)
    kinds = [o["kind"] for o in engine.describe_plan(p, lowered=True)["ops"]]
    assert kinds.count("yolo_task_head") == 1 and kinds.count("plugin") == 0
    dec, dec_ref = out["output"].reshape(B, -1).numpy(), ref["output"].reshape(B, -1).numpy()
    X, XR = _xyxy(dec, obb), _xyxy(dec_ref, obb)
    st = _match_detections(X, XR, mo)
    assert st["ref"] > 0
    assert st["matched"] / st["ref"] >= 1 - FP16_MATCH, st
    assert st["min_iou"] >= 1 - FP16_IOU, st
    hmax = max(ref[f"head{i}"].abs().max().item() for i in range(3))
    bv = fp16_walk(_sites(p), hmax) if fp16 else 1e-4 * hmax
    tol_k = 2 * 32 * bv + 1e-3
    pairs = kept = 0
    for b in range(B):
        G, R, GX, RX = _rows(dec, b), _rows(dec_ref, b), _rows(X, b), _rows(XR, b)
        for j, r in enumerate(RX):
            if abs(r[4] - 0.1) < 0.02:
                continue
            c = np.abs(GX[:, 0] + GX[:, 2] - r[0] - r[2]) + np.abs(GX[:, 1] + GX[:, 3] - r[1] - r[3]) + 1e9 * (GX[:, 5] != r[5])
            i = int(np.argmin(c))
            if c[i] >= 1.0:
                continue
            pairs += 1
            g, rr = G[i], R[j]
            if task == "seg":
                assert np.abs(g[6:38] - rr[6:38]).max() <= bv
            if task == "pose":
                gk, rk = g[38:89].reshape(17, 3), rr[38:89].reshape(17, 3)
                gv, rv = gk[:, 2] != -1, rk[:, 2] != -1
                both = gv & rv
                kept += int(both.sum())
                assert (np.abs(gk[both, :2] - rk[both, :2]) <= tol_k).all()
                assert (np.abs(gk[both, 2] - rk[both, 2]) <= bv / 4 + 1e-6).all()
                box_diff = np.abs(GX[i, :4] - r[:4]).max()
                for k in np.nonzero(gv != rv)[0]:
                    kx, ky = (gk[k, :2] if gv[k] else rk[k, :2])
                    other = r[:4] if gv[k] else GX[i, :4]
                    edge = min(abs(kx - other[0]), abs(kx - other[2]), abs(ky - other[1]), abs(ky - other[3]))
                    assert edge <= tol_k + box_diff, (k, edge)
            if obb:
                assert abs(g[89] - rr[89]) <= np.pi / 4 * bv + 1e-6
    assert pairs > 0
    if task == "pose":
        assert kept > 0


def test_yolo11n_seg_fp16_640_b32_permuting_images_permutes_outputs(gpu):
    """The seg configuration timed in DESIGN §5 (fp16, 640², batch 32, production plan): permuting the images permutes the records and
    the proto planes bit for bit (no cross-image addressing in the branch reads)"""
    B, S = 32, 640
    path, _ = task_wts("n", "seg")
    plan = engine.build_plan("yolo11n", path, batch=B, h=S, w=S, fp16=1, task=1)
    assert [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]].count("yolo_task_head") == 1
    x = synth.images(B, S, S, seed=1)
    perm = np.array([(7 * i + 3) % B for i in range(B)])
    a, b = _run(plan, {"images": x}, gpu), _run(plan, {"images": x[perm]}, gpu)
    dec, dec_p = a["output"].reshape(B, -1).numpy(), b["output"].reshape(B, -1).numpy()
    pa, pb = a["proto"].reshape(B, 32, S // 4, S // 4), b["proto"].reshape(B, 32, S // 4, S // 4)
    for j in range(B):
        n = int(dec_p[j, 0])
        assert n == int(dec[perm[j], 0]) and 0 < n <= 1000
        assert np.array_equal(_rows(dec_p, j)[:, :38], _rows(dec, perm[j])[:, :38])
        assert torch.equal(pb[j], pa[perm[j]])


# ------------------------------------------------------------------------------------------------------------- classifier
def test_yolo11n_cls_engines_b32_224(gpu):
    """fp32 logits within 1e-3 of the twin; fp16 logits within fp16_walk(sites, |W| . |pooled features|), the sites counted from the plan
    (test_gpu_yolo11.py's rule) plus the linear layer's weights and its input"""
    B, S = 32, 224
    path, sd = task_wts("n", "cls")
    x = synth.images(B, S, S, seed=9)
    with torch.inference_mode():
        ref, feat = Yolo11Task(sd, "n", 1000, "cls").classify(torch.from_numpy(x))
    mag = (feat.abs() @ torch.from_numpy(sd["model.10.linear.weight"]).double().abs().T + torch.from_numpy(sd["model.10.linear.bias"]).double().abs())
    p32 = engine.build_plan("yolo11n", path, batch=B, h=S, w=S, fp16=0, task=4)
    g32 = _run(p32, {"images": x}, gpu)["output"].reshape(B, 1000).double()
    assert (g32 - ref).abs().max().item() < 1e-3
    p16 = engine.build_plan("yolo11n", path, batch=B, h=S, w=S, fp16=1, task=4)
    g16 = _run(p16, {"images": x}, gpu)["output"].reshape(B, 1000).double()
    assert torch.isfinite(g16).all()
    bound = fp16_walk(_sites(p16) + 2, mag)
    assert ((g16 - ref).abs() <= bound).all(), ((g16 - ref).abs() - bound).max().item()
