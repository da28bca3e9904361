"""YOLO11 seg / pose / obb / cls (host builders, the fused task head's lowering): CPU-side checks."""
import collections
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import graph_interp as gi
from oracle import yolo_post as yp
from tensorrtx_amd import engine, synth
from tensorrtx_amd import wts as wts_writer
from test_yolo11_cpu import LINEAR_KINDS, yolo11_wts
from util import CACHE, synth_wts
from yolo11_task_twin import Yolo11Task

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = {"seg": (1, 80, 32), "pose": (2, 1, 51), "obb": (3, 15, 1), "cls": (4, 1000, 0)}   # task id, default classes, branch channels


def task_wts(scale, task, seed=0):
    tid, nc, _ = TASKS[task]
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"yolo11{scale}_{task}_synth_s{seed}.wts")
    sd = synth.yolo11_state(scale, seed=seed, num_class=nc, task=tid)
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, sd, dialect="double")
        os.replace(tmp, path)
    return path, sd


def task_plugin(orig):
    """graph_interp's plugin handler with the seg / pose / obb branches: the YoloLayer_TRT blob (yololayer.cu:75-101) read in full and
    decoded by yolo_post.decode_ex_c; every other plugin goes to the interpreter's own handler"""
    def run(l, ins, batch):
        if l["plugin_type"] != "YoloLayer_TRT":
            return orig(l, ins, batch)
        blob = bytes.fromhex(l["plugin_blob"])
        hdr = np.frombuffer(blob, dtype=np.int32, count=8)
        classes, nk, net_w, net_h, max_out, ns = (int(hdr[i]) for i in (0, 1, 4, 5, 6, 7))
        kpt_conf = float(np.frombuffer(blob, dtype=np.float32, count=1, offset=8)[0])
        strides = [int(v) for v in np.frombuffer(blob, dtype=np.int32, count=ns, offset=32)]
        seg, pose, obb = (bool(b) for b in blob[32 + 4 * ns:35 + 4 * ns])
        arrs = [np.ascontiguousarray(t.numpy().reshape(batch, t.shape[-2], -1)) for t in ins]
        out = yp.decode_ex_c(arrs, classes, net_h, net_w, strides, max_out, nk=nk, kpt_conf=kpt_conf, seg=seg, pose=pose, obb=obb)
        return [torch.from_numpy(out).reshape(batch, -1, 1, 1)]
    return run


@pytest.mark.parametrize("scale,task", [("n", "seg"), ("n", "pose"), ("n", "obb"), ("m", "seg")])
def test_yolo11_task_builder_matches_twin(scale, task, monkeypatch):
    """The host builder's seg / pose / obb graph (explicit batch, marked heads) through the interpreter against the twin; yolo11m-seg
    takes the C3k path"""
    tid, nc, extra = TASKS[task]
    path, sd = task_wts(scale, task)
    B, S = 2, 128
    plan = engine.build_plan("yolo11" + scale, path, batch=B, h=S, w=S, fp16=1, task=tid, mark_heads=1)
    desc = engine.describe_plan(plan)
    monkeypatch.setattr(gi, "_plugin", task_plugin(gi._plugin))
    x = torch.from_numpy(synth.images(B, S, S, seed=5))
    out = gi.run(desc, plan, {"images": x.numpy()}, batch=B)
    with torch.inference_mode():
        heads, strides, proto = Yolo11Task(sd, scale, nc, task).task_heads(x)
    assert strides == [8, 16, 32]
    for i, h in enumerate(heads):
        assert tuple(out[f"head{i}"].shape) == tuple(h.shape) == (B, 4 + nc + extra, (S // strides[i]) ** 2)
        assert (out[f"head{i}"] - h).abs().max().item() < 2e-4
    if task == "seg":
        assert tuple(out["proto"].shape) == tuple(proto.shape) == (B, 32, S // 4, S // 4)
        assert (out["proto"] - proto).abs().max().item() < 2e-4
    else:
        assert "proto" not in out
    # the plugin's parameters (task flag, keypoints, the truncated keypoint threshold 0, strides) as the reference's addYoLoLayer sets them
    okw = {task: True}
    got = out["output"].reshape(B, -1).numpy()
    dec = yp.decode_ex_c([out[f"head{i}"].numpy() for i in range(3)], nc, S, S, strides, kpt_conf=0.0, **okw)
    assert np.array_equal(got, dec)
    ref = yp.decode_ex_c([h.numpy() for h in heads], nc, S, S, strides, kpt_conf=0.0, **okw)
    assert np.array_equal(got[:, 0], ref[:, 0])
    assert got[:, 0].min() >= 5, "the synthetic weights must give candidates past the 0.1 gate"


def test_yolo11_cls_builder_matches_twin():
    path, sd = task_wts("n", "cls")
    B, S = 2, 224
    plan = engine.build_plan("yolo11n", path, batch=B, h=S, w=S, fp16=1, task=4)
    desc = engine.describe_plan(plan)
    x = torch.from_numpy(synth.images(B, S, S, seed=6))
    out = gi.run(desc, plan, {"images": x.numpy()}, batch=B)
    assert set(out) == {"output"}
    with torch.inference_mode():
        ref, _ = Yolo11Task(sd, "n", 1000, "cls").classify(x)
    assert tuple(out["output"].shape) == (B, 1000)
    assert (out["output"] - ref.float()).abs().max().item() < 2e-4


@pytest.mark.parametrize("task,S", [("seg", 640), ("pose", 640), ("obb", 1024)])
@pytest.mark.parametrize("fp16", [1, 0])
def test_yolo11n_task_tail_lowers_to_one_fused_op(task, S, fp16):
    tid = TASKS[task][0]
    path, _ = task_wts("n", task)
    low = engine.describe_plan(engine.build_plan("yolo11n", path, batch=32, h=S, w=S, fp16=fp16, task=tid), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["yolo_task_head"] == 1 and kinds["plugin"] == 0 and kinds["yolo_head"] == 0, kinds
    (op,) = [o for o in low["ops"] if o["kind"] == "yolo_task_head"]
    assert op["task"] == task and op["classes"] == TASKS[task][1] and op["nk"] == (17 if task == "pose" else 0)
    if fp16:
        assert kinds["attention"] == 1
        lin = [o for o in low["ops"] if o["kind"] in LINEAR_KINDS]
        # the seg plan's "proto" output binding is LINEAR fp32: its one conversion is the only linear-path op
        assert [o["name"] for o in lin] == (["to_linear:proto"] if task == "seg" else []), [o["name"] for o in lin]
    else:
        # fp32 plans keep the generic attention (its matmul / softmax / gathers): the tail adds none of those kinds to the det plan's
        det_path, _ = yolo11_wts("n")
        det = collections.Counter(o["kind"] for o in engine.describe_plan(
            engine.build_plan("yolo11n", det_path, batch=32, h=S, w=S, fp16=0), lowered=True)["ops"])
        for k in ("softmax", "gather", "scatter", "to_linear"):
            assert kinds[k] == det[k] + (k == "to_linear" and task == "seg"), (k, kinds[k], det[k])


@pytest.mark.parametrize("task", ["seg", "pose", "obb"])
def test_yolov8_task_plans_keep_the_plugin(task):
    """Implicit-batch (YOLOv8) task engines lower as before: the generic tail and the plugin"""
    tid, nc, _ = TASKS[task]
    path, _ = synth_wts(f"yolov8n_{task}")
    low = engine.describe_plan(engine.build_plan("yolov8n", path, batch=2, h=128, w=128, fp16=1, task=tid, classes=nc), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["plugin"] == 1 and kinds["yolo_task_head"] == 0 and kinds["yolo_head"] == 0


@pytest.mark.parametrize("fp16", [1, 0])
def test_yolo11_det_plans_keep_the_det_head(fp16):
    path, _ = yolo11_wts("n")
    low = engine.describe_plan(engine.build_plan("yolo11n", path, batch=2, h=128, w=128, fp16=fp16), lowered=True)
    kinds = collections.Counter(o["kind"] for o in low["ops"])
    assert kinds["yolo_head"] == 1 and kinds["yolo_task_head"] == 0 and kinds["plugin"] == 0


@pytest.mark.parametrize("task", [5, -1])
def test_yolo11_unknown_task_is_rejected(task):
    path, _ = yolo11_wts("n")
    with pytest.raises(RuntimeError):
        engine.build_plan("yolo11n", path, batch=1, h=128, w=128, task=task)


@pytest.mark.parametrize("scale", ["s", "l", "x"])
def test_every_yolo11_scale_builds_every_task(scale):
    for task in ("seg", "pose", "obb", "cls"):
        path, _ = task_wts(scale, task)
        S = 224 if task == "cls" else 128
        low = engine.describe_plan(engine.build_plan("yolo11" + scale, path, batch=1, h=S, w=S, fp16=1, task=TASKS[task][0]), lowered=True)
        assert low["n_ops"] > 0


def test_yolo11_det_plan_bytes_are_pinned(monkeypatch):
    """The det builder shares its graph with seg / pose / obb: the serialized det plans (no tactics: TRTX_TUNE=0) are the bytes recorded
    before that refactor"""
    monkeypatch.setenv("TRTX_TUNE", "0")
    with open(os.path.join(ROOT, "tests", "golden", "yolo11_det_plan_sha256.json")) as f:
        pinned = json.load(f)
    for key, want in pinned.items():
        scale, opts = key.split(" ", 1)
        kw = {k: int(v) for k, v in (p.split("=") for p in opts.split(";"))}
        path, _ = yolo11_wts(scale)
        assert hashlib.sha256(engine.build_plan("yolo11" + scale, path, **kw)).hexdigest() == want, key


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_yolo_decode_unit_passes_no_barrier_with_lds_reads_in_flight():
    """tools/isa_barrier_reads.py on plugins/yolo_decode.hip (the task head's score pass compacts its survivors in LDS between
    barriers), compiled with the flags the runtime Makefile gives plugins/*.hip (-ffp-contract=off), so the scanned code is what ships"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_barrier_reads as scan
    csrc = os.path.join(ROOT, "tensorrtx_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "yolo_decode.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{os.path.join(ROOT, 'include')}",
                               f"-I{csrc}", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", out,
                               os.path.join(csrc, "plugins", "yolo_decode.hip")], stderr=subprocess.DEVNULL)
        n, bad = scan.scan(out)
        assert n > 0
        assert not bad, f"barrier reached with LDS reads in flight in {bad}"
