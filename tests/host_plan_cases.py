"""What trtx_host_build answers, pinned per model: the serialized plan (tests/golden/host_plan_digests.json, recorded by
tests/golden/make_host_plan_golden.py) and the status of the calls it refuses.  The host builders (tensorrtx_amd/host/*.cpp) share their
blocks, their build session and their option parsing; these cases are what keeps a change to the shared pieces from moving a layer, a
Dims rank, a setter or an error code of any family.  CPU only: the shim serializes a network without a GPU.

Test infrastructure: nothing here is imported by the product.
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(HERE, "golden", "host_plan_digests.json")
OK, INVALID, UNSUPPORTED = 0, 1, 4   # TRTX_OK, TRTX_ERR_INVALID, TRTX_ERR_UNSUPPORTED


# ---- weights: the seeded synthetic files of the per-family CPU tests (one cache, one file per model), and small variants of them ----------

def _state_file(tag, make_state):
    from tensorrtx_amd import wts as wts_writer
    from util import CACHE
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, f"hostplan_{tag}_v1.wts")
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        wts_writer.write_wts(tmp, make_state(), dialect="double")
        os.replace(tmp, path)
    return path


def _short_anchor_grid(state_fn, key):
    """a detect layer whose anchor_grid holds two levels for three detect convolutions: the builders' null path"""
    def make():
        sd = state_fn()
        sd[key] = sd[key][:2]
        return sd
    return make


def weights(spec):
    """spec = (kind, *args) -> path of the .wts file"""
    from tensorrtx_amd import synth
    kind, a = spec[0], spec[1:]
    if kind == "util":          # lenet, resnet50, retinaface_r50, rcnn_r50c4, yolov8n and its task variants
        from util import synth_wts
        return synth_wts(a[0])[0]
    if kind == "yolo11":        # (scale, task name or None)
        if a[1] is None:
            from test_yolo11_cpu import yolo11_wts
            return yolo11_wts(a[0])[0]
        from test_yolo11_tasks_cpu import task_wts
        return task_wts(a[0], a[1])[0]
    if kind == "yolo11_nc":     # (scale, classes)
        return _state_file(f"yolo11{a[0]}_nc{a[1]}", lambda: synth.yolo11_state(a[0], num_class=a[1]))
    if kind == "yolo12":
        from test_yolo12_cpu import yolo12_wts
        return yolo12_wts(a[0])[0]
    if kind == "yolo12_nc":
        return _state_file(f"yolo12{a[0]}_nc{a[1]}", lambda: synth.yolo12_state(a[0], num_class=a[1]))
    if kind == "yolov5":        # ("n" / "n6", task name or None)
        if a[1] is None:
            from test_yolov5_cpu import yolov5_wts
            return yolov5_wts(a[0])[0]
        from test_yolov5_tasks_cpu import task_wts
        return task_wts(a[0], a[1])[0]
    if kind == "yolov5_nc":
        return _state_file(f"yolov5{a[0]}_nc{a[1]}", lambda: synth.yolov5_state(a[0], num_class=a[1]))
    if kind == "yolov5_short":
        return _state_file("yolov5n_short", _short_anchor_grid(lambda: synth.yolov5_state("n"), "model.24.anchor_grid"))
    if kind == "yolov9":        # (name, converted)
        from test_yolov9_cpu import yolov9_wts
        return yolov9_wts(a[0], a[1])[0]
    if kind == "yolov9_nc":
        return _state_file(f"{a[0]}_nc{a[1]}", lambda: synth.yolov9_state(a[0], num_class=a[1]))
    if kind == "yolov7":        # (name, classes)
        from test_yolov7_cpu import yolov7_wts
        return yolov7_wts(a[0], num_class=a[1])[0]
    if kind == "yolov7_short":
        return _state_file("yolov7tiny_short", _short_anchor_grid(lambda: synth.yolov7_state("yolov7tiny"), "model.77.anchor_grid"))
    if kind == "darknet":       # (name, classes)
        from test_darknet_cpu import darknet_wts
        return darknet_wts(a[0], num_class=a[1])[0]
    if kind == "yolov10":
        from test_yolov10_cpu import yolov10_wts
        return yolov10_wts(a[0])[0]
    if kind == "yolov10_nc":
        return _state_file(f"{a[0]}_nc{a[1]}", lambda: synth.yolov10_state(a[0], num_class=a[1]))
    raise KeyError(spec)


# ---- plans ------------------------------------------------------------------------------------------------------------------------

def _c(model, wts, **opts):
    return dict(model=model, wts=wts, opts=opts)


# Sizes are the smallest each family accepts (64 for three levels, 128 for the P6 models); the plan of a network does not get more
# interesting with the image.  lenet / resnet50 / retinaface / rcnn take the options of tests/ref_builder_cases.py.
PLAN_CASES = {
    "lenet": _c("lenet", ("util", "lenet"), batch=1),
    "lenet_b4": _c("lenet", ("util", "lenet"), batch=4),
    "resnet50": _c("resnet50", ("util", "resnet50"), batch=1, fp16=0, h=224, w=224),
    "resnet50_fp16_b3_96x64": _c("resnet50", ("util", "resnet50"), batch=3, fp16=1, h=96, w=64),
    "retinaface_r50": _c("retinaface_r50", ("util", "retinaface_r50"), batch=1, fp16=1, h=480, w=640),
    "retinaface_r50_int8": dict(model="retinaface_r50", wts=("util", "retinaface_r50"), opts=dict(batch=1, fp16=0, int8=1, h=480, w=640),
                                calib="retinaface_r50_int8"),   # the calibration table of ref_builder_cases
    "retinaface_r50_fp32_b3_64x96": _c("retinaface_r50", ("util", "retinaface_r50"), batch=3, fp16=0, h=64, w=96),
    "rcnn_r50c4": _c("rcnn_r50c4", ("util", "rcnn_r50c4"), batch=1, fp16=1, h=800, w=1067),
    "rcnn_r50c4_mask": _c("rcnn_r50c4", ("util", "rcnn_r50c4"), batch=1, fp16=1, h=800, w=1067, mask=1),
    "rcnn_r50c4_fp32_b3_stages": _c("rcnn_r50c4", ("util", "rcnn_r50c4"), batch=3, fp16=0, h=128, w=160, mark_stages=1, detections=50),
    # YOLOv8n, tasks 0 - 3 (pose: 1 class, obb: 15 classes)
    "yolov8n_det": _c("yolov8n", ("util", "yolov8n"), batch=1, fp16=1, h=64, w=64),
    "yolov8n_seg": _c("yolov8n", ("util", "yolov8n_seg"), batch=1, fp16=1, h=64, w=64, task=1),
    "yolov8n_pose": _c("yolov8n", ("util", "yolov8n_pose"), batch=1, fp16=1, h=64, w=64, task=2, classes=1),
    "yolov8n_obb": _c("yolov8n", ("util", "yolov8n_obb"), batch=1, fp16=1, h=64, w=64, task=3, classes=15),
    "yolov8n_heads_fp32_b3": _c("yolov8n", ("util", "yolov8n_obb"), batch=3, fp16=0, h=64, w=96, task=3, classes=15, max_out=300, mark_heads=1),
    # YOLO11, tasks 0 - 4, and the c3k switch of m
    "yolo11n_det": _c("yolo11n", ("yolo11", "n", None), batch=1, fp16=1, h=64, w=64),
    "yolo11n_seg": _c("yolo11n", ("yolo11", "n", "seg"), batch=1, fp16=1, h=64, w=64, task=1),
    "yolo11n_pose": _c("yolo11n", ("yolo11", "n", "pose"), batch=1, fp16=1, h=64, w=64, task=2),
    "yolo11n_obb": _c("yolo11n", ("yolo11", "n", "obb"), batch=1, fp16=1, h=64, w=64, task=3),
    "yolo11n_cls": _c("yolo11n", ("yolo11", "n", "cls"), batch=1, fp16=1, h=64, w=64, task=4),
    "yolo11m_det": _c("yolo11m", ("yolo11", "m", None), batch=1, fp16=1, h=64, w=64),
    "yolo11n_heads_fp32_b3": _c("yolo11n", ("yolo11_nc", "n", 7), batch=3, fp16=0, h=96, w=64, classes=7, max_out=300, mark_heads=1),
    "yolo11n_cls_fp32_b3": _c("yolo11n", ("yolo11", "n", "cls"), batch=3, fp16=0, h=64, w=96, task=4),
    # YOLOv12: 64 x 64 gives a 4 x 4 stride-16 grid, which the area count 4 divides; so does 96 x 32 (6 x 2)
    "yolo12n": _c("yolo12n", ("yolo12", "n"), batch=1, fp16=1, h=64, w=64),
    "yolo12n_heads_fp32_b3": _c("yolo12n", ("yolo12_nc", "n", 7), batch=3, fp16=0, h=96, w=32, classes=7, max_out=300, mark_heads=1),
    # YOLOv5: det / seg / cls and a P6 model
    "yolov5n_det": _c("yolov5n", ("yolov5", "n", None), batch=1, fp16=1, h=64, w=64),
    "yolov5n_seg": _c("yolov5n", ("yolov5", "n", "seg"), batch=1, fp16=1, h=64, w=64, task=1),
    "yolov5n_cls": _c("yolov5n", ("yolov5", "n", "cls"), batch=1, fp16=1, h=64, w=64, task=4),
    "yolov5n6": _c("yolov5n6", ("yolov5", "n6", None), batch=1, fp16=1, h=128, w=128),
    "yolov5n_heads_fp32_b3": _c("yolov5n", ("yolov5_nc", "n", 7), batch=3, fp16=0, h=64, w=96, classes=7, max_out=300, mark_heads=1),
    # YOLOv9: ELAN1 (t), converted, the auxiliary branch with first = 1 (unconverted m), ADown (gelan-c)
    "yolov9t": _c("yolov9t", ("yolov9", "yolov9t", 0), batch=1, fp16=1, h=64, w=64),
    "yolov9t_converted": _c("yolov9t", ("yolov9", "yolov9t", 1), batch=1, fp16=1, h=64, w=64, converted=1),
    "yolov9m": _c("yolov9m", ("yolov9", "yolov9m", 0), batch=1, fp16=1, h=64, w=64),
    "gelanc": _c("gelanc", ("yolov9", "gelanc", 0), batch=1, fp16=1, h=64, w=64),
    "yolov9t_heads_fp32_b3": _c("yolov9t", ("yolov9_nc", "yolov9t", 7), batch=3, fp16=0, h=64, w=96, classes=7, max_out=300, mark_heads=1),
    # YOLOv7: Leaky + eps 1e-5 (tiny), RepConv (v7), ReOrg (w6), DownC (e6)
    "yolov7tiny": _c("yolov7tiny", ("yolov7", "yolov7tiny", 80), batch=1, fp16=1, h=64, w=64),
    "yolov7": _c("yolov7", ("yolov7", "yolov7", 80), batch=1, fp16=1, h=64, w=64),
    "yolov7w6": _c("yolov7w6", ("yolov7", "yolov7w6", 80), batch=1, fp16=1, h=128, w=128),
    "yolov7e6": _c("yolov7e6", ("yolov7", "yolov7e6", 80), batch=1, fp16=1, h=128, w=128),
    "yolov7tiny_heads_fp32_b3": _c("yolov7tiny", ("yolov7", "yolov7tiny", 7), batch=3, fp16=0, h=96, w=64, classes=7, max_out=300, mark_heads=1),
    # Darknet
    "yolov3": _c("yolov3", ("darknet", "yolov3", 80), batch=1, fp16=1, h=64, w=64),
    "yolov3-tiny": _c("yolov3-tiny", ("darknet", "yolov3-tiny", 80), batch=1, fp16=1, h=64, w=64),
    "yolov4": _c("yolov4", ("darknet", "yolov4", 80), batch=1, fp16=1, h=64, w=64),
    "yolov3-tiny_heads_fp32_b3": _c("yolov3-tiny", ("darknet", "yolov3-tiny", 7), batch=3, fp16=0, h=64, w=96, classes=7, mark_heads=1),
    # YOLOv10: the three stage kinds (n: C2F + lk, s, m: C2fCIB without lk) and x
    "yolov10n": _c("yolov10n", ("yolov10", "yolov10n"), batch=1, fp16=1, h=64, w=64),
    "yolov10s": _c("yolov10s", ("yolov10", "yolov10s"), batch=1, fp16=1, h=64, w=64),
    "yolov10m": _c("yolov10m", ("yolov10", "yolov10m"), batch=1, fp16=1, h=64, w=64),
    "yolov10x": _c("yolov10x", ("yolov10", "yolov10x"), batch=1, fp16=1, h=64, w=64),
    "yolov10n_heads_fp32_b3": _c("yolov10n", ("yolov10_nc", "yolov10n", 7), batch=3, fp16=0, h=96, w=64, classes=7, max_out=300, mark_heads=1),
}


def build(case):
    from tensorrtx_amd import engine
    c = PLAN_CASES[case]
    path = weights(c["wts"])
    if "calib" in c:
        from tensorrtx_amd import calibrator
        from tests import ref_builder_cases as rb
        with calibrator.Calibrator(cache=rb.calibration_table(c["calib"])).installed():
            return engine.build_plan(c["model"], path, **c["opts"])
    return engine.build_plan(c["model"], path, **c["opts"])


def wts_sha(case):
    with open(weights(PLAN_CASES[case]["wts"]), "rb") as f:
        h = hashlib.sha256()
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- statuses ---------------------------------------------------------------------------------------------------------------------

_W = {   # one small weights file per family; most refusals come before it is opened
    "lenet": ("util", "lenet"), "yolov8n": ("util", "yolov8n"), "yolo11": ("yolo11", "n", None), "yolo12": ("yolo12", "n"),
    "yolov5": ("yolov5", "n", None), "yolov9": ("yolov9", "yolov9t", 0), "yolov7": ("yolov7", "yolov7tiny", 80),
    "darknet": ("darknet", "yolov3-tiny", 80), "yolov10": ("yolov10", "yolov10n"),
}


def _s(status, model, fam, **opts):
    return (model, opts, _W[fam], status)


# (model, options, weights, status): read off the parent of the change that introduced the family table, and kept
STATUS_CASES = [
    # names no family knows
    _s(INVALID, "yolov10q", "yolov10"), _s(INVALID, "yolov10", "yolov10"), _s(INVALID, "yolo11q", "yolo11"), _s(INVALID, "yolo12q", "yolo12"),
    _s(INVALID, "yolov5q", "yolov5"), _s(INVALID, "yolov5n7", "yolov5"), _s(INVALID, "yolov9x", "yolov9"), _s(INVALID, "yolov7s", "yolov7"),
    _s(INVALID, "yolov3-spp", "darknet"), _s(INVALID, "", "lenet"), _s(INVALID, None, "lenet"),
    _s(INVALID, "yolov10q", "yolov10", int8=1),       # the unknown letter answers before int8 is looked at
    _s(INVALID, "yolov9x", "yolov9", int8=1),
    _s(INVALID, "yolov9c", "yolov9", converted=1, h=64, w=64),
    # int8 on a family without it: UNSUPPORTED, before any size or task check
    _s(UNSUPPORTED, "yolov9t", "yolov9", int8=1, h=64, w=64), _s(UNSUPPORTED, "yolov9t", "yolov9", int8=1, h=100), _s(UNSUPPORTED, "yolov9t", "yolov9", int8=1, task=1),
    _s(UNSUPPORTED, "yolov7tiny", "yolov7", int8=1, h=64, w=64), _s(UNSUPPORTED, "yolov7w6", "yolov7", int8=1, h=96), _s(UNSUPPORTED, "yolov7tiny", "yolov7", int8=1, task=1),
    _s(UNSUPPORTED, "yolov3-tiny", "darknet", int8=1, h=64, w=64), _s(UNSUPPORTED, "yolov4", "darknet", int8=1, h=100), _s(UNSUPPORTED, "yolov3", "darknet", int8=1, task=1),
    _s(UNSUPPORTED, "yolov10n", "yolov10", int8=1, h=64, w=64), _s(UNSUPPORTED, "yolov10n", "yolov10", int8=1, h=100), _s(UNSUPPORTED, "yolov10n", "yolov10", int8=1, task=1),
    _s(UNSUPPORTED, "yolov5n", "yolov5", int8=1, task=1, h=64, w=64), _s(UNSUPPORTED, "yolov5n", "yolov5", int8=1, task=4, h=100),
    _s(INVALID, "yolov5n6", "yolov5", int8=1, task=1),   # the task is refused first
    _s(INVALID, "yolo12n", "yolo12", int8=1, task=1),
    # a size the largest stride does not divide, or below it
    _s(INVALID, "yolov5n", "yolov5", h=100, w=64), _s(INVALID, "yolov5n", "yolov5", h=16, w=32), _s(INVALID, "yolov5n6", "yolov5", h=96, w=128),
    _s(INVALID, "yolov9t", "yolov9", h=64, w=72), _s(INVALID, "yolov7tiny", "yolov7", h=64, w=72), _s(INVALID, "yolov7w6", "yolov7", h=96, w=128),
    _s(INVALID, "yolov7e6", "yolov7", h=128, w=32), _s(INVALID, "yolov3-tiny", "darknet", h=100, w=64), _s(INVALID, "yolov10n", "yolov10", h=100, w=64),
    _s(INVALID, "yolov10n", "yolov10", h=16, w=32),
    # batch, classes, max_out below 1
    _s(INVALID, "yolo11n", "yolo11", batch=0, h=64, w=64), _s(INVALID, "yolo12n", "yolo12", batch=0, h=64, w=64),
    _s(INVALID, "yolov5n", "yolov5", batch=0, h=64, w=64), _s(INVALID, "yolov5n", "yolov5", classes=0, h=64, w=64), _s(INVALID, "yolov5n", "yolov5", max_out=0, h=64, w=64),
    _s(INVALID, "yolov9t", "yolov9", batch=0, h=64, w=64), _s(INVALID, "yolov9t", "yolov9", classes=0, h=64, w=64), _s(INVALID, "yolov9t", "yolov9", max_out=0, h=64, w=64),
    _s(INVALID, "yolov7tiny", "yolov7", batch=0, h=64, w=64), _s(INVALID, "yolov7tiny", "yolov7", classes=0, h=64, w=64), _s(INVALID, "yolov7tiny", "yolov7", max_out=0, h=64, w=64),
    _s(INVALID, "yolov3-tiny", "darknet", batch=0, h=64, w=64), _s(INVALID, "yolov3-tiny", "darknet", classes=0, h=64, w=64),
    _s(INVALID, "yolov3-tiny", "darknet", max_out=0, h=64, w=64), _s(INVALID, "yolov3-tiny", "darknet", max_out=999, h=64, w=64),
    _s(OK, "yolov3-tiny", "darknet", max_out=1000, h=64, w=64),
    _s(INVALID, "yolov10n", "yolov10", batch=0, h=64, w=64), _s(INVALID, "yolov10n", "yolov10", classes=0, h=64, w=64), _s(INVALID, "yolov10n", "yolov10", max_out=0, h=64, w=64),
    # a task outside the family's set
    _s(INVALID, "yolov8n", "yolov8n", task=4, h=64, w=64), _s(INVALID, "yolov8n", "yolov8n", task=-1, h=64, w=64),
    _s(INVALID, "yolo11n", "yolo11", task=5, h=64, w=64), _s(INVALID, "yolo11n", "yolo11", task=-1, h=64, w=64), _s(INVALID, "yolo12n", "yolo12", task=1, h=64, w=64),
    _s(INVALID, "yolov5n", "yolov5", task=2, h=64, w=64), _s(INVALID, "yolov5n", "yolov5", task=3, h=64, w=64), _s(INVALID, "yolov5n6", "yolov5", task=1, h=128, w=128),
    _s(INVALID, "yolov5n6", "yolov5", task=4, h=128, w=128), _s(INVALID, "yolov9t", "yolov9", task=1, h=64, w=64), _s(INVALID, "yolov7tiny", "yolov7", task=1, h=64, w=64),
    _s(INVALID, "yolov3-tiny", "darknet", task=1, h=64, w=64), _s(INVALID, "yolov10n", "yolov10", task=1, h=64, w=64),
    # null plans: YOLOv12's grid (3 x 3) that the area count does not divide and YOLOv7's anchor_grid are INVALID, YOLOv5's anchor_grid UNSUPPORTED
    _s(INVALID, "yolo12n", "yolo12", h=48, w=48),
    ("yolov7tiny", dict(h=64, w=64), ("yolov7_short",), INVALID),
    ("yolov5n", dict(h=64, w=64), ("yolov5_short",), UNSUPPORTED),
    # aux_streams outside [-1, 15], whatever the model
    _s(INVALID, "lenet", "lenet", aux_streams=16), _s(INVALID, "lenet", "lenet", aux_streams=-2), _s(INVALID, "yolov9t", "yolov9", aux_streams=16, h=64, w=64),
    _s(OK, "lenet", "lenet", aux_streams=15), _s(OK, "lenet", "lenet", aux_streams=-1),
]


def status_of(model, opts, wts_spec):
    """trtx_host_build's status, called directly so that a null model name can be passed"""
    from tensorrtx_amd import engine
    M = engine.models_lib()
    blob, size = ctypes.c_void_p(), ctypes.c_size_t()
    o = ";".join(f"{k}={int(v)}" for k, v in opts.items())
    st = M.trtx_host_build(None if model is None else model.encode(), weights(wts_spec).encode(), o.encode(), ctypes.byref(blob), ctypes.byref(size))
    if st == OK:
        M.trtx_host_free.argtypes = [ctypes.c_void_p]
        M.trtx_host_free(blob)
    return st
