"""Pins the oracle — and the product — on the REFERENCE'S OWN code.

oracle/_ref/ is built by oracle/ref_build.py from the sources under /root/reference (nothing copied into git):
  * libref_host.so   — the reference's host NMS functions (yolov8 postprocess.cpp, retinaface common.hpp), g++;
  * libref_<family>.so — the reference's CUDA plugins, unmodified, compiled by hipcc as user plugins against
    include/NvInfer.h, so the reference's kernels run on the MI355X behind the same plugin v-table the engine uses.
Their outputs on the seeded cases of tests/ref_cases.py / ref_host_cases.py are committed under tests/golden/
(make_ref_golden.py), so the oracle stays pinned where neither /root/reference nor oracle/_ref exists.

CPU tests: oracle == committed reference outputs; oracle/_ref (when present) reproduces the committed outputs.
GPU tests: product == live reference plugin == committed reference outputs; reference plugin inside a full engine;
blob layouts interchangeable with the reference's.
"""
import os

import numpy as np
import pytest

import ref_cases as rc
import ref_host_cases as hc
from oracle import det_post as dp
from oracle import ref
from oracle import yolo_post as yp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAVE_REFERENCE = os.path.isdir("/root/reference")


def _need_ref(name):
    """oracle/_ref travels with the working tree; it can only be (re)built where /root/reference exists."""
    if ref.available(name):
        return
    if HAVE_REFERENCE:
        from oracle import ref_build
        ref_build.build_all()
        assert ref.available(name)
        return
    pytest.skip(f"oracle/_ref/{name} not present and /root/reference absent (cannot be built here); the committed goldens still pin the oracle")


# ------------------------------------------------------------------------------------------------ CPU: host NMS
def test_oracle_yolov8_nms_equals_reference_outputs():
    """oracle/csrc/yolo_post_ref.c vs what yolov8/src/postprocess.cpp:94-121 itself returned (committed golden)."""
    z = np.load(os.path.join(GOLD, "ref_host_nms.npz"))
    for name, rows in hc.yolov8_cases().items():
        ki, kc, kd = yp.batch_nms_c(rows)
        for b in range(rows.shape[0]):
            want = z[f"yolov8/{name}/{b}"]
            assert kc[b] == len(want), (name, b, kc[b], len(want))
            assert np.array_equal(kd[b, :kc[b]], want, equal_nan=True), (name, b)
            # kept slot indices point at exactly those records
            rec = rows[b, 1:].reshape(-1, 90)[ki[b, :kc[b]], :6]
            assert np.array_equal(rec, want, equal_nan=True)


def test_oracle_retina_nms_equals_reference_outputs():
    z = np.load(os.path.join(GOLD, "ref_host_nms.npz"))
    for name, rows in hc.retina_cases().items():
        idx, cnt = dp.retina_nms(rows, max_keep=4096)
        for b in range(rows.shape[0]):
            want = z[f"retina/{name}/{b}"]
            assert cnt[b] == len(want), (name, b, cnt[b], len(want))
            rec = rows[b, 1:].reshape(-1, 15)[idx[b, :cnt[b]]]
            assert np.array_equal(rec, want), (name, b)


def test_oracle_yolov5_nms_equals_reference_outputs():
    """oracle/csrc/yolov5_post_ref.c vs what yolov5/src/postprocess.cpp:50-73 itself returned (committed golden)."""
    z = np.load(os.path.join(GOLD, "ref_host_nms.npz"))
    for name, rows in hc.yolov5_cases().items():
        ki, kc, kd = yp.v5_batch_nms_c(rows)
        for b in range(rows.shape[0]):
            want = z[f"yolov5/{name}/{b}"]
            assert kc[b] == len(want), (name, b, kc[b], len(want))
            assert np.array_equal(kd[b, :kc[b]], want, equal_nan=True), (name, b)
            assert np.array_equal(rows[b, 1:].reshape(-1, 38)[ki[b, :kc[b]], :6], want, equal_nan=True)


def test_reference_host_code_reproduces_the_goldens():
    """The committed fixture really is the reference's output: rerun libref_host.so (built from /root/reference)."""
    _need_ref("libref_host.so")
    z = np.load(os.path.join(GOLD, "ref_host_nms.npz"))
    for name, rows in hc.yolov8_cases().items():
        per = ref.yolov8_batch_nms(rows)
        for b in range(rows.shape[0]):
            assert np.array_equal(ref.yolov8_nms(rows[b])[:, :6], z[f"yolov8/{name}/{b}"], equal_nan=True)
            assert np.array_equal(per[b][:, :6], z[f"yolov8/{name}/{b}"], equal_nan=True)  # batch_nms == per-image nms
    for name, rows in hc.retina_cases().items():
        for b in range(rows.shape[0]):
            assert np.array_equal(ref.retina_nms(rows[b]), z[f"retina/{name}/{b}"])
    for name, rows in hc.yolov5_cases().items():
        for b in range(rows.shape[0]):
            assert np.array_equal(ref.yolov5_nms(rows[b])[:, :6], z[f"yolov5/{name}/{b}"], equal_nan=True)


def test_reference_yolov8_nms_random_sweep_against_oracle():
    """Beyond the committed cases: 40 random decode buffers (clustered boxes, 1-5 classes) through both - the reference's results are
    committed (ref_host_sweeps.npz) and rerun live where oracle/_ref exists."""
    z = np.load(os.path.join(GOLD, "ref_host_sweeps.npz"))
    live = ref.available("libref_host.so")
    for trial, row in enumerate(hc.yolov8_sweep_cases()):
        ki, kc, kd = yp.batch_nms_c(row)
        want = z[f"yolov8_sweep/{trial}"]
        if live:
            assert np.array_equal(ref.yolov8_nms(row[0])[:, :6], want), trial
        assert kc[0] == len(want) and np.array_equal(kd[0, :kc[0]], want), trial


# ------------------------------------------------------------------------------------------------ CPU: plugin goldens
def _plugin_golden():
    p = os.path.join(GOLD, "ref_plugins.npz")
    if not os.path.exists(p):
        pytest.skip("tests/golden/ref_plugins.npz not generated yet (needs one run of make_ref_golden.py plugins on the GPU box)")
    return np.load(p)


def _golden_outputs(z, case):
    keys = sorted((k for k in z.files if k.startswith(case.name + "/")), key=lambda s: int(s.rsplit("/", 1)[1]))
    assert keys, f"no golden for {case.name}: regenerate tests/golden/ref_plugins.npz"
    return [z[k] for k in keys]


@pytest.mark.parametrize("idx", range(len(rc.all_cases())))
def test_oracle_equals_reference_plugin_outputs(idx):
    """CPU restatement (oracle/csrc/*.c) vs the outputs the reference's own kernels produced on the MI355X."""
    z = _plugin_golden()
    case, _, oracle = rc.all_cases()[idx]
    want = _golden_outputs(z, case)
    got = case.canon(oracle(case))
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (case.name, k, a.shape, b.shape)
        if case.rtol or case.atol:
            assert np.allclose(a, b, rtol=case.rtol, atol=case.atol), (case.name, k, np.abs(a - b).max())
        else:
            assert np.array_equal(a, b), (case.name, k)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(rc.all_cases())))
def test_product_equals_live_reference_plugin(gpu, idx):
    """This repo's HIP kernel vs the reference's own kernel, both on the MI355X, same inputs, through the C ABI."""
    case, product, oracle = rc.all_cases()[idx]
    _need_ref(f"libref_{case.family}.so")
    want = rc.run_reference(case, gpu)
    got = product(case, gpu)
    rc.compare(case, got, want, "product vs reference plugin")
    rc.compare(case, oracle(case), want, "oracle vs reference plugin")


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(rc.all_cases())))
def test_product_equals_committed_reference_outputs(gpu, idx):
    z = _plugin_golden()
    case, product, _ = rc.all_cases()[idx]
    got = case.canon(product(case, gpu))
    want = _golden_outputs(z, case)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (case.name, k)
        if case.rtol or case.atol:
            assert np.allclose(a, b, rtol=case.rtol, atol=case.atol), (case.name, k, np.abs(a - b).max())
        else:
            assert np.array_equal(a, b), (case.name, k)


@pytest.mark.gpu
def test_reference_yololayer_plugin_runs_inside_a_full_engine(gpu):
    """Boundary (b): the UNMODIFIED reference plugin (yolov8/plugin/yololayer.{h,cu}) registered as a user plugin — as an
    application linking it would — is picked up by the host builder (getPluginCreator), cloned / configured /
    serialized / deserialized by the runtime through the NvInfer.h trampolines and enqueued inside the lowered plan.
    Its detections equal the built-in HIP plugin's (same fp32 engine, same input), as sets: the reference appends
    with atomicAdd."""
    import torch
    from tensorrtx_amd import engine, synth
    from util import synth_wts
    _need_ref("libref_yolov8_plugin.so")
    creators = ref.load_plugins("yolov8_plugin")
    path, _ = synth_wts("yolov8n")
    B, S = 2, 160
    x = torch.from_numpy(synth.images(B, S, S, seed=17)).to(gpu)

    def run(plan):
        e = engine.Engine(plan)
        bufs = [x if e.is_input[i] else torch.zeros(B * int(np.prod(e.dims[i])), dtype=torch.float32, device=gpu)
                for i in range(e.nb_bindings)]
        e.enqueue(B, bufs)
        torch.cuda.synchronize()
        out = bufs[e.names.index("output")].reshape(B, -1).cpu().numpy()
        e.close()
        return out

    builtin_plan = engine.build_plan("yolov8n", path, batch=B, h=S, w=S, fp16=0)
    builtin = ref.registry_get("YoloLayer_TRT")
    with ref.use_creator(creators["YoloLayer_TRT"]):
        # what getPluginCreator("YoloLayer_TRT", "1") in the host builder and deserializePlugin in the runtime resolve to
        assert ref.registry_get("YoloLayer_TRT").self == creators["YoloLayer_TRT"].self != builtin.self
        ref_plan = engine.build_plan("yolov8n", path, batch=B, h=S, w=S, fp16=0)
        kinds = [op["kind"] for op in engine.describe_plan(ref_plan, lowered=True)["ops"]]
        assert "plugin" in kinds and "yolo_head" not in kinds  # a user plugin: fp32 LINEAR edge, never fused
        got_ref = run(ref_plan)
    assert ref.registry_get("YoloLayer_TRT").self == builtin.self
    got_builtin = run(builtin_plan)
    a, b = rc.canon_records(got_ref, 90, 6), rc.canon_records(got_builtin, 90, 6)
    for ra, rb in zip(a, b):
        assert ra.shape == rb.shape and ra.shape[0] > 0
        assert np.array_equal(ra[:, :4], rb[:, :4]) and np.array_equal(ra[:, 5], rb[:, 5])
        assert np.allclose(ra[:, 4], rb[:, 4], rtol=0, atol=2e-7)


@pytest.mark.gpu
def test_plugin_blobs_are_interchangeable_with_the_reference(gpu):
    """SURVEY 8b 'plugin serialization blobs (must round-trip)': every blob the product's R-CNN plugin classes write
    into a plan is accepted by the reference's deserializePlugin and re-serializes to the same bytes, and the YoloLayer
    blob of the built-in plugin loads in the reference's YoloLayerPlugin(const void*, size_t) (asserts d == a + length)."""
    from tensorrtx_amd import engine
    from util import synth_wts
    _need_ref("libref_rcnn_plugins.so")
    _need_ref("libref_yolov8_plugin.so")
    rcnn = ref.load_plugins("rcnn_plugins")
    path, _ = synth_wts("rcnn_r50c4")
    plan = engine.build_plan("rcnn_r50c4", path, batch=1, fp16=1, h=320, w=416, mask=1)
    seen = set()
    for l in engine.describe_plan(plan)["layers"]:
        t = l.get("plugin_type")
        if not t:
            continue
        blob = bytes.fromhex(l["plugin_blob"])
        v = ref.make_plugin(rcnn[t], blob=blob)
        assert ref.plugin_blob(v) == blob, t
        v.destroy(v.self)
        seen.add(t)
    assert seen == {"RpnDecode", "RpnNms", "RoiAlign", "PredictorDecode", "BatchedNms", "MaskRcnnInference"}, seen
    ypath, _ = synth_wts("yolov8n")
    yplan = engine.build_plan("yolov8n", ypath, batch=1, h=64, w=64, fp16=1)
    yblob = [bytes.fromhex(l["plugin_blob"]) for l in engine.describe_plan(yplan)["layers"] if l.get("plugin_type") == "YoloLayer_TRT"][0]
    v = ref.make_plugin(ref.load_plugins("yolov8_plugin")["YoloLayer_TRT"], blob=yblob)
    assert ref.plugin_blob(v) == yblob
    v.destroy(v.self)


@pytest.mark.gpu
def test_gpu_postprocess_mode_equals_reference_kernels(gpu):
    """a5': trtx_yolo_postprocess_gpu vs the reference's cuda_decode + cuda_nms (yolov8/src/postprocess.cu, compiled
    unmodified by hipcc) on identical decode buffers; kept records compared as sets (atomicAdd slot order)."""
    import ctypes

    import torch
    from tensorrtx_amd import capi, synth
    _need_ref("libref_yolov8_post.so")
    L = ref.family_lib("yolov8_post")
    dec = yp.decode_c(synth.yolo_head_tensors(3, seed=23), 80, 640, 640, [8, 16, 32])
    d = torch.from_numpy(dec).to(gpu)
    got = capi.yolo_postprocess_gpu(d).cpu().numpy()
    for b in range(dec.shape[0]):
        out = torch.zeros(1 + 1000 * 7, dtype=torch.float32, device=gpu)
        L.ref_yolov8_gpu_postprocess(ctypes.c_void_p(d[b].data_ptr()), 1000, ctypes.c_float(0.5), ctypes.c_float(0.45),
                                     ctypes.c_void_p(out.data_ptr()), 1000, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        want = out.cpu().numpy()
        assert got[b, 0] == want[0]
        n = int(want[0])
        gr = got[b, 1:1 + n * 7].reshape(n, 7)
        wr = want[1:1 + n * 7].reshape(n, 7)
        for keep in (1.0, 0.0):  # kept and suppressed records, and the all-zero slots of sub-threshold candidates
            assert np.array_equal(rc._sorted_rows(gr[gr[:, 6] == keep]), rc._sorted_rows(wr[wr[:, 6] == keep]))
        assert (wr[:, 6] == 1.0).sum() > 20


@pytest.mark.gpu
def test_reference_racy_kernels_at_full_size_are_reported_not_asserted(gpu):
    """rpnNms at 6000 proposals: the reference launches 6 blocks that synchronise with __syncthreads only
    (RpnNms.cu:93-110), so its output depends on block scheduling.  The product implements the intended exact greedy
    semantics (== the single-block reference, asserted in the cases above); here the overlap with the racy full-size
    run is measured and logged."""
    import json
    _need_ref("libref_rcnn_plugins.so")
    import struct

    from tensorrtx_amd import synth
    anchors = dp.generate_anchors()
    s, d = synth.rcnn_rpn_tensors(2, 15, 50, 84, seed=9)
    rs, rb = dp.rpn_decode(s.reshape(2, -1), d.reshape(2, -1), 50, 84, 800, 1333, 16.0, anchors, 6000)
    case = rc.Case("rpn_nms_6000_1000", "rcnn_plugins", "RpnNms", 2, [rs.reshape(2, 6000, 1), rb], [(2, 1000, 4)],
                   blob=struct.pack("<fiQ", 0.7, 1000, 6000), ref_exact=False, per_image=True)
    case.p = (6000, 1000)
    want = rc.run_reference(case, gpu)[0]
    got = rc.rpn_nms_product(case, gpu)[0]
    same = float(np.mean([np.array_equal(got[b, i], want[b, i]) for b in range(2) for i in range(1000)]))
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/parity_metrics.jsonl", "a") as f:
        f.write(json.dumps(dict(test="rpn_nms_6000_vs_racy_reference", rows_identical=same)) + "\n")
    assert np.array_equal(got, rc.rpn_nms_oracle(case)[0])
    assert same > 0.2  # informational: the racy reference still agrees on a large part of the list


@pytest.mark.gpu
def test_builtin_mish_equals_the_reference_kernel_bit_for_bit(gpu):
    """g1: the product's Mish_TRT (trtx_mish) vs the reference's mish_kernel (yolov4/mish.cu:119-135, compiled by hipcc into
    oracle/_ref/libref_yolov4_plugin.so), same inputs, both through the plugin v-table: the same device expf / logf, so NOT ONE bit may
    differ; blobs interchange (int input_size); the reference object's null version string (mish.cu:92-95) reads as "1"."""
    _need_ref("libref_yolov4_plugin.so")
    case = rc.mish_case(batch=3, shape=(8, 33, 17), seed=5)
    want = rc.run_reference(case, gpu)
    got = rc.mish_product(case, gpu)
    gu, wu = got[0].view(np.int32).astype(np.int64), want[0].view(np.int32).astype(np.int64)
    diff = np.abs(gu - wu)
    diff[(got[0] == 0) & (want[0] == 0)] = 0      # +0 / -0
    assert diff.max() == 0, f"{int((diff > 0).sum())} of {diff.size} elements differ, by up to {int(diff.max())} ulp; first at x = {case.inputs[0].ravel()[int(diff.argmax())]!r}"
    creators = ref.load_plugins("yolov4_plugin")
    ours = ref.make_plugin(ref.registry_get("Mish_TRT"), fields=[])
    assert ours.plugin_version(ours.self) == b"1"
    assert len(ref.plugin_blob(ours)) == 4
    a = ref.make_plugin(ref.registry_get("Mish_TRT"), blob=case.blob)
    b = ref.make_plugin(creators["Mish_TRT"], blob=case.blob)
    assert ref.plugin_blob(a) == case.blob, "our plugin does not re-serialize the reference's blob"
    assert ref.plugin_blob(b) == case.blob, "the reference plugin does not re-serialize its own blob"
    for v in (ours, a, b):
        v.destroy(v.self)
