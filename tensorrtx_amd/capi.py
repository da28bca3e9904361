"""ctypes binding of the C ABI in include/trtx_hip.h (section 1: plugin operators + single kernels)."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class TrtxError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        msg = lib().trtx_status_string(status).decode() if _LIB is not None else "?"
        super().__init__(f"{what}: status {status} ({msg})")


def lib_path() -> str:
    # TRTX_HIP_LIB: another BUILD of this same library (A/B measurements of kernel changes on one box); never a different implementation
    return os.environ.get("TRTX_HIP_LIB") or os.path.join(_HERE, "lib", "libtrtx_hip.so")


def hip_runtimes_mapped():
    """Paths of every libamdhip64 mapped into this process (must be exactly one once lib() has run)."""
    seen = []
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.rsplit(" ", 1)[-1].strip()
            if "libamdhip64" in os.path.basename(path) and path not in seen:
                seen.append(path)
    return seen


def _bind_hip_runtime():
    """libtrtx_hip.so NEEDs `libamdhip64.so.7` and PyTorch-ROCm bundles its own copy under torch/lib with the
    same SONAME.  Whichever copy is mapped first satisfies the other's NEEDED entry *only* in the torch-first
    order (torch dlopens its copy by path; ours is looked up by SONAME).  Two runtimes in one process each own a
    separate device table: torch sees the GPU, trtx_device_count() in the other does not.  So the binding always
    brings torch's runtime in first; a process that never uses torch (pure C++ callers) links the system ROCm."""
    import torch  # noqa: F401  (maps torch/lib/libamdhip64.so; plumbing only)


def lib() -> ctypes.CDLL:
    """Load libtrtx_hip.so.  Fails loudly when the extension has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _bind_hip_runtime()
        L = ctypes.CDLL(p)
        rts = hip_runtimes_mapped()
        if len(rts) > 1:
            raise ImportError("two HIP runtimes are mapped in this process (%s): something dlopened a HIP library "
                              "before tensorrtx_amd/torch; import torch (or tensorrtx_amd) first" % ", ".join(rts))
        L.trtx_status_string.restype = ctypes.c_char_p
        L.trtx_status_string.argtypes = [ctypes.c_int32]
        L.trtx_yolo_decode_workspace.restype = ctypes.c_size_t
        _LIB = L
    return _LIB


def check(status, what):
    if status != 0:
        raise TrtxError(status, what)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


DET_FLOATS = 90  # yolov8/include/types.h:4-12


def yolo_decode(inputs, classes, net_h, net_w, strides, max_out=1000, out=None):
    """YoloLayerPlugin::enqueue replacement (yolov8/plugin/yololayer.cu:167-316).
    inputs: list of CUDA fp32 tensors [B, 4+classes, gh*gw]. Returns [B, 1+max_out*90] fp32."""
    import torch
    L = lib()
    B = inputs[0].shape[0]
    n = len(inputs)
    ins = [x.contiguous() for x in inputs]
    for x in ins:
        assert x.is_cuda and x.dtype == torch.float32
    arr = (ctypes.c_void_p * n)(*[x.data_ptr() for x in ins])
    st = (ctypes.c_int * n)(*strides)
    ws_bytes = L.trtx_yolo_decode_workspace(B, net_h, net_w, st, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ins[0].device)
    if out is None:
        out = torch.empty((B, 1 + max_out * DET_FLOATS), dtype=torch.float32, device=ins[0].device)
    check(L.trtx_yolo_decode(arr, n, B, classes, net_h, net_w, st, max_out, _p(out), _p(ws),
                             ctypes.c_size_t(ws_bytes), _stream()), "trtx_yolo_decode")
    return out


def _nms_buffers(B, max_out, det_out, dev, out, ws, with_dets=True):
    """keep_idx, keep_cnt, keep_det and the workspace of an NMS call: the caller's (`out` = the three tensors, `ws` = a uint8 tensor) or new ones"""
    import torch
    L = lib()
    L.trtx_yolo_nms_workspace.restype = ctypes.c_size_t
    if out is None:
        out = (torch.full((B, max_out), -1, dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev),
               torch.zeros((B, max_out, det_out), dtype=torch.float32, device=dev) if with_dets else None)
    if ws is None:
        ws = torch.empty((L.trtx_yolo_nms_workspace(B),), dtype=torch.uint8, device=dev)
    keep_idx, keep_cnt, keep_det = out
    return keep_idx, keep_cnt, keep_det, ws


def yolo_nms(decode_out, max_out=1000, conf_thresh=0.5, nms_thresh=0.45, with_dets=True, out=None, ws=None):
    """batch_nms replacement (yolov8/src/postprocess.cpp:71-129). Returns keep_idx, keep_cnt, keep_det."""
    L = lib()
    B = decode_out.shape[0]
    keep_idx, keep_cnt, keep_det, ws = _nms_buffers(B, max_out, 6, decode_out.device, out, ws, with_dets)
    check(L.trtx_yolo_nms(_p(decode_out), B, max_out, ctypes.c_float(conf_thresh), ctypes.c_float(nms_thresh),
                          _p(keep_idx), _p(keep_cnt), _p(keep_det), _p(ws), ctypes.c_size_t(ws.numel()), _stream()),
          "trtx_yolo_nms")
    return keep_idx, keep_cnt, keep_det


def yolo_decode_ex(inputs, classes, net_h, net_w, strides, max_out=1000, nk=17, kpt_conf=0.0, seg=False, pose=False, obb=False):
    """YoloLayerPlugin::enqueue with the seg / pose / obb branches (yolov8/plugin/yololayer.cu:178-279)."""
    import torch
    L = lib()
    B, n = inputs[0].shape[0], len(inputs)
    ins = [x.contiguous() for x in inputs]
    arr = (ctypes.c_void_p * n)(*[x.data_ptr() for x in ins])
    st = (ctypes.c_int * n)(*strides)
    ws_bytes = L.trtx_yolo_decode_workspace(B, net_h, net_w, st, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ins[0].device)
    out = torch.zeros((B, 1 + max_out * DET_FLOATS), dtype=torch.float32, device=ins[0].device)
    check(L.trtx_yolo_decode_ex(arr, n, B, classes, net_h, net_w, st, max_out, nk, ctypes.c_float(kpt_conf), int(seg), int(pose), int(obb),
                                _p(out), _p(ws), ctypes.c_size_t(ws_bytes), _stream()), "trtx_yolo_decode_ex")
    return out


def _head_table(tensors):
    n = len(tensors)
    return (ctypes.c_void_p * n)(*[x.data_ptr() for x in tensors]), (ctypes.c_int * n)(*[x.shape[-1] for x in tensors])


def yolo_head_decode_workspace(batch, net_h, net_w, strides):
    L = lib()
    L.trtx_yolo_head_decode_workspace.restype = ctypes.c_size_t
    return L.trtx_yolo_head_decode_workspace(batch, net_h, net_w, (ctypes.c_int * len(strides))(*strides), len(strides))


def _head_call(heads, net_h, net_w, strides, max_out, out, ws, batch, n_levels):
    """What the two fused-head wrappers share: the batch, the stride table (None: a null pointer), the level count passed, `out` and `ws`"""
    import torch
    B, n, dev = heads[0].shape[0] if batch is None else batch, len(heads), heads[0].device
    st = None if strides is None else (ctypes.c_int * len(strides))(*strides)
    if ws is None:
        ws = torch.empty(max(yolo_head_decode_workspace(B, net_h, net_w, strides), 256), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.zeros(B, 1 + max_out * DET_FLOATS, dtype=torch.float32, device=dev)
    return B, n if n_levels is None else n_levels, st, out, ws


def yolo_head_decode_nhwc(heads, classes, net_h, net_w, strides, dfl_w, max_out=1000, out=None, ws=None, batch=None, ld=None, n_levels=None,
                          status_only=False):
    """The fused det head on NHWC head tensors [B, gh, gw, ld] (fp16 or fp32): trtx_yolo_head_decode_nhwc{,_f32}.
    `out` / `ws`: the caller's buffers; `batch`, `ld`, `n_levels`: what is passed instead of the tensors' own; `strides` / `dfl_w` None: a
    null pointer; `status_only`: return the status code instead of raising (the refusal tests; a failure otherwise raises TrtxError)."""
    import torch
    L = lib()
    hp, hl = _head_table(heads)
    if ld is not None:
        hl = (ctypes.c_int * len(ld))(*ld)
    B, n, st, out, ws = _head_call(heads, net_h, net_w, strides, max_out, out, ws, batch, n_levels)
    fn = L.trtx_yolo_head_decode_nhwc_f32 if heads[0].dtype == torch.float32 else L.trtx_yolo_head_decode_nhwc
    status = fn(hp, hl, n, B, classes, net_h, net_w, st, _p(dfl_w), max_out, _p(out), _p(ws), ctypes.c_size_t(ws.numel()), _stream())
    if status_only:
        return status
    check(status, "trtx_yolo_head_decode_nhwc")
    return out


def yolo_task_head_decode_nhwc(heads, branches, classes, net_h, net_w, strides, dfl_w, max_out=1000, nk=17, kpt_conf=0.0, seg=False,
                               pose=False, obb=False, out=None, ws=None, batch=None, ld=None, branch_ld=None, n_levels=None, status_only=False):
    """The fused YOLO11 task head (trtx_yolo_task_head_decode_nhwc{,_f32}): NHWC head tensors [B, gh, gw, ld] and branch tensors
    [B, gh, gw, branch_ld], fp16 or fp32; output rows as yolo_decode_ex.  The keyword arguments behind `obb` as in yolo_head_decode_nhwc."""
    import torch
    L = lib()
    hp, hl = _head_table(heads)
    bp, bl = _head_table(branches)
    if ld is not None:
        hl = (ctypes.c_int * len(ld))(*ld)
    if branch_ld is not None:
        bl = (ctypes.c_int * len(branch_ld))(*branch_ld)
    B, n, st, out, ws = _head_call(heads, net_h, net_w, strides, max_out, out, ws, batch, n_levels)
    fn = L.trtx_yolo_task_head_decode_nhwc_f32 if heads[0].dtype == torch.float32 else L.trtx_yolo_task_head_decode_nhwc
    status = fn(hp, hl, bp, bl, n, B, classes, net_h, net_w, st, _p(dfl_w), max_out, int(seg), int(pose), int(obb), nk, ctypes.c_float(kpt_conf),
                _p(out), _p(ws), ctypes.c_size_t(ws.numel()), _stream())
    if status_only:
        return status
    check(status, "trtx_yolo_task_head_decode_nhwc")
    return out


def yolo_nms_obb(decode_out, max_out=1000, conf_thresh=0.5, nms_thresh=0.45, out=None, ws=None):
    """nms_obb replacement (yolov8/src/postprocess.cpp:303-393).  keep_det: [B, max_out, 7] = cx, cy, w, h, conf, cls, angle."""
    L = lib()
    B = decode_out.shape[0]
    keep_idx, keep_cnt, keep_det, ws = _nms_buffers(B, max_out, 7, decode_out.device, out, ws)
    check(L.trtx_yolo_nms_obb(_p(decode_out), B, max_out, ctypes.c_float(conf_thresh), ctypes.c_float(nms_thresh), _p(keep_idx), _p(keep_cnt),
                              _p(keep_det), _p(ws), ctypes.c_size_t(ws.numel()), _stream()), "trtx_yolo_nms_obb")
    return keep_idx, keep_cnt, keep_det


def yolo_postprocess_gpu_obb(decode_out, max_out=1000, conf_thresh=0.5, nms_thresh=0.45, out=None, ws=None):
    """The reference's GPU mode for oriented boxes (yolov8/src/postprocess.cu: decode_kernel_obb + nms_kernel_obb): [B, 1 + max_out*8].
    `out`: the caller's buffer; `ws`: accepted like the NMS wrappers' and not used (this entry point takes no workspace)."""
    import torch
    if out is None:
        out = torch.empty((decode_out.shape[0], 1 + max_out * 8), dtype=torch.float32, device=decode_out.device)
    check(lib().trtx_yolo_postprocess_gpu_obb(_p(decode_out), decode_out.shape[0], max_out, ctypes.c_float(conf_thresh), ctypes.c_float(nms_thresh),
                                              _p(out), _stream()), "trtx_yolo_postprocess_gpu_obb")
    return out


DET5_FLOATS = 38  # yolov5/src/types.h:11-16
DET7_FLOATS = 6   # yolov7/include/types.h: bbox[4], conf, class_id


def _grid_tables(grids, anchors, n):
    import numpy as np
    gw = (ctypes.c_int * max(n, 1))(*[g[0] for g in grids[:n]])
    gh = (ctypes.c_int * max(n, 1))(*[g[1] for g in grids[:n]])
    an = np.ascontiguousarray(anchors, dtype=np.float32).reshape(-1, 6)
    return gw, gh, an


# The anchor-based families share their kernels (plugins/anchor_decode.hip, anchor_head.hip); a family is its record length and the
# prefix of its entry points: (38, "trtx_yolov5") or (6, "trtx_yolov7").
def _anchor_decode(det, prefix, inputs, classes, net_h, net_w, grids, anchors, max_out, out, seg_args=()):
    import torch
    L = lib()
    n = len(inputs)
    ins = [x.contiguous() for x in inputs]
    B, dev = ins[0].shape[0], ins[0].device
    arr = (ctypes.c_void_p * n)(*[x.data_ptr() for x in ins])
    gw, gh, an = _grid_tables(grids, anchors, n)
    ws_fn = getattr(L, prefix + "_decode_workspace")
    ws_fn.restype = ctypes.c_size_t
    ws_bytes = ws_fn(B, gw, gh, n)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.zeros((B, 1 + max_out * det), dtype=torch.float32, device=dev)
    check(getattr(L, prefix + "_decode")(arr, n, B, classes, net_h, net_w, gw, gh, an.ctypes.data_as(ctypes.c_void_p), max_out, *seg_args,
                                         _p(out), _p(ws), ctypes.c_size_t(ws_bytes), _stream()), prefix + "_decode")
    return out


def _anchor_head_workspace(prefix, batch, grids):
    n = len(grids)
    gw, gh, _ = _grid_tables(grids, [0.0] * 6 * n, n)
    fn = getattr(lib(), prefix + "_head_decode_workspace")
    fn.restype = ctypes.c_size_t
    return fn(batch, gw, gh, n)


def _anchor_head(det, prefix, heads, classes, net_h, net_w, grids, anchors, max_out, out, ws, ld, n_levels, status_only):
    import torch
    L = lib()
    B, n, dev = heads[0].shape[0], len(heads), heads[0].device
    hp, hl = _head_table(heads)
    if ld is not None:
        hl = (ctypes.c_int * n)(*ld)
    gw, gh, an = _grid_tables(grids, anchors, n)
    if ws is None:
        ws = torch.empty(max(_anchor_head_workspace(prefix, B, grids), 256), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.zeros((B, 1 + max_out * det), dtype=torch.float32, device=dev)
    fn = getattr(L, prefix + ("_head_decode_nhwc_f32" if heads[0].dtype == torch.float32 else "_head_decode_nhwc"))
    st = fn(hp, hl, n if n_levels is None else n_levels, B, classes, net_h, net_w, gw, gh, an.ctypes.data_as(ctypes.c_void_p), max_out, _p(out),
            _p(ws), ctypes.c_size_t(ws.numel()), _stream())
    if status_only:
        return st
    check(st, prefix + "_head_decode_nhwc")
    return out


def yolov5_decode(inputs, classes, net_h, net_w, grids, anchors, max_out=1000, is_seg=False, out=None):
    """Anchor-based YoloLayerPlugin::enqueue replacement (yolov5/plugin/yololayer.cu:161-233).
    inputs: CUDA fp32 [B, 3*(5+classes(+32)), gh*gw] per level; grids: [(gw, gh)]; anchors: [n_levels][6].  -> [B, 1+max_out*38]
    `out`: a caller's buffer of at least B rows (rows beyond B are not touched)."""
    return _anchor_decode(DET5_FLOATS, "trtx_yolov5", inputs, classes, net_h, net_w, grids, anchors, max_out, out, (1 if is_seg else 0,))


def yolov5_head_decode_workspace(batch, grids):
    return _anchor_head_workspace("trtx_yolov5", batch, grids)


def yolov5_head_decode_nhwc(heads, classes, net_h, net_w, grids, anchors, max_out=1000, out=None, ws=None, ld=None, n_levels=None,
                            status_only=False):
    """The fused anchor head on NHWC head tensors [B, gh, gw, ld] (fp16 or fp32; ld >= 3 * (5 + classes), the rest is padding):
    trtx_yolov5_head_decode_nhwc{,_f32}.  grids: [(gw, gh)]; anchors: [n_levels][6].  -> [B, 1 + max_out * 38].
    `out` / `ws`: the caller's buffers; `ld`, `n_levels`: what is passed instead of the tensors' own; `status_only`: return the
    status code instead of raising (the refusal tests)."""
    return _anchor_head(DET5_FLOATS, "trtx_yolov5", heads, classes, net_h, net_w, grids, anchors, max_out, out, ws, ld, n_levels, status_only)


def yolov5_nms(decode_out, max_out=1000, conf_thresh=0.5, nms_thresh=0.45, out=None, ws=None):
    """yolov5 batch_nms replacement (yolov5/src/postprocess.cpp:30-80). Returns keep_idx, keep_cnt, keep_det [B, max_out, 6]."""
    L = lib()
    B = decode_out.shape[0]
    keep_idx, keep_cnt, keep_det, ws = _nms_buffers(B, max_out, 6, decode_out.device, out, ws)
    check(L.trtx_yolov5_nms(_p(decode_out), B, max_out, ctypes.c_float(conf_thresh), ctypes.c_float(nms_thresh), _p(keep_idx), _p(keep_cnt),
                            _p(keep_det), _p(ws), ctypes.c_size_t(ws.numel()), _stream()), "trtx_yolov5_nms")
    return keep_idx, keep_cnt, keep_det


def reorg_fold_weights(w):
    """trtx_reorg_fold_weights: numpy KCRS [cout, 4 * cin, kh, kw] fp32 -> [cout, cin, 2 * kh, 2 * kw], the filter the lowering packs for a
    convolution that absorbed the ReOrg in front of it."""
    import numpy as np
    w = np.ascontiguousarray(w, dtype=np.float32)
    cout, c4, kh, kw = w.shape
    out = np.empty((cout, c4 // 4, 2 * kh, 2 * kw), dtype=np.float32)
    check(lib().trtx_reorg_fold_weights(w.ctypes.data_as(ctypes.c_void_p), cout, c4 // 4, kh, kw, out.ctypes.data_as(ctypes.c_void_p)),
          "trtx_reorg_fold_weights")
    return out


def repvggdw_fold_weights(w7, scale7, shift7, w3, scale3, shift3):
    """trtx_repvggdw_fold_weights: numpy fp32 depthwise filters [C, 1, 7, 7] and [C, 1, 3, 3] with their per-channel scales and shifts ->
    (w [C, 1, 7, 7], shift [C]), what the lowering packs for a folded RepVGGDW."""
    import numpy as np
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (w7, scale7, shift7, w3, scale3, shift3)]
    C = a[0].shape[0]
    w, sh = np.empty((C, 1, 7, 7), np.float32), np.empty(C, np.float32)
    ptr = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(lib().trtx_repvggdw_fold_weights(*[ptr(v) for v in a], C, ptr(w), ptr(sh)), "trtx_repvggdw_fold_weights")
    return w, sh


def yolov7_decode(inputs, classes, net_h, net_w, grids, anchors, max_out=1000, out=None):
    """YOLOv7 YoloLayerPlugin::enqueue replacement (yolov7/plugin/yololayer.cu:152-207).
    inputs: CUDA fp32 [B, 3*(5+classes), gh*gw] per level; grids: [(gw, gh)]; anchors: [n_levels][6].  -> [B, 1+max_out*6]
    `out`: a caller's buffer of at least B rows (rows beyond B are not touched)."""
    return _anchor_decode(DET7_FLOATS, "trtx_yolov7", inputs, classes, net_h, net_w, grids, anchors, max_out, out)


def yolov7_head_decode_workspace(batch, grids):
    return _anchor_head_workspace("trtx_yolov7", batch, grids)


def yolov7_head_decode_nhwc(heads, classes, net_h, net_w, grids, anchors, max_out=1000, out=None, ws=None, ld=None, n_levels=None,
                            status_only=False):
    """The fused YOLOv7 head: yolov5_head_decode_nhwc with 6-float records, trtx_yolov7_head_decode_nhwc{,_f32}.  -> [B, 1 + max_out * 6]."""
    return _anchor_head(DET7_FLOATS, "trtx_yolov7", heads, classes, net_h, net_w, grids, anchors, max_out, out, ws, ld, n_levels, status_only)


def yolov7_nms(decode_out, max_out=1000, conf_thresh=0.5, nms_thresh=0.45, out=None, ws=None):
    """yolov7 batch_nms replacement (yolov7/src/postprocess.cpp:48-89) on 6-float records.  Returns keep_idx, keep_cnt,
    keep_det [B, max_out, 6]."""
    L = lib()
    B = decode_out.shape[0]
    keep_idx, keep_cnt, keep_det, ws = _nms_buffers(B, max_out, 6, decode_out.device, out, ws)
    check(L.trtx_yolov7_nms(_p(decode_out), B, max_out, ctypes.c_float(conf_thresh), ctypes.c_float(nms_thresh), _p(keep_idx), _p(keep_cnt),
                            _p(keep_det), _p(ws), ctypes.c_size_t(ws.numel()), _stream()), "trtx_yolov7_nms")
    return keep_idx, keep_cnt, keep_det


DARKNET_DET_FLOATS = 7   # yolov4/yololayer.h:41-47: bbox[4], det_confidence, class_id, class_confidence


def darknet_decode(inputs, classes, net_h, net_w, grids, anchors, max_out=1000, out=None):
    """Darknet YoloLayerPlugin::enqueue replacement (yolov4/yololayer.cu:154-219; YOLOv3, YOLOv3-tiny and YOLOv4).
    inputs: CUDA fp32 [B, 3*(5+classes), gh*gw] per level; grids: [(gw, gh)]; anchors: [n_levels][6].  -> [B, 1+max_out*7]"""
    return _anchor_decode(DARKNET_DET_FLOATS, "trtx_darknet", inputs, classes, net_h, net_w, grids, anchors, max_out, out)


def darknet_head_decode_workspace(batch, grids):
    return _anchor_head_workspace("trtx_darknet", batch, grids)


def darknet_head_decode_nhwc(heads, classes, net_h, net_w, grids, anchors, max_out=1000, out=None, ws=None, ld=None, n_levels=None,
                             status_only=False):
    """The fused Darknet head: yolov5_head_decode_nhwc with the Darknet arithmetic and 7-float records,
    trtx_darknet_head_decode_nhwc{,_f32}.  -> [B, 1 + max_out * 7]."""
    return _anchor_head(DARKNET_DET_FLOATS, "trtx_darknet", heads, classes, net_h, net_w, grids, anchors, max_out, out, ws, ld, n_levels,
                        status_only)


def darknet_nms(decode_out, max_out=1000, conf_thresh=0.5, nms_thresh=0.4, out=None, ws=None):
    """Darknet nms() replacement (yolov4/yolov4.cpp:81-124) on 7-float records.  Returns keep_idx, keep_cnt, keep_det [B, max_out, 6]."""
    L = lib()
    B = decode_out.shape[0]
    keep_idx, keep_cnt, keep_det, ws = _nms_buffers(B, max_out, 6, decode_out.device, out, ws)
    check(L.trtx_darknet_nms(_p(decode_out), B, max_out, ctypes.c_float(conf_thresh), ctypes.c_float(nms_thresh), _p(keep_idx), _p(keep_cnt),
                             _p(keep_det), _p(ws), ctypes.c_size_t(ws.numel()), _stream()), "trtx_darknet_nms")
    return keep_idx, keep_cnt, keep_det


def yolov9_decode(inputs, classes, net_h, net_w, max_out=1000, is_seg=False, out=None):
    """YOLOv9 YoloLayerPlugin::enqueue replacement (yolov9/plugin/yololayer.cu:124-197).
    inputs: three CUDA fp32 [B, 4 + classes (+ 32), gh * gw] (strides 8 / 16 / 32).  -> [B, 1 + max_out * 38]"""
    import torch
    L = lib()
    ins = [x.contiguous() for x in inputs]
    assert len(ins) == 3 and all(x.is_cuda and x.dtype == torch.float32 for x in ins)
    B, dev = ins[0].shape[0], ins[0].device
    arr = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in ins])
    L.trtx_yolov9_decode_workspace.restype = ctypes.c_size_t
    ws_bytes = L.trtx_yolov9_decode_workspace(B, net_h, net_w)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.zeros((B, 1 + max_out * DET5_FLOATS), dtype=torch.float32, device=dev)
    check(L.trtx_yolov9_decode(arr, B, classes, net_h, net_w, max_out, 1 if is_seg else 0, _p(out), _p(ws), ctypes.c_size_t(ws_bytes), _stream()),
          "trtx_yolov9_decode")
    return out


def yolov9_head_decode_nhwc(box, cls, classes, net_h, net_w, dfl_w, max_out=1000, out=None, batch=None, box_ld=None, cls_ld=None, ws=None):
    """The fused DDetect head (trtx_yolov9_head_decode_nhwc{,_f32}) on the NHWC outputs of cv2.l.2 and cv3.l.2, three levels:
    box[l] [B, cells_l, box_ld] (channels [0, 64) = DFL bins), cls[l] [B, cells_l, cls_ld] (channels [0, classes) = logits), fp16 or
    fp32.  `out` (rows of 1 + max_out * 38), `batch`, the strides and the workspace can be given.  -> [B, 1 + max_out * 38]"""
    import torch
    L = lib()
    assert len(box) == 3 and len(cls) == 3
    B = box[0].shape[0] if batch is None else batch
    dev = box[0].device
    bp = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in box])
    cp = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in cls])
    bl = (ctypes.c_int * 3)(*(box_ld if box_ld is not None else [x.shape[-1] for x in box]))
    cl = (ctypes.c_int * 3)(*(cls_ld if cls_ld is not None else [x.shape[-1] for x in cls]))
    L.trtx_yolov9_head_decode_workspace.restype = ctypes.c_size_t
    if ws is None:
        ws = torch.empty(max(L.trtx_yolov9_head_decode_workspace(B, net_h, net_w), 256), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.zeros((B, 1 + max_out * DET5_FLOATS), dtype=torch.float32, device=dev)
    fn = L.trtx_yolov9_head_decode_nhwc_f32 if box[0].dtype == torch.float32 else L.trtx_yolov9_head_decode_nhwc
    check(fn(bp, bl, cp, cl, B, classes, net_h, net_w, _p(dfl_w), max_out, _p(out), _p(ws), ctypes.c_size_t(ws.numel()), _stream()),
          "trtx_yolov9_head_decode_nhwc")
    return out


def yolov9_nms(decode_out, max_out=1000, conf_thresh=0.5, nms_thresh=0.45, out=None, ws=None):
    """yolov9 batch_nms replacement (yolov9/src/postprocess.cpp:48-91) on 38-float records with corner boxes.  Returns keep_idx, keep_cnt,
    keep_det [B, max_out, 6] = cx, cy, w, h, conf, class: the centre format the reference's nms() leaves in `res`."""
    L = lib()
    B = decode_out.shape[0]
    keep_idx, keep_cnt, keep_det, ws = _nms_buffers(B, max_out, 6, decode_out.device, out, ws)
    check(L.trtx_yolov9_nms(_p(decode_out), B, max_out, ctypes.c_float(conf_thresh), ctypes.c_float(nms_thresh), _p(keep_idx), _p(keep_cnt),
                            _p(keep_det), _p(ws), ctypes.c_size_t(ws.numel()), _stream()), "trtx_yolov9_nms")
    return keep_idx, keep_cnt, keep_det


def seg_masks(decode_out, keep_idx, keep_cnt, proto, net_h, net_w, max_keep, box_format=0, out=None):
    """process_mask's coefficient loop on the GPU (yolov5/src/postprocess.cpp:94-120, yolov8/yolov8_seg.cpp:17-53).
    decode_out [B, 1 + max_out * 38 | 90] (the record length follows from keep_idx's max_out), keep_idx [B, max_out] and keep_cnt [B]
    as yolov5_nms / yolo_nms return them, proto [B, 32, mask_h, mask_w].  box_format 0: yolov5's centre boxes, 1: yolov8 / yolo11's
    corner boxes.  Returns masks [B, max_keep, mask_h, mask_w] (`out`, or a new zero-filled tensor): slot d of an image is its kept
    detection d for d < min(keep_cnt, max_keep); later slots are not written."""
    import torch
    B, max_out = keep_idx.shape
    assert decode_out.shape[0] == B and (decode_out.shape[1] - 1) % max_out == 0
    det_floats = (decode_out.shape[1] - 1) // max_out
    assert proto.dim() == 4 and proto.shape[0] == B and proto.shape[1] == 32
    mask_h, mask_w = int(proto.shape[2]), int(proto.shape[3])
    for t, dt in ((decode_out, torch.float32), (keep_idx, torch.int32), (keep_cnt, torch.int32), (proto, torch.float32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    if out is None:
        out = torch.zeros((B, max(max_keep, 0), mask_h, mask_w), dtype=torch.float32, device=proto.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= B * max(max_keep, 0) * mask_h * mask_w
    check(lib().trtx_seg_masks(_p(decode_out), det_floats, box_format, _p(keep_idx), _p(keep_cnt), B, max_out, max_keep, _p(proto), mask_h,
                               mask_w, net_h, net_w, _p(out), _stream()), "trtx_seg_masks")
    return out


def yolo_postprocess_gpu(decode_out, max_out=1000, conf_thresh=0.5, nms_thresh=0.45, out=None, ws=None):
    """The reference's GPU post-processing mode "g" (yolov8/src/postprocess.cu:42-111): [B, 1 + max_out*7].
    `out`: the caller's buffer; `ws`: accepted like the NMS wrappers' and not used (this entry point takes no workspace)."""
    import torch
    B = decode_out.shape[0]
    if out is None:
        out = torch.empty((B, 1 + max_out * 7), dtype=torch.float32, device=decode_out.device)
    check(lib().trtx_yolo_postprocess_gpu(_p(decode_out), B, max_out, ctypes.c_float(conf_thresh), ctypes.c_float(nms_thresh),
                                          _p(out), _stream()), "trtx_yolo_postprocess_gpu")
    return out


ACT = {"none": 0, "relu": 1, "sigmoid": 2, "silu": 3, "leaky": 4, "tanh": 5, "mish": 6}


def _hw(v):
    """an int, or an (h, w) pair -> (h, w)"""
    if isinstance(v, (tuple, list)):
        h, w = v
        return int(h), int(w)
    return int(v), int(v)


def pack_conv_weights_f16(w_kcrs, cin_pad=None, ch_scale=None):
    """Host: KCRS fp32 numpy -> (packed uint16 [Cout_pad, Kpad], cout_pad, kpad, bn)."""
    import numpy as np
    L = lib()
    w = np.ascontiguousarray(w_kcrs, dtype=np.float32)
    cout, cin, kh, kw = w.shape
    cin_pad = cin_pad or (cin + 7) // 8 * 8
    cp, kp, bn = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    check(L.trtx_conv_packed_dims(cout, cin_pad, kh, kw, ctypes.byref(cp), ctypes.byref(kp), ctypes.byref(bn)),
          "trtx_conv_packed_dims")
    packed = np.zeros((cp.value, kp.value), dtype=np.uint16)
    sc = None
    if ch_scale is not None:
        sc = np.ascontiguousarray(ch_scale, dtype=np.float32)
    check(L.trtx_conv_pack_weights_f16(w.ctypes.data_as(ctypes.c_void_p), cout, cin, kh, kw, cin_pad,
                                       sc.ctypes.data_as(ctypes.c_void_p) if sc is not None else None,
                                       packed.ctypes.data_as(ctypes.c_void_p)), "trtx_conv_pack_weights_f16")
    return packed, cp.value, kp.value, bn.value


def conv2d_nhwc_f16(x, wpacked, bias, cout, kh, kw, stride, pad, act1="none", residual=None, act2="none",
                    out=None, out_ld=None):
    """Single fused conv launch on NHWC fp16 tensors (x: [N,H,W,Cin] CUDA half); stride / pad: an int or an (h, w) pair."""
    import torch
    L = lib()
    N, H, W, Cin = x.shape
    (sh, sw), (ph, pw) = _hw(stride), _hw(pad)
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, cout), dtype=torch.float16, device=x.device)
    ld_out = out_ld or out.shape[-1]
    check(L.trtx_op_conv2d_nhwc_f16(_p(x), N, H, W, Cin, x.stride(2), _p(wpacked), _p(bias), _p(out), cout, ld_out,
                                    kh, kw, sh, sw, ph, pw, ACT[act1], _p(residual),
                                    residual.stride(2) if residual is not None else 0, ACT[act2], _stream()),
          "trtx_op_conv2d_nhwc_f16")
    return out


def stem_weights(w_kcrs):
    """Host: KCRS fp32 numpy -> the stem kernels' layout [tap = (c*k + r)*k + q][Cout] (fp32)."""
    import numpy as np
    w = np.ascontiguousarray(w_kcrs, dtype=np.float32)
    return np.ascontiguousarray(w.reshape(w.shape[0], -1).T)


def conv_stem_nchw_f16(x, w_taps_cout, bias, k, stride, pad, act="none", out=None, out_ld=None):
    """The first layer of an fp16 engine: x [N,C,H,W] CUDA float (C <= 4), w_taps_cout [C*k*k, Cout] CUDA float -> NHWC half."""
    import torch
    N, C, H, W = x.shape
    cout = w_taps_cout.shape[1]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, cout), dtype=torch.float16, device=x.device)
    check(lib().trtx_op_conv_stem_nchw_f16(_p(x), N, C, H, W, _p(w_taps_cout), _p(bias), _p(out), cout, out_ld or out.shape[-1], k, stride, pad,
                                           ACT[act], _stream()), "trtx_op_conv_stem_nchw_f16")
    return out


def conv_stem_pair_f16(x, stem_w_taps_cout, stem_bias, conv_wpacked, conv_bias, stem_act="silu", conv_act="silu", out=None, out_ld=None):
    """The 3x3 / 2 stem (C <= 4 -> 16) and the 16 -> 32 3x3 / 2 convolution behind it in one launch: x [N,C,H,W] CUDA float -> NHWC half [N,Ho,Wo,32]
    (or into `out` with channel stride out_ld)."""
    import torch
    N, C, H, W = x.shape
    Hi, Wi = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, 32), dtype=torch.float16, device=x.device)
    check(lib().trtx_op_conv_stem_pair_f16(_p(x), N, C, H, W, _p(stem_w_taps_cout), _p(stem_bias), ACT[stem_act], _p(conv_wpacked), _p(conv_bias),
                                           ACT[conv_act], _p(out), out_ld or out.shape[-1], _stream()), "trtx_op_conv_stem_pair_f16")
    return out


def conv_bneck_pair_f16(x, w1_packed, bias1, w2_packed, bias2, act1="silu", act2="silu", shortcut=True, act_after="none", out=None, out_ld=None, in_coff=None,
                        mid=None):
    """The two 3x3 convolutions of a 16-channel bottleneck (16 -> 16 -> 16, stride 1, pad 1) in one launch: x [N,H,W,16] CUDA half or a 16-channel slice of
    a wider tensor (pixel stride x.stride(2)) -> NHWC half [N,H,W,16] (or into `out` with channel stride out_ld); shortcut: x is added to the result.
    in_coff: x is the WHOLE wider tensor and the 16 input channels start at this channel.  mid (NHWC half [N,H,W,16]): the executor's form - the fused
    launch where it is possible, the two launches through `mid` where it is not (an `out` that lies on the input channels, which the fused launch refuses)."""
    import torch
    N, H, W, C = x.shape
    assert x.dtype == torch.float16 and x.stride(3) == 1 and (C == 16 if in_coff is None else in_coff + 16 <= C)
    if out is None:
        out = torch.empty((N, H, W, 16), dtype=torch.float16, device=x.device)
    head = (_p(x), N, H, W, x.stride(2), in_coff or 0, _p(w1_packed), _p(bias1), ACT[act1], _p(w2_packed), _p(bias2), ACT[act2], 1 if shortcut else 0, ACT[act_after])
    if mid is None:
        check(lib().trtx_op_conv_bneck_pair_f16(*head, _p(out), out_ld or out.shape[-1], _stream()), "trtx_op_conv_bneck_pair_f16")
    else:
        assert mid.dtype == torch.float16 and mid.is_contiguous() and tuple(mid.shape) == (N, H, W, 16)
        check(lib().trtx_op_conv_bneck_pair_or_two_f16(*head, _p(mid), _p(out), out_ld or out.shape[-1], _stream()), "trtx_op_conv_bneck_pair_or_two_f16")
    return out


def conv_dual_group_f16(xs, w0, b0, outs0, w1, b1, outs1, k=3, stride=1, pad=1, act0="silu", act1="silu", cout0=None, cout1=None, res1=None, i8_1=False,
                        or_two=False, status_only=False):
    """1..3 pairs of convolutions over shared inputs in one launch (the dual tile): xs[j] [N,H,W,Cin] CUDA half (or a channel slice: pixel stride
    xs[j].stride(2)); w0[j] / w1[j] packed weights of the 64-wide and the 80-wide side, b0[j] / b1[j] their biases; outs0[j] / outs1[j] the outputs, whole tensors
    or channel slices (pixel stride .stride(2)); cout0 / cout1: per-problem channel counts (default: the outputs' last dimension).  res1: a shortcut for the
    second side (refused by the launch).  or_two: the executor's form, which computes what the launch refuses as the launches of each side.
    status_only: return the status instead of raising."""
    import torch
    n = len(xs)
    A = lambda seq: None if seq is None else (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in seq])
    geom = (ctypes.c_int32 * (5 * n))(*[v for x in xs for v in (x.shape[0], x.shape[1], x.shape[2], x.shape[3], x.stride(2))])
    side = lambda outs, couts, act: (ctypes.c_int32 * (3 * n))(*[v for j, o in enumerate(outs) for v in (couts[j] if couts else o.shape[-1], o.stride(2), ACT[act])])
    assert all(t.dtype == torch.float16 and t.stride(3) == 1 for t in list(xs) + list(outs0) + list(outs1))
    fn = lib().trtx_op_conv_dual_group_or_two_f16 if or_two else lib().trtx_op_conv_dual_group_f16
    st = fn(n, A(xs), geom, k, stride, pad, A(w0), A(b0), A(outs0), side(outs0, cout0, act0), A(w1), A(b1), A(outs1), side(outs1, cout1, act1),
            A(res1), res1[0].stride(2) if res1 is not None else 0, 1 if i8_1 else 0, _stream())
    if status_only:
        return st
    check(st, "trtx_op_conv_dual_group_f16")
    return outs0, outs1


# ---------------------------------------------------------------------------------------------------- grouped conv on the matrix pipe (tests / tools)
def pack_conv_weights_grouped_f16(w_kcrs, ch_scale=None):
    """Host: KCRS fp32 numpy [Cout, Cin / groups, k, k] -> packed uint16 [Cout, Kpad] for conv2d_grouped_nhwc_f16."""
    import numpy as np
    L = lib()
    w = np.ascontiguousarray(w_kcrs, dtype=np.float32)
    cout, cin_g, kh, kw = w.shape
    kp = ctypes.c_int32()
    check(L.trtx_conv_pack_weights_grouped_f16(w.ctypes.data_as(ctypes.c_void_p), cout, cin_g, kh, kw, None, None, ctypes.byref(kp)),
          "trtx_conv_pack_weights_grouped_f16 (dims)")
    packed = np.zeros((cout, kp.value), dtype=np.uint16)
    sc = None if ch_scale is None else np.ascontiguousarray(ch_scale, dtype=np.float32)
    check(L.trtx_conv_pack_weights_grouped_f16(w.ctypes.data_as(ctypes.c_void_p), cout, cin_g, kh, kw,
                                               sc.ctypes.data_as(ctypes.c_void_p) if sc is not None else None,
                                               packed.ctypes.data_as(ctypes.c_void_p), ctypes.byref(kp)), "trtx_conv_pack_weights_grouped_f16")
    return packed


def conv2d_grouped_nhwc_f16(x, wpacked, bias, cout, groups, k, pad, act1="none", residual=None, act2="none", out=None, out_ld=None):
    """Single grouped-convolution launch (kernels/conv_grouped.hip) on NHWC fp16 tensors; x: [N,H,W,Cin] CUDA half or a channel slice of
    a wider tensor (its pixel stride is taken from x.stride(2)); out / out_ld: a channel slice of a wider buffer."""
    import torch
    N, H, W, Cin = x.shape
    if out is None:
        out = torch.empty((N, H + 2 * pad - k + 1, W + 2 * pad - k + 1, cout), dtype=torch.float16, device=x.device)
    check(lib().trtx_op_conv2d_grouped_nhwc_f16(_p(x), N, H, W, Cin, x.stride(2), _p(wpacked), _p(bias), _p(out), cout, out_ld or out.shape[-1], groups, k,
                                                pad, ACT[act1], _p(residual), residual.stride(2) if residual is not None else 0, ACT[act2], _stream()),
          "trtx_op_conv2d_grouped_nhwc_f16")
    return out


# ---------------------------------------------------------------------------------------------------- depthwise conv and the attention kernels (tests / tools)
def conv2d_dw_nhwc(x, w, bias, k, stride, act1="none", residual=None, act2="none", out=None, out_ld=None, alpha1=0.1, alpha2=0.1, pad=None, dilation=1):
    """Single depthwise-convolution launch (kernels/conv_dw.hip) on NHWC fp16 or fp32 tensors.  x: [N,H,W,C] CUDA, or a channel slice of a wider
    tensor (its pixel stride is x.stride(2)); residual likewise; out / out_ld: a channel slice of a wider buffer.  w: the filter as a host
    array [C, k, k] (or [C, 1, k, k]) - transposed here into the device layout, fp32 [k * k][C]; bias: a CUDA fp32 tensor [C] or None.
    pad: k // 2 unless given (the kernel takes nothing else: TrtxError with status 4)."""
    import numpy as np
    import torch
    N, H, W, C = x.shape
    assert x.dtype in (torch.float16, torch.float32) and (residual is None or residual.dtype == x.dtype)
    pad = k // 2 if pad is None else pad
    Ho, Wo = (H + 2 * pad - dilation * (k - 1) - 1) // stride + 1, (W + 2 * pad - dilation * (k - 1) - 1) // stride + 1
    taps = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(C, k * k).T)
    wg = torch.from_numpy(taps).to(x.device)
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    assert out.dtype == x.dtype
    check(lib().trtx_op_conv2d_dw_nhwc(_p(x), 1 if x.dtype == torch.float16 else 0, N, H, W, C, x.stride(2), _p(wg), _p(bias), _p(out),
                                       out_ld or out.shape[-1], _p(residual), residual.stride(2) if residual is not None else 0, k, stride, pad, dilation,
                                       ACT[act1], ctypes.c_float(alpha1), ACT[act2], ctypes.c_float(alpha2), _stream()), "trtx_op_conv2d_dw_nhwc")
    return out


def _attention(fn, what, qkv, heads, scale, out, vimg, out_ld, v_ld, qkv_ld, kd, hd, extra):
    import torch
    B, N, _ = qkv.shape
    for t in (qkv, out, vimg):
        assert t.is_cuda and t.dtype == torch.float16
    check(fn(_p(qkv), qkv_ld or qkv.stride(1), _p(out), out_ld or out.stride(1), _p(vimg), v_ld or vimg.stride(1), B, heads, N, *extra, kd, hd,
             ctypes.c_float(scale), _stream()), what)
    return out, vimg


def psa_attention(qkv, heads, scale, out=None, vimg=None, out_ld=None, v_ld=None, qkv_ld=None, kd=32, hd=64):
    """The fused PSA attention (kernels/attention.hip).  qkv: CUDA fp16 [B, N, heads * (2 kd + hd)] or a channel slice of a wider tensor (pixel
    stride qkv.stride(1)); out / vimg: [B, N, heads * hd] tensors or channel slices (out_ld / v_ld: their pixel strides).  -> (O, V image)"""
    import torch
    B, N, _ = qkv.shape
    out = torch.empty((B, N, heads * hd), dtype=torch.float16, device=qkv.device) if out is None else out
    vimg = torch.empty((B, N, heads * hd), dtype=torch.float16, device=qkv.device) if vimg is None else vimg
    return _attention(lib().trtx_op_psa_attention_f16, "trtx_op_psa_attention_f16", qkv, heads, scale, out, vimg, out_ld, v_ld, qkv_ld, kd, hd, ())


def area_attention(qkv, heads, area, scale, out=None, vimg=None, out_ld=None, v_ld=None, qkv_ld=None, kd=32, hd=32):
    """The area attention on MFMA (kernels/attention_mfma.hip): as psa_attention, the N pixels of an image split into `area` contiguous ranges."""
    import torch
    B, N, _ = qkv.shape
    out = torch.empty((B, N, heads * hd), dtype=torch.float16, device=qkv.device) if out is None else out
    vimg = torch.empty((B, N, heads * hd), dtype=torch.float16, device=qkv.device) if vimg is None else vimg
    return _attention(lib().trtx_op_area_attention_f16, "trtx_op_area_attention_f16", qkv, heads, scale, out, vimg, out_ld, v_ld, qkv_ld, kd, hd, (area,))


def area_attention_split(q, k, v, heads, area, scale, out=None, q_ld=None, k_ld=None, v_ld=None, out_ld=None, kd=32, hd=32):
    """The area attention on separate operands (kernels/attention_mfma.hip; YOLOv13's AAttn): q, k: CUDA fp16 [B, N, heads * kd], v: [B, N, heads * hd],
    each a tensor of its own or a channel slice of a wider one (pixel stride t.stride(1), or the *_ld given); out likewise (allocated when None).  -> O"""
    import torch
    B, N, _ = q.shape
    out = torch.empty((B, N, heads * hd), dtype=torch.float16, device=q.device) if out is None else out
    for t in (q, k, v, out):
        assert t.is_cuda and t.dtype == torch.float16
    check(lib().trtx_op_area_attention_split_f16(_p(q), q_ld or q.stride(1), _p(k), k_ld or k.stride(1), _p(v), v_ld or v.stride(1), _p(out),
                                                 out_ld or out.stride(1), B, heads, N, area, kd, hd, ctypes.c_float(scale), _stream()),
          "trtx_op_area_attention_split_f16")
    return out


HGCONV_WEIGHTS = ("w_ctx", "b_ctx", "proto", "w_pre", "b_pre", "w_edge", "b_edge", "w_node", "b_node")   # trtx_op_hgconv_f16's nine fp32 arrays, in its order


def hgconv_workspace_bytes(B, N, D, E):
    """Bytes of device workspace trtx_op_hgconv_f16 needs: a pure function of its arguments (host only); 0 = (D, E) is not implemented."""
    L = lib()
    L.trtx_op_hgconv_workspace_bytes.restype = ctypes.c_size_t
    return int(L.trtx_op_hgconv_workspace_bytes(int(B), int(N), int(D), int(E)))


def hgconv_geometry():
    """The node-tile sizes of the hypergraph convolution's launcher, ascending (host only)."""
    arr, n = (ctypes.c_int32 * 8)(), ctypes.c_int32()
    check(lib().trtx_op_hgconv_geometry(arr, 8, ctypes.byref(n)), "trtx_op_hgconv_geometry")
    return [int(arr[i]) for i in range(min(n.value, 8))]


def hgconv(x, E, logit_scale, weights, out=None, x_ld=None, out_ld=None, D=None, workspace=None):
    """YOLOv13's hypergraph convolution (kernels/hgconv.hip).  x: CUDA fp16 [B, N, D] or a channel slice of a wider tensor (pixel stride x.stride(1));
    out: likewise (allocated [B, N, D] when None); weights: a dict of CUDA fp32 tensors keyed by HGCONV_WEIGHTS (the layers' own layouts);
    workspace: a CUDA uint8 tensor of at least hgconv_workspace_bytes() bytes (allocated when None).  -> out"""
    import torch
    L = lib()
    B, N, Dx = x.shape
    D = Dx if D is None else D
    assert x.is_cuda and x.dtype == torch.float16
    out = torch.empty((B, N, D), dtype=torch.float16, device=x.device) if out is None else out
    assert out.is_cuda and out.dtype == torch.float16
    ws = workspace if workspace is not None else torch.empty(max(hgconv_workspace_bytes(B, N, D, E), 256), dtype=torch.uint8, device=x.device)
    ws_arr = [weights[k].contiguous() for k in HGCONV_WEIGHTS]
    for w in ws_arr:
        assert w.is_cuda and w.dtype == torch.float32
    L.trtx_op_hgconv_f16.argtypes = ([ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 4 + [ctypes.c_float] +
                                     [ctypes.c_void_p] * 9 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p])
    check(L.trtx_op_hgconv_f16(_p(x), x_ld or x.stride(1), _p(out), out_ld or out.stride(1), B, N, D, E, float(logit_scale), *[_p(w) for w in ws_arr],
                               _p(ws), ws.numel(), _stream()), "trtx_op_hgconv_f16")
    return out


# ---------------------------------------------------------------------------------------------------- fp32 engines: conv on the fp32 MFMA (tests / tools)
def pack_conv_weights_f32(w_kcrs, cin_pad=None, ch_scale=None):
    """Host: KCRS fp32 numpy -> (packed float32 [Cout_pad, Kpad], cout_pad, kpad, cink) for conv2d_nhwc_f32."""
    import numpy as np
    L = lib()
    w = np.ascontiguousarray(w_kcrs, dtype=np.float32)
    cout, cin, kh, kw = w.shape
    cin_pad = cin_pad or (cin + 3) // 4 * 4
    cp, kp, ck = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    check(L.trtx_conv_packed_dims_f32(cout, cin_pad, kh, kw, ctypes.byref(cp), ctypes.byref(kp), ctypes.byref(ck)), "trtx_conv_packed_dims_f32")
    packed = np.zeros((cp.value, kp.value), dtype=np.float32)
    sc = np.ascontiguousarray(ch_scale, dtype=np.float32) if ch_scale is not None else None
    check(L.trtx_conv_pack_weights_f32(w.ctypes.data_as(ctypes.c_void_p), cout, cin, kh, kw, cin_pad,
                                       sc.ctypes.data_as(ctypes.c_void_p) if sc is not None else None,
                                       packed.ctypes.data_as(ctypes.c_void_p)), "trtx_conv_pack_weights_f32")
    return packed, cp.value, kp.value, ck.value


def conv2d_nhwc_f32(x, wpacked, bias, cout, kh, kw, stride, pad, act1="none", residual=None, act2="none", out=None, out_ld=None, tile=None):
    """Single fused conv launch on NHWC fp32 tensors (x: [N,H,W,Cin] CUDA float32, Cin % 4 == 0); stride / pad: an int or an (h, w) pair; tile = (bn, bm, operand path, channels per k-step) or None.
    bias: cout_pad floats (cout rounded up to 16; pack_conv_weights_f32 returns cout_pad) - the kernel reads it in 16-byte pieces up to the padded width."""
    import torch
    L = lib()
    N, H, W, Cin = x.shape
    if bias is not None and bias.numel() < (cout + 15) // 16 * 16:
        raise ValueError(f"bias holds {bias.numel()} floats, the fp32 tile reads cout_pad = {(cout + 15) // 16 * 16}")
    (sh, sw), (ph, pw) = _hw(stride), _hw(pad)
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    ld_out = out_ld or out.shape[-1]
    t2 = (ctypes.c_int32 * 4)(*tile) if tile is not None else None
    check(L.trtx_op_conv2d_nhwc_f32(_p(x), N, H, W, Cin, x.stride(2), _p(wpacked), _p(bias), _p(out), cout, ld_out, kh, kw, sh, sw, ph, pw,
                                    ACT[act1], _p(residual), residual.stride(2) if residual is not None else 0, ACT[act2], t2, _stream()),
          "trtx_op_conv2d_nhwc_f32")
    return out


def conv2d_tactics_f32(N, H, W, Cin, Cout, k, stride, pad, residual=False, ld_in=None, ld_out=None, ld_res=None, max_out=32):
    """The launch configurations (bn, bm, operand path, channels per k-step) of one fp32 conv layer (host only); [0] is the launcher's own choice.
    k: an int or (kh, kw); stride / pad: an int or an (h, w) pair."""
    arr = (ctypes.c_int32 * (4 * max_out))()
    (kh, kw), (sh, sw), (ph, pw) = _hw(k), _hw(stride), _hw(pad)
    n = lib().trtx_op_conv2d_tactics_f32(N, H, W, Cin, ld_in or Cin, Cout, ld_out or Cout, kh, kw, sh, sw, ph, pw, 1 if residual else 0,
                                         (ld_res or Cout) if residual else 0, arr, max_out)
    return [(arr[4 * i], arr[4 * i + 1], arr[4 * i + 2], arr[4 * i + 3]) for i in range(n)]


# ---------------------------------------------------------------------------------------------------- test support
def poison_lds(sync=True):
    """Test support: fill every CU's LDS with fp16 NaN patterns (LDS is not cleared between kernels).  sync=False: only enqueued, on the
    current stream - the poisoning workgroups then run BESIDE whatever the other streams have in flight."""
    import torch
    w = torch.zeros(4, dtype=torch.int32, device="cuda")
    check(lib().trtx_op_poison_lds(_p(w), _stream()), "trtx_op_poison_lds")
    if sync:
        torch.cuda.synchronize()


def conv2d_tactics(N, H, W, Cin, Cout, k, stride, pad, residual=False, ld_in=None, ld_out=None, ld_res=None, max_out=32):
    """The exchangeable launch configurations of one conv layer (host only): list of (bn, bk, bm, wsk, ws, r3); [0] is the default.
    k: an int or (kh, kw); stride / pad: an int or an (h, w) pair."""
    arr = (ctypes.c_int32 * (6 * max_out))()
    (kh, kw), (sh, sw), (ph, pw) = _hw(k), _hw(stride), _hw(pad)
    n = lib().trtx_op_conv2d_tactics(N, H, W, Cin, ld_in or Cin, Cout, ld_out or Cout, kh, kw, sh, sw, ph, pw, 1 if residual else 0,
                                     (ld_res or Cout) if residual else 0, arr, max_out)
    return [tuple(arr[6 * i + j] for j in range(6)) for i in range(n)]


def conv_force_tactic(tactic=None):
    """Pin the launch configuration used by the following conv2d_nhwc_f16 calls of this process (None: back to the default)."""
    if tactic is None:
        check(lib().trtx_op_conv_force_tactic(None), "trtx_op_conv_force_tactic")
    else:
        check(lib().trtx_op_conv_force_tactic((ctypes.c_int32 * 6)(*tactic)), "trtx_op_conv_force_tactic")


# ---------------------------------------------------------------------------------------------------- kINT8 conv (tests / tools)
def pack_conv_weights_i8(w_kcrs, ch_scale=None):
    """Host: KCRS fp32 numpy -> (packed int8 [Cout_pad, Kpad], wscale [Cout_pad]) with per-output-channel symmetric scales."""
    import numpy as np
    L = lib()
    w = np.ascontiguousarray(w_kcrs, dtype=np.float32)
    cout, cin, kh, kw = w.shape
    cp, kp = ctypes.c_int32(), ctypes.c_int32()
    check(L.trtx_conv_pack_weights_i8(w.ctypes.data_as(ctypes.c_void_p), cout, cin, kh, kw, None, None, None, ctypes.byref(cp), ctypes.byref(kp)),
          "trtx_conv_pack_weights_i8 (dims)")
    packed = np.zeros((cp.value, kp.value), dtype=np.int8)
    wscale = np.zeros((cp.value,), dtype=np.float32)
    sc = None if ch_scale is None else np.ascontiguousarray(ch_scale, dtype=np.float32)
    check(L.trtx_conv_pack_weights_i8(w.ctypes.data_as(ctypes.c_void_p), cout, cin, kh, kw,
                                      sc.ctypes.data_as(ctypes.c_void_p) if sc is not None else None, packed.ctypes.data_as(ctypes.c_void_p),
                                      wscale.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cp), ctypes.byref(kp)), "trtx_conv_pack_weights_i8")
    return packed, wscale


def conv2d_nhwc_i8(x_i8, wpacked, cscale, bias, cout, kh, kw, stride, pad, act1="none", out_scale=None, residual=None, res_scale=1.0,
                   act2="none", out=None, out_ld=None):
    """int8 MFMA conv: x_i8 CUDA int8 [N,H,W,Cin]; returns int8 (out_scale given: quantised with 1/out_scale) or fp16 NHWC.
    stride / pad: an int or an (h, w) pair; out / out_ld: a channel slice of a wider buffer (offset and width multiples of 8)."""
    import torch
    N, H, W, Cin = x_i8.shape
    (sh, sw), (ph, pw) = _hw(stride), _hw(pad)
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, cout), dtype=torch.int8 if out_scale else torch.float16, device=x_i8.device)
    res_i8 = residual is not None and residual.dtype == torch.int8
    check(lib().trtx_op_conv2d_nhwc_i8(_p(x_i8), N, H, W, Cin, x_i8.stride(2), _p(wpacked), _p(cscale), _p(bias), _p(out), 1 if out_scale else 0,
                                       ctypes.c_float(1.0 / out_scale if out_scale else 0.0), cout, out_ld or out.shape[-1], kh, kw, sh, sw, ph, pw, ACT[act1],
                                       _p(residual), 1 if res_i8 else 0, ctypes.c_float(res_scale), residual.stride(2) if residual is not None else 0,
                                       ACT[act2], _stream()), "trtx_op_conv2d_nhwc_i8")
    return out


DET10_FLOATS = 6   # yolov10/include/types.h: bbox[4] (xyxy), conf, class_id


def yolov10_decode(inputs, classes, net_h, net_w, strides, max_out=1000, out=None, ws=None, batch=None, n_levels=None, status_only=False):
    """YOLOv10 YoloLayerPlugin::enqueue replacement (yolov10/plugin/yololayer.cu:157-240): trtx_yolov10_decode.
    inputs: CUDA fp32 tensors [B, 4 + classes, gh * gw] (None: a null level pointer).  -> [B, 1 + max_out * 6].  `out` / `ws`: the caller's
    buffers; `batch`, `n_levels`: what is passed instead of the tensors' own; `strides` None: a null pointer; `status_only`: the status code."""
    import torch
    L = lib()
    first = next(x for x in inputs if x is not None)
    B, n, dev = first.shape[0] if batch is None else batch, len(inputs), first.device
    ins = [None if x is None else x.contiguous() for x in inputs]
    arr = (ctypes.c_void_p * n)(*[0 if x is None else x.data_ptr() for x in ins])
    st = None if strides is None else (ctypes.c_int * len(strides))(*strides)
    if ws is None:
        ws = torch.empty(max(L.trtx_yolo_decode_workspace(max(B, 1), net_h, net_w, st, len(strides or ())), 256), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.zeros((max(B, 1), 1 + max_out * DET10_FLOATS), dtype=torch.float32, device=dev)
    status = L.trtx_yolov10_decode(arr, n if n_levels is None else n_levels, B, classes, net_h, net_w, st, max_out, _p(out), _p(ws),
                                   ctypes.c_size_t(ws.numel()), _stream())
    if status_only:
        return status
    check(status, "trtx_yolov10_decode")
    return out


def yolov10_head_decode_workspace(batch, net_h, net_w, strides):
    L = lib()
    L.trtx_yolov10_head_decode_workspace.restype = ctypes.c_size_t
    return L.trtx_yolov10_head_decode_workspace(batch, net_h, net_w, (ctypes.c_int * len(strides))(*strides), len(strides))


def yolov10_head_decode_nhwc(heads, classes, net_h, net_w, strides, dfl_w, max_out=1000, out=None, ws=None, batch=None, ld=None, n_levels=None,
                             status_only=False):
    """The fused YOLOv10 head on NHWC head tensors [B, gh, gw, ld] (fp16 or fp32): trtx_yolov10_head_decode_nhwc{,_f32}, any class count.
    -> [B, 1 + max_out * 6].  The keyword arguments as in yolo_head_decode_nhwc."""
    import torch
    L = lib()
    hp, hl = _head_table(heads)
    if ld is not None:
        hl = (ctypes.c_int * len(ld))(*ld)
    B, n, dev = heads[0].shape[0] if batch is None else batch, len(heads), heads[0].device
    st = None if strides is None else (ctypes.c_int * len(strides))(*strides)
    if ws is None:
        ws = torch.empty(max(yolov10_head_decode_workspace(B, net_h, net_w, strides), 256), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.zeros(B, 1 + max_out * DET10_FLOATS, dtype=torch.float32, device=dev)
    fn = L.trtx_yolov10_head_decode_nhwc_f32 if heads[0].dtype == torch.float32 else L.trtx_yolov10_head_decode_nhwc
    status = fn(hp, hl, n if n_levels is None else n_levels, B, classes, net_h, net_w, st, _p(dfl_w), max_out, _p(out), _p(ws),
                ctypes.c_size_t(ws.numel()), _stream())
    if status_only:
        return status
    check(status, "trtx_yolov10_head_decode_nhwc")
    return out


def yolov10_topk(decode_out, max_out=1000, conf_thresh=0.5, topk=0, out=None, batch=None, status_only=False):
    """get_topk / batch_topk on the device (yolov10/src/postprocess.cpp:35-52): trtx_yolov10_topk.  decode_out [B, 1 + max_out * 6] ->
    a buffer of the same shape: row[0] = records kept, then the records.  topk <= 0: conf > conf_thresh in slot order (the reference);
    topk > 0: the topk highest of those by descending conf, ties in slot order.  `out`: the caller's buffer (None: zeros)."""
    import torch
    B = decode_out.shape[0] if batch is None else batch
    if out is None:
        out = torch.zeros((max(B, 1), 1 + max_out * DET10_FLOATS), dtype=torch.float32, device=decode_out.device)
    status = lib().trtx_yolov10_topk(_p(decode_out), B, max_out, ctypes.c_float(conf_thresh), int(topk), _p(out), _stream())
    if status_only:
        return status
    check(status, "trtx_yolov10_topk")
    return out
