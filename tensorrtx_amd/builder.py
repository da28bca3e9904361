"""ctypes binding of the network-definition half of the C ABI (include/trtx_hip.h section 2: createInferBuilder /
createNetworkV2 / INetworkDefinition::add* / buildSerializedNetwork).  The C++ host builders go through include/NvInfer.h;
this thin Python spelling exists for tests and tools that assemble small ad-hoc networks."""
import ctypes

import numpy as np

from .capi import check, lib
from .engine import Dims

P_STRIDE, P_PADDING, P_DILATION, P_GROUPS, P_KERNEL, P_NB_OUT = 1, 2, 3, 4, 15, 16
TRTX_P_ALPHA, TRTX_P_RESIZE_SCALES, TRTX_P_RESIZE_OUT_DIMS, TRTX_P_AVG_EXCLUSIVE = 5, 12, 13, 14
TRTX_P_AXIS, TRTX_P_RESHAPE, TRTX_P_FIRST_TRANSPOSE, TRTX_P_SECOND_TRANSPOSE = 7, 8, 9, 10
ACT = {"relu": 0, "sigmoid": 1, "tanh": 2, "leaky": 3}
EW = {"sum": 0, "prod": 1, "max": 2, "min": 3, "sub": 4, "div": 5, "pow": 6}
REDUCE = {"sum": 0, "max": 2, "avg": 4}
UNARY = {"exp": 0, "log": 1, "sqrt": 2, "recip": 3, "abs": 4, "neg": 5}
FLAG_FP16, FLAG_INT8 = 0, 1


def _dims(shape):
    d = Dims()
    d.nb = len(shape)
    for i, v in enumerate(shape):
        d.d[i] = int(v)
    return d


def _f(a):
    a = None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    return a, (a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None), (0 if a is None else a.size)


class Network:
    def __init__(self, max_batch=1, fp16=False, int8=False, explicit_batch=False):
        L = lib()
        self.L = L
        self.b = ctypes.c_void_p()
        check(L.trtx_builder_create(ctypes.byref(self.b)), "trtx_builder_create")
        check(L.trtx_builder_set_max_batch(self.b, max_batch), "set_max_batch")
        if fp16:
            check(L.trtx_builder_set_flag(self.b, FLAG_FP16, 1), "set_flag fp16")
        if int8:
            check(L.trtx_builder_set_flag(self.b, FLAG_INT8, 1), "set_flag int8")
        self.n = ctypes.c_void_p()
        check(L.trtx_network_create(self.b, 1 if explicit_batch else 0, ctypes.byref(self.n)), "trtx_network_create")
        self._keep = []

    def _layer(self, idx, what):
        if idx < 0:
            self.L.trtx_network_last_error.restype = ctypes.c_char_p
            raise RuntimeError(f"{what}: {self.L.trtx_network_last_error(self.n)}")
        return idx

    def out(self, layer, i=0):
        return self.L.trtx_layer_output(self.n, layer, i)

    def input(self, name, shape):
        d = _dims(shape)
        return self._layer(self.L.trtx_add_input(self.n, name.encode(), 0, ctypes.byref(d)), "add_input")

    def _set2(self, layer, param, v):
        arr = (ctypes.c_int32 * 2)(v, v) if np.isscalar(v) else (ctypes.c_int32 * 2)(*v)
        check(self.L.trtx_layer_set_ints(self.n, layer, param, arr, 2), "trtx_layer_set_ints")

    def conv(self, x, w, bias=None, stride=1, padding=0, deconv=False, groups=1, dilation=1):
        """w: KCRS (conv, C = input channels / groups) or CKRS (deconv, K = output channels / groups) fp32 numpy; stride, padding and
        dilation: one int or (h, w); returns the layer index"""
        w = np.ascontiguousarray(w, dtype=np.float32)
        nb_out = w.shape[1] * groups if deconv else w.shape[0]
        wa, wp, wn = _f(w)
        ba, bp, bn = _f(bias)
        self._keep += [wa, ba]
        fn = self.L.trtx_add_deconvolution if deconv else self.L.trtx_add_convolution
        l = self._layer(fn(self.n, x, nb_out, w.shape[2], w.shape[3], wp, ctypes.c_int64(wn), bp, ctypes.c_int64(bn)), "add_conv")
        self._set2(l, P_STRIDE, stride)
        self._set2(l, P_PADDING, padding)
        if not np.isscalar(dilation) or dilation != 1:
            self._set2(l, P_DILATION, dilation)
        if groups != 1:
            check(self.L.trtx_layer_set_ints(self.n, l, P_GROUPS, (ctypes.c_int32 * 1)(groups), 1), "trtx_layer_set_ints(groups)")
        return l

    def activation(self, x, kind, alpha=None):
        """IActivationLayer; alpha: setAlpha (the slope of kLEAKY_RELU; the layer's default is 0.01)"""
        l = self._layer(self.L.trtx_add_activation(self.n, x, ACT[kind]), "add_activation")
        if alpha is not None:
            check(self.L.trtx_layer_set_floats(self.n, l, TRTX_P_ALPHA, (ctypes.c_float * 1)(float(alpha)), 1), "trtx_layer_set_floats(alpha)")
        return l

    def scale(self, x, shift, scale, power=None):
        """IScaleLayer, ScaleMode::kCHANNEL (a folded BatchNorm, e.g. addBatchNorm2d of yolov4/yolov4.cpp:181-197)"""
        sa, sp, sn = _f(shift)
        ca, cp, cn = _f(scale)
        pa, pp, pn = _f(np.ones_like(sa) if power is None else power)
        self._keep += [sa, ca, pa]
        return self._layer(self.L.trtx_add_scale(self.n, x, 1, sp, ctypes.c_int64(sn), cp, ctypes.c_int64(cn), pp, ctypes.c_int64(pn)), "add_scale")

    def plugin(self, inputs, name, version="1", fields=None):
        """getPluginRegistry()->getPluginCreator(name, version)->createPlugin(name, field collection), then addPluginV2 - with the empty
        collection what convBnMish does for "Mish_TRT" (yolov4/yolov4.cpp:207-212).  fields: [(name, int32 / float32 / uint8 array)] or
        [(name, array, length)] where the creator counts elements of a struct type (the "kernels" field of the anchor-based
        "YoloLayer_TRT", yolov5/src/model.cpp:270-273).  The v-tables are opaque blobs here (sized generously)."""
        creator = (ctypes.c_void_p * 8)()
        self.L.trtx_registry_get.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p]
        self.L.trtx_add_plugin_v2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        check(self.L.trtx_registry_get(name.encode(), version.encode(), ctypes.cast(creator, ctypes.c_void_p)), f"no plugin creator {name}/{version}")
        create = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p)(creator[3])
        vt = (ctypes.c_void_p * 16)()
        farr, nf, keep = None, 0, []
        if fields:
            class Field(ctypes.Structure):   # trtx_plugin_field
                _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("type", ctypes.c_int32), ("length", ctypes.c_int32)]
            nf = len(fields)
            farr = (Field * nf)()
            for i, f in enumerate(fields):
                a = np.ascontiguousarray(f[1])
                keep.append(a)
                code = 5 if a.dtype == np.int32 else (1 if a.dtype == np.float32 else 6)   # nvinfer1::PluginFieldType
                farr[i] = Field(f[0].encode(), a.ctypes.data_as(ctypes.c_void_p), code, f[2] if len(f) > 2 else a.size)
            farr = ctypes.cast(farr, ctypes.c_void_p)
        if create(creator[0], name.encode(), farr, nf, ctypes.cast(vt, ctypes.c_void_p)) != 0:
            raise RuntimeError(f"createPlugin({name}) failed")
        arr = (ctypes.c_int32 * len(inputs))(*inputs)
        l = self._layer(self.L.trtx_add_plugin_v2(self.n, ctypes.cast(arr, ctypes.c_void_p), len(inputs), ctypes.cast(vt, ctypes.c_void_p)), "add_plugin_v2")
        destroy = ctypes.CFUNCTYPE(None, ctypes.c_void_p)(vt[13])   # the network holds its own clone
        destroy(vt[0])
        return l

    def pooling(self, x, k, stride, padding=0, avg=False, avg_exclusive=None):
        """IPoolingLayer; k, stride, padding: one int or (h, w); avg_exclusive: setAverageCountExcludesPadding"""
        kh, kw = (k, k) if np.isscalar(k) else k
        l = self._layer(self.L.trtx_add_pooling(self.n, x, 1 if avg else 0, kh, kw), "add_pooling")
        self._set2(l, P_STRIDE, stride)
        self._set2(l, P_PADDING, padding)
        if avg_exclusive is not None:
            check(self.L.trtx_layer_set_ints(self.n, l, TRTX_P_AVG_EXCLUSIVE, (ctypes.c_int32 * 1)(int(avg_exclusive)), 1),
                  "trtx_layer_set_ints(avg_exclusive)")
        return l

    def elementwise(self, a, b, op=0):
        """IElementWiseLayer; op: an ElementWiseOperation code or its name in EW"""
        return self._layer(self.L.trtx_add_elementwise(self.n, a, b, EW.get(op, op)), "add_elementwise")

    def resize_nearest(self, x, scale=2, out_dims=None):
        """IResizeLayer, nearest: integer scale on H and W (setScales({1, s, s})), or out_dims = the full output dims (setOutputDimensions)"""
        l = self._layer(self.L.trtx_add_resize(self.n, x), "add_resize")
        if out_dims is not None:
            d = _dims(out_dims)
            check(self.L.trtx_layer_set_dims(self.n, l, TRTX_P_RESIZE_OUT_DIMS, ctypes.byref(d)), "trtx_layer_set_dims(resize out dims)")
            return l
        sc = (ctypes.c_float * 3)(1.0, float(scale), float(scale))
        check(self.L.trtx_layer_set_floats(self.n, l, TRTX_P_RESIZE_SCALES, sc, 3), "trtx_layer_set_floats(resize scales)")
        return l

    def reduce(self, x, op, axes, keep_dims=False):
        """IReduceLayer; op: "sum" / "avg" / "max"; axes: bit mask over the tensor's dims"""
        self.L.trtx_add_reduce.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32]
        return self._layer(self.L.trtx_add_reduce(self.n, x, REDUCE.get(op, op), int(axes), int(bool(keep_dims))), "add_reduce")

    def fully_connected(self, x, w, bias=None):
        """IFullyConnectedLayer on a (C, H, W) tensor; w: (nb_out, C * H * W)"""
        w = np.ascontiguousarray(w, dtype=np.float32)
        wa, wp, wn = _f(w)
        ba, bp, bn = _f(bias)
        self._keep += [wa, ba]
        return self._layer(self.L.trtx_add_fully_connected(self.n, x, w.shape[0], wp, ctypes.c_int64(wn), bp, ctypes.c_int64(bn)), "add_fully_connected")

    def constant(self, values):
        """IConstantLayer: a tensor of values.shape (no batch dimension in an implicit-batch network)"""
        va, vp, vn = _f(values)
        self._keep.append(va)
        d = _dims(va.shape)
        return self._layer(self.L.trtx_add_constant(self.n, ctypes.byref(d), vp, ctypes.c_int64(vn)), "add_constant")

    def identity(self, x):
        return self._layer(self.L.trtx_add_identity(self.n, x), "add_identity")

    def unary(self, x, op="exp"):
        """IUnaryLayer; op: a UnaryOperation code or its name in UNARY (only kEXP has a kernel: build() refuses the others by name)"""
        self.L.trtx_network_add_unary.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
        return self._layer(self.L.trtx_network_add_unary(self.n, x, UNARY.get(op, op)), "add_unary")

    def padding(self, x, pre=(0, 0), post=(0, 0)):
        """IPaddingLayer (addPaddingNd), zero fill: pre = (top, left), post = (bottom, right); build() refuses a negative (cropping) value"""
        a, b = _dims(pre), _dims(post)
        self.L.trtx_add_padding.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        return self._layer(self.L.trtx_add_padding(self.n, x, ctypes.byref(a), ctypes.byref(b)), "add_padding")

    def slice_channels(self, x, start, size, chw):
        """ISliceLayer over the channel axis of a (C, H, W) tensor: channels [start, start + size) (block.cpp:134-149, the C2f split)"""
        c, h, w = chw
        st, sz, sp = _dims((start, 0, 0)), _dims((size, h, w)), _dims((1, 1, 1))
        return self._layer(self.L.trtx_add_slice(self.n, x, ctypes.byref(st), ctypes.byref(sz), ctypes.byref(sp)), "add_slice")

    def slice(self, x, start, size, step=None):
        """ISliceLayer, any rank"""
        st, sz, sp = _dims(start), _dims(size), _dims(step if step is not None else (1,) * len(start))
        return self._layer(self.L.trtx_add_slice(self.n, x, ctypes.byref(st), ctypes.byref(sz), ctypes.byref(sp)), "add_slice")

    def shuffle(self, x, reshape=None, perm1=None, perm2=None):
        """IShuffleLayer: first transpose, reshape (0 copies, -1 infers), second transpose"""
        l = self._layer(self.L.trtx_add_shuffle(self.n, x), "add_shuffle")
        for param, perm in ((TRTX_P_FIRST_TRANSPOSE, perm1), (TRTX_P_SECOND_TRANSPOSE, perm2)):
            if perm is not None:
                check(self.L.trtx_layer_set_ints(self.n, l, param, (ctypes.c_int32 * len(perm))(*perm), len(perm)), "trtx_layer_set_ints(transpose)")
        if reshape is not None:
            d = _dims(reshape)
            check(self.L.trtx_layer_set_dims(self.n, l, TRTX_P_RESHAPE, ctypes.byref(d)), "trtx_layer_set_dims(reshape)")
        return l

    def softmax(self, x, axes=None):
        """ISoftMaxLayer; axes: bit mask (setAxes), None keeps the default axis"""
        l = self._layer(self.L.trtx_add_softmax(self.n, x), "add_softmax")
        if axes is not None:
            check(self.L.trtx_layer_set_ints(self.n, l, TRTX_P_AXIS, (ctypes.c_int32 * 1)(axes), 1), "trtx_layer_set_ints(axes)")
        return l

    def matmul(self, a, b, transpose_a=False, transpose_b=False):
        """IMatrixMultiplyLayer, MatrixOperation kNONE / kTRANSPOSE"""
        return self._layer(self.L.trtx_add_matrix_multiply(self.n, a, int(transpose_a), b, int(transpose_b)), "add_matrix_multiply")

    def scale_uniform(self, x, scale, shift=0.0, power=1.0):
        """IScaleLayer, ScaleMode::kUNIFORM (the Attention's score scale, yolo11/src/block.cpp:313-324)"""
        sa, sp, sn = _f(np.array([shift]))
        ca, cp, cn = _f(np.array([scale]))
        pa, pp, pn = _f(np.array([power]))
        self._keep += [sa, ca, pa]
        return self._layer(self.L.trtx_add_scale(self.n, x, 0, sp, ctypes.c_int64(sn), cp, ctypes.c_int64(cn), pp, ctypes.c_int64(pn)), "add_scale")

    def concat(self, tensors, axis=None):
        """IConcatenationLayer; axis: setAxis (None keeps the default, the channel axis)"""
        arr = (ctypes.c_int32 * len(tensors))(*tensors)
        l = self._layer(self.L.trtx_add_concatenation(self.n, arr, len(tensors)), "add_concatenation")
        if axis is not None:
            check(self.L.trtx_layer_set_ints(self.n, l, TRTX_P_AXIS, (ctypes.c_int32 * 1)(axis), 1), "trtx_layer_set_ints(axis)")
        return l

    def mark_output(self, tensor, name):
        check(self.L.trtx_tensor_set_name(self.n, tensor, name.encode()), "set_name")
        check(self.L.trtx_mark_output(self.n, tensor), "mark_output")

    def set_int8_calibrator(self, cal):
        """IBuilderConfig::setInt8Calibrator: cal is a tensorrtx_amd.calibrator.Calibrator (kept alive by this object)"""
        self._keep.append(cal)
        check(self.L.trtx_builder_set_int8_calibrator(self.b, ctypes.byref(cal.vtbl)), "trtx_builder_set_int8_calibrator")

    def build(self):
        hm = ctypes.c_void_p()
        check(self.L.trtx_build_serialized(self.b, self.n, ctypes.byref(hm)), "trtx_build_serialized")
        self.L.trtx_hostmem_data.restype = ctypes.c_void_p
        self.L.trtx_hostmem_size.restype = ctypes.c_size_t
        plan = ctypes.string_at(self.L.trtx_hostmem_data(hm), self.L.trtx_hostmem_size(hm))
        self.L.trtx_hostmem_destroy(hm)
        return plan

    def close(self):
        if self.n:
            self.L.trtx_network_destroy(self.n)
            self.n = None
        if self.b:
            self.L.trtx_builder_destroy(self.b)
            self.b = None
