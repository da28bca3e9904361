"""Seeded synthetic inputs of the shapes SURVEY.md §8(d) prescribes (no datasets / weights offline)."""
import numpy as np


def yolo_head_tensors(batch, classes=80, net_h=640, net_w=640, strides=(8, 16, 32), objects=(40, 180), seed=0,
                      bg_mean=-8.0, bg_std=1.5):
    """Planted-object head tensors for the YoloLayer plugin: list of [B, 4+classes, gh*gw] fp32.

    Box channels ltrb ~ U(0, 10) cells, class logits ~ N(bg_mean, bg_std^2); per image K in `objects`
    planted objects: one class gets logit +4..+8 on 3-8 neighbouring cells with consistent boxes so
    that NMS clusters exist (candidates(sigma >= 0.1) << 1000, survivors(conf > 0.5) ~ 100-600).
    """
    rng = np.random.default_rng(seed)
    outs = []
    for s in strides:
        gh, gw = net_h // s, net_w // s
        x = np.empty((batch, 4 + classes, gh * gw), dtype=np.float32)
        x[:, :4] = rng.uniform(0.0, 10.0, size=(batch, 4, gh * gw)).astype(np.float32)
        x[:, 4:] = rng.normal(bg_mean, bg_std, size=(batch, classes, gh * gw)).astype(np.float32)
        outs.append(x)
    for b in range(batch):
        k_obj = int(rng.integers(objects[0], objects[1] + 1))
        for _ in range(k_obj):
            l = int(rng.integers(0, len(strides)))
            s = strides[l]
            gh, gw = net_h // s, net_w // s
            row, col = int(rng.integers(1, gh - 1)), int(rng.integers(1, gw - 1))
            cls = int(rng.integers(0, classes))
            # object box in pixels around the anchor point
            cx, cy = (col + 0.5) * s, (row + 0.5) * s
            hw_, hh_ = rng.uniform(1.0, 6.0) * s, rng.uniform(1.0, 6.0) * s
            x1, y1, x2, y2 = cx - hw_, cy - hh_, cx + hw_, cy + hh_
            n_cells = int(rng.integers(3, 9))
            for _c in range(n_cells):
                r = min(max(row + int(rng.integers(-1, 2)), 0), gh - 1)
                c = min(max(col + int(rng.integers(-1, 2)), 0), gw - 1)
                e = r * gw + c
                jit = rng.normal(0.0, 0.15, size=4)
                outs[l][b, 0, e] = (c + 0.5) - x1 / s + jit[0]
                outs[l][b, 1, e] = (r + 0.5) - y1 / s + jit[1]
                outs[l][b, 2, e] = x2 / s - (c + 0.5) + jit[2]
                outs[l][b, 3, e] = y2 / s - (r + 0.5) + jit[3]
                outs[l][b, 4 + cls, e] = rng.uniform(0.5, 8.0)
    return outs


def images(batch, h=640, w=640, seed=0, n_rect=(8, 30)):
    """Synthetic RGB images in [0, 1], [B, 3, H, W] fp32: dark noisy background with random bright
    rectangles, so that a randomly initialised detector sees spatially varying features
    (uniform noise alone averages out to a constant feature map)."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 0.15, size=(batch, 3, h, w)).astype(np.float32)
    for b in range(batch):
        for _ in range(int(rng.integers(n_rect[0], n_rect[1] + 1))):
            rw, rh = int(rng.integers(w // 40, w // 4)), int(rng.integers(h // 40, h // 4))
            x0, y0 = int(rng.integers(0, w - rw)), int(rng.integers(0, h - rh))
            col = rng.uniform(0.2, 1.0, size=(3, 1, 1)).astype(np.float32)
            img[b, :, y0:y0 + rh, x0:x0 + rw] = col + rng.normal(0, 0.03, size=(3, rh, rw)).astype(np.float32)
    return np.clip(img, 0.0, 1.0)


def retina_head_tensors(batch, net_h, net_w, faces=200, seed=0):
    """RetinaFace plugin inputs: list of [B, 32, h*w] fp32 for stride 8/16/32 =
    bbox(2x4) | cls(2x2) | landmark(2x10) planes; cls pair difference ~ N(-5, 2^2), deltas ~ N(0, 1),
    ~`faces` planted high-confidence anchors per image with clustered neighbours."""
    rng = np.random.default_rng(seed)
    outs = []
    for s in (8, 16, 32):
        h, w = net_h // s, net_w // s
        x = rng.normal(0.0, 1.0, size=(batch, 32, h * w)).astype(np.float32)
        diff = rng.normal(-5.0, 2.0, size=(batch, 2, h * w)).astype(np.float32)
        base = rng.normal(0.0, 1.0, size=(batch, 2, h * w)).astype(np.float32)
        x[:, 8] = base[:, 0]; x[:, 9] = base[:, 0] + diff[:, 0]      # k = 0: (conf1, conf2)
        x[:, 10] = base[:, 1]; x[:, 11] = base[:, 1] + diff[:, 1]    # k = 1
        outs.append(x)
    for b in range(batch):
        for _ in range(faces):
            l = int(rng.integers(0, 3))
            h, w = net_h // (8 << l), net_w // (8 << l)
            cy, cx, k = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(0, 2))
            for dy, dx in ((0, 0), (0, 1), (1, 0)):
                y, x_ = min(cy + dy, h - 1), min(cx + dx, w - 1)
                e = y * w + x_
                outs[l][b, 8 + 2 * k + 1, e] = outs[l][b, 8 + 2 * k, e] + rng.uniform(1.0, 6.0)
                outs[l][b, 4 * k:4 * k + 4, e] = rng.normal(0, 0.3, size=4)
    return outs


def rcnn_rpn_tensors(batch, anchors=15, h=50, w=84, seed=0):
    """RPN head outputs (C5): logits ~ N(0, 2^2) [B, A, h, w], deltas ~ N(0, 0.5^2) [B, 4A, h, w]."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 2.0, size=(batch, anchors, h, w)).astype(np.float32),
            rng.normal(0, 0.5, size=(batch, anchors * 4, h, w)).astype(np.float32))


def rcnn_box_head_tensors(batch, n=1000, classes=80, img_h=800, img_w=1333, seed=0):
    """Box-head outputs (C5): softmax scores from logits ~ N(0, 3^2) over classes+1 (background dropped),
    deltas ~ N(0, 1) [B, N, C, 4], proposals = random boxes inside the image."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 3.0, size=(batch, n, classes + 1))
    e = np.exp(logits - logits.max(-1, keepdims=True))
    scores = (e / e.sum(-1, keepdims=True))[..., :classes].astype(np.float32)
    deltas = rng.normal(0, 1.0, size=(batch, n, classes, 4)).astype(np.float32)
    x1 = rng.uniform(0, img_w - 40, size=(batch, n)); y1 = rng.uniform(0, img_h - 40, size=(batch, n))
    bw = rng.uniform(8, 300, size=(batch, n)); bh = rng.uniform(8, 300, size=(batch, n))
    props = np.stack([x1, y1, np.minimum(x1 + bw, img_w), np.minimum(y1 + bh, img_h)], -1).astype(np.float32)
    return scores, deltas, props


def yolov8n_state(seed=0, num_class=80):
    """Seeded synthetic weights of YOLOv8n-det under the reference's `.wts` key names (ultralytics state_dict keys, as
    read by yolov8/src/block.cpp:79-257 / model.cpp:98-310): OrderedDict name -> fp32 array.  Trained weights cannot be
    obtained offline; the values are He-scaled with near-identity BatchNorm statistics, the class head has gain 80 and
    bias -7 so that a few hundred cells per image pass the 0.1 confidence gate.  Used by bench.py (product side: no oracle
    involved).  Draw order and distributions are those of the test-suite's generator, so both produce the same file
    (tests/test_runtime_cpu.py::test_product_side_yolov8n_weights_match_the_test_generator)."""
    import math
    from collections import OrderedDict

    import torch
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    randn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    rand = lambda *shape: torch.rand(*shape, generator=g)    # noqa: E731

    def conv(name, cout, cin, k, gain=2.0):
        sd[name + ".weight"] = (randn(cout, cin, k, k) * math.sqrt(gain / (cin * k * k))).float()

    def cbs(name, cout, cin, k):  # Conv + BatchNorm (+ SiLU)
        conv(name + ".conv", cout, cin, k)
        sd[name + ".bn.weight"] = (1.0 * (0.9 + 0.2 * rand(cout))).float()
        sd[name + ".bn.bias"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_mean"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_var"] = (0.8 + 0.4 * rand(cout)).float()
        sd[name + ".bn.num_batches_tracked"] = torch.zeros(1)

    def c2f(name, cin, c2, n):
        c_ = c2 // 2
        cbs(name + ".cv1", 2 * c_, cin, 1)
        for i in range(n):
            cbs(f"{name}.m.{i}.cv1", c_, c_, 3)
            cbs(f"{name}.m.{i}.cv2", c_, c_, 3)
        cbs(name + ".cv2", c2, (2 + n) * c_, 1)

    cbs("model.0", 16, 3, 3)
    cbs("model.1", 32, 16, 3)
    c2f("model.2", 32, 32, 1)
    cbs("model.3", 64, 32, 3)
    c2f("model.4", 64, 64, 2)
    cbs("model.5", 128, 64, 3)
    c2f("model.6", 128, 128, 2)
    cbs("model.7", 256, 128, 3)
    c2f("model.8", 256, 256, 1)
    cbs("model.9.cv1", 128, 256, 1)
    cbs("model.9.cv2", 256, 512, 1)
    c2f("model.12", 384, 128, 1)
    c2f("model.15", 192, 64, 1)
    cbs("model.16", 64, 64, 3)
    c2f("model.18", 192, 128, 1)
    cbs("model.19", 128, 128, 3)
    c2f("model.21", 384, 256, 1)
    c3 = max(64, min(num_class, 100))
    for lv, cin in enumerate((64, 128, 256)):
        cbs(f"model.22.cv2.{lv}.0", 64, cin, 3)
        cbs(f"model.22.cv2.{lv}.1", 64, 64, 3)
        conv(f"model.22.cv2.{lv}.2", 64, 64, 1, gain=4.0)
        sd[f"model.22.cv2.{lv}.2.bias"] = (1.0 + 0.1 * randn(64)).float()
        cbs(f"model.22.cv3.{lv}.0", c3, cin, 3)
        cbs(f"model.22.cv3.{lv}.1", c3, c3, 3)
        conv(f"model.22.cv3.{lv}.2", num_class, c3, 1, gain=80.0)
        sd[f"model.22.cv3.{lv}.2.bias"] = (-7.0 + 0.1 * randn(num_class)).float()
        if lv == 0:
            sd["model.22.dfl.conv.weight"] = torch.arange(16.0).reshape(1, 16, 1, 1)
    return OrderedDict((k, v.numpy()) for k, v in sd.items())


YOLO11_SCALES = {  # yolo11_det.cpp:120-150: gd, gw, max_channels; m / l / x use C3k blocks (model.cpp:160-163)
    "n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512), "l": (1.00, 1.00, 512), "x": (1.00, 1.50, 512)}


YOLO11_TASK_CLS_BIAS = {0: -8.0, 1: -8.0, 2: -2.0, 3: -5.0}   # class-head bias per task: one (pose) or 15 (obb) classes need a higher one


def yolo11_state(scale="n", seed=0, num_class=80, task=0):
    """Seeded synthetic weights of YOLO11{n,s,m,l,x} under the reference's `.wts` key names (ultralytics state_dict keys, as
    read by yolo11/src/block.cpp / model.cpp): OrderedDict name -> fp32 array.  He-scaled convolutions with near-identity
    BatchNorm statistics (the yolov8n_state recipe); the class head has gain 800 and bias -8 (det / seg; see YOLO11_TASK_CLS_BIAS)
    so that a few hundred cells per image pass the 0.1 confidence gate.

    task: 0 det, 1 seg, 2 pose, 3 obb, 4 cls.  The task tensors (model.23.cv4.*, model.23.proto.*) are drawn after every det
    tensor, so a seg / pose / obb model shares its backbone and neck with the det model of the same seed, and its detect head as
    well when num_class is the same (the class biases are drawn num_class at a time, so every later draw moves with it).  cls
    (model.cpp:33-136) has its own keys after model.8: C2PSA as model.9, then model.10.conv and model.10.linear."""
    import math
    from collections import OrderedDict

    import torch
    gd, gw, mc = YOLO11_SCALES[scale]
    c3k = scale in "mlx"
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    randn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    rand = lambda *shape: torch.rand(*shape, generator=g)    # noqa: E731

    def W(x):
        return int(math.ceil(min(x, mc) * gw / 8)) * 8

    def D(x):
        if x == 1:
            return 1
        r = round(x * gd)   # Python's round: half to even, as get_depth
        return max(int(r), 1)

    def conv(name, cout, cin, k, gain=2.0):
        sd[name + ".weight"] = (randn(cout, cin, k, k) * math.sqrt(gain / (cin * k * k))).float()

    def cb(name, cout, cin, k, groups=1, gain=2.0):  # Conv + BatchNorm (+ SiLU)
        conv(name + ".conv", cout, cin // groups, k, gain)
        sd[name + ".bn.weight"] = (0.9 + 0.2 * rand(cout)).float()
        sd[name + ".bn.bias"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_mean"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_var"] = (0.8 + 0.4 * rand(cout)).float()
        sd[name + ".bn.num_batches_tracked"] = torch.zeros(1)

    def bottleneck(name, c1, c2, e):
        c_ = int(c2 * e)
        cb(name + ".cv1", c_, c1, 3)
        cb(name + ".cv2", c2, c_, 3)

    def c3k_block(name, c1, c2, n, e=0.5):
        c_ = int(c2 * e)
        cb(name + ".cv1", c_, c1, 1)
        cb(name + ".cv2", c_, c1, 1)
        for i in range(n):
            bottleneck(f"{name}.m.{i}", c_, c_, 1.0)
        cb(name + ".cv3", c2, 2 * c_, 1)

    def c3k2(name, c1, c2, n, use_c3k, e):
        c_ = int(c2 * e)
        cb(name + ".cv1", 2 * c_, c1, 1)
        for i in range(n):
            if use_c3k:
                c3k_block(f"{name}.m.{i}", c_, c_, 2)
            else:
                bottleneck(f"{name}.m.{i}", c_, c_, 0.5)
        cb(name + ".cv2", c2, (2 + n) * c_, 1)

    def c2psa(name, c1, c2, n):
        c = int(c1 * 0.5)
        cb(name + ".cv1", 2 * c, c1, 1)
        heads = c // 64
        kd = (c // heads) // 2
        for i in range(n):
            m = f"{name}.m.{i}"
            cb(m + ".attn.qkv", c + 2 * kd * heads, c, 1)
            cb(m + ".attn.proj", c, c, 1, gain=1.0)
            cb(m + ".attn.pe", c, c, 3, groups=c, gain=1.0)
            cb(m + ".ffn.0", 2 * c, c, 1)
            cb(m + ".ffn.1", c, 2 * c, 1, gain=1.0)
        cb(name + ".cv2", c2, 2 * c, 1)

    cb("model.0", W(64), 3, 3)
    cb("model.1", W(128), W(64), 3)
    c3k2("model.2", W(128), W(256), D(2), c3k, 0.25)
    cb("model.3", W(256), W(256), 3)
    c3k2("model.4", W(256), W(512), D(2), c3k, 0.25)
    cb("model.5", W(512), W(512), 3)
    c3k2("model.6", W(512), W(512), D(2), True, 0.5)
    cb("model.7", W(1024), W(512), 3)
    c3k2("model.8", W(1024), W(1024), D(2), True, 0.5)
    if task == 4:
        c2psa("model.9", W(1024), W(1024), D(2))
        cb("model.10.conv", 1280, W(1024), 1)
        sd["model.10.linear.weight"] = (randn(num_class, 1280) * math.sqrt(1.0 / 1280)).float()
        sd["model.10.linear.bias"] = (0.1 * randn(num_class)).float()
        return OrderedDict((k, v.numpy()) for k, v in sd.items())
    cb("model.9.cv1", W(1024) // 2, W(1024), 1)
    cb("model.9.cv2", W(1024), 2 * W(1024), 1)
    c2psa("model.10", W(1024), W(1024), D(2))
    c3k2("model.13", W(1024) + W(512), W(512), D(2), c3k, 0.5)
    c3k2("model.16", W(512) + W(512), W(256), D(2), c3k, 0.5)
    cb("model.17", W(256), W(256), 3)
    c3k2("model.19", W(256) + W(512), W(512), D(2), c3k, 0.5)
    cb("model.20", W(512), W(512), 3)
    c3k2("model.22", W(512) + W(1024), W(1024), D(2), True, 0.5)
    c2 = max(16, W(256) // 4, 64)
    c3 = max(W(256), min(num_class, 100))
    for lv, cin in enumerate((W(256), W(512), W(1024))):
        cb(f"model.23.cv2.{lv}.0", c2, cin, 3)
        cb(f"model.23.cv2.{lv}.1", c2, c2, 3)
        conv(f"model.23.cv2.{lv}.2", 64, c2, 1, gain=4.0)
        sd[f"model.23.cv2.{lv}.2.bias"] = (1.0 + 0.1 * randn(64)).float()
        cb(f"model.23.cv3.{lv}.0.0", cin, cin, 3, groups=cin, gain=1.0)
        cb(f"model.23.cv3.{lv}.0.1", c3, cin, 1)
        cb(f"model.23.cv3.{lv}.1.0", c3, c3, 3, groups=c3, gain=1.0)
        cb(f"model.23.cv3.{lv}.1.1", c3, c3, 1)
        conv(f"model.23.cv3.{lv}.2", num_class, c3, 1, gain=800.0)
        sd[f"model.23.cv3.{lv}.2.bias"] = (YOLO11_TASK_CLS_BIAS[task] + 0.1 * randn(num_class)).float()
        if lv == 0:
            sd["model.23.dfl.conv.weight"] = torch.arange(16.0).reshape(1, 16, 1, 1)
    if task in (1, 2, 3):   # cv4_conv_combined (model.cpp:474-507): 32 mask coefficients, 17 * 3 keypoint values or one angle logit
        extra = {1: 32, 2: 17 * 3, 3: 1}[task]
        c4 = max(W(256) // 4, extra)
        for lv, cin in enumerate((W(256), W(512), W(1024))):
            cb(f"model.23.cv4.{lv}.0", c4, cin, 3)
            cb(f"model.23.cv4.{lv}.1", c4, c4, 3)
            conv(f"model.23.cv4.{lv}.2", extra, c4, 1, gain=0.5 if task == 2 else 2.0)   # keypoints stay near their cell
            sd[f"model.23.cv4.{lv}.2.bias"] = (0.1 * randn(extra)).float()
    if task == 1:           # Proto (model.cpp:412-472)
        mid = W(256)
        cb("model.23.proto.cv1", mid, W(256), 3)
        sd["model.23.proto.upsample.weight"] = (randn(mid, mid, 2, 2) * math.sqrt(2.0 / (mid * 4))).float()
        sd["model.23.proto.upsample.bias"] = (0.1 * randn(mid)).float()
        cb("model.23.proto.cv2", mid, mid, 3)
        cb("model.23.proto.cv3", 32, mid, 1)
    return OrderedDict((k, v.numpy()) for k, v in sd.items())


YOLO12_QKV_GAIN = 100.0   # He gain of the q and k rows of the AAttn qkv convolutions: large enough that the softmax over an area's keys is far from uniform


def yolo12_state(scale="n", seed=0, num_class=80):
    """Seeded synthetic weights of YOLOv12{n,s,m,l,x} detection under the reference's `.wts` key names (yolov12/src/block.cpp /
    model.cpp): OrderedDict name -> fp32 array.  The yolo11_state recipe (He-scaled convolutions, near-identity BatchNorm statistics, a
    class head with gain 800 and bias -8; with these backbones most cells pass the 0.1 confidence gate, 6.6k of 8.4k per image for n at
    640 x 640 and all of them for s, so tests that compare detections give the plugin `max_out` above the cell count), and the q and k rows of the qkv
    convolutions of the eight area-attention blocks with gain YOLO12_QKV_GAIN: tests/test_yolo12_cpu.py asserts that the attention these weights
    produce is not uniform, so an engine that averaged V instead of attending would not pass.

    Channel counts follow the reference's A2C2f (block.cpp:459-495), not ultralytics': c = c2 / 4, and cv1, the blocks and the C3k
    branch all work on 2c channels."""
    import math
    from collections import OrderedDict

    import torch
    gd, gw, mc = YOLO11_SCALES[scale]   # yolo12_det.cpp:120-150 has the same table
    c3k = scale in "mlx"
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    randn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    rand = lambda *shape: torch.rand(*shape, generator=g)    # noqa: E731

    def W(x):
        return int(math.ceil(min(x, mc) * gw / 8)) * 8

    def D(x):
        return 1 if x == 1 else max(int(round(x * gd)), 1)

    def conv(name, cout, cin, k, gain=2.0):
        sd[name + ".weight"] = (randn(cout, cin, k, k) * math.sqrt(gain / (cin * k * k))).float()

    def cb(name, cout, cin, k, groups=1, gain=2.0, bias=False):  # Conv + BatchNorm (+ SiLU)
        conv(name + ".conv", cout, cin // groups, k, gain)
        if bias:
            sd[name + ".conv.bias"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.weight"] = (0.9 + 0.2 * rand(cout)).float()
        sd[name + ".bn.bias"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_mean"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_var"] = (0.8 + 0.4 * rand(cout)).float()
        sd[name + ".bn.num_batches_tracked"] = torch.zeros(1)

    def bottleneck(name, c1, c2, e):
        c_ = int(c2 * e)
        cb(name + ".cv1", c_, c1, 3)
        cb(name + ".cv2", c2, c_, 3)

    def c3k_block(name, c1, c2, n, e=0.5):
        c_ = int(c2 * e)
        cb(name + ".cv1", c_, c1, 1)
        cb(name + ".cv2", c_, c1, 1)
        for i in range(n):
            bottleneck(f"{name}.m.{i}", c_, c_, 1.0)
        cb(name + ".cv3", c2, 2 * c_, 1)

    def c3k2(name, c1, c2, n, use_c3k, e):
        c_ = int(c2 * e)
        cb(name + ".cv1", 2 * c_, c1, 1)
        for i in range(n):
            if use_c3k:
                c3k_block(f"{name}.m.{i}", c_, c_, 2)
            else:
                bottleneck(f"{name}.m.{i}", c_, c_, 0.5)
        cb(name + ".cv2", c2, (2 + n) * c_, 1)

    def a2c2f(name, c1, c2, a2):
        c = 2 * int(c2 * 0.25)   # the channel count everything inside works on
        cb(name + ".cv1", c, c1, 1)
        if a2:
            for m in (f"{name}.m.0.0", f"{name}.m.0.1", f"{name}.m.1.0", f"{name}.m.1.1"):
                cb(m + ".attn.qkv", 3 * c, c, 1)
                qk = sd[m + ".attn.qkv.conv.weight"].view(c // 32, 3, 32, c)   # per head: 32 q rows, 32 k rows, 32 v rows
                # the first block of a stage reads cv1's SiLU output, whose common positive mean makes all keys look alike: four times the gain
                qk[:, :2] *= math.sqrt(YOLO12_QKV_GAIN * (4.0 if m.endswith(".m.0.0") else 1.0) / 2.0)
                cb(m + ".attn.pe", c, c, 7, groups=c, gain=1.0, bias=True)
                cb(m + ".attn.proj", c, c, 1, gain=0.1)    # the two residual branches of the eight blocks in a row stay small against
                cb(m + ".mlp.0", 2 * c, c, 1)              # the stream they add to, so it keeps its magnitude to the last block
                cb(m + ".mlp.1", c, 2 * c, 1, gain=0.1)
            cb(name + ".cv2", c2, 3 * c, 1)
        else:
            c3k_block(name + ".m.0", c, c, 2)
            cb(name + ".cv2", c2, 2 * c, 1)

    cb("model.0", W(64), 3, 3)
    cb("model.1", W(128), W(64), 3)
    c3k2("model.2", W(128), W(256), D(2), c3k, 0.25)
    cb("model.3", W(256), W(256), 3)
    c3k2("model.4", W(256), W(512), D(2), c3k, 0.25)
    cb("model.5", W(512), W(512), 3)
    a2c2f("model.6", W(512), W(512), True)
    cb("model.7", W(1024), W(512), 3)
    a2c2f("model.8", W(1024), W(1024), True)
    a2c2f("model.11", W(1024) + W(512), W(512), False)
    a2c2f("model.14", W(512) + W(512), W(256), False)
    cb("model.15", W(256), W(256), 3)
    a2c2f("model.17", W(256) + W(512), W(512), False)
    cb("model.18", W(512), W(512), 3)
    c3k2("model.20", W(512) + W(1024), W(1024), D(2), True, 0.5)
    c2 = max(16, W(256) // 4, 64)
    c3 = max(W(256), min(num_class, 100))
    for lv, cin in enumerate((W(256), W(512), W(1024))):
        cb(f"model.21.cv2.{lv}.0", c2, cin, 3)
        cb(f"model.21.cv2.{lv}.1", c2, c2, 3)
        conv(f"model.21.cv2.{lv}.2", 64, c2, 1, gain=4.0)
        sd[f"model.21.cv2.{lv}.2.bias"] = (1.0 + 0.1 * randn(64)).float()
        cb(f"model.21.cv3.{lv}.0.0", cin, cin, 3, groups=cin, gain=1.0)
        cb(f"model.21.cv3.{lv}.0.1", c3, cin, 1)
        cb(f"model.21.cv3.{lv}.1.0", c3, c3, 3, groups=c3, gain=1.0)
        cb(f"model.21.cv3.{lv}.1.1", c3, c3, 1)
        conv(f"model.21.cv3.{lv}.2", num_class, c3, 1, gain=800.0)
        sd[f"model.21.cv3.{lv}.2.bias"] = (-8.0 + 0.1 * randn(num_class)).float()
        if lv == 0:
            sd["model.21.dfl.conv.weight"] = torch.arange(16.0).reshape(1, 16, 1, 1)
    return OrderedDict((k, v.numpy()) for k, v in sd.items())


class _Draw:
    """Seeded tensor provider of the synthetic-weight generators below: the draw order and distributions are those of the test-suite's
    generator (oracle/models_torch.py run in init mode), so both write the same file - tests/test_runtime_cpu.py asserts it per model.
    A name drawn twice keeps its first position and its LAST value (the R-CNN generator touches res5 from the box and the mask branch)."""

    def __init__(self, seed):
        import torch
        from collections import OrderedDict
        self.torch = torch
        self.g = torch.Generator().manual_seed(seed)
        self.sd = OrderedDict()

    def randn(self, *shape):
        return self.torch.randn(*shape, generator=self.g)

    def rand(self, *shape):
        return self.torch.rand(*shape, generator=self.g)

    def conv_w(self, name, cout, cin, k, gain=2.0):
        import math
        self.sd[name] = (self.randn(cout, cin, k, k) * math.sqrt(gain / (cin * k * k))).float()

    def bn(self, prefix, c, gamma_scale=1.0):
        self.sd[prefix + ".weight"] = (gamma_scale * (0.9 + 0.2 * self.rand(c))).float()
        self.sd[prefix + ".bias"] = (0.1 * self.randn(c)).float()
        self.sd[prefix + ".running_mean"] = (0.1 * self.randn(c)).float()
        self.sd[prefix + ".running_var"] = (0.8 + 0.4 * self.rand(c)).float()
        self.sd[prefix + ".num_batches_tracked"] = self.torch.zeros(1)

    def state(self):
        from collections import OrderedDict
        return OrderedDict((k, v.numpy()) for k, v in self.sd.items())


def _resnet50_body(d, prefix, bn3_gamma):
    """conv1 / bn1 + the 16 bottlenecks of torchvision's ResNet-50 naming (resnet/resnet50.cpp:155-229, retinaface/retina_r50.cpp:100-140)"""
    def conv_bn(cname, bname, cout, cin, k):
        d.conv_w(cname + ".weight", cout, cin, k)
        d.bn(bname, cout, bn3_gamma if bname.endswith("bn3") else 1.0)
    conv_bn(prefix + "conv1", prefix + "bn1", 64, 3, 7)
    inch = 64
    for stage, nblk in enumerate((3, 4, 6, 3)):
        width = 64 << stage
        for b in range(nblk):
            l = f"{prefix}layer{stage + 1}.{b}."
            stride = 2 if (b == 0 and stage > 0) else 1
            conv_bn(l + "conv1", l + "bn1", width, inch, 1)
            conv_bn(l + "conv2", l + "bn2", width, width, 3)
            conv_bn(l + "conv3", l + "bn3", width * 4, width, 1)
            if stride != 1 or inch != width * 4:
                conv_bn(l + "downsample.0", l + "downsample.1", width * 4, inch, 1)
            inch = width * 4


def resnet50_state(seed=0):
    """Seeded synthetic ResNet-50 weights under the keys resnet/resnet50.cpp reads (torchvision state_dict): OrderedDict name -> fp32 array."""
    import math
    d = _Draw(seed)
    _resnet50_body(d, "", 1.0)
    d.sd["fc.weight"] = (d.randn(1000, 2048) * math.sqrt(1.0 / 2048)).float()
    d.sd["fc.bias"] = (0.1 * d.randn(1000)).float()
    return d.state()


def retinaface_r50_state(seed=0, head_gain=0.5):
    """Seeded synthetic RetinaFace-R50 weights (retinaface/retina_r50.cpp:100-212 key names).  The last BatchNorm of every residual branch has a
    small gamma so that activations stay O(1-10) through 16 bottlenecks (fp16 storage, the exp() of the decode)."""
    d = _Draw(seed)
    _resnet50_body(d, "body.", 0.25)

    def cbr(name, cout, cin, k):
        d.conv_w(name + ".0.weight", cout, cin, k)
        d.bn(name + ".1", cout)
    cbr("fpn.output1", 256, 512, 1)
    cbr("fpn.output2", 256, 1024, 1)
    cbr("fpn.output3", 256, 2048, 1)
    cbr("fpn.merge2", 256, 256, 3)
    cbr("fpn.merge1", 256, 256, 3)
    for l in ("ssh1", "ssh2", "ssh3"):
        cbr(l + ".conv3X3", 128, 256, 3)
        cbr(l + ".conv5X5_1", 64, 256, 3)
        cbr(l + ".conv5X5_2", 64, 64, 3)
        cbr(l + ".conv7X7_2", 64, 64, 3)
        cbr(l + ".conv7x7_3", 64, 64, 3)
    for l in range(3):
        for name, ch in (("BboxHead", 8), ("ClassHead", 4), ("LandmarkHead", 20)):
            d.conv_w(f"{name}.{l}.conv1x1.weight", ch, 256, 1, gain=head_gain)
            d.sd[f"{name}.{l}.conv1x1.bias"] = (0.1 * d.randn(ch)).float()
    return d.state()


def rcnn_r50c4_state(seed=0, num_classes=80, anchors=15):
    """Seeded synthetic Faster / Mask R-CNN R50-C4 weights (detectron2 export after fuse-bn, the keys of rcnn/rcnn.cpp:79-278 and
    rcnn/backbone.hpp:26-229): every conv has a bias; small gains on the residual branches and the stem bring the (x - mean) input to O(1)."""
    import math
    d = _Draw(seed)

    def conv(name, cout, cin, k, gain=2.0):
        d.conv_w(name + ".weight", cout, cin, k, gain=gain)
        d.sd[name + ".bias"] = (0.05 * d.randn(cout)).float()

    def stage(n, inch, mid, outch, l):
        for i in range(n):
            b = f"{l}.{i}"
            conv(b + ".conv1", mid, inch, 1)
            conv(b + ".conv2", mid, mid, 3)
            conv(b + ".conv3", outch, mid, 1, gain=0.125)
            if inch != outch:
                conv(b + ".shortcut", outch, inch, 1, gain=1.0)
            inch = outch

    conv("backbone.stem.conv1", 64, 3, 7, gain=2.0 / 70.0 ** 2)
    inch, mid, outch = 64, 64, 256
    for s_, n in enumerate((3, 4, 6)):
        stage(n, inch, mid, outch, f"backbone.res{s_ + 2}")
        inch, mid, outch = outch, mid * 2, outch * 2
    conv("proposal_generator.rpn_head.conv", 1024, 1024, 3)
    conv("proposal_generator.rpn_head.objectness_logits", anchors, 1024, 1, gain=8.0)
    conv("proposal_generator.rpn_head.anchor_deltas", 4 * anchors, 1024, 1, gain=0.05)
    stage(3, 1024, 512, 2048, "roi_heads.res5")
    nc = num_classes
    d.sd["roi_heads.box_predictor.cls_score.weight"] = (d.randn(nc + 1, 2048) * 0.06).float()
    d.sd["roi_heads.box_predictor.cls_score.bias"] = (0.1 * d.randn(nc + 1)).float()
    d.sd["roi_heads.box_predictor.bbox_pred.weight"] = (d.randn(4 * nc, 2048) * 0.01).float()
    d.sd["roi_heads.box_predictor.bbox_pred.bias"] = (0.01 * d.randn(4 * nc)).float()
    stage(3, 1024, 512, 2048, "roi_heads.res5")   # the mask branch runs res5 again: second draw, first position (see _Draw)
    d.sd["roi_heads.mask_head.deconv.weight"] = (d.randn(2048, 256, 2, 2) * math.sqrt(2.0 / 2048)).float()
    d.sd["roi_heads.mask_head.deconv.bias"] = (0.05 * d.randn(256)).float()
    conv("roi_heads.mask_head.predictor", nc, 256, 1, gain=4.0)
    return d.state()


STATE = {"resnet50": resnet50_state, "retinaface_r50": retinaface_r50_state, "rcnn_r50c4": rcnn_r50c4_state}   # (yolov8n_state is added below its definition)


YOLOV5_ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]  # yolov5s P3/P4/P5 (ultralytics yaml)


def yolov5_head_tensors(batch, classes=80, net_h=640, net_w=640, strides=(8, 16, 32), objects=(40, 160), seed=0, seg=False):
    """Planted-object inputs of the anchor-based YoloLayer: list of [B, 3*(5+classes(+32)), gh*gw] fp32 (channel-major, as the
    detect convolutions emit them, yolov5/src/model.cpp:331-343).  Objectness logits ~ N(-6, 1.5^2) with `objects` planted
    anchors per image (obj +2..+6, one class +3..+7, small clusters of neighbouring cells so that NMS has work)."""
    rng = np.random.default_rng(seed)
    info = 5 + classes + (32 if seg else 0)
    outs = []
    for s in strides:
        gh, gw = net_h // s, net_w // s
        x = rng.normal(0.0, 1.0, size=(batch, 3, info, gh * gw)).astype(np.float32)
        x[:, :, 4] = rng.normal(-6.0, 1.5, size=(batch, 3, gh * gw))
        x[:, :, 5:5 + classes] = rng.normal(-4.0, 1.5, size=(batch, 3, classes, gh * gw))
        outs.append(x)
    for b in range(batch):
        for _ in range(int(rng.integers(*objects))):
            l = int(rng.integers(0, len(strides)))
            gh, gw = net_h // strides[l], net_w // strides[l]
            cy, cx, k, c = int(rng.integers(0, gh)), int(rng.integers(0, gw)), int(rng.integers(0, 3)), int(rng.integers(0, classes))
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                if rng.uniform() < 0.35 and (dy, dx) != (0, 0):
                    continue
                e = min(cy + dy, gh - 1) * gw + min(cx + dx, gw - 1)
                outs[l][b, k, 4, e] = rng.uniform(2.0, 6.0)
                outs[l][b, k, 5 + c, e] = rng.uniform(3.0, 7.0)
                outs[l][b, k, 0:4, e] = rng.normal(0, 0.4, size=4)
    return [x.reshape(batch, 3 * info, -1) for x in outs]


YOLOV5_P6_ANCHORS = [[19, 27, 44, 40, 38, 94], [96, 68, 86, 152, 180, 137], [140, 301, 303, 264, 238, 542],
                     [436, 615, 739, 380, 925, 792]]  # yolov5s6 P3 .. P6 (ultralytics yaml)
YOLOV5_SCALES = {"n": (0.33, 0.25), "s": (0.33, 0.50), "m": (0.67, 0.75), "l": (1.0, 1.0), "x": (1.33, 1.25)}   # yolov5_det.cpp:22-41: gd, gw
YOLOV5_OBJ_SCALE, YOLOV5_OBJ_BIAS = 24.0, -5.0   # objectness rows of the detect convolutions: He rows times the scale, around the bias
YOLOV5_CLS_BIAS, YOLOV5_CLS_MARGIN = -2.0, 2.5   # class rows: every class around the bias, one favoured class per (level, anchor) above it by the margin


YOLOV5_COEF_SCALE = 4.0     # seg: the 32 mask-coefficient rows per anchor are He rows (gain 2) times this
YOLOV5_PROTO_SCALE = 8.0    # seg: the rows of Proto's last convolution (model.24.proto.cv3) are He rows (gain 2) times this


def yolov5_state(scale="n", seed=0, num_class=80, p6=False, task=0):
    """Seeded synthetic weights of YOLOv5{n,s,m,l,x} (v6 graph; p6: the n6 ... x6 models) under the reference's `.wts` key names
    (ultralytics state_dict keys as gen_wts.py writes them, read by yolov5/src/model.cpp:99-476): OrderedDict name -> fp32 array,
    including <detect>.anchor_grid (P5: YOLOV5_ANCHORS) and <detect>.strides.  He-scaled convolutions with near-identity BatchNorm
    statistics (the yolov8n_state recipe).  The detect convolutions are He rows (gain 2) with biases 0.1 N(0, 1), except:
      * the three objectness rows are scaled by YOLOV5_OBJ_SCALE around a bias of YOLOV5_OBJ_BIAS.  The features these random backbones
        produce vary little over an image (a He row gives logits with a spread of 0.1 - 0.5), so it takes that scale for a useful share
        of the anchors to pass the plugin's 0.1 gate (logit > -2.197): 2 - 55 % of them, by model and size (the counts measured with
        the fp32 twin are in tests/test_gpu_yolov5.py);
      * the class rows sit around YOLOV5_CLS_BIAS and, per (level, anchor), one favoured class (7 level + 29 anchor + 3 mod the class
        count) lies YOLOV5_CLS_MARGIN above.  The gate of this plugin is on objectness alone, so unlike YOLOv8's the class argmax of EVERY
        passing anchor is compared between engines; eighty near-equal logits would flip it under fp16 rounding in 1 - 2 % of them (the
        top-two gap of 80 equal-variance logits is below twice the rounding error that often, at any gain), above the 0.5 % the fp16
        allowance has for all causes together.

    task: 0 det, 1 seg, 4 cls (P5 only).  With task = 0 the dict is what it was before the keyword existed, tensor for tensor and in
    draw order.  The task tensors are drawn after every tensor the det model shares with them:
      * seg (yolov5/src/model.cpp:539-628): the detect rows are drawn with 5 + classes + 32 values per anchor, objectness and class rows
        by the recipe above.  The 32 coefficient rows per anchor are He rows times YOLOV5_COEF_SCALE, and Proto (model.24.proto.cv1 /
        cv2 / cv3, drawn last) ends in a convolution of He rows times YOLOV5_PROTO_SCALE.  Plain He rows give mask logits
        e = sum_j coef_j * proto_j that are flat (std 0.13 on yolov5n, 0.014 on yolov5s: sigmoid within 0.41 - 0.59), for the reason the
        objectness rows are scaled; much larger scales saturate them (4 x 16: 43 % of yolov5n's logits beyond +-8).  Measured with the
        fp64 twin (weight seed 0 unless stated) on synth.images(2, S, S, seed=12), over the candidates that pass the 0.1 gate and every pixel of the plane:
        yolov5n, 160^2 (507 candidates): e mean 0.02, std 3.8, max |e| 10.9, 0.2 % beyond +-8; yolov5s, 128^2, at weight seed 1 (689
        candidates; seed 0 passes a single anchor at that size, over which the spread is 0.43): mean -1.7, std 0.94, max |e| 7.7
        (sigmoid 0.0005 - 0.94); seeds 2 - 8 of yolov5s: std 0.46 - 2.9, max |e| 2.4 - 13.2, at most 0.7 % beyond +-8
      * cls (model.cpp:479-537): the backbone to model.8 as det, then model.9.conv (to 1280 channels) and model.9.linear
        (N(0, 1 / 1280) rows, biases 0.1 N(0, 1)); num_class is the classifier's class count (kClsNumClass is 1000).
    """
    import math
    from collections import OrderedDict

    import torch
    gd, gw = YOLOV5_SCALES[scale]
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    randn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    rand = lambda *shape: torch.rand(*shape, generator=g)    # noqa: E731

    def W(x):
        return int(math.ceil(x * gw / 8)) * 8

    def D(x):
        return 1 if x == 1 else max(int(round(x * gd)), 1)   # Python's round: half to even, as get_depth

    def cb(name, cout, cin, k):  # Conv + BatchNorm (+ SiLU)
        sd[name + ".conv.weight"] = (randn(cout, cin, k, k) * math.sqrt(2.0 / (cin * k * k))).float()
        sd[name + ".bn.weight"] = (0.9 + 0.2 * rand(cout)).float()
        sd[name + ".bn.bias"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_mean"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_var"] = (0.8 + 0.4 * rand(cout)).float()
        sd[name + ".bn.num_batches_tracked"] = torch.zeros(1)

    def c3(name, c1, c2, n):
        c_ = int(c2 * 0.5)
        cb(name + ".cv1", c_, c1, 1)
        cb(name + ".cv2", c_, c1, 1)
        cb(name + ".cv3", c2, 2 * c_, 1)
        for i in range(n):
            cb(f"{name}.m.{i}.cv1", c_, c_, 1)
            cb(f"{name}.m.{i}.cv2", c_, c_, 3)

    def sppf(name, c1, c2):
        cb(name + ".cv1", c1 // 2, c1, 1)
        cb(name + ".cv2", c2, 2 * c1, 1)

    cb("model.0", W(64), 3, 6)
    cb("model.1", W(128), W(64), 3)
    c3("model.2", W(128), W(128), D(3))
    cb("model.3", W(256), W(128), 3)
    c3("model.4", W(256), W(256), D(6))
    cb("model.5", W(512), W(256), 3)
    c3("model.6", W(512), W(512), D(9))
    assert task in (0, 1, 4) and not (task and p6), "yolov5 tasks: 0 det, 1 seg, 4 cls; P6 is det only"
    if task == 4:
        cb("model.7", W(1024), W(512), 3)
        c3("model.8", W(1024), W(1024), D(3))
        cb("model.9.conv", 1280, W(1024), 1)   # Classify.conv is a Conv module: model.9.conv.conv.weight, model.9.conv.bn.*
        sd["model.9.linear.weight"] = (randn(num_class, 1280) * math.sqrt(1.0 / 1280)).float()
        sd["model.9.linear.bias"] = (0.1 * randn(num_class)).float()
        return OrderedDict((k, v.numpy()) for k, v in sd.items())
    if not p6:
        cb("model.7", W(1024), W(512), 3)
        c3("model.8", W(1024), W(1024), D(3))
        sppf("model.9", W(1024), W(1024))
        cb("model.10", W(512), W(1024), 1)
        c3("model.13", W(1024), W(512), D(3))
        cb("model.14", W(256), W(512), 1)
        c3("model.17", W(512), W(256), D(3))
        cb("model.18", W(256), W(256), 3)
        c3("model.20", W(512), W(512), D(3))
        cb("model.21", W(512), W(512), 3)
        c3("model.23", W(1024), W(1024), D(3))
        det, feats, anchors, strides = "model.24", (W(256), W(512), W(1024)), YOLOV5_ANCHORS, (8, 16, 32)
    else:
        cb("model.7", W(768), W(512), 3)
        c3("model.8", W(768), W(768), D(3))
        cb("model.9", W(1024), W(768), 3)
        c3("model.10", W(1024), W(1024), D(3))
        sppf("model.11", W(1024), W(1024))
        cb("model.12", W(768), W(1024), 1)
        c3("model.15", W(1536), W(768), D(3))
        cb("model.16", W(512), W(768), 1)
        c3("model.19", W(1024), W(512), D(3))
        cb("model.20", W(256), W(512), 1)
        c3("model.23", W(512), W(256), D(3))
        cb("model.24", W(256), W(256), 3)
        c3("model.26", W(512), W(512), D(3))
        cb("model.27", W(512), W(512), 3)
        c3("model.29", W(1024), W(768), D(3))
        cb("model.30", W(768), W(768), 3)
        c3("model.32", W(1536), W(1024), D(3))
        det, feats, anchors, strides = "model.33", (W(256), W(512), W(768), W(1024)), YOLOV5_P6_ANCHORS, (8, 16, 32, 64)
    info = 5 + num_class + (32 if task == 1 else 0)
    for lv, cin in enumerate(feats):
        w = randn(3 * info, cin, 1, 1) * math.sqrt(2.0 / cin)
        b = 0.1 * randn(3 * info)
        for k in range(3):
            w[k * info + 4] *= YOLOV5_OBJ_SCALE
            b[k * info + 4] += YOLOV5_OBJ_BIAS
            b[k * info + 5:k * info + 5 + num_class] += YOLOV5_CLS_BIAS
            b[k * info + 5 + (7 * lv + 29 * k + 3) % num_class] += YOLOV5_CLS_MARGIN
            if task == 1:
                w[k * info + 5 + num_class:(k + 1) * info] *= YOLOV5_COEF_SCALE
        sd[f"{det}.m.{lv}.weight"] = w.float()
        sd[f"{det}.m.{lv}.bias"] = b.float()
    sd[det + ".anchor_grid"] = torch.tensor(anchors, dtype=torch.float32).reshape(len(feats), 1, 3, 1, 1, 2)
    sd[det + ".strides"] = torch.tensor(strides, dtype=torch.float32)
    if task == 1:   # Proto (model.cpp:219-232): 3x3, nearest x2, 3x3, 1x1 to 32
        cb(det + ".proto.cv1", W(256), W(256), 3)
        cb(det + ".proto.cv2", W(256), W(256), 3)
        cb(det + ".proto.cv3", 32, W(256), 1)
        sd[det + ".proto.cv3.conv.weight"] *= YOLOV5_PROTO_SCALE
    return OrderedDict((k, v.numpy()) for k, v in sd.items())


STATE["yolov8n"] = yolov8n_state


# The arguments of the reference's builders (yolov9/src/model.cpp:35-109 t, 188-254 s, 334-435 m, 568-645 c, 1171-1248 gelan-c), in the
# order of the main branch.  "L<k>" is the layer whose weights are model.<k + first>.  rep = (c2, c3, c4, n) of RepNCSPELAN4.
YOLOV10_MODELS = ("yolov10n", "yolov10s", "yolov10m", "yolov10b", "yolov10l", "yolov10x")
YOLOV10_SCALES = {  # yolov10_det.cpp:111-141: gd, gw, max_channels
    "n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 768), "b": (0.67, 1.00, 512), "l": (1.00, 1.00, 512), "x": (1.00, 1.25, 512)}
# which of the stages 6, 8, 13, 19, 22 are C2F ("f"), C2fCIB ("c") or C2fCIB with the large kernel ("l": RepVGGDW): yolov10/src/model.cpp, the
# five buildEngineYolov10Det* functions (b and l share one)
YOLOV10_STAGES = {"n": "ffffl", "s": "flffl", "m": "fcfcc", "b": "fcccc", "l": "fcccc", "x": "ccccc"}
# The class head (the yolo11_state recipe: He rows of gain 800) around a bias, with one favoured class per level lifted by the margin.
# These random backbones give features that vary little over an image: with a zero bias the largest logit of a cell lies within +- 0.5 of
# 6.0 (yolov10n; 6.4 for yolov10m), so the bias puts the plugin's 0.1 gate (logit -2.197) inside that narrow band and a useful share of a
# small image's cells, far from all of them, passes it.  Set with the fp64 twin for yolov10n and yolov10m at 80 classes (counts:
# tests/test_gpu_yolov10.py); the other four models take yolov10n's bias untuned.
YOLOV10_CLS_BIAS, YOLOV10_CLS_MARGIN = -8.25, 0.5
YOLOV10_CLS_BIAS_OF = {"yolov10m": -8.7}


def yolov10_state(name="yolov10n", seed=0, num_class=80):
    """Seeded synthetic weights of yolov10n / s / m / b / l / x under the reference's `.wts` key names (the ultralytics state_dict keys that
    yolov10/src/block.cpp / model.cpp read; the one-to-many head the reference never builds is absent): OrderedDict name -> fp32 array.
    He-scaled convolutions with near-identity BatchNorm statistics (the yolo11_state recipe); the class head as described at YOLOV10_CLS_BIAS."""
    import math
    from collections import OrderedDict

    import torch
    assert name in YOLOV10_MODELS, name
    letter = name[7]
    gd, gw, mc = YOLOV10_SCALES[letter]
    stages = YOLOV10_STAGES[letter]
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    randn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    rand = lambda *shape: torch.rand(*shape, generator=g)    # noqa: E731

    def W(x):
        return int(math.ceil(min(x, mc) * gw / 8)) * 8

    def D(x):
        if x == 1:
            return 1
        v = x * gd          # get_depth: round half away from zero, one less on an exact half with an even integer part
        r = int(math.floor(v + 0.5))
        if v - int(v) == 0.5 and int(v) % 2 == 0:
            r -= 1
        return max(r, 1)

    def conv(name, cout, cin, k, gain=2.0):
        sd[name + ".weight"] = (randn(cout, cin, k, k) * math.sqrt(gain / (cin * k * k))).float()

    def cb(name, cout, cin, k, groups=1, gain=2.0):  # Conv + BatchNorm (+ SiLU)
        conv(name + ".conv", cout, cin // groups, k, gain)
        sd[name + ".bn.weight"] = (0.9 + 0.2 * rand(cout)).float()
        sd[name + ".bn.bias"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_mean"] = (0.1 * randn(cout)).float()
        sd[name + ".bn.running_var"] = (0.8 + 0.4 * rand(cout)).float()
        sd[name + ".bn.num_batches_tracked"] = torch.zeros(1)

    def c2f(name, c1, c2, n):
        c_ = int(c2 * 0.5)
        cb(name + ".cv1", 2 * c_, c1, 1)
        for i in range(n):
            cb(f"{name}.m.{i}.cv1", c_, c_, 3)
            cb(f"{name}.m.{i}.cv2", c_, c_, 3)
        cb(name + ".cv2", c2, (2 + n) * c_, 1)

    def cib(name, c, lk):   # CIB with c1 == c2 == c and e = 1.0: 2 c_ = 2 c in the middle
        cb(name + ".cv1.0", c, c, 3, groups=c, gain=1.0)
        cb(name + ".cv1.1", 2 * c, c, 1)
        if lk:
            cb(name + ".cv1.2.conv", 2 * c, 2 * c, 7, groups=2 * c, gain=1.0)
            cb(name + ".cv1.2.conv1", 2 * c, 2 * c, 3, groups=2 * c, gain=1.0)
        else:
            cb(name + ".cv1.2", 2 * c, 2 * c, 3, groups=2 * c, gain=1.0)
        cb(name + ".cv1.3", c, 2 * c, 1)
        cb(name + ".cv1.4", c, c, 3, groups=c, gain=1.0)

    def c2fcib(name, c1, c2, n, lk):
        c_ = int(c2 * 0.5)
        cb(name + ".cv1", 2 * c_, c1, 1)
        for i in range(n):
            cib(f"{name}.m.{i}", c_, lk)
        cb(name + ".cv2", c2, (2 + n) * c_, 1)

    def stage(kind, name, c1, c2, n):
        if kind == "f":
            c2f(name, c1, c2, n)
        else:
            c2fcib(name, c1, c2, n, kind == "l")

    def scdown(name, c1, c2):
        cb(name + ".cv1", c2, c1, 1)
        cb(name + ".cv2", c2, c2, 3, groups=c2, gain=1.0)

    def psa(name, ch):
        c = int(ch * 0.5)
        cb(name + ".cv1", 2 * c, ch, 1)
        heads = c // 64
        kd = (c // heads) // 2
        cb(name + ".attn.qkv", c + 2 * kd * heads, c, 1)
        cb(name + ".attn.pe", c, c, 3, groups=c, gain=1.0)
        cb(name + ".attn.proj", c, c, 1, gain=1.0)
        cb(name + ".ffn.0", 2 * c, c, 1)
        cb(name + ".ffn.1", c, 2 * c, 1, gain=1.0)
        cb(name + ".cv2", ch, 2 * c, 1)

    cb("model.0", W(64), 3, 3)
    cb("model.1", W(128), W(64), 3)
    c2f("model.2", W(128), W(128), D(3))
    cb("model.3", W(256), W(128), 3)
    c2f("model.4", W(256), W(256), D(6))
    scdown("model.5", W(256), W(512))
    stage(stages[0], "model.6", W(512), W(512), D(6))
    scdown("model.7", W(512), W(1024))
    stage(stages[1], "model.8", W(1024), W(1024), D(3))
    cb("model.9.cv1", W(1024) // 2, W(1024), 1)
    cb("model.9.cv2", W(1024), 2 * W(1024), 1)
    psa("model.10", W(1024))
    stage(stages[2], "model.13", W(1024) + W(512), W(512), D(3))
    c2f("model.16", W(512) + W(256), W(256), D(3))
    cb("model.17", W(256), W(256), 3)
    stage(stages[3], "model.19", W(256) + W(512), W(512), D(3))
    scdown("model.20", W(512), W(512))
    stage(stages[4], "model.22", W(512) + W(1024), W(1024), D(3))
    c2 = max(16, W(256) // 4, 64)
    c3 = max(W(256), min(num_class, 100))
    for lv, cin in enumerate((W(256), W(512), W(1024))):
        a, b = f"model.23.one2one_cv2.{lv}", f"model.23.one2one_cv3.{lv}"
        cb(a + ".0", c2, cin, 3)
        cb(a + ".1", c2, c2, 3)
        conv(a + ".2", 64, c2, 1, gain=4.0)
        sd[a + ".2.bias"] = (1.0 + 0.1 * randn(64)).float()
        cb(b + ".0.0", cin, cin, 3, groups=cin, gain=1.0)
        cb(b + ".0.1", c3, cin, 1)
        cb(b + ".1.0", c3, c3, 3, groups=c3, gain=1.0)
        cb(b + ".1.1", c3, c3, 1)
        conv(b + ".2", num_class, c3, 1, gain=800.0)
        bias = YOLOV10_CLS_BIAS_OF.get(name, YOLOV10_CLS_BIAS) + 0.1 * randn(num_class)
        bias[(7 * lv + 3) % num_class] += YOLOV10_CLS_MARGIN
        sd[b + ".2.bias"] = bias.float()
        if lv == 0:
            sd["model.23.dfl.conv.weight"] = torch.arange(16.0).reshape(1, 16, 1, 1)
    return OrderedDict((k, v.numpy()) for k, v in sd.items())


YOLOV9_SPECS = {
    "yolov9t": dict(stem=(16, 32), elan1=True, b2=(32, 32, 16, 0), adown=False, down=(64, 96, 128), rep=((64, 64, 32, 3), (96, 96, 48, 3), (128, 128, 64, 3)),
                    spp=(128, 64), r12=(96, 96, 48, 3), r15=(64, 64, 32, 3), d16=48, r18=(96, 96, 48, 3), d19=64, r21=(128, 128, 64, 3), aux=False),
    "yolov9s": dict(stem=(32, 64), elan1=True, b2=(64, 64, 32, 0), adown=False, down=(128, 192, 256), rep=((128, 128, 64, 3), (192, 192, 96, 3), (256, 256, 128, 3)),
                    spp=(256, 128), r12=(192, 192, 96, 3), r15=(128, 128, 64, 3), d16=96, r18=(192, 192, 96, 3), d19=128, r21=(256, 256, 128, 1), aux=False),
    "yolov9m": dict(stem=(32, 64), elan1=False, b2=(128, 128, 64, 1), adown=False, down=(240, 360, 480), rep=((240, 240, 120, 1), (360, 360, 180, 1), (480, 480, 240, 1)),
                    spp=(480, 240), r12=(360, 360, 180, 1), r15=(240, 240, 120, 1), d16=184, r18=(360, 360, 180, 1), d19=240, r21=(480, 480, 240, 1), aux=True),
    "yolov9c": dict(stem=(64, 128), elan1=False, b2=(256, 128, 64, 1), adown=True, down=(256, 512, 512), rep=((512, 256, 128, 1), (512, 512, 256, 1), (512, 512, 256, 1)),
                    spp=(512, 256), r12=(512, 512, 256, 1), r15=(256, 256, 128, 1), d16=256, r18=(512, 512, 256, 1), d19=512, r21=(512, 512, 256, 1), aux=True),
}
YOLOV9_SPECS["gelanc"] = dict(YOLOV9_SPECS["yolov9c"], aux=False)
YOLOV9_CLS_GAIN = 800.0   # He gain of the class rows (yolo11_state's): these random backbones give features that vary little over an image
YOLOV9_CLS_BIAS = -9.5    # ... around this bias 4 - 36 % of the cells pass the plugin's 0.1 gate (counts: tests/test_gpu_yolov9.py)
YOLOV9_CLS_BIAS_OF = {"gelanc": -11.5}   # ... but for gelan-c, whose largest logit per cell lies two units higher: -9.5 passes 70 % of its cells, -11.5 4 - 15 %


def yolov9_state(name="yolov9t", seed=0, num_class=80, converted=False):
    """Seeded synthetic weights of yolov9t / yolov9s / yolov9m / yolov9c / gelanc under the reference's `.wts` key names (the state_dict
    keys gen_wts.py writes, read by yolov9/src/block.cpp / model.cpp): OrderedDict name -> fp32 array.  Only the layers the host builder
    reads are there: the main branch and the head (model.29 DualDDetect, or model.22 DDetect when `converted`) for t / s, the backbone,
    the auxiliary branch and model.38 for unconverted m and for c, the main branch and model.22 for converted m and gelan-c.  `converted`
    is the reference's isConvert (t / s / m).  He-scaled convolutions with near-identity BatchNorm statistics (the yolo11_state recipe);
    the box rows have gain 4 around a bias of 1, the class rows YOLOV9_CLS_GAIN around YOLOV9_CLS_BIAS (YOLOV9_CLS_BIAS_OF for gelanc), so that every image keeps
    candidates well above zero and well below the cell count."""
    import math
    from collections import OrderedDict

    import torch
    sp = YOLOV9_SPECS[name]
    assert not (converted and name in ("yolov9c", "gelanc")), "converted: yolov9t / s / m only"
    aux = sp["aux"] and not converted
    first = 1 if aux else 0
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    randn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    rand = lambda *shape: torch.rand(*shape, generator=g)    # noqa: E731
    M = lambda k: f"model.{k + first}"                       # noqa: E731

    def conv(key, cout, cin, k, gain=2.0):
        sd[key + ".weight"] = (randn(cout, cin, k, k) * math.sqrt(gain / (cin * k * k))).float()

    def cb(key, cout, cin, k, groups=1, gain=2.0):  # Conv + BatchNorm (+ SiLU)
        conv(key + ".conv", cout, cin // groups, k, gain)
        sd[key + ".bn.weight"] = (0.9 + 0.2 * rand(cout)).float()
        sd[key + ".bn.bias"] = (0.1 * randn(cout)).float()
        sd[key + ".bn.running_mean"] = (0.1 * randn(cout)).float()
        sd[key + ".bn.running_var"] = (0.8 + 0.4 * rand(cout)).float()
        sd[key + ".bn.num_batches_tracked"] = torch.zeros(1)

    def repncsp(key, c1, c2, n):
        c_ = c2 // 2
        cb(key + ".cv1", c_, c1, 1)
        for i in range(n):
            cb(f"{key}.m.{i}.cv1.conv1", c_, c_, 3, gain=1.0)   # RepConvN: the two branches are summed before the SiLU
            cb(f"{key}.m.{i}.cv1.conv2", c_, c_, 1, gain=1.0)
            cb(f"{key}.m.{i}.cv2", c_, c_, 3)
        cb(key + ".cv2", c_, c1, 1)
        cb(key + ".cv3", c2, 2 * c_, 1)

    def elan1(key, c1, c2, c3, c4):
        cb(key + ".cv1", c3, c1, 1)
        cb(key + ".cv2", c4, c3 // 2, 3)
        cb(key + ".cv3", c4, c4, 3)
        cb(key + ".cv4", c2, c3 + 2 * c4, 1)

    def rep(key, c1, r):
        c2, c3, c4, n = r
        cb(key + ".cv1", c3, c1, 1)
        repncsp(key + ".cv2.0", c3 // 2, c4, n)
        cb(key + ".cv2.1", c4, c4, 3)
        repncsp(key + ".cv3.0", c4, c4, n)
        cb(key + ".cv3.1", c4, c4, 3)
        cb(key + ".cv4", c2, c3 + 2 * c4, 1)
        return c2

    def down(key, c1, c2):
        if sp["adown"]:
            cb(key + ".cv1", c2 // 2, c1 // 2, 3)
            cb(key + ".cv2", c2 // 2, c1 // 2, 1)
        else:
            cb(key + ".cv1", c2, c1, 3)
        return c2

    def block2(key, c1):
        if sp["elan1"]:
            elan1(key, c1, *sp["b2"][:3])
            return sp["b2"][0]
        return rep(key, c1, sp["b2"])

    def cblinear(key, c1, c2s):
        conv(key + ".conv", sum(c2s), c1, 1, gain=1.0)
        sd[key + ".conv.bias"] = (0.1 * randn(sum(c2s))).float()

    d3, d5, d7 = sp["down"]
    cb(M(0), sp["stem"][0], 3, 3)
    cb(M(1), sp["stem"][1], sp["stem"][0], 3)
    c = block2(M(2), sp["stem"][1])
    c4 = rep(M(4), down(M(3), c, d3), sp["rep"][0])
    c6 = rep(M(6), down(M(5), c4, d5), sp["rep"][1])
    c8 = rep(M(8), down(M(7), c6, d7), sp["rep"][2])
    if not aux:
        cb(M(9) + ".cv1", sp["spp"][1], c8, 1)
        cb(M(9) + ".cv5", sp["spp"][0], 4 * sp["spp"][1], 1)
        c9 = sp["spp"][0]
        c12 = rep(M(12), c9 + c6, sp["r12"])
        c15 = rep(M(15), c12 + c4, sp["r15"])
        c18 = rep(M(18), down(M(16), c15, sp["d16"]) + c12, sp["r18"])
        c21 = rep(M(21), down(M(19), c18, sp["d19"]) + c9, sp["r21"])
        feats = (c15, c18, c21)
        dual = sp["elan1"] and not converted
        det = "model.29" if dual else "model.22"
    else:
        cblinear(M(22), c4, [d3])
        cblinear(M(23), c6, [d3, d5])
        cblinear(M(24), c8, [d3, d5, d7])
        cb(M(25), sp["stem"][0], 3, 3)
        cb(M(26), sp["stem"][1], sp["stem"][0], 3)
        c = rep(M(27), sp["stem"][1], sp["b2"])
        a31 = rep(M(30), down(M(28), c, d3), sp["rep"][0])
        a34 = rep(M(33), down(M(31), a31, d5), sp["rep"][1])
        a37 = rep(M(36), down(M(34), a34, d7), sp["rep"][2])
        feats = (a31, a34, a37)
        dual = True
        det = M(37)
    c2 = max(feats[0] // 4, 64)
    c3 = max(feats[0], min(num_class * 2 if dual else num_class, 128))
    for lv, cin in enumerate(feats):
        cb(f"{det}.cv2.{lv}.0", c2, cin, 3)
        cb(f"{det}.cv2.{lv}.1", c2, c2, 3, groups=4)
        conv(f"{det}.cv2.{lv}.2", 64, c2 // 4, 1, gain=4.0)
        sd[f"{det}.cv2.{lv}.2.bias"] = (1.0 + 0.1 * randn(64)).float()
        cb(f"{det}.cv3.{lv}.0", c3, cin, 3)
        cb(f"{det}.cv3.{lv}.1", c3, c3, 3)
        conv(f"{det}.cv3.{lv}.2", num_class, c3, 1, gain=YOLOV9_CLS_GAIN)
        sd[f"{det}.cv3.{lv}.2.bias"] = (YOLOV9_CLS_BIAS_OF.get(name, YOLOV9_CLS_BIAS) + 0.1 * randn(num_class)).float()
    sd[det + ".dfl.conv.weight"] = torch.arange(16.0).reshape(1, 16, 1, 1)
    return OrderedDict((k, v.numpy()) for k, v in sd.items())


# YOLOv7 (tiny, v7, x, w6, e6), after the models' published deploy yamls: one row per yaml layer, "model.<row>" its weights.  The anchors are
# the yamls'; yolov7x shares yolov7's and yolov7e6 shares yolov7w6's.
YOLOV7_ANCHORS = [[12, 16, 19, 36, 40, 28], [36, 75, 76, 55, 72, 146], [142, 110, 192, 243, 459, 401]]
YOLOV7_TINY_ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
YOLOV7_P6_ANCHORS = [[19, 27, 44, 40, 38, 94], [96, 68, 86, 152, 180, 137], [140, 301, 303, 264, 238, 542], [436, 615, 739, 380, 925, 792]]
YOLOV7_MODELS = ("yolov7tiny", "yolov7", "yolov7x", "yolov7w6", "yolov7e6")
YOLOV7_OBJ_SCALE = 24.0   # objectness rows of the detect convolutions (the yolov5_state recipe): He rows times the scale, around a bias
# ... but the SiLU models' random backbones give features that vary little over an image and from image to image (the objectness logits of
# a model spread by 2 - 3 around an offset of the same size that depends on the draw), so the bias that lets between 2 and 20 % of the anchors pass
# the 0.1 gate is set per model, from the logits measured with the fp64 twin for 80 classes (counts: tests/test_gpu_yolov7.py); another class
# count draws other detect rows, and nothing is promised for it
YOLOV7_OBJ_BIAS_OF = {"yolov7tiny": -24.0, "yolov7": -1.7, "yolov7x": -5.7, "yolov7w6": -8.3, "yolov7e6": -3.7}
YOLOV7_CLS_BIAS, YOLOV7_CLS_MARGIN = -2.0, 2.5
# yolov7-tiny's LeakyReLU backbone keeps its features' spread (class logits of std 1 over 80 classes: the largest of 79 reaches the favoured
# class's margin, and a fifth of the candidates had their two best classes within 0.1 - fp16 rounding flips those): its class rows are scaled down
YOLOV7_TINY_CLS_ROW_SCALE = 0.1
# ... and so are its box rows: box logits of std 1.2 carry an absolute fp16 error that moved a box's IoU against the fp32 engine to 0.936
YOLOV7_TINY_BOX_ROW_SCALE = 0.1


def yolov7_rows(name):
    """The yaml of a YOLOv7 model as rows (from, module, args): `from` an int or a list (negative: relative), module one of "Conv" (args
    c2, k, s), "MP", "SP" (k), "Concat", "Upsample", "ReOrg", "DownC" (c2), "SPPCSPC" (c2), "RepConv" (c2) and, last, "Detect"."""
    rows = []

    def conv(f, c, k=1, s=1):
        rows.append((f, "Conv", (c, k, s)))
        return len(rows) - 1

    def cat(f):
        rows.append((list(f), "Concat", ()))

    def elan(c1, c3, n, picks, out):   # two 1x1 of one input, n 3x3 behind the second, `picks` joined, 1x1
        conv(-1, c1)
        conv(-2, c1)
        for _ in range(n):
            conv(-1, c3, 3)
        cat(picks)
        return conv(-1, out)

    def mpdown(c, extra=None):   # [MP, 1x1] beside [1x1, 3x3 stride 2]
        rows.append((-1, "MP", ()))
        conv(-1, c)
        conv(-3, c)
        conv(-1, c, 3, 2)
        cat([-1, -3] + ([extra] if extra is not None else []))

    def downc(c2, extra=None):
        rows.append((-1, "DownC", (c2,)))
        if extra is not None:
            cat([-1, extra])

    def upjoin(c, lateral):
        conv(-1, c)
        rows.append((-1, "Upsample", ()))
        conv(lateral, c)
        cat([-1, -2])

    if name == "yolov7tiny":
        p4 = [-1, -2, -3, -4]
        conv(-1, 32, 3, 2)
        conv(-1, 64, 3, 2)
        elan(32, 32, 2, p4, 64)
        rows.append((-1, "MP", ()))
        b3 = elan(64, 64, 2, p4, 128)
        rows.append((-1, "MP", ()))
        b4 = elan(128, 128, 2, p4, 256)
        rows.append((-1, "MP", ()))
        elan(256, 256, 2, p4, 512)
        conv(-1, 256)
        conv(-2, 256)
        rows.extend([(-1, "SP", (5,)), (-2, "SP", (9,)), (-3, "SP", (13,))])
        cat(p4)
        conv(-1, 256)
        cat([-1, -7])
        b5 = conv(-1, 256)
        upjoin(128, b4)
        n4 = elan(64, 64, 2, p4, 128)
        upjoin(64, b3)
        n3 = elan(32, 32, 2, p4, 64)
        conv(-1, 128, 3, 2)
        cat([-1, n4])
        m4 = elan(64, 64, 2, p4, 128)
        conv(-1, 256, 3, 2)
        cat([-1, b5])
        m5 = elan(128, 128, 2, p4, 256)
        feats = [conv(n3, 128, 3), conv(m4, 256, 3), conv(m5, 512, 3)]
    elif name in ("yolov7", "yolov7x"):
        x = name == "yolov7x"
        w = (lambda c: c * 5 // 4) if x else (lambda c: c)   # the x model's transition widths are 1.25 times v7's; its ELAN widths are not
        n = 6 if x else 4
        back = [-1, -3, -5, -7, -8] if x else [-1, -3, -5, -6]
        head = back if x else [-1, -2, -3, -4, -5, -6]
        h3 = (lambda c: c) if x else (lambda c: c // 2)      # v7's head ELANs halve the 3x3 width
        conv(-1, w(32), 3, 1)
        conv(-1, w(64), 3, 2)
        conv(-1, w(64), 3, 1)
        conv(-1, w(128), 3, 2)
        elan(64, 64, n, back, w(256))
        mpdown(w(128))
        b3 = elan(128, 128, n, back, w(512))
        mpdown(w(256))
        b4 = elan(256, 256, n, back, w(1024))
        mpdown(w(512))
        elan(256, 256, n, back, w(1024))
        rows.append((-1, "SPPCSPC", (w(512),)))
        b5 = len(rows) - 1
        upjoin(w(256), b4)
        n4 = elan(256, h3(256), n, head, w(256))
        upjoin(w(128), b3)
        n3 = elan(128, h3(128), n, head, w(128))
        mpdown(w(128), n4)
        m4 = elan(256, h3(256), n, head, w(256))
        mpdown(w(256), b5)
        m5 = elan(512, h3(512), n, head, w(512))
        feats = []
        for f, c in ((n3, 256), (m4, 512), (m5, 1024)):
            rows.append((f, "Conv", (w(c), 3, 1)) if x else (f, "RepConv", (c,)))
            feats.append(len(rows) - 1)
    else:
        e6 = name == "yolov7e6"
        assert e6 or name == "yolov7w6", name
        w = (lambda c: c * 5 // 4) if e6 else (lambda c: c)
        n = 6 if e6 else 4
        back = [-1, -3, -5, -7, -8] if e6 else [-1, -3, -5, -6]
        head = list(range(-1, -n - 3, -1))

        def down(c, extra=None):   # w6: 3x3 stride 2; e6: DownC
            if e6:
                downc(w(c), extra)
            else:
                conv(-1, c, 3, 2)
                if extra is not None:
                    cat([-1, extra])

        rows.append((-1, "ReOrg", ()))
        conv(-1, w(64), 3, 1)
        down(128)
        elan(64, 64, n, back, w(128))
        down(256)
        b3 = elan(128, 128, n, back, w(256))
        down(512)
        b4 = elan(256, 256, n, back, w(512))
        down(768)
        b5 = elan(384, 384, n, back, w(768))
        down(1024)
        elan(512, 512, n, back, w(1024))
        rows.append((-1, "SPPCSPC", (w(512),)))
        b6 = len(rows) - 1
        upjoin(w(384), b5)
        n5 = elan(384, 192, n, head, w(384))
        upjoin(w(256), b4)
        n4 = elan(256, 128, n, head, w(256))
        upjoin(w(128), b3)
        n3 = elan(128, 64, n, head, w(128))
        down(256, n4)
        m4 = elan(256, 128, n, head, w(256))
        down(384, n5)
        m5 = elan(384, 192, n, head, w(384))
        down(512, b6)
        m6 = elan(512, 256, n, head, w(512))
        feats = [conv(n3, w(256), 3), conv(m4, w(512), 3), conv(m5, w(768), 3), conv(m6, w(1024), 3)]
    rows.append((feats, "Detect", ()))
    return rows


def yolov7_state(name="yolov7", seed=0, num_class=80):
    """Seeded synthetic weights of yolov7tiny / yolov7 / yolov7x / yolov7w6 / yolov7e6 under the reference's `.wts` key names (the state_dict
    keys of the deploy model, read by yolov7/src/block.cpp / model.cpp): OrderedDict name -> fp32 array.  Only what the host builder reads
    is there: Conv + BatchNorm per convolution row, the two branches of RepConv (no identity branch: its c1 != c2), the biased detect
    convolutions `m.i` and <detect>.anchor_grid - no implicit `ia` / `im` tensors, no strides.  He-scaled convolutions (gain 2 under SiLU,
    2 / (1 + 0.1^2) under LeakyReLU(0.1), 1 for each of RepConv's summed branches) with near-identity BatchNorm statistics.  The detect
    rows follow yolov5_state: objectness rows scaled by YOLOV7_OBJ_SCALE around YOLOV7_OBJ_BIAS_OF[name] so that 2 - 20 % of the anchors
    of a small image pass the plugin's 0.1 gate (7 - 9 % for the SiLU models, 10 - 19 % for yolov7tiny at 128 x 128), class rows around YOLOV7_CLS_BIAS with one favoured class per (level, anchor)."""
    import math
    from collections import OrderedDict

    import torch
    assert name in YOLOV7_MODELS, name
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    randn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    rand = lambda *shape: torch.rand(*shape, generator=g)    # noqa: E731
    gain = 2.0 / 1.01 if name == "yolov7tiny" else 2.0

    def bn(key, c):
        sd[key + ".weight"] = (0.9 + 0.2 * rand(c)).float()
        sd[key + ".bias"] = (0.1 * randn(c)).float()
        sd[key + ".running_mean"] = (0.1 * randn(c)).float()
        sd[key + ".running_var"] = (0.8 + 0.4 * rand(c)).float()
        sd[key + ".num_batches_tracked"] = torch.zeros(1)

    def cb(key, cout, cin, k):
        sd[key + ".conv.weight"] = (randn(cout, cin, k, k) * math.sqrt(gain / (cin * k * k))).float()
        bn(key + ".bn", cout)

    ch = []   # output channels per row
    rows = yolov7_rows(name)
    for i, (f, mod, args) in enumerate(rows):
        src = [(ch[j] if j >= 0 else (ch[i + j] if i + j >= 0 else 3)) for j in (f if isinstance(f, list) else [f])]
        key = f"model.{i}"
        if mod == "Conv":
            cb(key, args[0], src[0], args[1])
            ch.append(args[0])
        elif mod in ("MP", "SP", "Upsample"):
            ch.append(src[0])
        elif mod == "Concat":
            ch.append(sum(src))
        elif mod == "ReOrg":
            ch.append(4 * src[0])
        elif mod == "DownC":
            c2 = args[0]
            cb(key + ".cv1", src[0], src[0], 1)
            cb(key + ".cv2", c2 // 2, src[0], 3)
            cb(key + ".cv3", c2 // 2, src[0], 1)
            ch.append(c2)
        elif mod == "SPPCSPC":
            c_ = args[0]
            for cv, cin, k in (("cv1", src[0], 1), ("cv2", src[0], 1), ("cv3", c_, 3), ("cv4", c_, 1), ("cv5", 4 * c_, 1), ("cv6", c_, 3), ("cv7", 2 * c_, 1)):
                cb(f"{key}.{cv}", c_, cin, k)
            ch.append(c_)
        elif mod == "RepConv":
            c2 = args[0]
            sd[key + ".rbr_dense.0.weight"] = (randn(c2, src[0], 3, 3) * math.sqrt(1.0 / (src[0] * 9))).float()
            bn(key + ".rbr_dense.1", c2)
            sd[key + ".rbr_1x1.0.weight"] = (randn(c2, src[0], 1, 1) * math.sqrt(1.0 / src[0])).float()
            bn(key + ".rbr_1x1.1", c2)
            ch.append(c2)
        else:
            assert mod == "Detect" and i == len(rows) - 1
            info = 5 + num_class
            for lv, cin in enumerate(src):
                w = randn(3 * info, cin, 1, 1) * math.sqrt(2.0 / cin)
                b = 0.1 * randn(3 * info)
                for k in range(3):
                    w[k * info + 4] *= YOLOV7_OBJ_SCALE
                    b[k * info + 4] += YOLOV7_OBJ_BIAS_OF[name]
                    b[k * info + 5:(k + 1) * info] += YOLOV7_CLS_BIAS
                    b[k * info + 5 + (7 * lv + 29 * k + 3) % num_class] += YOLOV7_CLS_MARGIN
                    if name == "yolov7tiny":
                        w[k * info + 5:(k + 1) * info] *= YOLOV7_TINY_CLS_ROW_SCALE
                        w[k * info:k * info + 4] *= YOLOV7_TINY_BOX_ROW_SCALE
                sd[f"{key}.m.{lv}.weight"] = w.float()
                sd[f"{key}.m.{lv}.bias"] = b.float()
            anchors = YOLOV7_TINY_ANCHORS if name == "yolov7tiny" else (YOLOV7_P6_ANCHORS if len(src) == 4 else YOLOV7_ANCHORS)
            sd[key + ".anchor_grid"] = torch.tensor(anchors, dtype=torch.float32).reshape(len(src), 1, 3, 1, 1, 2)
    return OrderedDict((k, v.numpy()) for k, v in sd.items())


# Darknet YOLO (YOLOv3, YOLOv3-tiny, YOLOv4), after the models' published cfg files: one row per cfg module, "module_list.<row>" its weights
# (the reference's gen_wts.py writes the state_dict of a PyTorch port whose module_list follows the cfg).  The anchors are compiled into the
# reference's plugins (yololayer.h of each directory) and are no part of a weight file; they are listed in the plugin's input order.
DARKNET_MODELS = ("yolov3", "yolov3-tiny", "yolov4")
DARKNET_ANCHORS = {
    "yolov3": [[116, 90, 156, 198, 373, 326], [30, 61, 62, 45, 59, 119], [10, 13, 16, 30, 33, 23]],      # strides 32, 16, 8
    "yolov3-tiny": [[81, 82, 135, 169, 344, 319], [23, 27, 37, 58, 81, 82]],                               # strides 32, 16
    "yolov4": [[12, 16, 19, 36, 40, 28], [36, 75, 76, 55, 72, 146], [142, 110, 192, 243, 459, 401]],      # strides 8, 16, 32
}
DARKNET_STRIDES = {"yolov3": (32, 16, 8), "yolov3-tiny": (32, 16), "yolov4": (8, 16, 32)}
DARKNET_BN_EPS = {"yolov3": 1e-5, "yolov3-tiny": 1e-4, "yolov4": 1e-4}   # what each reference file passes to addBatchNorm2d
# The detect rows.  The plugin keeps an anchor whose objectness AND class maximum both reach 0.1.  Objectness rows are He rows times
# DARKNET_OBJ_SCALE around a per-model bias, set with the fp64 twin so that some, but far from all, of the 252 (tiny: 60) anchors of a 64 x 64
# image pass (counts: tests/test_gpu_darknet.py).  Class rows are scaled down around DARKNET_CLS_BIAS (sigmoid 0.047, below the gate) with one
# favoured class per (level, anchor) lifted by DARKNET_CLS_MARGIN (sigmoid 0.62, above it), so the class gate passes by a margin that fp16
# does not reach.  The width and height rows are scaled by DARKNET_WH_ROW_SCALE: the box is exp(t) * anchor, an absolute error e in t is a
# relative error e in the width, and with |t| of a few tenths fp16's head error stays far from the IoU the parity constants ask for.
DARKNET_OBJ_SCALE = 8.0
DARKNET_OBJ_BIAS_OF = {"yolov3": -13.0, "yolov3-tiny": -9.0, "yolov4": -2.7}
DARKNET_CLS_BIAS, DARKNET_CLS_MARGIN, DARKNET_CLS_ROW_SCALE = -3.0, 3.5, 0.1
DARKNET_XY_ROW_SCALE, DARKNET_WH_ROW_SCALE = 0.5, 0.1
DARKNET_BRANCH_GAIN = 0.25   # BatchNorm weight of the convolution that ends a residual branch


def darknet_rows(name):
    """The cfg of a Darknet model as rows [module, kind, channels, k, s, p, from]: kind "L" (conv + BN + LeakyReLU 0.1), "M" (conv + BN +
    Mish), "D" (biased 1x1 detect convolution), "S" (shortcut of two modules), "R" (route: one module, or the concatenation of several in the
    order given), "P" (max-pool), "Z" (zero pad right and bottom by one, then max-pool 2 stride 1), "U" (nearest upsample by 2), "Y" (yolo);
    `from` lists module numbers, empty for the module in front.  Written from the cfg files, not from the host builder's table: the two are
    compared in tests/test_darknet_cpu.py."""
    rows = []

    def add(kind, ch=0, k=0, s=0, p=0, frm=()):
        rows.append([len(rows), kind, ch, k, s, p, list(frm)])
        return len(rows) - 1

    def conv(kind, ch, k, s=1):
        return add(kind, ch, k, s, k // 2)

    def res(kind, c1, c3):   # 1x1, 3x3, shortcut over the two
        conv(kind, c1, 1)
        conv(kind, c3, 3)
        add("S", frm=(len(rows) - 1, len(rows) - 3))

    def alternate(ch, n):    # 1x1 to ch, 3x3 to 2 ch, ...
        for i in range(n):
            conv("L", 2 * ch if i % 2 else ch, 3 if i % 2 else 1)

    def head():
        add("D")
        add("Y")

    if name == "yolov3":
        conv("L", 32, 3)
        for ch, n in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
            conv("L", ch, 3, 2)
            for _ in range(n):
                res("L", ch // 2, ch)
        alternate(512, 6)
        head()
        add("R", frm=(79,))
        conv("L", 256, 1)
        add("U")
        add("R", frm=(85, 61))
        alternate(256, 6)
        head()
        add("R", frm=(91,))
        conv("L", 128, 1)
        add("U")
        add("R", frm=(97, 36))
        alternate(128, 6)
        head()
    elif name == "yolov3-tiny":
        for ch in (16, 32, 64, 128, 256):
            conv("L", ch, 3)
            add("P", 0, 2, 2, 0)
        conv("L", 512, 3)
        add("Z")
        conv("L", 1024, 3)
        conv("L", 256, 1)
        conv("L", 512, 3)
        head()
        add("R", frm=(13,))
        conv("L", 128, 1)
        add("U")
        add("R", frm=(19, 8))
        conv("L", 256, 3)
        head()
    else:
        assert name == "yolov4", name
        conv("M", 32, 3)
        for ch, n in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
            first = ch == 64
            half = ch if first else ch // 2
            d = conv("M", ch, 3, 2)
            aside = conv("M", half, 1)
            add("R", frm=(d,))
            conv("M", half, 1)
            for _ in range(n):
                res("M", ch // 2 if first else half, half)
            last = conv("M", half, 1)
            add("R", frm=(last, aside))
            conv("M", ch, 1)
        alternate(512, 3)
        add("P", 0, 5, 1, 2)
        add("R", frm=(107,))
        add("P", 0, 9, 1, 4)
        add("R", frm=(107,))
        add("P", 0, 13, 1, 6)
        add("R", frm=(112, 110, 108, 107))
        alternate(512, 3)
        conv("L", 256, 1)
        add("U")
        add("R", frm=(85,))
        conv("L", 256, 1)
        add("R", frm=(120, 118))
        alternate(256, 5)
        conv("L", 128, 1)
        add("U")
        add("R", frm=(54,))
        conv("L", 128, 1)
        add("R", frm=(130, 128))
        alternate(128, 6)
        head()
        add("R", frm=(136,))
        conv("L", 256, 3, 2)
        add("R", frm=(141, 126))
        alternate(256, 6)
        head()
        add("R", frm=(147,))
        conv("L", 512, 3, 2)
        add("R", frm=(152, 116))
        alternate(512, 6)
        head()
    return rows


def darknet_channels(rows, num_class):
    """output channels per module of darknet_rows (None for a yolo module)"""
    ch = []
    for i, kind, c, k, s, p, frm in rows:
        src = [ch[j] for j in frm] if frm else [ch[i - 1] if i else 3]
        if kind in ("L", "M"):
            ch.append(c)
        elif kind == "D":
            ch.append(3 * (5 + num_class))
        elif kind == "R":
            ch.append(sum(src))
        elif kind == "Y":
            ch.append(None)
        else:
            ch.append(src[0])
    return ch


def darknet_state(name="yolov4", seed=0, num_class=80):
    """Seeded synthetic weights of yolov3 / yolov3-tiny / yolov4 under the reference's `.wts` key names: module_list.<i>.Conv2d.weight and
    module_list.<i>.BatchNorm2d.{weight,bias,running_mean,running_var} per convolution module, module_list.<i>.Conv2d.{weight,bias} for the
    detect convolutions.  OrderedDict name -> fp32 array.  He-scaled convolutions (gain 2 / (1 + 0.1^2) under LeakyReLU(0.1), 2 under Mish)
    with near-identity BatchNorm statistics; the detect rows as described at DARKNET_OBJ_SCALE."""
    import math
    from collections import OrderedDict

    import torch
    assert name in DARKNET_MODELS, name
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    randn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    rand = lambda *shape: torch.rand(*shape, generator=g)    # noqa: E731
    rows = darknet_rows(name)
    ch = darknet_channels(rows, num_class)
    info = 5 + num_class
    lv = 0
    for i, kind, c, k, s, p, frm in rows:
        cin = ch[frm[0]] if frm else (ch[i - 1] if i else 3)
        key = f"module_list.{i}"
        if kind in ("L", "M"):
            gain = 2.0 if kind == "M" else 2.0 / 1.01
            sd[key + ".Conv2d.weight"] = (randn(c, cin, k, k) * math.sqrt(gain / (cin * k * k))).float()
            bn = key + ".BatchNorm2d"
            # a convolution that ends a residual branch: Darknet-53 has 23 shortcuts in a row and CSPDarknet as many, and branches of unit gain would
            # double the variance at each (head values of 3e4 with plain rows); a quarter of the gain keeps the trunk's scale
            branch = DARKNET_BRANCH_GAIN if i + 1 < len(rows) and rows[i + 1][1] == "S" else 1.0
            sd[bn + ".weight"] = (branch * (0.9 + 0.2 * rand(c))).float()
            sd[bn + ".bias"] = (0.1 * randn(c)).float()
            sd[bn + ".running_mean"] = (0.1 * randn(c)).float()
            sd[bn + ".running_var"] = (0.8 + 0.4 * rand(c)).float()
            sd[bn + ".num_batches_tracked"] = torch.zeros(1)
        elif kind == "D":
            w = randn(3 * info, cin, 1, 1) * math.sqrt(2.0 / cin)
            b = 0.1 * randn(3 * info)
            for a in range(3):
                o = a * info
                w[o:o + 2] *= DARKNET_XY_ROW_SCALE
                w[o + 2:o + 4] *= DARKNET_WH_ROW_SCALE
                w[o + 4] *= DARKNET_OBJ_SCALE
                b[o + 4] += DARKNET_OBJ_BIAS_OF[name]
                w[o + 5:o + info] *= DARKNET_CLS_ROW_SCALE
                b[o + 5:o + info] += DARKNET_CLS_BIAS
                b[o + 5 + (7 * lv + 29 * a + 3) % num_class] += DARKNET_CLS_MARGIN
            sd[key + ".Conv2d.weight"] = w.float()
            sd[key + ".Conv2d.bias"] = b.float()
            lv += 1
    return OrderedDict((k, v.numpy()) for k, v in sd.items())
