"""Independent PyTorch restatement of the YOLO11 seg / pose / obb heads and the YOLO11 classifier (ultralytics semantics: Segment's cv4
branch and Proto, Pose's and OBB's cv4 branch, Classify), on top of yolo11_twin.Yolo11.  Used by the YOLO11 task tests to check the C++
host builder's graphs.  Not a test module (no test_ prefix)."""
import torch
import torch.nn.functional as F

from yolo11_twin import Yolo11


class Yolo11Task(Yolo11):
    def __init__(self, sd, scale="n", num_class=80, task="seg"):
        super().__init__(sd, scale, num_class)
        self.task = task
        self.feat = {}

    def c3k2(self, x, name, n, c3k, shortcut=True):   # keeps the neck outputs the task branches read
        y = super().c3k2(x, name, n, c3k, shortcut)
        self.feat[name] = y
        return y

    def task_heads(self, x):
        """x: [B, 3, H, W] -> three [B, 4 + nc + extra, g] plugin inputs, the strides, and the [B, 32, H/4, W/4] prototypes (seg) or None"""
        out, strides = self.heads(x)
        feats = [self.feat[k] for k in ("model.16", "model.19", "model.22")]
        heads = []
        for lv, f in enumerate(feats):
            s = f"model.23.cv4.{lv}"
            b = self.conv(self.conv(f, s + ".0"), s + ".1")
            b = F.conv2d(b, self.sd[s + ".2.weight"], self.sd[s + ".2.bias"])
            heads.append(torch.cat([out[lv], b.reshape(b.shape[0], b.shape[1], -1).float()], 1))
        proto = None
        if self.task == "seg":
            p = self.conv(feats[0], "model.23.proto.cv1")
            p = F.conv_transpose2d(p, self.sd["model.23.proto.upsample.weight"], self.sd["model.23.proto.upsample.bias"], stride=2)
            proto = self.conv(self.conv(p, "model.23.proto.cv2"), "model.23.proto.cv3").float()
        return heads, strides, proto

    def classify(self, x):
        """Classify on the backbone to model.8 and C2PSA as model.9: [B, 3, H, W] -> ([B, classes] logits, [B, 1280] pooled features)"""
        x = x.to(torch.float64)
        d, c3k = self.depth(2), self.c3k
        x = self.conv(x, "model.0", 2)
        x = self.conv(x, "model.1", 2)
        x = self.c3k2(x, "model.2", d, c3k)
        x = self.conv(x, "model.3", 2)
        x = self.c3k2(x, "model.4", d, c3k)
        x = self.conv(x, "model.5", 2)
        x = self.c3k2(x, "model.6", d, True)
        x = self.conv(x, "model.7", 2)
        x = self.c3k2(x, "model.8", d, True)
        x = self.c2psa(x, "model.9", d)
        f = self.conv(x, "model.10.conv").mean((2, 3))
        return F.linear(f, self.sd["model.10.linear.weight"], self.sd["model.10.linear.bias"]), f
