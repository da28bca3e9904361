"""Independent PyTorch restatement of the YOLOv5 v7 segmentation head and classifier (ultralytics modules Segment, Proto and Classify),
on top of yolov5_twin.Yolov5, evaluated in fp64 from a state dict under the ultralytics key names.
  Segment (yolov5s-seg.yaml, layer 24, reading layers 17, 20, 23): Detect with no = 5 + nc + 32 outputs per anchor, and
      Proto(c1, c_ = width(256), c2 = 32) on the first of its inputs: Conv 3x3, nn.Upsample(scale_factor=2, mode="nearest"), Conv 3x3,
      Conv 1x1.
  Classify (yolov5s-cls.yaml: the backbone to layer 8, then layer 9): Conv 1x1 to 1280, AdaptiveAvgPool2d(1), flatten, Linear.
Used by the YOLOv5 task tests to check the C++ host builder's graphs.  Not a test module (no test_ prefix)."""
import torch
import torch.nn.functional as F

from yolov5_twin import Yolov5


class Yolov5Task(Yolov5):
    def __init__(self, sd, scale="n", num_class=80):
        super().__init__(sd, scale, num_class)
        self.seen = {}

    def c3(self, x, name, n, shortcut=True):   # keeps layer 17's output, which Proto reads
        y = super().c3(x, name, n, shortcut)
        self.seen[name] = y
        return y

    def seg_heads(self, x):
        """x: [B, 3, H, W] -> the three detect convolutions' outputs [B, 3 * (5 + nc + 32), gh * gw], the strides, and the prototypes
        [B, 32, H / 4, W / 4]"""
        heads, strides = self.heads(x)
        p = self.conv(self.seen["model.17"], "model.24.proto.cv1")
        p = torch.nn.Upsample(scale_factor=2, mode="nearest")(p)
        p = self.conv(self.conv(p, "model.24.proto.cv2"), "model.24.proto.cv3")
        return heads, strides, p.float()

    def classify(self, x):
        """[B, 3, H, W] -> ([B, classes] logits, [B, 1280] pooled features)"""
        x = x.to(torch.float64)
        x = self.conv(x, "model.0", 2, 2)
        x = self.conv(x, "model.1", 2)
        x = Yolov5.c3(self, x, "model.2", 3)
        x = self.conv(x, "model.3", 2)
        x = Yolov5.c3(self, x, "model.4", 6)
        x = self.conv(x, "model.5", 2)
        x = Yolov5.c3(self, x, "model.6", 9)
        x = self.conv(x, "model.7", 2)
        x = Yolov5.c3(self, x, "model.8", 3)
        f = F.adaptive_avg_pool2d(self.conv(x, "model.9.conv"), 1).flatten(1)
        return F.linear(f, self.sd["model.9.linear.weight"], self.sd["model.9.linear.bias"]), f


__all__ = ["Yolov5Task"]
