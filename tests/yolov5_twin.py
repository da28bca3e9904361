"""Independent PyTorch restatement of the YOLOv5 v6 detection model, P5 (yolov5{n,s,m,l,x}.yaml) and P6 (yolov5{n,s,m,l,x}6.yaml), from
the model's definition (ultralytics modules Conv, Bottleneck, C3, SPPF, Detect), evaluated in fp64 from a state dict under the
ultralytics key names.  Returns what the detect convolutions emit, the tensors the reference hands to its YoloLayer plugin.  Used by the
YOLOv5 tests to check the C++ host builder's graph.  Not a test module (no test_ prefix)."""
import torch
import torch.nn.functional as F

SCALES = {"n": (0.33, 0.25), "s": (0.33, 0.50), "m": (0.67, 0.75), "l": (1.0, 1.0), "x": (1.33, 1.25)}   # depth_multiple, width_multiple


class Yolov5:
    def __init__(self, sd, scale="n", num_class=80, p6=False):
        self.sd = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items()}
        self.gd, self.gw = SCALES[scale]
        self.nc = num_class
        self.p6 = p6

    def depth(self, n):   # parse_model: max(round(n * gd), 1) if n > 1
        return max(round(n * self.gd), 1) if n > 1 else n

    # Conv = conv2d(bias=False, padding) -> BatchNorm2d(eps=1e-3) -> SiLU; padding is k // 2 unless the yaml gives it (the stem: 6, 2, 2)
    def conv(self, x, name, s=1, p=None):
        w = self.sd[name + ".conv.weight"]
        y = F.conv2d(x, w, None, s, w.shape[-1] // 2 if p is None else p)
        gm, bt = self.sd[name + ".bn.weight"], self.sd[name + ".bn.bias"]
        mu, var = self.sd[name + ".bn.running_mean"], self.sd[name + ".bn.running_var"]
        return F.silu((y - mu[:, None, None]) / torch.sqrt(var[:, None, None] + 1e-3) * gm[:, None, None] + bt[:, None, None])

    def c3(self, x, name, n, shortcut=True):   # cv3(cat(m(cv1(x)), cv2(x))), m = n Bottlenecks (1x1, 3x3, e = 1.0)
        a = self.conv(x, name + ".cv1")
        for i in range(self.depth(n)):
            y = self.conv(self.conv(a, f"{name}.m.{i}.cv1"), f"{name}.m.{i}.cv2")
            a = a + y if shortcut else y
        return self.conv(torch.cat([a, self.conv(x, name + ".cv2")], 1), name + ".cv3")

    def sppf(self, x, name):
        y = [self.conv(x, name + ".cv1")]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], 5, 1, 2))
        return self.conv(torch.cat(y, 1), name + ".cv2")

    def heads(self, x):
        """x: [B, 3, H, W] -> the detect convolutions' outputs [B, 3 * (5 + nc), gh * gw] per level, and the strides"""
        x = x.to(torch.float64)
        H = x.shape[2]
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
        x = self.conv(x, "model.0", 2, 2)
        x = self.conv(x, "model.1", 2)
        x = self.c3(x, "model.2", 3)
        x = self.conv(x, "model.3", 2)
        x4 = x = self.c3(x, "model.4", 6)
        x = self.conv(x, "model.5", 2)
        x6 = x = self.c3(x, "model.6", 9)
        x = self.conv(x, "model.7", 2)
        if not self.p6:
            x = self.c3(x, "model.8", 3)
            x = self.sppf(x, "model.9")
            x10 = self.conv(x, "model.10")
            x = self.c3(torch.cat([up(x10), x6], 1), "model.13", 3, False)
            x14 = self.conv(x, "model.14")
            x17 = self.c3(torch.cat([up(x14), x4], 1), "model.17", 3, False)
            x20 = self.c3(torch.cat([self.conv(x17, "model.18", 2), x14], 1), "model.20", 3, False)
            x23 = self.c3(torch.cat([self.conv(x20, "model.21", 2), x10], 1), "model.23", 3, False)
            det, feats = "model.24", [x17, x20, x23]
        else:
            x8 = x = self.c3(x, "model.8", 3)
            x = self.conv(x, "model.9", 2)
            x = self.c3(x, "model.10", 3)
            x = self.sppf(x, "model.11")
            x12 = self.conv(x, "model.12")
            x = self.c3(torch.cat([up(x12), x8], 1), "model.15", 3, False)
            x16 = self.conv(x, "model.16")
            x = self.c3(torch.cat([up(x16), x6], 1), "model.19", 3, False)
            x20 = self.conv(x, "model.20")
            x23 = self.c3(torch.cat([up(x20), x4], 1), "model.23", 3, False)
            x26 = self.c3(torch.cat([self.conv(x23, "model.24", 2), x20], 1), "model.26", 3, False)
            x29 = self.c3(torch.cat([self.conv(x26, "model.27", 2), x16], 1), "model.29", 3, False)
            x32 = self.c3(torch.cat([self.conv(x29, "model.30", 2), x12], 1), "model.32", 3, False)
            det, feats = "model.33", [x23, x26, x29, x32]
        out = [F.conv2d(f, self.sd[f"{det}.m.{lv}.weight"], self.sd[f"{det}.m.{lv}.bias"]).flatten(2).float() for lv, f in enumerate(feats)]
        return out, [H // f.shape[2] for f in feats]

    def anchors(self):
        det = "model.33" if self.p6 else "model.24"
        return self.sd[det + ".anchor_grid"].reshape(-1, 6).float().numpy()


__all__ = ["SCALES", "Yolov5"]
