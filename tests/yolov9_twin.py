"""Independent PyTorch restatement of the YOLOv9 / GELAN detection graphs the host builder makes (yolov9t / s / m / c, gelanc), from the
modules' definitions (Conv, RepConvN, RepNBottleneck, RepNCSP, ELAN1, RepNCSPELAN4, AConv, ADown, SPPELAN, CBLinear, CBFuse, DFL, DDetect /
DualDDetect), evaluated in fp64 from a state dict under the reference's key names.  Every channel count and repeat count is read from
the weights; what is stated here is the wiring: which block sits where, which features the head reads and under which "model.N" its
weights are.  Returns the three (B, 4 + nc, cells) tensors the reference hands to its YoloLayer plugin.  Used by the YOLOv9 tests to
check the C++ host builder's graph.  Not a test module (no test_ prefix)."""
import torch
import torch.nn.functional as F


class Yolov9:
    def __init__(self, sd, name="yolov9t", converted=False):
        self.sd = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items()}
        self.name, self.converted = name, converted

    def bn(self, y, name):
        gm, bt = self.sd[name + ".weight"], self.sd[name + ".bias"]
        mu, var = self.sd[name + ".running_mean"], self.sd[name + ".running_var"]
        return (y - mu[:, None, None]) / torch.sqrt(var[:, None, None] + 1e-3) * gm[:, None, None] + bt[:, None, None]

    # Conv = conv2d(bias=False, padding k // 2, groups) -> BatchNorm2d(eps=1e-3) (-> SiLU)
    def conv(self, x, name, s=1, g=1, act=True):
        w = self.sd[name + ".conv.weight"]
        y = self.bn(F.conv2d(x, w, None, s, w.shape[-1] // 2, 1, g), name + ".bn")
        return F.silu(y) if act else y

    def repeats(self, name):
        n = 0
        while f"{name}.m.{n}.cv2.conv.weight" in self.sd:
            n += 1
        return n

    def repncsp(self, x, name):   # cv3(cat(m(cv1(x)), cv2(x))); m = RepNBottlenecks: x + cv2(SiLU(conv1(x) + conv2(x))), 3x3 and 1x1 branches
        a = self.conv(x, name + ".cv1")
        for i in range(self.repeats(name)):
            m = f"{name}.m.{i}"
            y = F.silu(self.conv(a, m + ".cv1.conv1", act=False) + self.conv(a, m + ".cv1.conv2", act=False))
            a = a + self.conv(y, m + ".cv2")
        return self.conv(torch.cat([a, self.conv(x, name + ".cv2")], 1), name + ".cv3")

    def elan1(self, x, name):
        y = list(self.conv(x, name + ".cv1").chunk(2, 1))
        y.append(self.conv(y[-1], name + ".cv2"))
        y.append(self.conv(y[-1], name + ".cv3"))
        return self.conv(torch.cat(y, 1), name + ".cv4")

    def elan4(self, x, name):   # RepNCSPELAN4
        y = list(self.conv(x, name + ".cv1").chunk(2, 1))
        y.append(self.conv(self.repncsp(y[-1], name + ".cv2.0"), name + ".cv2.1"))
        y.append(self.conv(self.repncsp(y[-1], name + ".cv3.0"), name + ".cv3.1"))
        return self.conv(torch.cat(y, 1), name + ".cv4")

    def down(self, x, name):   # ADown where the block has a cv2 (c / gelan-c), else AConv
        x = F.avg_pool2d(x, 2, 1, 0, False, True)
        if name + ".cv2.conv.weight" not in self.sd:
            return self.conv(x, name + ".cv1", 2)
        a, b = x.chunk(2, 1)
        return torch.cat([self.conv(a, name + ".cv1", 2), self.conv(F.max_pool2d(b, 3, 2, 1), name + ".cv2")], 1)

    def sppelan(self, x, name):
        y = [self.conv(x, name + ".cv1")]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], 5, 1, 2))
        return self.conv(torch.cat(y, 1), name + ".cv5")

    def cblinear(self, x, name, parts):
        y = F.conv2d(x, self.sd[name + ".conv.weight"], self.sd[name + ".conv.bias"])
        n = y.shape[1]
        # the split sizes are the channel counts of the tensors the pieces are added to; the caller names them
        assert sum(parts) == n
        return y.split(parts, 1)

    @staticmethod
    def cbfuse(xs, last):   # every routed piece resized (nearest) to the last tensor's size, all summed
        out = F.interpolate(xs[0], size=last.shape[2:], mode="nearest")
        for t in xs[1:]:
            out = out + F.interpolate(t, size=last.shape[2:], mode="nearest")
        return out + last

    def detect(self, feats, det):
        out = []
        w = self.sd[det + ".dfl.conv.weight"].reshape(16)
        for lv, f in enumerate(feats):
            b = self.conv(self.conv(f, f"{det}.cv2.{lv}.0"), f"{det}.cv2.{lv}.1", g=4)
            b = F.conv2d(b, self.sd[f"{det}.cv2.{lv}.2.weight"], self.sd[f"{det}.cv2.{lv}.2.bias"], groups=4).flatten(2)   # (B, 64, cells)
            k = self.conv(self.conv(f, f"{det}.cv3.{lv}.0"), f"{det}.cv3.{lv}.1")
            k = F.conv2d(k, self.sd[f"{det}.cv3.{lv}.2.weight"], self.sd[f"{det}.cv3.{lv}.2.bias"]).flatten(2)
            B, _, n = b.shape
            dist = (b.reshape(B, 4, 16, n).softmax(2) * w[None, None, :, None]).sum(2)   # DFL
            out.append(torch.cat([dist, k], 1))
        return out

    def heads(self, x):
        """x: [B, 3, H, W] -> ([B, 4 + nc, gh * gw] per level in fp64, strides)"""
        x = x.to(torch.float64)
        H = x.shape[2]
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
        tiny = self.name in ("yolov9t", "yolov9s")
        # unconverted m and c keep the checkpoint's leading Silence layer (model.0) and read the auxiliary branch
        aux = self.name == "yolov9c" or (self.name == "yolov9m" and not self.converted)
        o = 1 if aux else 0
        M = lambda k: f"model.{k + o}"  # noqa: E731
        img = x
        x = self.conv(self.conv(img, M(0), 2), M(1), 2)
        x = self.elan1(x, M(2)) if tiny else self.elan4(x, M(2))
        p3 = self.elan4(self.down(x, M(3)), M(4))
        p4 = self.elan4(self.down(p3, M(5)), M(6))
        p5 = self.elan4(self.down(p4, M(7)), M(8))
        if not aux:
            s9 = self.sppelan(p5, M(9))
            n12 = self.elan4(torch.cat([up(s9), p4], 1), M(12))
            n15 = self.elan4(torch.cat([up(n12), p3], 1), M(15))
            n18 = self.elan4(torch.cat([self.down(n15, M(16)), n12], 1), M(18))
            n21 = self.elan4(torch.cat([self.down(n18, M(19)), s9], 1), M(21))
            feats = [n15, n18, n21]
            det = "model.29" if tiny and not self.converted else "model.22"
        else:
            a = self.conv(self.conv(img, M(25), 2), M(26), 2)
            a29 = self.down(self.elan4(a, M(27)), M(28))
            c3 = a29.shape[1]
            c4 = self.sd[M(31) + ".cv1.conv.weight"].shape[0] * (2 if M(31) + ".cv2.conv.weight" in self.sd else 1)
            c5 = self.sd[M(34) + ".cv1.conv.weight"].shape[0] * (2 if M(34) + ".cv2.conv.weight" in self.sd else 1)
            r23 = self.cblinear(p3, M(22), [c3])
            r24 = self.cblinear(p4, M(23), [c3, c4])
            r25 = self.cblinear(p5, M(24), [c3, c4, c5])
            a31 = self.elan4(self.cbfuse([r23[0], r24[0], r25[0]], a29), M(30))
            a34 = self.elan4(self.cbfuse([r24[1], r25[1]], self.down(a31, M(31))), M(33))
            a37 = self.elan4(self.cbfuse([r25[2]], self.down(a34, M(34))), M(36))
            feats = [a31, a34, a37]
            det = M(37)
        return self.detect(feats, det), [H // f.shape[2] for f in feats]


__all__ = ["Yolov9"]
