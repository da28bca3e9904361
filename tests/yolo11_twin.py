"""Independent PyTorch restatement of the YOLO11 detection model (ultralytics semantics, the modules the reference's
yolo11/src/block.cpp comments quote: Conv, Bottleneck, C3k, C3k2, SPPF, Attention, PSABlock, C2PSA, DWConv, DFL, Detect),
evaluated from a state dict under the ultralytics key names.  Used by the YOLO11 tests to check the C++ host builder's graph.
Not a test module (no test_ prefix)."""
import math

import torch
import torch.nn.functional as F

SCALES = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512), "l": (1.00, 1.00, 512), "x": (1.00, 1.50, 512)}


class Yolo11:
    def __init__(self, sd, scale="n", num_class=80):
        self.sd = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items()}
        self.gd, self.gw, self.mc = SCALES[scale]
        self.c3k = scale in "mlx"
        self.nc = num_class

    def width(self, x):
        return int(math.ceil(min(x, self.mc) * self.gw / 8)) * 8

    def depth(self, x):
        return 1 if x == 1 else max(round(x * self.gd), 1)

    # Conv = conv2d(bias=False, padding=k//2, groups) -> BatchNorm2d(eps=1e-3) -> SiLU (or identity with act=False)
    def conv(self, x, name, s=1, g=1, act=True):
        w = self.sd[name + ".conv.weight"]
        y = F.conv2d(x, w, None, s, w.shape[-1] // 2, 1, g)
        gm, bt = self.sd[name + ".bn.weight"], self.sd[name + ".bn.bias"]
        mu, var = self.sd[name + ".bn.running_mean"], self.sd[name + ".bn.running_var"]
        y = (y - mu[:, None, None]) / torch.sqrt(var[:, None, None] + 1e-3) * gm[:, None, None] + bt[:, None, None]
        return F.silu(y) if act else y

    def bottleneck(self, x, name, shortcut):
        y = self.conv(self.conv(x, name + ".cv1"), name + ".cv2")
        return x + y if shortcut and x.shape[1] == y.shape[1] else y

    def c3k_block(self, x, name, n, shortcut):
        a = self.conv(x, name + ".cv1")
        for i in range(n):
            a = self.bottleneck(a, f"{name}.m.{i}", shortcut)
        return self.conv(torch.cat([a, self.conv(x, name + ".cv2")], 1), name + ".cv3")

    def c3k2(self, x, name, n, c3k, shortcut=True):
        y = list(self.conv(x, name + ".cv1").chunk(2, 1))
        for i in range(n):
            m = f"{name}.m.{i}"
            y.append(self.c3k_block(y[-1], m, 2, shortcut) if c3k else self.bottleneck(y[-1], m, shortcut))
        return self.conv(torch.cat(y, 1), name + ".cv2")

    def sppf(self, x, name):
        y = [self.conv(x, name + ".cv1")]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], 5, 1, 2))
        return self.conv(torch.cat(y, 1), name + ".cv2")

    def attention(self, x, name, num_heads):
        B, C, H, W = x.shape
        N = H * W
        head_dim = C // num_heads
        key_dim = int(head_dim * 0.5)
        qkv = self.conv(x, name + ".qkv", act=False)
        q, k, v = qkv.view(B, num_heads, key_dim * 2 + head_dim, N).split([key_dim, key_dim, head_dim], dim=2)
        attn = ((q.transpose(-2, -1) @ k) * key_dim ** -0.5).softmax(dim=-1)
        y = (v @ attn.transpose(-2, -1)).view(B, C, H, W) + self.conv(v.reshape(B, C, H, W), name + ".pe", g=C, act=False)
        return self.conv(y, name + ".proj", act=False)

    def c2psa(self, x, name, n):
        a, b = self.conv(x, name + ".cv1").chunk(2, 1)
        c = b.shape[1]
        for i in range(n):
            m = f"{name}.m.{i}"
            b = b + self.attention(b, m + ".attn", c // 64)
            b = b + self.conv(self.conv(b, m + ".ffn.0"), m + ".ffn.1", act=False)
        return self.conv(torch.cat([a, b], 1), name + ".cv2")

    def heads(self, x):
        """x: [B, 3, H, W] -> three [B, 4 + nc, gh*gw] tensors (DFL-decoded boxes + class logits) and the strides"""
        x = x.to(torch.float64)
        H = x.shape[2]
        d, c3k = self.depth(2), self.c3k
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
        x = self.conv(x, "model.0", 2)
        x = self.conv(x, "model.1", 2)
        x = self.c3k2(x, "model.2", d, c3k)
        p3 = x = self.conv(x, "model.3", 2)
        x4 = x = self.c3k2(x, "model.4", d, c3k)
        p4 = x = self.conv(x, "model.5", 2)
        x6 = x = self.c3k2(x, "model.6", d, True)
        p5 = x = self.conv(x, "model.7", 2)
        x = self.c3k2(x, "model.8", d, True)
        x = self.sppf(x, "model.9")
        x10 = self.c2psa(x, "model.10", d)
        x13 = self.c3k2(torch.cat([up(x10), x6], 1), "model.13", d, c3k)
        x16 = self.c3k2(torch.cat([up(x13), x4], 1), "model.16", d, c3k)
        x19 = self.c3k2(torch.cat([self.conv(x16, "model.17", 2), x13], 1), "model.19", d, c3k)
        x22 = self.c3k2(torch.cat([self.conv(x19, "model.20", 2), x10], 1), "model.22", d, True)
        strides = [H // t.shape[2] for t in (p3, p4, p5)]
        dfl = self.sd["model.23.dfl.conv.weight"].reshape(16)
        out = []
        for lv, f in enumerate((x16, x19, x22)):
            s2, s3 = f"model.23.cv2.{lv}", f"model.23.cv3.{lv}"
            b = self.conv(self.conv(f, s2 + ".0"), s2 + ".1")
            b = F.conv2d(b, self.sd[s2 + ".2.weight"], self.sd[s2 + ".2.bias"])
            c = self.conv(f, s3 + ".0.0", g=f.shape[1])
            c = self.conv(c, s3 + ".0.1")
            c = self.conv(c, s3 + ".1.0", g=c.shape[1])
            c = self.conv(c, s3 + ".1.1")
            c = F.conv2d(c, self.sd[s3 + ".2.weight"], self.sd[s3 + ".2.bias"])
            B = b.shape[0]
            box = b.reshape(B, 4, 16, -1).softmax(2)
            box = (box * dfl[None, None, :, None]).sum(2)
            out.append(torch.cat([box, c.reshape(B, self.nc, -1)], 1).float())
        return out, strides
