"""Independent PyTorch fp64 restatement of the six YOLOv10 detection models, written from the reference's builders (yolov10/src/model.cpp:
buildEngineYolov10Det{N,S,M,BL,X}) and blocks (yolov10/src/block.cpp: convBnSiLU, C2F, SPPF, SCDown, Attention, PSA, RepVGGDW, CIB, C2fCIB,
DFL), evaluated from a state dict under the ultralytics key names.  The per-model differences are restated here from the reference's text,
not read from tensorrtx_amd.synth.  Not a test module (no test_ prefix)."""
import math

import torch
import torch.nn.functional as F

SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 768), "b": (0.67, 1.00, 512), "l": (1.00, 1.00, 512),
          "x": (1.00, 1.25, 512)}   # yolov10_det.cpp:111-141
# stages 6, 8, 13, 19, 22: (block, lk).  "c2f" takes the builder's shortcut (true in the backbone, false in the neck); "cib" is
# C2fCIB(shortcut = true, lk)
_F, _C, _L = ("c2f", False), ("cib", False), ("cib", True)
STAGES = {"n": (_F, _F, _F, _F, _L), "s": (_F, _L, _F, _F, _L), "m": (_F, _C, _F, _C, _C), "b": (_F, _C, _C, _C, _C),
          "l": (_F, _C, _C, _C, _C), "x": (_C, _C, _C, _C, _C)}


class Yolov10:
    def __init__(self, sd, name="yolov10n", num_class=80):
        self.sd = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items()}
        self.letter = name[-1]
        self.gd, self.gw, self.mc = SCALES[self.letter]
        self.nc = num_class

    def width(self, x):
        return int(math.ceil(min(x, self.mc) * self.gw / 8)) * 8

    def depth(self, x):
        return 1 if x == 1 else max(round(x * self.gd), 1)   # Python's round is the half-to-even get_depth spells out

    def conv(self, x, name, s=1, g=1, act=True):
        w = self.sd[name + ".conv.weight"]
        y = F.conv2d(x, w, None, s, w.shape[-1] // 2, 1, g)
        gm, bt = self.sd[name + ".bn.weight"], self.sd[name + ".bn.bias"]
        mu, var = self.sd[name + ".bn.running_mean"], self.sd[name + ".bn.running_var"]
        y = (y - mu[:, None, None]) / torch.sqrt(var[:, None, None] + 1e-3) * gm[:, None, None] + bt[:, None, None]
        return F.silu(y) if act else y

    def dw(self, x, name, act=True):
        return self.conv(x, name, g=x.shape[1], act=act)

    def c2f(self, x, name, n, shortcut):
        y = list(self.conv(x, name + ".cv1").chunk(2, 1))
        for i in range(n):
            m = f"{name}.m.{i}"
            t = self.conv(self.conv(y[-1], m + ".cv1"), m + ".cv2")
            y.append(y[-1] + t if shortcut else t)
        return self.conv(torch.cat(y, 1), name + ".cv2")

    def cib(self, x, name, lk):
        y = self.dw(x, name + ".cv1.0")
        y = self.conv(y, name + ".cv1.1")
        if lk:   # RepVGGDW: SiLU(dw7 + dw3)
            y = F.silu(self.dw(y, name + ".cv1.2.conv", act=False) + self.dw(y, name + ".cv1.2.conv1", act=False))
        else:
            y = self.dw(y, name + ".cv1.2")
        y = self.conv(y, name + ".cv1.3")
        y = self.dw(y, name + ".cv1.4")
        return x + y   # C2fCIB always passes shortcut = true and c1 == c2

    def c2fcib(self, x, name, n, lk):
        y = list(self.conv(x, name + ".cv1").chunk(2, 1))
        for i in range(n):
            y.append(self.cib(y[-1], f"{name}.m.{i}", lk))
        return self.conv(torch.cat(y, 1), name + ".cv2")

    def stage(self, x, idx, name, n, c2f_shortcut):
        kind, lk = STAGES[self.letter][idx]
        return self.c2f(x, name, n, c2f_shortcut) if kind == "c2f" else self.c2fcib(x, name, n, lk)

    def scdown(self, x, name):   # 1x1 + SiLU, then depthwise 3x3 stride 2 + BN, no activation
        y = self.conv(x, name + ".cv1")
        return self.conv(y, name + ".cv2", s=2, g=y.shape[1], act=False)

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

    def psa(self, x, name):
        a, b = self.conv(x, name + ".cv1").chunk(2, 1)
        b = b + self.attention(b, name + ".attn", b.shape[1] // 64)
        b = b + self.conv(self.conv(b, name + ".ffn.0"), name + ".ffn.1", act=False)
        return self.conv(torch.cat([a, b], 1), name + ".cv2")

    def heads(self, x):
        """x: [B, 3, H, W] -> three fp64 [B, 4 + nc, gh * gw] tensors (DFL-decoded distances + class logits) and the strides"""
        x = x.to(torch.float64)
        H = x.shape[2]
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
        x = self.conv(x, "model.0", 2)
        x = self.conv(x, "model.1", 2)
        x = self.c2f(x, "model.2", self.depth(3), True)
        p3 = x = self.conv(x, "model.3", 2)
        x4 = x = self.c2f(x, "model.4", self.depth(6), True)
        p4 = x = self.scdown(x, "model.5")
        x6 = x = self.stage(x, 0, "model.6", self.depth(6), True)
        p5 = x = self.scdown(x, "model.7")
        x = self.stage(x, 1, "model.8", self.depth(3), True)
        x = self.sppf(x, "model.9")
        x10 = self.psa(x, "model.10")
        x13 = self.stage(torch.cat([up(x10), x6], 1), 2, "model.13", self.depth(3), False)
        x16 = self.c2f(torch.cat([up(x13), x4], 1), "model.16", self.depth(3), False)
        x19 = self.stage(torch.cat([self.conv(x16, "model.17", 2), x13], 1), 3, "model.19", self.depth(3), False)
        x22 = self.stage(torch.cat([self.scdown(x19, "model.20"), x10], 1), 4, "model.22", self.depth(3), False)
        strides = [H // t.shape[2] for t in (p3, p4, p5)]
        dfl = self.sd["model.23.dfl.conv.weight"].reshape(16)
        out = []
        for lv, f in enumerate((x16, x19, x22)):
            s2, s3 = f"model.23.one2one_cv2.{lv}", f"model.23.one2one_cv3.{lv}"
            b = self.conv(self.conv(f, s2 + ".0"), s2 + ".1")
            b = F.conv2d(b, self.sd[s2 + ".2.weight"], self.sd[s2 + ".2.bias"])
            c = self.dw(f, s3 + ".0.0")
            c = self.conv(c, s3 + ".0.1")
            c = self.dw(c, s3 + ".1.0")
            c = self.conv(c, s3 + ".1.1")
            c = F.conv2d(c, self.sd[s3 + ".2.weight"], self.sd[s3 + ".2.bias"])
            B = b.shape[0]
            box = b.reshape(B, 4, 16, -1).softmax(2)
            box = (box * dfl[None, None, :, None]).sum(2)
            out.append(torch.cat([box, c.reshape(B, self.nc, -1)], 1))
        return out, strides
