"""Independent PyTorch restatement of the YOLOv12 detection model that the reference's yolov12/ builds (ultralytics-style modules:
Conv, Bottleneck, C3k, C3k2, AAttn, ABlock, A2C2f, DWConv, DFL, Detect), evaluated from a state dict under the ultralytics key names.
The channel arithmetic is the reference's: its A2C2f hidden width is 2 * int(c2 * 0.25), num_heads = that / 32, 32 channels per head for
each of q, k, v, scale 0.176777, and A2C2f has neither gamma nor the outer residual.  Used by the YOLOv12 tests to check the C++ host
builder's graph, and to record what the attention of the synthetic weights looks like.  Not a test module (no test_ prefix)."""
import torch
import torch.nn.functional as F

from yolo11_twin import SCALES, Yolo11


class Yolo12(Yolo11):
    """conv / bottleneck / c3k_block / c3k2 / width / depth are YOLO11's modules (ultralytics shares them too)"""

    def __init__(self, sd, scale="n", num_class=80):
        super().__init__(sd, scale, num_class)
        self.attn_peak = {}   # block name -> mean over (image, area, head, query) of the largest softmax weight, and keys per area

    def conv_b(self, x, name, g=1):   # Conv with a convolution bias, no activation (AAttn.pe)
        w = self.sd[name + ".conv.weight"]
        y = F.conv2d(x, w, self.sd[name + ".conv.bias"], 1, w.shape[-1] // 2, 1, g)
        gm, bt = self.sd[name + ".bn.weight"], self.sd[name + ".bn.bias"]
        mu, var = self.sd[name + ".bn.running_mean"], self.sd[name + ".bn.running_var"]
        return (y - mu[:, None, None]) / torch.sqrt(var[:, None, None] + 1e-3) * gm[:, None, None] + bt[:, None, None]

    def aattn(self, x, name, num_heads, area):
        B, C, H, W = x.shape
        N = H * W
        hd = C // num_heads
        qkv = self.conv(x, name + ".qkv", act=False).flatten(2).transpose(1, 2)   # (B, N, 3C)
        if area > 1:
            qkv = qkv.reshape(B * area, N // area, 3 * C)
            B, N = B * area, N // area
        q, k, v = qkv.view(B, N, num_heads, 3 * hd).permute(0, 2, 3, 1).split([hd, hd, hd], dim=2)   # each (B, heads, hd, N)
        attn = ((q.transpose(-2, -1) @ k) * 0.176777).softmax(dim=-1)
        self.attn_peak[name] = (attn.max(-1).values.mean().item(), N)
        y = (v @ attn.transpose(-2, -1)).permute(0, 3, 1, 2)   # (B, N, heads, hd)
        v = v.permute(0, 3, 1, 2)
        if area > 1:
            B, N = B // area, N * area
        y = y.reshape(B, H, W, C).permute(0, 3, 1, 2)
        v = v.reshape(B, H, W, C).permute(0, 3, 1, 2)
        return self.conv(y + self.conv_b(v, name + ".pe", g=C), name + ".proj", act=False)

    def ablock(self, x, name, num_heads, area):
        x = x + self.aattn(x, name + ".attn", num_heads, area)
        return x + self.conv(self.conv(x, name + ".mlp.0"), name + ".mlp.1", act=False)

    def a2c2f(self, x, name, a2, area=1):
        y = [self.conv(x, name + ".cv1")]
        if a2:
            heads = y[0].shape[1] // 32
            for i in range(2):
                t = y[-1]
                for j in range(2):
                    t = self.ablock(t, f"{name}.m.{i}.{j}", heads, area)
                y.append(t)
        else:
            y.append(self.c3k_block(y[0], name + ".m.0", 2, True))
        return self.conv(torch.cat(y, 1), name + ".cv2")

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
        x6 = x = self.a2c2f(x, "model.6", True, 4)
        p5 = x = self.conv(x, "model.7", 2)
        x8 = self.a2c2f(x, "model.8", True, 1)
        x11 = self.a2c2f(torch.cat([up(x8), x6], 1), "model.11", False)
        x14 = self.a2c2f(torch.cat([up(x11), x4], 1), "model.14", False)
        x17 = self.a2c2f(torch.cat([self.conv(x14, "model.15", 2), x11], 1), "model.17", False)
        x20 = self.c3k2(torch.cat([self.conv(x17, "model.18", 2), x8], 1), "model.20", d, True)
        strides = [H // t.shape[2] for t in (p3, p4, p5)]
        dfl = self.sd["model.21.dfl.conv.weight"].reshape(16)
        out = []
        for lv, f in enumerate((x14, x17, x20)):
            s2, s3 = f"model.21.cv2.{lv}", f"model.21.cv3.{lv}"
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


__all__ = ["SCALES", "Yolo12"]
