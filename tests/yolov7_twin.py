"""Independent PyTorch restatement of the YOLOv7 detection graphs the host builder makes (yolov7-tiny, yolov7, yolov7x, yolov7-w6,
yolov7-e6), from the models' published deploy yamls and module definitions (Conv, MP, SP, Concat, Upsample, ReOrg, DownC, SPPCSPC, RepConv,
Detect), evaluated in fp64 from a state dict under the checkpoint's key names.  A model is walked the way the yaml is parsed: every yaml
layer appends its output to a list, its weights are "model.<index>", and `from` fields are relative or absolute indices.  Every channel
count and kernel size is read from the weights; what is stated here is the wiring.  Returns what the detect convolutions `m.i` emit -
the tensors the reference hands to its YoloLayer plugin - and the level strides.  Like the reference, it applies neither ImplicitA nor
ImplicitM.  Used by the YOLOv7 tests to check the C++ host builder's graph.  Not a test module (no test_ prefix)."""
import torch
import torch.nn.functional as F


class Yolov7:
    def __init__(self, sd, name="yolov7"):
        self.sd = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items()}
        self.name = name
        self.tiny = name == "yolov7tiny"

    def bn(self, y, name, eps):
        gm, bt = self.sd[name + ".weight"], self.sd[name + ".bias"]
        mu, var = self.sd[name + ".running_mean"], self.sd[name + ".running_var"]
        return (y - mu[:, None, None]) / torch.sqrt(var[:, None, None] + eps) * gm[:, None, None] + bt[:, None, None]

    # Conv = conv2d(bias=False, autopad k // 2) -> BatchNorm2d -> SiLU; yolov7-tiny: LeakyReLU(0.1), and its BatchNorm keeps PyTorch's eps
    def conv(self, x, name, s=1):
        w = self.sd[name + ".conv.weight"]
        y = self.bn(F.conv2d(x, w, None, s, w.shape[-1] // 2), name + ".bn", 1e-5 if self.tiny else 1e-3)
        return F.leaky_relu(y, 0.1) if self.tiny else F.silu(y)

    # ---- the walk over the yaml: self.y[i] is layer i's output
    def src(self, f):
        return self.img if len(self.y) + f < 0 else self.y[f]

    def add(self, t):
        self.y.append(t)
        return len(self.y) - 1

    def key(self):
        return f"model.{len(self.y)}"

    def C(self, f=-1, s=1):
        return self.add(self.conv(self.src(f), self.key(), s))

    def cat(self, *fs):
        return self.add(torch.cat([self.src(f) for f in fs], 1))

    def MP(self):
        return self.add(F.max_pool2d(self.y[-1], 2, 2))

    def SP(self, f, k):
        return self.add(F.max_pool2d(self.src(f), k, 1, k // 2))

    def up(self):
        return self.add(F.interpolate(self.y[-1], scale_factor=2, mode="nearest"))

    def reorg(self):
        x = self.src(-1)
        return self.add(torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1))

    def downc(self):   # cat(cv2(cv1(x)) at stride 2, cv3(maxpool(x)))
        k, x = self.key(), self.y[-1]
        return self.add(torch.cat([self.conv(self.conv(x, k + ".cv1"), k + ".cv2", 2), self.conv(F.max_pool2d(x, 2, 2), k + ".cv3")], 1))

    def sppcspc(self):
        k, x = self.key(), self.y[-1]
        x1 = self.conv(self.conv(self.conv(x, k + ".cv1"), k + ".cv3"), k + ".cv4")
        y1 = self.conv(self.conv(torch.cat([x1] + [F.max_pool2d(x1, m, 1, m // 2) for m in (5, 9, 13)], 1), k + ".cv5"), k + ".cv6")
        return self.add(self.conv(torch.cat([y1, self.conv(x, k + ".cv2")], 1), k + ".cv7"))

    def repconv(self, f):   # SiLU(BN(3x3) + BN(1x1)); the identity branch exists only where c1 == c2, which no head of these models has
        k, x = self.key(), self.y[f]
        assert k + ".rbr_identity.weight" not in self.sd
        a = self.bn(F.conv2d(x, self.sd[k + ".rbr_dense.0.weight"], None, 1, 1), k + ".rbr_dense.1", 1e-3)
        b = self.bn(F.conv2d(x, self.sd[k + ".rbr_1x1.0.weight"]), k + ".rbr_1x1.1", 1e-3)
        return self.add(F.silu(a + b))

    def elan(self, n, picks):
        """[-1, Conv 1x1], [-2, Conv 1x1], n x [-1, Conv 3x3], [picks, Concat], [-1, Conv 1x1]"""
        self.C()
        self.C(-2)
        for _ in range(n):
            self.C()
        self.cat(*picks)
        return self.C()

    def mp_block(self, *extra):
        """[-1, MP], [-1, Conv 1x1], [-3, Conv 1x1], [-1, Conv 3x3 / 2], [[-1, -3, extra], Concat]"""
        self.MP()
        self.C()
        self.C(-3)
        self.C(-1, 2)
        return self.cat(-1, -3, *extra)

    def lateral(self, route):
        """[-1, Conv 1x1], [-1, Upsample], [route, Conv 1x1], [[-1, -2], Concat]"""
        self.C()
        self.up()
        self.C(route)
        return self.cat(-1, -2)

    def heads(self, x):
        """x: [B, 3, H, W] -> ([B, 3 * (5 + nc), gh, gw] per level in fp64, strides)"""
        self.img, self.y = x.to(torch.float64), []
        all4, all6, all8 = (-1, -2, -3, -4), (-1, -2, -3, -4, -5, -6), (-1, -2, -3, -4, -5, -6, -7, -8)
        odd4, odd6 = (-1, -3, -5, -6), (-1, -3, -5, -7, -8)
        n = self.name
        if n == "yolov7tiny":   # cfg/deploy/yolov7-tiny.yaml
            self.C(-1, 2)
            self.C(-1, 2)
            self.elan(2, all4)
            self.MP()
            b3 = self.elan(2, all4)
            self.MP()
            b4 = self.elan(2, all4)
            self.MP()
            self.elan(2, all4)
            self.C()                       # 29
            self.C(-2)                     # 30
            self.SP(-1, 5)
            self.SP(-2, 9)
            self.SP(-3, 13)
            self.cat(*all4)
            self.C()
            self.cat(-1, -7)
            b5 = self.C()                  # 37
            self.lateral(b4)
            n4 = self.elan(2, all4)
            self.lateral(b3)
            n3 = self.elan(2, all4)
            self.C(-1, 2)
            self.cat(-1, n4)
            m4 = self.elan(2, all4)
            self.C(-1, 2)
            self.cat(-1, b5)
            m5 = self.elan(2, all4)
            feats = [self.C(n3), self.C(m4), self.C(m5)]
        elif n in ("yolov7", "yolov7x"):   # cfg/deploy/yolov7.yaml, yolov7x.yaml
            k, back = (4, odd4) if n == "yolov7" else (6, odd6)
            head = all6 if n == "yolov7" else odd6
            self.C()
            self.C(-1, 2)
            self.C()
            self.C(-1, 2)
            self.elan(k, back)
            self.mp_block()
            b3 = self.elan(k, back)
            self.mp_block()
            b4 = self.elan(k, back)
            self.mp_block()
            self.elan(k, back)
            b5 = self.sppcspc()
            self.lateral(b4)
            n4 = self.elan(k, head)
            self.lateral(b3)
            n3 = self.elan(k, head)
            self.mp_block(n4)
            m4 = self.elan(k, head)
            self.mp_block(b5)
            m5 = self.elan(k, head)
            feats = [self.repconv(f) if n == "yolov7" else self.C(f) for f in (n3, m4, m5)]
        else:   # cfg/deploy/yolov7-w6.yaml, yolov7-e6.yaml
            assert n in ("yolov7w6", "yolov7e6"), n
            e6 = n == "yolov7e6"
            k, back, head = (6, odd6, all8) if e6 else (4, odd4, all6)

            def down(route=None):
                if e6:
                    self.downc()
                else:
                    self.C(-1, 2)
                return self.cat(-1, route) if route is not None else None

            self.reorg()
            self.C()
            down()
            self.elan(k, back)
            down()
            b3 = self.elan(k, back)
            down()
            b4 = self.elan(k, back)
            down()
            b5 = self.elan(k, back)
            down()
            self.elan(k, back)
            b6 = self.sppcspc()
            self.lateral(b5)
            n5 = self.elan(k, head)
            self.lateral(b4)
            n4 = self.elan(k, head)
            self.lateral(b3)
            n3 = self.elan(k, head)
            down(n4)
            m4 = self.elan(k, head)
            down(n5)
            m5 = self.elan(k, head)
            down(b6)
            m6 = self.elan(k, head)
            feats = [self.C(f) for f in (n3, m4, m5, m6)]
        det = self.key()
        out = [F.conv2d(self.y[f], self.sd[f"{det}.m.{i}.weight"], self.sd[f"{det}.m.{i}.bias"]) for i, f in enumerate(feats)]
        self.det = det
        return out, [x.shape[2] // o.shape[2] for o in out]

    def anchors(self):
        """[levels][6] from <detect>.anchor_grid (call heads() first)"""
        ag = self.sd[self.det + ".anchor_grid"].to(torch.float32)
        return ag.reshape(-1, 6).numpy()


__all__ = ["Yolov7"]
