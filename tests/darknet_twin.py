"""PyTorch fp64 restatement of the three Darknet detection networks (YOLOv3, YOLOv3-tiny, YOLOv4) up to their detect convolutions, evaluated
from a state dict under the reference's `.wts` key names (module_list.<i>.Conv2d / BatchNorm2d).  The network is walked the way Darknet parses
its cfg: every module appends its output to a list, `from` fields are module numbers, and the cfg itself is synth.darknet_rows - written from
the published cfg files and compared row by row with the C++ host builder's own table in tests/test_darknet_cpu.py.  What is stated here is
what each module kind computes:
  L   conv2d(no bias, padding k // 2) -> BatchNorm2d (the eps the reference file passes) -> LeakyReLU(0.1)
  M   the same with Mish, x * tanh(softplus(x))
  D   the biased 1x1 detect convolution
  S   the sum of two modules;  R  one module, or the channel concatenation of several in the order given
  P   max_pool2d(k, s, p);  U  nearest upsample by 2
  Z   yolov3-tiny's module 11: ZERO padding of one row below and one column right, then max_pool2d(2, stride 1).  The zeros are values: the
      map holds LeakyReLU outputs, negative in places, and the border maxima are taken against 0 (a pool that skipped its border would not).
Returns the detect convolutions' outputs in the plugin's input order (coarsest first for yolov3 and yolov3-tiny, finest first for yolov4)
and their strides.  Not a test module (no test_ prefix)."""
import torch
import torch.nn.functional as F

from tensorrtx_amd import synth


class Darknet:
    def __init__(self, sd, name):
        assert name in synth.DARKNET_MODELS, name
        self.sd = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items()}
        self.name = name
        self.eps = synth.DARKNET_BN_EPS[name]
        self.rows = synth.darknet_rows(name)

    def conv_bn(self, x, i, s, p):
        w = self.sd[f"module_list.{i}.Conv2d.weight"]
        bn = f"module_list.{i}.BatchNorm2d"
        gm, bt, mu, var = (self.sd[f"{bn}.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
        y = F.conv2d(x, w, None, s, p)
        return (y - mu[:, None, None]) / torch.sqrt(var[:, None, None] + self.eps) * gm[:, None, None] + bt[:, None, None]

    def strides(self):
        return synth.DARKNET_STRIDES[self.name]

    def anchors(self):
        return synth.DARKNET_ANCHORS[self.name]

    def heads(self, img):
        """img: [B, 3, H, W] -> ([B, 3 * (5 + classes), gh, gw] per plugin input, strides)"""
        x = torch.as_tensor(img, dtype=torch.float64)
        y, dets = [], []
        for i, kind, ch, k, s, p, frm in self.rows:
            src = [y[j] for j in frm] if frm else [y[i - 1] if i else x]
            if kind == "L":
                out = F.leaky_relu(self.conv_bn(src[0], i, s, p), 0.1)
            elif kind == "M":
                out = F.mish(self.conv_bn(src[0], i, s, p))
            elif kind == "D":
                out = F.conv2d(src[0], self.sd[f"module_list.{i}.Conv2d.weight"], self.sd[f"module_list.{i}.Conv2d.bias"])
                dets.append(out)
            elif kind == "S":
                out = src[0] + src[1]
            elif kind == "R":
                out = src[0] if len(src) == 1 else torch.cat(src, 1)
            elif kind == "P":
                out = F.max_pool2d(src[0], k, s, p)
            elif kind == "Z":
                out = F.max_pool2d(F.pad(src[0], (0, 1, 0, 1), value=0.0), 2, 1)
            elif kind == "U":
                out = F.interpolate(src[0], scale_factor=2, mode="nearest")
            else:
                assert kind == "Y", kind
                out = None
            y.append(out)
        return dets, self.strides()
