"""The layer conformance table: small networks for the generic NHWC kernels (kernels/nhwc_ops.hip) and the LINEAR kernels
(kernels/linear_ops.hip), shared by tests/test_layers_cpu.py (plans, instantiations, the interpreter) and tests/test_gpu_layers.py
(the engines).  Every case carries
  * `inputs`: name -> (dims, generator); dims are per sample (implicit batch) or whole (explicit batch), the data is seeded by the name;
  * `build(net, t)`: the network, through tensorrtx_amd.builder.Network, on the input tensor ids `t`; returns {output name: tensor id};
  * `ref(x)`: the same computation written directly in torch fp64 on the inputs `x` (already rounded to the engine's storage type);
    with `by_precision` set it is `ref(x, fp16)` - the MFMA convolutions and the stem of an fp16 plan multiply fp16 WEIGHTS, a rounding
    of a constant the reference has to apply itself rather than count as a site;
    returns {output name: Out or [Out, ...]} with, per Out, the reference, its magnitude (None = bit-exact data movement), the number
    of terms of the longest fp32 sum, an extra relative term where the function amplifies the rounding of its argument, and the fp16
    rounding sites between the rounded input and the output (counted next to each family below);
  * `kinds` / `absent`: op kinds the lowered plan must / must not contain (a pair (fp32, fp16) where the two plans differ);
  * `inst`: (op kind, instantiation in the fp32 plan, instantiation in the fp16 plan) the case is meant to hit;
  * `half`: the inputs an fp16 plan stores in fp16 (they enter an NHWC tensor); LINEAR tensors are fp32 in both engines.

Shared devices: `nhwc()` is a 1x1 stride-1 max-pool (to_nhwc -> pool: an exact way to put a network input into NHWC, 0 sites);
`select_conv()` is a 1x1 convolution with one-hot weights (each output channel a copy of one input channel: exact in fp32 and, on
fp16 inputs, in fp16 - the 12-channel neighbour of a concat, and the convolution in front of the SPPF pools)."""
import itertools
import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from tensorrtx_amd import builder

U32 = 2.0 ** -24
F16_MAX = 65504.0


@dataclass
class Out:
    ref: torch.Tensor
    mag: object = None      # None: exact
    n: int = 1
    amp: object = 0.0
    sites: int = 0
    ch: slice = None        # the channels (dim 1) of the binding this Out covers; None = all
    batched: bool = True    # False: the binding has no batch dimension (a constant)


@dataclass
class Case:
    name: str
    family: str
    inputs: dict
    build: object
    ref: object
    kinds: object
    absent: object = frozenset()
    inst: tuple = None
    half: object = "all"
    batch: int = 1
    max_batch: int = None
    explicit: bool = False
    cond: object = None     # conditioning of the reference alone: callable(x) that asserts
    direct: bool = False    # every conv / deconv of the plan must be the direct kernel (igemm, dw and stem false)
    igemm: bool = False     # the convolution under test (the plan's last; helpers come first) is on the MFMA implicit-GEMM kernel, in both plans
    stem: bool = False      # ... is the stem kernel (it reads the fp32 network input itself), in both plans
    by_precision: bool = False   # ref takes (x, fp16)
    fused: dict = None      # conv fields the lowered plan must show (act1, act2, residual)

    def __post_init__(self):
        if self.max_batch is None:
            self.max_batch = self.batch

    def kinds_for(self, fp16):
        return set(self.kinds[fp16] if isinstance(self.kinds, tuple) else self.kinds)

    def absent_for(self, fp16):
        return set(self.absent[fp16] if isinstance(self.absent, tuple) else self.absent)


# ---- input generators ----------------------------------------------------------------------------------------------------------------
SPECIAL = [0.0, 30.0, -30.0, 88.0, -88.0, F16_MAX, -F16_MAX, 1.0, -1.0, 0.5]


def _special(rng, shape):
    a = rng.standard_normal(shape).astype(np.float32) * 3
    flat = a.reshape(-1)
    n = min(len(SPECIAL), flat.size)
    flat[:n] = SPECIAL[:n]
    if flat.size >= 2 * len(SPECIAL):   # and at the far end (the last vector / the tail of the last sample)
        flat[-len(SPECIAL):] = SPECIAL
    return a


def _logits80(rng, shape):
    a = rng.standard_normal(shape).astype(np.float32) * 30
    a = np.clip(a, -80, 80)
    flat = a.reshape(-1)
    flat[::7] = 80.0
    flat[3::7] = -80.0
    return a


GEN = {
    "n": lambda rng, s: rng.standard_normal(s).astype(np.float32),
    "neg": lambda rng, s: (-np.abs(rng.standard_normal(s)) - 0.5).astype(np.float32),
    "pos": lambda rng, s: (0.25 * 16.0 ** rng.random(s)).astype(np.float32),                 # [0.25, 4]
    "div": lambda rng, s: ((0.25 + np.abs(rng.standard_normal(s))) * rng.choice([-1.0, 1.0], s)).astype(np.float32),
    "exp": lambda rng, s: rng.uniform(-2, 2, s).astype(np.float32),
    "special": _special,
    "logits": lambda rng, s: (rng.standard_normal(s) * 3).astype(np.float32),
    "logits80": _logits80,
    "equal": lambda rng, s: np.full(s, 1.25, np.float32),
}


def gen_inputs(case):
    """{name: fp32 numpy [batch, *dims] (implicit batch) or [*dims] (explicit)}"""
    out = {}
    for name, (dims, kind) in case.inputs.items():
        rng = np.random.default_rng(zlib.crc32((case.name + "/" + name).encode()))
        shape = tuple(dims) if case.explicit else (case.batch, *dims)
        out[name] = np.ascontiguousarray((kind if callable(kind) else GEN[kind])(rng, shape), dtype=np.float32)
    return out


def ref_inputs(case, inputs, fp16):
    """the fp64 inputs of the reference: rounded to fp16 where the fp16 engine stores them so"""
    x = {}
    for k, v in inputs.items():
        t = torch.from_numpy(v)
        if fp16 and (case.half == "all" or k in case.half):
            t = t.half()
        x[k] = t.double()
    return x


def build_plan(case, fp16):
    net = builder.Network(max_batch=case.max_batch, fp16=bool(fp16), explicit_batch=case.explicit)
    try:
        t = {name: net.input(name, dims) for name, (dims, _) in case.inputs.items()}
        for name, tid in case.build(net, t).items():
            net.mark_output(tid, name)
        return net.build()
    finally:
        net.close()


def outs_of(case, x, fp16=0):
    """the reference of the inputs `x` = ref_inputs(case, inputs, fp16)"""
    r = case.ref(x, bool(fp16)) if case.by_precision else case.ref(x)
    return {k: (v if isinstance(v, list) else [v]) for k, v in r.items()}


def fp32_bound(o):
    return (1e-5 + o.n * U32 + o.amp) * o.mag + 1e-7


# ---- shared network pieces -----------------------------------------------------------------------------------------------------------
def nhwc(net, t):
    return net.out(net.pooling(t, 1, 1))


def select_conv(net, t, cin, sel):
    w = np.zeros((len(sel), cin, 1, 1), np.float32)
    w[np.arange(len(sel)), np.asarray(sel)] = 1.0
    return net.out(net.conv(t, w))


NEIGHBOUR = [3, 0, 7, 5, 1, 2, 6, 4, 7, 7, 0, 3]   # the 12 channels of the concat's convolution, picked from 8 inputs


CASES = []


def add(**kw):
    c = Case(**kw)
    assert all(c.name != o.name for o in CASES), c.name
    CASES.append(c)
    return c


def _v(c, fp16):
    return c % (8 if fp16 else 4) == 0


def _inst(kind, C, aligned=True):
    """the instantiation a C-channel tensor with ld % v == 0 takes: vector iff C % v == 0 and the view is aligned"""
    return (kind, "x4" if aligned and C % 4 == 0 else "x1", "x8" if aligned and C % 8 == 0 else "x1")


def unary_nhwc(name, family, C, H, W, B, op, opref, kind, *, wrap="plain", gen="n", via_pool=False, out_hw=None, kinds=None, absent=frozenset(),
               max_batch=None, cond=None, inst="auto"):
    """one NHWC op on a C-channel map.  wrap: "plain"; "slice" - the op reads channels [4, 4 + C) of a wider NHWC tensor (coff 4: 16-byte
    aligned in fp32, not in fp16); "concat" - the op writes next to a 12-channel convolution (coff 12: aligned in fp32 only)"""
    Ho, Wo = out_hw if out_hw else (H, W)
    kinds = set(kinds if kinds is not None else {kind})
    if wrap == "plain":
        def build(net, t):
            return {"y": op(net, nhwc(net, t["x"]) if via_pool else t["x"], (C, H, W))}

        def ref(x):
            return {"y": opref(x["x"])}
        inputs = {"x": ((C, H, W), gen)}
        ins = _inst(kind, C)
    elif wrap == "slice":
        def build(net, t):
            return {"y": op(net, net.out(net.slice_channels(nhwc(net, t["x"]), 4, C, (C + 4, H, W))), (C, H, W))}

        def ref(x):
            return {"y": opref(x["x"][:, 4:])}
        inputs = {"x": ((C + 4, H, W), gen)}
        ins = (kind, "x4" if C % 4 == 0 else "x1", "x1")
    else:
        def build(net, t):
            a = select_conv(net, nhwc(net, t["z"]), 8, NEIGHBOUR)
            return {"y": net.out(net.concat([a, op(net, nhwc(net, t["x"]) if via_pool else t["x"], (C, H, W))]))}

        def ref(x):
            o = opref(x["x"])
            o.ch = slice(12, None)
            return {"y": [Out(x["z"][:, NEIGHBOUR], ch=slice(0, 12)), o]}
        inputs = {"x": ((C, H, W), gen), "z": ((8, Ho, Wo), "n")}
        kinds |= {"conv"}
        ins = (kind, "x4" if C % 4 == 0 else "x1", "x1")
    return add(name=name, family=family, inputs=inputs, build=build, ref=ref, kinds=kinds, absent=absent, inst=ins if inst == "auto" else inst,
               batch=B, max_batch=max_batch, cond=cond)


SHAPES = [(1, 13, 17, 1), (5, 13, 17, 3), (8, 1, 9, 1), (12, 13, 17, 3), (16, 1, 1, 1), (24, 13, 17, 1), (72, 13, 17, 3), (5, 1, 1, 3), (12, 1, 9, 1)]
BIG_SCALAR = (12, 128, 128, 3)    # 589 824 items on the fp16 scalar path (> 2048 * 256): the grid-stride loop iterates
BIG_VECTOR = (72, 128, 128, 4)    # 589 824 8-channel items on the fp16 vector path, 1 179 648 on the fp32 one


# ---- 1. pooling: max exact (0 sites); average: kh * kw terms, one fp16 store (1 site) -------------------------------------------------
def _pool(C, H, W, B, mode, k, s, p, **kw):
    kh, kw_ = (k, k) if np.isscalar(k) else k
    sh, sw = (s, s) if np.isscalar(s) else s
    ph, pw = (p, p) if np.isscalar(p) else p
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw_) // sw + 1

    def op(net, t, chw):
        return net.out(net.pooling(t, (kh, kw_), (sh, sw), (ph, pw), avg=mode != "max", avg_exclusive=None if mode == "max" else int(mode == "avgx")))

    def opref(x):
        if mode == "max":
            return Out(F.max_pool2d(x, (kh, kw_), (sh, sw), (ph, pw)))
        f = lambda v: F.avg_pool2d(v, (kh, kw_), (sh, sw), (ph, pw), count_include_pad=mode == "avg")  # noqa: E731
        return Out(f(x), f(x.abs()), n=kh * kw_, sites=1)
    tag = kw.pop("tag", "")
    name = f"pool_{mode}_k{kh}x{kw_}_s{sh}x{sw}_p{ph}x{pw}_c{C}_{H}x{W}_b{B}{tag}"
    return unary_nhwc(name, "pool", C, H, W, B, op, opref, "pool", out_hw=(Ho, Wo), **kw)


POOLS = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (5, 1, 2), (9, 1, 4), (13, 1, 6), ((3, 5), (2, 1), (1, 2)), ((5, 3), (1, 2), (2, 1))]
for (k, s, p), mode in itertools.product(POOLS, ("max", "avg", "avgx")):
    kh, kw_ = (k, k) if np.isscalar(k) else k
    ph, pw = (p, p) if np.isscalar(p) else p
    for C, H, W, B in SHAPES:
        if H + 2 * ph >= kh and W + 2 * pw >= kw_:
            _pool(C, H, W, B, mode, k, s, p)
for C, H, W, B in SHAPES:   # k = H: global pooling
    for mode in ("max", "avg"):
        _pool(C, H, W, B, mode, (H, W), 1, 0, tag="_global")
for C, H, W, B in ((5, 13, 17, 3), (8, 13, 17, 1), (12, 1, 9, 3)):   # all-negative maps: a zero start value or border must fail
    for k, s, p in ((3, 2, 1), (5, 1, 2), ((3, 5), (2, 1), (1, 2))):
        _pool(C, H, W, B, "max", k, s, p, gen="neg", tag="_neg")
for wrap in ("slice", "concat"):
    for C in (8, 12):
        for mode in ("max", "avgx"):
            _pool(C, 13, 17, 3, mode, 3, 1, 1, wrap=wrap, via_pool=True, tag="_" + wrap)
_pool(12, 13, 17, 1, "avgx", 3, 2, 1, max_batch=3, tag="_of3")
_pool(8, 13, 17, 1, "max", (3, 5), (2, 1), (1, 2), max_batch=3, tag="_of3")
_pool(*BIG_SCALAR, "max", 3, 1, 1, tag="_big")
_pool(*BIG_VECTOR, "avgx", 3, 2, 1, tag="_big")


# ---- 2. the SPPF pool chain: exact -------------------------------------------------------------------------------------------------------
def _chain(C, H, W, B, k, chained, gen="n", sppf=True, tag=""):
    sel = [(5 * i + 3) % C for i in range(C)]

    def build(net, t):
        a = select_conv(net, t["x"], C, sel) if sppf else nhwc(net, t["x"])
        y1 = net.out(net.pooling(a, k, 1, k // 2))
        y2 = net.out(net.pooling(y1, k, 1, k // 2))
        y3 = net.out(net.pooling(y2, k, 1, k // 2))
        if sppf:
            return {"y": net.out(net.concat([a, y1, y2, y3]))}
        return {"y1": y1, "y2": y2, "y3": y3}

    def ref(x):
        a = x["x"][:, sel] if sppf else x["x"]
        y1 = F.max_pool2d(a, k, 1, k // 2)
        y2 = F.max_pool2d(y1, k, 1, k // 2)
        y3 = F.max_pool2d(y2, k, 1, k // 2)
        if sppf:
            return {"y": Out(torch.cat([a, y1, y2, y3], 1))}
        return {"y1": Out(y1), "y2": Out(y2), "y3": Out(y3)}
    return add(name=f"chain_k{k}_c{C}_{H}x{W}_b{B}{'_sppf' if sppf else ''}{tag}", family="pool_chain", inputs={"x": ((C, H, W), gen)}, build=build, ref=ref,
               kinds={"pool_chain"} if chained else {"pool"}, absent={"pool"} if chained and sppf else ({"pool_chain"} if not chained else set()),
               inst=("pool_chain", "x4", "x8") if chained else ("pool", "x4", "x8"), batch=B)


for k in (3, 5, 9):
    for H, W in ((1, 1), (7, 9), (20, 20)):
        _chain(8, H, W, 2, k, True)
_chain(8, 40, 40, 1, 5, True)            # 44 * 44 * 32 bytes = 61 952: the largest map the 64 KiB rule accepts for k = 5
_chain(8, 42, 42, 1, 5, False)           # 46 * 46 * 32 = 67 712: stays three pools
_chain(16, 7, 9, 3, 5, True, gen="neg", tag="_neg")
_chain(24, 20, 20, 3, 3, True, gen="neg", tag="_neg")
_chain(8, 7, 9, 2, 5, True, sppf=False)   # behind the layout pass, three separate outputs
_chain(16, 20, 20, 1, 9, True, sppf=False, gen="neg", tag="_neg")


# ---- 3. nearest resize: exact, on the `resize` op (the folded Upsample -> Concat -> Conv1x1 form is tested elsewhere) ------------------------
def _resize(C, H, W, B, scale=None, out_hw=None, **kw):
    Ho, Wo = out_hw if out_hw else (H * scale, W * scale)

    def op(net, t, chw):
        return net.out(net.resize_nearest(t, scale) if scale else net.resize_nearest(t, out_dims=(C, Ho, Wo)))

    def opref(x):   # nearest, asymmetric, floor: source index = floor(dst * in / out) in integers
        hi = (torch.arange(Ho) * H) // Ho
        wi = (torch.arange(Wo) * W) // Wo
        return Out(x[:, :, hi][:, :, :, wi])
    tag = kw.pop("tag", "")
    name = f"resize_{'s%d' % scale if scale else 'to%dx%d' % (Ho, Wo)}_c{C}_{H}x{W}_b{B}{tag}"
    return unary_nhwc(name, "resize", C, H, W, B, op, opref, "resize", out_hw=(Ho, Wo), absent={"deconv"}, **kw)


for C, H, W, B in SHAPES:
    _resize(C, H, W, B, scale=2)
    _resize(C, H, W, B, scale=3)
    _resize(C, H, W, B, out_hw=(H + 2, 2 * W + 3))
_resize(8, 13, 17, 1, out_hw=(5, 6), tag="_down")
for wrap in ("slice", "concat"):
    for C in (8, 12):
        _resize(C, 5, 7, 3, scale=2, wrap=wrap, via_pool=True, tag="_" + wrap)
_resize(8, 5, 7, 1, scale=3, max_batch=3, tag="_of3")
_resize(12, 64, 64, 3, scale=2, tag="_big")
_resize(72, 64, 64, 4, scale=2, tag="_big")


# ---- 4. elementwise ------------------------------------------------------------------------------------------------------------------------
# NHWC: both operands through the exact 1x1 pool, one fp16 store of the result (1 site; max / min exact).  LINEAR: fp32, 0 sites.
EW_GEN = {"sum": ("n", "n"), "prod": ("n", "n"), "max": ("n", "n"), "min": ("n", "n"), "sub": ("n", "n"), "div": ("n", "div"), "pow": ("pos", "exp")}


def _ew_ref(op, a, b, sites):
    if op in ("max", "min"):
        return Out(torch.maximum(a, b) if op == "max" else torch.minimum(a, b))
    if op in ("sum", "sub"):
        return Out(a + b if op == "sum" else a - b, a.abs() + b.abs(), sites=sites)
    if op == "prod":
        return Out(a * b, (a * b).abs(), sites=sites)
    if op == "div":
        return Out(a / b, (a / b).abs(), sites=sites)
    r = a ** b   # pow: the argument b * ln a is rounded in fp32: U32 * |b ln a| relative on the result
    return Out(r, r.abs(), amp=U32 * (b * a.log()).abs() * torch.ones_like(r), sites=sites)


def _ew_cond(op):
    def cond(x):
        if op == "div":
            assert x["b"].abs().min() >= 0.25
        if op == "pow":
            assert 0.25 <= x["a"].min() and x["a"].max() <= 4 and x["b"].abs().max() <= 2
    return cond


def _ew_nhwc(op, C, H, W, B, wrap="plain", max_batch=None, tag=""):
    ga, gb = EW_GEN[op]

    def build(net, t):
        a, b = nhwc(net, t["a"]), nhwc(net, t["b"])
        if wrap == "slice":
            a = net.out(net.slice_channels(a, 4, C, (C + 4, H, W)))
        y = net.out(net.elementwise(a, b, op))
        if wrap == "concat":
            y = net.out(net.concat([select_conv(net, nhwc(net, t["z"]), 8, NEIGHBOUR), y]))
        return {"y": y}

    def ref(x):
        o = _ew_ref(op, x["a"][:, 4:] if wrap == "slice" else x["a"], x["b"], 1)
        if wrap == "concat":
            o.ch = slice(12, None)
            return {"y": [Out(x["z"][:, NEIGHBOUR], ch=slice(0, 12)), o]}
        return {"y": o}
    inputs = {"a": ((C + 4 if wrap == "slice" else C, H, W), ga), "b": ((C, H, W), gb)}
    if wrap == "concat":
        inputs["z"] = ((8, H, W), "n")
    inst = _inst("ew_nhwc", C) if wrap == "plain" else ("ew_nhwc", "x4" if C % 4 == 0 else "x1", "x1")
    add(name=f"ew_nhwc_{op}_c{C}_{H}x{W}_b{B}{tag}", family="ew_nhwc", inputs=inputs, build=build, ref=ref, kinds={"ew_nhwc"} | ({"conv"} if wrap == "concat" else set()),
        absent={"ew_lin"}, inst=inst, batch=B, max_batch=max_batch, cond=_ew_cond(op))


for op in EW_GEN:
    for C, H, W, B in ((5, 13, 17, 3), (8, 1, 9, 1), (12, 13, 17, 1), (72, 1, 1, 3), (16, 13, 17, 1)):
        _ew_nhwc(op, C, H, W, B)
for wrap in ("slice", "concat"):
    for C in (8, 12):
        for op in ("sum", "div"):
            _ew_nhwc(op, C, 13, 17, 3, wrap=wrap, tag="_" + wrap)
_ew_nhwc("sub", 12, 13, 17, 1, max_batch=3, tag="_of3")
_ew_nhwc("prod", *BIG_SCALAR, tag="_big")
_ew_nhwc("sum", *BIG_VECTOR, tag="_big")


def _bshape(a, b):
    return tuple(max(p, q) for p, q in zip(a, b))


def _ew_lin(op, da, db, B=2, const_b=False, max_batch=None, tag=""):
    ga, gb = EW_GEN[op]
    cval = GEN[gb](np.random.default_rng(zlib.crc32(repr((op, da, db)).encode())), db) if const_b else None

    def build(net, t):
        b = net.out(net.constant(cval)) if const_b else t["b"]
        return {"y": net.out(net.elementwise(t["a"], b, op))}

    def ref(x):
        b = torch.from_numpy(cval).double().unsqueeze(0) if const_b else x["b"]
        return {"y": _ew_ref(op, *torch.broadcast_tensors(x["a"], b), 0)}

    def cond(x):
        _ew_cond(op)({"a": x["a"], "b": torch.from_numpy(cval).double() if const_b else x["b"]})
    inputs = {"a": (da, ga)} if const_b else {"a": (da, ga), "b": (db, gb)}
    dims = lambda d: "x".join(map(str, d))  # noqa: E731
    add(name=f"ew_lin_{op}_{dims(da)}_{'const' if const_b else 'by'}_{dims(db)}_b{B}{tag}", family="ew_lin", inputs=inputs, build=build, ref=ref, kinds={"ew_lin"},
        absent={"ew_nhwc"}, half=(), batch=B, max_batch=max_batch, cond=cond)


FULL = (4, 5, 6)
for op in EW_GEN:
    _ew_lin(op, FULL, FULL)
    for pos in range(3):   # a 1 in each position of either operand
        one = tuple(1 if i == pos else d for i, d in enumerate(FULL))
        _ew_lin(op, one, FULL)
        _ew_lin(op, FULL, one)
    _ew_lin(op, (4, 1, 6), (1, 5, 1))       # both operands broadcast, in different positions
    _ew_lin(op, (1, 5, 1), (4, 1, 6))
    _ew_lin(op, FULL, FULL, const_b=True, B=3)        # a constant (unbatched) operand in an implicit-batch plan
    _ew_lin(op, FULL, (1, 5, 1), const_b=True, B=3)
_ew_lin("sub", (3, 7), (3, 1), B=3)
_ew_lin("div", (2, 3, 4, 5), (2, 1, 4, 1), B=1)
_ew_lin("sum", FULL, (1, 5, 1), B=1, max_batch=3, tag="_of3")
_ew_lin("sub", FULL, (1, 5, 1), const_b=True, B=1, max_batch=3, tag="_of3")
_ew_lin("prod", (12, 128, 128), (12, 1, 128), B=3, tag="_big")


# ---- 5. activation: relu exact; the others |ref| relative, one fp16 store on the NHWC path (1 site), none on the LINEAR one ------------------
def _act_ref(kind, alpha, x, sites):
    if kind == "relu":
        return Out(torch.relu(x))
    r = {"sigmoid": torch.sigmoid, "tanh": torch.tanh, "leaky": lambda v: F.leaky_relu(v, alpha)}[kind](x)
    return Out(r, r.abs(), sites=sites)


ACTS = [("relu", None), ("sigmoid", None), ("tanh", None), ("leaky", 0.1), ("leaky", 0.3)]
for kind, alpha in ACTS:
    tag = kind + ("%g" % alpha if alpha else "")

    def op(net, t, chw, kind=kind, alpha=alpha):
        return net.out(net.activation(t, kind, alpha))

    def opref(x, kind=kind, alpha=alpha):
        return _act_ref(kind, alpha, x, 1)
    for C, H, W, B in SHAPES:
        unary_nhwc(f"act_nhwc_{tag}_c{C}_{H}x{W}_b{B}", "act_nhwc", C, H, W, B, op, opref, "act_nhwc", gen="special", via_pool=True, kinds={"act_nhwc", "pool"},
                   absent={"act_lin"})
    for wrap in ("slice", "concat"):
        for C in (8, 12):
            unary_nhwc(f"act_nhwc_{tag}_c{C}_13x17_b3_{wrap}", "act_nhwc", C, 13, 17, 3, op, opref, "act_nhwc", gen="special", via_pool=True, wrap=wrap,
                       kinds={"act_nhwc", "pool"}, absent={"act_lin"})
    unary_nhwc(f"act_nhwc_{tag}_c12_13x17_b1_of3", "act_nhwc", 12, 13, 17, 1, op, opref, "act_nhwc", gen="special", via_pool=True, max_batch=3,
               kinds={"act_nhwc", "pool"})
    for dims, B in (((5, 13, 17), 3), ((7,), 1), ((3, 4, 5, 6), 2), ((12, 1, 9), 1)):
        def build(net, t, kind=kind, alpha=alpha):
            return {"y": net.out(net.activation(t["x"], kind, alpha))}

        def ref(x, kind=kind, alpha=alpha):
            return {"y": _act_ref(kind, alpha, x["x"], 0)}
        add(name=f"act_lin_{tag}_{'x'.join(map(str, dims))}_b{B}", family="act_lin", inputs={"x": (dims, "special")}, build=build, ref=ref, kinds={"act_lin"},
            absent={"act_nhwc"}, half=(), batch=B)
    add(name=f"act_lin_{tag}_5x13x17_b1_of3", family="act_lin", inputs={"x": ((5, 13, 17), "special")}, build=build, ref=ref, kinds={"act_lin"}, half=(), batch=1,
        max_batch=3)


def _act_big(kind, alpha, shape):
    C, H, W, B = shape

    def op(net, t, chw):
        return net.out(net.activation(t, kind, alpha))
    unary_nhwc(f"act_nhwc_{kind}_c{C}_{H}x{W}_b{B}_big", "act_nhwc", C, H, W, B, op, lambda x: _act_ref(kind, alpha, x, 1), "act_nhwc", gen="special", via_pool=True,
               kinds={"act_nhwc", "pool"})


_act_big("tanh", None, BIG_SCALAR)
_act_big("leaky", 0.1, BIG_VECTOR)
add(name="act_lin_sigmoid_12x128x128_b3_big", family="act_lin", inputs={"x": ((12, 128, 128), "special")}, build=lambda net, t: {"y": net.out(net.activation(t["x"], "sigmoid"))},
    ref=lambda x: {"y": _act_ref("sigmoid", None, x["x"], 0)}, kinds={"act_lin"}, half=(), batch=3)


# ---- 6. scale: x * scale + shift (2 terms, 1 site on the NHWC path); with a power, LINEAR fp32 on a positive base ---------------------------------
def _scale_w(name, C, power):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if power:   # positive base, no cancellation: base in [0.125, 9]
        return rng.uniform(0.0, 1.0, C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32), np.where(rng.random(C) < 0.5, rng.uniform(-2, 0.75, C), rng.uniform(1.25, 2, C)).astype(np.float32)
    return rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32), None


def _scale_ref(x, sh, sc, pw, caxis, sites):
    shape = [1] * x.dim()
    if len(sh) > 1:
        shape[caxis] = len(sh)
    shd, scd = torch.from_numpy(sh).double().reshape(shape), torch.from_numpy(sc).double().reshape(shape)
    base = x * scd + shd
    mag = x.abs() * scd.abs() + shd.abs()
    if pw is None:
        return Out(base, mag, n=2, sites=sites)
    p = torch.from_numpy(pw).double().reshape(shape)
    r = base ** p   # the base carries two fp32 roundings (relative: no cancellation), amplified |p| times; the argument p * ln(base) one more
    return Out(r, r.abs(), amp=U32 * (2 * p.abs() + (p * base.log()).abs()) * torch.ones_like(r), sites=sites)


def _scale_nhwc(C, H, W, B, uniform, **kw):
    tag = kw.pop("tag", "")
    name = f"scale_nhwc_{'uniform' if uniform else 'channel'}_c{C}_{H}x{W}_b{B}{tag}"
    sh, sc, _ = _scale_w(name, 1 if uniform else C, False)

    def op(net, t, chw):
        return net.out(net.scale_uniform(t, float(sc[0]), float(sh[0])) if uniform else net.scale(t, sh, sc))
    unary_nhwc(name, "scale_nhwc", C, H, W, B, op, lambda x: _scale_ref(x, sh, sc, None, 1, 1), "scale_nhwc", via_pool=True, kinds={"scale_nhwc", "pool"},
               absent={"scale_lin"}, **kw)


for C, H, W, B in SHAPES:
    _scale_nhwc(C, H, W, B, False)
    _scale_nhwc(C, H, W, B, True)
for wrap in ("slice", "concat"):
    for C in (8, 12):
        _scale_nhwc(C, 13, 17, 3, False, wrap=wrap, tag="_" + wrap)
_scale_nhwc(12, 13, 17, 1, False, max_batch=3, tag="_of3")
_scale_nhwc(*BIG_SCALAR, False, tag="_big")
_scale_nhwc(*BIG_VECTOR, True, tag="_big")


def _scale_lin(dims, B, uniform, spatial=False, power=True, max_batch=None, tag=""):
    name = f"scale_lin_{'uniform' if uniform else 'channel'}_{'x'.join(map(str, dims))}_b{B}{'_spatial' if spatial else ''}{'' if power else '_p1'}{tag}"
    caxis = max(len(dims) - 3, 0)
    sh, sc, pw = _scale_w(name, 1 if uniform else dims[caxis], power)

    def build(net, t):
        x = nhwc(net, t["x"]) if spatial else t["x"]   # a spatial (NHWC) tensor with power != 1 must leave NHWC and take scale_lin
        if uniform:
            return {"y": net.out(net.scale_uniform(x, float(sc[0]), float(sh[0]), 1.0 if pw is None else float(pw[0])))}
        return {"y": net.out(net.scale(x, sh, sc, pw))}

    def cond(x):
        if power:
            assert x["x"].min() >= 0.25 and x["x"].max() <= 4 and np.abs(pw).max() <= 2
    add(name=name, family="scale_lin", inputs={"x": (dims, "pos" if power else "n")}, build=build, ref=lambda x: {"y": _scale_ref(x["x"], sh, sc, pw, caxis + 1, 0)},
        kinds={"scale_lin"} | ({"pool", "to_linear"} if spatial else set()), absent={"scale_nhwc"}, half="all" if spatial else (), batch=B, max_batch=max_batch, cond=cond)


for dims, B in (((5, 13, 17), 3), ((8, 1, 9), 1), ((12, 13, 17), 1), ((3, 4, 5, 6), 2)):
    _scale_lin(dims, B, False)
    _scale_lin(dims, B, True)
    if len(dims) == 3:
        _scale_lin(dims, B, False, spatial=True)
        _scale_lin(dims, B, True, spatial=True)
_scale_lin((6, 7), 3, True)
_scale_lin((6, 7), 3, True, power=False)
_scale_lin((5, 13, 17), 1, False, max_batch=3, tag="_of3")
_scale_lin((12, 128, 128), 3, False, tag="_big")


# ---- 7. reduce -----------------------------------------------------------------------------------------------------------------------------
# NHWC average over HW: four partial sums of at most HW / 4 terms and their sum (n = HW bounds it), one division, one fp16 store (1 site).
for C, H, W, B in ((5, 1, 1, 3), (5, 1, 3, 1), (5, 7, 7, 3), (5, 13, 17, 1), (64, 1, 1, 1), (64, 1, 3, 3), (64, 7, 7, 1), (64, 13, 17, 3), (72, 1, 1, 3), (72, 1, 3, 1),
                   (72, 7, 7, 3), (72, 13, 17, 1), (2048, 1, 1, 1), (2048, 1, 3, 1), (2048, 7, 7, 3), (2048, 13, 17, 1), (12, 7, 7, 3), (20, 13, 17, 1)):
    def op(net, t, chw):
        return net.out(net.reduce(t, "avg", 0b110, True))

    def opref(x, hw=H * W):
        return Out(x.mean((2, 3), keepdim=True), x.abs().mean((2, 3), keepdim=True), n=hw, sites=1)
    unary_nhwc(f"reduce_hw_c{C}_{H}x{W}_b{B}", "reduce_hw", C, H, W, B, op, opref, "reduce_hw", via_pool=True, kinds={"reduce_hw", "pool"}, absent={"reduce_lin"},
               out_hw=(1, 1), inst=("reduce_hw", "x1", "x8" if C % 8 == 0 else "x1"))
    if (C, H, W) in ((64, 7, 7), (12, 7, 7)):
        for wrap in ("slice", "concat"):
            unary_nhwc(f"reduce_hw_c{C}_{H}x{W}_b{B}_{wrap}", "reduce_hw", C, H, W, B, op, opref, "reduce_hw", via_pool=True, kinds={"reduce_hw", "pool"}, wrap=wrap,
                       out_hw=(1, 1), inst=("reduce_hw", "x1", "x1"))
    if (C, H, W) == (72, 7, 7):
        unary_nhwc(f"reduce_hw_c{C}_{H}x{W}_b1_of3", "reduce_hw", C, H, W, 1, op, opref, "reduce_hw", via_pool=True, kinds={"reduce_hw", "pool"}, max_batch=3,
                   out_hw=(1, 1), inst=("reduce_hw", "x1", "x8"))


def _reduce_lin(dims, B, op, axes, keep, gen="n", max_batch=None, tag=""):
    ax = [i + 1 for i in range(len(dims)) if (axes >> i) & 1]
    n = int(np.prod([dims[i - 1] for i in ax]))

    def ref(x):
        v = x["x"]
        if op == "max":
            return {"y": Out(v.amax(ax, keepdim=bool(keep)))}
        if op == "sum":
            return {"y": Out(v.sum(ax, keepdim=bool(keep)), v.abs().sum(ax, keepdim=bool(keep)), n=n)}
        return {"y": Out(v.mean(ax, keepdim=bool(keep)), v.abs().mean(ax, keepdim=bool(keep)), n=n)}
    add(name=f"reduce_lin_{op}_{'x'.join(map(str, dims))}_axes{axes:b}_keep{keep}_b{B}{tag}", family="reduce_lin", inputs={"x": (dims, gen)},
        build=lambda net, t: {"y": net.out(net.reduce(t["x"], op, axes, keep))}, ref=ref, kinds={"reduce_lin"}, absent={"reduce_hw"}, half=(), batch=B,
        max_batch=max_batch)


for op in ("sum", "avg", "max"):
    for keep in (0, 1):
        for axes in (0b0001, 0b0010, 0b1000, 0b0110, 0b1100, 0b0011):   # first, middle, last, contiguous runs
            _reduce_lin((4, 5, 6, 7), 2, op, axes, keep)
        _reduce_lin((5, 7, 9), 3, op, 0b110, keep)   # the HW average of a LINEAR tensor
        _reduce_lin((33,), 1, op, 0b1, keep)
_reduce_lin((4, 5, 6, 7), 2, "max", 0b0110, 0, gen="neg", tag="_neg")
_reduce_lin((4, 5, 6, 7), 2, "max", 0b1000, 1, gen="neg", tag="_neg")
_reduce_lin((4, 5, 6, 7), 1, "sum", 0b0010, 0, max_batch=3, tag="_of3")
_reduce_lin((2, 450, 450), 3, "avg", 0b001, 0, tag="_big")


# ---- 8. softmax: LINEAR fp32.  |ref| relative; n = the axis length (the kernel's sequential sum); the subtraction logit - rowmax is rounded
#         once, which the exponential turns into U32 * |logit - rowmax| relative ----------------------------------------------------------------
def _softmax(dims, B, ax, gen="logits", max_batch=None, tag=""):
    def ref(x):
        v = x["x"]
        r = v.softmax(ax + 1)
        spread = (v - v.amax(ax + 1, keepdim=True)).abs()
        return {"y": Out(r, r, n=dims[ax], amp=U32 * spread)}

    def cond(x):
        assert x["x"].abs().max() <= 80
    add(name=f"softmax_{'x'.join(map(str, dims))}_ax{ax}_{gen}_b{B}{tag}", family="softmax", inputs={"x": (dims, gen)},
        build=lambda net, t: {"y": net.out(net.softmax(t["x"], 1 << ax))}, ref=ref, kinds={"softmax"}, half=(), batch=B, max_batch=max_batch, cond=cond)


for dims in ((16, 5), (2, 80), (1, 7), (2, 80, 3), (16, 1, 2), (3, 1, 5), (2, 3, 16, 2), (80, 2, 1, 3)):   # every axis position of rank 2-4
    for ax in range(len(dims)):
        _softmax(dims, 2, ax)
_softmax((8400, 3), 1, 0)              # the longest axis: inner extent 3 ...
_softmax((3, 8400), 2, 1)              # ... and 1
_softmax((4, 8400), 1, 1, gen="logits80")
for gen in ("logits80", "equal"):
    _softmax((16, 5), 3, 0, gen=gen)
    _softmax((6, 80), 3, 1, gen=gen)
    _softmax((2, 16, 3), 1, 1, gen=gen)
_softmax((6, 80), 1, 1, max_batch=3, tag="_of3")
_softmax((2, 450, 450), 3, 0, tag="_big")


# ---- 9. matmul (LINEAR fp32: K terms) and fully connected ---------------------------------------------------------------------------------------
def _mm_ref(a, b, ta, tb):
    a = a.transpose(-1, -2) if ta else a
    b = b.transpose(-1, -2) if tb else b
    return Out(a @ b, a.abs() @ b.abs(), n=a.shape[-1])


def _matmul(M, N, K, ta, tb, B=2, const_b=False, max_batch=None, tag=""):
    da, db = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    cval = np.random.default_rng(M * 1000 + N * 10 + K).standard_normal(db).astype(np.float32) if const_b else None

    def build(net, t):
        return {"y": net.out(net.matmul(t["a"], net.out(net.constant(cval)) if const_b else t["b"], ta, tb))}

    def ref(x):
        return {"y": _mm_ref(x["a"], torch.from_numpy(cval).double() if const_b else x["b"], ta, tb)}
    add(name=f"matmul_m{M}_n{N}_k{K}_t{int(ta)}{int(tb)}{'_const' if const_b else ''}_b{B}{tag}", family="matmul",
        inputs={"a": (da, "n")} if const_b else {"a": (da, "n"), "b": (db, "n")}, build=build, ref=ref, kinds={"matmul"}, half=(), batch=B, max_batch=max_batch)


for ta, tb in itertools.product((False, True), repeat=2):
    for M, N, K in ((1, 1, 1), (5, 7, 33), (33, 5, 7), (7, 33, 5), (1, 33, 7), (33, 1, 1), (7, 7, 1), (5, 1, 33)):
        _matmul(M, N, K, ta, tb)
    _matmul(5, 7, 33, ta, tb, B=3, const_b=True)     # a constant right operand in an implicit-batch plan
    _matmul(33, 5, 7, ta, tb, B=1, const_b=True, max_batch=3, tag="_of3")
_matmul(5, 7, 33, False, True, B=1, max_batch=3, tag="_of3")
_matmul(420, 420, 5, True, False, B=3, tag="_big")


def _matmul_lead(da, db, ta=False, tb=False):
    def build(net, t):
        return {"y": net.out(net.matmul(t["a"], t["b"], ta, tb))}
    add(name=f"matmul_lead_{'x'.join(map(str, da))}_by_{'x'.join(map(str, db))}_t{int(ta)}{int(tb)}", family="matmul", inputs={"a": (da, "n"), "b": (db, "n")}, build=build,
        ref=lambda x: {"y": _mm_ref(x["a"], x["b"], ta, tb)}, kinds={"matmul"}, half=(), explicit=True)


_matmul_lead((2, 1, 5, 7), (1, 3, 7, 4))              # both operands broadcast
_matmul_lead((1, 3, 5, 7), (2, 1, 7, 4))
_matmul_lead((2, 3, 5, 7), (2, 3, 7, 4))              # a merged pair of leading dims
_matmul_lead((2, 3, 5, 7), (1, 1, 7, 4))
_matmul_lead((1, 1, 5, 7), (2, 3, 7, 4))
_matmul_lead((2, 3, 7, 5), (2, 1, 4, 7), True, True)
_matmul_lead((3, 5, 7), (1, 7, 4))
_matmul_lead((2, 3, 2, 5, 7), (2, 3, 2, 7, 4))
_matmul_lead((2, 3, 2, 5, 7), (1, 1, 2, 7, 4))


def _fc(C, H, W, nb, bias, B=3):
    rng = np.random.default_rng(C * 100 + H * 10 + nb)
    w = (rng.standard_normal((nb, C * H * W)) / math.sqrt(C * H * W)).astype(np.float32)
    b = rng.standard_normal(nb).astype(np.float32) if bias else None

    def ref(x):   # an fp16 plan may run it on the MFMA path: fp16 weights (1 site) and the fp16 store of the result (1 site)
        wd = torch.from_numpy(w).double()
        bd = torch.from_numpy(b).double() if bias else torch.zeros(nb, dtype=torch.float64)
        v = x["x"].flatten(1)
        return {"y": Out((v @ wd.T + bd).reshape(-1, nb, 1, 1), (v.abs() @ wd.abs().T + bd.abs()).reshape(-1, nb, 1, 1), n=C * H * W + 1, sites=2)}
    add(name=f"fc_c{C}_{H}x{W}_to{nb}_{'bias' if bias else 'nobias'}_b{B}", family="fc", inputs={"x": ((C, H, W), "n")},
        build=lambda net, t: {"y": net.out(net.fully_connected(t["x"], w, b))}, ref=ref, kinds={"conv"}, batch=B)


for bias in (True, False):
    _fc(5, 3, 3, 7, bias)
    _fc(33, 1, 1, 5, bias)
    _fc(1, 1, 7, 1, bias)
    _fc(16, 4, 4, 33, bias)


# ---- 10. direct convolution: fp32 weights in both engines (pack.cpp packs them with pack_conv_weights_f32), kh * kw * Cin / groups terms
#          + bias + shortcut, one fp16 store of the fused result (1 site) -----------------------------------------------------------------------
def _conv(name, Cin, Cout, H, W, k, stride=1, padding=0, dilation=1, groups=1, fusedep=False, B=2, max_batch=None, wrap="plain"):
    kh, kw_ = (k, k) if np.isscalar(k) else k
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    w = (rng.standard_normal((Cout, Cin // groups, kh, kw_)) / math.sqrt(kh * kw_ * Cin / groups)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32) if fusedep else None
    wd, bd = torch.from_numpy(w).double(), (torch.from_numpy(b).double() if fusedep else None)
    conv = lambda x, ww, bb: F.conv2d(x, ww, bb, stride, padding, dilation, groups)  # noqa: E731
    Ho, Wo = conv(torch.zeros(1, Cin, H, W, dtype=torch.float64), wd, None).shape[2:]

    def build(net, t):
        x = nhwc(net, t["x"])   # (a 3-channel network input would otherwise take the stem kernel)
        if wrap == "slice":
            x = net.out(net.slice_channels(x, 4, Cin, (Cin + 4, H, W)))
        y = net.out(net.conv(x, w, b, stride, padding, groups=groups, dilation=dilation))
        if fusedep:
            y = net.out(net.activation(y, "leaky", 0.1))
            y = net.out(net.elementwise(y, nhwc(net, t["r"]), "sum"))
            y = net.out(net.activation(y, "relu"))
        if wrap == "concat":
            y = net.out(net.concat([select_conv(net, nhwc(net, t["z"]), 8, NEIGHBOUR), y]))
        return {"y": y}

    def ref(x):
        v = x["x"][:, 4:] if wrap == "slice" else x["x"]
        r, mag = conv(v, wd, bd), conv(v.abs(), wd.abs(), bd.abs() if fusedep else None)
        if fusedep:
            r, mag = torch.relu(F.leaky_relu(r, 0.1) + x["r"]), mag + x["r"].abs()
        o = Out(r, mag, n=kh * kw_ * Cin // groups + 2, sites=1)
        if wrap == "concat":
            o.ch = slice(12, None)
            return {"y": [Out(x["z"][:, NEIGHBOUR], ch=slice(0, 12)), o]}
        return {"y": o}
    inputs = {"x": ((Cin + 4 if wrap == "slice" else Cin, H, W), "n")}
    if fusedep:
        inputs["r"] = ((Cout, Ho, Wo), "n")
    if wrap == "concat":
        inputs["z"] = ((8, Ho, Wo), "n")
    add(name=name, family="conv_direct", inputs=inputs, build=build, ref=ref, kinds={"conv", "pool"}, absent={"ew_nhwc", "act_nhwc"}, batch=B, max_batch=max_batch,
        direct=wrap != "concat", fused=None if wrap == "concat" else dict(act1=4 if fusedep else 0, act2=1 if fusedep else 0, residual=fusedep))


CONVS = [dict(tag="g2", Cin=6, Cout=10, k=3, padding=1, groups=2), dict(tag="g4", Cin=16, Cout=32, k=3, padding=1, groups=4),
         dict(tag="dm2", Cin=3, Cout=6, k=3, padding=1, groups=3), dict(tag="dil2", Cin=3, Cout=5, k=3, padding=2, dilation=2),
         dict(tag="dil2x1_g2", Cin=6, Cout=4, k=3, padding=(2, 1), dilation=(2, 1), groups=2), dict(tag="k1x3", Cin=6, Cout=5, k=(1, 3), padding=(0, 1)),
         dict(tag="k3x1", Cin=3, Cout=5, k=(3, 1), padding=(1, 0)), dict(tag="k1x7_s2x1_g2", Cin=6, Cout=10, k=(1, 7), stride=(2, 1), padding=(0, 3), groups=2),
         dict(tag="k7x1_s1x2", Cin=3, Cout=5, k=(7, 1), stride=(1, 2), padding=(3, 0)), dict(tag="k3_s2", Cin=6, Cout=5, k=3, stride=2, padding=1)]
for cfg in CONVS:
    cfg = dict(cfg)
    tag = cfg.pop("tag")
    for fusedep in (False, True):
        for H, W in ((13, 17), (1, 9)):
            _conv(f"conv_{tag}_{H}x{W}{'_fused' if fusedep else ''}", H=H, W=W, fusedep=fusedep, **cfg)
_conv("conv_g2_13x17_slice", 6, 10, 13, 17, 3, padding=1, groups=2, wrap="slice")
_conv("conv_g2_13x17_concat", 6, 10, 13, 17, 3, padding=1, groups=2, wrap="concat")
_conv("conv_g2_13x17_fused_b1_of3", 6, 10, 13, 17, 3, padding=1, groups=2, fusedep=True, B=1, max_batch=3)
_conv("conv_g2_128x128_big", 6, 12, 128, 128, 3, padding=1, groups=2, B=3)


# ---- 10b. the MFMA convolutions at engine level: implicit GEMM (kernels/igemm_tile.h; `igemm: true` in the fp16 AND the fp32 plan) and the stem
#           kernels (conv_stem.hip / conv_stem_f32.hip; `stem: true`) on rectangular, strided and padded geometry.  An fp16 plan packs fp16 weights
#           (the stem converts them when it loads them): the reference multiplies w.half() there.  kh * kw * Cin products + bias + shortcut; one fp16
#           store, two with a shortcut (the MFMA epilogue rounds to fp16 in front of the add, and the sum again).  The operation-level table is
#           tests/conv_cases.py; here the same kernels meet what only a plan produces: zero-padded channels of a freshly converted tensor, channel
#           slices, a concat neighbour, an enqueue below max_batch, the fused epilogue chain ----------------------------------------------------------
def _mfma(name, Cin, Cout, H, W, k, stride=1, padding=0, fusedep=False, B=2, max_batch=None, wrap="plain", stem=False):
    kh, kw_ = (k, k) if np.isscalar(k) else k
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    w = (rng.standard_normal((Cout, Cin, kh, kw_)) / math.sqrt(kh * kw_ * Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32) if fusedep or stem else None
    conv = lambda x, ww, bb: F.conv2d(x, ww, bb, stride, padding)  # noqa: E731
    Ho, Wo = conv(torch.zeros(1, Cin, H, W, dtype=torch.float64), torch.zeros(Cout, Cin, kh, kw_, dtype=torch.float64), None).shape[2:]

    def build(net, t):
        x = t["x"]
        if wrap == "slice":     # channels [8, 8 + Cin) of a wider NHWC tensor: an aligned view in both plans
            x = net.out(net.slice_channels(nhwc(net, x), 8, Cin, (Cin + 8, H, W)))
        elif wrap not in ("fresh", "stem"):
            x = nhwc(net, x)    # ("fresh": the conv reads the converted network input itself, Cin padded with zeros to the vector width)
        z = select_conv(net, nhwc(net, t["z"]), 8, NEIGHBOUR) if wrap == "concat" else None   # (the helper convolution first)
        y = net.out(net.conv(x, w, b, stride, padding))
        if fusedep:
            y = net.out(net.activation(y, "leaky", 0.1))
            y = net.out(net.elementwise(y, nhwc(net, t["r"]), "sum"))
            y = net.out(net.activation(y, "relu"))
        elif stem:
            y = net.out(net.activation(y, "relu"))
        if wrap == "concat":
            y = net.out(net.concat([z, y]))
        return {"y": y}

    def ref(x, fp16):
        wd = torch.from_numpy(w)
        wd = (wd.half() if fp16 else wd).double()
        bd = None if b is None else torch.from_numpy(b).double()
        v = x["x"][:, 8:] if wrap == "slice" else x["x"]
        r, mag = conv(v, wd, bd), conv(v.abs(), wd.abs(), None if bd is None else bd.abs())
        if fusedep:
            r, mag = torch.relu(F.leaky_relu(r, 0.1) + x["r"]), mag + x["r"].abs()
        elif stem:
            r = torch.relu(r)
        o = Out(r, mag, n=kh * kw_ * Cin + 2, sites=2 if fusedep else 1)
        if wrap == "concat":
            o.ch = slice(12, None)
            return {"y": [Out(x["z"][:, NEIGHBOUR], ch=slice(0, 12)), o]}
        return {"y": o}
    inputs = {"x": ((Cin + 8 if wrap == "slice" else Cin, H, W), "n")}
    if fusedep:
        inputs["r"] = ((Cout, Ho, Wo), "n")
    if wrap == "concat":
        inputs["z"] = ((8, Ho, Wo), "n")
    add(name=name, family="conv_mfma", inputs=inputs, build=build, ref=ref, kinds={"conv"}, absent={"ew_nhwc", "act_nhwc"}, batch=B, max_batch=max_batch,
        igemm=not stem, stem=stem, by_precision=True,
        fused=None if wrap == "concat" else dict(act1=4 if fusedep else (1 if stem else 0), act2=1 if fusedep else 0, residual=fusedep))


_mfma("mfma_k1x3_c16_o16_13x17", 16, 16, 13, 17, (1, 3), padding=(0, 1))                               # two taps per k-step, three taps
_mfma("mfma_k7x1_s1x2_c32_o24_13x17", 32, 24, 13, 17, (7, 1), stride=(1, 2), padding=(3, 0))
_mfma("mfma_k3x5_s2x1_p0x2_c16_o40_13x17", 16, 40, 13, 17, (3, 5), stride=(2, 1), padding=(0, 2))      # 15 taps of 16 channels: the last k-step holds one
_mfma("mfma_k5x6_c32_o16_13x17", 32, 16, 13, 17, (5, 6), padding=2)                                    # 30 taps, the limit
_mfma("mfma_k3x3_p2_c24_o16_13x17", 24, 16, 13, 17, 3, padding=2)                                      # padding beyond k / 2, a ragged channel chunk
_mfma("mfma_k1x1_s2_p1_c64_o32_13x17", 64, 32, 13, 17, 1, stride=2, padding=1)                         # a border without a valid tap; not a plain GEMM
_mfma("mfma_k2x2_s2_c16_o21_13x17", 16, 21, 13, 17, 2, stride=2)                                       # Cout 21: element-wise stores
_mfma("mfma_k3x1_c20_o16_13x17_fresh", 20, 16, 13, 17, (3, 1), padding=(1, 0), wrap="fresh")           # Cin 20 -> 24 zero-padded channels: with Cin % 8 != 0 the plan grants `igemm` only to a tensor it knows zero-padded, so the flag asserts that path
_mfma("mfma_k1x7_p0x3_c16_o16_13x17_slice", 16, 16, 13, 17, (1, 7), padding=(0, 3), wrap="slice")      # reads a channel slice (ld_in 24)
_mfma("mfma_k3x5_p1x2_c16_o16_13x17_concat", 16, 16, 13, 17, (3, 5), padding=(1, 2), wrap="concat")    # writes behind the 12-channel neighbour
_mfma("mfma_k5x3_s2x1_c32_o16_13x17_b1_of3", 32, 16, 13, 17, (5, 3), stride=(2, 1), padding=(2, 1), B=1, max_batch=3)
_mfma("mfma_k3x5_s1x2_c32_o32_13x17_fused", 32, 32, 13, 17, (3, 5), stride=(1, 2), padding=(1, 2), fusedep=True)   # bias, leaky, shortcut, relu
_mfma("mfma_k1x3_c16_o16_1x9", 16, 16, 1, 9, (1, 3), padding=(0, 1), B=3)                              # a single row
_mfma("stem_k3x5_s2x1_p0x2_c3_o16_13x17", 3, 16, 13, 17, (3, 5), stride=(2, 1), padding=(0, 2), wrap="stem", stem=True)
_mfma("stem_k7x3_p0_c3_o32_13x17", 3, 32, 13, 17, (7, 3), wrap="stem", stem=True)
_mfma("mfma_k3x5_p1x2_c16_o16_128x128_big", 16, 16, 128, 128, (3, 5), padding=(1, 2), B=3)             # 384 row tiles


# ---- 11. direct transposed convolution: fp32 weights (pack_deconv_weights_f32), at most kh * kw * Cin / groups terms + bias, one fp16 store --------
def _deconv(name, Cin, Cout, H, W, k, stride, padding=0, dilation=1, groups=1, bias=True, B=2, max_batch=None, w=None, kinds={"deconv"}, absent={"resize"},
            exact=False, bvec=None, wrap="plain"):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if w is None:
        w = (rng.standard_normal((Cin, Cout // groups, k, k)) / math.sqrt(k * k * Cin / groups)).astype(np.float32)
    b = bvec if bvec is not None else (rng.standard_normal(Cout).astype(np.float32) if bias else None)
    wd, bd = torch.from_numpy(w).double(), (None if b is None else torch.from_numpy(b).double())
    dc = lambda x, ww, bb: F.conv_transpose2d(x, ww, bb, stride, padding, 0, groups, dilation)  # noqa: E731

    Ho, Wo = dc(torch.zeros(1, Cin, H, W, dtype=torch.float64), wd, None).shape[2:]

    def build(net, t):
        x = t["x"]
        if wrap == "slice":   # channels [4, 4 + Cin) of a wider NHWC tensor: ld_in != Cin
            x = net.out(net.slice_channels(nhwc(net, x), 4, Cin, (Cin + 4, H, W)))
        y = net.out(net.conv(x, w, b, stride, padding, True, groups, dilation))
        if wrap == "concat":  # next to the 12-channel convolution: ld_out != Cout
            y = net.out(net.concat([select_conv(net, nhwc(net, t["z"]), 8, NEIGHBOUR), y]))
        return {"y": y}

    def ref(x):
        v = x["x"][:, 4:] if wrap == "slice" else x["x"]
        o = Out(dc(v, wd, bd)) if exact else Out(dc(v, wd, bd), dc(v.abs(), wd.abs(), None if bd is None else bd.abs()), n=k * k * Cin // groups + 1, sites=1)
        if wrap == "concat":
            o.ch = slice(12, None)
            return {"y": [Out(x["z"][:, NEIGHBOUR], ch=slice(0, 12)), o]}
        return {"y": o}
    inputs = {"x": ((Cin + 4 if wrap == "slice" else Cin, H, W), "n")}
    if wrap == "concat":
        inputs["z"] = ((8, Ho, Wo), "n")
    add(name=name, family="deconv", inputs=inputs, build=build, ref=ref, kinds=set(kinds) | ({"conv"} if wrap == "concat" else set()) if not isinstance(kinds, tuple) else kinds,
        absent=absent, batch=B, max_batch=max_batch, direct="deconv" in kinds and wrap != "concat")


for tag, kw in (("k4s2p1", dict(k=4, stride=2, padding=1)), ("k3s2p1", dict(k=3, stride=2, padding=1)), ("k3s1p1", dict(k=3, stride=1, padding=1)),
                ("k3s1p2d2", dict(k=3, stride=1, padding=2, dilation=2)), ("k3s2p0d2", dict(k=3, stride=2, padding=0, dilation=2)), ("k2s3p0", dict(k=2, stride=3))):
    for gtag, Cin, Cout, g in (("g1", 5, 7, 1), ("g2", 6, 4, 2), ("g4", 8, 12, 4), ("dw", 5, 5, 5)):
        for H, W in ((5, 7), (1, 9)):
            _deconv(f"deconv_{tag}_{gtag}_{H}x{W}", Cin, Cout, H, W, groups=g, **kw)
for wrap in ("slice", "concat"):
    _deconv(f"deconv_k4s2p1_g2_5x7_{wrap}", 6, 4, 5, 7, 4, 2, 1, groups=2, wrap=wrap, B=3)
    _deconv(f"deconv_k3s1p1_g1_13x17_{wrap}", 5, 7, 13, 17, 3, 1, 1, wrap=wrap, B=1)
_deconv("deconv_k4s2p1_g2_13x17_nobias_b1_of3", 6, 4, 13, 17, 4, 2, 1, groups=2, bias=False, B=1, max_batch=3)
_deconv("deconv_k4s2p1_g2_64x64_big", 6, 12, 64, 64, 4, 2, 1, groups=2, B=3)
for C in (5, 8):   # the all-ones depthwise kernel == stride form is a nearest upsample: must become `resize` and be exact; its near misses must not
    ones = np.ones((C, 1, 2, 2), np.float32)
    _deconv(f"deconv_ones_c{C}_is_resize", C, C, 5, 7, 2, 2, groups=C, bias=False, w=ones, kinds={"resize"}, absent={"deconv"}, exact=True)
    half = ones.copy()
    half[C - 2, 0, 1, 0] = 0.5
    _deconv(f"deconv_ones_c{C}_one_weight_half", C, C, 5, 7, 2, 2, groups=C, bias=False, w=half)
    bv = np.zeros(C, np.float32)
    bv[1] = 0.25
    _deconv(f"deconv_ones_c{C}_bias", C, C, 5, 7, 2, 2, groups=C, w=ones, bvec=bv)


def _d2s(Cin, Cout, s, H, W, B):
    """kernel == stride, C and Cout multiples of 8: an fp16 plan runs a 1x1 convolution + depth_to_space.  One-hot weights: out[co, h*s + r, w*s + q] =
    in[sel(co, r, q), h, w], a copy in either plan (fp32: the direct kernel adds zeros)"""
    w = np.zeros((Cin, Cout, s, s), np.float32)
    for co, r, q in itertools.product(range(Cout), range(s), range(s)):
        w[(3 * co + 5 * r + 7 * q + 1) % Cin, co, r, q] = 1.0
    _deconv(f"deconv_d2s_c{Cin}_to{Cout}_s{s}_{H}x{W}_b{B}", Cin, Cout, H, W, s, s, bias=False, w=w, B=B, exact=True,
            kinds=({"deconv"}, {"depth_to_space", "conv"}), absent=({"resize"}, {"resize", "deconv"}))
    CASES[-1].direct = False


_d2s(8, 16, 2, 5, 7, 2)
_d2s(16, 8, 2, 13, 17, 3)
_d2s(8, 8, 3, 1, 9, 1)


# ---- 12. data movement: exact ----------------------------------------------------------------------------------------------------------------------
def _move(name, dims, build, ref, kinds, B=2, explicit=False, max_batch=None, half=(), inst=None, absent=frozenset()):
    add(name=name, family="move", inputs={"x": (dims, "n")}, build=build, ref=ref, kinds=kinds, half=half, batch=B, explicit=explicit, max_batch=max_batch, inst=inst,
        absent=absent)


# the layout conversions: to_nhwc -> 1x1 max-pool -> to_linear returns x (fp32 plans) or x.half() (fp16 plans)
for C, H, W, B in SHAPES + [(20, 13, 17, 1), (64, 7, 7, 3), (72, 1, 1, 1), (100, 3, 5, 2), (16, 33, 35, 1), (3, 13, 17, 2)]:
    _move(f"layout_c{C}_{H}x{W}_b{B}", (C, H, W), lambda net, t: {"y": nhwc(net, t["x"])}, lambda x: {"y": Out(x["x"])}, {"to_nhwc", "pool", "to_linear"}, B=B, half="all",
          inst=_inst("pool", C))
_move("layout_c12_13x17_b1_of3", (12, 13, 17), lambda net, t: {"y": nhwc(net, t["x"])}, lambda x: {"y": Out(x["x"])}, {"to_nhwc", "pool", "to_linear"}, B=1, max_batch=3, half="all")
_move("layout_c24_13x17_b1_of3", (24, 13, 17), lambda net, t: {"y": nhwc(net, t["x"])}, lambda x: {"y": Out(x["x"])}, {"to_nhwc", "pool", "to_linear"}, B=1, max_batch=3, half="all")
_move("layout_c12_128x128_b3_big", (12, 128, 128), lambda net, t: {"y": nhwc(net, t["x"])}, lambda x: {"y": Out(x["x"])}, {"to_nhwc", "pool", "to_linear"}, B=3, half="all")
_move("layout_c72_128x128_b4_big", (72, 128, 128), lambda net, t: {"y": nhwc(net, t["x"])}, lambda x: {"y": Out(x["x"])}, {"to_nhwc", "pool", "to_linear"}, B=4, half="all")


def _copy(C, H, W, B, max_batch=None, tag=""):
    """a tensor that already lives in one concat buffer is copied into the second: copy_nhwc into coff 0 and coff C"""
    def build(net, t):
        a = nhwc(net, t["x"])
        p = net.out(net.pooling(a, 3, 1, 1))
        return {"y0": net.out(net.concat([a, p])), "y1": net.out(net.concat([p, a]))}

    def ref(x):
        p = F.max_pool2d(x["x"], 3, 1, 1)
        return {"y0": Out(torch.cat([x["x"], p], 1)), "y1": Out(torch.cat([p, x["x"]], 1))}
    _move(f"copy_nhwc_c{C}_{H}x{W}_b{B}{tag}", (C, H, W), build, ref, {"copy_nhwc"}, B=B, max_batch=max_batch, half="all",
          inst=("copy_nhwc", "x4" if C % 4 == 0 else "x1", "x8" if C % 8 == 0 else "x1"))


for C, H, W, B in SHAPES:
    _copy(C, H, W, B)
_copy(12, 13, 17, 1, max_batch=3, tag="_of3")
_copy(*BIG_SCALAR, tag="_big")
_copy(*BIG_VECTOR, tag="_big")

for ax in range(4):   # slice with steps 2 and 3 on each axis
    for step in (2, 3):
        dims = (5, 6, 7, 8)
        start = [0, 1, 0, 2]
        stp = [1, 1, 1, 1]
        stp[ax] = step
        size = [(d - s0 - 1) // s + 1 for d, s0, s in zip(dims, start, stp)]
        sl = tuple(slice(s0, s0 + (n - 1) * s + 1, s) for s0, n, s in zip(start, size, stp))
        _move(f"slice_ax{ax}_step{step}", dims, lambda net, t, a=tuple(start), b=tuple(size), c=tuple(stp): {"y": net.out(net.slice(t["x"], a, b, c))},
              lambda x, sl=sl: {"y": Out(x["x"][(slice(None),) + sl])}, {"gather"})
_move("slice_all_steps", (5, 6, 7, 8), lambda net, t: {"y": net.out(net.slice(t["x"], (1, 0, 1, 0), (2, 2, 2, 3), (2, 3, 2, 3)))},
      lambda x: {"y": Out(x["x"][:, 1:4:2, 0:4:3, 1:4:2, 0:7:3])}, {"gather"}, B=3)
_move("slice_step2_b1_of3", (5, 6, 7), lambda net, t: {"y": net.out(net.slice(t["x"], (1, 0, 1), (2, 3, 3), (2, 2, 2)))},
      lambda x: {"y": Out(x["x"][:, 1:4:2, 0:5:2, 1:6:2])}, {"gather"}, B=1, max_batch=3)
_move("slice_step2_big", (12, 256, 256), lambda net, t: {"y": net.out(net.slice(t["x"], (0, 0, 1), (12, 256, 128), (1, 1, 2)))},
      lambda x: {"y": Out(x["x"][:, :, :, 1::2])}, {"gather"}, B=3)

for perm in itertools.permutations(range(3)):   # every permutation of rank 3
    if perm != (0, 1, 2):
        _move(f"shuffle_perm{''.join(map(str, perm))}", (4, 5, 6), lambda net, t, p=perm: {"y": net.out(net.shuffle(t["x"], perm1=p))},
              lambda x, p=perm: {"y": Out(x["x"].permute(0, *[i + 1 for i in p]).contiguous())}, {"gather"})
_move("shuffle_r4_perm_reshape", (4, 5, 6, 7), lambda net, t: {"y": net.out(net.shuffle(t["x"], perm1=(2, 0, 3, 1), reshape=(6, -1)))},
      lambda x: {"y": Out(x["x"].permute(0, 3, 1, 4, 2).reshape(-1, 6, 140))}, {"gather"})
_move("shuffle_r4_reshape_perm", (4, 5, 6, 7), lambda net, t: {"y": net.out(net.shuffle(t["x"], reshape=(20, 6, 7), perm2=(2, 0, 1)))},
      lambda x: {"y": Out(x["x"].reshape(-1, 20, 6, 7).permute(0, 3, 1, 2).contiguous())}, {"gather"})
_move("shuffle_r4_perm_reshape_perm", (4, 5, 6, 7), lambda net, t: {"y": net.out(net.shuffle(t["x"], perm1=(3, 2, 1, 0), reshape=(0, 0, 20), perm2=(1, 2, 0)))},
      lambda x: {"y": Out(x["x"].permute(0, 4, 3, 2, 1).reshape(-1, 7, 6, 20).permute(0, 2, 3, 1).contiguous())}, {"gather"}, B=3)
_move("shuffle_r5_perm", (2, 3, 4, 5, 6), lambda net, t: {"y": net.out(net.shuffle(t["x"], perm1=(4, 0, 3, 1, 2), reshape=(6, 2, -1)))},
      lambda x: {"y": Out(x["x"].permute(0, 5, 1, 4, 2, 3).reshape(-1, 6, 2, 60))}, {"gather"})
_move("shuffle_r5_to_r2_perm", (2, 3, 4, 5, 6), lambda net, t: {"y": net.out(net.shuffle(t["x"], reshape=(24, 30), perm2=(1, 0)))},
      lambda x: {"y": Out(x["x"].reshape(-1, 24, 30).transpose(1, 2).contiguous())}, {"gather"})
_move("shuffle_perm_b1_of3", (4, 5, 6), lambda net, t: {"y": net.out(net.shuffle(t["x"], perm1=(2, 0, 1)))},
      lambda x: {"y": Out(x["x"].permute(0, 3, 1, 2).contiguous())}, {"gather"}, B=1, max_batch=3)

for ax in (0, 1, 2, 3):   # concat on every axis of a LINEAR tensor (the channel axis is 0 here)
    _move(f"concat_lin_ax{ax}", (3, 4, 5, 6), lambda net, t, ax=ax: {"y": net.out(net.concat([t["x"], net.out(net.shuffle(t["x"], perm1=(0, 1, 2, 3))), t["x"]], axis=ax))},
          lambda x, ax=ax: {"y": Out(torch.cat([x["x"]] * 3, ax + 1))}, {"scatter"})


def _cat2(net, t, ax):
    a = net.out(net.slice(t["x"], (0, 0, 0), (4, 5, 3), (1, 1, 2)))
    return {"y": net.out(net.concat([a, t["x"]], axis=ax))}


_move("concat_lin_ax2_mixed", (4, 5, 6), lambda net, t: _cat2(net, t, 2), lambda x: {"y": Out(torch.cat([x["x"][..., 0:5:2], x["x"]], 3))}, {"scatter", "gather"}, B=3)
_move("concat_lin_ax2_mixed_b1_of3", (4, 5, 6), lambda net, t: _cat2(net, t, 2), lambda x: {"y": Out(torch.cat([x["x"][..., 0:5:2], x["x"]], 3))}, {"scatter", "gather"}, B=1,
      max_batch=3)
_move("identity", (4, 5), lambda net, t: {"y": net.out(net.identity(t["x"]))}, lambda x: {"y": Out(x["x"])}, {"copy_lin"}, B=3)
_move("identity_nhwc", (12, 5, 7), lambda net, t: {"y": net.out(net.identity(nhwc(net, t["x"])))}, lambda x: {"y": Out(x["x"])}, {"pool"}, B=3, half="all")
CONST = np.arange(24, dtype=np.float32).reshape(2, 3, 4) / 7
_move("constant_output", (4, 5), lambda net, t: {"c": net.out(net.constant(CONST)), "y": net.out(net.identity(t["x"]))},
      lambda x: {"c": Out(torch.from_numpy(CONST).double(), batched=False), "y": Out(x["x"])}, {"copy_lin"}, B=3)
