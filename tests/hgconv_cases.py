"""The case table of YOLOv13's hypergraph convolution (kernels/hgconv.hip; AdaHyperedgeGen + AdaHGConv, yolov13/src/block.cpp:607-790), shared by
tests/test_hgconv_cpu.py and tests/test_gpu_hgconv.py: seeded inputs and weights, a torch fp64 reference of the UNFOLDED definition with the
per-element error bound derived below, a NumPy fp32 emulation of the kernel's folded order (with one plausible bug at a time), and the builder
helper that spells the subgraph layer by layer as the reference does.

The definition (per image; X = N tokens of D channels, fp16; E hyperedges; heads = D / 16 contiguous channel groups of head_dim 16):
    ctx = [mean_n X, max_n X];  P = prototype_base + reshape(W_ctx ctx + b_ctx, E x D)
    logits[n, e] = mean_h(X_proj_h[n] . P_h[e]) / sqrt(head_dim),  X_proj = X W_pre^T + b_pre
    A = softmax(logits) over the NODE axis n;  He = A^T X;  He' = GELU(He W_edge^T + b_edge)
    out = GELU((A He') W_node^T + b_node) + X        GELU(v) = 0.5 v (1 + tanh(0.797885 (v + 0.044715 v^3)))

The bound.  u = 2^-24 (fp32), h = 2^-11 (fp16), g(k) = k u: a sum in which no term passes through more than k fp32 roundings, applied to the sum of
the absolute values.  k is the depth of the kernel's own summation order (kernels/hgconv.hip), not the term count: the column mean adds N / 32 rows per
lane and then 32 lanes (k_mean = N / 32 + 33); a prototype's dot product is 2 D / 64 terms per lane and a 6-step butterfly (k_P = 2 D / 64 + 8); Q, the edge
and the node projection add their D terms one after the other (k_D = D + 2); a logit is D / 8 terms per lane, a 3-step butterfly and the scale
(k_l = D / 8 + 4); the softmax sums add 32 nodes, 4 sub-tiles and the image's tiles (k_S = 42 + tiles); z adds E terms and the bias (k_z = E + 2).
The kernel keeps X in fp16 (the reference reads the same fp16 values) and everything else in fp32; its output is rounded to fp16 once.  Term by term,
with |.| taken per element and the sums over absolute values computed by the reference in fp64:
    d_ctx   = g(k_mean) mean|X|                              (the column mean; the max is exact)
    d_P     = g(k_P) (|W_ctx| |ctx| + |b_ctx| + |proto|) + |W_ctx| [d_ctx, 0]
    d_Q     = g(k_D) |P| |W_pre| + d_P |W_pre|               (Q = P W_pre, the folded pre_head_proj)
    d_l     = s (g(k_l) |X| |Q| + |X| d_Q)                   (the logit's error; the b_pre term is constant over n and drops out of the softmax)
    e_A[e]  = 2 max_n d_l[n, e] + g(k_S + 8) + 2 u (max_n l - min_n l)
              the relative error of A[., e]: exp turns a logit error d into a relative error d, in the numerator and (at most max_n d) in the
              denominator; the denominator is a sum of depth k_S; expf and the rounding of its argument l - M cost a few u
    d_He    = (e_A + g(k_S)) A^T |X|
    d_y1    = g(k_D) (|He| |W_edge|^T + |b_edge|) + d_He |W_edge|^T;   d_He' = 1.13 d_y1 + 8 u (|y1| + 1)     (|GELU'| <= 1.13)
    d_G     = g(k_D) |He'| |W_node|^T + d_He' |W_node|^T
    d_z     = A d_G + (e_A A) |G| + g(k_z) (A |G| + |b_node|)
    bound   = h |out| + 1.13 d_z + 8 u (|z| + 1) + u |out|
Every stage takes the worst case over the signs of the stage before it, so the bound grows with the row sums sum_j |W_ij| of the three D x D matrices and
of W_ctx.  Dense Gaussian rows would put a factor ~0.8 sqrt(D) on it at each of five stages for a signal that grows with the rows' 2-norm only; the
table's matrices therefore carry their weight in four entries per row at random columns over a dense Gaussian floor of 2 % (every entry is non-zero, an
index error in the dense part still moves the result by far more than the bound), which keeps the bound within two orders of the fp16 rounding.
Nothing in it is fitted: every term follows from the case's magnitudes."""
import collections
import functools
import math

import numpy as np
import torch

HEAD_DIM = 16
TILES = (32, 128)      # the launcher's node tiles (trtx_op_hgconv_geometry; tests/test_hgconv_cpu.py checks the table against the query)
U32, U16 = 2.0 ** -24, 2.0 ** -11
KAPPA, SQRT_2_OVER_PI = float(np.float32(0.044715)), float(np.float32(0.797885))
WEIGHTS = ("w_ctx", "b_ctx", "proto", "w_pre", "b_pre", "w_edge", "b_edge", "w_node", "b_node")

Case = collections.namedtuple("Case", "name D E H W B data")


def _c(D, E, hw, B, data="gauss"):
    return Case(f"d{D}e{E}_{hw[0]}x{hw[1]}_b{B}_{data}", D, E, hw[0], hw[1], B, data)


MODEL_DE = [(64, 4), (128, 8), (256, 8), (384, 12)]
OFF_MODEL_DE = [(16, 1), (48, 3), (384, 16)]
# N = 1, 35, 64, 65, 400, 1600 and T - 1, T, T + 1, 2 T + 1 for both tile sizes (31, 32, 33, 65, 127, 128, 129, 257)
NODE_MAPS = [(1, 1), (5, 7), (8, 8), (5, 13), (20, 20), (40, 40), (1, 31), (4, 8), (3, 11), (1, 127), (8, 16), (3, 43), (1, 257)]
DATA = ("gauss", "large", "tied", "dominant", "rising", "falling", "negative", "ctx", "bpre")

CASES = (
    [_c(D, E, (5, 7), 3) for D, E in MODEL_DE + OFF_MODEL_DE]
    + [_c(64, 4, hw, 1) for hw in NODE_MAPS]
    + [_c(384, 12, (40, 40), 1), _c(384, 12, (1, 257), 3), _c(384, 12, (8, 16), 1), _c(384, 12, (1, 127), 1), _c(384, 16, (3, 43), 3),
       _c(128, 8, (20, 20), 3), _c(256, 8, (8, 8), 1), _c(256, 8, (1, 31), 3), _c(48, 3, (3, 11), 1), _c(16, 1, (5, 13), 3)]
    + [_c(128, 8, (1, 257), 1, d) for d in ("large", "tied", "dominant", "rising", "falling", "negative")]
    + [_c(384, 12, (3, 43), 1, "large"), _c(64, 4, (5, 13), 3, "ctx"), _c(64, 4, (5, 7), 3, "bpre"), _c(256, 8, (3, 43), 3, "negative")]
)
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


def heads_of(D):
    return max(1, D // HEAD_DIM)


def logit_scale(D):
    """1 / (heads * scaling), scaling = sqrt(head_dim) as the reference rounds it to fp32 (block.cpp:681-688)"""
    return 1.0 / (heads_of(D) * float(np.float32(math.sqrt(D // heads_of(D)))))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gen(name):
    """(x: torch fp16 [B, N, D], weights: {name: numpy fp32}) of a case; seeded by its name"""
    c = BY_NAME[name]
    D, E, N, B = c.D, c.E, c.H * c.W, c.B
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31))
    n = lambda *s: rng.standard_normal(s).astype(np.float32)   # noqa: E731

    def mat(rows, cols, gain):
        """rows of 2-norm ~gain: four entries of +-gain / 2 at random columns on a dense Gaussian floor of 2 % (module docstring)"""
        m = n(rows, cols) * np.float32(0.02 * gain / math.sqrt(cols))
        idx = rng.integers(0, cols, (rows, 4))
        np.add.at(m, (np.arange(rows)[:, None], idx), (rng.choice([-0.5, 0.5], (rows, 4)) * gain).astype(np.float32))
        return m

    w = {
        "w_ctx": mat(E * D, 2 * D, 1.0),
        "b_ctx": 0.1 * n(E * D),
        "proto": n(E, D),
        "w_pre": mat(D, D, 0.3 * math.sqrt(D)),        # logits of spread ~2: s |X . Q| with |Q| ~ 0.3 sqrt(D) |P|, s = 4 / D
        "b_pre": n(D),
        "w_edge": mat(D, D, 2.0),
        "b_edge": 0.5 * n(D),
        # A's entries are ~1 / N (a softmax over the nodes), so A He' is ~E / N of He': node_proj's gain brings its result back to O(1)
        "w_node": mat(D, D, max(1.0, N / (2.0 * E))),
        "b_node": 0.5 * n(D),
    }
    x = n(B, N, D)
    if c.data == "large":          # logits beyond 100: exp without the max subtraction overflows fp32
        w["w_pre"] *= np.float32(40.0)
    elif c.data == "tied":         # Q = 0: every logit of a hyperedge is the same number (the b_pre term), A = 1 / N exactly
        w["w_pre"][:] = 0
    elif c.data in ("dominant", "rising", "falling"):
        w["w_ctx"][:] = 0          # P = prototype_base + b_ctx: the prototypes do not depend on X, so X can be built against Q
        w["b_ctx"][:] = 0
        if c.data != "dominant":   # one common direction in every prototype: X moving along it moves every hyperedge's logit the same way
            w["proto"] = (w["proto"][:1] + 0.05 * w["proto"]).astype(np.float32)
        q = w["proto"].astype(np.float64) @ w["w_pre"].astype(np.float64)                 # Q [E, D]
        s = logit_scale(D)
        if c.data == "dominant":   # node 17 e + 3 gets +30 on hyperedge e's logit
            for e in range(E):
                x[:, 17 * e + 3] += (30.0 / (s * (q[e] @ q[e])) * q[e]).astype(np.float32)
        else:
            v = q.mean(0)
            ramp = np.arange(N, dtype=np.float64) if c.data == "rising" else np.arange(N, dtype=np.float64)[::-1]
            x = (0.01 * x + ((ramp / N * 60.0)[None, :, None] * (v / (s * (v @ v)))[None, None, :])).astype(np.float32)   # logits 0 .. 60 along n
    elif c.data == "negative":     # a zero-filled pad row would be the column maximum
        x = -np.abs(x) - np.float32(0.1)
    elif c.data == "ctx":          # the images of the batch differ in their context: a prototype taken from the wrong image shows
        x = x + np.array([0.0, 2.0, -2.0], np.float32)[:B, None, None]
        w["w_ctx"] *= np.float32(3.0)
    elif c.data == "bpre":         # must have no effect
        w["b_pre"] *= np.float32(100.0)
    return torch.from_numpy(x).half(), {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


# ---- the fp64 reference of the unfolded definition, and the bound ---------------------------------------------------------------------------------------
def gelu64(v):
    return 0.5 * v * (1.0 + torch.tanh(SQRT_2_OVER_PI * (v + KAPPA * v ** 3)))


Ref = collections.namedtuple("Ref", "out bound A logits delta bound_generic")


def reference_of(x, w, D, E):
    """x: [B, N, D] (any float dtype; its values are taken as they are), w: {name: numpy fp32}.  -> Ref: out, bound [B, N, D], A, logits [B, N, E] fp64,
    delta = out - x"""
    X = x.double()
    B, N, _ = X.shape
    heads = heads_of(D)
    hd = D // heads
    W = {k: torch.from_numpy(v).double() for k, v in w.items()}
    ctx = torch.cat([X.mean(1), X.max(1).values], 1)                                   # [B, 2 D]
    P = W["proto"][None] + (ctx @ W["w_ctx"].T + W["b_ctx"]).reshape(B, E, D)
    Xp = X @ W["w_pre"].T + W["b_pre"]
    Xh = Xp.reshape(B, N, heads, hd).transpose(1, 2)                                    # [B, heads, N, hd]
    Ph = P.reshape(B, E, heads, hd).permute(0, 2, 1, 3)                                 # [B, heads, E, hd]
    scaling = float(np.float32(math.sqrt(hd)))
    logits = ((Xh @ Ph.transpose(-2, -1)) / scaling).mean(1)                            # [B, N, E]
    A = logits.softmax(1)                                                               # over the nodes
    He = A.transpose(1, 2) @ X                                                          # [B, E, D]
    y1 = He @ W["w_edge"].T + W["b_edge"]
    He2 = gelu64(y1)
    G = He2 @ W["w_node"].T
    z = A @ G + W["b_node"]
    out = gelu64(z) + X
    # ---- the bound (module docstring)
    g = lambda k: k * U32   # noqa: E731
    nt = -(-N // TILES[1])
    k_mean, k_P, k_D, k_l, k_S, k_z = -(-N // 32) + 33, -(-2 * D // 64) + 8, D + 2, -(-D // 64) * 8 + 4, 42 + nt, E + 2
    s = logit_scale(D)
    aW = {k: v.abs() for k, v in W.items()}
    aX = X.abs()
    d_ctx = torch.cat([g(k_mean) * aX.mean(1), torch.zeros(B, D, dtype=torch.float64)], 1)
    d_P = (g(k_P) * (ctx.abs() @ aW["w_ctx"].T + aW["b_ctx"]) + d_ctx @ aW["w_ctx"].T).reshape(B, E, D) + g(k_P) * aW["proto"][None]
    Q = P @ W["w_pre"]
    d_Q = g(k_D) * (P.abs() @ aW["w_pre"]) + d_P @ aW["w_pre"]
    d_l = s * (g(k_l) * (aX @ Q.abs().transpose(1, 2)) + aX @ d_Q.transpose(1, 2))                    # [B, N, E]
    e_A = 2 * d_l.max(1).values + g(k_S + 8) + 2 * U32 * (logits.max(1).values - logits.min(1).values)  # [B, E]
    At = A.transpose(1, 2)
    d_He = (e_A + g(k_S))[:, :, None] * (At @ aX)
    d_y1 = g(k_D) * (He.abs() @ aW["w_edge"].T + aW["b_edge"]) + d_He @ aW["w_edge"].T
    d_He2 = 1.13 * d_y1 + 8 * U32 * (y1.abs() + 1)
    d_G = g(k_D) * (He2.abs() @ aW["w_node"].T) + d_He2 @ aW["w_node"].T
    d_z = A @ d_G + (A * e_A[:, None, :]) @ G.abs() + g(k_z) * (A @ G.abs() + aW["b_node"])
    bound = U16 * out.abs() + 1.13 * d_z + 8 * U32 * (z.abs() + 1) + U32 * out.abs()
    # ---- the generic lowering of the same fp16 graph (TRTX_HGCONV=0) has fp16 sites the fused op does not: the four fully connected layers run as
    # convolutions with fp16 weights, fp16 inputs and fp16 stored outputs, and both GELU chains store fp16.  Its bound is the fused one plus, with
    # h = 2^-11 per site: ctx, W_ctx and the stored offsets into P; X_proj's weights and store into the logits; He, W_edge, y1 and He' ; x_new = A He',
    # W_node, z and GELU(z).  (The fp32 linear matmuls, the softmax and the residual add are covered by the fused bound's fp32 terms.)
    off = ctx @ W["w_ctx"].T + W["b_ctx"]
    g_P = (U16 * (2 * ctx.abs() @ aW["w_ctx"].T + off.abs())).reshape(B, E, D)
    g_Xp = U16 * (aX @ aW["w_pre"].T + Xp.abs())
    g_l = ((g_Xp.reshape(B, N, heads, hd).transpose(1, 2) @ Ph.abs().transpose(-2, -1)
            + Xh.abs() @ g_P.reshape(B, E, heads, hd).permute(0, 2, 1, 3).transpose(-2, -1)) / scaling).mean(1)
    ge_A = 2 * g_l.max(1).values                                                        # [B, E]
    g_He = ge_A[:, :, None] * (At @ aX) + U16 * He.abs()
    g_y1 = g_He @ aW["w_edge"].T + U16 * (He.abs() @ aW["w_edge"].T + y1.abs())
    g_He2 = 1.13 * g_y1 + U16 * He2.abs()
    xn = A @ He2
    g_xn = A @ g_He2 + (A * ge_A[:, None, :]) @ He2.abs() + U16 * xn.abs()
    g_z = g_xn @ aW["w_node"].T + U16 * (xn.abs() @ aW["w_node"].T + z.abs())
    bound_generic = bound + 1.13 * g_z + U16 * gelu64(z).abs()
    return Ref(out, bound, A, logits, out - X, bound_generic)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = BY_NAME[name]
    x, w = gen(name)
    return reference_of(x, w, c.D, c.E)


# ---- NumPy fp32 emulation of the kernel's folded order ---------------------------------------------------------------------------------------------------
BUGS = ("softmax_e", "no_heads", "erf", "no_residual", "swap_ctx", "pad_max", "pad_sum", "he_from_xproj")


def _gelu32(v, erf=False):
    f = np.float32
    if erf:
        return (f(0.5) * v * (f(1) + torch.erf(torch.from_numpy(v * f(1 / math.sqrt(2)))).numpy())).astype(f)
    inner = v + ((v * v) * v) * f(0.044715)
    return ((v * (np.tanh(inner * f(0.797885)) + f(1))) * f(0.5)).astype(f)


def emulate(name, bug=None):
    """The launch chain of kernels/hgconv.hip in NumPy float32: column mean / max, P, Q = P W_pre, logits = s X . Q, the online softmax over sub-tiles of
    32 nodes inside tiles of 128 with the tiles merged in ascending order, He' and G = He' W_node^T, out = GELU(A G + b_node) + X rounded to fp16.
    bug: one of BUGS, a plausible mistake restated.  -> torch fp16 [B, N, D]"""
    assert bug is None or bug in BUGS
    c = BY_NAME[name]
    x16, w = gen(name)
    f = np.float32
    X = x16.float().numpy()
    B, N, D = X.shape
    E, sub, tile = c.E, TILES[0], TILES[1]
    s = f(logit_scale(D) * (heads_of(D) if bug == "no_heads" else 1))
    gelu = functools.partial(_gelu32, erf=bug == "erf")
    out = np.empty_like(X)
    for b in range(B):
        xb = X[b]
        mean, mx = xb.sum(0, dtype=f) / f(N), xb.max(0)
        if bug == "pad_max" and N % sub:
            mx = np.maximum(mx, f(0))                       # a zero-filled row of the last tile joins the column maximum
        ctx = np.concatenate([mx, mean] if bug == "swap_ctx" else [mean, mx])
        P = w["proto"] + (w["w_ctx"] @ ctx + w["b_ctx"]).reshape(E, D)
        Q = (P @ w["w_pre"]).astype(f)
        l = ((xb @ Q.T) * s).astype(f)                      # [N, E]
        if bug == "softmax_e":                              # the softmax over the hyperedges: the b_pre term no longer cancels
            lf = l + s * (P @ w["b_pre"])[None]
            A = np.exp(lf - lf.max(1, keepdims=True))
            A = (A / A.sum(1, keepdims=True)).astype(f)
            He = (A.T @ xb).astype(f)
        else:
            parts = []
            for t0 in range(0, N, tile):
                m, ssum, H = np.full(E, -np.inf, f), np.zeros(E, f), np.zeros((E, D), f)
                for s0 in range(t0, min(t0 + tile, N), sub):
                    ls, xs = l[s0:min(s0 + sub, N, t0 + tile)], xb[s0:min(s0 + sub, N, t0 + tile)]
                    mn = np.maximum(m, ls.max(0))
                    fac = np.exp(m - mn).astype(f)
                    a = np.exp(ls - mn).astype(f)
                    ssum = ssum * fac + a.sum(0, dtype=f)
                    H = H * fac[:, None] + (a.T @ xs).astype(f)
                    m = mn
                parts.append((m, ssum, H))
            M = np.max([p[0] for p in parts], 0)
            if bug == "pad_sum" and N % tile:
                M = np.maximum(M, f(0))
            S, Hs = np.zeros(E, f), np.zeros((E, D), f)
            for m, ssum, H in parts:
                r = np.exp(m - M).astype(f)
                S = S + ssum * r
                Hs = Hs + H * r[:, None]
            if bug == "pad_sum" and N % tile:               # the zero rows that fill the last tile have logit 0 and join the denominator
                S = S + f(tile - N % tile) * np.exp(-M).astype(f)
            He = (Hs / S[:, None]).astype(f)
            A = (np.exp(l - M[None]).astype(f) / S[None]).astype(f)
            if bug == "he_from_xproj":
                He = (A.T @ (xb @ w["w_pre"].T + w["b_pre"])).astype(f)
        He2 = gelu((He @ w["w_edge"].T + w["b_edge"]).astype(f))
        G = (He2 @ w["w_node"].T).astype(f)
        z = (A @ G + w["b_node"]).astype(f)
        out[b] = gelu(z) + (f(0) if bug == "no_residual" else xb)
    return torch.from_numpy(out).half()


# ---- the subgraph, layer by layer as the reference builds it -------------------------------------------------------------------------------------------
def gelu_chain(net, t, rank, sqrt_c=0.797885):
    """GELU() of yolov13/src/block.cpp:702-744 on tensor t: nine computing layers and four one-element constants -> the last layer"""
    one = (1,) * rank
    k = lambda v: net.out(net.constant(np.full(one, v, np.float32)))   # noqa: E731
    x2 = net.out(net.elementwise(t, t, "prod"))
    x3 = net.out(net.elementwise(x2, t, "prod"))
    sx3 = net.out(net.elementwise(x3, k(0.044715), "prod"))
    inner = net.out(net.elementwise(t, sx3, "sum"))
    si = net.out(net.elementwise(inner, k(sqrt_c), "prod"))
    th = net.out(net.activation(si, "tanh"))
    a1 = net.out(net.elementwise(th, k(1.0), "sum"))
    hx = net.out(net.elementwise(t, a1, "prod"))
    return net.elementwise(hx, k(0.5), "prod")


def ada_hg_computation(net, x, B, D, H, W, E, w, spelling="a", miss=None, heads=None):
    """AdaHGComputation (block.cpp:792-812) on the image tensor x (B, D, H, W) -> the tensor of its x_out shuffle.  spelling 'a': the batch-correct
    reshapes; 'b': the reference's literal ones (a valid network at B == 1 only: at B > 1 its edge_proj would need D x (B D) weights and its last
    reshape (1, B N, D) cannot be added to the (B, N, D) tokens); 'b2': what of (b) a network definition accepts at B > 1 - He as (E, B, D, 1) into an
    edge_proj over B D inputs (w_edge repeated B times along its inputs) and the 2-d matmul of (N B, E) with (E, D), the last reshape as in (a).  miss breaks one thing the matcher checks: 'softmax_e' (the softmax
    over the hyperedges), 'gelu_const' (0.797886 in the edge GELU), 'mean_only' (context "mean"), 'a_output' (A is also a network output), 'he_reader'
    (He has a second reader, marked as an output)."""
    N = H * W
    heads = heads or heads_of(D)
    hd = D // heads
    o = net.out
    tok = o(net.shuffle(x, reshape=(B, D, N), perm2=(0, 2, 1)))
    mean = o(net.reduce(tok, "avg", 1 << 1))
    if miss == "mean_only":
        cat, kc = mean, D
    else:
        cat, kc = o(net.concat([mean, o(net.reduce(tok, "max", 1 << 1))], axis=1)), 2 * D
    w_ctx = w["w_ctx"][:, :kc]
    off = o(net.shuffle(o(net.fully_connected(o(net.shuffle(cat, reshape=(B, kc, 1, 1))), w_ctx, w["b_ctx"])), reshape=(B, E, D)))
    protos = o(net.elementwise(o(net.constant(w["proto"].reshape(1, E, D))), off, "sum"))
    xp = o(net.fully_connected(o(net.shuffle(tok, reshape=(B * N, D, 1, 1))), w["w_pre"], w["b_pre"]))
    xh = o(net.shuffle(xp, reshape=(B, N, heads, hd), perm2=(0, 2, 1, 3)))
    ph = o(net.shuffle(protos, reshape=(B, E, heads, hd), perm2=(0, 2, 1, 3)))
    xhf = o(net.shuffle(xh, reshape=(B * heads, N, hd)))
    phf = o(net.shuffle(ph, reshape=(B * heads, E, hd), perm2=(0, 2, 1)))
    lg = o(net.matmul(xhf, phf))
    sc = o(net.constant(np.full((1, 1, 1), math.sqrt(hd), np.float32)))
    lgv = o(net.shuffle(o(net.elementwise(lg, sc, "div")), reshape=(B, heads, N, E)))
    A = o(net.softmax(o(net.reduce(lgv, "avg", 1 << 1)), axes=1 << (2 if miss == "softmax_e" else 1)))
    if miss == "a_output":
        net.mark_output(A, "A")
    He = o(net.matmul(A, tok, transpose_a=True))
    if miss == "he_reader":
        net.mark_output(o(net.identity(He)), "He")
    he4 = o(net.shuffle(He, reshape=(B * E, D, 1, 1) if spelling == "a" else (E, B, D, 1)))
    w_edge = np.tile(w["w_edge"], (1, B)) if spelling == "b2" else w["w_edge"]
    g1 = o(gelu_chain(net, o(net.fully_connected(he4, w_edge, w["b_edge"])), 4, sqrt_c=0.797886 if miss == "gelu_const" else 0.797885))
    if spelling == "a":
        xn = o(net.matmul(A, o(net.shuffle(g1, reshape=(B, E, D)))))
    else:
        xn = o(net.matmul(o(net.shuffle(A, reshape=(N * B, E))), o(net.shuffle(g1, reshape=(E, D)))))
    g2 = o(gelu_chain(net, o(net.fully_connected(o(net.shuffle(xn, reshape=(B * N, D, 1, 1))), w["w_node"], w["b_node"])), 4))
    fin = o(net.shuffle(g2, reshape=(1, B * N, D) if spelling == "b" else (B, N, D)))
    add = o(net.elementwise(fin, tok, "sum"))
    return o(net.shuffle(add, perm1=(0, 2, 1), reshape=(B, D, H, W)))


def c3ah_weights(D, cin=3, cout=32, seed=0):
    """cv1 / cv2 (cin -> D) and cv3 (2 D -> cout), 1x1, no activation: the convolutions around AdaHGComputation in C3AH (block.cpp:814-829)"""
    rng = np.random.default_rng(1000 + seed)
    return {"cv1": (rng.standard_normal((D, cin, 1, 1)) * 0.8).astype(np.float32), "cv2": (rng.standard_normal((D, cin, 1, 1)) * 0.8).astype(np.float32),
            "cv3": (rng.standard_normal((cout, 2 * D, 1, 1)) / math.sqrt(2 * D)).astype(np.float32)}


def subgraph_net(B, D, E, H, W, w, cw, spelling="a", miss=None, fp16=True, heads=None, mark_inner=False):
    """conv -> AdaHGComputation -> concat -> conv on a (B, cin, H, W) input "x": the serialized plan.  mark_inner: cv1's output ("x1") and the
    hypergraph convolution's ("m") are network outputs too (for the interpreter check)."""
    from tensorrtx_amd import builder
    net = builder.Network(explicit_batch=True, fp16=fp16)
    try:
        xi = net.input("x", (B, cw["cv1"].shape[1], H, W))
        x1 = net.out(net.conv(xi, cw["cv1"]))
        x2 = net.out(net.conv(xi, cw["cv2"]))
        m = ada_hg_computation(net, x1, B, D, H, W, E, w, spelling=spelling, miss=miss, heads=heads)
        if mark_inner:
            net.mark_output(x1, "x1")
            net.mark_output(m, "m")
        y = net.out(net.conv(net.out(net.concat([m, x2])), cw["cv3"]))
        net.mark_output(y, "y")
        return net.build()
    finally:
        net.close()
