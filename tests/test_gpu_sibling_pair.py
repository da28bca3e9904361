"""The dual tile on the GPU (kernels/igemm_tile.h, conv_igemm_dual_group_f16_kernel): convolutions to 64 and to 80 channels that read the same tensor, as one
launch, return bit for bit what their own launches of the implicit-GEMM kernel's main K order return - single problems over ragged tiles, a tile seam inside an
image, a ragged channel chunk, strided outputs, two different epilogues and a ragged last column fragment; a group of three with empty XCD chunks; what the launch
refuses; and the engine with the lowering switch on and off.  Outputs start from a guard value: whatever the launch does not own must keep it."""
import numpy as np
import pytest

GUARD = -7.0
TAIL = 16                      # guard rows behind the last pixel of every output buffer
INVALID, UNSUPPORTED = 1, 4    # TRTX_ERR_*


def _main_k_order(bn):         # 32-wide k-steps, 128-row tiles, no wave-split-K, no weight-stationary kernel: the K order of a grouped launch's members
    return (bn, 32, 128, 1, 1, 0)


class Problem:
    """one input and the two layers that read it; outputs are channel windows [coff, coff + cout) of guard-filled [M + TAIL][ld] buffers"""

    def __init__(self, gpu, N, H, W, cin, seed, cout=(64, 80), ld=(64, 80), coff=(0, 0), act=("silu", "silu"), one_buffer=False):
        import torch
        from tensorrtx_amd import capi
        rng = np.random.default_rng(seed)
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.gpu, self.shape, self.cout, self.ld, self.coff, self.act, self.one_buffer = gpu, (N, H, W), cout, ld, coff, act, one_buffer
        self.x = torch.randn((N, H, W, cin), generator=g, dtype=torch.float32).to(torch.float16).to(gpu)
        self.w, self.b = [], []
        for c in cout:
            w = (rng.standard_normal((c, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32)
            packed, cout_pad, _, bn = capi.pack_conv_weights_f16(w)
            assert bn == cout_pad == (64 if c <= 64 else 80)
            self.w.append(torch.from_numpy(packed.view(np.int16)).to(gpu))
            self.b.append(torch.from_numpy(rng.standard_normal(cout_pad).astype(np.float32)).to(gpu))

    def buffers(self):
        import torch
        N, H, W = self.shape
        rows = N * H * W + TAIL
        bufs = [torch.full((rows, ld), GUARD, dtype=torch.float16, device=self.gpu) for ld in (self.ld[:1] if self.one_buffer else self.ld)]
        if self.one_buffer:
            bufs = [bufs[0], bufs[0]]
        return bufs

    def views(self, bufs):
        N, H, W = self.shape
        return [b[:N * H * W, o:o + c].view(N, H, W, c) for b, o, c in zip(bufs, self.coff, self.cout)]

    def reference(self, residual=None):
        """each layer as its own launch"""
        from tensorrtx_amd import capi
        bufs = self.buffers()
        for side, v in enumerate(self.views(bufs)):
            capi.conv_force_tactic(_main_k_order(64 if side == 0 else 80))
            try:
                capi.conv2d_nhwc_f16(self.x, self.w[side], self.b[side], self.cout[side], 3, 3, 1, 1, act1=self.act[side], out=v, out_ld=self.ld[side],
                                     residual=residual if side == 1 else None)
            finally:
                capi.conv_force_tactic(None)
        return bufs


def _dual(problems, bufs, **kw):
    from tensorrtx_amd import capi
    v = [p.views(b) for p, b in zip(problems, bufs)]
    p0 = problems[0]
    return capi.conv_dual_group_f16([p.x for p in problems], [p.w[0] for p in problems], [p.b[0] for p in problems], [x[0] for x in v],
                                    [p.w[1] for p in problems], [p.b[1] for p in problems], [x[1] for x in v], act0=p0.act[0], act1=p0.act[1], **kw)


def _same(got, want):
    import torch
    return all(torch.equal(g.view(torch.int16), w.view(torch.int16)) for g, w in zip(got, want))


CASES = {
    "one ragged tile":            dict(N=1, H=5, W=5, cin=64),                                    # M = 25: every border tap
    "tile seam inside an image":  dict(N=3, H=7, W=9, cin=64),                                    # M = 189: row 128 lies inside image 2
    "ragged channel chunk":       dict(N=2, H=6, W=7, cin=40),                                    # CinK 64: the second k-step of a tap holds 8 real channels
    "strided outputs":            dict(N=2, H=6, W=7, cin=64, ld=(96, 144), coff=(16, 32)),       # channel windows of wider buffers, both sides
    "side by side in one buffer": dict(N=2, H=6, W=7, cin=64, ld=(144, 144), coff=(0, 64), one_buffer=True),
    "two epilogues":              dict(N=2, H=6, W=7, cin=64, act=("silu", "none")),
    "ragged last fragment":       dict(N=2, H=6, W=7, cin=64, cout=(64, 72), ld=(64, 72)),        # 72 of the 80 columns exist
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_one_dual_problem_equals_its_two_launches_bit_for_bit(gpu, name):
    import torch
    p = Problem(gpu, seed=sum(map(ord, name)), **CASES[name])
    want = p.reference()
    got = p.buffers()
    _dual([p], [got])
    torch.cuda.synchronize()
    assert _same(got, want), name                                     # the written windows AND every guard element around them
    N, H, W = p.shape
    for b, v, act in zip(want, p.views(want), p.act):
        assert bool((b[N * H * W:] == GUARD).all()) and float(v.float().abs().max()) > 0.5      # rows behind the last pixel untouched; not a comparison of zeros
    written = sum(int((b != GUARD).sum()) for b in (want[:1] if p.one_buffer else want))
    assert written <= N * H * W * sum(p.cout) and written > 0.99 * N * H * W * sum(p.cout)     # nothing outside the windows (a result that equals the guard is rare)
    if name == "two epilogues":
        assert float(p.views(want)[1].min()) < -0.5 < float(p.views(want)[0].min())               # SiLU is bounded below by -0.28, no activation is not


@pytest.mark.gpu
@pytest.mark.parametrize("or_two", [False, True])
def test_group_of_three_with_empty_xcd_chunks(gpu, or_two):
    """the head's shape in small: 64 / 128 / 256 channels at 8 x 8 / 4 x 4 / 2 x 2, three images - 2, 1 and 1 tiles for eight XCD chunks each"""
    import torch
    ps = [Problem(gpu, 3, s, s, cin, seed=cin) for cin, s in ((64, 8), (128, 4), (256, 2))]
    want = [p.reference() for p in ps]
    got = [p.buffers() for p in ps]
    _dual(ps, got, or_two=or_two)
    torch.cuda.synchronize()
    for p, g, w in zip(ps, got, want):
        assert _same(g, w), p.x.shape
        assert all(float(v.float().abs().max()) > 0.5 for v in p.views(w))


@pytest.mark.gpu
def test_an_output_on_the_input_or_on_the_other_output_is_invalid_and_nothing_is_written(gpu):
    import torch
    from tensorrtx_amd import capi
    p = Problem(gpu, 2, 6, 7, 64, seed=5)
    N, H, W = p.shape
    wide = torch.full((N, H, W, 224), GUARD, dtype=torch.float16, device=gpu)
    wide[..., :64] = p.x
    x = wide[..., :64]
    before = wide.clone()
    apart = p.views(p.buffers())
    args = lambda o0, o1: ([x], [p.w[0]], [p.b[0]], [o0], [p.w[1]], [p.b[1]], [o1])
    for o0, o1 in ((wide[..., 32:96], apart[1]),                   # half on the input channels
                   (apart[0], wide[..., 0:80]),                     # the second side on the input
                   (wide[..., 64:128], wide[..., 112:192])):        # the two outputs on each other
        assert capi.conv_dual_group_f16(*args(o0, o1), status_only=True) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(wide.view(torch.int16), before.view(torch.int16)) and all(bool((v == GUARD).all()) for v in apart)
    # next to the input and next to each other is fine
    want = p.reference()
    capi.conv_dual_group_f16(*args(wide[..., 64:128], wide[..., 128:208]))
    torch.cuda.synchronize()
    for lo, hi, v in ((64, 128, p.views(want)[0]), (128, 208, p.views(want)[1])):
        assert torch.equal(wide[..., lo:hi].contiguous().view(torch.int16), v.contiguous().view(torch.int16))
    for lo, hi in ((0, 64), (208, 224)):
        assert torch.equal(wide[..., lo:hi].contiguous().view(torch.int16), before[..., lo:hi].contiguous().view(torch.int16))


@pytest.mark.gpu
def test_what_the_dual_tile_does_not_take_is_unsupported_and_the_executors_form_computes_it(gpu):
    import torch
    from tensorrtx_amd import capi
    # an int8 side
    p = Problem(gpu, 2, 6, 7, 64, seed=6)
    got = p.buffers()
    assert _dual([p], [got], i8_1=True, status_only=True) == UNSUPPORTED
    # a shortcut on a side
    res = torch.randn((2, 6, 7, 80), dtype=torch.float32, generator=torch.Generator(device="cpu").manual_seed(1)).to(torch.float16).to(gpu)
    assert _dual([p], [got], res1=[res], status_only=True) == UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((b == GUARD).all()) for b in got)
    _dual([p], [got], res1=[res], or_two=True)
    torch.cuda.synchronize()
    assert _same(got, p.reference(residual=res))
    # Cin <= 16: two filter taps per k-step
    q = Problem(gpu, 2, 6, 7, 16, seed=7)
    got = q.buffers()
    assert _dual([q], [got], status_only=True) == UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((b == GUARD).all()) for b in got)
    _dual([q], [got], or_two=True)
    torch.cuda.synchronize()
    assert _same(got, q.reference())


def _outputs(e, B, gpu):
    import torch
    return [None if e.is_input[i] else torch.full((B * int(np.prod(e.dims[i])),), float("nan"), dtype=torch.float32, device=gpu) for i in range(e.nb_bindings)]


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["0", None])
def test_engine_with_and_without_the_pair_is_bit_identical(gpu, monkeypatch, tune):
    """YOLOv8n at 2 x 3 x 128 x 128 (head maps 16 / 8 / 4), built for contexts in flight (one lane): the marked engine against the same plan lowered with
    TRTX_SIBLING_PAIR=0, static tactics and timed ones; one profile row per op either way, the first group of the pair reporting no kernel."""
    import torch
    from tensorrtx_amd import engine, synth
    from util import synth_wts
    if tune is not None:
        monkeypatch.setenv("TRTX_TUNE", tune)
    path, _ = synth_wts("yolov8n")
    B, S = 2, 128
    plan = engine.build_plan("yolov8n", path, batch=B, h=S, w=S, fp16=1, mark_heads=1, aux_streams=0)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    marked = [k for k, o in enumerate(ops) if o.get("sibling_pair")]
    assert len(marked) == 1 and sorted(m["hw_in"][0] for m in ops[marked[0]]["members"]) == [4, 8, 16]
    k = marked[0]
    x = torch.from_numpy(synth.images(B, S, S, seed=3)).to(gpu)
    engines = {}
    try:
        engines["on"] = engine.Engine(plan)
        monkeypatch.setenv("TRTX_SIBLING_PAIR", "0")
        assert not any(o.get("sibling_pair") for o in engine.describe_plan(plan, lowered=True)["ops"])
        engines["off"] = engine.Engine(plan)
        monkeypatch.delenv("TRTX_SIBLING_PAIR")
        res = {}
        for name, e in engines.items():
            res[name] = []
            for b in (B, 1):                                           # ... and a batch below the largest
                outs = _outputs(e, B, gpu)
                e.enqueue(b, [x if t is None else t for t in outs])
                torch.cuda.synchronize()
                res[name].append(outs)
            rows = e.profile(B, [x if t is None else t for t in _outputs(e, B, gpu)])
            assert len(rows) == len(ops) and [r["kind"] for r in rows] == [o["kind"] for o in ops]
            assert rows[k]["kernel_ms"] > 0 and (rows[k - 1]["kernel_ms"] <= 0) == (name == "on"), (name, rows[k - 1], rows[k])
        on = engines["on"]
        for r_on, r_off in zip(res["on"], res["off"]):
            for i in range(on.nb_bindings):
                if on.is_input[i]:
                    continue
                a, b = r_on[i].view(torch.int32), r_off[i].view(torch.int32)
                assert torch.equal(a, b), (on.names[i], int((a != b).sum()))
        for i in range(on.nb_bindings):
            if not on.is_input[i] and on.names[i].startswith("head"):
                assert not torch.isnan(res["off"][0][i]).any()         # (every element of a head tensor is written: not a comparison of sentinels)
    finally:
        for e in engines.values():
            e.close()
