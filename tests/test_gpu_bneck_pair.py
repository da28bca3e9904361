"""The fused bottleneck pair on the GPU (kernels/conv_bneck_pair.hip): the two 3x3 convolutions of a 16-channel bottleneck in one launch return, bit for bit,
what two launches of the implicit-GEMM kernel's main K order return - at the op level over shapes that exercise partial tiles, image seams, odd sizes
and the real plan's aliasing (source and destination are channel slices of one concat buffer), and at the engine level with the lowering switch on and off."""
import numpy as np
import pytest

# N, H, W of the 16-channel NHWC input (tile 8 x 16); what the shape catches
SHAPES = [
    (1, 5, 6),       # everything inside one partial tile
    (2, 16, 32),     # exact tiles, an image seam inside a workgroup's tile run
    (3, 19, 35),     # ragged in both directions, odd sizes, runs crossing images
    (2, 9, 17),      # one row and one column past a tile
]
MAIN_K_ORDER = (16, 32, 128, 1, 1, 0)   # column tile 16, 32-wide k-steps, 128-row tiles, no wave-split-K, no weight-stationary kernel: the default tactic's K order


@pytest.fixture(scope="module")
def layers(gpu):
    """the two layers' packed weights (random normal, non-zero biases), shared by the op-level tests"""
    import torch
    from tensorrtx_amd import capi
    rng = np.random.default_rng(13)
    L = {}
    for name in ("1", "2"):
        w = (rng.standard_normal((16, 16, 3, 3)) * (2.0 / 144) ** 0.5).astype(np.float32)
        packed, cout_pad, kpad, _ = capi.pack_conv_weights_f16(w, cin_pad=16)
        assert (cout_pad, kpad) == (16, 160)
        L["w" + name] = torch.from_numpy(packed.view(np.int16)).to(gpu)
        L["b" + name] = torch.from_numpy(rng.standard_normal(16).astype(np.float32)).to(gpu)
    return L


def _two_launches(x, L, act, shortcut, act_after="none"):
    from tensorrtx_amd import capi
    capi.conv_force_tactic(MAIN_K_ORDER)
    try:
        mid = capi.conv2d_nhwc_f16(x, L["w1"], L["b1"], 16, 3, 3, 1, 1, act1=act)
        return capi.conv2d_nhwc_f16(mid, L["w2"], L["b2"], 16, 3, 3, 1, 1, act1=act, residual=x if shortcut else None, act2=act_after)
    finally:
        capi.conv_force_tactic(None)


def _input(gpu, N, H, W, C=16):
    import torch
    g = torch.Generator(device="cpu").manual_seed(N * 100000 + H * 100 + W)
    return torch.randn((N, H, W, C), generator=g, dtype=torch.float32).to(torch.float16).to(gpu)


@pytest.fixture(scope="module")
def references(gpu, layers):
    """the two-launch result per (shape, shortcut), computed once"""
    import torch
    ref = {}
    for N, H, W in SHAPES:
        for shortcut in (True, False):
            ref[(N, H, W, shortcut)] = _two_launches(_input(gpu, N, H, W), layers, "silu", shortcut)
    torch.cuda.synchronize()
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("shortcut", [True, False])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_pair_equals_two_convolutions_bit_for_bit(gpu, layers, references, N, H, W, shortcut):
    import torch
    from tensorrtx_amd import capi
    x = _input(gpu, N, H, W)
    want = references[(N, H, W, shortcut)]
    got = capi.conv_bneck_pair_f16(x, layers["w1"], layers["b1"], layers["w2"], layers["b2"], shortcut=shortcut)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (N, H, W, 16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got.view(torch.int16) != want.view(torch.int16)).sum())
    assert float(want.float().abs().max()) > 0.5    # (not a comparison of zeros)


@pytest.mark.gpu
def test_pair_reads_and_writes_channel_slices_of_one_buffer(gpu, layers):
    """the real plan's aliasing: one 48-wide buffer, input = channels 16 .. 31, output = channels 32 .. 47"""
    import torch
    from tensorrtx_amd import capi
    N, H, W = SHAPES[2]
    wide = torch.full((N, H, W, 48), -7.0, dtype=torch.float16, device=gpu)   # sentinel
    wide[..., 16:32] = _input(gpu, N, H, W)
    before = wide.clone()
    want = _two_launches(wide[..., 16:32].contiguous(), layers, "silu", True)
    sliced = _two_launches(wide[..., 16:32], layers, "silu", True)            # (the two launches on the strided slice agree with the contiguous form)
    capi.conv_bneck_pair_f16(wide[..., 16:32], layers["w1"], layers["b1"], layers["w2"], layers["b2"], out=wide[..., 32:], out_ld=48)
    torch.cuda.synchronize()
    assert torch.equal(sliced.view(torch.int16), want.view(torch.int16))
    assert torch.equal(wide[..., 32:].contiguous().view(torch.int16), want.view(torch.int16))
    assert torch.equal(wide[..., :32].contiguous().view(torch.int16), before[..., :32].contiguous().view(torch.int16))
    assert float(want.float().abs().max()) > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("shortcut,act_after", [(True, "none"), (True, "relu"), (False, "none")])
def test_pair_with_relu(gpu, layers, shortcut, act_after):
    import torch
    from tensorrtx_amd import capi
    N, H, W = SHAPES[3]
    x = _input(gpu, N, H, W)
    want = _two_launches(x, layers, "relu", shortcut, act_after)
    got = capi.conv_bneck_pair_f16(x, layers["w1"], layers["b1"], layers["w2"], layers["b2"], act1="relu", act2="relu", shortcut=shortcut, act_after=act_after)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and float(want.float().max()) > 0.5
    if not shortcut or act_after == "relu":
        assert float(want.float().min()) == 0.0


def _outputs(e, B, gpu):
    import torch
    return [None if e.is_input[i] else torch.full((B * int(np.prod(e.dims[i])),), float("nan"), dtype=torch.float32, device=gpu) for i in range(e.nb_bindings)]


@pytest.mark.gpu
def test_engine_with_and_without_the_pair_is_bit_identical(gpu, monkeypatch):
    """YOLOv8n at 2 x 3 x 96 x 96, static tactics: the marked engine (one launch for ops 3 and 4) against the same plan lowered with TRTX_BNECK_PAIR=0, and
    with TRTX_STEM_PAIR=0 on top; one profile row per op either way, the first op of the pair reporting no kernel; a batch below the largest; three contexts
    on three streams return what one context returns."""
    import torch
    from tensorrtx_amd import engine, synth
    from util import synth_wts
    monkeypatch.setenv("TRTX_TUNE", "0")
    path, _ = synth_wts("yolov8n")
    B, S = 2, 96
    plan = engine.build_plan("yolov8n", path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    ops_on = engine.describe_plan(plan, lowered=True)["ops"]
    assert [k for k, o in enumerate(ops_on) if o.get("bneck_pair")] == [4]
    x = torch.from_numpy(synth.images(B, S, S, seed=3)).to(gpu)
    engines = {}
    try:
        engines["on"] = engine.Engine(plan)
        monkeypatch.setenv("TRTX_BNECK_PAIR", "0")
        assert not any(o.get("bneck_pair") for o in engine.describe_plan(plan, lowered=True)["ops"])
        engines["off"] = engine.Engine(plan)
        monkeypatch.setenv("TRTX_STEM_PAIR", "0")
        engines["both_off"] = engine.Engine(plan)
        monkeypatch.delenv("TRTX_BNECK_PAIR")
        monkeypatch.delenv("TRTX_STEM_PAIR")
        res, one = {}, {}
        for name, e in engines.items():
            outs = _outputs(e, B, gpu)
            e.enqueue(B, [x if t is None else t for t in outs])
            first = _outputs(e, B, gpu)
            e.enqueue(1, [x if t is None else t for t in first])           # a batch below the largest
            torch.cuda.synchronize()
            res[name], one[name] = outs, first
            rows = e.profile(B, [x if t is None else t for t in _outputs(e, B, gpu)])
            assert len(rows) == len(ops_on) and [r["kind"] for r in rows] == [o["kind"] for o in ops_on]
            # the fused launch is timed in the marked op's row and the op before it launches nothing; the two-launch form times both
            assert rows[4]["kernel_ms"] > 0 and (rows[3]["kernel_ms"] <= 0) == (name == "on"), (name, rows[3], rows[4])
        on = engines["on"]
        for other in ("off", "both_off"):
            for i in range(on.nb_bindings):
                if on.is_input[i]:
                    continue
                for got, want in ((res["on"][i], res[other][i]), (one["on"][i], one[other][i])):
                    a, b = got.view(torch.int32), want.view(torch.int32)
                    assert torch.equal(a, b), (other, on.names[i], int((a != b).sum()))
                if on.names[i].startswith("head"):
                    assert not torch.isnan(res[other][i]).any()     # (every element of a head tensor is written: not a comparison of sentinels)
        # three contexts in flight on three streams, the same input
        ctxs = [on.create_context() for _ in range(3)]
        streams = [torch.cuda.Stream(device=gpu) for _ in range(3)]
        many = [_outputs(on, B, gpu) for _ in range(3)]
        torch.cuda.synchronize()
        for c, s, outs in zip(ctxs, streams, many):
            c.enqueue(B, [x if t is None else t for t in outs], stream=s.cuda_stream)
        torch.cuda.synchronize()
        for outs in many:
            for i in range(on.nb_bindings):
                if not on.is_input[i]:
                    assert torch.equal(outs[i].view(torch.int32), res["on"][i].view(torch.int32)), on.names[i]
    finally:
        for e in engines.values():
            e.close()


@pytest.mark.gpu
def test_pair_takes_a_channel_offset_and_refuses_an_output_on_its_input(gpu, layers):
    """in_coff: the whole 48-wide buffer and a channel offset instead of a slice pointer.  The fused launch cannot run in place (other workgroups still read
    the pixels a workgroup stores): an output that lies on the input channels is an invalid argument, refused before anything is launched."""
    import torch
    from tensorrtx_amd import capi
    N, H, W = SHAPES[1]
    wide = torch.full((N, H, W, 48), -7.0, dtype=torch.float16, device=gpu)
    wide[..., 16:32] = _input(gpu, N, H, W)
    before = wide.clone()
    want = _two_launches(wide[..., 16:32].contiguous(), layers, "silu", True)
    args = (layers["w1"], layers["b1"], layers["w2"], layers["b2"])
    capi.conv_bneck_pair_f16(wide, *args, in_coff=16, out=wide[..., 32:], out_ld=48)
    torch.cuda.synchronize()
    assert torch.equal(wide[..., 32:].contiguous().view(torch.int16), want.view(torch.int16))
    assert torch.equal(wide[..., :32].contiguous().view(torch.int16), before[..., :32].contiguous().view(torch.int16))
    x = wide[..., 16:32]
    dense = x.contiguous()
    for out, ld, shortcut in ((x, 48, False), (x, 48, True), (wide[..., 24:40], 48, True), (wide[..., 8:24], 48, False), (dense, 16, False)):
        src = dense if out is dense else x
        with pytest.raises(capi.TrtxError) as e:
            capi.conv_bneck_pair_f16(src, *args, shortcut=shortcut, out=out, out_ld=ld)
        assert e.value.status == 1   # TRTX_ERR_INVALID
    with pytest.raises(capi.TrtxError):
        capi.conv_bneck_pair_f16(wide, *args, in_coff=12, out=wide[..., 32:], out_ld=48)   # not a 16-byte boundary
    # the slices next to the input on either side are fine
    for lo in (0, 32):
        capi.conv_bneck_pair_f16(x, *args, out=wide[..., lo:lo + 16], out_ld=48)
        torch.cuda.synchronize()
        assert torch.equal(wide[..., lo:lo + 16].contiguous().view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("shortcut", [False, True])
def test_the_executors_form_falls_back_to_two_launches_in_place(gpu, layers, shortcut):
    """What the engine issues at a marked op (conv_bneck_pair_or_two_f16): the fused launch where the kernel takes the pointers - the tensor between the two
    layers is then never written - and BOTH convolutions, the first one included, where it does not: here an output placed on the input, which an arena may
    do for a pair of launches.  Either way the bits of the two launches."""
    import torch
    from tensorrtx_amd import capi
    N, H, W = SHAPES[2]                      # several tiles per image: in place the fused kernel would read pixels other workgroups have stored
    x = _input(gpu, N, H, W)
    want = _two_launches(x, layers, "silu", shortcut)
    capi.conv_force_tactic(MAIN_K_ORDER)
    try:
        mid_want = capi.conv2d_nhwc_f16(x, layers["w1"], layers["b1"], 16, 3, 3, 1, 1, act1="silu")
    finally:
        capi.conv_force_tactic(None)
    args = (layers["w1"], layers["b1"], layers["w2"], layers["b2"])
    # apart: one launch, `mid` untouched
    mid = torch.full((N, H, W, 16), -7.0, dtype=torch.float16, device=gpu)
    got = capi.conv_bneck_pair_f16(x, *args, shortcut=shortcut, mid=mid)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and bool((mid == -7.0).all())
    # in place: two launches through `mid`
    buf = x.clone()
    capi.conv_bneck_pair_f16(buf, *args, shortcut=shortcut, mid=mid, out=buf)
    torch.cuda.synchronize()
    assert torch.equal(mid.view(torch.int16), mid_want.view(torch.int16)), "the first convolution was left out"
    assert torch.equal(buf.view(torch.int16), want.view(torch.int16))
    assert float(want.float().abs().max()) > 0.5


@pytest.mark.gpu
def test_engine_of_a_pair_without_shortcut_on_a_multi_tile_map(gpu, monkeypatch):
    """A network whose two-launch form runs the pair IN PLACE (the first convolution is the only reader of the pair's input, so the arena puts the second
    one's output on it; tests/test_bneck_pair_cpu.py pins both placements): the marked engine, whose arena keeps the two apart, returns the bits of the
    engine lowered with TRTX_BNECK_PAIR=0, on a 24 x 40 map (3 x 3 tiles per image), at the largest batch and below it."""
    import torch
    from tensorrtx_amd import engine
    from test_bneck_pair_cpu import _toy
    monkeypatch.setenv("TRTX_TUNE", "0")
    plan = _toy(shortcut=False, pointwise=True, hw=(96, 160))
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    marked = [k for k, o in enumerate(ops) if o.get("bneck_pair")]
    assert len(marked) == 1 and not ops[marked[0]]["residual"] and ops[marked[0]]["hw_in"] == [24, 40]
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn((2, 3, 96, 160), generator=g, dtype=torch.float32).to(gpu)
    engines = {}
    try:
        engines["on"] = engine.Engine(plan)
        monkeypatch.setenv("TRTX_BNECK_PAIR", "0")
        engines["off"] = engine.Engine(plan)
        monkeypatch.delenv("TRTX_BNECK_PAIR")
        res = {}
        for name, e in engines.items():
            res[name] = []
            for b in (2, 1):
                outs = _outputs(e, 2, gpu)
                e.enqueue(b, [x if t is None else t for t in outs])
                torch.cuda.synchronize()
                res[name].append(outs)
            rows = e.profile(2, [x if t is None else t for t in _outputs(e, 2, gpu)])
            k = marked[0]
            assert len(rows) == len(ops) and rows[k]["kernel_ms"] > 0 and (rows[k - 1]["kernel_ms"] <= 0) == (name == "on")
        on = engines["on"]
        for r_on, r_off in zip(res["on"], res["off"]):
            for i in range(on.nb_bindings):
                if not on.is_input[i]:
                    assert torch.equal(r_on[i].view(torch.int32), r_off[i].view(torch.int32)), on.names[i]
        y = res["off"][0][[i for i in range(on.nb_bindings) if not on.is_input[i]][0]]
        assert not torch.isnan(y).any() and float(y.abs().max()) > 0.01
    finally:
        for e in engines.values():
            e.close()
