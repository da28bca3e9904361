"""The fused stem pair on the GPU (kernels/conv_stem_pair.hip): the 3x3 / 2 stem and the 16 -> 32 3x3 / 2 convolution behind it in one launch return, bit
for bit, what the stem kernel followed by the implicit-GEMM kernel's main K order returns - at the op level over shapes that exercise partial tiles,
image seams, odd intermediate sizes and a strided destination, and at the engine level with the lowering switch on and off."""
import numpy as np
import pytest

# N, H, W of the fp32 NCHW input -> intermediate -> output; what the shape catches
SHAPES = [
    (1, 20, 24),     # 10 x 12 -> 5 x 6: everything inside one partial tile
    (2, 64, 64),     # 32 x 32 -> 16 x 16: exact tiles, an image seam inside a workgroup's tile run
    (3, 70, 132),    # 35 x 66 -> 18 x 33: odd intermediate height (the bottom padding row is a zero, not a stem value), ragged tiles, runs crossing images
    (2, 38, 68),     # 19 x 34 -> 10 x 17: odd height and a width one past a 16-pixel fragment
]
MAIN_K_ORDER = (32, 32, 128, 1, 1, 0)   # column tile 32, 32-wide k-steps, 128-row tiles, no wave-split-K, no weight-stationary kernel: the default tactic's K order


@pytest.fixture(scope="module")
def layers(gpu):
    """the two layers' weights (random normal, non-zero biases) in both kernels' layouts, shared by the op-level tests"""
    import torch
    from tensorrtx_amd import capi
    rng = np.random.default_rng(11)
    w0 = (rng.standard_normal((16, 3, 3, 3)) * (2.0 / 27) ** 0.5).astype(np.float32)
    w1 = (rng.standard_normal((32, 16, 3, 3)) * (2.0 / 144) ** 0.5).astype(np.float32)
    packed, cout_pad, kpad, _ = capi.pack_conv_weights_f16(w1, cin_pad=16)
    assert (cout_pad, kpad) == (32, 160)
    return dict(stem_w=torch.from_numpy(capi.stem_weights(w0)).to(gpu), stem_b=torch.from_numpy(rng.standard_normal(16).astype(np.float32)).to(gpu),
                conv_w=torch.from_numpy(packed.view(np.int16)).to(gpu), conv_b=torch.from_numpy(rng.standard_normal(32).astype(np.float32)).to(gpu))


def _two_launches(x, L, act):
    from tensorrtx_amd import capi
    mid = capi.conv_stem_nchw_f16(x, L["stem_w"], L["stem_b"], 3, 2, 1, act=act)
    capi.conv_force_tactic(MAIN_K_ORDER)
    try:
        return capi.conv2d_nhwc_f16(mid, L["conv_w"], L["conv_b"], 32, 3, 3, 2, 1, act1=act)
    finally:
        capi.conv_force_tactic(None)


def _input(gpu, N, H, W):
    import torch
    g = torch.Generator(device="cpu").manual_seed(N * 100000 + H * 100 + W)
    return torch.randn((N, 3, H, W), generator=g, dtype=torch.float32).to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_pair_equals_stem_then_conv_bit_for_bit(gpu, layers, N, H, W):
    import torch
    from tensorrtx_amd import capi
    x = _input(gpu, N, H, W)
    want = _two_launches(x, layers, "silu")
    got = capi.conv_stem_pair_f16(x, layers["stem_w"], layers["stem_b"], layers["conv_w"], layers["conv_b"])
    torch.cuda.synchronize()
    assert got.shape == want.shape == (N, ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1, 32)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got.view(torch.int16) != want.view(torch.int16)).sum())
    assert float(want.float().abs().max()) > 0.5    # (not a comparison of zeros)


@pytest.mark.gpu
def test_pair_writes_a_channel_slice_of_a_wider_buffer(gpu, layers):
    import torch
    from tensorrtx_amd import capi
    N, H, W = SHAPES[2]
    x = _input(gpu, N, H, W)
    want = _two_launches(x, layers, "silu")
    wide = torch.full((N, want.shape[1], want.shape[2], 48), -7.0, dtype=torch.float16, device=gpu)   # sentinel
    capi.conv_stem_pair_f16(x, layers["stem_w"], layers["stem_b"], layers["conv_w"], layers["conv_b"], out=wide[..., 8:], out_ld=48)
    torch.cuda.synchronize()
    assert torch.equal(wide[..., 8:40].contiguous().view(torch.int16), want.view(torch.int16))
    assert bool((wide[..., :8] == -7.0).all()) and bool((wide[..., 40:] == -7.0).all())


@pytest.mark.gpu
def test_pair_with_relu(gpu, layers):
    import torch
    from tensorrtx_amd import capi
    N, H, W = SHAPES[3]
    x = _input(gpu, N, H, W)
    want = _two_launches(x, layers, "relu")
    got = capi.conv_stem_pair_f16(x, layers["stem_w"], layers["stem_b"], layers["conv_w"], layers["conv_b"], stem_act="relu", conv_act="relu")
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and float(want.float().max()) > 0.5 and float(want.float().min()) == 0.0


def _outputs(e, B, gpu):
    import torch
    return [None if e.is_input[i] else torch.full((B * int(np.prod(e.dims[i])),), float("nan"), dtype=torch.float32, device=gpu) for i in range(e.nb_bindings)]


@pytest.mark.gpu
def test_engine_with_and_without_the_pair_is_bit_identical(gpu, monkeypatch):
    """YOLOv8n at 2 x 3 x 96 x 96, static tactics: the marked engine (one launch for the first two layers) against the same plan lowered with
    TRTX_STEM_PAIR=0; one profile row per op either way; camera frames (which keep the two launches) match the marked engine's own enqueue; three
    contexts on three streams return what one context returns."""
    import torch
    from tensorrtx_amd import engine, preproc, synth
    from util import synth_wts
    monkeypatch.setenv("TRTX_TUNE", "0")
    path, _ = synth_wts("yolov8n")
    B, S = 2, 96
    plan = engine.build_plan("yolov8n", path, batch=B, h=S, w=S, fp16=1, mark_heads=1)
    ops_on = engine.describe_plan(plan, lowered=True)["ops"]
    assert [k for k, o in enumerate(ops_on) if o.get("stem_pair")] == [1]
    x = torch.from_numpy(synth.images(B, S, S, seed=3)).to(gpu)
    engines = []
    try:
        on = engine.Engine(plan)
        engines.append(on)
        monkeypatch.setenv("TRTX_STEM_PAIR", "0")
        assert not any(o.get("stem_pair") for o in engine.describe_plan(plan, lowered=True)["ops"])
        off = engine.Engine(plan)
        engines.append(off)
        monkeypatch.delenv("TRTX_STEM_PAIR")
        res = {}
        for name, e in (("on", on), ("off", off)):
            outs = _outputs(e, B, gpu)
            e.enqueue(B, [x if t is None else t for t in outs])
            torch.cuda.synchronize()
            res[name] = outs
            rows = e.profile(B, [x if t is None else t for t in _outputs(e, B, gpu)])
            assert len(rows) == len(ops_on) and [r["kind"] for r in rows] == [o["kind"] for o in ops_on]
        for i in range(on.nb_bindings):
            if on.is_input[i]:
                continue
            a, b = res["on"][i].view(torch.int32), res["off"][i].view(torch.int32)
            assert torch.equal(a, b), (on.names[i], int((a != b).sum()))
            if on.names[i].startswith("head"):
                assert not torch.isnan(res["off"][i]).any()     # (every element of a head tensor is written: not a comparison of sentinels)
        # camera frames -> letterbox -> enqueue on the marked engine == enqueue_frames on it
        rng = np.random.default_rng(5)
        frames = [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).to(gpu) for h, w in ((120, 160), (97, 61))]
        two, one = _outputs(on, B, gpu), _outputs(on, B, gpu)
        xl = preproc.letterbox_batch(frames, S, S)
        on.enqueue(B, [xl if t is None else t for t in two])
        on.enqueue_frames(B, frames, one)
        torch.cuda.synchronize()
        for i in range(on.nb_bindings):
            if not on.is_input[i]:
                assert torch.equal(one[i].view(torch.int32), two[i].view(torch.int32)), on.names[i]
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
        for e in engines:
            e.close()
