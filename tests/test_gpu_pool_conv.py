"""YOLOv9's AConv / ADown halves as one launch each (kernels/conv_pool.hip) on the device: the table of tests/pool_conv_cases.py against its fp64 reference and derived
bound, contiguous and as channel slices of framed buffers; the refusals; the ops inside plans ("pool_conv" ops and no "pool", TRTX_POOL_CONV=0)."""
import pytest
import torch

from tensorrtx_amd import capi, engine
from tests import pool_conv_cases as pc
from tests.util import SENTINEL, guarded_slice, outside_untouched, sync, time_limit

pytestmark = pytest.mark.gpu
UNSUPPORTED, INVALID = 4, 1


def _launch(c, d, gpu, sliced, images=None):
    """-> (output on the host, whether everything around the output is untouched and the input is unchanged); sliced: channel slices of wider buffers"""
    B = images or c.B
    off = (8, 16, 24) if sliced else (0, 0, 0)   # first channel of in / out, channels beyond each slice
    x = guarded_slice((B, c.H, c.W, c.cin), off[0], c.cin + off[2], torch.float16, gpu, float("nan"))[1]
    ob, o = guarded_slice((B, c.H // 2, c.W // 2, c.cout), off[1], c.cout + off[2], torch.float16, gpu)
    x.copy_(d["x"][:B])
    x0 = x.clone()
    with time_limit():
        capi.conv_pool_f16(x, d["w"].numpy(), d["bias"].to(gpu), c.mode, "silu", out=o, out_ld=o.stride(2))
        sync(c.name)
    return o.cpu(), torch.equal(x, x0) and outside_untouched(ob, off[1], c.cout)[0]


@pytest.mark.parametrize("name", list(pc.CASES))
def test_pool_conv_matches_fp64_in_both_layouts(gpu, name):
    c, (d, y, bound) = pc.CASES[name], pc.reference(name)
    got, clean = _launch(c, d, gpu, False)
    got_s, clean_s = _launch(c, d, gpu, True)
    err = (got.double() - y).abs()
    print(f"{name}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
    assert clean and clean_s, "the input changed, or something outside the output slice was written"
    assert torch.equal(got, got_s), "the contiguous and the sliced layout differ"
    assert torch.isfinite(got).all() and (err <= bound).all(), ((err / bound).max().item(), int((err > bound).sum()))
    if c.B == 3:
        assert torch.equal(_launch(c, d, gpu, False, images=1)[0][0], got[0]), "image 0 of the batch of 3 differs from the same image run alone"


@pytest.mark.parametrize("what,status", [("cin12", UNSUPPORTED), ("map1xW", UNSUPPORTED), ("ld_out", UNSUPPORTED), ("overlap", INVALID)])
def test_refusals_return_their_status_and_write_nothing(gpu, what, status):
    cin, H = 12 if what == "cin12" else 16, 1 if what == "map1xW" else 8
    buf = torch.full((2, H, 8, 32), SENTINEL, dtype=torch.float16, device=gpu)   # in: channels 0 .. 15; overlap: out = the first bytes of the same buffer
    ho = max(H // 2, 1)
    out = buf.view(-1)[:2 * ho * 4 * 16].view(2, ho, 4, 16) if what == "overlap" else torch.full((2, ho, 4, 16), SENTINEL, dtype=torch.float16, device=gpu)
    st = capi.conv_pool_f16(buf[..., :cin], torch.ones(16, cin, 3, 3).numpy(), None, "avg_c3", out=out, out_ld=12 if what == "ld_out" else 16, status_only=True)
    sync(what)
    assert st == status and bool((buf == SENTINEL).all()) and bool((out == SENTINEL).all())


def _run(plan, x, B, shape):
    eng = engine.Engine(plan)
    y = torch.empty((B, *shape), dtype=torch.float32, device=x.device)
    with time_limit():
        eng.enqueue(B, [x[:B].contiguous(), y])
        sync("downsampler plan")
    eng.close()
    return y.cpu()


@pytest.mark.parametrize("kind,modes", [("adown", ["avg_c3", "avgmax_c1"]), ("aconv", ["avg_c3"])])
def test_downsampler_plans_run_pool_conv_ops(gpu, kind, modes, monkeypatch):
    kw, B = dict(B=4, C=32, H=12, W=14, cout=48), 4
    x = torch.from_numpy(pc._rng(kind, "x").standard_normal((B, kw["C"], kw["H"], kw["W"])).astype("float32"))
    monkeypatch.setenv("TRTX_POOL_CONV", "2")   # read at every lowering: the build's and the engine's (unset, the lowering declines what measured slower)
    plan, layers = pc.down_net(kind, **kw)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    assert [o["mode"] for o in ops if o["kind"] == "pool_conv"] == modes and not any(o["kind"] in ("pool", "conv") for o in ops), ops
    y, bound = pc.net_reference(x, layers)
    got = _run(plan, x.to(gpu), B, y.shape[1:])
    err = (got.double() - y).abs()
    print(f"{kind}: max err / bound {(err / bound).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), (err / bound).max().item()
    monkeypatch.setenv("TRTX_POOL_CONV", "0")
    plan0, _ = pc.down_net(kind, **kw)
    kinds0 = [o["kind"] for o in engine.describe_plan(plan0, lowered=True)["ops"]]
    assert "pool_conv" not in kinds0 and kinds0.count("pool") == len(modes) and kinds0.count("conv") == len(modes), kinds0
    diff = (_run(plan0, x.to(gpu), B, y.shape[1:]).double() - got.double()).abs()
    assert (diff <= 2 * bound).all(), (diff / bound).max().item()
