"""YOLOv13's DSConv as one launch (kernels/conv_dw_pw.hip) on the device: the table of tests/dsconv_cases.py against its fp64 reference and derived bound, contiguous
and as channel slices of framed buffers; the executor's entry on both routes; the refusals; the op inside plans ("dsconv" ops, TRTX_DSCONV=0, batch independence)."""
import pytest
import torch

from tensorrtx_amd import capi, engine
from tests import dsconv_cases as dc
from tests.util import SENTINEL, guarded_slice, outside_untouched, sync, time_limit

pytestmark = pytest.mark.gpu
UNSUPPORTED, INVALID = 4, 1


def _launch(c, d, gpu, sliced, mid=None):
    """-> (output on the host, whether everything around the output is untouched and the inputs are unchanged); sliced: channel slices of wider buffers"""
    hw = dc.out_hw(c.H, c.W, c.k, c.s)
    off = (8, 16, 8, 24) if sliced else (0, 0, 0, 0)   # first channel of in / residual / out, channels beyond each slice
    x = guarded_slice((c.B, c.H, c.W, c.cin), off[0], c.cin + off[3], torch.float16, gpu, float("nan"))[1]
    r = guarded_slice((c.B, *hw, c.cout), off[1], c.cout + off[3], torch.float16, gpu, float("nan"))[1]
    ob, o = guarded_slice((c.B, *hw, c.cout), off[2], c.cout + off[3], torch.float16, gpu)
    x.copy_(d["x"])
    r.copy_(d["res"] if c.res else torch.zeros(()))
    x0, r0 = x.clone(), r.clone()
    with time_limit():
        capi.conv_dw_pw_f16(x, d["wd"].numpy(), d["wp"].numpy(), None if d["bias"] is None else d["bias"].to(gpu), c.k, c.s, c.act, r if c.res else None, out=o,
                            out_ld=o.stride(2), mid=mid, act2=c.act2)
        sync(c.name)
    return o.cpu(), torch.equal(x, x0) and torch.equal(r, r0) and outside_untouched(ob, off[2], c.cout)[0]


@pytest.mark.parametrize("name", list(dc.CASES))
def test_dsconv_matches_fp64_in_both_layouts(gpu, name):
    c, (d, y, bound) = dc.CASES[name], dc.reference(name)
    got, clean = _launch(c, d, gpu, False)
    got_s, clean_s = _launch(c, d, gpu, True)
    err = (got.double() - y).abs()
    print(f"{name}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
    assert clean and clean_s, "an input changed, or something outside the output slice was written"
    assert torch.equal(got, got_s), "the contiguous and the sliced layout differ"
    assert torch.isfinite(got).all() and (err <= bound).all(), ((err / bound).max().item(), int((err > bound).sum()))


@pytest.mark.parametrize("name", ["cin40_cout24_s2_odd", "cin136_cout264_passes", "cin32_cout136_passes"])   # admitted; two that the admission rule declines
def test_or_two_fuses_where_admitted_and_else_runs_two_launches_through_mid(gpu, name):
    c, (d, y, bound) = dc.CASES[name], dc.reference(name)
    fused, _ = _launch(c, d, gpu, False)   # the fused launch alone, on an output of its own
    mid = torch.full((c.B, *dc.out_hw(c.H, c.W, c.k, c.s), c.cin), SENTINEL, dtype=torch.float16, device=gpu)
    via = _launch(c, d, gpu, False, mid=mid)[0]
    if 16 <= c.cin <= 64 and 16 <= c.cout <= 64:   # admitted: the same launch again, `mid` left alone
        assert torch.equal(via, fused) and bool((mid == SENTINEL).all())
    else:
        err, diff = (via.double() - y).abs(), (via.double() - fused.double()).abs()
        print(f"{name}: two launches max err / bound {(err / bound).max().item():.3f}, against the fused launch {(diff / bound).max().item():.3f}")
        assert torch.equal(mid, capi.conv2d_dw_nhwc(d["x"].half().to(gpu), d["wd"].numpy(), None, c.k, c.s)), "`mid` must hold the fp16 depthwise result"
        assert (err <= bound).all() and (diff <= 2 * bound).all()


@pytest.mark.parametrize("what,status", [("dilation", UNSUPPORTED), ("cin12", UNSUPPORTED), ("bias_dw", UNSUPPORTED), ("ld_out", UNSUPPORTED), ("in_place", INVALID)])
def test_refusals_return_their_status_and_write_nothing(gpu, what, status):
    cin = 12 if what == "cin12" else 16
    buf = torch.full((2, 9, 9, 32), SENTINEL, dtype=torch.float16, device=gpu)   # in: channels 0 .. 15; in place: out = channels 8 .. 23 of the same pixels
    out = buf[..., 8:24] if what == "in_place" else torch.full((2, 9, 9, 16), SENTINEL, dtype=torch.float16, device=gpu)
    st = capi.conv_dw_pw_f16(buf[..., :cin], torch.ones(cin, 3, 3).numpy(), torch.ones(16, cin).numpy(), None, 3, 1, "silu", out=out,
                             out_ld=8 if what == "ld_out" else out.stride(2), dilation=2 if what == "dilation" else 1,
                             bias_dw=torch.ones(cin, device=gpu) if what == "bias_dw" else None, status_only=True)
    sync(what)
    assert st == status and bool((buf == SENTINEL).all()) and bool((out == SENTINEL).all())


NETS = {"c16_k3_k7": dict(C=16, H=24, W=20, k1=3, k2=7, shortcut=True, stride=1), "c64_k3_k3": dict(C=64, H=10, W=12, k1=3, k2=3, shortcut=True, stride=1),
        "c32_to_48_s2": dict(C=32, H=13, W=15, k1=3, k2=3, shortcut=False, stride=2, cout=48, single=True)}


def _run(plan, x, B, shape):
    eng = engine.Engine(plan)
    y = torch.empty((B, *shape), dtype=torch.float32, device=x.device)
    with time_limit():
        eng.enqueue(B, [x[:B].contiguous(), y])
        sync("dsbottleneck plan")
    eng.close()
    return y.cpu()


@pytest.mark.parametrize("name", list(NETS))
def test_dsbottleneck_plans_run_dsconv_ops(gpu, name, monkeypatch):
    kw, B = NETS[name], 8
    x = torch.from_numpy(dc._rng(name, "x").standard_normal((B, kw["C"], kw["H"], kw["W"])).astype("float32"))
    plan, layers = dc.dsbottleneck_net(B, **kw)
    ops = engine.describe_plan(plan, lowered=True)["ops"]
    assert [o["fused"] for o in ops if o["kind"] == "dsconv"] == [True] * len(layers) and not any(o["kind"] == "conv" for o in ops), ops
    y, bound = dc.net_reference(x, layers, kw["shortcut"])
    got = _run(plan, x.to(gpu), B, y.shape[1:])
    err = (got.double() - y).abs()
    print(f"{name}: max err / bound {(err / bound).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), (err / bound).max().item()
    assert torch.equal(_run(plan, x.to(gpu), 1, y.shape[1:])[0], got[0]), "image 0 of the batch of 8 differs from the same image run alone"
    monkeypatch.setenv("TRTX_DSCONV", "0")   # read at every lowering: the build's and the engine's
    plan0, _ = dc.dsbottleneck_net(B, **kw)
    kinds0 = [o["kind"] for o in engine.describe_plan(plan0, lowered=True)["ops"]]
    assert "dsconv" not in kinds0 and kinds0.count("conv") == 2 * len(layers), kinds0
    diff = (_run(plan0, x.to(gpu), B, y.shape[1:]).double() - got.double()).abs()
    assert (diff <= 2 * bound).all(), (diff / bound).max().item()
