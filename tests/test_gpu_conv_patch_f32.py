"""kernels/conv_patch_f32.hip on the device: every case of tests/conv_patch_f32_cases.py as one C-ABI launch (NaN beside the input view, a sentinel frame with
one extra image in front and behind around the output slice) and as an fp32 engine with TRTX_CONV_F32_PATCH=1 and unset (the direct kernel), against torch
fp64 under the table's bound (nothing fitted).  Every launch runs under a time limit of its own, and a HIP error ends the session."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import capi, engine
from tests import conv_patch_f32_cases as pc
from tests.test_gpu_conv_view import _launch

pytestmark = pytest.mark.gpu
SENTINEL = -1234.0
UNSUPPORTED = 4   # TRTX_ERR_UNSUPPORTED


def _view(a_nchw, off, c, gpu):
    """channels [off, off + c) of the NHWC fp32 tensor, every other channel NaN"""
    t = torch.from_numpy(np.ascontiguousarray(a_nchw.transpose(0, 2, 3, 1)))
    t[..., :off] = t[..., off + c:] = float("nan")
    return t.to(gpu)[..., off:off + c]


def _check(case, got_nchw, what, batch=None):
    ref, bound = (t[:batch] for t in pc.reference(case))
    err = (got_nchw.double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f"{case.name} {what}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
    assert torch.isfinite(got_nchw).all() and (err <= bound).all(), (what, ratio, int((err > bound).sum()), err.numel())


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_single_launch_matches_fp64_and_stays_inside_its_slice(gpu, case):
    d = pc.gen(case)
    off, ld = case.out_view if case.out_view else (4, 4 + case.Cout + 8)
    xg = _view(d["x"], (case.in_view or (0,))[0], case.Cin, gpu)
    rg = _view(d["r"], case.res_view[0], case.Cout, gpu) if case.res_view else None
    wg = torch.from_numpy(capi.pack_conv_weights_patch_f32(d["w"], case.groups)).to(gpu)
    buf = torch.full((case.N + 2, case.H, case.W, ld), SENTINEL, dtype=torch.float32, device=gpu)
    with _launch(case.name):
        capi.conv2d_patch_nhwc_f32(xg, wg, torch.from_numpy(d["b"]).to(gpu), case.Cout, case.groups, case.k, case.k // 2, case.act, rg, "none",
                                   out=buf[1:case.N + 1, :, :, off:off + case.Cout], out_ld=ld)
    b = buf.cpu()
    got = b[1:case.N + 1, :, :, off:off + case.Cout].clone()
    b[1:case.N + 1, :, :, off:off + case.Cout] = SENTINEL
    assert bool((b == SENTINEL).all()), "written outside the slice"
    _check(case, got.permute(0, 3, 1, 2), "C ABI")


# every case at its maximum batch on both kernels (with the switch unset the bound rests on no property of the new one), and one below it
@pytest.mark.parametrize("case,on,batch", [(c, o, c.N) for c in pc.CASES for o in (True, False)] + [(pc.BY_NAME["g4_3x3"], True, 2)],
                         ids=lambda v: getattr(v, "name", {True: "patch_f32", False: "direct"}.get(v, v)))
def test_engine_matches_fp64(gpu, case, on, batch, monkeypatch):
    if on:
        monkeypatch.setenv("TRTX_CONV_F32_PATCH", "1")
    plan, ops = pc.build_plan(case)
    (c,) = [o for o in ops if o["kind"] == "conv"]
    assert not c["igemm"] and (c.get("patch_f32") is True) == on, c
    d = pc.gen(case)
    e = engine.Engine(plan)
    try:
        bufs = [torch.from_numpy(np.ascontiguousarray(d[e.names[i]]).reshape(-1)).to(gpu) if e.is_input[i] else
                torch.full((int(np.prod(e.dims[i])) * case.N,), float("nan"), dtype=torch.float32, device=gpu) for i in range(e.nb_bindings)]
        with _launch(case.name):
            e.enqueue(batch, bufs)
        y = bufs[e.names.index("y")].cpu().reshape(case.N, -1, case.H, case.W)
    finally:
        e.close()
    at = case.out_view[0] if case.out_view else 0
    _check(case, y[:batch, at:at + case.Cout], "engine", batch)
    assert torch.isnan(y[batch:]).all(), "written beyond the samples of the enqueue"
    if case.out_view:   # the neighbour's channels of the concat buffer: exactly what their own producer wrote
        assert torch.equal(y[:batch, :at], torch.from_numpy(d["z"][:batch]))


@pytest.mark.parametrize("what,kw", [("dilation 2", dict(dilation=2)), ("5x5 filter", dict(k=5)), ("9 groups", dict(groups=9, cin=144, cout=144)),
                                     ("Cin_g 6", dict(groups=2, cin=12, cout=32))])
def test_refusals_launch_nothing(gpu, what, kw):
    """TRTX_ERR_UNSUPPORTED and an untouched output.  The launch entry has no dilation argument: a dilated filter goes to the predicate, and to the launch as its padding."""
    cin, cout, groups, k, dil = kw.get("cin", 64), kw.get("cout", 64), kw.get("groups", 4), kw.get("k", 3), kw.get("dilation", 1)
    N, H, W, pad = 2, 5, 7, dil * (k // 2)
    assert capi.lib().trtx_conv_patch_f32_supported(N, H, W, 64, 3, 160, 64, 4, 76, 3, 1, 1, 1, 4, 0, 0, 0) == 1
    assert capi.lib().trtx_conv_patch_f32_supported(N, H, W, cin, 3, 160, cout, 4, cout + 12, k, 1, pad, dil, groups, 0, 0, 0) == 0, what
    x = torch.zeros((N, H, W, 160), dtype=torch.float32, device=gpu)[..., 3:3 + cin]
    wg = torch.from_numpy(capi.pack_conv_weights_patch_f32(np.zeros((cout, cin // groups, k, k), np.float32), groups)).to(gpu)
    buf = torch.full((N, H, W, cout + 12), SENTINEL, dtype=torch.float32, device=gpu)
    with _launch(what):
        st = capi.conv2d_patch_nhwc_f32(x, wg, None, cout, groups, k, pad, out=buf[..., 4:4 + cout], out_ld=cout + 12, status_only=True)
    assert st == UNSUPPORTED and bool((buf == SENTINEL).all()), (what, st)
