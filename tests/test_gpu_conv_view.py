"""kernels/conv_view.hip on the device: every case of tests/conv_view_cases.py as one C-ABI launch (NaN beside the input view, a sentinel frame with one
extra image in front and behind around the output slice) and as an engine, against torch fp64 under the table's bound (nothing fitted), and the same
engines with TRTX_CONV_VIEW=0 on the direct kernel.  Every launch runs under a time limit of its own, and a HIP error ends the session."""
import contextlib
import faulthandler

import numpy as np
import pytest
import torch

from tensorrtx_amd import capi, engine
from tests import conv_view_cases as vc

pytestmark = pytest.mark.gpu
SENTINEL = -1234.0
UNSUPPORTED = 4   # TRTX_ERR_UNSUPPORTED


@contextlib.contextmanager
def _launch(what, seconds=60):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:   # the device has faulted: every later launch would run on a broken context
            pytest.exit(f"HIP error after {what}: {e}", returncode=3)
    finally:
        faulthandler.cancel_dump_traceback_later()


def _view(a_nchw, off, c, gpu):
    """channels [off, off + c) of the NHWC tensor, every other channel NaN"""
    t = torch.from_numpy(np.ascontiguousarray(a_nchw.transpose(0, 2, 3, 1))).half()
    t[..., :off] = float("nan")
    t[..., off + c:] = float("nan")
    return t.to(gpu)[..., off:off + c]


def _check(case, got_nchw, what, batch=None):
    ref, bound = (t[:batch] for t in vc.reference(case))
    err = (got_nchw.double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f"{case.name} {what}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
    assert torch.isfinite(got_nchw).all() and (err <= bound).all(), (what, ratio, int((err > bound).sum()), err.numel())


@pytest.mark.parametrize("case", vc.CASES, ids=lambda c: c.name)
def test_single_launch_matches_fp64_and_stays_inside_its_slice(gpu, case):
    d = vc.gen(case)
    off, ld = case.out_view if case.out_view else (6, 6 + case.Cout + 10)
    xg = _view(d["x"], case.in_view[0], case.Cin, gpu)
    rg = _view(d["r"], case.res_view[0], case.Cout, gpu) if case.res_view else None
    wg = torch.from_numpy(capi.pack_conv_weights_view_f16(d["w"]).view(np.int16)).to(gpu)
    buf = torch.full((case.N + 2, case.H, case.W, ld), SENTINEL, dtype=torch.float16, device=gpu)
    with _launch(case.name):
        capi.conv2d_view_nhwc_f16(xg, wg, torch.from_numpy(d["b"]).to(gpu), case.Cout, case.k, case.k // 2, case.act, rg, "none",
                                  out=buf[1:case.N + 1, :, :, off:off + case.Cout], out_ld=ld)
    b = buf.cpu()
    got = b[1:case.N + 1, :, :, off:off + case.Cout].clone()
    b[1:case.N + 1, :, :, off:off + case.Cout] = SENTINEL
    assert bool((b == SENTINEL).all()), "written outside the slice"
    _check(case, got.permute(0, 3, 1, 2), "C ABI")


# every case at its maximum batch on both kernels (with TRTX_CONV_VIEW=0 the bound rests on no property of the new one), and one below it
@pytest.mark.parametrize("case,off,batch", [(c, o, c.N) for c in vc.CASES for o in (False, True)] + [(vc.BY_NAME["c90_3x3"], False, 2)],
                         ids=lambda v: getattr(v, "name", {False: "view", True: "direct"}.get(v, v)))
def test_engine_matches_fp64(gpu, case, off, batch, monkeypatch):
    if off:
        monkeypatch.setenv("TRTX_CONV_VIEW", "0")
    plan, c = vc.build_plan(case)
    assert not c["igemm"] and (("view" not in c) if off else (c.get("view") is True)), c
    d = vc.gen(case)
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


@pytest.mark.parametrize("what,kw", [("odd Cin", dict(cin=59)), ("odd output offset", dict(at=7)), ("stride 2", dict(stride=2)),
                                     ("5x5 filter", dict(k=5)), ("Cin above the cap", dict(cin=258))])
def test_refusals_launch_nothing(gpu, what, kw):
    """TRTX_ERR_UNSUPPORTED and an untouched output.  The launch entry has no stride argument (its stride is 1): stride 2 goes to the predicate's own
    C-ABI face, which launches nothing by construction."""
    cin, k, at, stride = kw.get("cin", 60), kw.get("k", 3), kw.get("at", 6), kw.get("stride", 1)
    N, H, W, cout = 2, 5, 7, 60
    assert capi.lib().trtx_conv_view_supported(N, H, W, 60, 60, 320, cout, 6, 76, 3, 1, 1, 1, 1, 0, 0, 0) == 1
    assert capi.lib().trtx_conv_view_supported(N, H, W, cin, 60, 320, cout, at, 76, k, stride, k // 2, 1, 1, 0, 0, 0) == 0, what
    if stride != 1:
        return
    x = torch.zeros((N, H, W, 320), dtype=torch.float16, device=gpu)[..., 60:60 + cin]
    wg = torch.from_numpy(capi.pack_conv_weights_view_f16(np.zeros((cout, cin, k, k), np.float32)).view(np.int16)).to(gpu)
    buf = torch.full((N, H, W, 76), SENTINEL, dtype=torch.float16, device=gpu)
    with _launch(what):
        st = capi.conv2d_view_nhwc_f16(x, wg, None, cout, k, k // 2, out=buf[..., at:at + cout], out_ld=76, status_only=True)
    assert st == UNSUPPORTED and bool((buf == SENTINEL).all()), (what, st)
