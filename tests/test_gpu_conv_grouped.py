"""The grouped-convolution kernel (kernels/conv_grouped.hip) on the device: every case of tests/conv_grouped_cases.py as a single launch
through the C ABI and as an engine, against the table's torch fp64 reference under its per-element bound (nothing fitted), and the same
engines with TRTX_CONV_GROUPED=0, where the direct kernel must pass the same comparison.

A C-ABI launch stores into a channel slice of a wider buffer that carries one extra image in front and one behind, all pre-filled with a
sentinel (as tests/test_gpu_conv_geometry.py does): nothing outside the slice may change.  Every launch runs under a time limit of its own, and
a HIP error ends the session."""
import contextlib
import faulthandler

import numpy as np
import pytest
import torch

from tensorrtx_amd import capi, engine
from tests import conv_grouped_cases as gc

pytestmark = pytest.mark.gpu

SENTINEL = -1234.0
STEP_LIMIT = 60   # seconds for one launch and its synchronisation (they take milliseconds)


@contextlib.contextmanager
def _time_limit(seconds=STEP_LIMIT):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # the device has faulted: every later launch would run on a broken context
        pytest.exit(f"HIP error after {what}: {e}", returncode=3)


def _nhwc(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).half().to(gpu)


def _launch(case, d, gpu, x=None, w=None):
    """one launch into a sentinel-framed slice -> (clean, [N, H, W, Cout] fp16 CPU)"""
    off, ld = case.out_view if case.out_view else (8, 8 + case.Cout + 8)
    xg = _nhwc(d["x"] if x is None else x, gpu)
    if case.in_view:
        xg = xg[..., case.in_view[0]:case.in_view[0] + case.Cin]
    wg = torch.from_numpy(capi.pack_conv_weights_grouped_f16(d["w"] if w is None else w).view(np.int16)).to(gpu)
    bg = torch.from_numpy(d["b"]).to(gpu)
    rg = _nhwc(d["r"], gpu) if case.res else None
    buf = torch.full((case.N + 2, case.H, case.W, ld), SENTINEL, dtype=torch.float16, device=gpu)
    view = buf[1:case.N + 1, :, :, off:off + case.Cout]
    with _time_limit():
        capi.conv2d_grouped_nhwc_f16(xg, wg, bg, case.Cout, case.groups, case.k, case.pad, case.act, rg, "none", out=view, out_ld=ld)
        _sync(case.name)
    b = buf.cpu()
    inside = b[1:case.N + 1, :, :, off:off + case.Cout].clone()
    b[1:case.N + 1, :, :, off:off + case.Cout] = SENTINEL
    return bool((b == SENTINEL).all()), inside


def _check(case, got_nchw, what):
    ref, bound = gc.reference(case)
    err = (got_nchw.double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f"{case.name} {what}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
    assert torch.isfinite(got_nchw).all(), what
    assert (err <= bound).all(), (what, ratio, int((err > bound).sum()), err.numel())


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_single_launch_matches_fp64_and_stays_inside_its_slice(gpu, case):
    clean, got = _launch(case, gc.gen(case), gpu)
    assert clean, "written outside the slice"
    _check(case, got.permute(0, 3, 1, 2), "C ABI")


def test_groups_do_not_leak_into_each_other(gpu):
    """group-permuted weights and inputs give the group-permuted output, bit for bit"""
    case = gc.BY_NAME["g4_3x3_13x17"]
    d = gc.gen(case)
    perm = [2, 0, 3, 1]
    cg, og = case.cin_g, case.Cout // case.groups
    xi = np.concatenate([np.arange(g * cg, (g + 1) * cg) for g in perm])
    oi = np.concatenate([np.arange(g * og, (g + 1) * og) for g in perm])
    _, base = _launch(case, d, gpu)
    d2 = dict(d, b=np.ascontiguousarray(d["b"][oi]))
    _, got = _launch(case, d2, gpu, x=np.ascontiguousarray(d["x"][:, xi]), w=np.ascontiguousarray(d["w"][oi]))
    assert torch.equal(got, base[..., torch.from_numpy(oi)])


def _run_engine(case, plan, gpu, batch=None):
    d = gc.gen(case)
    batch = batch or case.N
    e = engine.Engine(plan)
    try:
        bufs = []
        for i in range(e.nb_bindings):
            n = int(np.prod(e.dims[i])) * case.N
            if e.is_input[i]:
                bufs.append(torch.from_numpy(np.ascontiguousarray(d[e.names[i]]).reshape(-1)).to(gpu))
                assert bufs[-1].numel() == n
            else:
                bufs.append(torch.full((n,), float("nan"), dtype=torch.float32, device=gpu))
        with _time_limit():
            e.enqueue(batch, bufs)
            _sync(case.name)
        out_c = case.out_view[1] if case.out_view else case.Cout
        return bufs[e.names.index("y")].cpu().reshape(case.N, out_c, case.H, case.W), d
    finally:
        e.close()


def _check_engine(case, y, d, batch, what):
    ref, bound = gc.reference(case)
    got = y[:batch, :case.Cout]
    err = (got.double() - ref[:batch]).abs()
    ratio = (err / bound[:batch]).max().item()
    print(f"{case.name} {what}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
    assert torch.isfinite(got).all() and (err <= bound[:batch]).all(), (what, ratio, int((err > bound[:batch]).sum()))
    assert torch.isnan(y[batch:]).all(), "written beyond the samples of the enqueue"
    if case.out_view:   # the neighbour's channels of the concat buffer: exactly what their own producer wrote
        assert torch.equal(y[:batch, case.Cout:], torch.from_numpy(d["z"][:batch]))


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_engine_matches_fp64(gpu, case):
    plan = gc.build_plan(case)
    (c,) = gc.convs_of(plan)
    assert c.get("grouped") is True
    y, d = _run_engine(case, plan, gpu)
    _check_engine(case, y, d, case.N, "engine")


def test_engine_below_its_maximum_batch(gpu):
    case = gc.BY_NAME["g4_3x3_13x17"]
    y, d = _run_engine(case, gc.build_plan(case), gpu, batch=2)
    _check_engine(case, y, d, 2, "engine, batch 2 of 3")


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_direct_kernel_passes_the_same_comparison(gpu, case, monkeypatch):
    monkeypatch.setenv("TRTX_CONV_GROUPED", "0")
    plan = gc.build_plan(case)
    (c,) = gc.convs_of(plan)
    assert "grouped" not in c and not c["igemm"]
    y, d = _run_engine(case, plan, gpu)
    _check_engine(case, y, d, case.N, "engine on the direct kernel")
