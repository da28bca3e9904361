"""The convolution geometry table (tests/conv_cases.py) on the device: every case through the C ABI, on every launch configuration the
library lists for that exact geometry (and on no other), against the table's torch fp64 reference - every output element under the
per-element bound derived in tests/conv_cases.py, nothing fitted.

  * fp16: every tactic of conv2d_tactics; those with wsk == 1 and ws in (1, 3, 7, 8) walk K in the same order and must agree bit for bit;
  * fp32: every tile of conv2d_tactics_f32; all of them the same bits;
  * int8: the integer accumulator is exact; fp16 output under the per-element bound, int8 output exactly - but for the elements the
    reference itself marks as sitting on a rounding boundary, which may be one step off.

Nothing may be written outside: a launch stores into a channel slice of a wider buffer that carries one extra image in front and one
behind, all pre-filled with a sentinel.  Every fp16 and fp32 case runs in both layouts, one after the other: the slice starts at channel 8
of a row whose width is a multiple of 8 (16-byte stores; the only layout the special-case kernels ws 2, 3, 7, 8 take), and at channel 6 of
a row that is not (element-wise stores).  On the degenerate 3x3 maps the test asserts that what it forced contains tests/conv_cases.py's
EXPECT_WS, the same sets the host test demands of the lists.

Every launch runs under a time limit of its own (a watchdog that ends the process), and a HIP error ends the session: nothing more is
launched on a device that has hung or faulted."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import capi
from tests import conv_cases as cc
from tests.util import SENTINEL, STEP_LIMIT, sync as _sync, time_limit as _time_limit  # noqa: F401

pytestmark = pytest.mark.gpu


def _layouts(case):
    """(channel offset, row width) of the output slice: the aligned layout, then the misaligned one"""
    return [(8, (8 + case.Cout + 8 + 7) // 8 * 8), (6, (6 + case.Cout + 8 + 7) // 8 * 8 + 6)]


def _buffer(case, off, ld, dtype, gpu, sentinel=SENTINEL):
    Ho, Wo = case.out_hw
    buf = torch.full((case.N + 2, Ho, Wo, ld), sentinel, dtype=dtype, device=gpu)
    return buf, buf[1:case.N + 1, :, :, off:off + case.Cout]


def _untouched(case, buf, off, sentinel=SENTINEL):
    b = buf.cpu()
    inside = b[1:case.N + 1, :, :, off:off + case.Cout].clone()
    b[1:case.N + 1, :, :, off:off + case.Cout] = sentinel
    return bool((b == sentinel).all()), inside


def _report(case, eng, what, got, ref):
    err = (got.double() - ref.y).abs()
    ratio = (err / ref.bound).max().item()
    print(f"{case.name} {eng} {what}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
    return err, ratio


F16 = [c for c in cc.CASES if "f16" in c.engines]
F32 = [c for c in cc.CASES if "f32" in c.engines]
I8 = [c for c in cc.CASES if "i8" in c.engines]


@pytest.mark.parametrize("case", F16, ids=lambda c: c.name)
def test_conv_f16_every_tactic_matches_fp64(gpu, case):
    d = cc.gen_inputs(case.name)
    ref = cc.reference(case.name, "f16")
    packed, cout_pad, _, _ = capi.pack_conv_weights_f16(d["w"].numpy(), cin_pad=case.Cin)
    bias = torch.zeros(cout_pad)
    bias[:case.Cout] = d["bias"]
    xg, wg, bg = d["x"].half().to(gpu), torch.from_numpy(packed.view(np.int16)).to(gpu), bias.to(gpu)
    rg = d["res"].half().to(gpu) if case.res else None
    exact, failures, forced = None, [], set()
    try:
        for off, ld in _layouts(case):
            tactics = capi.conv2d_tactics(case.N, case.H, case.W, case.Cin, case.Cout, case.k, case.s, case.p, residual=case.res, ld_out=ld)
            assert tactics and len(set(tactics)) == len(tactics)
            for t in tactics:
                what = f"tactic {t} at channel {off} of {ld}"
                buf, view = _buffer(case, off, ld, torch.float16, gpu)
                capi.conv_force_tactic(t)
                with _time_limit():
                    capi.conv2d_nhwc_f16(xg, wg, bg, case.Cout, *case.k, case.s, case.p, case.act1, rg, case.act2, out=view, out_ld=ld)
                    _sync(f"{case.name} {what}")
                forced.add(t[4])
                clean, got = _untouched(case, buf, off)
                err, ratio = _report(case, "f16", what, got, ref)
                if not clean:
                    failures.append(f"{what} wrote outside its slice")
                if not torch.isfinite(got).all() or not (err <= ref.bound).all():
                    failures.append(f"{what}: max err / bound {ratio:.3f}, {int((err > ref.bound).sum())} of {err.numel()} elements beyond the bound")
                if t[3] == 1 and t[4] in (1, 3, 7, 8) and t[5] == 0:
                    if exact is None:
                        exact = (what, got)
                    elif not torch.equal(got, exact[1]):
                        failures.append(f"{what} is not bit-identical to {exact[0]}")
    finally:
        capi.conv_force_tactic(None)
    assert not failures, failures
    if case.name in cc.EXPECT_WS:
        assert cc.EXPECT_WS[case.name]["f16"] <= forced, (forced, "the special-case kernels this map is in the table for were not all run")


@pytest.mark.parametrize("case", F32, ids=lambda c: c.name)
def test_conv_f32_every_tile_is_the_same_bits_within_the_fp32_bound(gpu, case):
    d = cc.gen_inputs(case.name)
    ref = cc.reference(case.name, "f32")
    packed, cout_pad, _, _ = capi.pack_conv_weights_f32(d["w"].numpy(), cin_pad=case.Cin)
    bias = torch.zeros(cout_pad)
    bias[:case.Cout] = d["bias"]
    xg, wg, bg = d["x"].to(gpu), torch.from_numpy(packed).to(gpu), bias.to(gpu)
    rg = d["res"].to(gpu) if case.res else None
    first, failures, forced = None, [], set()
    for off, ld in _layouts(case):
        tiles = capi.conv2d_tactics_f32(case.N, case.H, case.W, case.Cin, case.Cout, case.k, case.s, case.p, residual=case.res, ld_out=ld)
        assert tiles and len(set(tiles)) == len(tiles)
        for t in tiles:
            what = f"tile {t} at channel {off} of {ld}"
            buf, view = _buffer(case, off, ld, torch.float32, gpu)
            with _time_limit():
                capi.conv2d_nhwc_f32(xg, wg, bg, case.Cout, *case.k, case.s, case.p, case.act1, rg, case.act2, out=view, out_ld=ld, tile=t)
                _sync(f"{case.name} {what}")
            forced.add(t[2])
            clean, got = _untouched(case, buf, off)
            if not clean:
                failures.append(f"{what} wrote outside its slice")
            if first is None:
                first = (what, got)
                err, ratio = _report(case, "f32", f"{what} (every other tile must equal it)", got, ref)
                if not torch.isfinite(got).all() or not (err <= ref.bound).all():
                    failures.append(f"{what}: max err / bound {ratio:.3f}, {int((err > ref.bound).sum())} of {err.numel()} elements beyond the bound")
            elif not torch.equal(got, first[1]):
                failures.append(f"{what} differs from {first[0]}: {int((got != first[1]).sum())} elements, max {(got - first[1]).abs().max().item():.3e}")
    assert not failures, failures
    if case.name in cc.EXPECT_WS:
        assert cc.EXPECT_WS[case.name]["f32"] <= forced, (forced, "the operand paths this map is in the table for were not all run")


# int8 output is specified without a shortcut (tests/conv_cases.py: the fp16 rounding in front of the add cannot be written out in the reference)
I8_RUNS = [(c, False) for c in I8] + [(c, True) for c in I8 if not c.res]


@pytest.mark.parametrize("case,out_i8", I8_RUNS, ids=[f"{c.name}-{'i8out' if o else 'f16out'}" for c, o in I8_RUNS])
def test_conv_i8_matches_the_integer_reference(gpu, case, out_i8):
    """The int8 entry point stores whole 8-channel vectors only (it refuses anything else), so the slice is always the aligned one."""
    d = cc.gen_inputs(case.name)
    ref = cc.reference(case.name, "i8")
    off, ld = _layouts(case)[0]
    packed, wscale = capi.pack_conv_weights_i8(d["w"].numpy())
    cout_pad = packed.shape[0]
    wq, sw = cc.quantise_weights(d["w"])
    assert np.array_equal(wscale[:case.Cout], sw.numpy()) or np.allclose(wscale[:case.Cout], sw.numpy(), rtol=1e-6)
    cscale, bias = torch.zeros(cout_pad), torch.zeros(cout_pad)
    cscale[:case.Cout] = torch.tensor(cc.S_IN, dtype=torch.float32) * torch.from_numpy(wscale[:case.Cout])
    bias[:case.Cout] = d["bias"]
    rg = d["res"].half().to(gpu) if case.res else None
    sentinel = 77 if out_i8 else SENTINEL
    buf, view = _buffer(case, off, ld, torch.int8 if out_i8 else torch.float16, gpu, sentinel)
    s_out = None
    if out_i8:
        want, near, s_out = cc.i8_expected(case.name)
    with _time_limit():
        capi.conv2d_nhwc_i8(d["xq"].to(torch.int8).to(gpu), torch.from_numpy(packed).to(gpu), cscale.to(gpu), bias.to(gpu), case.Cout, *case.k, case.s, case.p,
                            case.act1, out_scale=s_out, residual=rg, act2=case.act2, out=view, out_ld=ld)
        _sync(case.name)
    clean, got = _untouched(case, buf, off, sentinel)
    assert clean, "written outside the slice"
    if out_i8:
        diff = (got.double() - want).abs()
        moved = diff > 0
        print(f"{case.name} i8 int8 output: {int(moved.sum())} of {diff.numel()} differ ({int(near.sum())} may), max step {int(diff.max())}")
        assert diff.max() <= 1 and not (moved & ~near).any(), (int(diff.max()), int((moved & ~near).sum()))
    else:
        err, ratio = _report(case, "i8", "fp16 output", got, ref)
        assert torch.isfinite(got).all() and (err <= ref.bound).all(), (ratio, int((err > ref.bound).sum()))
