"""The depthwise table (tests/dw_cases.py) on the device: every case through the C ABI entry trtx_op_conv2d_dw_nhwc, fp16 and fp32, against the
table's torch fp64 reference - every output element under the per-element bound derived in tests/dw_cases.py, nothing fitted.

Layouts.  The output lives in a channel slice of a wider buffer with one extra image in front and one behind, all pre-filled with a sentinel: nothing
outside the slice may change.  The input and the shortcut live in such slices too, their surroundings and guard images NaN: a read outside the tensor that
reaches a result shows.  Every case runs with all three slices aligned (channel 8 of a row that is a multiple of 8: the 16-byte path wherever C allows it) and
with all three misaligned (channel 6 of an odd row: the element-wise path); cases with C % 8 == 0 also with only the base pointers misaligned (channel 6,
rows a multiple of 8) and with only one of ld_in, ld_out, ld_res off the vector width.  Which path a layout takes is computed here from the pointers, by the
launcher's own rule, and asserted to be the intended one.  Both paths sum in the same order: all layouts of a case must agree bit for bit.

Every launch runs under a watchdog of its own, and a HIP error ends the session (tests/util.py)."""
import pytest
import torch

from tensorrtx_amd import capi
from tests import dw_cases as dc
from tests.util import SENTINEL, guarded_slice, outside_untouched, sync, time_limit

pytestmark = pytest.mark.gpu

NAN = float("nan")
DTYPE = {"f16": torch.float16, "f32": torch.float32}


def _r8(n):
    return (n + 7) // 8 * 8


def _layouts(case):
    """[(name, {tensor: (channel offset, row width)})]"""
    C = case.C
    al, mis, base = (8, _r8(8 + C + 8)), (6, _r8(6 + C + 8) + 7), (6, _r8(6 + C + 8))
    off_ld = (8, _r8(8 + C + 8) + 2)     # a row width that is a multiple of neither 8 halves nor 4 floats
    every = lambda v: {"in": v, "out": v, "res": v}  # noqa: E731
    out = [("aligned", every(al)), ("misaligned", every(mis))]
    if C % 8 == 0 and not case.big:
        out.append(("base only", every(base)))
        for t in ("in", "out") + (("res",) if case.res else ()):
            lay = every(al)
            lay[t] = off_ld
            out.append((f"ld_{t} only", lay))
    return out


def _vector_path(case, engine, x, out, res, lds):
    """the launcher's rule (kernels/conv_dw.hip conv_dw), restated on the pointers of this launch"""
    v = dc.VEC[engine]
    ts = [(x, lds["in"]), (out, lds["out"])] + ([(res, lds["res"])] if res is not None else [])
    return case.C % v == 0 and all(ld % v == 0 and t.data_ptr() % 16 == 0 for t, ld in ts)


RUNS = [(c, e) for c in dc.CASES for e in c.engines]


@pytest.mark.parametrize("case,engine", RUNS, ids=[f"{c.name}-{e}" for c, e in RUNS])
def test_dw_every_layout_matches_fp64_and_each_other(gpu, case, engine):
    d = dc.gen_inputs(case.name)
    ref = dc.reference(case.name, engine)
    xs, rs = dc.stored(case, engine)
    Ho, Wo = case.out_hw
    bias = d["bias"].to(gpu) if case.bias else None
    w = d["w"].numpy()
    first, failures, paths = None, [], set()
    for name, lay in _layouts(case):
        _, xv = guarded_slice((case.N, case.H, case.W, case.C), *lay["in"], DTYPE[engine], gpu, NAN)
        xv.copy_(xs.to(gpu))
        rv = None
        if case.res:
            _, rv = guarded_slice((case.N, Ho, Wo, case.C), *lay["res"], DTYPE[engine], gpu, NAN)
            rv.copy_(rs.to(gpu))
        buf, view = guarded_slice((case.N, Ho, Wo, case.C), *lay["out"], DTYPE[engine], gpu)
        vec = _vector_path(case, engine, xv, view, rv, {t: ld for t, (_, ld) in lay.items()})
        assert vec == (name == "aligned" and case.C % dc.VEC[engine] == 0), (name, vec)
        paths.add("vector" if vec else "scalar")
        what = f"{case.name} {engine} {name} ({'vector' if vec else 'scalar'} path)"
        with time_limit():
            capi.conv2d_dw_nhwc(xv, w, bias, case.k, case.s, case.act1, rv, case.act2, out=view, out_ld=lay["out"][1], alpha1=dc.ALPHA, alpha2=dc.ALPHA)
            sync(what)
        clean, got = outside_untouched(buf, lay["out"][0], case.C)
        if not clean:
            failures.append(f"{name} wrote outside its slice")
        if first is None:
            first = (name, got)
            err = (got.double() - ref.y).abs()
            ratio = (err / ref.bound).max().item()
            print(f"{what}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
            if not torch.isfinite(got).all() or not (err <= ref.bound).all():
                failures.append(f"{name}: max err / bound {ratio:.3f}, {int((err > ref.bound).sum())} of {err.numel()} elements beyond the bound")
        elif not torch.equal(got, first[1]):
            failures.append(f"{name} is not bit-identical to {first[0]}: {int((got != first[1]).sum())} elements differ")
    assert not failures, failures
    assert paths == case.paths(engine)


@pytest.mark.parametrize("engine", ["f16", "f32"])
@pytest.mark.parametrize("what,kw", [("k 4", dict(k=4, pad=2)), ("dilation 2", dict(k=3, dilation=2, pad=2)), ("pad 0 under k 3", dict(k=3, pad=0)),
                                     ("pad 2 under k 3", dict(k=3, pad=2)), ("stride 3", dict(k=3, stride=3))])
def test_dw_unsupported_arguments_are_refused_and_nothing_is_written(gpu, engine, what, kw):
    N, H, W, C = 1, 9, 9, 8
    k, stride, pad, dil = kw["k"], kw.get("stride", 1), kw["pad"] if "pad" in kw else kw["k"] // 2, kw.get("dilation", 1)
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    x = torch.ones((N, H, W, C), dtype=DTYPE[engine], device=gpu)
    buf, view = guarded_slice((N, Ho, Wo, C), 8, 24, DTYPE[engine], gpu)
    with pytest.raises(capi.TrtxError) as e, time_limit():
        capi.conv2d_dw_nhwc(x, torch.ones(C, k, k).numpy(), None, k, stride, out=view, out_ld=24, pad=pad, dilation=dil)
    sync(what)
    assert e.value.status == 4   # TRTX_ERR_UNSUPPORTED
    assert bool((buf == SENTINEL).all())
