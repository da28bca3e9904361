"""The attention table (tests/attention_cases.py) on the device: psa_attention_f16 and area_attention_f16 through the C ABI against the table's torch
fp64 reference - every element of O under the per-element bound derived in tests/attention_cases.py, the V image bit-equal to the v slice of qkv; O and
the V image are compared separately (the plan-level tests only see their sum).

Layouts.  O and the V image each live in a channel slice of a wider buffer with one extra image in front and one behind, pre-filled with a sentinel:
nothing outside the slices may change.  qkv lives in such a slice too, its surroundings and guard images NaN: a key of a pixel outside the batch, or a
channel outside the tensor, that reaches a result shows; keys of the neighbouring area or image show through the table's leak cases.
The area kernel's launcher derives three independent flags - 16-byte loads of qkv, 8-byte stores of O, 16-byte stores of the V image - from base pointer
and channel stride; every case runs with all on, all off and each single one off (an offset of 4 halves keeps the 8-byte O store legal where the 16-byte
accesses are not), the flags computed here by the launcher's rule and asserted to be the intended ones.  The PSA kernel is element-wise throughout and runs
aligned and misaligned.  All layouts of a case must agree bit for bit.

Every launch runs under a watchdog of its own, and a HIP error ends the session (tests/util.py)."""
import pytest
import torch

from tensorrtx_amd import capi
from tests import attention_cases as ac
from tests.util import SENTINEL, guarded_slice, outside_untouched, sync, time_limit

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _r8(n):
    return (n + 7) // 8 * 8


def _on(C):
    return (8, _r8(8 + C + 8))


def _layouts(case):
    """[(name, (qkv, O, V image) slices as (channel offset, row width), the flags (vec_in, vec_o, vec_v) the area launcher must derive)]"""
    W, C = case.width, case.heads * case.hd
    odd = lambda n: (3, _r8(3 + n + 8) + 1)   # noqa: E731  6 bytes into an odd row
    four = lambda n: (4, _r8(4 + n + 8))      # noqa: E731  8 bytes into a row of whole vectors: 8-byte accesses stay legal, 16-byte ones do not
    two = lambda n: (2, _r8(2 + n + 8))       # noqa: E731  4 bytes in
    lay = [("all on", (_on(W), _on(C), _on(C)), (1, 1, 1)), ("all off", (odd(W), odd(C), odd(C)), (0, 0, 0))]
    if case.kind == "area":
        lay += [("loads off", (four(W), four(C), _on(C)), (0, 1, 1)), ("O stores off", (_on(W), two(C), _on(C)), (1, 0, 1)),
                ("V stores off", (_on(W), _on(C), four(C)), (1, 1, 0))]
    return lay


def _flags(qkv, out, vimg, lds):
    """kernels/attention_mfma.hip aligned(): base and row pitch in bytes both multiples of the access width"""
    ok = lambda t, ld, n: int(t.data_ptr() % n == 0 and (ld * 2) % n == 0)   # noqa: E731
    return ok(qkv, lds[0], 16), ok(out, lds[1], 8), ok(vimg, lds[2], 16)


def _launch(case, qv, ov, vv, lds):
    if case.kind == "psa":
        capi.psa_attention(qv, case.heads, ac.SCALE, out=ov, vimg=vv, qkv_ld=lds[0], out_ld=lds[1], v_ld=lds[2])
    else:
        capi.area_attention(qv, case.heads, case.area, ac.SCALE, out=ov, vimg=vv, qkv_ld=lds[0], out_ld=lds[1], v_ld=lds[2])


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_attention_every_layout_matches_fp64_and_each_other(gpu, case):
    qkv = ac.gen_inputs(case.name)
    ref = ac.reference(case.name)
    C = case.heads * case.hd
    first, failures = None, []
    for name, (lq, lo, lv), flags in _layouts(case):
        _, qv = guarded_slice((case.B, case.N, case.width), *lq, torch.float16, gpu, NAN)
        qv.copy_(qkv.to(gpu))
        obuf, ov = guarded_slice((case.B, case.N, C), *lo, torch.float16, gpu)
        vbuf, vv = guarded_slice((case.B, case.N, C), *lv, torch.float16, gpu)
        lds = (lq[1], lo[1], lv[1])
        assert _flags(qv, ov, vv, lds) == flags, (name, _flags(qv, ov, vv, lds))
        what = f"{case.name} {name}"
        with time_limit():
            _launch(case, qv, ov, vv, lds)
            sync(what)
        clean_o, got = outside_untouched(obuf, lo[0], C)
        clean_v, gotv = outside_untouched(vbuf, lv[0], C)
        if not (clean_o and clean_v):
            failures.append(f"{name} wrote outside its slices (O clean: {clean_o}, V image clean: {clean_v})")
        if not torch.equal(gotv, ref.v):
            failures.append(f"{name}: the V image is not the v slice: {int((gotv != ref.v).sum())} elements differ")
        if first is None:
            first = (name, got)
            err = (got.double() - ref.o).abs()
            ratio = (err / ref.bound).max().item()
            print(f"{what}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
            if not torch.isfinite(got).all() or not (err <= ref.bound).all():
                failures.append(f"{name}: max err / bound {ratio:.3f}, {int((err > ref.bound).sum())} of {err.numel()} elements beyond the bound")
        elif not torch.equal(got, first[1]):
            failures.append(f"{name} is not bit-identical to {first[0]}: {int((got != first[1]).sum())} elements differ")
    assert not failures, failures


def _refused(gpu, kind, B, heads, N, width, ld_qkv=None, **kw):
    C = heads * ac.HD[kind]
    area = kw.pop("area", 1)
    qkv = torch.ones((B, N, width), dtype=torch.float16, device=gpu)
    obuf, ov = guarded_slice((B, N, C), 8, C + 16, torch.float16, gpu)
    vbuf, vv = guarded_slice((B, N, C), 8, C + 16, torch.float16, gpu)
    with pytest.raises(capi.TrtxError) as e, time_limit():
        if kind == "psa":
            capi.psa_attention(qkv, heads, ac.SCALE, out=ov, vimg=vv, out_ld=C + 16, v_ld=C + 16, qkv_ld=ld_qkv, **kw)
        else:
            capi.area_attention(qkv, heads, area, ac.SCALE, out=ov, vimg=vv, out_ld=C + 16, v_ld=C + 16, qkv_ld=ld_qkv, **kw)
    sync(f"{kind} refusal")
    assert e.value.status == 4   # TRTX_ERR_UNSUPPORTED
    assert bool((obuf == SENTINEL).all()) and bool((vbuf == SENTINEL).all())


def test_area_attention_refuses_what_it_does_not_implement(gpu):
    _refused(gpu, "area", 1, 2, 30, 192, area=4)                  # N % area != 0
    _refused(gpu, "area", 1, 2, 32, 192, kd=32, hd=64)            # the PSA pair
    _refused(gpu, "area", 1, 2, 32, 192, kd=16, hd=32)
    _refused(gpu, "area", 1, 2, 32, 192, ld_qkv=2 * 96 - 8)       # a row narrower than the heads' channels


def test_psa_attention_refuses_what_it_does_not_implement(gpu):
    _refused(gpu, "psa", 1, 2, 32, 256, kd=32, hd=32)             # the area pair
    _refused(gpu, "psa", 1, 2, 32, 256, kd=64, hd=64)
    _refused(gpu, "psa", 1, 2, 32, 256, ld_qkv=2 * 128 - 8)
