"""Attention in fp32 engines (kernels/attention_f32.hip) against torch fp64 on the same fp32 inputs, through capi.attention_f32: every `psa` and `area` case of
tests/attention_cases.py upcast to fp32, and fp32 randn inputs (not fp16-representable) at the kernel's own edges - N 1; 17 and 65 (a second key tile / chunk of
one key, a second query block of one query); area 4 with Na 17; the (36, 72) heads at N 65 (the ninth k-step, the half-full fifth tile); three heads launched
on the middle one with NaN in the neighbours, k behind q scaled and v behind k offset.  Every case runs in a 16-byte aligned channel slice and in one 3 floats
into an odd-stride row of buffers with guard images - NaN around qkv, a sentinel around O and the V image: the two agree bit for bit, nothing outside is written,
the V image is the v slice bit for bit, O is finite and within the bound.  Then one-attention fp32 engines under TRTX_ATTENTION_F32=1 and on the generic route.

The bound, per element, in the style of tests/attention_cases.py, U32 = 2^-24, w = softmax(s), sites from the kernel text (nothing is rounded to fp16):
    |err| <= E_exp(d + ds) + (Na + 2) * 2 * U32 * (w @ |v|) + FLOOR * max|v|
  * ds = (kd + 1) * U32 * scale * (|q|^T |k|): a score is an fp32 sum of kd products in any order, times the scale;
  * d = 3 * U32 * |s - max|, the exponential's argument as in attention_cases.py; both are errors of the logarithm of a weight and propagate as that file's
    E_exp does: E_exp(e) = (w * e) @ |v| + (sum_m w_m e_m) * |O|;
  * (Na + 2) * 2 * U32 * (w @ |v|): the P.V sum and the denominator, Na + 2 roundings each in any order, relative to sum_m w_m |v_m|;
  * FLOOR * max|v| over the v rows a query may see, the table's floor.
An engine's qkv is its fp32 convolution's output, off the fp64 one by eq = layer_cases.fp32_bound: the scores move by scale * (eq_q^T |k| + |q|^T eq_k +
eq_q^T eq_k), added to ds; v moves by eq_v: w @ eq_v on O and eq_v on the V image; the sum O + V rounds once more."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import capi, engine
from tests import attention_cases as ac
from tests.layer_cases import U32, Out, fp32_bound
from tests.test_attention_f32_cpu import NETS, attention_net
from tests.util import guarded_slice, outside_untouched, sync, time_limit

pytestmark = pytest.mark.gpu


def _reference(qkv, heads, area, kd, hd, scale, eq=None):
    # qkv [B, N, heads * (2 kd + hd)] (eq: a bound on its own error, same shape) -> O fp64, the v slice and the bound on O, each [B, N, heads * hd]
    B, N, _ = qkv.shape
    blocks = lambda t: t.double().reshape(B, area, N // area, heads, 2 * kd + hd).permute(0, 3, 1, 2, 4).split([kd, kd, hd], -1)   # noqa: E731
    img = lambda t: t.permute(0, 2, 3, 1, 4).reshape(B, N, heads * hd).contiguous()   # noqa: E731
    q, k, v = blocks(qkv)
    s = (q @ k.transpose(-2, -1)) * scale
    w, o = s.softmax(-1), s.softmax(-1) @ v
    e = 3 * U32 * (s - s.max(-1, keepdim=True).values).abs() + (kd + 1) * U32 * scale * (q.abs() @ k.abs().transpose(-2, -1))
    eq_q, eq_k, eq_v = blocks(torch.zeros_like(qkv) if eq is None else eq)
    e = e + scale * (eq_q @ k.abs().transpose(-2, -1) + (q.abs() + eq_q) @ eq_k.transpose(-2, -1))
    bound = (w * e) @ v.abs() + (w * e).sum(-1, keepdim=True) * o.abs() + (N // area + 2) * 2 * U32 * (w @ v.abs()) + w @ eq_v
    return img(o), img(v), img(bound + ac.FLOOR * v.abs().amax((-2, -1), keepdim=True))


def _check(gpu, what, wide, c0, heads, area, kd, hd):
    (B, N, W), width, C, first = wide.shape, heads * (2 * kd + hd), heads * hd, None   # launches on the channels [c0, c0 + width) of `wide`, in both layouts
    scale = float(np.float32(kd ** -0.5))
    o_ref, v_ref, bound = _reference(wide[..., c0:c0 + width], heads, area, kd, hd, scale)
    for name, lay in (("aligned", lambda n: (4, (n + 11) // 4 * 4)), ("misaligned", lambda n: (3, (n + 10) // 4 * 4 + 1))):
        (oq, lq), (oo, lo), (ov_, lv) = lay(W), lay(C), lay(C)
        _, qv = guarded_slice((B, N, W), oq, lq, torch.float32, gpu, float("nan"))
        qv.copy_(wide.to(gpu))
        (obuf, ov), (vbuf, vv) = guarded_slice((B, N, C), oo, lo, torch.float32, gpu), guarded_slice((B, N, C), ov_, lv, torch.float32, gpu)
        assert (qv[..., c0:].data_ptr() % 16 == 0 and lq % 4 == 0) == (name == "aligned")
        with time_limit():
            capi.attention_f32(qv[..., c0:c0 + width], heads, area, scale, out=ov, vimg=vv, qkv_ld=lq, out_ld=lo, v_ld=lv, kd=kd, hd=hd)
            sync(f"{what} {name}")
        (clean_o, got), (clean_v, gotv) = outside_untouched(obuf, oo, C), outside_untouched(vbuf, ov_, C)
        assert clean_o and clean_v, f"{what} {name}: wrote outside its slices"
        assert torch.equal(gotv.double(), v_ref), f"{what} {name}: the V image is not the v slice"
        if first is None:
            first = got
            err = (got.double() - o_ref).abs()
            print(f"{what}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
            assert torch.isfinite(got).all() and (err <= bound).all(), f"{what} {name}: beyond the bound"
        else:
            assert torch.equal(got, first), f"{what}: {name} differs from aligned in {int((got != first).sum())} elements"


@pytest.mark.parametrize("case", ac.PSA + ac.AREA, ids=lambda c: c.name)
def test_table_cases_match_fp64_in_both_layouts(gpu, case):
    _check(gpu, case.name, ac.gen_inputs(case.name).float(), 0, case.heads, case.area, ac.KD, case.hd)


@pytest.mark.parametrize("kd,hd,B,heads,N,area,leak", [(32, 32, 1, 1, 1, 1, 0), (36, 72, 2, 1, 1, 1, 0), (32, 64, 1, 2, 17, 1, 0), (32, 32, 2, 1, 65, 1, 0), (32, 64, 1, 1, 65, 1, 0),
                                                     (32, 32, 1, 2, 68, 4, 0), (36, 72, 2, 2, 65, 1, 0), (36, 72, 1, 3, 65, 1, 1), (32, 32, 2, 3, 68, 4, 1)])
def test_fp32_inputs_at_the_kernel_edges_match_fp64_in_both_layouts(gpu, kd, hd, B, heads, N, area, leak):
    hw = 2 * kd + hd
    qkv = torch.randn((B, N, heads * hw), generator=torch.Generator().manual_seed(1000 * hd + 10 * N + heads))
    c0, launch_heads = 0, heads
    if leak:   # the middle head alone; what a read beyond a fragment would find: k behind q (scaled), v behind k (offset), NaN outside the head
        qkv[..., :hw] = qkv[..., 2 * hw:] = float("nan")
        qkv[..., hw + kd:hw + kd + 12] *= 8
        qkv[..., hw + 2 * kd:hw + 2 * kd + 12] += 200
        c0, launch_heads = hw, 1
    _check(gpu, f"kd{kd} hd{hd} B{B} h{heads} N{N} a{area}" + (" leak" if leak else ""), qkv, c0, launch_heads, area, kd, hd)


@pytest.mark.parametrize("kind,area,kd,hd", NETS)
def test_fp32_engine_takes_the_kernel_under_the_switch(gpu, kind, area, kd, hd, monkeypatch):
    plan, x, wq = attention_net(kind, area, kd, hd)
    (B, cin, H, W), heads, conv = x.shape, 2, torch.nn.functional.conv2d
    bnc = lambda t: t.reshape(B, -1, H * W).transpose(1, 2)   # noqa: E731
    qkv, mag = conv(torch.from_numpy(x).double(), torch.from_numpy(wq).double()), conv(torch.from_numpy(x).double().abs(), torch.from_numpy(wq).double().abs())
    eq = bnc(fp32_bound(Out(qkv, mag, n=cin + 2)))
    o, v, bound = _reference(bnc(qkv), heads, area, kd, hd, float(np.float32(kd ** -0.5)), eq=eq)
    eq_v = eq.reshape(B, H * W, heads, 2 * kd + hd)[..., 2 * kd:].reshape(B, H * W, heads * hd)
    bound = bound + eq_v + 2 * U32 * (o.abs() + v.abs())   # the V image's own error and the rounding of the sum
    got = {}
    for switch in ("1", None):
        monkeypatch.delenv("TRTX_ATTENTION_F32", raising=False) if switch is None else monkeypatch.setenv("TRTX_ATTENTION_F32", switch)
        assert [op.get("f32") for op in engine.describe_plan(plan, lowered=True)["ops"] if op["kind"] == "attention"] == ([True] if switch else [])
        e = engine.Engine(plan)   # lowers under the switch as it is now
        y = torch.full((B * heads * hd * H * W,), float("nan"), dtype=torch.float32, device=gpu)
        with time_limit():
            e.enqueue(B, [torch.from_numpy(x).to(gpu), y])
            sync(f"engine {kind} kd {kd} switch {switch}")
        e.close()
        got[switch] = bnc(y.cpu().double().reshape(B, heads * hd, H, W))
    err = (got["1"] - (o + v)).abs()
    print(f"engine {kind} {kd}/{hd}: max err / bound {(err / bound).max().item():.3f}, to generic / (2 bound) {((got['1'] - got[None]).abs() / (2 * bound)).max().item():.3f}")
    assert torch.isfinite(got["1"]).all() and (err <= bound).all()
    assert ((got["1"] - got[None]).abs() <= 2 * bound).all()
