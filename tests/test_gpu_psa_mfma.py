"""PSA attention on the matrix pipe (kernels/attention_mfma.hip) against torch fp64: every `psa` case of tests/attention_cases.py (kd 32 / hd 64) and yolov10m's
kd 36 / hd 72 heads through the C ABI, under the table's PSA bound plus the term it adds for kernels that round P to fp16; the V image bit-equal.  Every case
runs in a 16-byte aligned channel slice and in one 6 bytes into an odd row (element-wise accesses) of buffers with guard images - NaN around qkv, a sentinel
around O and the V image - and the two agree bit for bit.  Then a single-attention engine in both head shapes, on the new route (the default for heads of 72,
TRTX_PSA_MFMA=2 for heads of 64) and with TRTX_PSA_MFMA=0."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import builder, capi, engine
from tests import attention_cases as ac
from tests.layer_cases import U32
from tests.parity import EPS16, fp16_walk
from tests.util import guarded_slice, outside_untouched, sync, time_limit

pytestmark = pytest.mark.gpu


def _reference(qkv, heads, kd, hd, scale):
    # qkv [B, N, heads * (2 kd + hd)] fp16 -> O fp64, the v slice, the P-rounding term and the whole bound of tests/attention_cases.py, each [B, N, heads * hd]
    B, N, _ = qkv.shape
    q, k, v = qkv.double().reshape(B, N, heads, 2 * kd + hd).permute(0, 2, 1, 3).split([kd, kd, hd], -1)
    s = (q @ k.transpose(-2, -1)) * scale
    w, o, pv = s.softmax(-1), s.softmax(-1) @ v, s.softmax(-1) @ v.abs()
    d = 3 * U32 * (s - s.max(-1, keepdim=True).values).abs()
    e_exp = (w * d) @ v.abs() + (w * d).sum(-1, keepdim=True) * o.abs()
    bound = fp16_walk(1, o.abs()) + ac.FLOOR * v.abs().amax((-2, -1), keepdim=True) + e_exp + 2 * EPS16 * pv
    img = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, heads * hd).contiguous()   # noqa: E731
    return img(o), img(v).half(), 2 * EPS16 * img(pv), img(bound)


def _check(gpu, what, wide, c0, heads, kd, hd, scale, bound=None):
    (B, N, W), width, C, first = wide.shape, heads * (2 * kd + hd), heads * hd, None   # launches on the channels [c0, c0 + width) of `wide`, in both layouts
    o_ref, v_ref, p_term, full = _reference(wide[..., c0:c0 + width], heads, kd, hd, scale)
    bound = full if bound is None else bound + p_term
    for name, lay in (("aligned", lambda n: (8, (n + 23) // 8 * 8)), ("misaligned", lambda n: (3, (n + 18) // 8 * 8 + 1))):
        (oq, lq), (oo, lo), (ov_, lv) = lay(W), lay(C), lay(C)
        _, qv = guarded_slice((B, N, W), oq, lq, torch.float16, gpu, float("nan"))
        qv.copy_(wide.to(gpu))
        (obuf, ov), (vbuf, vv) = guarded_slice((B, N, C), oo, lo, torch.float16, gpu), guarded_slice((B, N, C), ov_, lv, torch.float16, gpu)
        assert (qv[..., c0:].data_ptr() % 16 == 0 and lq % 8 == 0) == (name == "aligned")
        with time_limit():
            capi.psa_attention_mfma(qv[..., c0:c0 + width], heads, scale, out=ov, vimg=vv, qkv_ld=lq, out_ld=lo, v_ld=lv, kd=kd, hd=hd)
            sync(f"{what} {name}")
        (clean_o, got), (clean_v, gotv) = outside_untouched(obuf, oo, C), outside_untouched(vbuf, ov_, C)
        assert clean_o and clean_v, f"{what} {name}: wrote outside its slices"
        assert torch.equal(gotv, v_ref), f"{what} {name}: the V image is not the v slice"
        if first is None:
            first = got
            err = (got.double() - o_ref).abs()
            print(f"{what}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
            assert torch.isfinite(got).all() and (err <= bound).all(), f"{what} {name}: beyond the bound"
        else:
            assert torch.equal(got, first), f"{what}: {name} differs from aligned in {int((got != first).sum())} elements"


@pytest.mark.parametrize("case", ac.PSA, ids=lambda c: c.name)
def test_table_cases_match_fp64_in_both_layouts(gpu, case):
    _check(gpu, case.name, ac.gen_inputs(case.name), 0, case.heads, ac.KD, case.hd, ac.SCALE, bound=ac.reference(case.name).bound)


@pytest.mark.parametrize("B,heads,N,leak", [(1, 1, 1, False), (2, 4, 65, False), (1, 4, 200, False), (2, 3, 65, True)])
def test_heads_of_72_match_fp64_in_both_layouts(gpu, B, heads, N, leak):
    kd, hd = 36, 72
    qkv = torch.randn((B, N, heads * 144), generator=torch.Generator().manual_seed(100 * N + heads)).half()
    c0, launch_heads = 0, heads
    if leak:   # the middle head alone; what padding read from memory would find: k behind q and v behind k (+200, exact in fp16), NaN outside the head
        qkv[..., :144] = qkv[..., 288:] = float("nan")
        qkv[..., 144 + kd:144 + kd + 12] *= 8
        qkv[..., 144 + 2 * kd:144 + 2 * kd + 12] += 200
        c0, launch_heads = 144, 1
    _check(gpu, f"kd36 B{B} h{heads} N{N}" + (" leak" if leak else ""), qkv, c0, launch_heads, kd, hd, kd ** -0.5)


def _attention_net(B, heads, H, W, kd, hd, seed):
    """The Attention subgraph of YOLO11's C2PSA / YOLOv10's PSA on a 1x1 qkv convolution, O + V summed into the output (both results have a reader)"""
    C, cin, N = heads * (2 * kd + hd), 16, H * W
    rng = np.random.default_rng(seed)
    x, wq = rng.standard_normal((B, cin, H, W)).astype(np.float32), (rng.standard_normal((C, cin, 1, 1)) / 4).astype(np.float32)
    net = builder.Network(explicit_batch=True, fp16=True)
    try:
        qkv = net.out(net.conv(net.input("x", (B, cin, H, W)), wq))
        v4 = net.out(net.shuffle(qkv, reshape=(B, heads, -1, N)))
        q, k, v = (net.out(net.slice(v4, (0, 0, c, 0), (B, heads, n, N))) for c, n in ((0, kd), (kd, kd), (2 * kd, hd)))
        s = net.out(net.scale_uniform(net.out(net.matmul(net.out(net.shuffle(q, perm1=(0, 1, 3, 2))), k)), kd ** -0.5))
        pt = net.out(net.shuffle(net.out(net.softmax(s, axes=1 << 3)), perm1=(0, 1, 3, 2)))
        o = net.out(net.shuffle(net.out(net.matmul(v, pt)), reshape=(B, -1, H, W)))
        net.mark_output(net.out(net.elementwise(o, net.out(net.shuffle(v, reshape=(B, -1, H, W))))), "y")
        return net.build(), x, wq
    finally:
        net.close()


@pytest.mark.parametrize("kd,hd", [(32, 64), (36, 72)])
def test_engine_takes_the_mfma_kernel_where_the_switch_admits_it(gpu, kd, hd, monkeypatch):
    B, heads, H, W = 2, 2, 9, 11
    plan, x, wq = _attention_net(B, heads, H, W, kd, hd, seed=kd)
    qkv = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wq).double()).half()   # the fp16 storage site
    o, v, p_term, _ = _reference(qkv.reshape(B, -1, H * W).transpose(1, 2), heads, kd, hd, kd ** -0.5)
    q, k, _ = qkv.double().reshape(B, heads, 2 * kd + hd, H * W).split([kd, kd, hd], 2)
    s_abs, vmax = ((q.abs().transpose(-2, -1) @ k.abs()) * kd ** -0.5).max().item(), v.abs().max().item()
    # tests/test_gpu_yolo11.py's bound (O's store and the sum's, a one-ulp disagreement of q / k, the fp32 floor); the MFMA route adds P's rounding
    base = fp16_walk(2, o.abs() + v.double().abs()) + 2 * EPS16 * s_abs * vmax + ac.FLOOR * vmax
    for switch, mfma in ((None, kd == 36), ("2", True), ("0", False)):
        bound = base + p_term if mfma else base
        monkeypatch.delenv("TRTX_PSA_MFMA", raising=False) if switch is None else monkeypatch.setenv("TRTX_PSA_MFMA", switch)
        (att,) = [op for op in engine.describe_plan(plan, lowered=True)["ops"] if op["kind"] == "attention"]
        assert (att["kd"], att["hd"], att.get("mfma", False)) == (kd, hd, mfma)
        e = engine.Engine(plan)   # lowers under the switch as it is now
        y = torch.full((B * heads * hd * H * W,), float("nan"), dtype=torch.float32, device=gpu)
        e.enqueue(B, [torch.from_numpy(x).to(gpu), y])
        sync(f"engine kd {kd} switch {switch}")
        e.close()
        got = y.cpu().double().reshape(B, heads * hd, H * W).transpose(1, 2)
        assert torch.isfinite(got).all() and ((got - (o + v.double())).abs() <= bound).all()
