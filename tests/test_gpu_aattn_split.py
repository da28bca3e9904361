"""YOLOv13's area attention on separate qk and v on the device: area_attention_split_f16 through the C ABI on the attention table's "area" cases
(tests/attention_cases.py, repacked by tests/aattn_split_cases.py) and the attention_split op inside plans.

The kernel.  Every case runs in seven layouts: q, k, v and O each a channel slice of a wider buffer with one guard image in front and one behind - the
inputs' surroundings NaN, O's a sentinel.  The launcher derives one flag per operand from base pointer and pixel stride (16-byte loads of q, k, v, 8-byte
stores of O); the layouts turn each off alone, all off, all on with q and k in one buffer (YOLOv13's: k = q + C, one stride) and all on with q and k apart.
The flags are computed here by the launcher's rule and asserted to be the intended ones.  All layouts agree bit for bit, every element is under the table's
bound, and O is torch.equal to area_attention_f16's O on the same case's packed qkv: the two are one kernel body that differs in addresses only.

The plans (aattn13_net).  Rounding sites, u = 2^-11; the reference is fp64 from the qk and v convolution outputs rounded to fp16 (the engine's storage
sites).  Scores are fp32 MFMA sums of exact fp16 products, scaled in fp32; max, exp and the denominator are fp32.  Then
  * P is rounded to fp16 as the P.V operand, relative u per weight, the fp32 denominator unrounded: 2u * (softmax @ |v|);
  * O is rounded at its store and the final sum once more: fp16_walk(2, |O| + |other|), other = v or pe(v);
  * the engine rounds the fp32 sums of the two convolutions where the reference rounds fp64 ones, so an element of q, k or v may land on the neighbouring
    fp16 value (2u relative).  In q / k that moves a score by at most 2u * s_abs (s_abs = the largest scale * sum_j |q_j k_j|) and O by that times max |v|;
    in v it moves O by at most 2u * (softmax @ |v|), the summand v by 2u |v|, and the summand pe(v) by 2u * (|w_pe| * |v|);
  * pe is 25 fp32 multiply-adds on fp32 weights, (25 + 1) * 2^-24 * (|w_pe| * |v|), and its epilogue adds O before the one store counted above;
  * a floor of 1e-4 * max |v| for the fp32 arithmetic in between.
The generic lowering of the same graph has fewer sites (fp32 linear tensors between the images and the sum), so the same bound holds for it against fp64
and twice the bound between the two routes.

Every launch runs under a watchdog of its own, and a HIP error ends the session (tests/util.py)."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import capi, engine
from tests import aattn_split_cases as sc
from tests import attention_cases as ac
from tests.parity import fp16_walk
from tests.util import SENTINEL, guarded_slice, outside_untouched, sync, time_limit

pytestmark = pytest.mark.gpu

NAN = float("nan")
U16, U32 = 2.0 ** -11, 2.0 ** -24


# ---- the kernel on the table -------------------------------------------------------------------------------------------------------------------------------
def _r8(n):
    return (n + 7) // 8 * 8


def _on(n):      # 16 bytes into a row of whole vectors
    return (8, _r8(8 + n + 8))


def _four(n):    # 8 bytes in: 8-byte accesses stay legal, 16-byte ones do not
    return (4, _r8(4 + n + 8))


def _two(n):     # 4 bytes in
    return (2, _r8(2 + n + 8))


def _odd(n):     # 6 bytes into an odd row
    return (3, _r8(3 + n + 8) + 1)


# name, (q, k, v, O) slices as (channel offset, row width) - q = None: q and k are the two halves of ONE slice of 2C channels placed as k's entry says -,
# and the flags (vec_q, vec_k, vec_v, vec_o) the launcher must derive
def _layouts(C):
    return [("all on, q | k in one buffer", (None, _on(2 * C), _on(C), _on(C)), (1, 1, 1, 1)),
            ("all on, q and k apart", (_on(C), _on(C), _on(C), _on(C)), (1, 1, 1, 1)),
            ("q off", (_four(C), _on(C), _on(C), _on(C)), (0, 1, 1, 1)),
            ("k off", (_on(C), _four(C), _on(C), _on(C)), (1, 0, 1, 1)),
            ("v off", (_on(C), _on(C), _four(C), _on(C)), (1, 1, 0, 1)),
            ("O stores off", (_on(C), _on(C), _on(C), _two(C)), (1, 1, 1, 0)),
            ("all off", (_odd(C), _odd(C), _odd(C), _odd(C)), (0, 0, 0, 0))]


def _flags(q, k, v, out, lds):
    """kernels/attention_mfma.hip aligned(): base and row pitch in bytes both multiples of the access width"""
    ok = lambda t, ld, n: int(t.data_ptr() % n == 0 and (ld * 2) % n == 0)   # noqa: E731
    return ok(q, lds[0], 16), ok(k, lds[1], 16), ok(v, lds[2], 16), ok(out, lds[3], 8)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("case", ac.AREA, ids=lambda c: c.name)
def test_split_attention_every_layout_matches_fp64_the_packed_kernel_and_each_other(gpu, case):
    qkv = ac.gen_inputs(case.name)
    ref = ac.reference(case.name)
    C = case.heads * case.hd
    qk, v = sc.split_operands(case, qkv)
    shape = (case.B, case.N, C)
    with time_limit():
        packed, _ = capi.area_attention(qkv.to(gpu), case.heads, case.area, ac.SCALE)
        sync(f"{case.name} packed")
    packed = packed.cpu()
    failures, worst = [], 0.0
    for name, (lq, lk, lv, lo), flags in _layouts(C):
        if lq is None:
            qkbuf, qkv_ = guarded_slice((case.B, case.N, 2 * C), *lk, torch.float16, gpu, NAN)
            qkv_.copy_(qk.to(gpu))
            inputs, qv, kv, lq = [qkbuf], qkv_[..., :C], qkv_[..., C:], lk
        else:
            qbuf, qv = guarded_slice(shape, *lq, torch.float16, gpu, NAN)
            kbuf, kv = guarded_slice(shape, *lk, torch.float16, gpu, NAN)
            qv.copy_(qk[..., :C].to(gpu))
            kv.copy_(qk[..., C:].to(gpu))
            inputs = [qbuf, kbuf]
        vbuf, vv = guarded_slice(shape, *lv, torch.float16, gpu, NAN)
        vv.copy_(v.to(gpu))
        inputs.append(vbuf)
        before = [t.clone() for t in inputs]
        obuf, ov = guarded_slice(shape, *lo, torch.float16, gpu)
        lds = (lq[1], lk[1], lv[1], lo[1])
        assert _flags(qv, kv, vv, ov, lds) == flags, (name, _flags(qv, kv, vv, ov, lds))
        what = f"{case.name} {name}"
        with time_limit():
            capi.area_attention_split(qv, kv, vv, case.heads, case.area, ac.SCALE, out=ov, q_ld=lds[0], k_ld=lds[1], v_ld=lds[2], out_ld=lds[3])
            sync(what)
        clean, got = outside_untouched(obuf, lo[0], C)
        if not clean:
            failures.append(f"{name} wrote outside the O slice")
        if not all(_same_bits(a, b) for a, b in zip(inputs, before)):
            failures.append(f"{name} changed an input buffer")
        err = (got.double() - ref.o).abs()
        ratio = (err / ref.bound).max().item()
        worst = max(worst, ratio)
        if not torch.isfinite(got).all() or not (err <= ref.bound).all():
            failures.append(f"{name}: max err / bound {ratio:.3f}, {int((err > ref.bound).sum())} of {err.numel()} elements beyond the bound")
        if not torch.equal(got, packed):
            failures.append(f"{name} is not bit-identical to area_attention_f16: {int((got != packed).sum())} elements differ")
    print(f"{case.name}: max err / bound {worst:.3f} over {len(_layouts(C))} layouts")
    assert not failures, failures


def _refused(gpu, N=32, area=4, ld_q=None, ld_v=None, ld_out=None, **kw):
    B, heads, C = 1, 2, 64
    qk = torch.ones((B, N, 2 * C), dtype=torch.float16, device=gpu)
    v = torch.ones((B, N, C), dtype=torch.float16, device=gpu)
    obuf, ov = guarded_slice((B, N, C), 8, C + 16, torch.float16, gpu)
    with pytest.raises(capi.TrtxError) as e, time_limit():
        capi.area_attention_split(qk[..., :C], qk[..., C:], v, heads, area, ac.SCALE, out=ov, q_ld=ld_q, v_ld=ld_v, out_ld=ld_out or C + 16, **kw)
    sync("split attention refusal")
    assert e.value.status == 4   # TRTX_ERR_UNSUPPORTED
    assert bool((obuf == SENTINEL).all()) and bool((qk == 1).all()) and bool((v == 1).all())


def test_split_attention_refuses_what_it_does_not_implement(gpu):
    _refused(gpu, N=30)            # N % area != 0
    _refused(gpu, kd=16)
    _refused(gpu, hd=64)
    _refused(gpu, ld_q=2 * 32 - 8)     # rows narrower than the heads' channels
    _refused(gpu, ld_v=2 * 32 - 8)
    _refused(gpu, ld_out=2 * 32 - 8)


# ---- the op inside plans -----------------------------------------------------------------------------------------------------------------------------------
def _run(plan, inputs, gpu, what):
    with time_limit():
        e = engine.Engine(plan)
        batch = next(iter(inputs.values())).shape[0]
        bufs = []
        for i in range(e.nb_bindings):
            if e.is_input[i]:
                bufs.append(torch.from_numpy(np.ascontiguousarray(inputs[e.names[i]], dtype=np.float32)).to(gpu))
            else:
                bufs.append(torch.full((int(np.prod(e.dims[i])),), float("nan"), dtype=torch.float32, device=gpu))
        e.enqueue(batch, bufs)
        sync(what)
        out = {e.names[i]: bufs[i].cpu() for i in range(e.nb_bindings) if not e.is_input[i]}
        e.close()
    return out


def _net(*args, **kw):
    """aattn13_net under the watchdog: on a machine with a GPU building a plan times the convolutions' tactics"""
    with time_limit():
        return sc.aattn13_net(*args, **kw)


def _kinds(plan):
    return [o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]]


def _bound(x, weights, heads, area, gain, tail="v"):
    """(the fp64 result, the per-element bound of the module docstring)"""
    o, other, scores, pv_abs, s_abs, pe_abs, vmax = sc.aattn13_reference(x, weights, heads, area, tail)
    if gain > 1:
        assert scores.abs().max().item() > 40   # the large-score case: softmax without max subtraction overflows
        assert (scores.softmax(-1).max(-1).values > 0.99).float().mean().item() > 0.3   # rows one key dominates
    summand = 2 * U16 * other.abs() if tail == "v" else (2 * U16 + 26 * U32) * pe_abs
    return o + other, fp16_walk(2, o.abs() + other.abs()) + 4 * U16 * pv_abs + 2 * U16 * s_abs * vmax + summand + 1e-4 * vmax


# heads, (H, W), area, B, q / k gain, softmax spelling.  Keys per query: 8 (less than one group), 100 (the area-1 spelling), 42 (a partial chunk; both
# spellings), 168 (three chunks), 100 of 400 pixels, 42 with large scores
OP_CASES = [(1, (4, 8), 4, 1, 1.0, "chain"), (2, (10, 10), 1, 3, 1.0, "chain"), (4, (12, 14), 4, 3, 1.0, "chain"), (4, (12, 14), 4, 3, 1.0, "layer"),
            (6, (12, 14), 1, 1, 1.0, "chain"), (2, (20, 20), 4, 3, 1.0, "chain"), (2, (12, 14), 4, 3, 6.0, "chain")]


@pytest.mark.parametrize("heads,hw,area,B,gain,softmax", OP_CASES)
def test_attention_split_op_matches_torch(heads, hw, area, B, gain, softmax, gpu):
    H, W = hw
    plan, x, weights = _net(B, heads, H, W, area, softmax=softmax, gain=gain, seed=heads * 7 + H + area)
    kinds = _kinds(plan)
    assert kinds.count("attention_split") == 1 and not {"matmul", "softmax", "gather"} & set(kinds)
    got = _run(plan, {"x": x}, gpu, "attention_split plan")["y"].reshape(B, heads * 32, H, W).double()
    ref, bound = _bound(x, weights, heads, area, gain)
    err = (got - ref).abs()
    print(f"heads {heads} {H}x{W} area {area} B {B} gain {gain} {softmax}: max err {err.max().item():.3g}, max err / bound {(err / bound).max().item():.3g}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.mark.parametrize("tail", ["v", "pe"])
@pytest.mark.parametrize("heads,hw,area,B,gain", [(4, (12, 14), 4, 3, 1.0), (2, (10, 10), 1, 3, 1.0), (2, (12, 14), 4, 3, 6.0)])
def test_fused_attention_split_agrees_with_generic_lowering(heads, hw, area, B, gain, tail, gpu, monkeypatch):
    H, W = hw
    plan, x, weights = _net(B, heads, H, W, area, tail=tail, gain=gain, seed=heads * 7 + H + area)
    kinds = _kinds(plan)
    assert kinds.count("attention_split") == 1 and (tail == "v" or "ew_nhwc" not in kinds)
    fused = _run(plan, {"x": x}, gpu, "fused")["y"].reshape(B, heads * 32, H, W).double()
    monkeypatch.setenv("TRTX_AATTN_SPLIT", "0")
    kinds = _kinds(plan)
    assert kinds.count("attention_split") == 0 and kinds.count("matmul") == 2 and kinds.count("softmax") == 1
    generic = _run(plan, {"x": x}, gpu, "generic")["y"].reshape(B, heads * 32, H, W).double()
    ref, bound = _bound(x, weights, heads, area, gain, tail)
    print(f"tail {tail}: fused vs fp64 / bound {((fused - ref).abs() / bound).max().item():.3g}, generic vs fp64 / bound "
          f"{((generic - ref).abs() / bound).max().item():.3g}, fused vs generic / bound {((fused - generic).abs() / bound).max().item():.3g}")
    assert torch.isfinite(fused).all() and ((fused - ref).abs() <= bound).all()
    assert ((generic - ref).abs() <= bound).all()
    assert ((fused - generic).abs() <= 2 * bound).all()


def test_attention_split_is_batch_invariant(gpu):
    """Image 0 of a B = 8 run is bit-equal to the same image run alone: the kernel's reduction order does not depend on B (and the 1x1 convolutions on
    16 channels take the same tactic for both)"""
    p8, x, weights = _net(8, 2, 20, 20, 4, seed=3)
    p1, _, _ = _net(1, 2, 20, 20, 4, x=x[:1], weights=weights)
    a = _run(p8, {"x": x}, gpu, "B = 8")["y"].reshape(8, -1)[0]
    b = _run(p1, {"x": x[:1]}, gpu, "B = 1")["y"].reshape(-1)
    assert torch.equal(a, b)
