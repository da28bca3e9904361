"""The layer conformance table (tests/layer_cases.py) on the device: every case through engine.Engine, as an fp32 and as an fp16 plan,
against the case's own torch fp64 reference of the inputs rounded to the engine's storage type (x.half() for the inputs an fp16 plan
puts into an NHWC tensor - the storage site the engine has by design; LINEAR tensors are fp32 in both engines).

Error model, per element, nothing fitted:
  * data movement (Out.mag is None) is exact, bit for bit, in both engines;
  * fp32 arithmetic: |err| <= (1e-5 + n * 2^-24 + amp) * magnitude + 1e-7 - 1e-5 * magnitude + 1e-7 is the bound tests/test_gpu_yolo11.py uses
    for the fp32 depthwise kernel, n * 2^-24 the worst case of the kernel's own sequential fp32 sum of n terms, amp the derived amplification
    of an argument's rounding (softmax, pow), magnitude the same expression on absolute values;
  * fp16 storage: + tests.parity.fp16_walk(sites, magnitude), the sites counted per family in tests/layer_cases.py.
The direct convolution kernels read fp32 weights in both engines (`const float* w` in conv_direct_kernel / deconv_direct_kernel; pack.cpp
packs them with pack_conv_weights_f32 / pack_deconv_weights_f32), so their weights are no rounding site.  The MFMA convolutions and the stem of an
fp16 plan multiply fp16 weights - a rounding of a constant, which the references of the family `conv_mfma` apply themselves (Case.by_precision:
ref(x, fp16) multiplies w.half() in an fp16 plan) rather than count as a site.

Every element of every output binding is compared.  The bindings are allocated for the plan's max_batch and pre-filled with NaN: the
`batch` samples the enqueue covers must be finite afterwards, and with batch < max_batch the rest must still be NaN (the runtime computes
its extents from the enqueue batch; the inputs beyond it hold a finite sentinel, so an op that ran on max_batch samples would show).
Channels of a concat buffer the op under test does not own are compared exactly with what their own producer wrote."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import engine
from tests import layer_cases as lc
from tests.parity import fp16_walk

pytestmark = pytest.mark.gpu


def _run(case, plan, inputs, gpu):
    """{output name: fp32 CPU tensor of the whole binding, max_batch samples}"""
    e = engine.Engine(plan)
    try:
        bufs = []
        for i in range(e.nb_bindings):
            n = int(np.prod(e.dims[i])) * (1 if case.explicit else case.max_batch)
            if e.is_input[i]:
                b = torch.full((n,), 7.0, dtype=torch.float32)
                x = np.ascontiguousarray(inputs[e.names[i]], dtype=np.float32).reshape(-1)
                b[:x.size] = torch.from_numpy(x)
                bufs.append(b.to(gpu))
            else:
                bufs.append(torch.full((n,), float("nan"), dtype=torch.float32, device=gpu))
        e.enqueue(case.batch, bufs)
        torch.cuda.synchronize()
        return {e.names[i]: bufs[i].cpu() for i in range(e.nb_bindings) if not e.is_input[i]}
    finally:
        e.close()


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("case", lc.CASES, ids=[c.name for c in lc.CASES])
def test_layer_matches_fp64_reference(case, fp16, gpu):
    plan = lc.build_plan(case, fp16)
    kinds = {o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"]}
    assert case.kinds_for(fp16) <= kinds and not case.absent_for(fp16) & kinds, sorted(kinds)
    inputs = lc.gen_inputs(case)
    got = _run(case, plan, inputs, gpu)
    expected = lc.outs_of(case, lc.ref_inputs(case, inputs, fp16), fp16)
    assert set(got) == set(expected)
    for name, outs in expected.items():
        flat = got[name]
        for o in outs:
            if not o.batched:
                vol = o.ref.numel()
                g, rest = flat[:vol].reshape(o.ref.shape).double(), flat[vol:]
            else:
                per = flat.numel() if case.explicit else flat.numel() // case.max_batch
                used = per if case.explicit else per * case.batch
                full = [o.ref.shape[0]] + ([-1] if o.ch is not None else []) + list(o.ref.shape[2 if o.ch is not None else 1:])
                g, rest = flat[:used].reshape(full).double(), flat[used:]
                if o.ch is not None:
                    g = g[:, o.ch]
            assert g.shape == o.ref.shape, (name, g.shape, o.ref.shape)
            assert torch.isfinite(g).all(), name
            assert torch.isnan(rest).all(), f"{name}: written beyond the {case.batch} sample(s) of the enqueue"
            if o.mag is None:
                bad = g != o.ref
                print(f"{case.name} fp16={fp16} {name}: exact, {int(bad.sum())} of {g.numel()} differ")
                assert not bad.any(), (name, int(bad.sum()), (g - o.ref).abs().max().item())
            else:
                bound = lc.fp32_bound(o) + (fp16_walk(o.sites, o.mag) if fp16 and o.sites else 0.0)
                err = (g - o.ref).abs()
                print(f"{case.name} fp16={fp16} {name}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
                assert (err <= bound).all(), (name, err.max().item(), (err / bound).max().item())
