"""The hypergraph-convolution table (tests/hgconv_cases.py) on the device: trtx_op_hgconv_f16 through the C ABI against the table's fp64 reference of the
unfolded definition, every element under the per-element bound derived there.

Layouts.  Every case runs twice: on dense tensors, and with x as a channel slice of a wider buffer whose other channels and guard images are NaN and out
as a channel slice of a buffer pre-filled with a sentinel (tests/util.py).  A token of a pixel outside the batch or a channel outside the tensor that
reaches a result shows as NaN, a store outside the slice shows in the sentinel, and both layouts must agree bit for bit.  On top of that: image i of a
batch against the same image run alone, two runs of one call, the fused op against the generic lowering of the same subgraph, and the refusals."""
import collections

import numpy as np
import pytest
import torch

from tensorrtx_amd import capi, engine
from tests import hgconv_cases as hc
from tests.util import SENTINEL, guarded_slice, outside_untouched, sync, time_limit

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev_weights(w, gpu):
    return {k: torch.from_numpy(v).to(gpu) for k, v in w.items()}


def _run(c, x, w, gpu, sliced):
    """-> (out on the host, whether everything outside the output slice is untouched)"""
    B, N, D = x.shape
    if sliced:
        _, xv = guarded_slice((B, N, D), 8, D + 24, torch.float16, gpu, NAN)
        xv.copy_(x.to(gpu))
        obuf, ov = guarded_slice((B, N, D), 16, D + 40, torch.float16, gpu)
        lds = (D + 24, D + 40)
    else:
        xv = x.to(gpu)
        obuf, ov = guarded_slice((B, N, D), 0, D, torch.float16, gpu)
        lds = (D, D)
    with time_limit():
        capi.hgconv(xv, c.E, hc.logit_scale(D), w, out=ov, x_ld=lds[0], out_ld=lds[1], D=D)
        sync(f"{c.name} {'sliced' if sliced else 'dense'}")
    clean, got = outside_untouched(obuf, 16 if sliced else 0, D)
    return got, clean


@pytest.mark.parametrize("name", hc.IDS)
def test_every_case_matches_fp64_in_both_layouts(gpu, name):
    c = hc.BY_NAME[name]
    x, w = hc.gen(name)
    ref = hc.reference(name)
    wd = _dev_weights(w, gpu)
    dense, clean_d = _run(c, x, wd, gpu, False)
    sliced, clean_s = _run(c, x, wd, gpu, True)
    err = (dense.double() - ref.out).abs()
    ratio = (err / ref.bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, max err / bound {ratio:.3f}")
    assert clean_d and clean_s, "a store outside the output slice"
    assert torch.isfinite(dense).all()
    assert (err <= ref.bound).all(), (ratio, int((err > ref.bound).sum()))
    assert torch.equal(dense, sliced), f"{int((dense != sliced).sum())} elements differ between the layouts"


@pytest.mark.parametrize("name", ["d384e12_1x257_b3_gauss", "d64e4_5x13_b3_ctx", "d256e8_3x43_b3_negative"])
def test_image_of_a_batch_equals_the_image_alone_and_runs_repeat(gpu, name):
    c = hc.BY_NAME[name]
    x, w = hc.gen(name)
    wd = _dev_weights(w, gpu)
    whole, _ = _run(c, x, wd, gpu, False)
    again, _ = _run(c, x, wd, gpu, False)
    assert torch.equal(whole, again), "two runs of one call differ"
    for i in range(c.B):
        alone, _ = _run(c, x[i:i + 1].contiguous(), wd, gpu, False)
        assert torch.equal(alone[0], whole[i]), f"image {i}: {int((alone[0] != whole[i]).sum())} elements differ from the batch of {c.B}"


def _engine_run(plan, x, gpu):
    e = engine.Engine(plan)
    bufs = []
    for i in range(e.nb_bindings):
        if e.is_input[i]:
            bufs.append(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu))
        else:
            bufs.append(torch.full((int(np.prod(e.dims[i])),), NAN, dtype=torch.float32, device=gpu))
    with time_limit():
        e.enqueue(x.shape[0], bufs)
        sync("subgraph engine")
    out = {e.names[i]: bufs[i].cpu() for i in range(e.nb_bindings) if not e.is_input[i]}
    e.close()
    return out


@pytest.mark.parametrize("D,E,hw", [(64, 4, (12, 14)), (128, 8, (20, 20)), (384, 12, (6, 6))])
def test_fused_subgraph_agrees_with_the_generic_lowering(gpu, monkeypatch, D, E, hw):
    """conv -> AdaHGComputation -> concat -> conv at B = 3, the hypergraph convolution's result marked as an output ("m"): the fused op lies within the
    table's bound of the fp64 reference computed from cv1's fp16 output, the generic lowering (TRTX_HGCONV=0) within its own - the fused bound plus the
    fp16 sites only that path has (fp16 weights, inputs and stored outputs of its four fully connected layers, the stored GELU results:
    hgconv_cases.reference_of) - and the two agree within the sum of both bounds."""
    B, (H, W) = 3, hw
    _, w = hc.gen(hc._c(D, E, (5, 7), 3).name)
    w = dict(w, w_node=(w["w_node"] * np.float32(max(1.0, H * W / (2.0 * E)) / max(1.0, 35 / (2.0 * E)))))   # node_proj's gain for this N (hgconv_cases.gen)
    cw = hc.c3ah_weights(D, seed=7)
    plan = hc.subgraph_net(B, D, E, H, W, w, cw, mark_inner=True)
    x = np.random.default_rng(11).standard_normal((B, 3, H, W)).astype(np.float32)
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert kinds["hgconv"] == 1 and kinds["matmul"] == 0 and kinds["softmax"] == 0, kinds
    fused = _engine_run(plan, x, gpu)
    monkeypatch.setenv("TRTX_HGCONV", "0")
    kinds = collections.Counter(o["kind"] for o in engine.describe_plan(plan, lowered=True)["ops"])
    assert kinds["hgconv"] == 0 and kinds["matmul"] == 3 and kinds["softmax"] == 1, kinds
    generic = _engine_run(plan, x, gpu)
    tokens = lambda t: t.reshape(B, D, H * W).transpose(1, 2)   # noqa: E731
    x1 = tokens(fused["x1"])
    assert torch.equal(x1, tokens(generic["x1"])) and torch.equal(x1.half().float(), x1), "cv1's fp16 output, the same on both paths"
    ref = hc.reference_of(x1, w, D, E)
    ef, eg = (tokens(fused["m"]).double() - ref.out).abs(), (tokens(generic["m"]).double() - ref.out).abs()
    d = (tokens(fused["m"]).double() - tokens(generic["m"]).double()).abs()
    both = ref.bound + ref.bound_generic
    print(f"D {D} E {E} {H}x{W}: fused / bound {(ef / ref.bound).max().item():.3f}, generic / its bound {(eg / ref.bound_generic).max().item():.3f}, "
          f"fused vs generic / (sum of both bounds) {(d / both).max().item():.3f}, median generic bound / fused bound "
          f"{(ref.bound_generic.median() / ref.bound.median()).item():.1f}")
    assert torch.isfinite(fused["y"]).all() and torch.isfinite(generic["y"]).all()
    assert (ef <= ref.bound).all()
    assert (eg <= ref.bound_generic).all()
    assert (d <= both).all()


def test_refusals_return_their_status_without_a_launch(gpu):
    c = hc.BY_NAME["d64e4_5x7_b3_gauss"]
    x, w = hc.gen(c.name)
    wd = _dev_weights(w, gpu)
    B, N, D = x.shape
    xd = x.to(gpu)

    def refused(status, **kw):
        obuf, ov = guarded_slice((B, N, D), 8, D + 16, torch.float16, gpu)
        args = dict(x=xd, E=c.E, logit_scale=hc.logit_scale(D), weights=wd, out=ov, out_ld=D + 16, D=D)
        args.update(kw)
        with pytest.raises(capi.TrtxError) as e, time_limit():
            capi.hgconv(args.pop("x"), args.pop("E"), args.pop("logit_scale"), args.pop("weights"), **args)
        sync("hgconv refusal")
        assert e.value.status == status, kw
        assert bool((obuf == SENTINEL).all()), kw

    refused(4, E=17)                                                                    # TRTX_ERR_UNSUPPORTED
    refused(4, D=24, x_ld=D)                                                            # D % 16 != 0
    refused(4, out_ld=D + 12)                                                           # a pixel stride that rules out 16-byte stores
    refused(4, x=torch.zeros((B, N, D + 8), dtype=torch.float16, device=gpu)[:, :, 4:4 + D])   # x 8 bytes into a row
    refused(1, x_ld=D - 8)                                                              # TRTX_ERR_INVALID
    refused(1, workspace=torch.empty(capi.hgconv_workspace_bytes(B, N, D, c.E) - 256, dtype=torch.uint8, device=gpu))
