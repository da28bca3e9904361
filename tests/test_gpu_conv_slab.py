"""kernels/conv_slab.hip on the device: every case of tests/conv_slab_cases.py as ONE C-ABI launch into a sentinel-framed channel slice (one guard image in
front and one behind), NaN beside the input view, against torch fp64 under the table's bound.  A cross-group leak would be an O(1) error."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import capi
from tests import conv_slab_cases as sc
from tests import util

pytestmark = pytest.mark.gpu


def _nhwc_f16(a_nchw, gpu, view=None):
    """the NHWC fp16 tensor on the device; view (offset, channels): that channel slice, every other channel NaN"""
    t = torch.from_numpy(np.ascontiguousarray(a_nchw.transpose(0, 2, 3, 1))).half()
    if view:
        t[..., :view[0]] = t[..., sum(view):] = float("nan")
    return t.to(gpu)[..., view[0]:sum(view)] if view else t.to(gpu)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_single_launch_matches_fp64_and_stays_inside_its_slice(gpu, case):
    d = sc.gen(case)
    ref, bound = sc.reference(case, d)
    off, ld = case.out_view if case.out_view else (8, case.C + 24)
    x = _nhwc_f16(d["x"], gpu, (case.in_view[0], case.C) if case.in_view else None)
    r = _nhwc_f16(d["r"], gpu) if case.res else None
    w = torch.from_numpy(capi.pack_conv_weights_slab_f16(d["w"], case.groups).view(np.float16)).to(gpu)
    buf, out = util.guarded_slice((case.N, *ref.shape[2:], case.C), off, ld, torch.float16, gpu)
    with util.time_limit():
        capi.conv2d_slab_nhwc_f16(x, w, torch.from_numpy(d["b"]).to(gpu), case.groups, case.stride, case.act1, r, case.act2, out=out, out_ld=ld)
        util.sync(case.name)
    clean, got = util.outside_untouched(buf, off, case.C)
    assert clean, "written outside the slice"
    err = (got.permute(0, 3, 1, 2).double() - ref).abs()
    print(f"{case.name}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), ((err / bound).max().item(), int((err > bound).sum()), err.numel())
