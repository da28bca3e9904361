"""The convolution geometry table (tests/conv_cases.py) on the host: every case is accepted by the MFMA launchers, the table covers the axes it
claims, and its references are conditioned well enough to catch what tests/test_gpu_conv_geometry.py is there to catch - all of it computed from
the references alone, so that nothing here can be fitted to a kernel."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import builder, capi, engine
from tests import conv_cases as cc

DEGENERATE_3X3 = [c for c in cc.CASES if c.degenerate and c.k == (3, 3)]


def _tactics(c, **kw):
    return capi.conv2d_tactics(c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.s, c.p, residual=c.res, **kw)


def _tactics_f32(c, **kw):
    return capi.conv2d_tactics_f32(c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.s, c.p, residual=c.res, **kw)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_every_case_is_accepted_and_small(case):
    Ho, Wo = case.out_hw
    assert Ho >= 1 and Wo >= 1
    assert case.degenerate or 130 <= case.rows <= 1000, case.rows
    assert case.degenerate or case.rows % 128, "a ragged last tile"
    for eng, fn in (("f16", _tactics), ("f32", _tactics_f32)):
        if eng in case.engines:
            t = fn(case)
            assert t and len(set(t)) == len(t), (eng, t)
            wide = fn(case, ld_out=case.Cout + 22)   # the element-wise epilogue of a misaligned slice is accepted too
            assert wide and len(set(wide)) == len(wide), (eng, wide)
    if "i8" in case.engines:
        assert case.Cin % 16 == 0 and case.Cout % 8 == 0
    assert "f16" not in case.engines or case.Cin % 8 == 0
    assert case.Cin % 4 == 0


def test_the_wrappers_take_pairs_and_ints_alike():
    assert capi.conv2d_tactics(2, 20, 20, 64, 64, 3, 1, 1) == capi.conv2d_tactics(2, 20, 20, 64, 64, (3, 3), (1, 1), (1, 1))
    assert capi.conv2d_tactics_f32(2, 20, 20, 64, 64, 3, 2, 1) == capi.conv2d_tactics_f32(2, 20, 20, 64, 64, (3, 3), (2, 2), (1, 1))
    assert capi.conv2d_tactics(2, 20, 20, 64, 64, (3, 5), (2, 1), (1, 2)) != capi.conv2d_tactics(2, 20, 20, 64, 64, 3, 1, 1)
    assert capi.conv2d_tactics(2, 20, 20, 64, 64, (1, 3), 1, (0, 1)) and capi.conv2d_tactics(2, 20, 20, 64, 64, (3, 1), 1, (1, 0))


@pytest.mark.parametrize("case", DEGENERATE_3X3, ids=[c.name for c in DEGENERATE_3X3])
def test_degenerate_maps_list_the_special_case_kernels(case):
    """the sets are spelled out per map in tests/conv_cases.py (EXPECT_WS) and asserted again, of what was actually launched, by the device test: a
    predicate that tightens fails here instead of turning a case into no case.  The special-case kernels store whole vectors only, so a misaligned
    slice must list none of them."""
    want = cc.EXPECT_WS[case.name]
    ws = {t[4] for t in _tactics(case)}
    assert want["f16"] <= ws, (want["f16"], ws)
    ws32 = {t[2] for t in _tactics_f32(case)}
    assert want["f32"] <= ws32, (want["f32"], ws32)
    assert not {t[4] for t in _tactics(case, ld_out=case.Cout + 22)} & {2, 3, 7, 8}
    assert not {t[2] for t in _tactics_f32(case, ld_out=case.Cout + 22)} & {3, 7}


def test_the_special_case_kernels_are_all_met_on_degenerate_maps():
    assert set(cc.EXPECT_WS) == {c.name for c in DEGENERATE_3X3}
    seen, seen32 = set(), set()
    for want in cc.EXPECT_WS.values():
        seen |= want["f16"]
        seen32 |= want["f32"]
    assert {1, 2, 3, 7, 8} <= seen, seen
    assert {3, 7} <= seen32, seen32
    names = {c.name.split("_")[1] for c in DEGENERATE_3X3}
    assert {"1x9", "9x1", "1x1", "1x16", "3x2"} <= names
    for short in ("1x9", "9x1", "1x1", "1x16", "3x2"):   # each of the five maps meets at least one special-case fp16 kernel
        assert any(w["f16"] & {2, 3, 7, 8} for n, w in cc.EXPECT_WS.items() if n.split("_")[1] == short), short


def test_the_table_covers_its_axes():
    for eng in ("f16", "f32"):
        cases = [c for c in cc.CASES if eng in c.engines]
        for axis, values in cc.AXES.items():
            for v in values:
                assert any(getattr(c, axis) == v for c in cases), (eng, axis, v)
        has = lambda f: any(f(c) for c in cases)  # noqa: E731
        assert has(lambda c: c.k == (3, 3) and c.p == (0, 0)) and has(lambda c: c.k == (1, 7) and c.p == (0, 0))
        assert has(lambda c: c.k == (3, 3) and c.p == (2, 2))
        assert has(lambda c: c.k == (1, 1) and c.p == (1, 1)) and has(lambda c: c.p[0] >= c.k[0] and c.p[1] >= c.k[1] and c.k != (1, 1))   # padding >= k
        assert has(lambda c: c.k == (1, 1) and c.s == (2, 2))
        assert has(lambda c: c.s[0] > c.k[0] and c.s[1] > c.k[1] and c.k != (1, 1))
        assert has(lambda c: c.taps == 30)
        assert has(lambda c: c.Cin == 16 and c.taps % 2 == 1 and c.k == (1, 3)) and has(lambda c: c.Cin == 16 and c.k == (5, 5))
        assert has(lambda c: c.res and c.act2 != "none" and c.k[0] != c.k[1]) and has(lambda c: c.res and c.act2 != "none" and c.s != (1, 1))
        assert has(lambda c: c.act1 == "leaky")
    f16 = [c for c in cc.CASES if "f16" in c.engines]
    assert any(c.k[0] != c.k[1] and c.taps * ((c.Cin + 31) // 32) > 64 for c in f16), "a rectangular kernel whose 64-step window is rebuilt"
    f32 = [c for c in cc.CASES if "f32" in c.engines]
    assert any(c.Cin == 4 and c.k[0] != c.k[1] for c in f32) and any(c.Cin == 8 and c.k[0] != c.k[1] for c in f32)
    i8 = [c for c in cc.CASES if "i8" in c.engines]
    assert any(c.k[0] != c.k[1] for c in i8) and any(c.s != (1, 1) for c in i8) and any(c.p[0] > c.k[0] // 2 for c in i8) and any(c.res for c in i8)
    assert any(not c.res for c in i8)


def test_padding_beyond_the_filter_leaves_rows_that_are_the_bias():
    """where no tap lies inside the image the sum is the bias alone: the references of those cases do contain such elements (magnitude == |bias|)"""
    for c in cc.CASES:
        if c.p[0] >= c.k[0] and not c.res:
            ref = cc.reference(c.name, c.engines[0])
            b = cc.gen_inputs(c.name)["bias"].double().abs()
            assert (ref.mag[:, 0] == b).all() and (ref.mag[:, -1] == b).all(), c.name
            assert not (ref.mag[:, ref.mag.shape[1] // 2] == b).all(), c.name


def test_a_36_tap_filter_is_refused_by_the_mfma_launchers_and_lowers_to_the_direct_kernel():
    assert capi.conv2d_tactics(1, 12, 12, 32, 32, 6, 1, 3) == [] and capi.conv2d_tactics_f32(1, 12, 12, 32, 32, 6, 1, 3) == []
    assert capi.conv2d_tactics(1, 12, 12, 32, 32, (5, 6), 1, 3) and capi.conv2d_tactics_f32(1, 12, 12, 32, 32, (5, 6), 1, 3)
    w = np.zeros((32, 32, 6, 6), np.float32)
    for fp16 in (0, 1):
        net = builder.Network(max_batch=1, fp16=bool(fp16))
        try:
            x = net.out(net.pooling(net.input("x", (32, 12, 12)), 1, 1))
            net.mark_output(net.out(net.conv(x, w, None, 1, 3)), "y")
            desc = engine.describe_plan(net.build(), lowered=True)
        finally:
            net.close()
        (conv,) = [o for o in desc["ops"] if o["kind"] == "conv"]
        assert not (conv["igemm"] or conv["stem"] or conv.get("dw")), conv


@pytest.mark.parametrize("case", [c for c in cc.CASES if "i8" in c.engines and not c.res], ids=lambda c: c.name)
def test_int8_outputs_near_a_rounding_boundary_are_few(case):
    q, near, s_out = cc.i8_expected(case.name)
    share = near.double().mean().item()
    print(f"{case.name}: {share:.4f} of the requantised outputs may move by one step")
    assert share <= cc.I8_NEAR_CAP, share
    assert q.abs().max() == 127 and s_out > 0


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_every_tap_matters_more_than_the_bound(case):
    """Sensitivity, from the reference alone: a case whose bound is wider than what one filter tap contributes could not tell a kernel that drops a tap
    from a correct one.  For randn inputs and He-scaled weights the expected share is 0.9 and more (the contribution of one tap is N(0, 2 / taps),
    the bound 7e-4 of a sum of absolute values): required 0.8 of the outputs where the tap lies inside the image."""
    for eng in case.engines:
        ref = cc.reference(case.name, eng)
        assert torch.isfinite(ref.y).all() and ref.y.abs().max() < 60000 and (ref.mag >= ref.y.abs() * (1 - 1e-12)).all()
        shares = cc.tap_share(case.name, eng)
        assert shares, "no tap inside the image"
        worst = min(shares, key=shares.get)
        print(f"{case.name} {eng}: worst tap {worst} share {shares[worst]:.3f} over {len(shares)} taps")
        assert shares[worst] >= 0.8, (eng, worst, shares[worst])
