"""The depthwise and attention tables (tests/dw_cases.py, tests/attention_cases.py) without a GPU: the tables cover what they claim, the fp64
references are conditioned - a torch fp32 restatement of each kernel's arithmetic, rounded to fp16 exactly where the kernel rounds, lies within the
derived bound on every element of every case, so the reference alone passes before a kernel is asked to - and the tables have teeth: restatements
with one plausible kernel bug each leave the bound on at least one case."""
import pytest
import torch

from tests import attention_cases as ac
from tests import dw_cases as dc


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------------------------
def test_dw_table_covers_the_axes():
    assert len({c.name for c in dc.CASES}) == len(dc.CASES)
    for eng in ("f16", "f32"):
        cases = [c for c in dc.CASES if eng in c.engines]
        for k in dc.AXES["k"]:
            for s in dc.AXES["s"]:
                for path in ("vector", "scalar"):
                    assert any(c.k == k and c.s == s and path in c.paths(eng) for c in cases), (eng, k, s, path)
                # the element-wise path by the channel count itself (fp16: C % 8 != 0), not only by the layout of the slice
                if eng == "f16":
                    assert any(c.k == k and c.s == s and c.paths(eng) == {"scalar"} for c in cases), (k, s)
        assert {c.C for c in cases} >= set(dc.AXES["C"]), eng
        assert {(c.H, c.W) for c in cases if c.s == 2} >= set(dc.AXES["s2_maps"])
        for wo in dc.AXES["Wo"]:
            s2 = [c for c in cases if c.s == 2 and c.out_hw[1] == wo]
            assert s2, (eng, wo)
        for r in (1, 2, 3):   # a ragged last strip under stride 2, from an even and from an odd W
            assert {c.W % 2 for c in cases if c.s == 2 and c.out_hw[1] % dc.STRIP == r} == {0, 1}, (eng, r)
        assert {(c.H, c.W) for c in cases if c.k == 7} >= set(dc.AXES["small_k7"])
        assert {c.act1 for c in cases} >= set(dc.AXES["act1"])
        assert any(c.res and c.act2 != "none" for c in cases) and any(c.res and c.act2 == "none" for c in cases)
        assert any(c.res and c.s == 2 for c in cases)
        assert any(not c.bias and not c.res for c in cases) and any(not c.bias and c.res for c in cases)
    c12 = dc.BY_NAME["k3s2_c12_13x17_relu"]      # C 12: whole vectors in fp32, element-wise in fp16
    assert c12.paths("f32") == {"vector", "scalar"} and c12.paths("f16") == {"scalar"}


def test_dw_two_trip_cases_exceed_the_grid():
    big = [c for c in dc.CASES if c.big]
    assert len(big) == 2
    scalar, vector = big
    assert scalar.engines == ("f16",) and scalar.C % 8 != 0 and scalar.work_items(1) > dc.GRID_CAP          # the only path a C of 36 has in fp16
    assert vector.engines == ("f32",) and vector.C % 4 == 0 and vector.work_items(4) > dc.GRID_CAP
    # ... and only just: one row less fits in one trip
    assert (scalar.work_items(1) // scalar.H) * (scalar.H - 1) <= dc.GRID_CAP
    assert (vector.work_items(4) // (vector.N * vector.H)) * (vector.N * vector.H - 1) <= dc.GRID_CAP
    for c in dc.CASES:
        if not c.big:
            assert c.outputs <= 20000 and c.work_items(1) <= dc.GRID_CAP, c.name


def test_attention_table_covers_the_axes():
    assert len({c.name for c in ac.CASES}) == len(ac.CASES)
    ax = ac.AXES["psa"]
    assert {c.heads for c in ac.PSA} >= set(ax["heads"]) and {c.B for c in ac.PSA} >= set(ax["B"]) and {c.N for c in ac.PSA} >= set(ax["N"])
    ax = ac.AXES["area"]
    assert {c.heads for c in ac.AREA} >= set(ax["heads"]) and {c.B for c in ac.AREA} >= set(ax["B"])
    assert {c.area for c in ac.AREA} >= set(ax["area"]) and {c.Na for c in ac.AREA} >= set(ax["Na"])
    assert any(c.area > 1 and c.Na % ac.CHUNK for c in ac.AREA)
    assert {c.Na % ac.GROUP for c in ac.AREA} >= {1, 8}      # three of the four lane groups hold masked keys only
    for kind in (ac.PSA, ac.AREA):
        assert {c.data for c in kind} >= set(ac.AXES["data"]) - {"leak"}
        assert all(c.Na > 2 * ac.CHUNK for c in kind if c.data in ("rising", "falling"))     # at least three chunks
    leaks = [c for c in ac.AREA if c.data == "leak"]
    assert any(c.area > 1 for c in leaks) and any(c.B > 1 and c.area == 1 for c in leaks) and all(c.Na % ac.CHUNK for c in leaks)


# ---- the special data is what it is said to be -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in ac.CASES if c.data != "gauss"])
def test_attention_data_has_the_stated_shape(name):
    c = ac.BY_NAME[name]
    ref = ac.reference(name)
    s = ref.scores
    if c.data == "rising":
        assert (s[..., 1:] > s[..., :-1]).all()
    elif c.data == "falling":
        assert (s[..., 1:] < s[..., :-1]).all()
    elif c.data == "large":
        assert s.abs().max().item() > 40
        assert (s.softmax(-1).max(-1).values > 0.99).double().mean().item() > 0.3
    elif c.data == "tied":
        assert (s == s[..., :1]).all() and s.abs().max().item() > 0.1
        q, k, v = (t.float() for t in ac.split(c, ac.gen_inputs(name)))
        s32 = (ac._blocks(c, q) @ ac._blocks(c, k).transpose(-2, -1)) * ac.SCALE
        assert (s32 == s32[..., :1]).all()      # tied in the kernel's fp32 too
    elif c.data == "leak":
        qkv = ac.gen_inputs(name)
        assert torch.equal(qkv.float().half(), qkv) and torch.isfinite(qkv).all()
        tb, ta = c.target
        v = ac._blocks(c, ac.split(c, qkv)[2].double())
        for b in range(c.B):
            for a in range(c.area):
                m = v[b, :, a].mean().item()
                assert (abs(m) < 1) if (b, a) == (tb, ta) else (abs(abs(m) - ac.LEAK_OFFSET) < 1), (b, a, m)
        # the target's outputs are Gaussian-sized and their bound is far below a leaked key's pull
        img = ref.bound.reshape(c.B, c.area, c.Na, -1)[tb, ta]
        assert img.max().item() < 0.01


# ---- conditioning: the restated kernel arithmetic lies within the bound ----------------------------------------------------------------------------------------
def _dw_runs():
    return [(c.name, e) for c in dc.CASES for e in c.engines]


@pytest.mark.parametrize("name,engine", _dw_runs())
def test_dw_restatement_within_the_bound(name, engine):
    ref = dc.reference(name, engine)
    got = dc.restate(name, engine)
    err = (got.double() - ref.y).abs()
    print(f"{name} {engine}: max err / bound {(err / ref.bound).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= ref.bound).all(), ((err / ref.bound).max().item(), int((err > ref.bound).sum()))
    assert (ref.mag >= ref.y.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("name", ac.IDS)
def test_attention_restatement_within_the_bound(name):
    ref = ac.reference(name)
    got = ac.restate(name)
    err = (got.double() - ref.o).abs()
    print(f"{name}: max err / bound {(err / ref.bound).max().item():.3f}, E_exp / bound up to {(ref.e_exp / ref.bound).max().item():.3f}")
    assert torch.isfinite(got).all() and (err <= ref.bound).all(), ((err / ref.bound).max().item(), int((err > ref.bound).sum()))


# ---- the tables have teeth ---------------------------------------------------------------------------------------------------------------------------------------
def _caught_dw(mutate, cases):
    caught = []
    for c in cases:
        for e in c.engines:
            ref = dc.reference(c.name, e)
            if ((dc.restate(c.name, e, mutate).double() - ref.y).abs() > ref.bound).any():
                caught.append((c.name, e))
    return caught


def _caught_attention(mutate, cases):
    caught = []
    for c in cases:
        ref = ac.reference(c.name)
        got = ac.restate(c.name, mutate).double()
        if not torch.isfinite(got).all() or ((got - ref.o).abs() > ref.bound).any():
            caught.append(c.name)
    return caught


SMALL_DW = [c for c in dc.CASES if not c.big]


def test_dw_border_tap_clamped_instead_of_skipped_is_caught():
    caught = _caught_dw("clamp", SMALL_DW)
    assert len(caught) == sum(len(c.engines) for c in SMALL_DW), "every case has a border"


def test_dw_last_strip_column_from_wo0_plus_3_is_caught():
    ragged = [c for c in SMALL_DW if c.out_hw[1] % dc.STRIP]
    assert {c.out_hw[1] % dc.STRIP for c in ragged} == {1, 2, 3}
    caught = _caught_dw("strip", ragged)
    assert len(caught) == sum(len(c.engines) for c in ragged), set((c.name, e) for c in ragged for e in c.engines) - set(caught)
    assert not _caught_dw("strip", [c for c in SMALL_DW if c.out_hw[1] % dc.STRIP == 0])     # whole strips: the mutation changes nothing


@pytest.mark.parametrize("kind", ["psa", "area"])
def test_attention_without_the_out_of_area_mask_is_caught(kind):
    cases = [c for c in ac.CASES if c.kind == kind]
    step = ac.GROUP if kind == "area" else ac.CHUNK
    caught = _caught_attention("nomask", cases)
    assert set(caught) >= {c.name for c in cases if c.data == "leak"}, caught
    assert not set(caught) & {c.name for c in cases if c.Na % step == 0}          # no partial chunk, nothing to leak


@pytest.mark.parametrize("kind", ["psa", "area"])
def test_attention_without_the_rescale_is_caught(kind):
    cases = [c for c in ac.CASES if c.kind == kind]
    caught = _caught_attention("norescale", cases)
    assert set(caught) >= {c.name for c in cases if c.data == "rising"}, caught
    step = ac.GROUP if kind == "area" else ac.CHUNK
    assert not set(caught) & {c.name for c in cases if c.Na <= step or c.data == "falling"}   # one step, or a max that never rises: no rescale to miss


def test_area_attention_normalised_by_one_lane_group_is_caught():
    caught = _caught_attention("lanegroup", ac.AREA)
    assert set(caught) >= {c.name for c in ac.AREA if c.Na > 8}, set(c.name for c in ac.AREA) - set(caught)
