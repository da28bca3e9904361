"""The fused YOLOv8 / YOLO11 head table (tests/yolo_head_cases.py) without a GPU: the table covers what it claims, the reference meets the
conditions under which a GPU comparison may leave out no record at all (every probability off the gate, no accidental tie, no keypoint on
a box edge or on kpt_conf), each family's data is what it is said to be, and an fp32 NumPy restatement of both DFL orders of the kernel
(acc / sum, and fmaf(ex * inv, w, acc)) stays under the derived bound on every element of every case - so the reference alone passes
before a kernel is asked to."""
import ctypes

import numpy as np
import pytest

from tests import yolo_head_cases as hc

ALL = [(c.name, dt) for c in hc.CASES for dt in hc.DTYPES]


def _ids(v):
    return v if isinstance(v, str) else None


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------------
def test_table_covers_the_axes():
    assert len({c.name for c in hc.CASES}) == len(hc.CASES)
    for geom, (H, W, strides) in hc.GEOMS.items():
        assert sum(hc.level_cells(geom)) == hc.CELLS[geom]
        assert all(s & (s - 1) == 0 for s in strides)          # the error model takes '* stride' to be exact
        for fam in hc.FAMILIES:
            for head in ("det", "task"):
                assert any(c.geom == geom and c.family == fam and c.head == head for c in hc.CASES), (geom, fam, head)
        seeded = [c for c in hc.CASES if c.geom == geom and c.family == "seeded"]
        assert any(("exact", "exact") in c.layouts for c in seeded if c.head == "det")
        assert any(("exact", "exact") in c.layouts for c in seeded if c.head == "task")
    assert hc.level_cells("64x96") == [96, 24, 6] and hc.level_cells("160x160") == [400, 100, 25]
    assert hc.level_cells("128x128") == [256, 64, 16, 4] and hc.level_cells("64x64") == [64, 16, 4, 1] and hc.level_cells("40x56") == [35, 6]
    det, task = [c for c in hc.CASES if c.head == "det"], [c for c in hc.CASES if c.head == "task"]
    assert {c.classes for c in det} == {80, 8} and {c.classes for c in task} == {1, 13, 15, 80, 8}
    assert {c.B for c in hc.CASES} == {2, 3}
    assert {(c.task, c.nk) for c in task} >= {("seg", 17), ("pose", 17), ("pose", 5), ("obb", 17)}
    assert any(c.task == "seg" and ("pad", "odd") in c.layouts for c in task) and any(c.task == "pose" and ("pad", "odd") in c.layouts for c in task)
    assert any(c.classes == 13 and c.family == "ties" for c in task)         # full = 8: five logits in the element tail
    assert sum(c.dfl == "arange" for c in hc.CASES) == 1
    over = hc.BY_NAME["det_64x96_overflow_nc80"] if "det_64x96_overflow_nc80" in hc.BY_NAME else hc.BY_NAME["det_64x96_overflow_nc8"]
    assert over.mo == 40
    for c in hc.CASES:
        for dt in hc.DTYPES:
            vec = hc.VEC[dt]
            assert hc.head_ld(c, dt, "pad") == hc.round_up(64 + c.classes, vec) + vec
            assert hc.head_ld(c, dt, "exact") >= 64 + c.classes and hc.head_ld(c, dt, "exact") % vec == 0
            if c.head == "det":
                assert hc.head_ld(c, dt, "exact") == 64 + c.classes
            if c.task:
                assert hc.branch_ld(c, dt, "odd") % 2 == 1 and hc.branch_ld(c, dt, "odd") >= c.extra and hc.branch_ld(c, dt, "pad") % vec == 0


def test_every_gate_value_sits_at_every_kind_of_position():
    """first and last lane of a wave, the last cell of a level and the first of the next: each logit of family (c), for each storage type and
    each head, somewhere in the table"""
    for dt in hc.DTYPES:
        for head in ("det", "task"):
            seen = set()
            for c in hc.CASES:
                if c.family != "threshold" or c.head != head:
                    continue
                pos = hc.positions(c.geom)
                for (b, g), (v, _, _) in hc.build(c.name, dt).expect["gate"].items():
                    seen |= {(v, k) for k in hc.KINDS if g in pos[k]}
            missing = {(v, k) for v, _, _ in hc.thresholds(dt) for k in hc.KINDS} - seen
            assert not missing, (dt, head, missing)


def test_gate_values_are_where_the_pre_filter_and_the_gate_put_them():
    for dt in hc.DTYPES:
        for v, flagged, kept in hc.thresholds(dt):
            assert hc.to_grid(np.array([v]), dt)[0] == v                       # held exactly
            assert (np.float32(v) > np.float32(-2.3)) == flagged
            p32 = np.float32(1) / (np.float32(1) + np.exp(-np.float32(v), dtype=np.float32))
            p64 = 1 / (1 + np.exp(-float(v)))
            assert (not (float(p32) < 0.1)) == kept and (p64 >= 0.1) == kept
            assert abs(p64 - 0.1) > 40 * 2.0 ** -27, (v, p64)                # 40 ulps of 0.1 and more: expf's ulp cannot move it across
    assert sum(k for _, _, k in hc.THRESH32) == 2 and sum(f and not k for _, f, k in hc.THRESH32) == 4


def test_tie_pairs_reach_pieces_and_tail():
    assert hc.tie_pairs(80) == [(0, 79), (41, 42), (17, 75)]
    assert hc.tie_pairs(8) == [(0, 7), (1, 2)]
    p13 = hc.tie_pairs(13)
    assert (7, 8) in p13 and (8, 12) in p13 and (0, 12) in p13 and any(lo < 8 <= hi for lo, hi in p13)
    for nc in (8, 13, 15, 80):
        assert all(0 <= lo < hi < nc for lo, hi in hc.tie_pairs(nc))


# ---- the conditions of a comparison that leaves out nothing -----------------------------------------------------------------------------------------------
def _sigmoid64(x):
    with np.errstate(all="ignore"):
        return 1 / (1 + np.exp(-x.astype(np.float64)))


@pytest.mark.parametrize("name,dt", ALL, ids=_ids)
def test_reference_meets_the_conditions(name, dt):
    c, bt, ref = hc.BY_NAME[name], hc.build(name, dt), hc.reference(name, dt)
    kept = hc.kept_cells(name, dt)
    # counts: the oracle's, the logits' own, the family's
    for b in range(c.B):
        assert ref[b, 0] == min(len(kept[b]), c.mo), (b, ref[b, 0], len(kept[b]))
        if c.family == "seeded":
            assert 3 <= ref[b, 0] < c.mo, (b, ref[b, 0])
    for b, n in bt.expect.get("counts", {}).items():
        assert ref[b, 0] == n, (b, ref[b, 0], n)
    # every probability that was not placed at the gate is farther than 1e-6 from it
    p = _sigmoid64(bt.logits)
    free = ~bt.delib[..., None] & ~np.isnan(bt.logits)
    assert (np.abs(p - hc.GATE)[free] > 1e-6).all()
    # no accidental tie for the maximum
    lg = np.where(np.isnan(bt.logits), -np.inf, bt.logits)
    top = lg.max(-1, keepdims=True)
    assert (((lg == top).sum(-1) == 1) | bt.delib).all()
    if c.classes > 1:   # and the winner of a kept cell wins by more than a confidence's error
        second = np.sort(p, -1)[..., -2]
        for b in range(c.B):
            g = kept[b][~bt.delib[b][kept[b]]]
            assert (p[b, g].max(-1) - second[b, g] > 1e-6).all()
    row, col, stride = hc.cell_geometry(c.geom)
    for b in range(c.B):
        R, g = hc.records(ref, b), kept[b][:int(ref[b, 0])]
        assert np.array_equal(R[:, 5], np.nanargmax(np.where(np.isnan(bt.logits[b, g]), -np.inf, bt.logits[b, g]), -1))
        if c.task == "pose":
            kp = bt.branch[b, g].astype(np.float64).reshape(len(g), c.nk, 3)
            kx = (kp[..., 0] * 2 + col[g][:, None]) * stride[g][:, None]
            ky = (kp[..., 1] * 2 + row[g][:, None]) * stride[g][:, None]
            box = R[:, None, :4].astype(np.float64)
            with np.errstate(invalid="ignore"):
                edge = np.minimum(np.minimum(np.abs(kx - box[..., 0]), np.abs(kx - box[..., 2])), np.minimum(np.abs(ky - box[..., 1]), np.abs(ky - box[..., 3])))
            assert not (edge <= 1e-2).any(), (b, np.nanmin(edge))
            assert (np.abs(_sigmoid64(kp[..., 2]) - c.kpt_conf) > 1e-5).all()
            out = R[:, 38:38 + 3 * c.nk]
            if c.family == "seeded":
                assert (out == -1).any() and (out != -1).any()
        if c.task == "seg":
            assert np.array_equal(R[:, 6:38], bt.branch[b, g])


def test_pose_cases_suppress_by_confidence_and_by_the_box():
    by_conf = by_box = 0
    for c in hc.CASES:
        if c.task != "pose" or c.family != "seeded":
            continue
        for dt in hc.DTYPES:
            bt, ref, kept = hc.build(c.name, dt), hc.reference(c.name, dt), hc.kept_cells(c.name, dt)
            for b in range(c.B):
                R, g = hc.records(ref, b), kept[b]
                conf = _sigmoid64(bt.branch[b, g].reshape(len(g), c.nk, 3)[..., 2])
                gone = R[:, 38:38 + 3 * c.nk].reshape(len(g), c.nk, 3)[..., 2] == -1
                by_conf += int((gone & (conf < c.kpt_conf)).sum())
                by_box += int((gone & (conf > c.kpt_conf)).sum())
                assert not (~gone & (conf < c.kpt_conf)).any()
    assert by_conf > 10 and by_box > 10, (by_conf, by_box)


# ---- each family's data is what it is said to be ------------------------------------------------------------------------------------------------------------
def _slot_of(kept_b, g):
    hit = np.nonzero(kept_b == g)[0]
    return int(hit[0]) if len(hit) else None


@pytest.mark.parametrize("name,dt", [(n, d) for n, d in ALL if hc.BY_NAME[n].family != "seeded"], ids=_ids)
def test_family_properties(name, dt):
    c, bt, ref = hc.BY_NAME[name], hc.build(name, dt), hc.reference(name, dt)
    kept = hc.kept_cells(name, dt)
    if c.family == "overflow":
        # the clamped rows are the first max_out of the canonical order
        full = hc.reference(name, dt, c.cells + 1)
        assert ref[1, 0] == 0 and ref[2, 0] == c.mo and full[2, 0] == c.cells and c.mo < c.cells
        assert np.array_equal(hc.records(full, 2)[:c.mo], hc.records(ref, 2), equal_nan=True)
    if c.family == "full":
        assert ref[1, 0] == 0 and ref[2, 0] == c.cells and c.mo == c.cells + 1
    if c.family == "threshold":
        gate = bt.expect["gate"]
        # (a net with fewer boundary cells than values holds some of them; test_every_gate_value_sits_at_every_kind_of_position counts the table's)
        assert len(gate) >= 12 and {v for v, _, _ in gate.values()} <= {v for v, _, _ in hc.thresholds(dt)}
        for (b, g), (v, _, keep) in gate.items():
            assert bt.logits[b, g].max() == np.float32(v) and (bt.logits[b, g] > -29).sum() == 1
            slot = _slot_of(kept[b], g)
            assert (slot is not None) == keep, (b, g, v)
            if keep:
                assert abs(hc.records(ref, b)[slot, 4] - 1 / (1 + np.exp(-v))) < 1e-7
    if c.family == "ties":
        for b in range(c.B):
            assert np.array_equal(hc.records(ref, b)[:, 5], bt.expect["classes"][b])
        lo, hi = hc.tie_pairs(c.classes)[0]
        assert hc.records(ref, 1)[0, 5] == hi and hc.records(ref, 0)[0, 5] == lo
        assert bt.expect["ties_broken"] == 0
    if c.family == "naninf":
        for b, g in bt.expect["dropped"]:
            assert np.isnan(bt.logits[b, g]).all() and _slot_of(kept[b], g) is None
            assert _slot_of(kept[b], g - 1) is not None and (np.isnan(bt.logits[b, g - 1]).sum() == c.classes - 1)
        for b, g in bt.expect["inf"]:
            assert hc.records(ref, b)[_slot_of(kept[b], g), 4] == 1.0
        for b, g in bt.expect["nanbox"]:
            r = hc.records(ref, b)[_slot_of(kept[b], g)]
            assert np.isnan(r[:4]).any() and not np.isnan(r[4:6]).any()
            if not c.task or c.task != "obb":
                assert np.isnan(r[:4]).tolist() == [False, True, False, False]
    if c.family == "dfl":
        d = hc.dfl64(name, dt)[0]
        w = bt.dfl_w.astype(np.float64)
        for b, g in bt.expect["equal"]:
            assert np.allclose(d[b, g], w.mean(), rtol=1e-15) and _slot_of(kept[b], g) is not None
        for b, g in bt.expect["onehot"]:
            assert np.array_equal(d[b, g], w[list(bt.expect["onehot_bins"])]) and _slot_of(kept[b], g) is not None
        for b, g in bt.expect["wide"]:
            x = bt.bins[b, g]
            assert ((x.max(-1) - x.min(-1)) > 88).all() and np.isfinite(d[b, g]).all() and _slot_of(kept[b], g) is not None


# ---- the error model ----------------------------------------------------------------------------------------------------------------------------------------
def test_fp32_restatements_of_both_dfl_orders_stay_under_the_bound():
    worst = {"div": (0.0, ""), "inv": (0.0, "")}
    for name, dt in ALL:
        bt = hc.build(name, dt)
        d, bd = hc.dfl64(name, dt)[0], hc.bound_d(name, dt)
        for order in ("div", "inv"):
            got = hc.dfl_restated(bt.bins, bt.dfl_w, order).astype(np.float64)
            ok = ~np.isnan(d)
            assert np.array_equal(np.isnan(got), ~ok), (name, dt, order)
            frac = float((np.abs(got - d)[ok] / bd[ok]).max())
            assert frac <= 1.0, (name, dt, order, frac)
            if frac > worst[order][0]:
                worst[order] = (frac, f"{name} {dt}")
    for order, (frac, where) in worst.items():
        print(f"fp32 restatement '{order}': largest |d - d64| / bound_d {frac:.3f} ({where})")
    # the bound is of the size the arithmetic asks for - within an order of magnitude of what a restatement reaches, not a blanket
    assert min(f for f, _ in worst.values()) > 0.02


def test_the_bound_tells_the_dfl_weights_from_their_index():
    """a kernel that took the bin's index for its weight lies outside the bound on every seeded case (but the one with arange weights)"""
    for c in hc.CASES:
        if c.family != "seeded":
            continue
        for dt in hc.DTYPES:
            bt, kept = hc.build(c.name, dt), hc.kept_cells(c.name, dt)
            wrong = hc.dfl_restated(bt.bins, np.arange(16, dtype=np.float32), "div").astype(np.float64)
            d, bd = hc.dfl64(c.name, dt)[0], hc.bound_d(c.name, dt)
            for b in range(c.B):
                off = np.abs(wrong - d)[b, kept[b]] > bd[b, kept[b]]
                assert off.any() == (c.dfl != "arange"), (c.name, dt, b)


# ---- host code of the C ABI that needs no device ------------------------------------------------------------------------------------------------------
def test_workspace_of_a_bad_geometry_is_zero():
    """the size functions divide by the strides too: a null table or a stride below 1 gives 0, not a host division by zero"""
    from tensorrtx_amd import capi
    L = capi.lib()
    for fn in (L.trtx_yolo_head_decode_workspace, L.trtx_yolo_decode_workspace):
        fn.restype = ctypes.c_size_t
        st = (ctypes.c_int * 3)(8, 0, 32)
        assert fn(2, 64, 96, st, 3) == 0 and fn(2, 64, 96, None, 3) == 0 and fn(2, 0, 96, (ctypes.c_int * 3)(8, 16, 32), 3) == 0
        assert fn(2, 64, 96, (ctypes.c_int * 3)(8, 16, 32), 3) > 0
