"""The NMS table (tests/nms_cases.py) without a GPU: every case reaches the edge its family names - survivor counts, class boundaries and ranks
computed from the oracle's sort order - the oracle gives the analytic result where there is one, the C oracle equals the independent
oracle.yolo_post.nms_py on the small MODE 0 cases, the family 7 pairs sit at the threshold and flip under every emulated contraction, and no
oriented case has a pair within OBB_MARGIN of its threshold."""
import numpy as np
import pytest

import nms_cases as nc
from oracle import yolo_post as yp

F = np.float32


def ranks_of(ep, case, b=0):
    """slot -> rank in the oracle's sort order, and the sorted classes, of image b"""
    buf = case.buffer(ep)
    order = nc.sort_order(ep, buf, case.max_out, case.conf)[b]
    cls = buf[b, 1:].reshape(case.max_out, nc.ENTRIES[ep]["det"])[order, 5]
    return {int(s): r for r, s in enumerate(order)}, cls


def survivors(ep, case):
    return [len(o) for o in nc.sort_order(ep, case.buffer(ep), case.max_out, case.conf)]


def test_every_combination_has_cases_and_every_family_its_entry_points():
    assert set(nc.FAMILIES["counts"]) == set(nc.ENTRIES) and set(nc.FAMILIES["capacity"]) == set(nc.ENTRIES)
    for fam in ("class_block", "chains", "chains_1024", "ties", "gates", "iou_threshold"):
        assert set(nc.AABB) <= set(nc.FAMILIES[fam]), fam
    assert {"obb", "g", "gobb"} <= set(nc.FAMILIES["chains"]) and "obb" in nc.FAMILIES["ties"] and "g" in nc.FAMILIES["iou_threshold"]
    assert "obb" not in nc.FAMILIES["iou_threshold"] and "gobb" not in nc.FAMILIES["iou_threshold"]
    for ep, fam in nc.COMBOS:
        assert len(nc.cases(ep, fam)) >= 1, (ep, fam)


@pytest.mark.parametrize("ep", list(nc.ENTRIES))
def test_counts_are_survivor_counts_and_slots_are_not_ranks(ep):
    cs = nc.cases(ep, "counts")
    assert [survivors(ep, c)[0] for c in cs] == list(nc.COUNTS)
    assert [c.max_out for c in cs] == [1000] * 10 + [1024] * 2
    for c, n in zip(cs, nc.COUNTS):
        buf = c.buffer(ep)
        rec = buf[0, 1:].reshape(c.max_out, -1)
        assert buf[0, 0] == c.images[0].m <= c.max_out
        if 2 < n <= 1000 - n // 2:
            assert buf[0, 0] == n + (n - 1) // 2 and (rec[2:int(buf[0, 0]):3, 4] <= F(c.conf)).all()   # every third slot is dropped
        order = nc.sort_order(ep, buf, c.max_out)[0]
        if n >= 63:
            cls = rec[order, 5]
            assert (np.diff(cls) >= 0).all() and set(cls) == set(nc.CLASSES)                         # the sort reversed the classes
            slots_cls = rec[:int(buf[0, 0]), 5]
            assert (np.diff(slots_cls) <= 0).all()
            assert (order != np.arange(n)).any()
            kept = nc.kept_slots(ep, buf, c.max_out, c.conf, c.nms)[0]
            assert 0 < len(kept) < n, "some records are suppressed, not all"


@pytest.mark.parametrize("ep", list(nc.ENTRIES))
def test_capacity_headers_exceed_full_buffers(ep):
    cs = nc.cases(ep, "capacity")
    assert [c.max_out for c in cs] == list(nc.CAPACITIES)
    for c in cs:
        buf = c.buffer(ep)
        assert buf.shape == (2, 1 + c.max_out * nc.ENTRIES[ep]["det"])
        assert buf[:, 0].tolist() == [c.max_out + 7, 5000] and all(im.m == c.max_out for im in c.images)
        assert survivors(ep, c) == [c.max_out - c.max_out // 3] * 2
    (r,) = nc.cases(ep, "refusal")
    assert r.max_out == 1025 and r.expect_status == nc.UNSUPPORTED


@pytest.mark.parametrize("ep", nc.FAMILIES["class_block"])
def test_class_boundaries_sit_on_block_boundaries(ep):
    five, one = nc.cases(ep, "class_block")
    rank, cls = ranks_of(ep, five)
    assert len(cls) == 342
    for c, (first, members) in nc.CLASS_BLOCK.items():
        assert (cls[first:first + members] == c).all() and (cls == c).sum() == members
    for lo, hi in ((63, 64), (64, 65), (127, 128)):
        assert cls[lo] != cls[hi]
    assert cls[128] == cls[191] == 17 and cls[127] < 17 < cls[192]            # one class is block 2: both neighbouring tiles are skipped
    assert cls[64 + 63] < cls[128] and cls[128 + 63] < cls[192]                  # the skip rule itself, tiles (1, 2) and (2, 3)
    assert cls[192] == cls[341] == 79 and 192 // 64 == 3 and 341 // 64 == 5      # one class over three blocks
    buf = five.buffer(ep)
    order = nc.sort_order(ep, buf, five.max_out)[0]
    kept = nc.kept_slots(ep, buf, five.max_out, five.conf, five.nms)[0]
    dead79 = [r for r in range(192, 342) if int(order[r]) not in kept]
    assert dead79 == list(range(320, 342, 2)), "the victims sit in the third block, their suppressors (ranks 192 .. 213) in the first"
    assert survivors(ep, one) == [1024] and len(set(ranks_of(ep, one)[1])) == 1


@pytest.mark.parametrize("ep", nc.FAMILIES["chains"])
def test_chains_have_their_ranks_and_their_analytic_result(ep):
    greedy = nc.ENTRIES[ep]["greedy"]
    cs = {c.name: c for c in nc.cases(ep, "chains")}
    want_ranks = dict(a_in_block=dict(A=0, B=1, C=2), b_three_blocks=dict(A=0, B=71, C=136), c_dead_suppressor=dict(A=0, B=1, D=72))
    for name, want in want_ranks.items():
        c = cs[name]
        rank, cls = ranks_of(ep, c)
        marks = c.images[0].marks
        assert len(set(cls)) == 1
        assert {k: rank[marks[k]] for k in want} == want, name
        kept = nc.kept_slots(ep, c.buffer(ep), c.max_out, c.conf, c.nms)[0]
        last = "D" if "D" in want else "C"
        assert marks["A"] in kept and marks["B"] not in kept
        assert (marks[last] in kept) == greedy, "greedy keeps the box whose only suppressor is dead, the g modes drop it"
        assert len(kept) == len(cls) - (1 if greedy else 2)
    c = cs["d_chain_of_200"]
    rank, cls = ranks_of(ep, c)
    marks = c.images[0].marks
    assert [rank[marks[f"L{i}"]] for i in range(200)] == list(range(200))
    assert [marks[f"L{i}"] for i in range(200)] != sorted(marks.values()), "the slots are scrambled"
    kept = nc.kept_slots(ep, c.buffer(ep), c.max_out, c.conf, c.nms)[0]
    if greedy:
        assert kept == {marks[f"L{i}"] for i in range(0, 200, 2)}, "exactly the even ranks, across three block boundaries"
    else:
        assert kept == {marks["L0"]}


def test_chain_geometry():
    a, b, c = (np.array(nc.chain_box(i, False)[0], dtype=F)[None] for i in range(3))
    v = nc.fma_variants("xyxy", a, b)["plain"][0], nc.fma_variants("xyxy", a, c)["plain"][0]
    assert v[0] == F(F(7000) / F(13000)) > nc.IOU > v[1] == F(F(4000) / F(16000))
    s = nc.obb_chain_step()
    p = [nc.probiou64([0, 0, nc.OBB_W, nc.OBB_H, nc.OBB_ANG], [k * s, 0, nc.OBB_W, nc.OBB_H, nc.OBB_ANG]) for k in (1, 2, 3)]
    assert abs(p[0] - 0.6) < 0.01 and p[1] < nc.IOU - 0.1 and p[2] < p[1]


@pytest.mark.parametrize("ep", nc.FAMILIES["chains_1024"])
def test_1024_identical_and_1024_disjoint(ep):
    same, apart = nc.cases(ep, "chains_1024")
    assert same.max_out == apart.max_out == 1024 and survivors(ep, same) == survivors(ep, apart) == [1024]
    idx, cnt, det = nc.oracle(ep, same.buffer(ep), 1024, same.conf, same.nms)
    assert cnt[0] == 1 and det[0, 0, 4] == same.images[0].conf.max()
    idx, cnt, det = nc.oracle(ep, apart.buffer(ep), 1024, apart.conf, apart.nms)
    assert cnt[0] == 1024 and (np.diff(det[0, :, 4]) < 0).all() and sorted(idx[0].tolist()) == list(range(1024))


@pytest.mark.parametrize("ep", nc.FAMILIES["ties"])
def test_ties_are_ties_and_the_canonical_order_is_what_the_family_says(ep):
    (c,) = nc.cases(ep, "ties")
    assert not c.tie_free
    buf = c.buffer(ep)
    det = nc.ENTRIES[ep]["det"]
    orders = nc.sort_order(ep, buf, c.max_out)
    for b, order in enumerate(orders):
        rec = buf[b, 1:].reshape(c.max_out, det)[order]
        tied = rec[rec[:, 5] == 3]
        slots = order[rec[:, 5] == 3]
        assert len(tied) >= nc.TIED >= 50 and len(set(tied[:, 4])) == 1
        kept = nc.kept_slots(ep, buf, c.max_out, c.conf, c.nms)[b]
        assert len(tied) // 3 < len(kept & set(slots.tolist())) < len(tied), "the chain makes the order decide who survives"
        if nc.b0_decides(ep) and b == 0:
            assert (np.diff(tied[:, 0]) >= 0).all() and (tied[:, 0] < 0).sum() == 20
            m = c.images[0].marks
            zeros = [int(s) for s in slots if tied[list(slots).index(s), 0] == 0]
            assert zeros == [m["zero_a"], m["zero_minus"], m["zero_b"]] == sorted(zeros), "+0.0, -0.0, +0.0 tie: the slot decides"
            z = buf[0, 1:].reshape(c.max_out, det)[zeros, 0]
            assert np.signbit(z).tolist() == [False, True, False]
            assert (slots != np.sort(slots)).any(), "bbox[0], not the slot, orders the rest"
        elif nc.b0_decides(ep):
            assert len(set(tied[:, 0])) == 1 and (np.diff(slots) > 0).all(), "full ties: the slot decides"
        else:
            assert (np.diff(slots) > 0).all() and (np.diff(tied[:, 0]) < 0).all(), "bbox[0] descends along the slots; the slot alone decides"


@pytest.mark.parametrize("ep", nc.FAMILIES["gates"])
def test_gates(ep):
    (c,) = nc.cases(ep, "gates")
    buf = c.buffer(ep)
    m = c.images[0].marks
    rec = buf[0, 1:].reshape(c.max_out, -1)
    assert rec[m["at_gate"], 4] == F(c.conf) and rec[m["above_gate"], 4] == np.nextafter(F(c.conf), F(1))
    kept = nc.kept_slots(ep, buf, c.max_out, c.conf, c.nms)[0]
    assert m["at_gate"] not in kept and m["above_gate"] in kept and m["normal"] in kept and m["victim"] not in kept
    assert {m["zero_a"], m["zero_b"], m["point_a"], m["point_b"]} <= kept, "0 / 0 is not above a threshold"
    assert m["inv_a"] in kept
    assert ("nan" in m) == (ep == "nms")
    if ep == "nms":
        assert np.isnan(rec[m["nan"], 4]) and m["nan"] not in kept
    else:
        assert not np.isnan(rec[:int(buf[0, 0]), 4]).any()
    x1, x2 = (rec[m["inv_a"], 0], rec[m["inv_a"], 2]) if nc.ENTRIES[ep]["box"] == "corner" else (F(0), rec[m["inv_a"], 2])
    assert x2 < x1


def c_iou(kind, l, r):
    return nc.fma_variants(kind, l[None], r[None])


@pytest.mark.parametrize("kind", ["xyxy", "cxcywh"])
def test_iou_pairs_sit_at_the_threshold_and_flip_under_every_contraction(kind):
    pairs = nc.threshold_pairs(kind)
    assert len(pairs) >= 4 and len({p[2] for p in pairs}) == len(pairs) <= 4, "one call per threshold, eight calls at most over both functions"
    at_threshold = 0
    for l, r, thr, direction in pairs:
        assert F(thr) == thr, "the threshold is a float"
        a, b = (l, r) if kind == "xyxy" else (nc.to_centre(l), nc.to_centre(r))
        v = {k: x[0] for k, x in c_iou(kind, a, b).items()}
        plain = v.pop("plain")
        if direction == "up":
            assert plain == F(thr) and not plain > F(thr)
            at_threshold += 1
        for name, x in v.items():
            assert (x > F(thr)) != (plain > F(thr)), (name, direction, float(plain), float(x), thr)
        sw = c_iou(kind, b, a)   # the g kernel passes the less confident box first: the plain value is the same
        assert sw["plain"][0] == plain and all((sw[k][0] > F(thr)) != (plain > F(thr)) for k in v)
    assert at_threshold >= 2


@pytest.mark.parametrize("ep", nc.FAMILIES["iou_threshold"])
def test_iou_threshold_cases_decide_as_the_plain_fp32_evaluation(ep):
    cs = nc.cases(ep, "iou_threshold")
    assert len(cs) == 4
    for c, (l, r, thr, direction) in zip(cs, nc.threshold_pairs(nc.iou_kind(ep))):
        m = c.images[0].marks
        kept = nc.kept_slots(ep, c.buffer(ep), c.max_out, c.conf, c.nms)[0]
        assert c.nms == thr and m["first"] in kept
        assert (m["second"] in kept) == (direction == "up"), "at the threshold the box stays; above it, it goes"


def test_the_plain_variant_is_the_oracles_iou():
    """fma_variants' "plain" against the C oracle: a pair is suppressed exactly when plain > threshold, over random pairs and thresholds"""
    rng = np.random.default_rng(5)
    l = (rng.uniform(100, 300, (200, 4)) + np.array([0, 0, 100, 100])).astype(F)
    r = (l + rng.uniform(-20, 20, (200, 4))).astype(F)
    plain = nc.fma_variants("xyxy", l, r)["plain"]
    plain_c = nc.fma_variants("cxcywh", nc.to_centre(l), nc.to_centre(r))["plain"]
    for k in range(200):
        rr = nc.Recs()
        rr.add(l[k].astype(np.float64), 0.9, 3.0)
        rr.add(r[k].astype(np.float64), 0.8, 3.0)
        img = nc.place(rr, total=2)
        for ep, p in (("nms", plain), ("v9", plain_c), ("v5", plain_c)):
            for thr in (float(p[k]), float(np.nextafter(p[k], F(0)))):
                kept = nc.kept_slots(ep, nc.emit(ep, [img], 2), 2, 0.5, thr)[0]
                assert (1 in kept) == (not p[k] > F(thr)), (ep, k, thr)


def test_small_cases_equal_the_independent_python_nms():
    n_checked = 0
    for fam in nc.FAMILIES:
        if "nms" not in nc.FAMILIES[fam] or fam == "refusal":
            continue
        for c in nc.cases("nms", fam):
            buf = c.buffer("nms")
            idx, cnt, _ = nc.oracle("nms", buf, c.max_out, c.conf, c.nms)
            for b, im in enumerate(c.images):
                if min(int(buf[b, 0]), c.max_out) > 200:
                    continue
                assert yp.nms_py(buf[b], c.max_out, c.conf, c.nms) == idx[b, :cnt[b]].tolist(), (fam, c.name, b)
                n_checked += 1
    assert n_checked >= 20


def test_no_oriented_case_is_near_its_threshold():
    worst = np.inf
    for ep in ("obb", "gobb"):
        for fam, eps in nc.FAMILIES.items():
            if ep not in eps or fam == "refusal":
                continue
            for c in nc.cases(ep, fam):
                m = nc.obb_margin(ep, c)
                assert m >= nc.OBB_MARGIN, (ep, fam, c.name, m)
                worst = min(worst, m)
    print(f"smallest |ProbIoU - threshold| over the oriented cases: {worst:.3f}")
    assert np.isfinite(worst)


@pytest.mark.parametrize("ep", list(nc.ENTRIES))
def test_batch_and_workspace_calls(ep):
    first, second, third = nc.cases(ep, "batch_workspace")
    assert survivors(ep, first) == [1024, 0, 65] and first.max_out == 1024
    assert second.same_ws and third.same_ws and len(second.images) == 3 and len(third.images) == 1
    assert max(survivors(ep, second)) <= 65 and survivors(ep, third)[0] <= 80
    if not nc.is_obb(ep) and nc.ENTRIES[ep]["greedy"]:
        assert nc.oracle(ep, first.buffer(ep), 1024, first.conf, first.nms)[1].tolist()[:2] == [1, 0]   # image 0: every bit of the triangle is set
