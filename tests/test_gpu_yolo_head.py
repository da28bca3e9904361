"""The fused YOLOv8 / YOLO11 det and task heads alone (plugins/yolo_decode.hip: head_score<T, TAIL>, yolo_emit_kernel, yolo_task_emit_kernel)
through trtx_yolo_head_decode_nhwc{,_f32} and trtx_yolo_task_head_decode_nhwc{,_f32}, on the table of tests/yolo_head_cases.py: small ragged
nets, every family of edge (seeded, empty / full / overflow, the gate and the pre-filter in front of it, class ties, NaN and inf, extreme
DFL bins, the task branches), fp16 and fp32 storage, padded and exact strides, against the C oracle fed with a float64 DFL of the case's
own weights.  Counts, slot order, class ids, seg coefficients and the keypoints' -1 pattern must be equal, the confidence within 2e-7, every
box float under the per-element bound derived in the case module (printed as max err / bound per case), and no record is left out.

Every call writes into an `out` of one row more than the batch, filled with a sentinel: the row behind the batch, the floats behind a
row's last record and the floats of a record the head does not own must still hold it.  Refused calls must leave `out` and the workspace
bit for bit; the tensors they are handed are views into allocations large enough for any stride the call names, so no case depends on
the refusal to stay inside the test's own memory.  Every launch runs under tests.util.time_limit."""
import numpy as np
import pytest
import torch

from tensorrtx_amd import capi
from tests import yolo_head_cases as hc
from tests.util import SENTINEL, sync, time_limit

pytestmark = pytest.mark.gpu
DET = hc.DET
ALL = [(c.name, dt) for c in hc.CASES for dt in hc.DTYPES]
PLANAR_NETS = ("64x96", "160x160")   # the seeded cases of these nets also run the planar plugin kernel


def _ids(v):
    return v if isinstance(v, str) else None


def decode(case, dtype, gpu, heads, branches, head=None, max_out=None, batch=None, rows=None, ws=None, dfl=None):
    """one call of the det or the task head into a sentinel-filled `out` of batch + 1 rows -> the whole of `out` on the host"""
    H, W, strides = case.net
    mo = case.mo if max_out is None else max_out
    B = case.B if batch is None else batch
    out = torch.full(((B + 1) if rows is None else rows, 1 + mo * DET), SENTINEL, dtype=torch.float32, device=gpu)
    w = torch.from_numpy(hc.build(case.name, dtype).dfl_w if dfl is None else dfl).to(gpu)
    with time_limit():
        if (head or case.head) == "det":
            capi.yolo_head_decode_nhwc(heads, case.classes, H, W, list(strides), w, mo, out=out, batch=B, ws=ws)
        else:
            capi.yolo_task_head_decode_nhwc(heads, branches, case.classes, H, W, list(strides), w, mo, nk=case.nk, kpt_conf=case.kpt_conf,
                                            out=out, batch=B, ws=ws, **case.flags)
        sync(f"{case.name} {dtype}")
    return out.cpu().numpy()


def on_gpu(name, dtype, gpu, layout=("pad", "pad")):
    heads, branches = hc.tensors(name, dtype, layout)
    return [h.to(gpu) for h in heads], None if branches is None else [b.to(gpu) for b in branches]


def untouched(case, got, B, own):
    """the row behind the batch, the floats behind each row's last record, and what the head does not own of every record"""
    assert (got[B:] == SENTINEL).all(), "a row behind the batch was written"
    for b in range(B):
        n = int(got[b, 0])
        assert (got[b, 1 + n * DET:] == SENTINEL).all(), f"image {b}: floats behind the last record were written"
        assert (hc.records(got, b)[:, ~own] == SENTINEL).all(), f"image {b}: floats of a record the head does not own were written"


def compare(case, dtype, got, ref, own, what):
    """-> the largest |box - oracle| / bound over the case's records; everything else is asserted"""
    B, worst = ref.shape[0], 0.0
    assert np.array_equal(got[:B, 0], ref[:, 0]), (what, got[:B, 0], ref[:, 0])
    kept = hc.kept_cells(case.name, dtype)
    for b in range(B):
        G, R = hc.records(got, b), hc.records(ref, b)
        assert np.array_equal(G[:, 5], R[:, 5]), f"{what}: class ids / slot order, image {b}"
        assert (np.abs(G[:, 4] - R[:, 4]) <= hc.CONF_ATOL).all(), (what, b, np.abs(G[:, 4] - R[:, 4]).max())
        assert np.array_equal(np.isnan(G[:, :4]), np.isnan(R[:, :4])), f"{what}: NaN pattern of the boxes, image {b}"
        if len(G):
            bound = hc.box_bound(case.name, dtype, b, kept[b][:len(G)], R)
            ok = ~np.isnan(R[:, :4])
            frac = np.abs(G[:, :4].astype(np.float64) - R[:, :4])[ok] / bound[ok]
            if frac.size:
                worst = max(worst, float(frac.max()))
        if case.task == "seg" and own[6]:
            assert np.array_equal(G[:, 6:38], R[:, 6:38]), f"{what}: mask coefficients are copies"
        if case.task == "pose" and own[38]:
            gk, rk = G[:, 38:38 + 3 * case.nk], R[:, 38:38 + 3 * case.nk]
            assert np.array_equal(gk == -1, rk == -1), f"{what}: which keypoints are suppressed, image {b}"
            assert np.allclose(gk, rk, rtol=1e-6, atol=1e-4), what
        if case.task == "obb" and own[DET - 1]:
            assert np.allclose(G[:, DET - 1], R[:, DET - 1], rtol=1e-6, atol=1e-7, equal_nan=True), what
    return worst


@pytest.mark.parametrize("name,dt", ALL, ids=_ids)
def test_head_matches_oracle(gpu, name, dt):
    case, bt, ref = hc.BY_NAME[name], hc.build(name, dt), hc.reference(name, dt)
    own = hc.owned(case)
    first = None
    for layout in case.layouts:
        hs, bs = on_gpu(name, dt, gpu, layout)
        if case.task:
            assert (bs[0].shape[-1] % 2 == 1) == (layout[1] == "odd")
        got = decode(case, dt, gpu, hs, bs)
        untouched(case, got, case.B, own)
        worst = compare(case, dt, got, ref, own, f"{name} {dt} {layout}")
        print(f"{name} {dt} ld {hs[0].shape[-1]}{'/' + str(bs[0].shape[-1]) if bs else ''}: records {ref[:, 0].astype(int).tolist()} of {case.cells}, "
              f"max err / bound {worst:.3f}")
        assert worst <= 1.0, (name, dt, layout, worst)
        if first is None:
            first, first_hs = got, hs
        else:
            assert np.array_equal(got, first, equal_nan=True), f"{layout}: the strides of the tensors change the result"
    hs = first_hs
    if case.family == "overflow":
        # the clamped rows are the first max_out records of the canonical order: the same call with room for every cell
        full = decode(case, dt, gpu, *on_gpu(name, dt, gpu), max_out=case.cells + 1)
        assert full[2, 0] == case.cells and first[2, 0] == case.mo and first[1, 0] == 0
        for b in range(case.B):
            assert np.array_equal(hc.records(full, b)[:case.mo], hc.records(first, b), equal_nan=True)
    if case.head == "task" and case.classes % 8 == 0:
        # the det head on the same head tensors: the same candidates, and box / conf / class to the bit (obb replaces the box)
        det = decode(case, dt, gpu, hs, None, head="det")
        untouched(case, det, case.B, np.arange(DET) < 6)
        assert np.array_equal(det[:, 0], first[:, 0])
        cols = slice(4, 6) if case.task == "obb" else slice(0, 6)
        for b in range(case.B):
            assert np.array_equal(hc.records(det, b)[:, cols], hc.records(first, b)[:, cols], equal_nan=True), "det head against task head"
    if case.family == "seeded" and case.geom in PLANAR_NETS:
        # the planar plugin kernel on the oracle's inputs: count, conf and class to the bit
        H, W, strides = case.net
        ins = [torch.from_numpy(x).to(gpu) for x in hc.planar(name, dt)]
        with time_limit():
            if case.task:
                plug = capi.yolo_decode_ex(ins, case.classes, H, W, list(strides), case.mo, nk=case.nk, kpt_conf=case.kpt_conf, **case.flags)
            else:
                plug = capi.yolo_decode(ins, case.classes, H, W, list(strides), case.mo)
            sync(f"{name} planar")
        plug = plug.cpu().numpy()
        assert np.array_equal(plug[:, 0], first[:case.B, 0])
        for b in range(case.B):
            assert np.array_equal(hc.records(plug, b)[:, 4:6], hc.records(first, b)[:, 4:6]), "fused head against the planar plugin kernel"
    if case.family == "threshold":
        # said once more without the oracle: of the cells placed at the gate, exactly those the table marks as kept have a record
        kept = hc.kept_cells(name, dt)
        for (b, g), (v, _, keep) in bt.expect["gate"].items():
            assert (g in kept[b]) == keep
        assert np.array_equal(first[:case.B, 0], [len(k) for k in kept])


@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("name", ["det_64x96_full_nc8" if "det_64x96_full_nc8" in hc.BY_NAME else "det_64x96_full_nc80",
                                  next(c.name for c in hc.CASES if c.head == "task" and c.family == "full" and c.geom == "160x160")])
def test_batch_below_the_tensors_leading_dimension(gpu, name, dt):
    """three images in the tensors, batch 2 in the call, a workspace sized for three: rows 2 and 3 of `out` keep the sentinel, rows 0 and 1
    are the three-image call's"""
    case = hc.BY_NAME[name]
    assert case.B == 3
    hs, bs = on_gpu(name, dt, gpu)
    H, W, strides = case.net
    allb = decode(case, dt, gpu, hs, bs)
    ws = torch.full((capi.yolo_head_decode_workspace(3, H, W, list(strides)),), 0x5A, dtype=torch.uint8, device=gpu)
    part = decode(case, dt, gpu, hs, bs, batch=2, rows=4, ws=ws)
    untouched(case, part, 2, hc.owned(case))
    assert np.array_equal(part[:2], allb[:2], equal_nan=True)


@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("name", ["det_160x160_seeded_nc80", "seg_160x160_seeded_nc80", "pose_64x96_seeded_nc1_nk17"])
def test_head_is_batch_invariant(gpu, name, dt):
    """image 0 of a batch decodes bit-equal when run alone"""
    case = hc.BY_NAME[name]
    hs, bs = on_gpu(name, dt, gpu)
    allb = decode(case, dt, gpu, hs, bs)
    alone = decode(case, dt, gpu, [h[:1].contiguous() for h in hs], None if bs is None else [b[:1].contiguous() for b in bs], batch=1)
    assert allb[0, 0] >= 3 and np.array_equal(alone[0], allb[0], equal_nan=True)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def _roomy(name, dt, gpu):
    """the case's tensors with strides of three vectors more than the padded ones and one image more than the batch: whatever stride, base
    offset or batch a refusal case names (all of them at most these), the addresses it spans lie inside the allocations"""
    case, bt = hc.BY_NAME[name], hc.build(name, dt)
    off, vec = hc.level_offsets(case.geom), hc.VEC[dt]
    x = np.concatenate([bt.bins.reshape(case.B, case.cells, 64), bt.logits], -1)
    x = np.concatenate([x, x[:1]], 0)
    heads = [hc.nhwc(x[:, off[i]:off[i + 1]], hc.head_ld(case, dt, "pad") + 3 * vec, dt).to(gpu) for i in range(len(off) - 1)]
    branches = None
    if case.task:
        br = np.concatenate([bt.branch, bt.branch[:1]], 0)
        branches = [hc.nhwc(br[:, off[i]:off[i + 1]], hc.branch_ld(case, dt, "pad") + 3 * vec, dt).to(gpu) for i in range(len(off) - 1)]
    return heads, branches


def _refusals(gpu, name, dt, cases, call):
    case = hc.BY_NAME[name]
    H, W, strides = case.net
    mo = 50
    ws_bytes = capi.yolo_head_decode_workspace(case.B, H, W, list(strides))
    dfl = torch.from_numpy(hc.build(name, dt).dfl_w).to(gpu)
    for what, status, kw in cases:
        kw = dict(kw)
        out = torch.full((case.B + 1, 1 + mo * DET), SENTINEL, dtype=torch.float32, device=gpu)
        ws = torch.full((ws_bytes - kw.pop("ws_short", 0),), 0x5A, dtype=torch.uint8, device=gpu)
        args = dict(classes=case.classes, net_h=H, net_w=W, strides=list(strides), dfl_w=dfl, max_out=mo, batch=case.B)
        args.update(kw)
        with time_limit():
            st = call(out=out, ws=ws, status_only=True, **args)
            sync(f"refusal: {what}")
        assert st == status, (what, st, status)
        assert (out == SENTINEL).all() and (ws == 0x5A).all(), f"{what}: a refused call wrote"
    return dfl, mo


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_det_head_refusals_leave_the_buffers_untouched(gpu, dt):
    name = "det_64x96_seeded_nc80"
    case = hc.BY_NAME[name]
    hs, _ = _roomy(name, dt, gpu)
    vec, ld, n = hc.VEC[dt], hs[0].shape[-1], len(hs)
    H, W, strides = case.net
    need = 64 + case.classes
    assert ld - 2 * vec >= need and need - vec > 0
    # a base one element off: the same allocation from its second element on, with a stride one vector shorter (still legal, still inside)
    off_base = [hs[0].flatten()[1:1 + hs[0].shape[0] * hs[0].shape[1] * (ld - vec)].view(hs[0].shape[0], hs[0].shape[1], ld - vec)] + hs[1:]

    def call(heads=hs, **kw):
        return capi.yolo_head_decode_nhwc(heads, kw.pop("classes"), kw.pop("net_h"), kw.pop("net_w"), kw.pop("strides"), kw.pop("dfl_w"),
                                          kw.pop("max_out"), **kw)

    dfl, mo = _refusals(gpu, name, dt, [
        ("ld no 16-byte multiple", 4, dict(ld=[ld - 1] * n)),
        ("ld no 16-byte multiple on the last level only", 4, dict(ld=[ld] * (n - 1) + [ld - vec // 2])),
        ("base off by one element", 4, dict(heads=off_base, ld=[ld - vec] + [ld] * (n - 1))),
        ("ld < 64 + classes", 4, dict(ld=[need - vec] * n)),
        ("ld < 64 + classes on one level", 4, dict(ld=[ld, need - vec] + [ld] * (n - 2))),
        ("classes 12", 1, dict(classes=12)),
        ("classes 0", 1, dict(classes=0)),
        ("n_levels 0", 1, dict(n_levels=0)),
        ("n_levels 9", 1, dict(n_levels=9)),
        ("batch 0", 1, dict(batch=0)),
        ("max_out 0", 1, dict(max_out=0)),
        ("null dfl_weights", 1, dict(dfl_w=None)),
        ("workspace 256 bytes short", 3, dict(ws_short=256)),
        ("null strides", 1, dict(strides=None)),
        ("a stride of 0", 1, dict(strides=[strides[0], 0, strides[2]])),
        ("a negative stride", 1, dict(strides=[strides[0], strides[1], -strides[2]])),
        ("net_h 0", 1, dict(net_h=0)),
        ("net_w -8", 1, dict(net_w=-8)),
    ], call)
    # and the same tensors with their true strides decode, and equal the table's own tensors' result
    with time_limit():
        out = capi.yolo_head_decode_nhwc(hs, case.classes, H, W, list(strides), dfl, mo, batch=case.B)
        sync("after the refusals")
    want = decode(case, dt, gpu, *on_gpu(name, dt, gpu), max_out=mo)
    assert want[0, 0] >= 3 and np.array_equal(out.cpu().numpy()[:, :1], want[:case.B, :1])
    for b in range(case.B):
        assert np.array_equal(hc.records(out.cpu().numpy(), b)[:, :6], hc.records(want, b)[:, :6])


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_task_head_refusals_leave_the_buffers_untouched(gpu, dt):
    name = "pose_64x96_seeded_nc8_nk5"
    case = hc.BY_NAME[name]
    hs, bs = _roomy(name, dt, gpu)
    vec, ld, bld, n = hc.VEC[dt], hs[0].shape[-1], bs[0].shape[-1], len(hs)
    H, W, strides = case.net
    need = 64 + case.classes

    def call(**kw):
        a = [kw.pop(k) for k in ("classes", "net_h", "net_w", "strides", "dfl_w", "max_out")]
        flags = kw.pop("flags", dict(pose=True))
        return capi.yolo_task_head_decode_nhwc(hs, bs, *a, nk=kw.pop("nk", case.nk), kpt_conf=case.kpt_conf, **flags, **kw)

    dfl, mo = _refusals(gpu, name, dt, [
        ("ld < 64 + classes", 4, dict(ld=[need - vec] * n)),
        ("ld no 16-byte multiple", 4, dict(ld=[ld - 1] * n)),
        ("branch_ld < extra", 1, dict(branch_ld=[bld, case.extra - 1, bld])),
        ("no task flag", 1, dict(flags={})),
        ("two task flags", 1, dict(flags=dict(pose=True, seg=True))),
        ("pose with nk 0", 1, dict(nk=0)),
        ("pose with nk 18", 1, dict(nk=18)),
        ("workspace 256 bytes short", 3, dict(ws_short=256)),
        ("null strides", 1, dict(strides=None)),
        ("a stride of 0", 1, dict(strides=[0, strides[1], strides[2]])),
        ("net_w 0", 1, dict(net_w=0)),
    ], call)
    with time_limit():
        out = capi.yolo_task_head_decode_nhwc(hs, bs, case.classes, H, W, list(strides), dfl, mo, nk=case.nk, kpt_conf=case.kpt_conf, batch=case.B,
                                              pose=True)
        sync("after the refusals")
    want = decode(case, dt, gpu, *on_gpu(name, dt, gpu), max_out=mo)
    own = hc.owned(case)
    assert want[0, 0] >= 3 and np.array_equal(out.cpu().numpy()[:, :1], want[:case.B, :1])
    for b in range(case.B):
        assert np.array_equal(hc.records(out.cpu().numpy(), b)[:, own], hc.records(want, b)[:, own])
