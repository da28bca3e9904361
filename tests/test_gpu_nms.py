"""plugins/yolo_nms.hip through its C entry points on the NMS table (tests/nms_cases.py): one test per (entry point, family), every call into
buffers the test filled beforehand - the workspace with 0xFF, keep_idx with -1, keep_det with NaN, keep_cnt with a sentinel, each with a guard
row (the workspace: guard bytes) behind it.

Asserted, bit for bit against the project's sequential C oracle: keep_cnt, keep_idx[:cnt], keep_det[:cnt] (MODE 3: the converted centre boxes,
MODE 2: 7 floats with the angle) of every image of the batch; everything behind cnt and every guard still holds what the test wrote; the g
modes' whole output buffer [B, 1 + max_out * 7 | 8].  A refused call (max_out = 1025) returns TRTX_ERR_UNSUPPORTED and writes nothing.  Where
oracle/_ref/libref_host.so exists, the tie-free cases whose header the reference's own host functions can read (count <= max_out, <= 1000)
are compared with those as well."""
import ctypes

import numpy as np
import pytest
import torch

import nms_cases as nc
import util
from oracle import ref
from tensorrtx_amd import capi

pytestmark = pytest.mark.gpu
CNT_SENTINEL = -77
NAN_BITS = np.float32(np.nan).view(np.int32)
GUARD_BYTES = 4096


def workspace(batch, gpu):
    L = capi.lib()
    L.trtx_yolo_nms_workspace.restype = ctypes.c_size_t
    need = int(L.trtx_yolo_nms_workspace(batch))
    return torch.full((need + GUARD_BYTES,), 0xFF, dtype=torch.uint8, device=gpu), need


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def call(ep, case, gpu, ws_buf, ws_need):
    """one call of the table into pre-filled outputs -> the outputs on the host, guard rows included"""
    e = nc.ENTRIES[ep]
    buf = case.buffer(ep)
    B, mo = buf.shape[0], case.max_out
    d = torch.from_numpy(buf).to(gpu)
    fn = getattr(capi, e["fn"])
    if e["greedy"]:
        out = (torch.full((B + 1, mo), -1, dtype=torch.int32, device=gpu), torch.full((B + 1,), CNT_SENTINEL, dtype=torch.int32, device=gpu),
               torch.full((B + 1, mo, e["det_out"]), float("nan"), dtype=torch.float32, device=gpu))
        kw = dict(out=out, ws=ws_buf[:ws_need])
    else:
        out = torch.full((B + 1, 1 + mo * e["det_out"]), float("nan"), dtype=torch.float32, device=gpu)
        kw = dict(out=out)
    status = 0
    with util.time_limit():
        try:
            fn(d, mo, case.conf, case.nms, **kw)
        except capi.TrtxError as err:
            status = err.status
        util.sync(f"{e['fn']} on {case.name}")
    assert status == case.expect_status, (case.name, status)
    assert (ws_buf[ws_need:] == 0xFF).all(), "the bytes behind the workspace were written"
    assert np.array_equal(bits(d.cpu().numpy()), bits(buf)), "the decode buffer was written"
    return buf, ([t.cpu().numpy() for t in out] if e["greedy"] else out.cpu().numpy())


def check_greedy(ep, case, buf, got):
    B, mo = buf.shape[0], case.max_out
    gi, gc, gd = got
    assert gc[B] == CNT_SENTINEL and (gi[B] == -1).all() and (bits(gd[B]) == NAN_BITS).all(), "the rows behind the batch were written"
    if case.expect_status:
        assert (gc == CNT_SENTINEL).all() and (gi == -1).all() and (bits(gd) == NAN_BITS).all(), "a refused call wrote its outputs"
        return
    ri, rc, rd = nc.oracle(ep, buf, mo, case.conf, case.nms)
    print(f"{ep} {case.name}: header {buf[:, 0].astype(int).tolist()} max_out {mo} -> kept {gc[:B].tolist()} (oracle {rc.tolist()})")
    for b in range(B):
        n = int(rc[b])
        assert gc[b] == n, (case.name, b, int(gc[b]), n)
        assert np.array_equal(gi[b, :n], ri[b, :n]), (case.name, b, np.flatnonzero(gi[b, :n] != ri[b, :n])[:8])
        assert np.array_equal(bits(gd[b, :n]), bits(rd[b, :n])), (case.name, b)
        assert (gi[b, n:] == -1).all() and (bits(gd[b, n:]) == NAN_BITS).all(), (case.name, b, "written behind keep_cnt")
    reference = {"nms": ref.yolov8_nms, "v5": ref.yolov5_nms, "obb": ref.yolov8_nms_obb}.get(ep)
    if reference is not None and case.tie_free and ref.available("libref_host.so"):
        for b in range(B):
            if buf[b, 0] <= min(mo, 1000) and not np.isnan(buf[b, 1:].reshape(mo, -1)[:int(buf[b, 0]), 4]).any():
                want = reference(buf[b], case.conf, case.nms)
                assert len(want) == gc[b] and np.array_equal(bits(gd[b, :gc[b], :6]), bits(want[:, :6])), (case.name, b, "the reference's host function")


def check_g(ep, case, buf, got):
    B, mo = buf.shape[0], case.max_out
    assert (bits(got[B]) == NAN_BITS).all(), "the row behind the batch was written"
    if case.expect_status:
        assert (bits(got) == NAN_BITS).all(), "a refused call wrote its output"
        return
    want = nc.oracle(ep, buf, mo, case.conf, case.nms)
    w = nc.ENTRIES[ep]["det_out"]
    print(f"{ep} {case.name}: header {buf[:, 0].astype(int).tolist()} max_out {mo} -> keep flags {[int(got[b, 1:].reshape(mo, w)[:, 6].sum()) for b in range(B)]}")
    for b in range(B):
        diff = np.flatnonzero(bits(got[b]) != bits(want[b]))
        assert len(diff) == 0, (case.name, b, diff[:8], got[b, diff[:8]], want[b, diff[:8]])


@pytest.mark.parametrize("ep,family", nc.COMBOS, ids=[f"{ep}-{fam}" for ep, fam in nc.COMBOS])
def test_nms_table(gpu, ep, family):
    cases = nc.cases(ep, family)
    ws_buf = None
    for case in cases:
        if ws_buf is None or not case.same_ws:
            ws_buf, ws_need = workspace(max(len(c.images) for c in cases), gpu)   # fresh: every byte 0xFF
        buf, got = call(ep, case, gpu, ws_buf, ws_need)
        (check_greedy if nc.ENTRIES[ep]["greedy"] else check_g)(ep, case, buf, got)
