"""The sibling pair (plan_passes.cpp mark_sibling_pair; the dual tile of kernels/igemm_tile.h) on the CPU: which plans carry the mark, that the mark is all that
changes in a plan, and that the arena keeps the six tensors the one launch writes apart from what it reads and from each other.  The kernel itself:
tests/test_gpu_sibling_pair.py.

The pair needs both groups on one stream, so it is looked at in the engine a throughput caller builds - setMaxAuxStreams(0), what bench.py's headline uses -;
an engine with auxiliary streams puts the two independent groups on different lanes, where they overlap, and is left as it is (the last test)."""
import struct

import pytest

from tensorrtx_amd import engine
from util import synth_wts


def _low(plan):
    return engine.describe_plan(plan, lowered=True)


def _marked(ops):
    return [k for k, o in enumerate(ops) if o.get("sibling_pair")]


def _members(op):
    return sorted((m["cout"], m["k"][0], m["in"][0], m["out"][0]) for m in op["members"])


def _window(low, t):
    """(storage, first channel, one past the last channel) of an NHWC tensor"""
    pt = low["tensors"][t]
    assert pt["layout"] == "nhwc"
    return pt["storage"], pt["coff"], pt["coff"] + pt["dims"][0]


def _order_is_topological(low):
    """every op that writes channels of a block another op reads (or writes) sits where the data flow wants it: a reader after the writer"""
    writers = {}
    for k, o in enumerate(low["ops"]):
        for t in o["out"]:
            if low["tensors"][t]["layout"] == "nhwc":
                writers.setdefault(low["tensors"][t]["storage"], []).append((k,) + _window(low, t)[1:])
    for k, o in enumerate(low["ops"]):
        for t in o["in"]:
            if low["tensors"][t]["layout"] != "nhwc":
                continue
            st, lo, hi = _window(low, t)
            for w, wlo, whi in writers.get(st, []):
                if w != k and wlo < hi and lo < whi and w > k:
                    return False
    return True


@pytest.fixture(scope="module")
def bench_plan():
    path, _ = synth_wts("yolov8n")
    return engine.build_plan("yolov8n", path, batch=32, h=640, w=640, fp16=1, aux_streams=0)


def test_benchmark_plan_has_one_marked_group_right_behind_its_sibling(bench_plan, monkeypatch):
    on = _low(bench_plan)
    ops = on["ops"]
    m = _marked(ops)
    assert len(m) == 1
    k = m[0]
    first, second = ops[k - 1], ops[k]
    assert first["kind"] == second["kind"] == "conv_group" and first["lane"] == second["lane"]
    assert sorted((c, f) for c, f, _, _ in _members(second)) == [(80, 3)] * 3 and sorted((c, f) for c, f, _, _ in _members(first)) == [(64, 3)] * 3
    assert sorted(i for _, _, i, _ in _members(first)) == sorted(i for _, _, i, _ in _members(second)) == sorted(first["in"]) == sorted(second["in"])
    assert sorted(mm["hw_in"][0] for mm in second["members"]) == [20, 40, 80]
    assert _order_is_topological(on)
    monkeypatch.setenv("TRTX_SIBLING_PAIR", "0")
    off = _low(bench_plan)
    assert _marked(off["ops"]) == [] and _order_is_topological(off)
    # the mark (and where the marked group stands) is all that differs: op count, kinds, names, members
    assert len(ops) == len(off["ops"]) == 53 and on["n_conv"] == off["n_conv"] == 63
    strip = lambda o: {key: v for key, v in o.items() if key not in ("sibling_pair", "waits")}
    key = lambda o: (o["kind"], o["name"])
    assert sorted(map(key, ops)) == sorted(map(key, off["ops"]))
    assert sorted((key(o), _members(o)) for o in ops if o["kind"] == "conv_group") == sorted((key(o), _members(o)) for o in off["ops"] if o["kind"] == "conv_group")
    rest_on = [strip(o) for j, o in enumerate(ops) if j != k]
    rest_off = [strip(o) for o in off["ops"] if key(o) != key(second)]
    assert rest_on == rest_off          # every other op, in the same order
    assert [t for t in on["tensors"]] == [t for t in off["tensors"]]


def test_the_arena_keeps_the_six_outputs_off_the_inputs_and_off_each_other(bench_plan):
    low = _low(bench_plan)
    ops = low["ops"]
    k = _marked(ops)[0]
    outs, ins = ops[k - 1]["out"] + ops[k]["out"], ops[k]["in"]
    assert len(outs) == 6 and len(ins) == 3

    def block(t):
        s = low["storages"][low["tensors"][t]["storage"]]
        return s["offset"], s["offset"] + s["bytes"]
    apart = lambda a, b: a[1] <= b[0] or b[1] <= a[0]
    for i, t in enumerate(outs):
        for u in ins:
            assert apart(block(t), block(u)), (t, u)
        for u in outs[i + 1:]:
            assert apart(block(t), block(u)), (t, u)


def test_other_builds_are_not_marked(monkeypatch):
    from tensorrtx_amd import calibrator
    path, _ = synth_wts("yolov8n")
    assert _marked(_low(engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=0, aux_streams=0))["ops"]) == []     # fp32 build
    plan16 = engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=1, aux_streams=0)
    assert len(_marked(_low(plan16)["ops"])) == 1
    names = [t["name"] or f"(Unnamed Tensor* {t['id']})" for t in engine.describe_plan(plan16)["tensors"]]
    cache = b"TRT-8601-EntropyCalibration2\n" + b"".join(f"{n}: {struct.unpack('<I', struct.pack('<f', 0.05))[0]:08x}\n".encode() for n in names)
    with calibrator.Calibrator(cache=cache).installed():
        plan8 = engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=1, int8=1, aux_streams=0)
    assert engine.describe_plan(plan8)["int8"] is True and _marked(_low(plan8)["ops"]) == []
    monkeypatch.setenv("TRTX_GROUP_CONVS", "0")     # no groups, no pair of groups
    assert _marked(_low(plan16)["ops"]) == []


def test_the_serialized_plan_does_not_carry_the_mark(monkeypatch):
    """the mark is re-derived wherever a plan is lowered: the plan bytes are the same with the switch on and off, and one plan lowers either way"""
    path, _ = synth_wts("yolov8n")
    plan = engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=1, aux_streams=0)
    assert engine.describe_plan(plan) == engine.describe_plan(bytes(bytearray(plan)))
    monkeypatch.setenv("TRTX_SIBLING_PAIR", "0")
    assert engine.build_plan("yolov8n", path, batch=2, h=160, w=160, fp16=1, aux_streams=0) == plan
    assert _marked(_low(plan)["ops"]) == []
    monkeypatch.delenv("TRTX_SIBLING_PAIR")
    assert len(_marked(_low(plan)["ops"])) == 1


def test_no_mark_where_the_two_groups_sit_on_different_lanes(monkeypatch):
    """an engine with auxiliary streams (the default: 3) spreads independent branches over lanes - the two sibling groups overlap there instead, and the
    plan is what it is with the switch off, op order included; the same plan on one lane (TRTX_LANES=1) has the pair"""
    path, _ = synth_wts("yolov8n")
    plan = engine.build_plan("yolov8n", path, batch=32, h=640, w=640, fp16=1)
    low = _low(plan)
    ops = low["ops"]
    assert low["n_lanes"] > 1 and _marked(ops) == [] and _order_is_topological(low)
    groups = [o for o in ops if o["kind"] == "conv_group"]
    g64 = next(o for o in groups if sorted((c, f) for c, f, _, _ in _members(o)) == [(64, 3)] * 3)      # (the first one: cv2.x.0)
    g80 = next(o for o in groups if sorted(o["in"]) == sorted(g64["in"]) and o is not g64)
    assert g64["lane"] != g80["lane"]
    monkeypatch.setenv("TRTX_SIBLING_PAIR", "0")
    assert _low(plan)["ops"] == ops
    monkeypatch.delenv("TRTX_SIBLING_PAIR")
    monkeypatch.setenv("TRTX_LANES", "1")
    one = _low(plan)
    assert one["n_lanes"] == 1 and len(_marked(one["ops"])) == 1
