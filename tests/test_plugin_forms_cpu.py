"""Every built-in plugin comes back from a plan as itself: the six forms that share the name "YoloLayer_TRT" (told apart by their creator
fields when created and by nothing but the blob's length when deserialized), "Decode_TRT" and "Mish_TRT".  Created through the registry
at the smallest and the largest level count the creator takes, read back with describe_plan (which deserializes the layer and serializes
it again), and refused one byte short and one byte long.  No GPU."""
import ctypes
import itertools
import struct

import numpy as np
import pytest

from oracle import graph_interp as gi
from tensorrtx_amd import builder, capi, engine

MAX_OUT = 50
ANCH = np.arange(48, dtype=np.float32).reshape(8, 6) + 1

# form -> (blob length for n levels, the n a blob may hold, floats per Detection record): plugins/builtin_plugins.cpp, kYoloForms
FORMS = {
    "v8": (lambda n: 35 + 4 * n, range(0, 9), 90),
    "v5": (lambda n: 25 + 32 * n, range(1, 9), 38),
    "v9": (lambda n: 21, range(0, 1), 38),
    "v7": (lambda n: 24 + 32 * n, range(1, 9), 6),
    "darknet": (lambda n: 20 + 32 * n, range(0, 9), 7),
    "v10": (lambda n: 24 + 4 * n, range(1, 6), 6),
}


def test_no_blob_length_belongs_to_two_forms():
    """what yolo_deserialize rests on: the length alone names the form"""
    lengths = {form: {f(n) for n in ns} for form, (f, ns, _) in FORMS.items()}
    assert [len(v) for v in lengths.values()] == [9, 8, 1, 8, 9, 5]
    for a, b in itertools.combinations(FORMS, 2):
        assert not lengths[a] & lengths[b], (a, b, sorted(lengths[a] & lengths[b]))


def form_net(form, n, classes=7):
    """(plan, leading ints of the blob, output dims) of one plugin on network inputs, implicit batch.  H x W = 256 x 384, level k on stride 2^k
    (the Darknet form reads its geometry off its inputs: coarsest first on 32 / 16 (/ 8) for n = 2 (3))"""
    H, W = 256, 384
    net = builder.Network(max_batch=2)
    try:
        strides = [32, 16, 8][:n] if form == "darknet" else ([8, 16, 32] if form == "v9" else [1 << k for k in range(n)])
        grid = [(H // s, W // s) for s in strides]
        fields, lead = None, None
        if form in ("v8", "v9", "v10"):
            info = 4 + classes
            ins = [net.input(f"x{k}", (info, gh * gw)) for k, (gh, gw) in enumerate(grid)]
            if form == "v8":
                fields = [("combinedInfo", np.array([classes, 17, 0, W, H, MAX_OUT, 0, 0, 0] + strides, np.int32))]
                lead = [classes, 17, 0, 256, W, H, MAX_OUT, n] + strides
            elif form == "v9":
                fields = [("netinfo", np.array([classes, W, H, MAX_OUT, 0], np.int32))]
                lead = [classes, 256, W, H, MAX_OUT]
            else:
                fields = [("combinedInfo", np.array([classes, W, H, MAX_OUT] + strides, np.int32))]
                lead = [classes, 256, W, H, MAX_OUT, n] + strides
        else:
            ins = [net.input(f"x{k}", (3 * (5 + classes), gh, gw)) for k, (gh, gw) in enumerate(grid)]
            if form == "darknet":
                lead = [classes, 256, n]
            else:
                kern = np.concatenate([np.concatenate([np.array([gw, gh], np.int32).view(np.float32), ANCH[k]]) for k, (gh, gw) in enumerate(grid)])
                fields = [("netinfo", np.array([classes, W, H, MAX_OUT] + ([0] if form == "v5" else []), np.int32)), ("kernels", kern.astype(np.float32), n)]
                lead = [classes, 256, n, W, H, MAX_OUT]
        net.mark_output(net.out(net.plugin(ins, "YoloLayer_TRT", fields=fields)), "prob")
        return net.build(), lead
    finally:
        net.close()


def other_net(kind):
    net = builder.Network(max_batch=2)
    try:
        if kind == "Decode_TRT":
            ins = [net.input(f"x{k}", (32, 96 >> (3 + k), 160 >> (3 + k))) for k in range(3)]
        else:
            ins = [net.input("x", (3, 5, 7))]
        net.mark_output(net.out(net.plugin(ins, kind)), "prob")
        return net.build()
    finally:
        net.close()


def plugin_of(plan):
    desc = engine.describe_plan(plan)
    (pl,) = [l for l in desc["layers"] if l["kind"] == gi.L_PLUGIN]
    (out,) = [t for t in desc["tensors"] if t["is_output"]]
    return pl["plugin_type"], bytes.fromhex(pl["plugin_blob"]), out["dims"]


def with_blob(plan, old, new):
    """the plan with the plugin's blob `old` (a uint64 length, then the bytes: Network::serialize) exchanged for `new`"""
    stored = struct.pack("<Q", len(old)) + old
    assert plan.count(stored) == 1
    return plan.replace(stored, struct.pack("<Q", len(new)) + new)


def round_trips(plan, kind, length):
    """the blob the plan stores is what a deserialized instance serializes, twice over; returns (blob, output dims)"""
    typ, blob, dims = plugin_of(plan)
    assert typ == kind and len(blob) == length
    again = plugin_of(with_blob(plan, blob, blob))   # also: the plan stores exactly these bytes
    assert again == (typ, blob, dims)
    return blob, dims


def refused(plan):
    """a plugin blob that no form takes: trtx_plan_describe answers status 6 (I/O or parse error), as it did before the forms became a table"""
    with pytest.raises(capi.TrtxError) as e:
        engine.describe_plan(plan)
    return e.value.status == 6


CASES = [("v8", 1), ("v8", 8), ("v5", 1), ("v5", 8), ("v9", 0), ("v7", 1), ("v7", 8), ("darknet", 2), ("darknet", 3), ("v10", 1), ("v10", 5)]


@pytest.mark.parametrize("form,n", CASES, ids=[f"{f}-{n}" for f, n in CASES])
def test_yolo_form_comes_back_as_itself(form, n):
    length, levels, rec = FORMS[form]
    assert n in levels
    plan, lead = form_net(form, n)
    blob, dims = round_trips(plan, "YoloLayer_TRT", length(n))
    ints = np.frombuffer(blob[:4 * len(lead)], "<i4").tolist()
    if form == "v8":
        ints[2] = struct.unpack("<f", blob[8:12])[0]   # the keypoint threshold is a float
    assert ints == lead
    assert dims == [1 + (1000 if form == "darknet" else MAX_OUT) * rec, 1, 1]
    if form in ("v5", "v7", "darknet"):
        at = {"v5": 25, "v7": 24, "darknet": 12}[form]
        kern = np.frombuffer(blob[at:at + 32 * n], "<i4").reshape(n, 8)
        want = [[384 * s // 32, 256 * s // 32] for s in (1, 2, 4)[:n]] if form == "darknet" else [[384 >> k, 256 >> k] for k in range(n)]
        assert kern[:, :2].tolist() == want
    if form == "darknet":
        assert np.frombuffer(blob[-8:], "<i4").tolist() == [384, 256]


@pytest.mark.parametrize("form,n", [("v8", 3), ("v5", 3), ("v9", 0), ("v7", 3), ("darknet", 3), ("v10", 3)], ids=list(FORMS))
def test_yolo_blob_one_byte_off_is_refused(form, n):
    plan, _ = form_net(form, n)
    _, blob, _ = plugin_of(plan)
    short = with_blob(plan, blob, blob[:-1])
    if form == "v5":
        # 25 + 32 n - 1 is YOLOv7's length, and without its last byte the blob IS a YOLOv7 blob: the six ints, then YoloKernels that start where
        # the segmentation flag stood.  Their grids are shifted by a byte, but nothing bounds them from above: it comes back as YOLOv7's
        typ, back, dims = plugin_of(short)
        assert (typ, back, dims) == ("YoloLayer_TRT", blob[:-1], [1 + MAX_OUT * FORMS["v7"][2], 1, 1])
    else:
        assert refused(short), "one byte short"
    assert refused(with_blob(plan, blob, blob + b"\0")), "one byte long"


def test_decode_and_mish_come_back_as_themselves():
    plan = other_net("Decode_TRT")
    blob, dims = round_trips(plan, "Decode_TRT", 8)
    assert np.frombuffer(blob, "<i4").tolist() == [96, 160]
    L = capi.lib()
    L.trtx_retina_decode_output_floats.restype = ctypes.c_size_t
    assert dims == [L.trtx_retina_decode_output_floats(96, 160), 1, 1]
    assert plugin_of(with_blob(plan, blob, b""))[1] == struct.pack("<ii", 480, 640), "an empty blob is the reference's 480 x 640"
    assert refused(with_blob(plan, blob, blob[:-1])) and refused(with_blob(plan, blob, blob + b"\0"))
    plan = other_net("Mish_TRT")
    blob, dims = round_trips(plan, "Mish_TRT", 4)
    assert np.frombuffer(blob, "<i4").tolist() == [3 * 5 * 7] and dims == [3, 5, 7]
    assert refused(with_blob(plan, blob, blob[:-1])) and refused(with_blob(plan, blob, blob + b"\0"))
