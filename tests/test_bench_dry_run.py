"""bench.py's control flow on CPU: the exact launch line the driver uses for N > 1 (python -m torch.distributed.run --nproc-per-node N
... bench.py --gpus N --steps K --warmup W), with --dry-run putting stand-ins in place of every GPU object and gloo in place of RCCL.
What runs for real: RANK / WORLD_SIZE handling, rank 0 building the plan and broadcasting it, the per-rank input seeds, settle / warm-up
/ K-step legs with their barriers and the max-over-ranks reduce, the host-fed ring, one JSON line from rank 0 only."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(n, extra=(), full=True):
    """full: the line with every side measurement (--full, three legs); otherwise the plain run the driver times"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    flags = ["--steps", "6", "--warmup", "2"] + (["--repeats", "3", "--full"] if full else []) + list(extra)
    if n == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--gpus", "1", *flags]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port",
               str(_free_port()), os.path.join(ROOT, "bench.py"), "--dry-run", "--gpus", str(n), *flags]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line (rank 0 only), got {len(lines)}"
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2])
def test_bench_control_flow_weak_scaling(n):
    d = _run(n)
    assert d["dry_run"] is True and d["n_gpus"] == n and d["steps"] == 6 and d["warmup"] == 2
    assert d["scaling"] == "weak" and d["higher_is_better"] is True and d["unit"] == "images/sec"
    assert len(d["legs_ms"]) == 3 and all(x > 0 for x in d["legs_ms"])
    assert abs(d["value"] - 32 * n / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]      # whole-job aggregate over all ranks
    assert d["config"]["workload"] and "roofline" in d and d["roofline"]["launches_per_step"] > 40
    # every rank's own step time and pinning report travel in the line: a straggler is visible, not folded into the max (VERDICT r5 Weak 10)
    assert len(d["per_rank_ms_per_step"]) == n and all(0 < x <= d["ms_per_step"] * (1 + 1e-6) + 1e-3 for x in d["per_rank_ms_per_step"])
    assert len(d["config"]["cpu_affinity_per_rank"]) == n
    assert "plugins" in d["roofline"] and "frac_serialized_kernels" in d["roofline"] and "frac_whole_step_hbm" in d["roofline"]
    assert ("cpu_baseline" in d) == False   # noqa: E712  (the oracle needs real GPU outputs to be compared with: not in a dry run)


def test_bench_control_flow_strong_scaling_two_ranks():
    d = _run(2, ("--mode", "strong"))
    assert d["scaling"] == "strong" and d["n_gpus"] == 2
    assert abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]          # the global batch is fixed: 16 + 16


def test_bench_control_flow_c4_strong_split_builds_small_batch_engines():
    """C4 (RetinaFace-R50 1280x1280, global batch 8) is strong-scaled by default: with 8 GPUs every rank gets ONE image, so the builders must
    accept a max batch below the config's.  Two ranks here (4 images each) through the same code; the batch-1 build itself is checked on
    this process (the shape rank k of 8 would build)."""
    d = _run(2, ("--config", "retinaface_r50"))
    assert d["scaling"] == "strong" and d["n_gpus"] == 2 and d["config"]["global_batch"] == 8
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tensorrtx_amd import engine, replicas
    from util import synth_wts
    assert [len(list(replicas.partition(8, 8, r))) for r in range(8)] == [1] * 8
    path, _ = synth_wts("retinaface_r50")
    plan = engine.build_plan("retinaface_r50", path, batch=1, fp16=1, h=1280, w=1280, aux_streams=0)
    assert engine.describe_plan(plan, lowered=True)["max_batch"] == 1


def test_bench_control_flow_c4_eight_ranks_one_image_each():
    """the driver's 8-GPU line for C4 - `--gpus 8 --config retinaface_r50`, strong scaling by default: rank k gets image k of the global
    batch of 8 - rehearsed with eight gloo ranks: plan broadcast of a batch-1 engine, per-rank partition, barriers, max over ranks, one JSON line."""
    d = _run(8, ("--config", "retinaface_r50"))
    assert d["scaling"] == "strong" and d["n_gpus"] == 8 and d["config"]["global_batch"] == 8
    assert len(d["per_rank_ms_per_step"]) == 8 and len(d["config"]["cpu_affinity_per_rank"]) == 8
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]


def test_numa_pinning_helpers_without_a_gpu():
    """replicas.pin_to_gpu_numa_node: cpulist parsing, and no GPU / no sysfs entry leaves the affinity alone and says why (never raises)."""
    from tensorrtx_amd import replicas
    assert replicas.parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11] and replicas.parse_cpulist("5") == [5]
    before = os.sched_getaffinity(0)
    note = replicas.pin_to_gpu_numa_node(0, 0, 1)
    assert note.startswith("affinity unchanged") and os.sched_getaffinity(0) == before


def test_bench_prints_the_tolerance_engine_leg():
    """the default line (yolov8n, fp16) carries `tolerance_engine` - the fp32 build timed like `value` - with its own legs, dtype and
    roofline against the fp32 MFMA peak; --no-tolerance-engine drops it."""
    d = _run(1)
    t = d["tolerance_engine"]
    assert t["dtype"] == "f32" and t["value"] > 0 and len(t["legs_ms"]) >= 3 and t["roofline"]["peak"] == 157.3 and t["roofline"]["launches_per_step"] >= 60
    assert "tolerance_engine" not in _run(1, ("--no-tolerance-engine",))


def test_bench_in_process_replicas_control_flow():
    """--replicas in-process: one process, N devices through DeviceReplicas (the reference's tutorials/multi_GPU_processing.md recipe); dry run
    with three stand-in devices: every device gets a batch per step, value = all devices' images over the host clock."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--replicas", "in-process", "--gpus", "3", "--steps", "6", "--warmup", "2",
                        "--repeats", "3"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["dry_run"] is True and d["n_gpus"] == 3 and d["config"]["global_batch"] == 96 and len(d["legs_ms"]) == 3
    assert abs(d["value"] - 96 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]


@pytest.mark.parametrize("n", [1, 2])
def test_plain_run_times_one_leg_of_exactly_the_steps_and_nothing_else(n):
    """Without --full the line is the headline figure alone: one leg of exactly --steps timed steps (ms_per_step is that leg's), none of the
    side legs, the roofline profile, the fp32 engine or the CPU oracle."""
    d = _run(n, full=False)
    assert d["dry_run"] is True and d["n_gpus"] == n and d["steps"] == 6 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["unit"] == "images/sec" and d["dtype"] == "f16" and d["metric"].startswith("images/sec @ batch=32 640x640 fp16")
    assert len(d["legs_ms"]) == 1 and d["legs_ms"][0] == round(d["ms_per_step"], 4)
    assert abs(d["value"] - 32 * n / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "single_context", "d2h_inclusive", "host_fed", "tolerance_engine", "cpu_baseline", "parity"):
        assert k not in d, k


def _dumped(path):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".npy")}


@pytest.mark.parametrize("full", [False, True])
def test_dump_outputs_writes_the_last_steps_results(tmp_path, full):
    """--dump-outputs DIR: the decode buffer and the NMS results of the last timed step as DIR/<name>.npy, float32 / float64, at most 64 MB,
    the same from run to run (stale records past each image's count are zeroed)."""
    import numpy as np
    a, b = tmp_path / "a", tmp_path / "b"
    _run(1, ("--dump-outputs", str(a)), full=full)
    _run(1, ("--dump-outputs", str(b)), full=full)
    da, db = _dumped(a), _dumped(b)
    assert sorted(da) == ["nms_keep_count", "nms_keep_det", "nms_keep_index", "output"]
    assert da["output"].shape == (32, 1 + 1000 * 90) and da["nms_keep_det"].shape == (32, 1000, 6) and da["nms_keep_count"].shape == (32,)
    assert all(x.dtype in (np.float32, np.float64) for x in da.values())
    assert sum(x.nbytes for x in da.values()) <= 64 << 20
    assert all(np.array_equal(da[k], db[k]) for k in da)


def test_dump_helpers_canonicalise_and_bound_the_outputs(tmp_path):
    """the dump's own rules, on made-up arrays: records past a decode count and NMS entries past the kept count are cleared; an output larger
    than the 64 MB budget is replaced by the same seeded sample every time"""
    code = r'''
import sys, os, numpy as np
import bench
buf = np.arange(2 * (1 + 3 * 2), dtype=np.float32).reshape(2, 7); buf[0, 0] = 1; buf[1, 0] = 9
d = bench._decode_records(buf, 2)
assert d[0, 1:3].tolist() == [1, 2] and not d[0, 3:].any() and d[1, 1:].tolist() == buf[1, 1:].tolist()
n = bench._nms_arrays(np.array([1, 0], np.int32), np.array([[5, 6], [7, 8]], np.int32), np.ones((2, 2, 6), np.float32))
assert n["nms_keep_index"].tolist() == [[5, -1], [-1, -1]] and n["nms_keep_det"][0, 0].all() and not n["nms_keep_det"][0, 1:].any()
assert n["nms_keep_count"].dtype == np.float64 and not n["nms_keep_det"][1].any()
big = np.arange(10 << 20, dtype=np.float64)   # 80 MB
for out in sys.argv[1:]:
    bench.dump_outputs(out, {"big": big, "small": np.arange(4, dtype=np.int32)})
x, y = (np.load(os.path.join(o, "big.npy")) for o in sys.argv[1:])
assert x.nbytes <= 32 << 20 and np.array_equal(x, y) and np.all(np.diff(x) > 0)
assert np.load(os.path.join(sys.argv[1], "small.npy")).dtype == np.float64
'''
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "a"), str(tmp_path / "b")], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
