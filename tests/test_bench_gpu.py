"""bench.py end to end on the GPU box: the single-process line (all contract fields, roofline + isolated pass + cpu_baseline
object) and the N = 2 control flow (two ranks sharing cuda:0 over gloo -- the box has one GPU -- so every collective of the
timed region, the isolated pass and the max-over-ranks reduction is matched on both ranks)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
          "dtype", "data", "config", "roofline")


def _fresh_process_only():
    """bench.py is started as a child process; this file sorts first in the suite, so the pytest process has not touched the
    GPU yet -- if it has (another order), skip rather than spawn a program from a process that already initialised the GPU"""
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        pytest.skip("run tests/test_bench_gpu.py in a fresh process")


def _the_line(out):
    """stdout holds exactly ONE JSON line, it is the last line, it is compact (the driver keeps an 8 KB tail) and it round-trips"""
    lines = out.splitlines()
    js = [l for l in lines if l.startswith("{")]
    assert len(js) == 1 and lines[-1] == js[0], out[-2000:]
    assert len(js[0]) < 4096, len(js[0])
    d = json.loads(js[0])
    assert json.loads(json.dumps(d)) == d
    return d


def _detail(d):
    with open(os.path.join(ROOT, d["detail"])) as f:
        return json.load(f)


def test_bench_single_process_line():
    _fresh_process_only()
    r = subprocess.run([sys.executable, "bench.py", "--full", "--model", "crnn", "--experts", "3", "--batch", "32", "--steps", "2",
                        "--warmup", "1", "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _the_line(r.stdout)
    for k in FIELDS:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["scaling"] == "weak" and d["data"] == "synthetic"
    rl = d["roofline"]
    assert rl["bound"] in ("mfma", "hbm") and 0 < rl["frac"] < 1 and rl["peak"] > 0 and "isolated" in rl
    assert len(rl["kernel"]) < 64                      # a kernel name, not a paragraph
    full = _detail(d)                                  # everything else: the side file
    assert full["value"] == pytest.approx(d["value"], rel=1e-4) and "measured" in full["roofline"]


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """without --full: the headline fields only, --steps timed steps, and --dump-outputs writes the last timed step's losses, fused
    logits, routing weights and router parameters as float32 .npy files"""
    _fresh_process_only()
    r = subprocess.run([sys.executable, "bench.py", "--model", "crnn", "--experts", "3", "--batch", "32", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _the_line(r.stdout)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] == pytest.approx(32e3 / d["ms_per_step"], rel=1e-3)
    for k in ("roofline", "cpu_baseline", "extra", "comm", "detail"):
        assert k not in d, k
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("loss_clf", "loss_taski", "logits", "routing_weights", "router_parameters")}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["logits"].ndim == 3 and got["logits"].shape[0] == 32 and got["routing_weights"].shape == (32, 3)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20


def test_bench_default_command_line_is_compact_and_complete():
    """the --full command (default workload: TRBA x 6, batch 256, every extra line, the CPU baseline leg), shortened only in
    --steps / --warmup: ONE parseable line under 4 KB carrying roofline.frac and cpu_baseline.value (the 20 KB line
    of round 5 did not parse and voided the round's measurement)"""
    _fresh_process_only()
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1"], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _the_line(r.stdout)
    for k in FIELDS + ("cpu_baseline", "extra", "detail"):
        assert k in d, k
    assert d["metric"] == "text-line images/sec (fwd+bwd) at 32x256, TRBA+MRN 6 experts" and d["dtype"] == "f32" and d["vs_baseline"] is None
    assert d["config"]["per_gpu_batch"] == 256 and len(d["config"]["classes"]) == 6 and len(d["config"]["workload"]) <= 120
    rl, cb = d["roofline"], d["cpu_baseline"]
    assert rl["bound"] == "mfma" and 0 < rl["frac"] < 1 and rl["achieved"] / rl["peak"] == pytest.approx(rl["frac"], rel=1e-3)
    assert rl["kernel"].startswith("wino_rows_kernel") and rl["avg_launch_ms"] > 0 and rl["launches_per_step"] > 0
    assert cb["value"] > 0 and cb["kind"] == "port" and cb["cores"] >= 1 and cb["unit"] == "images/s"
    ia = cb["index_agreement"]                         # measured on this run's noise crops against the oracle
    assert ia["routing_argmax_agreement"] >= 0.9 and ia["greedy_index_agreement"] >= 0.99
    for name in ("loop_a", "der", "fp16_loop_b", "fp16_der", "crnn3_loop_b", "svtr6_loop_b"):
        assert d["extra"][name]["value"] > 0 and d["extra"][name]["ms_per_step"] > 0
    full = _detail(d)
    assert "roofline_other_kernels" in full and "roofline" in full["extra"]["loop_a"]


def test_bench_two_ranks_control_flow():
    _fresh_process_only()
    # the DRIVER's command: bare `python bench.py --gpus 2 ...`, no launcher -- bench.py starts its own ranks as child processes
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(MRN_DIST_BACKEND="gloo", MRN_SHARE_DEVICE="1")
    cmd = [sys.executable, "bench.py", "--full", "--gpus", "2", "--model", "crnn", "--experts", "3", "--batch", "16", "--steps", "2", "--warmup", "1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)     # (a timeout FAILS the test)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = _the_line(r.stdout)                 # rank 0 prints exactly one line
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 32 and d["config"]["parallelism"] == "dp2"
    assert "cpu_baseline" not in d          # reported at N = 1 only
    assert d["comm"]["ranks_seen"] == [0, 1] and d["comm"]["backend"] == "gloo"
    # comm telemetry of the N > 1 record: did the backend see both ranks, what one step's gradient exchange moves and costs
    full = _detail(d)
    for line in (full, full["extra"]["loop_a"]):
        c = line["comm"]
        assert c["backend"] == "gloo" and c["ranks_seen"] == [0, 1] and "rccl_version" in c
        assert c["allreduce_bytes_per_step"] > 0 and c["buckets"] >= 1 and c["allreduce_ms_per_step"] > 0
        assert c["exposed_ms_per_step"] >= 0 and 0.0 <= c["overlap_frac"] <= 1.0
    assert full["comm"]["allreduce_bytes_per_step"] < full["extra"]["loop_a"]["comm"]["allreduce_bytes_per_step"]     # router only vs a whole expert
    # N > 1 runs the single-GPU schedule: parameter gradients on the side stream, the buckets told through direct_gradients(notify=)
    assert full["extra"]["loop_a"]["comm"]["side_stream_parameters_per_step"] > 0


def test_bench_refuses_a_mismatched_world():
    """under a launcher (RANK set) --gpus must equal WORLD_SIZE; nothing touches the GPU before the check"""
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stdout + r.stderr)


DP_WORKER = r"""
import contextlib, io, os, sys, torch
sys.path.insert(0, os.environ["MRN_ROOT"])
import bench
from mrn_amd import parallel
from mrn_amd.data.synthetic import SyntheticTextLines
from mrn_amd.tools.utils import to_device
rank, world, local = parallel.init_distributed()
torch.cuda.set_device(0)
torch.manual_seed(111 + 17 * rank)                  # replicas are BUILT differently: the broadcasts must equalise them
opt = bench.make_opt("crnn", 8)
learner = bench.build_learner(opt, 3)
assert learner.reducer is not None
data = SyntheticTextLines(opt, seed=5 + rank)       # every rank its own shard
data.set_characters(learner.character)
for it in range(2):
    image, labels, idx = data.get_batch2()
    learner.routing_step(image, labels, to_device(torch.LongTensor(idx).squeeze()))
torch.cuda.synchronize()
flat = learner.optimizer.flat.detach().cpu()
frozen = torch.cat([p.detach().reshape(-1).cpu() for p in learner.model.module.model.parameters()])
both = [torch.zeros_like(flat) for _ in range(world)]
torch.distributed.all_gather(both, flat)
assert torch.equal(both[0], both[1]), "router parameters differ between the ranks after two steps"
bf = [torch.zeros_like(frozen) for _ in range(world)]
torch.distributed.all_gather(bf, frozen)
assert torch.equal(bf[0], bf[1]), "frozen experts differ between the ranks (broadcast_module)"
# CrossEntropyLoss(ignore_index=[PAD]) under data parallelism: this rank's loss, weighted by its share of the valid targets, has
# the gradient (after the 1 / world average) of DataParallel's mean over the GATHERED batch (reference il_modules/base.py:68,134)
from mrn_amd.il_modules.base import Criterion
def shard(r):
    g = torch.Generator().manual_seed(900 + r)
    lg = torch.randn(6, 26, 40, generator=g)
    tg = torch.randint(2, 40, (6, 27), generator=g)
    for b in range(6):
        tg[b, 3 + 4 * r + b:] = 1                       # [PAD] = 1 after a rank-dependent label length
    return lg, tg
lg, tg = shard(rank)
mine = lg.cuda().requires_grad_(True)
Criterion("Attn", pad_index=1)(mine, tg.cuda()).backward()
allg = torch.cat([shard(r)[0] for r in range(world)]).requires_grad_(True)
allt = torch.cat([shard(r)[1] for r in range(world)])
torch.nn.functional.cross_entropy(allg.view(-1, 40), allt[:, 1:].reshape(-1), ignore_index=1).backward()
want = allg.grad[6 * rank:6 * rank + 6]
got = mine.grad.cpu() / world
assert (got - want).abs().max().item() <= 1e-7 * max(1.0, want.abs().max().item()) + 1e-9, (got - want).abs().max().item()
path = learner.checkpoint_path(2, 1)
learner.save_checkpoint(2, 1)                        # rank 0 writes, the others return
parallel.barrier()
assert os.path.exists(path) == True
open(os.path.join(os.environ["MRN_OUT"], f"dp_ok_{rank}"), "w").write("ok")
"""


DP_LOOP_A_WORKER = r"""
import os, sys, torch
sys.path.insert(0, os.environ["MRN_ROOT"])
import bench
from mrn_amd import ops, parallel
from mrn_amd.data.synthetic import SyntheticTextLines
rank, world, local = parallel.init_distributed()
torch.cuda.set_device(0)
torch.manual_seed(7 + 31 * rank)                    # replicas are BUILT differently: the broadcasts must equalise them
model = os.environ["MRN_MODEL"]
opt = bench.make_opt(model, 8)
learner = bench.build_loop_a_learner(opt)
assert learner.reducer is not None and ops.WGRAD_SIDE_STREAM
data = SyntheticTextLines(opt, seed=50 + rank)      # every rank its own shard
data.set_characters(learner.character)
n_params = len(learner.optimizer.params)
for it in range(3):
    before = ops.DIRECT_STATS["parameters"]
    learner.train_step(*data.get_batch())
    side = ops.DIRECT_STATS["parameters"] - before
    # the side stream carried the weight gradients of the convolutions, Linear / LSTM / decoder layers (BatchNorm / LayerNorm parameters and
    # some biases come back through autograd), and every bucket was still launched exactly once, in order
    assert side >= 0.4 * n_params, (side, n_params)
    assert learner.reducer.launched_log == list(range(len(learner.reducer.buckets))), learner.reducer.launched_log
torch.cuda.synchronize()
flat = learner.optimizer.flat.detach().cpu()
assert torch.isfinite(flat).all()
both = [torch.zeros_like(flat) for _ in range(world)]
torch.distributed.all_gather(both, flat)
assert torch.equal(both[0], both[1]), "trained parameters differ between the ranks after three loop-A steps"
open(os.path.join(os.environ["MRN_OUT"], f"dpa_ok_{rank}"), "w").write("ok")
"""


@pytest.mark.parametrize("model", ["crnn", "trba", "svtr"])
def test_two_ranks_loop_a_side_stream_identical_parameters(tmp_path, model):
    """loop A under data parallelism keeps the single-GPU schedule: parameter gradients are accumulated on the
    side stream and the bucketed all-reduce is told through direct_gradients(notify=); after three steps on different shards the
    two ranks' flat parameter buffers are bit-identical (reference: DataParallel at il_modules/base.py:68)"""
    _fresh_process_only()
    script = tmp_path / "dp_loop_a_worker.py"
    script.write_text(DP_LOOP_A_WORKER)
    env = dict(os.environ, MRN_ROOT=ROOT, MRN_OUT=str(tmp_path), MRN_DIST_BACKEND="gloo", MRN_SHARE_DEVICE="1", MRN_MODEL=model,
               MRN_BUCKET_MB="4")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(29561 + ["crnn", "trba", "svtr"].index(model)), str(script)], cwd=tmp_path,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert (tmp_path / "dpa_ok_0").exists() and (tmp_path / "dpa_ok_1").exists()


def test_two_ranks_routing_steps_identical_parameters(tmp_path):
    """two ranks (one GPU shared, gloo) built from DIFFERENT seeds: after the learner's broadcasts and two routing steps on
    different shards the trainable flat buffer and the frozen experts are bit-identical on both ranks; one checkpoint file"""
    _fresh_process_only()
    root = ROOT
    script = tmp_path / "dp_worker.py"
    script.write_text(DP_WORKER)
    env = dict(os.environ, MRN_ROOT=root, MRN_OUT=str(tmp_path), MRN_DIST_BACKEND="gloo", MRN_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29547", str(script)], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert (tmp_path / "dp_ok_0").exists() and (tmp_path / "dp_ok_1").exists()
    assert len([f for f in os.listdir(tmp_path / "saved_models" / "bench") if f.endswith(".pth")]) == 1


NATIVE_WORKER = r"""
import os, sys, torch
sys.path.insert(0, os.environ["MRN_ROOT"])
from mrn_amd import parallel
rank, world, local = parallel.init_distributed()          # gloo carries the 128-byte rendezvous id only
torch.cuda.set_device(0)
out = os.environ["MRN_OUT"]
try:
    assert parallel.init_native_comm() == 2               # mrn_comm_unique_id / mrn_comm_init: the library's own RCCL communicator
except RuntimeError as e:
    open(os.path.join(out, f"native_refused_{rank}"), "w").write(str(e))
    sys.exit(0)
g = torch.full((1 << 16,), float(rank + 1), device="cuda")
parallel._avg_inplace(g)                                   # MRN_COMM=native: mrn_allreduce_f32 on the comm stream
torch.cuda.synchronize()
assert torch.equal(g, torch.full_like(g, 1.5)), g[:4]
b = torch.full((33,), float(rank), device="cuda")
parallel.native_broadcast(b, src=1)
torch.cuda.synchronize()
assert torch.equal(b, torch.ones_like(b))
open(os.path.join(out, f"native_ok_{rank}"), "w").write("ok")
"""


def test_two_ranks_native_rccl_on_the_shared_device(tmp_path):
    """csrc/comm.cpp with world > 1: two ranks, MRN_COMM=native, both on cuda:0 -- the box has one GPU.  RCCL
    either forms the communicator (then mrn_allreduce_f32 / mrn_broadcast_f32 are checked numerically) or refuses two ranks on one
    device (its duplicate-GPU check): then the refusal must arrive as the library's RuntimeError on BOTH ranks, not as a hang, and the
    test is reported as skipped with RCCL's own message -- the world > 1 path then stays covered by the gloo tests only."""
    _fresh_process_only()
    script = tmp_path / "native_worker.py"
    script.write_text(NATIVE_WORKER)
    env = dict(os.environ, MRN_ROOT=ROOT, MRN_OUT=str(tmp_path), MRN_DIST_BACKEND="gloo", MRN_SHARE_DEVICE="1", MRN_COMM="native",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    try:
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                            "127.0.0.1", "--master-port", "29571", str(script)], cwd=tmp_path, env=env, capture_output=True, text=True,
                           timeout=240)
    except subprocess.TimeoutExpired:
        pytest.skip("RCCL communicator of two ranks on ONE device did not form within 240 s (duplicate-GPU rendezvous): world > 1 of "
                    "csrc/comm.cpp needs two GPUs")
    refused = sorted(f for f in os.listdir(tmp_path) if f.startswith("native_refused_"))
    if refused:
        assert len(refused) == 2 and r.returncode == 0, (refused, (r.stdout + r.stderr)[-2000:])
        pytest.skip("RCCL refuses two ranks on one device: " + (tmp_path / refused[0]).read_text()[:300])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert (tmp_path / "native_ok_0").exists() and (tmp_path / "native_ok_1").exists()

