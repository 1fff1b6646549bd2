"""The herding kernels (csrc/herding.hip, include/mrn_herding.h) through ops.herding_features / ops.herding_select, and the learners
that use them.  The yardsticks are mrn_amd/modules/herding.py::herding_host and features_host in float64 (held to the definition by
tests/test_herding_cpu.py) and a float64 replay of the kernel's own picks; never the code under test.

Exact cases: tables of integers -2 ... 2 with N a power of two make every quantity exact in fp32 and float64 under any summation order
(test_herding_cpu.py checks that claim with an fp32 emulation), so picks must equal herding_host's element for element and dist exactly.
Their shapes: D = 4 (one lane per row), 8, 132 (33 chunks of 16 bytes on 64 lanes: a ragged lane group), 512 (two chunks per lane) and
8192 (the limit); N = 1, 2 (less than one pass of a wave), 16 and 32 (one whole workgroup), 64 (two), 256, 1024 and 4096 (many); m = 1,
N / 2 and N.  The
reference of a table is computed once, for m = N: a prefix of it is the reference of a smaller m (test_herding_cpu.py).

Real-valued case: the kernel's picks are replayed in float64; at every step the picked row's objective may exceed the minimum over the
unpicked rows by at most tau_k = 4 (D + 4) 2^-24 (max ||f||^2 + max ||f|| ||r_k||), the worst case of one fp32 dot product, of the fp32
norms and of the rounding of r -- derived, not measured.  N = 700 and 3000 leave a ragged last workgroup."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_close
from tests.test_herding_cpu import U32, duplicated_table, integer_table, replay, unit_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


@functools.lru_cache(maxsize=None)
def exact_reference(kind, N, D):
    """(table, herding_host(table, N)) -- computed once per table, never written to"""
    from mrn_amd.modules.herding import herding_host
    F = integer_table(1000 * D + N, N, D) if kind == "random" else duplicated_table(1000 * D + N, N, D)
    picks, dist = herding_host(F, N)
    for a in (F, picks, dist):
        a.setflags(write=False)
    return F, picks, dist


def check_exact(ops, kind, N, D):
    F, picks, dist = exact_reference(kind, N, D)
    dev = torch.tensor(F, device="cuda")                                # (a copy: the cached table is read-only)
    for m in sorted({1, max(N // 2, 1), N}):
        got_p, got_d = ops.herding_select(dev, m)
        assert got_p.is_cuda and got_p.dtype == torch.int64 and got_d.dtype == torch.float32 and got_p.shape == got_d.shape == (m,)
        p, d = got_p.cpu().numpy(), got_d.cpu().numpy().astype(np.float64)
        wrong = np.nonzero(p != picks[:m])[0]
        assert wrong.size == 0, (N, D, m, "first difference at step", int(wrong[0]), int(p[wrong[0]]), int(picks[wrong[0]]))
        assert np.array_equal(d, dist[:m]), (N, D, m)
    again_p, again_d = ops.herding_select(dev, N)                       # determinism: the same bits
    assert torch.equal(again_p, got_p) and torch.equal(again_d, got_d)


@pytest.mark.parametrize("N,D", [(1, 4), (2, 4), (64, 4), (256, 4), (1024, 4), (4096, 4),
                                 (2, 8), (32, 8), (64, 8), (4096, 8),
                                 (1, 132), (16, 132), (256, 132), (1024, 132), (4096, 132),
                                 (2, 512), (64, 512), (1024, 512),
                                 (1, 8192), (64, 8192), (256, 8192)])
def test_integer_tables_are_selected_exactly(ops, N, D):
    check_exact(ops, "random", N, D)


@pytest.mark.parametrize("N,D", [(256, 8), (1024, 4), (512, 132)])
def test_ties_go_to_the_lower_row_across_workgroups(ops, N, D):
    """every row occurs twice, the copies N / 2 rows apart, that is in different workgroups: the lower copy first"""
    check_exact(ops, "duplicated", N, D)
    F, picks, _ = exact_reference("duplicated", N, D)
    at = np.empty(N, dtype=np.int64)
    at[picks] = np.arange(N)
    assert (at[:N // 2] < at[N // 2:]).all()


@pytest.mark.parametrize("N,D,m", [(700, 128, 200), (3000, 512, 300)])
def test_real_valued_tables_pass_the_float64_replay(ops, N, D, m):
    F = unit_table(N + D, N, D)
    dev = torch.from_numpy(F).cuda()
    picks, dist = ops.herding_select(dev, m)
    again = ops.herding_select(dev, m)
    assert torch.equal(picks, again[0]) and torch.equal(dist, again[1])
    p = picks.cpu().numpy()
    assert len(set(p.tolist())) == m
    excess, tau, objective = replay(F, p)
    off = np.abs(dist.cpu().numpy().astype(np.float64) - objective)
    print(f"N {N} D {D} m {m}: max excess / tau {np.max(excess / tau):.3e}, max |dist - objective| / tau {np.max(off / tau):.3e}, "
          f"tau {tau.min():.2e} ... {tau.max():.2e}")
    assert (excess <= tau).all(), (int(np.argmax(excess / tau)), float(np.max(excess / tau)))
    assert (off <= tau).all()                                            # (half of tau is the bound of one row's d)


@pytest.mark.parametrize("D", [128, 512])
def test_features_against_the_host_form(ops, D):
    from mrn_amd.modules.herding import features_host
    rng = np.random.default_rng(D)
    for B in (1, 5, 33):
        for T in (1, 31, 65):
            x = (rng.standard_normal((B, T, D)) + 0.5 * rng.standard_normal((1, 1, D))).astype(np.float32)
            got = ops.herding_features(torch.from_numpy(x).cuda())
            assert got.is_cuda and got.shape == (B, D) and got.dtype == torch.float32
            err = np.abs(got.cpu().numpy().astype(np.float64) - features_host(x)).max()
            print(f"B {B} T {T} D {D}: max error {err:.3e}, bound {(T + D + 8) * U32:.3e}")
            assert err <= (T + D + 8) * U32, (B, T, err)
    # a batch stride and a time stride that are not the dense ones, rows row0 ... row0 + B of a larger table, an all-zero sample
    big = (rng.standard_normal((10, 14, D)) + 0.3).astype(np.float32)
    big[4] = 0
    dev = torch.from_numpy(big).cuda()
    view = dev[::2, 1::3]                                                # samples 0, 2, 4, 6, 8; frames 1, 4, 7, 10, 13
    assert not view.is_contiguous() and view.stride(2) == 1
    table = torch.full((12, D), 7.0, device="cuda")
    out = ops.herding_features(view, out=table, row0=3)
    assert out is table and (table[:3] == 7).all() and (table[8:] == 7).all()
    ref = features_host(big[::2, 1::3])
    assert np.abs(table[3:8].cpu().numpy().astype(np.float64) - ref).max() <= (5 + D + 8) * U32
    assert (table[5] == 0).all() and (ref[2] == 0).all()
    with pytest.raises(ValueError, match="out must be"):
        ops.herding_features(view, out=table, row0=8)


def test_a_violated_limit_is_an_error_and_launches_nothing(ops):
    from mrn_amd._lib import LIB, call
    from mrn_amd.modules.herding import herding_host
    N, D, m = 40, 8, 5
    F = unit_table(3, N, D)
    dev = torch.from_numpy(F).cuda()
    big = torch.zeros(N * 8196, device="cuda")                            # (room for every D tried below)
    big[:N * D] = dev.reshape(-1)
    picks = torch.full((N + 1,), 7, dtype=torch.int32, device="cuda")
    dist = torch.full((N + 1,), 7.0, device="cuda")
    need = LIB.load().mrn_herding_select_work_bytes(N, 8192)
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def select(**kw):
        a = dict(F=big.data_ptr(), N=N, D=D, m=m, picks=picks.data_ptr(), dist=dist.data_ptr(), work=work.data_ptr(), work_bytes=need)
        a.update(kw)
        call("mrn_herding_select_f32", *a.values(), ops._stream())

    for kw, match in ((dict(m=N + 1), "m = 41"), (dict(m=0), "m = 0"), (dict(D=6), "D = 6"), (dict(D=8196), "D = 8196"), (dict(D=0), "D = 0"),
                      (dict(N=0), "N = 0"), (dict(N=(1 << 24) + 1), "rows"), (dict(F=None), "bad operands"), (dict(picks=None), "bad operands"),
                      (dict(dist=None), "bad operands"), (dict(work=None), "bad operands"), (dict(work_bytes=64), "workspace")):
        with pytest.raises(RuntimeError, match=match):
            select(**kw)
    feat = torch.ones(3, 4, D, device="cuda")
    table = torch.full((N, D), 7.0, device="cuda")

    def features(**kw):
        a = dict(feat=feat.data_ptr(), B=3, T=4, D=D, batch_stride=4 * D, time_stride=D, F=table.data_ptr(), N=N, row0=0)
        a.update(kw)
        call("mrn_herding_features_f32", *a.values(), ops._stream())

    for kw, match in ((dict(D=6), "D = 6"), (dict(D=8196), "D = 8196"), (dict(T=0), "T = 0"), (dict(B=-1), "B = -1"), (dict(row0=N - 2), "outside a table"),
                      (dict(row0=-1), "outside a table"), (dict(batch_stride=-1), "negative"), (dict(feat=None), "bad operands"),
                      (dict(F=None), "bad operands")):
        with pytest.raises(RuntimeError, match=match):
            features(**kw)
    torch.cuda.synchronize()
    assert (picks == 7).all() and (dist == 7).all() and (work == 0).all() and (table == 7).all()         # nothing was launched
    select()                                                                                             # the same operands within the limits
    ref = herding_host(F, m)
    assert np.array_equal(picks[:m].cpu().numpy(), ref[0]) and (picks[m:] == 7).all() and (dist[m:] == 7).all()
    # the op refuses what the kernel would, before any launch; CPU tensors take the host form
    for bad in (torch.zeros(4, 6, device="cuda"), torch.zeros(4, 8196, device="cuda")):
        with pytest.raises(ValueError, match="D % 4"):
            ops.herding_select(bad, 2)
    with pytest.raises(ValueError, match="outside 1"):
        ops.herding_select(dev, N + 1)
    poisoned = dev.clone()
    poisoned[7, 3] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        ops.herding_select(poisoned, 2)
    host = ops.herding_select(torch.from_numpy(F), m)
    assert not host[0].is_cuda and np.array_equal(host[0].numpy(), ref[0])


# ---- the learners, end to end ------------------------------------------------------------------------------------------------------
def run_two_tasks(tmp_path, monkeypatch, il, memory, seed=3, start_task=0):
    """two tasks of tiny_train.train() on the tiny in-memory datasets of tests/test_learner_gpu.py (a CRNN, memory_num = 20) -> (learner,
    data manager, log, what the herding ops were handed)"""
    from torch.utils.data import ConcatDataset
    from mrn_amd import ops, tiny_train
    from mrn_amd.data.data_manage import Dataset_Manager, Val_Dataset
    from mrn_amd.data.dataset import ArrayDataset
    from tests.helpers import fake_text_samples
    from tests.test_learner_gpu import make_opt
    os.chdir(tmp_path)
    opt = make_opt(tmp_path, "crnn")
    opt.__dict__.update(il=il, memory=memory, exp_name=f"h_{il}_{memory}", select_data=["rootA"], valid_datas=["valA"], Aug="None", memory_num=20,
                        batch_size=6, num_iter=4, val_interval=2, start_task=start_task)

    def open_fake(path, o, mode="train"):
        images, labels = fake_text_samples(path)
        return ArrayDataset(images, labels, o, mode)

    np.random.seed(seed)
    torch.manual_seed(seed)
    dm = Dataset_Manager(opt, open_dataset=open_fake)
    valid = Val_Dataset(["valA/A", "valA/B"], opt, open_tree=lambda root, o, mode: (ConcatDataset([open_fake(root, o, mode)]), "log"))
    alphabet = {0: "abcdefghijklmnopqrstuvwxyz", 1: "abcdefghijklmnopqrstuvwxyzAB"}
    seen = dict(feats=[], tables=[], picks=[], recomputed=[], state=None)
    real_features, real_select = ops.herding_features, ops.herding_select
    holder = {}

    def spy_features(feat, out=None, row0=0):
        seen["feats"].append((row0, feat.detach().clone()))
        return real_features(feat, out=out, row0=row0)

    def spy_select(F, m):
        # the weights are still those the table was made with: the features once more through the learner's hook, in eval mode
        learner = holder["learner"]
        taski = len(learner.memory_index) + 1
        loader, n = dm.rehearsal_prev_model(taski)
        modes = [(mod, mod.training) for mod in learner.model.modules()]
        learner.model.eval()
        with torch.no_grad():
            again = torch.cat([learner.herding_feature(image.to(learner.device), taski).float() for image, _ in loader], 0)
        for mod, training in modes:
            mod.training = training
        seen["recomputed"].append((taski, n, again))
        seen["tables"].append(F.detach().clone())
        picks, dist = real_select(F, m)
        seen["picks"].append(picks.cpu().numpy().copy())
        return picks, dist

    monkeypatch.setattr(ops, "herding_features", spy_features)
    monkeypatch.setattr(ops, "herding_select", spy_select)
    real_make = tiny_train.make_learner

    def make(o):
        holder["learner"] = real_make(o)
        return holder["learner"]
    monkeypatch.setattr(tiny_train, "make_learner", make)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        learner, best, ned = tiny_train.train(opt, io.StringIO(), data=(dm, valid, lambda t: alphabet[t], lambda t: [valid.create_dataset("valA/A")]))
    assert len(best) == 2 and all(torch.isfinite(p).all() for p in learner.model.parameters())
    return learner, dm, sink.getvalue(), seen


@pytest.mark.parametrize("il", ["base", "der", "mrn"])
def test_learners_select_their_memory_by_herding(tmp_path, monkeypatch, il):
    from mrn_amd.modules.herding import features_host
    learner, dm, log, seen = run_two_tasks(tmp_path, monkeypatch, il, "herding")
    assert type(learner).__name__ == {"base": "BaseLearner", "der": "DER", "mrn": "MRN"}[il]
    assert len(seen["tables"]) == 1 and len(learner.memory_index) == 1
    taski, n, again = seen["recomputed"][0]
    table = seen["tables"][0]
    index = learner.memory_index[0]
    assert taski == 1 and isinstance(index, np.ndarray) and index.dtype.kind == "i"
    assert len(index) == 20 and len(set(index.tolist())) == 20 and index.min() >= 0 and index.max() < n
    assert np.array_equal(index, seen["picks"][0])                       # in pick order, as the op returned them
    # the table: the ordered pass over the previous task's data, the hook's feature of the network as task 0 left it
    feats = torch.cat([f for _, f in seen["feats"]], 0)
    assert [r for r, _ in seen["feats"]] == list(np.cumsum([0] + [f.shape[0] for _, f in seen["feats"]][:-1]))
    hidden = learner.opt.hidden_size
    assert tuple(table.shape) == (n, hidden * taski) and feats.shape[0] == n and feats.shape[2] == hidden * taski
    assert_close(f"{il}: the hook's features", again, feats)
    net = learner.model
    T = feats.shape[1]
    ref = features_host(feats.cpu().numpy())
    err = np.abs(table.cpu().numpy().astype(np.float64) - ref).max()
    print(f"{il}: table [{n}, {table.shape[1]}], T = {T}, max feature error {err:.3e}, bound {(T + table.shape[1] + 8) * U32:.3e}")
    assert err <= (T + table.shape[1] + 8) * U32
    # the replay criterion on the table the selection was made on
    excess, tau, _ = replay(table.cpu().numpy(), index)
    print(f"{il}: max excess / tau {np.max(excess / tau):.3e}")
    assert (excess <= tau).all()
    # the second task trained on the mixed loader
    assert learner.opt_step > 0 and "Is using rehearsal memory, has 1 prev datasets, each has 20" in log
    if il == "mrn":
        assert "Train_taski_loss" in log and len(net.model) == 2
    if il == "der":
        assert len(net.model) == 2


def test_the_feature_hooks_of_the_three_learners(tmp_path, monkeypatch):
    """the hook of the MRN learner at task 1 is expert 0's extractor, DER's the first extractor alone, the base learner's its only one"""
    from mrn_amd.il_modules.base import BaseLearner
    from mrn_amd.il_modules.der import DER
    from mrn_amd.il_modules.mrn import MRN
    from tests.test_learner_gpu import make_opt
    image = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (3, 4, 32, 256)).astype(np.float32)).cuda()
    torch.manual_seed(1)
    for cls in (BaseLearner, DER, MRN):
        opt = make_opt(tmp_path, "crnn")
        with contextlib.redirect_stdout(io.StringIO()):
            learner = cls(opt)
            learner.character = "abcdefghij"
            learner.converter = learner.build_converter()
            learner.build_model()
            learner.character = "abcdefghijklmno"
            learner.converter = learner.build_converter()
            learner.change_model()
        learner.model.eval()
        net = learner.model.module
        with torch.no_grad():
            if cls is not BaseLearner:                                   # (DER starts a new extractor from the previous one's weights)
                for p in (net.model[1] if cls is DER else net.model[1].model).parameters():
                    p.mul_(1.25)
            got = learner.herding_feature(image, 1)
            want = {BaseLearner: lambda: net.model(image), DER: lambda: net.model[0](image), MRN: lambda: net.model[0].model(image)}[cls]()
            assert got.shape == (3, want.shape[1], opt.hidden_size) and torch.equal(got, want)
            if cls is not BaseLearner:
                newest = net.model[1](image) if cls is DER else net.model[1].model(image)
                assert not torch.equal(got, newest)
        learner.model.train()


@pytest.mark.parametrize("il", ["base", "mrn"])
def test_a_resumed_run_selects_the_same_memory(tmp_path, monkeypatch, il):
    """opt.start_task = 2: both tasks skip training and load their checkpoints; the selection of task 1 is made on the weights the
    trained run made it on (incremental_train / MRN._train call load_task_data before the checkpoint that would replace them), so the
    table and the picks are the same, bit for bit"""
    trained = run_two_tasks(tmp_path, monkeypatch, il, "herding")
    resumed = run_two_tasks(tmp_path, monkeypatch, il, "herding", start_task=2)
    assert resumed[0].opt_step == 0                                       # nothing was trained
    assert torch.equal(trained[3]["tables"][0], resumed[3]["tables"][0])
    assert np.array_equal(trained[0].memory_index[0], resumed[0].memory_index[0])


def test_random_memory_draws_what_it_drew_before(tmp_path, monkeypatch):
    """memory="random" in a process that has used the herding ops: the index list is the first draw of numpy's global stream after the
    seed, np.random.choice(range(len(previous dataset)), 20, replace=False), as build_random_current_memory has always made it; the
    herding ops are not called"""
    from mrn_amd import ops
    ops.herding_select(torch.from_numpy(unit_table(1, 50, 8)).cuda(), 5)
    learner, dm, log, seen = run_two_tasks(tmp_path, monkeypatch, "base", "random", seed=3)
    assert not seen["tables"] and not seen["feats"]
    n = dm.rehearsal_prev_model(1)[1]
    assert len(learner.memory_index) == 1
    assert np.array_equal(learner.memory_index[0], np.random.RandomState(3).choice(range(n), 20, replace=False))
