"""mrn_greedy_score_f32 (mrn_amd/csrc/score.hip) against the Python restatement of its contract (tests/test_scoring_cpu.py::contract),
and validation() through the device scorer against the reference's recorded returns (tests/golden/scoring.npz) and against its own
host path."""
import contextlib

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.test_scoring_cpu import contract, converter

pytestmark = pytest.mark.gpu

LABEL_LENGTHS = [0, 1, 63, 64, 65, 255, 256]


def run_kernel(idx, prob, label, label_len, canon, mode, eos):
    from mrn_amd import ops
    dev = torch.device("cuda")
    tokens, result, conf, _ = ops.greedy_score(torch.from_numpy(idx).to(dev), torch.from_numpy(prob).to(dev), torch.from_numpy(label).to(dev),
                                               torch.from_numpy(label_len).to(dev), torch.from_numpy(canon).to(dev), mode, eos)
    torch.cuda.synchronize()
    return tokens.cpu().numpy(), result.cpu().numpy(), conf.cpu().numpy()


def kernel_rows(kind, T, rng):
    """(prediction row [T], label tokens) pairs: per label length the row kinds at which the kernel can go wrong"""
    from mrn_amd.modules import scoring as S
    conv = converter(kind)
    canon = S.canonical_table(conv, "CTC" if kind == "ctc" else "Attn")
    attn = kind == "attn"
    eos = conv.dict["[EOS]"] if attn else 0
    singles = [k for k in range(len(canon)) if canon[k] >= 0 and k != eos and (attn or k != 0)]
    special = 1                                                        # [PAD] on both heads: canon -2

    def ctc_frames(tok):                                              # one frame per token, a blank where two equal classes meet
        row = []
        for t in tok:
            if row and row[-1] == t:
                row.append(0)
            row.append(t)
        return (row + [0] * T)[:T]

    def attn_frames(tok, tail=None):                                  # tokens, [EOS], filler
        return (list(tok) + [eos] + [singles[0] if tail is None else tail] * T)[:T]
    frames = attn_frames if attn else ctc_frames
    cases = []
    for L in LABEL_LENGTHS:
        cls = [int(v) for v in rng.choice(singles, size=L)]           # the classes that would predict the label
        label = [int(canon[k]) for k in cls]
        cases.append((frames(cls), label))                            # equal to the label (cut short where T cannot hold it)
        cases.append(([eos] * T if attn else [0] * T, label))         # [EOS] at 0 / all blank: nothing kept
        cases.append(([singles[1]] * T, label))                       # no [EOS] at all / one class repeated (collapses to one token)
        for K in (63, 65):                                            # prediction shorter / longer than the label on either side of 64
            other = [int(v) for v in rng.choice(singles, size=K)]
            other[:min(K, L) // 2] = cls[:min(K, L) // 2]
            cases.append((frames(other), label))
        if L:
            holed = list(label)
            holed[L // 2] = -1                                        # a label character outside the dictionary
            cases.append((frames(cls), holed))
        cases.append((frames(cls[:3] + [special] + cls[3:]), label))  # a multi-character token before the cut: flagged
        if attn:
            cases.append((attn_frames(cls[:max(T - 1, 0)][:L], tail=special), label))     # ... only after the cut: not flagged
            cases.append((([singles[2]] * T)[:T - 1] + [eos], label))                     # [EOS] at T - 1
    return conv, canon, eos, cases


@pytest.mark.parametrize("kind", ["ctc", "attn"])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 129, 512])
def test_kernel_equals_the_contract(kind, T):
    """every integer output equal, the confidence equal on its float32 bits (probabilities in [0.75, 1): every partial product is a
    normal number); launches of B = 5 and B = 1 (not multiples of the four samples per block), label widths on both sides of 64"""
    rng = np.random.default_rng(17 * T + (kind == "attn"))
    conv, canon, eos, cases = kernel_rows(kind, T, rng)
    mode = int(kind == "attn")
    start, sizes, launch = 0, [5, 1], 0
    seen_flag, seen_plain = False, False
    while start < len(cases):
        chunk = cases[start:start + sizes[launch % 2]]
        start += len(chunk)
        launch += 1
        B = len(chunk)
        Lmax = max(len(lab) for _, lab in chunk)
        idx = np.array([row for row, _ in chunk], dtype=np.int64).reshape(B, T)
        prob = rng.uniform(0.75, 1.0, size=(B, T)).astype(np.float32)
        label = np.full((B, Lmax), -1, dtype=np.int32)
        for b, (_, lab) in enumerate(chunk):
            label[b, :len(lab)] = lab
        label_len = np.array([len(lab) for _, lab in chunk], dtype=np.int32)
        tokens, result, conf = run_kernel(idx, prob, label, label_len, canon, mode, eos)
        for b in range(B):
            want_tok, want_res, want_conf = contract(idx[b], prob[b], label[b], label_len[b], canon, mode, eos)
            assert result[b, 3] == want_res[3], (T, start, b, result[b], want_res)
            if want_res[3]:
                seen_flag = True
                continue                                               # flagged: the other outputs are unspecified
            seen_plain = True
            assert result[b].tolist() == want_res, (T, start, b, result[b], want_res)
            assert tokens[b, :want_res[0]].tolist() == want_tok and (tokens[b, want_res[0]:] == -1).all()
            assert conf[b].view(np.uint32) == np.float32(want_conf).view(np.uint32), (T, start, b, conf[b], want_conf)
    assert seen_plain and seen_flag


@pytest.mark.parametrize("kind", ["ctc", "attn"])
def test_confidence_that_underflows(kind):
    """probabilities in (0, 0.1) at T = 129: the product leaves the normal range; only the band tests/test_validation_gpu.py uses is
    asserted (subnormal handling is the compiler's)"""
    from mrn_amd.modules import scoring as S
    T, B = 129, 3
    conv = converter(kind)
    canon = S.canonical_table(conv, "CTC" if kind == "ctc" else "Attn")
    rng = np.random.default_rng(5)
    idx = np.full((B, T), 5, dtype=np.int64)                          # no blank, no [EOS]: all T (CTC) / T - 1 (attention) factors
    prob = rng.uniform(1e-3, 0.1, size=(B, T)).astype(np.float32)
    label = np.full((B, 1), 5, dtype=np.int32)
    _, result, conf = run_kernel(idx, prob, label, np.ones(B, dtype=np.int32), canon, int(kind == "attn"), conv.dict.get("[EOS]", 0))
    for b in range(B):
        want = contract(idx[b], prob[b], label[b], 1, canon, int(kind == "attn"), conv.dict.get("[EOS]", 0))[2]
        assert abs(float(conf[b]) - float(want)) <= 1e-37


def test_bad_limits_are_errors():
    conv = converter("ctc")
    from mrn_amd.modules import scoring as S
    canon = S.canonical_table(conv, "CTC")
    one = np.ones((1, 1), dtype=np.int32)
    with pytest.raises(RuntimeError, match="mrn_greedy_score_f32"):
        run_kernel(np.ones((1, 513), dtype=np.int64), np.ones((1, 513), dtype=np.float32), one, one[0], canon, 0, 0)
    with pytest.raises(RuntimeError, match="mrn_greedy_score_f32"):
        run_kernel(np.ones((1, 4), dtype=np.int64), np.ones((1, 4), dtype=np.float32), np.ones((1, 257), dtype=np.int32), one[0], canon, 0, 0)


# ---- validation() end to end ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recorded_calls():
    """names of every C-ABI call made inside the block"""
    from mrn_amd import _lib
    log, real = [], _lib.LIB.call

    def spy(name, *a):
        log.append(name)
        return real(name, *a)
    _lib.LIB.call = spy
    try:
        yield log
    finally:
        del _lib.LIB.call           # (the instance attribute: the class's method is back)


def fixture_case(kind):
    from tests.test_validation_gpu import converter_and_criterion, make_opt
    g = load_golden("scoring")
    vkind = "crnn" if kind == "ctc" else "trba"
    conv, crit = converter_and_criterion(vkind, str(g[f"{kind}/chars"]))
    opt = make_opt(vkind)
    opt.batch_max_length = int(g[f"{kind}/batch_max_length"])
    n = int(g[f"{kind}/n_batches"])
    logits = [torch.from_numpy(g[f"{kind}/batch{i}/logits"]) for i in range(n)]
    batches = [(torch.zeros(len(g[f"{kind}/batch{i}/labels"]), 4, 32, 256), [str(s) for s in g[f"{kind}/batch{i}/labels"]]) for i in range(n)]
    return g, conv, crit, opt, batches, logits


def run_validation(conv, crit, opt, batches, logits):
    from mrn_amd.test import validation
    calls = iter(logits)
    with recorded_calls() as log:
        res = validation(lambda image, *a, **k: {"predict": next(calls).cuda(), "feature": None}, crit, batches, conv, opt)
    return res, log.count("mrn_greedy_score_f32")


@pytest.mark.parametrize("kind", ["ctc", "attn"])
def test_validation_on_the_device_vs_reference_and_vs_the_host_path(kind, monkeypatch):
    from tests.test_validation_gpu import check
    g, conv, crit, opt, batches, logits = fixture_case(kind)
    monkeypatch.delenv("MRN_VALIDATION_SCORING", raising=False)
    dev, launches = run_validation(conv, crit, opt, batches, logits)
    assert launches == len(batches)                                   # one launch per batch
    check(g, f"{kind}/", dev)
    assert [str(s) for s in dev[5]] == [str(s) for s in g[f"{kind}/labels_last_batch"]]
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "host")
    host, launches = run_validation(conv, crit, opt, batches, logits)
    assert launches == 0                                              # the host path never launches it
    for i in (0, 1, 2, 3, 4, 5, 7):                                   # all but infer_time; floats with ==
        assert dev[i] == host[i], (i, dev[i], host[i])
    assert [type(c) for c in dev[4]] == [type(c) for c in host[4]]
    monkeypatch.delenv("MRN_VALIDATION_SCORING")
    for i in range(len(batches)):                                     # every batch as the last one: its strings and confidences
        one, _ = run_validation(conv, crit, opt, [batches[i]], [logits[i]])
        check(g, f"{kind}/batch{i}/", one)
    opt.NED = False
    assert run_validation(conv, crit, opt, batches, logits)[0][2] is None


def test_validation_beyond_the_kernel_limits_stays_on_the_host(monkeypatch):
    """T = 513 decoding steps: one more than the kernel takes -- scored by the host loop, the kernel is never called"""
    from tests.test_validation_gpu import converter_and_criterion, make_opt
    monkeypatch.delenv("MRN_VALIDATION_SCORING", raising=False)
    conv, crit = converter_and_criterion("trba", "abcdefgh")
    opt = make_opt("trba")
    opt.batch_max_length = 512
    T, C = 513, len(conv.character)
    labels = ["abc", "hgf"]
    rows = torch.full((2, T), conv.dict["[EOS]"], dtype=torch.long)
    rows[0, :3] = torch.tensor([conv.dict[c] for c in "abc"])
    rows[1, :3] = torch.tensor([conv.dict[c] for c in "hgd"])
    lg = torch.zeros(2, T, C).scatter_(2, rows.unsqueeze(2), 4.0)
    res, launches = run_validation(conv, crit, opt, [(torch.zeros(2, 4, 32, 256), labels)], [lg])
    assert launches == 0
    assert res[1] == 50.0 and abs(res[2] - (1 + 2 / 3) / 2 * 100) < 1e-9 and [s[:8] for s in res[3]] == ["abc[EOS]", "hgd[EOS]"]
    # the same rows at T = 512 go through the kernel and score the same
    opt.batch_max_length = 511
    res2, launches = run_validation(conv, crit, opt, [(torch.zeros(2, 4, 32, 256), labels)], [lg[:, :512].contiguous()])
    assert launches == 1 and res2[1] == res[1] and res2[2] == res[2] and res2[4][0] == res[4][0]
