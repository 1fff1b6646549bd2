"""Validation scoring on integer tokens (mrn_amd/modules/scoring.py, the contract of mrn_greedy_score_f32) against the reference's
per-sample string loop (mrn_amd/test.py::_host_scores = reference test.py:222-260).  No kernel is launched here: `contract` restates
what the kernel computes in plain Python, and every sample it does not hand to the host must score EQUAL (==) to the string loop."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.helpers import load_golden

CHARS = "abcda fghij"            # 'a' twice and a space besides the converters' built-in one: two classes decode to one string


def converter(kind, chars=CHARS):
    from mrn_amd.tools.utils import AttnLabelConverter, CTCLabelConverter
    with contextlib.redirect_stdout(io.StringIO()):
        return CTCLabelConverter(chars) if kind == "ctc" else AttnLabelConverter(chars)


def contract(idx, prob, label, label_len, canon, mode, eos):
    """one sample of mrn_greedy_score_f32 (include/mrn_hip.h) -> (kept tokens, [kept, distance, match, needs_host], confidence)"""
    T = len(idx)
    if mode == 0:
        kept = [t for t in range(T) if idx[t] != 0 and (t == 0 or idx[t] != idx[t - 1])]
        scanned, n_prob = kept, T
    else:
        cut = next((t for t in range(T) if idx[t] == eos), None)
        kept = list(range(T - 1 if cut is None else cut))
        scanned, n_prob = range(T if cut is None else cut), len(kept)
    needs_host = int(any(canon[idx[t]] == -2 for t in scanned))
    tokens = [int(canon[idx[t]]) for t in kept]
    lab = [int(v) for v in label[:label_len]]
    prev = list(range(len(lab) + 1))
    for i, a in enumerate(tokens, 1):
        cur = [i]
        for j, b in enumerate(lab, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a != b)))      # a label token of -1 equals nothing: a is never -1
        prev = cur
    conf = np.float32(0)
    if n_prob:
        conf = np.float32(prob[0])
        for p in prob[1:n_prob]:
            conf = np.float32(conf * np.float32(p))                                   # left to right, rounded to fp32 at every step
    return tokens, [len(tokens), prev[-1], int(prev[-1] == 0), needs_host], conf


def contract_scores(conv, prediction, labels, idx, prob):
    """the batch through `contract` in the form _host_scores gives: per sample (NED term or None, match, confidence), and the flags"""
    from mrn_amd.modules import scoring as S
    from mrn_amd.test import _ned_term
    attn = "Attn" in prediction
    canon = S.canonical_table(conv, prediction)
    width = max((len(w) for w in labels), default=0)
    lab, lab_len = S.canonical_labels(conv, labels, width)
    out, flags = [], []
    for b in range(len(labels)):
        _, (n, dist, match, flag), conf = contract(idx[b], prob[b], lab[b], lab_len[b], canon, int(attn), conv.dict.get("[EOS]", 0))
        out.append((_ned_term(int(lab_len[b]), n, lambda: dist), bool(match), float(conf) if not attn or n else 0))
        flags.append(flag)
    return out, flags


def host_scores(conv, prediction, labels, idx, prob):
    from mrn_amd.test import _host_scores
    strings = conv.decode(idx, [idx.shape[1]] * len(labels))
    return _host_scores(labels, strings, prob, "Attn" in prediction, True)


# ---- the rule module ---------------------------------------------------------------------------------------------------------
def test_canonical_table_and_labels():
    from mrn_amd.modules import scoring as S
    c, a = converter("ctc"), converter("attn")
    # CTC: 0 blank, 1 [PAD], 2 [UNK], 3 ' ', 4 a, 5 b, 6 c, 7 d, 8 a, 9 ' ', 10 f ...: a repeated character keeps its LAST index
    t = S.canonical_table(c, "CTC")
    assert t.dtype == np.int32 and t.shape == (len(c.character),)
    assert t.tolist() == [0, -2, -2, 9, 8, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]
    # attention: 0 [UNK], 1 [PAD], 2 [SOS], 3 [EOS], 4 ' ', 5 a ... 9 a, 10 ' '
    t = S.canonical_table(a, "Attn")
    assert t.tolist() == [-2, -2, -2, 3, 10, 9, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
    for conv, pred in ((c, "CTC"), (a, "Attn")):
        t = S.canonical_table(conv, pred)
        for k, s in enumerate(conv.character):
            if t[k] >= 0 and len(s) == 1:
                assert conv.character[t[k]] == s              # the canonical class decodes to the same string
    lab, n = S.canonical_labels(c, ["a d", "", "bé", "jjjj"], 4)
    assert lab.dtype == np.int32 and n.dtype == np.int32 and n.tolist() == [3, 0, 2, 4]
    assert lab.tolist() == [[8, 9, 7, -1], [-1] * 4, [5, -1, -1, -1], [14] * 4]
    lab, n = S.canonical_labels(a, [], 0)
    assert lab.shape == (0, 0) and n.shape == (0,)
    lab, n = S.canonical_labels(a, ["", ""], 0)
    assert lab.shape == (2, 0) and n.tolist() == [0, 0]
    with pytest.raises(RuntimeError):
        S.canonical_labels(c, ["abc"], 2)


def test_device_scoring_supported(monkeypatch):
    from mrn_amd.modules import scoring as S
    monkeypatch.delenv("MRN_VALIDATION_SCORING", raising=False)
    c, a = converter("ctc"), converter("attn")
    assert S.device_scoring_supported(c, "CTC", 63, 25) and S.device_scoring_supported(a, "Attn", 26, 25)
    assert S.device_scoring_supported(c, "CTC", 1, 0) and S.device_scoring_supported(c, "CTC", 512, 256)
    assert not S.device_scoring_supported(c, "CTC", 513, 25) and not S.device_scoring_supported(c, "CTC", 0, 25)
    assert not S.device_scoring_supported(c, "CTC", 63, 257) and not S.device_scoring_supported(a, "Attn", 513, 25)
    # a character set that can spell "[EOS]": the reference cuts at the STRING, so the attention head stays on the host; CTC does not cut
    spell = "[]EOSab"
    assert not S.device_scoring_supported(converter("attn", spell), "Attn", 26, 25)
    assert S.device_scoring_supported(converter("ctc", spell), "CTC", 63, 25)
    assert S.device_scoring_supported(converter("attn", "[]EOab"), "Attn", 26, 25)      # no 'S': cannot spell it
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "host")
    assert not S.device_scoring_supported(c, "CTC", 63, 25) and not S.device_scoring_supported(a, "Attn", 26, 25)
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "device")
    assert S.device_scoring_supported(c, "CTC", 63, 25)
    monkeypatch.setenv("MRN_VALIDATION_SCORING", "gpu")
    with pytest.raises(ValueError):
        S.device_scoring_supported(c, "CTC", 63, 25)


# ---- the contract against the string loop ------------------------------------------------------------------------------------
def assert_equal_where_not_flagged(got, flags, want, what):
    assert len(got) == len(want) == len(flags)
    for b, (g, w, f) in enumerate(zip(got, want, flags)):
        if not f:
            assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2], (what, b, g, w)


def greedy(logits):
    """preds.max(2) and softmax(preds, 2).max(2) (reference test.py:211,218-219) on the host"""
    lg = torch.from_numpy(np.asarray(logits))
    return lg.max(2)[1].numpy(), torch.softmax(lg, 2).max(2)[0].numpy()


@pytest.mark.parametrize("kind", ["ctc", "attn"])
def test_contract_replays_the_reference_fixture(kind):
    """scoring.npz (reference validation() on crafted logits): the token contract, with the string loop for the flagged rows only,
    reproduces the reference's accuracy and normalised edit distance; exactly the rows that predict [UNK] / [PAD] where it counts are
    flagged"""
    g = load_golden("scoring")
    conv = converter(kind, str(g[f"{kind}/chars"]))
    prediction = "CTC" if kind == "ctc" else "Attn"
    n_correct, norm_ed, n = 0, 0.0, 0
    flagged_rows = []
    for i in range(int(g[f"{kind}/n_batches"])):
        labels = [str(s) for s in g[f"{kind}/batch{i}/labels"]]
        idx, prob = greedy(g[f"{kind}/batch{i}/logits"])
        got, flags = contract_scores(conv, prediction, labels, idx, prob)
        want = host_scores(conv, prediction, labels, idx, prob)
        assert_equal_where_not_flagged(got, flags, want, f"{kind} batch {i}")
        flagged_rows.append([b for b, f in enumerate(flags) if f])
        for b in range(len(labels)):
            term, correct, _ = want[b] if flags[b] else got[b]
            norm_ed += term if term is not None else 0
            n_correct += bool(correct)
        n += len(labels)
    assert flagged_rows == ([[5], [3]] if kind == "ctc" else [[4], [1, 2]])
    assert abs(n_correct / n * 100 - float(g[f"{kind}/accuracy"])) < 1e-9 and abs(norm_ed / n * 100 - float(g[f"{kind}/ned"])) < 1e-9


def fuzz_batch(rng, conv, kind, T, n, specials):
    """n samples: random rows, rows near the label, out-of-dictionary label characters, duplicate characters, with and without [EOS];
    `specials` lets [PAD] / [UNK] / [SOS] into the predictions -> (labels, idx [n,T], prob [n,T])"""
    C = len(conv.character)
    attn = kind == "attn"
    special = [0, 1, 2] if attn else [1, 2]
    singles = [k for k, s in enumerate(conv.character) if len(s) == 1]
    eos = conv.dict["[EOS]"] if attn else None
    pool = singles + (special if specials else [])
    alphabet = list(CHARS) + ["é", "Z"]
    labels, rows = [], []
    for _ in range(n):
        L = int(rng.integers(0, min(T, 25) + 1))
        label = "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=L))
        tok = [int(rng.choice([k for k in singles if conv.character[k] == ch])) if ch in conv.dict else int(rng.choice(pool)) for ch in label]
        mode = int(rng.integers(0, 4))
        if mode == 0:                                            # random row
            row = [int(v) for v in rng.choice(pool + ([eos] if attn else [0]), size=T)]
        else:
            if mode >= 2 and tok:                                # near the label: substitute / delete / insert
                for _e in range(int(rng.integers(1, 3))):
                    p = int(rng.integers(0, len(tok)))
                    op = int(rng.integers(0, 3))
                    if op == 0:
                        tok[p] = int(rng.choice(pool))
                    elif op == 1:
                        del tok[p]
                    else:
                        tok.insert(p, int(rng.choice(pool)))
                    if not tok:
                        break
            if attn:
                tail = int(rng.choice(pool))
                row = (tok + ([eos] if rng.integers(0, 4) else []) + [tail] * T)[:T]
            else:
                row = []
                for t in tok:
                    if row and row[-1] == t or rng.integers(0, 3) == 0:
                        row.append(0)
                    row += [t] * int(rng.integers(1, 3))
                row = (row + [0] * T)[:T]
        labels.append(label)
        rows.append(row)
    return labels, np.array(rows, dtype=np.int64), rng.uniform(0.5, 1.0, size=(n, T)).astype(np.float32)


@pytest.mark.parametrize("kind", ["ctc", "attn"])
@pytest.mark.parametrize("T", [1, 2, 5, 26, 63, 65, 70])
def test_contract_equals_the_string_loop_on_a_seeded_fuzz(kind, T):
    conv = converter(kind)
    prediction = "CTC" if kind == "ctc" else "Attn"
    rng = np.random.default_rng(1000 * T + (kind == "attn"))
    # without special tokens nothing may go to the host: the fallback cannot hide a wrong rule
    labels, idx, prob = fuzz_batch(rng, conv, kind, T, 120, specials=False)
    got, flags = contract_scores(conv, prediction, labels, idx, prob)
    assert not any(flags)
    assert_equal_where_not_flagged(got, flags, host_scores(conv, prediction, labels, idx, prob), f"{kind} T={T} plain")
    labels, idx, prob = fuzz_batch(rng, conv, kind, T, 120, specials=True)
    got, flags = contract_scores(conv, prediction, labels, idx, prob)
    assert_equal_where_not_flagged(got, flags, host_scores(conv, prediction, labels, idx, prob), f"{kind} T={T} specials")
    assert sum(flags) < len(flags)                                # some rows with specials in reach still score on tokens
