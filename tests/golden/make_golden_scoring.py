"""Golden vectors for the validation scorer (mrn_greedy_score_f32 behind mrn_amd/test.py::validation), produced by running the
REFERENCE's validation() (test.py:139-279) on CPU with stub models that return fixed logits.

Run in the build container only (the reference never travels to the GPU box):
    python tests/golden/make_golden_scoring.py
Writes tests/golden/scoring.npz: per case the logits, the labels, the character set and the reference's eight return values.  The
import shims (nltk's edit_distance as a plain Levenshtein, mmcv, lmdb, ...) are those of make_golden_il.py.

What tests/helpers.py::crafted_validation_case does not reach, and these cases do:
  * a character set with a repeated character and a space (two classes decode to the same string);
  * CTC at T = 127 with labels of 64, 65 and 100 characters (batch_max_length 100), rows that collapse across the 64th kept token;
  * attention at T = 129 with [EOS] at 0, at 64, at T - 1 and absent;
  * a [UNK] / [PAD] prediction before [EOS] (scored on the host) and after it (must stay on the device);
  * an empty label.
The logits are multiples of 1/8 (exact in fp32, so the file compresses) with +4 on the wanted class.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_il as G  # noqa: E402  (reference import shims; imports the reference's test.py as ref_test)

from mrn_amd.tools import weights as W  # noqa: E402

CHARS = "abcda fghij"          # 'a' twice (classes 4 and 8 of the CTC table decode to "a") and a space besides the built-in one
CTC_T, CTC_BML = 127, 100
ATTN_T, ATTN_BML = 129, 128


def logits_for(rows, C, tag):
    tgt = torch.tensor(rows, dtype=torch.long)
    B, T = tgt.shape
    lg = torch.from_numpy(np.round(W.uniform(f"scoring:{tag}", (B, T, C), -1.0, 1.0, 91) * 8) / 8).float()
    lg.scatter_add_(2, tgt.unsqueeze(2), torch.full((B, T, 1), 4.0))
    return lg


def word(n, start=0, alphabet="bcdfghij"):
    """n characters without adjacent repeats (a CTC alignment of length n then exists for T >= n)"""
    return "".join(alphabet[(start + i) % len(alphabet)] for i in range(n))


def ctc_cases():
    from tools.utils import CTCLabelConverter
    with contextlib.redirect_stdout(io.StringIO()):
        conv = CTCLabelConverter(CHARS)
    d, T = conv.dict, CTC_T
    first_a = 1 + conv.character[1:].index("a")            # the class of the FIRST 'a': decodes to "a", dict["a"] is the last one
    assert first_a != d["a"]

    def frames(tokens, gap=False):                         # one frame per token (+ a blank where two equal tokens meet), then blanks
        seq = []
        for t in tokens:
            if gap or (seq and seq[-1] == t):
                seq.append(0)
            seq.append(t)
        assert len(seq) <= T, len(seq)
        return seq + [0] * (T - len(seq))

    def ids(w):
        return [d[c] for c in w]
    w64, w65, w100 = word(64), word(65, 3), word(100, 5)
    b0_labels = [w64, w65, w100, "a da", "", "bcé"]
    b0_rows = [
        frames(ids(w64)),                                  # exact, 64 kept tokens
        frames(ids(w65)[:63] + [d["j"]] + ids(w65)[63:]),  # 66 kept: one insertion at the 64th token
        frames(ids(w100)[:99]),                            # 99 kept against 100
        frames([first_a, 3, d["d"], d["a"]]),              # the repeated character through both of its classes; 3 = the built-in space
        frames(ids("bc")),                                 # empty label, non-empty prediction
        frames(ids("bc") + [d["[UNK]"]]),                  # [UNK] predicted for the out-of-dictionary character: host row, not correct
    ]
    # rows that collapse across the 64th kept token: 63 singles, then the 64th token over three frames, then more
    long_tok = ids(word(70, 1))
    seq = long_tok[:63] + [long_tok[63]] * 3 + long_tok[64:]
    b1_labels = [word(70, 1), word(64, 2), "fg", "hi", "b"]
    b1_rows = [
        seq + [0] * (T - len(seq)),
        frames(ids(word(64, 2))[:32], gap=True),           # blanks between all tokens: 32 kept against 64
        [0] * T,                                           # all blank: empty prediction
        frames([d["h"], d["[PAD]"], d["i"]]),              # [PAD] predicted: host row
        [d["b"]] * T,                                      # one class repeated: collapses to one token
    ]
    return conv, CTC_BML, [(b0_labels, b0_rows), (b1_labels, b1_rows)]


def attn_cases():
    from tools.utils import AttnLabelConverter
    with contextlib.redirect_stdout(io.StringIO()):
        conv = AttnLabelConverter(CHARS)
    d, T = conv.dict, ATTN_T
    eos, unk, pad = d["[EOS]"], d["[UNK]"], d["[PAD]"]
    first_a = conv.character.index("a")
    assert first_a != d["a"]

    def ids(w):
        return [d[c] for c in w]

    def row(tokens, tail):                                 # tokens, [EOS], then `tail` repeated
        seq = tokens + [eos] + [tail] * T
        return seq[:T]
    w64, w128 = word(64), word(128, 2)
    b0_labels = [w64, w128, "", "a da", "bcd", "bc"]
    b0_rows = [
        row(ids(w64), d["b"]),                             # [EOS] at 64, exact
        row(ids(w128), d["b"]),                            # [EOS] at T - 1, exact (128 kept)
        row([], d["c"]),                                   # [EOS] at 0: empty prediction against an empty label
        row([first_a, 4, d["d"], d["a"]], unk),            # the repeated character, 4 = the built-in space; [UNK] AFTER [EOS]: device
        row(ids("bc") + [unk], d["b"]),                    # [UNK] BEFORE [EOS]: host row
        row(ids("bc"), pad),                               # [PAD] after [EOS]: stays on the device, exact
    ]
    b1_labels = [word(127, 4), "fgh", "ij", "b"]
    b1_rows = [
        (ids(word(128, 4)) * 2)[:T],                       # no [EOS]: the last position is dropped, 128 kept against 127
        row([d["f"], pad, d["h"]], d["b"]),                # [PAD] before [EOS]: host row
        (ids("ij") + [d["b"]] * T)[:T - 1] + [unk],        # no [EOS] and a [UNK] in the dropped last position: host row
        row(ids("b"), d["c"]),
    ]
    return conv, ATTN_BML, [(b0_labels, b0_rows), (b1_labels, b1_rows)]


def run(kind):
    conv, bml, batches = ctc_cases() if kind == "ctc" else attn_cases()
    opt = G.make_opt("crnn" if kind == "ctc" else "trba")
    opt.NED, opt.batch_max_length = True, bml
    C = len(conv.character)
    crit = torch.nn.CTCLoss(zero_infinity=True) if kind == "ctc" else torch.nn.CrossEntropyLoss(ignore_index=conv.dict["[PAD]"])
    d = {f"{kind}/chars": np.array(CHARS), f"{kind}/batch_max_length": np.int64(bml), f"{kind}/n_batches": np.int64(len(batches))}
    logits = [logits_for(rows, C, f"{kind}:{i}") for i, (_, rows) in enumerate(batches)]
    loader = [(torch.zeros(len(labels), 4, 32, 256), labels) for labels, _ in batches]
    for i, (labels, _) in enumerate(batches):
        d[f"{kind}/batch{i}/logits"] = logits[i].numpy()
        d[f"{kind}/batch{i}/labels"] = np.array(labels)

    def record(pre, r):
        loss, acc, ned, preds, conf, labels, _, n = r
        d[pre + "valid_loss"], d[pre + "accuracy"], d[pre + "ned"] = np.float64(float(loss)), np.float64(acc), np.float64(ned)
        d[pre + "preds_last_batch"] = np.array(list(preds))
        d[pre + "confidence_last_batch"] = np.array([float(c) for c in conf], dtype=np.float64)
        d[pre + "labels_last_batch"] = np.array(list(labels))
        d[pre + "length"] = np.int64(n)
        print(pre, "acc", acc, "ned", ned, "loss", float(loss), [float(c) for c in conf])
    with torch.no_grad(), contextlib.redirect_stderr(io.StringIO()):
        calls = iter(logits)
        record(f"{kind}/", G.ref_test.validation(lambda image, *a, **k: {"predict": next(calls), "feature": None}, crit, loader, conv, opt))
        for i in range(len(batches)):            # every batch alone too: the reference returns strings / confidences of the last batch only
            one = iter([logits[i]])
            record(f"{kind}/batch{i}/", G.ref_test.validation(lambda image, *a, **k: {"predict": next(one), "feature": None}, crit,
                                                               [loader[i]], conv, opt))
    return d


if __name__ == "__main__":
    out = {}
    for kind in ("ctc", "attn"):
        out.update(run(kind))
    path = os.path.join(HERE, "scoring.npz")
    np.savez_compressed(path, **out)
    print("scoring ->", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
