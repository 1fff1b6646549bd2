"""mrn_ctc_beam_lm_decode_f32 (mrn_amd/csrc/ctc_beam.hip, LM = true) against the float64 host form of the fused search
(mrn_amd/modules/decoding.py::ctc_beam_host(lm=), itself held against a brute force in tests/test_ctc_lm_cpu.py): every shape that
reaches another mechanism of the kernel, models with an empty table, with fewer classes than the head and with forced collisions,
strided views, a planted tie the model decides, the limits, and validation() with opt.ctc_lm.

Tolerances follow tests/test_ctc_beam_gpu.py.  The kernel runs in float32, the reference in float64, and what float32 costs is
measured on the host form itself, run in both: d = the largest |best fused key in float32 - in float64| over a case's inputs (both
kinds, every sample); tol = 4 d for the score and the fused key of a prefix both sides returned, gap = 10 d for "the reference's top
two keys are far enough apart that the best prefix must agree".  The values of D below were printed by

    python -m tests.test_ctc_lm_gpu

which needs no GPU for the kernel cases (it also checks that the float32 host form meets the anti-vacuity conditions against the
float64 one); the validation() case takes its logits from a CRNN forward, so its d is printed only where a GPU is present."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_ctc_beam_cpu import make_logits, n_best
from tests.test_ctc_beam_gpu import as_frames, log_likelihood
from tests.test_ctc_lm_cpu import DISCOUNT, collision_lm, planted_case, synthetic_rows

pytestmark = pytest.mark.gpu

KINDS = ("noise", "planted")
ALPHA, BETA = 0.5, 0.25
SHAPES = [(5, 9, 21, 3, 4, 2), (8, 31, 37, 16, 15, 3), (3, 17, 70, 1, 1, 3), (4, 63, 5374, 8, 15, 3)]      # (B, T, C, W, K, order)
EDGES = [(2, 512, 40, 16, 15, 2), (4, 300, 40, 16, 15, 3)]       # one sample per block / three per block, B not a multiple of the rows
SMALL = SHAPES[1]                                                 # the shape of the cases that vary the model
SEED = {shape: 3000 + n for n, shape in enumerate(SHAPES + EDGES)}
SEED[EDGES[0]] = 3017     # (3004: no sample of the noise kind has a reference gap above 10 d)
CASES = ("unigram", "unk", "collision")
D = {                                            # measured d per case, see the module docstring
    (5, 9, 21, 3, 4, 2): 2.20e-06,
    (8, 31, 37, 16, 15, 3): 7.84e-06,
    (3, 17, 70, 1, 1, 3): 5.31e-06,
    (4, 63, 5374, 8, 15, 3): 5.06e-05,
    (2, 512, 40, 16, 15, 2): 5.65e-04,
    (4, 300, 40, 16, 15, 3): 1.10e-04,
    "unigram": 5.46e-06,        # the three models of CASES on the shape SMALL
    "unk": 9.16e-06,
    "collision": 8.10e-06,
    "validation": 3.75e-06,     # T = 31, C = 40: the logits of the CRNN of validation_case()
}


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    B, T, C = shape[:3]
    x = make_logits(kind, B, T, C, SEED[shape] + 100 * KINDS.index(kind))
    x.setflags(write=False)
    return x


def best_path_rows(x):
    """the greedy labels of x [B][T][C]: text in which the n-grams the decoder meets are seen"""
    rows = []
    for frames in x.argmax(axis=2):
        row = [int(c) for n, c in enumerate(frames) if c != 0 and (n == 0 or c != frames[n - 1])]
        if row:
            rows.append(row)
    return rows


@functools.lru_cache(maxsize=None)
def model(shape, case=None):
    """the model of a shape: synthetic text over the head's classes and the greedy labels of the first half of each batch, so that
    some contexts of the search are seen and most are not.  case: "unigram" = order 1 (an empty table), "unk" = seven classes fewer
    than the head, "collision" = tests/test_ctc_lm_cpu.py collision_lm"""
    from mrn_amd.modules.char_lm import lm_from_rows
    B, T, C, _, _, order = shape
    if case == "collision":
        return collision_lm(C)
    C_lm = C - 7 if case == "unk" else C
    rows = synthetic_rows(C_lm, 200, SEED[shape])
    for kind in KINDS:
        rows += [r for r in best_path_rows(inputs(shape, kind)[:(B + 1) // 2]) if max(r) < C_lm] * 3
    return lm_from_rows(rows, C_lm, 1 if case == "unigram" else order, DISCOUNT)


@functools.lru_cache(maxsize=None)
def host_lists(shape, kind, case=None, dtype=np.float64):
    """[(prefix, score, fused)] per sample from the host form"""
    from mrn_amd.modules.decoding import ctc_beam_host
    _, _, _, W, K, _ = shape
    tokens, length, score, _, _, fused = ctc_beam_host(inputs(shape, kind), W, K, lm=model(shape, case), lm_weight=ALPHA, lm_bonus=BETA,
                                                       dtype=dtype)
    return [[(p, float(score[b, w]), float(fused[b, w])) for w, (p, _) in enumerate(n_best(tokens[b], length[b], score[b]))]
            for b in range(len(tokens))]


def measure_d(lists32, lists64):
    return max(abs(a[0][2] - b[0][2]) for a, b in zip(lists32, lists64))


def top_gap(entries):
    return entries[0][2] - entries[1][2] if len(entries) > 1 else math.inf


@functools.lru_cache(maxsize=None)
def handle(shape, case=None):
    from mrn_amd import ops
    return ops.upload_char_lm(model(shape, case), "cuda")


def decode(x, W, K, lm=None, alpha=ALPHA, beta=BETA):
    from mrn_amd import ops
    x = x if torch.is_tensor(x) else torch.from_numpy(np.array(x)).cuda()
    out = ops.ctc_beam_decode(x, W, K) if lm is None else ops.ctc_beam_decode(x, W, K, lm, alpha, beta)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def agreement(got, want, W, tol, gap):
    """one sample: got / want = [(prefix, score, fused)] of the side under test / of the float64 reference -> is the reference's gap
    above `gap`.  The conditions every float32 form of the search has to meet against the float64 one"""
    ref = {p: (s, f) for p, s, f in want}
    shared = [e for e in got if e[0] in ref]
    assert 2 * len(shared) >= W or len(shared) == len(want) == len(got), (len(shared), len(got), len(want))      # not vacuous
    for p, s, f in shared:
        assert abs(s - ref[p][0]) <= tol and abs(f - ref[p][1]) <= tol, (p, s, f, ref[p])
    if top_gap(want) > gap:
        assert got[0][0] == want[0][0], (got[0], want[0])
        return True
    return False


def check_structure(x, outs, b, tol):
    """one sample of the kernel's outputs -> its live entries [(prefix, score, fused)]"""
    tokens, length, score, path, prob, fused = outs
    W, T = tokens.shape[1], tokens.shape[2]
    live = int((length[b] >= 0).sum())
    assert live >= 1 and (length[b, :live] >= 0).all() and (length[b, live:] == -1).all()
    assert np.isneginf(score[b, live:]).all() and np.isfinite(score[b, :live]).all()
    assert np.isneginf(fused[b, live:]).all() and np.isfinite(fused[b, :live]).all()
    assert (np.diff(fused[b, :live]) <= 0).all()                                                   # descending fused key
    for w in range(W):
        n = max(int(length[b, w]), 0)
        assert n <= T and (tokens[b, w, :n] >= 1).all() and (tokens[b, w, :n] < x.shape[1]).all() and (tokens[b, w, n:] == 0).all()
    got = [(p, s, float(fused[b, w])) for w, (p, s) in enumerate(n_best(tokens[b], length[b], score[b]))]
    assert len({p for p, _, _ in got}) == len(got)
    for (p, s, _), ll in zip(got, log_likelihood(x, [p for p, _, _ in got])):
        assert s <= ll + tol, (b, p, s, ll)                                                        # score is acoustic: never above the likelihood
    assert path[b].tolist() == as_frames(got[0][0], T)
    assert abs(float(prob[b, 0]) - math.exp(got[0][1])) <= 4e-7 * math.exp(got[0][1]) + 1.5e-45
    assert (prob[b, 1:] == 1).all()
    return got


def kernel_vs_host(shape, kind, case=None):
    B, T, C, W, K, _ = shape
    d = D[case or shape]
    x = inputs(shape, kind)
    want = host_lists(shape, kind, case)
    outs = decode(x, W, K, handle(shape, case))
    clear = 0
    for b in range(B):
        got = check_structure(x[b], outs, b, 4 * d)
        ref = {p: (s, f) for p, s, f in want[b]}
        diffs = [max(abs(s - ref[p][0]), abs(f - ref[p][1])) for p, s, f in got if p in ref]
        print(f"{case or shape} {kind} b={b}: {len(diffs)}/{len(got)} shared, max |score or fused - ref| {max(diffs, default=0.0):.3e} "
              f"(tol {4 * d:.3e}), reference gap {top_gap(want[b]):.3e} (gap {10 * d:.3e})")
        clear += agreement(got, want[b], W, 4 * d, 10 * d)
    assert clear >= 1                                                                              # a sample whose best label is pinned


# ---- 1. the kernel against the float64 host form -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES + EDGES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_the_float64_host_form(shape, kind):
    kernel_vs_host(shape, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES)
def test_kernel_vs_the_float64_host_form_on_other_models(case, kind):
    """an order-1 model with an empty table; a model of seven classes fewer than the head (the unk path); eight trigrams in one probe
    sequence of a 16-slot table"""
    lm = model(SMALL, case)
    assert {"unigram": lm.max_probe == 0 and not lm.keys.any(), "unk": lm.C_lm == SMALL[2] - 7,
            "collision": lm.max_probe == 8 and len(lm.keys) == 16}[case]
    kernel_vs_host(SMALL, kind, case)


# ---- 2. exactness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], EDGES[1]], ids=lambda s: "x".join(map(str, s)))
def test_without_weights_the_outputs_are_the_plain_decoder_s(shape):
    B, T, C, W, K, _ = shape
    for kind in KINDS:
        x = inputs(shape, kind)
        plain = decode(x, W, K)
        fused = decode(x, W, K, handle(shape), 0.0, 0.0)
        assert len(plain) == 5 and len(fused) == 6
        for a, b in zip(plain, fused):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert fused[5].tobytes() == fused[2].tobytes()                                            # the key is the total


def test_two_calls_return_the_same_bits_and_strided_views_too():
    shape = SMALL
    B, T, C, W, K, _ = shape
    x = torch.from_numpy(inputs(shape, "planted").copy()).cuda()
    base = decode(x, W, K, handle(shape))
    padded = torch.full((B, T, 64), 1e30, device="cuda")
    padded[:, :, :C] = x
    stepped = torch.full((B, 2 * T, C), 1e30, device="cuda")
    stepped[:, ::2] = x
    for view in (x, padded[:, :, :C], stepped[:, ::2]):
        assert view is x or not view.is_contiguous()
        for a, b in zip(base, decode(view, W, K, handle(shape))):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_model_decides_a_planted_tie():
    from mrn_amd import ops
    x, lm = planted_case()
    h = ops.upload_char_lm(lm, "cuda")
    tokens, length, score, _, _, _ = decode(x, 4, 3, h, 0.0, 0.0)
    assert n_best(tokens[0], length[0], score[0])[0][0] == (1, 2) and score[0, 0] == score[0, 1]   # the acoustic tie order
    tokens, length, score, path, _, fused = decode(x, 4, 3, h, 0.5, 0.0)
    assert n_best(tokens[0], length[0], score[0])[0][0] == (1, 3) and path[0].tolist() == [1, 3, 0, 0] and fused[0, 0] > fused[0, 1]


# ---- 3. limits -----------------------------------------------------------------------------------------------------------------------
def test_bad_limits_are_errors_before_any_launch():
    from mrn_amd import ops
    from mrn_amd.modules.char_lm import CharLM
    from tests.test_scoring_gpu import recorded_calls
    h = handle(SHAPES[0])
    ok = dict(T=8, C=12, W=4, K=3)
    for key, bad in (("T", 513), ("W", 17), ("W", 0), ("K", 16), ("K", 0), ("C", 1), ("C", 65536)):
        a = {**ok, key: bad}
        with pytest.raises(RuntimeError, match="mrn_ctc_beam_lm_decode_f32"):
            ops.ctc_beam_decode(torch.zeros(1, a["T"], a["C"], device="cuda"), a["W"], a["K"], h, 0.5, 0.0)
    x = torch.zeros(1, 8, 12, device="cuda")
    for kw in (dict(lm_weight=-1.0), dict(lm_weight=math.inf), dict(lm_bonus=math.nan)):
        with pytest.raises(ValueError, match="lm_weight|lm_bonus"):
            ops.ctc_beam_decode(x, 4, 3, h, **kw)
    with pytest.raises(RuntimeError, match="CharLMHandle"):
        ops.ctc_beam_decode(x, 4, 3, model(SHAPES[0]), 0.5, 0.0)
    with recorded_calls() as log:
        with pytest.raises(ValueError, match="above 65535"):
            ops.upload_char_lm(CharLM(1, np.full(65536, -11.1), np.zeros(65536), -11.1), "cuda")
    assert not log
    outs = [torch.empty(1, 4, 8, device="cuda", dtype=torch.int32), torch.empty(1, 4, device="cuda", dtype=torch.int32),
            torch.empty(1, 4, device="cuda"), torch.empty(1, 8, device="cuda", dtype=torch.int64), torch.empty(1, 8, device="cuda"),
            torch.empty(1, 4, device="cuda")]
    good = dict(mask=h.size - 1, probe=h.max_probe, C_lm=h.C_lm, unk=h.unk_logp, order=h.order, alpha=0.5, beta=0.0)
    for key, bad, match in (("mask", h.size, "power of two"), ("mask", (1 << 26) * 2 - 1, "power of two"), ("probe", h.size + 1, "max_probe"),
                            ("probe", -1, "max_probe"), ("C_lm", 65536, "C_lm"), ("C_lm", 0, "C_lm"), ("order", 0, "order"),
                            ("order", 4, "order"), ("alpha", -0.5, "alpha"), ("beta", math.inf, "beta"), ("unk", -math.inf, "unk_logp")):
        a = {**good, key: bad}
        with pytest.raises(RuntimeError, match=f"mrn_ctc_beam_lm_decode_f32.*{match}"):
            ops.call("mrn_ctc_beam_lm_decode_f32", x.data_ptr(), x.stride(0), x.stride(1), 1, 8, 12, 4, 3, *[o.data_ptr() for o in outs[:5]],
                     h.keys.data_ptr(), h.vals.data_ptr(), a["mask"], a["probe"], h.uni_logp.data_ptr(), h.uni_bow.data_ptr(), a["C_lm"],
                     a["unk"], a["order"], a["alpha"], a["beta"], outs[5].data_ptr(), None)
    assert len(ops.ctc_beam_decode(torch.zeros(0, 8, 12, device="cuda"), 4, 3, h, 0.5, 0.0)) == 6
    torch.cuda.synchronize()


# ---- 4. validation() -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def validation_lm():
    """a trigram model over the 40 classes of validation_case(): its labels and random strings of its characters"""
    from mrn_amd.modules.char_lm import build_char_lm
    from tests.test_ctc_beam_gpu import validation_case
    _, conv, _, _, batches, _ = validation_case()
    chars = conv.character[4:]
    rng = np.random.default_rng(17)
    texts = [lab for _, labels in batches for lab in labels] * 2
    texts += ["".join(chars[i] for i in rng.integers(0, len(chars), size=int(rng.integers(1, 9)))) for _ in range(100)]
    return build_char_lm(conv, texts, order=3)


def validation_lists(dtype=np.float64, W=8):
    from mrn_amd.modules.decoding import ctc_beam_host
    from tests.test_ctc_beam_gpu import validation_case
    out = []
    for lg in validation_case()[5]:
        tokens, length, score, _, _, fused = ctc_beam_host(lg, W, 15, lm=validation_lm(), lm_weight=0.5, lm_bonus=0.0, dtype=dtype)
        out.append([[(p, float(score[b, w]), float(fused[b, w])) for w, (p, _) in enumerate(n_best(tokens[b], length[b], score[b]))]
                    for b in range(len(lg))])
    return out


def test_validation_with_the_fused_beam_decoder(monkeypatch):
    """opt.ctc_lm with the default weights (0.5, 0): the eight returns are those of scoring the host form's best entries"""
    from mrn_amd.test import _host_scores
    from tests.test_ctc_beam_gpu import run_validation, validation_case
    from tests.test_scoring_gpu import recorded_calls
    _, conv, _, _, batches, logits = validation_case()
    tol, gap = 4 * D["validation"], 10 * D["validation"]
    T = logits[0].shape[1]
    n_correct, norm_ed, strings, scores = 0, 0.0, None, None
    for (_, labels), lists in zip(batches, validation_lists()):
        assert all(top_gap(e) > gap for e in lists), [top_gap(e) for e in lists]
        strings = conv.decode(np.array([as_frames(e[0][0], T) for e in lists]), [T] * len(lists))
        scores = [e[0][1] for e in lists]
        probs = np.ones((len(lists), T), dtype=np.float32)
        probs[:, 0] = np.exp(scores)
        for term, correct, _ in _host_scores(labels, strings, probs, False, True):
            norm_ed += term if term is not None else 0
            n_correct += bool(correct)
    with recorded_calls() as log:
        fused = run_validation(monkeypatch, ctc_decode="beam", ctc_lm=validation_lm())
    assert log.count("mrn_ctc_beam_lm_decode_f32") == 2 and log.count("mrn_ctc_beam_decode_f32") == 0
    assert list(fused[3]) == strings
    assert fused[1] == n_correct / 16 * 100 and fused[2] == norm_ed / 16 * 100 and fused[7] == 16
    for conf, s in zip(fused[4], scores):
        assert conf > 0 and abs(math.log(conf) - s) <= tol                                         # the confidence is acoustic
    host = run_validation(monkeypatch, scoring="host", ctc_decode="beam", ctc_lm=validation_lm())
    for i in (0, 1, 2, 3, 4, 5, 7):
        assert fused[i] == host[i], (i, fused[i], host[i])
    with recorded_calls() as log:
        wide = run_validation(monkeypatch, ctc_decode="beam", ctc_lm=validation_lm(), beam_width=17)      # the host form decodes
    last17 = validation_lists(W=17)[-1]                    # (a wider beam may find another label: its own host form is the yardstick)
    assert log.count("mrn_ctc_beam_lm_decode_f32") == 0
    assert list(wide[3]) == conv.decode(np.array([as_frames(e[0][0], T) for e in last17]), [T] * len(last17))
    with recorded_calls() as log:
        absent = run_validation(monkeypatch, ctc_decode="beam")
    assert log.count("mrn_ctc_beam_decode_f32") == 2 and log.count("mrn_ctc_beam_lm_decode_f32") == 0
    none = run_validation(monkeypatch, ctc_decode="beam", ctc_lm=None, lm_weight=3.0)
    zero = run_validation(monkeypatch, ctc_decode="beam", ctc_lm=validation_lm(), lm_weight=0.0)
    for i in (0, 1, 2, 3, 4, 5, 7):
        assert absent[i] == none[i] == zero[i], (i, absent[i], none[i], zero[i])
    assert fused[4] != absent[4]                                                                   # the model changes what is decoded
    attn_like = run_validation(monkeypatch, ctc_lm=None)                                          # greedy, the option absent
    assert attn_like[3] == run_validation(monkeypatch)[3]


if __name__ == "__main__":                                # the measured d values of D, and the conditions on the float32 host form
    def report(name, shape, case):
        W = shape[3]
        l32 = {k: host_lists(shape, k, case, np.float32) for k in KINDS}
        l64 = {k: host_lists(shape, k, case) for k in KINDS}
        d = max(measure_d(l32[k], l64[k]) for k in KINDS)
        gaps = [top_gap(e) for k in KINDS for e in l64[k]]
        for k in KINDS:
            assert sum(agreement(a, b, W, 4 * d, 10 * d) for a, b in zip(l32[k], l64[k])) >= 1, (name, k)
        print(f"    {name}: {d:.2e},    # smallest reference gap {min(gaps):.2e}, under 10 d: {sum(g <= 10 * d for g in gaps)} of {len(gaps)}",
              flush=True)

    import sys
    only_validation = "validation" in sys.argv[1:]        # python -m tests.test_ctc_lm_gpu validation: that line alone
    for shape in [] if only_validation else SHAPES + EDGES:
        report(repr(shape), shape, None)
    for case in () if only_validation else CASES:
        report(f'"{case}"', SMALL, case)
    if torch.cuda.is_available():
        l32, l64 = validation_lists(np.float32), validation_lists()
        d = max(measure_d(a, b) for a, b in zip(l32, l64))
        print(f'    "validation": {d:.2e},    # smallest reference gap {min(top_gap(e) for batch in l64 for e in batch):.2e}', flush=True)
