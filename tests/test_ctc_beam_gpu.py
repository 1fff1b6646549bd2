"""mrn_ctc_beam_decode_f32 (mrn_amd/csrc/ctc_beam.hip) against the float64 restatement of the algorithm in
tests/test_ctc_beam_cpu.py (reference()), against a brute force over all alignments and against the CTC log-likelihood
(torch ctc_loss, float64, CPU); strided views; the limits; validation() with opt.ctc_decode = "beam".

Tolerances.  The kernel runs the algorithm in float32, the reference in float64, and two prefixes at the beam boundary are routinely
as close as float32's own error, so the n-best lists need not be identical.  What float32 costs is measured on the reference itself:
d = the largest |best score in float32 - best score in float64| over a shape's inputs (both kinds, every sample), and then
tol = 4 d for a score, gap = 10 d for "the reference's top two are far enough apart that the best prefix must agree".  The values of
D below were printed by

    python -m tests.test_ctc_beam_gpu

which needs no GPU for the kernel shapes (it runs reference() twice); the validation() case takes its logits from a CRNN forward, so
its d is printed only where a GPU is present."""
import contextlib
import functools
import io
import math

import numpy as np
import pytest
import torch

from tests.test_ctc_beam_cpu import brute_force, ctc_converter, make_logits, n_best, reference

pytestmark = pytest.mark.gpu

KINDS = ("noise", "planted")
SHAPES = [(5, 9, 21, 3, 4), (8, 31, 37, 4, 8), (8, 31, 37, 16, 15), (6, 31, 5, 16, 15), (8, 63, 200, 8, 15), (4, 127, 5374, 8, 15),
          (3, 17, 70, 1, 1)]                     # (B, T, C, W, K)
EDGES = [(2, 512, 40, 16, 15), (4, 300, 40, 16, 15)]      # one sample per block (the largest LDS row) / three per block, B not a multiple
SEED = {shape: 2000 + n for n, shape in enumerate(SHAPES + EDGES)}
D = {                                            # measured d per shape, see the module docstring
    (5, 9, 21, 3, 4): 2.93e-06,
    (8, 31, 37, 4, 8): 5.87e-06,
    (8, 31, 37, 16, 15): 5.69e-06,
    (6, 31, 5, 16, 15): 3.16e-06,
    (8, 63, 200, 8, 15): 2.13e-05,
    (4, 127, 5374, 8, 15): 9.15e-05,
    (3, 17, 70, 1, 1): 1.46e-06,
    (2, 512, 40, 16, 15): 9.07e-05,
    (4, 300, 40, 16, 15): 6.04e-05,
    "validation": 3.79e-06,     # T = 31, C = 40: the logits of the CRNN of validation_case()
}


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    B, T, C, _, _ = shape
    x = make_logits(kind, B, T, C, SEED[shape] + 100 * KINDS.index(kind))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference_lists(shape, kind, dtype=np.float64):
    _, _, _, W, K = shape
    return [reference(x, W, K, dtype) for x in inputs(shape, kind)]


def measure_d(lists32, lists64):
    return max(abs(float(a[0][1]) - float(b[0][1])) for a, b in zip(lists32, lists64))


def top_gap(entries):
    return float(entries[0][1]) - float(entries[1][1]) if len(entries) > 1 else math.inf


def decode(x, W, K):
    from mrn_amd import ops
    out = ops.ctc_beam_decode(x if torch.is_tensor(x) else torch.from_numpy(np.array(x)).cuda(), W, K)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def log_likelihood(x, prefixes):
    """float64 CTC log-likelihood of every prefix under the logits x [T][C] (torch ctc_loss on the CPU, negated)"""
    T, _ = x.shape
    lp = torch.log_softmax(torch.from_numpy(np.array(x)).double(), dim=1).unsqueeze(1).expand(T, len(prefixes), -1)
    lens = torch.tensor([len(p) for p in prefixes], dtype=torch.long)
    width = max(1, int(lens.max()))
    tgt = torch.ones(len(prefixes), width, dtype=torch.long)
    for n, p in enumerate(prefixes):
        tgt[n, :len(p)] = torch.tensor(p, dtype=torch.long)
    nll = torch.nn.functional.ctc_loss(lp, tgt, torch.full((len(prefixes),), T, dtype=torch.long), lens, blank=0, reduction="none")
    return (-nll).tolist()


def as_frames(prefix, T):
    row = []
    for c in prefix:
        if row and row[-1] == c:
            row.append(0)
        row.append(c)
    assert len(row) <= T
    return row + [0] * (T - len(row))


def check_structure_and_mass(x, outs, b, tol):
    """(a) and (d) of one sample -> its live entries"""
    tokens, length, score, path, prob = outs
    W, T = tokens.shape[1], tokens.shape[2]
    live = int((length[b] >= 0).sum())
    assert live >= 1 and (length[b, :live] >= 0).all() and (length[b, live:] == -1).all()       # dead slots only behind live ones
    assert np.isneginf(score[b, live:]).all() and np.isfinite(score[b, :live]).all()
    assert (np.diff(score[b, :live]) <= 0).all()                                                   # descending total
    for w in range(W):
        n = max(int(length[b, w]), 0)
        assert n <= T and (tokens[b, w, :n] >= 1).all() and (tokens[b, w, :n] < x.shape[1]).all() and (tokens[b, w, n:] == 0).all()
    got = n_best(tokens[b], length[b], score[b])
    assert len({p for p, _ in got}) == len(got)                                                    # no duplicate prefixes
    for (p, s), ll in zip(got, log_likelihood(x, [p for p, _ in got])):
        assert s <= ll + tol, (b, p, s, ll)                                                        # pruning loses mass, never invents it
    assert path[b].tolist() == as_frames(got[0][0], T)
    assert abs(float(prob[b, 0]) - math.exp(got[0][1])) <= 4e-7 * math.exp(got[0][1]) + 1.5e-45          # expf of the float32 score
    assert (prob[b, 1:] == 1).all()
    return got


# ---- 5. core agreement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_the_float64_reference(shape, kind):
    B, T, C, W, K = shape
    tol, gap = 4 * D[shape], 10 * D[shape]
    x = inputs(shape, kind)
    want = reference_lists(shape, kind)
    outs = decode(x, W, K)
    under_gap = 0
    for b in range(B):
        got = check_structure_and_mass(x[b], outs, b, tol)
        ref = dict(want[b])
        shared = [(p, s) for p, s in got if p in ref]
        print(f"{shape} {kind} b={b}: {len(shared)}/{len(got)} shared, max |score - ref| "
              f"{max((abs(s - float(ref[p])) for p, s in shared), default=0.0):.3e} (tol {tol:.3e}), reference gap {top_gap(want[b]):.3e}")
        assert 2 * len(shared) >= W or len(shared) == len(want[b]) == len(got)      # (b) cannot pass vacuously
        for p, s in shared:
            assert abs(s - float(ref[p])) <= tol, (b, p, s, ref[p])
        if top_gap(want[b]) > gap:
            assert got[0][0] == want[b][0][0], (b, got[0], want[b][0])
        else:
            under_gap += 1
    assert under_gap <= B // 8


# ---- 6. exactness ------------------------------------------------------------------------------------------------------------------
def test_kernel_equals_the_brute_force_when_nothing_is_pruned():
    """T = 4, C = 3, W = 16, K = 2: all 15 labels fit the beam; four float32 frames are far inside 1e-5"""
    x = np.concatenate([(2.0 * np.random.default_rng(seed).standard_normal((1, 4, 3))).astype(np.float32) for seed in range(20)])
    tokens, length, score, _, _ = decode(x, 16, 2)
    for b in range(20):
        exact = brute_force(x[b])
        got = n_best(tokens[b], length[b], score[b])
        assert len(got) == 15 and {p for p, _ in got} == set(exact)
        for p, s in got:
            assert abs(s - exact[p]) <= 1e-5, (b, p, s, exact[p])
        assert got[0][0] == max(exact, key=exact.get)


# ---- 7. strides --------------------------------------------------------------------------------------------------------------------
def test_strided_views_decode_bit_identically():
    shape = SHAPES[1]
    B, T, C, W, K = shape
    x = torch.from_numpy(inputs(shape, "planted").copy()).cuda()
    base = decode(x, W, K)
    padded = torch.full((B, T, 64), 1e30, device="cuda")
    padded[:, :, :C] = x
    stepped = torch.full((B, 2 * T, C), 1e30, device="cuda")
    stepped[:, ::2] = x
    for view in (padded[:, :, :C], stepped[:, ::2]):
        assert not view.is_contiguous()
        for a, b in zip(base, decode(view, W, K)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 8. limits -----------------------------------------------------------------------------------------------------------------------
def test_bad_limits_are_errors():
    from mrn_amd import ops
    ok = dict(T=8, C=12, W=4, K=3)
    for key, bad in (("T", 513), ("W", 17), ("W", 0), ("K", 16), ("K", 0), ("C", 1), ("C", 65536)):
        a = {**ok, key: bad}
        with pytest.raises(RuntimeError, match="mrn_ctc_beam_decode_f32"):
            ops.ctc_beam_decode(torch.zeros(1, a["T"], a["C"], device="cuda"), a["W"], a["K"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctc_beam_decode(torch.zeros(1, 8, 12), 4, 3)
    with pytest.raises(RuntimeError, match="contiguous last dimension"):
        ops.ctc_beam_decode(torch.zeros(1, 8, 24, device="cuda")[:, :, ::2], 4, 3)
    assert ops.ctc_beam_decode(torch.zeros(0, 8, 12, device="cuda"), 4, 3)[0].shape == (0, 4, 8)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "x".join(map(str, s)))
def test_the_longest_rows(shape):
    """T = 512 at W = 16 is the largest LDS row (one sample per block); T = 300 puts three samples in a block with B = 4"""
    B, T, C, W, K = shape
    x = inputs(shape, "planted")
    outs = decode(x, W, K)
    for b in range(B):
        got = check_structure_and_mass(x[b], outs, b, 4 * D[shape])
        assert len(got[0][0]) > T // 8                      # a long label: the token rows are really used


# ---- 9. validation() -----------------------------------------------------------------------------------------------------------------
N_CHARS, VAL_SEED = 36, 61


@functools.lru_cache(maxsize=None)
def validation_case():
    """a small CRNN (32 x 128 input, hidden 128, 40 classes, random weights), two batches of 8 -> (net, converter, criterion, opt,
    batches, per-batch logits on the host)"""
    from mrn_amd.modules.model import Model
    from mrn_amd.test import _forward
    from mrn_amd.tools import weights as Wt
    from tests.test_validation_gpu import converter_and_criterion, make_opt
    opt = make_opt("crnn")
    opt.imgW, opt.hidden_size = 128, 128
    chars = "".join(chr(0x4E00 + i) for i in range(N_CHARS))
    classes = N_CHARS + 4
    with contextlib.redirect_stdout(io.StringIO()):
        net = Model(opt)
        net.update_fc(opt.hidden_size, classes)
        net.build_prediction(opt, classes)
    Wt.fill_state_dict(net.state_dict(), VAL_SEED)
    with torch.no_grad():
        net.fc.weight *= 60.0
    net = net.cuda().eval()
    conv, crit = converter_and_criterion("crnn", chars)
    batches = []
    for n in range(2):
        image = torch.from_numpy(Wt.smooth_image(f"beam:{n}:img", (8, 4, 32, 128), VAL_SEED))
        lens = Wt.randint(f"beam:{n}:len", (8,), 1, 9, VAL_SEED)
        labels = ["".join(chars[i] for i in Wt.randint(f"beam:{n}:lab{b}", (int(lens[b]),), 0, N_CHARS, VAL_SEED)) for b in range(8)]
        batches.append((image, labels))
    with torch.no_grad():
        logits = [_forward(net, image.cuda(), opt, conv, "val").cpu().numpy() for image, _ in batches]
    return net, conv, crit, opt, batches, logits


def run_validation(monkeypatch, scoring=None, **keys):
    from mrn_amd.test import validation
    net, conv, crit, opt, batches, _ = validation_case()
    if scoring is None:
        monkeypatch.delenv("MRN_VALIDATION_SCORING", raising=False)
    else:
        monkeypatch.setenv("MRN_VALIDATION_SCORING", scoring)
    o = type(opt)(**{**vars(opt), **keys})
    with torch.no_grad():
        return validation(net, crit, batches, conv, o)


def test_validation_with_the_beam_decoder(monkeypatch):
    from mrn_amd.test import _host_scores
    _, conv, _, _, batches, logits = validation_case()
    tol, gap = 4 * D["validation"], 10 * D["validation"]
    W, K = 8, 15
    T = logits[0].shape[1]
    n_correct, norm_ed, strings, scores = 0, 0.0, None, None
    for (_, labels), lg in zip(batches, logits):          # the expected returns: the reference's best labels through the host string loop
        lists = [reference(x, W, K) for x in lg]
        assert all(top_gap(e) > gap for e in lists), [top_gap(e) for e in lists]
        strings = conv.decode(np.array([as_frames(e[0][0], T) for e in lists]), [T] * len(lists))
        scores = [float(e[0][1]) for e in lists]
        probs = np.ones((len(lists), T), dtype=np.float32)
        probs[:, 0] = np.exp(scores)
        for term, correct, _ in _host_scores(labels, strings, probs, False, True):
            norm_ed += term if term is not None else 0
            n_correct += bool(correct)
    beam = run_validation(monkeypatch, ctc_decode="beam", beam_width=W, beam_top_n=K)
    assert list(beam[3]) == strings
    assert beam[1] == n_correct / 16 * 100 and beam[2] == norm_ed / 16 * 100 and beam[7] == 16
    for conf, s in zip(beam[4], scores):
        print(f"confidence {conf:.6e}, exp(reference score) {math.exp(s):.6e}, log difference {abs(math.log(conf) - s):.3e} (tol {tol:.3e})")
        assert conf > 0 and abs(math.log(conf) - s) <= tol
    host = run_validation(monkeypatch, scoring="host", ctc_decode="beam", beam_width=W, beam_top_n=K)
    for i in (0, 1, 2, 3, 4, 5, 7):                       # all but infer_time, which is a clock reading
        assert beam[i] == host[i], (i, beam[i], host[i])
    default = run_validation(monkeypatch, beam_width=W)    # the key absent: greedy, whatever the beam's own keys say
    greedy = run_validation(monkeypatch, ctc_decode="greedy")
    for i in (0, 1, 2, 3, 4, 5, 7):
        assert default[i] == greedy[i], (i, default[i], greedy[i])
    assert beam[0] == greedy[0]                            # the loss does not depend on the decoder
    assert default[4] != beam[4]                           # ... the confidences do: label probability against the best alignment's


def test_validation_takes_the_host_decoder_outside_the_kernel_limits(monkeypatch):
    """a beam of 17 is one more than the kernel takes: the float64 host form decodes, the kernel is never called, the labels agree"""
    from tests.test_scoring_gpu import recorded_calls
    with recorded_calls() as log:
        wide = run_validation(monkeypatch, ctc_decode="beam", beam_width=17, beam_top_n=15)
    assert log.count("mrn_ctc_beam_decode_f32") == 0
    with recorded_calls() as log:
        beam = run_validation(monkeypatch, ctc_decode="beam", beam_width=16, beam_top_n=15)
    assert log.count("mrn_ctc_beam_decode_f32") == 2      # one launch per batch
    assert wide[3] == beam[3] and wide[1] == beam[1]


if __name__ == "__main__":                                # the measured d values of D
    for shape in SHAPES + EDGES:
        kinds = KINDS if shape in SHAPES else ("planted",)
        d = max(measure_d(reference_lists(shape, k, np.float32), reference_lists(shape, k)) for k in kinds)
        gaps = [top_gap(e) for k in kinds for e in reference_lists(shape, k)]
        print(f"    {shape}: {d:.2e},    # smallest reference gap {min(gaps):.2e}, under 10 d: {sum(g <= 10 * d for g in gaps)}", flush=True)
    if torch.cuda.is_available():
        logits = validation_case()[5]
        lists32 = [reference(x, 8, 15, np.float32) for lg in logits for x in lg]
        lists64 = [reference(x, 8, 15) for lg in logits for x in lg]
        d = measure_d(lists32, lists64)
        print(f'    "validation": {d:.2e},    # T = {logits[0].shape[1]}, C = {logits[0].shape[2]}, smallest reference gap '
              f"{min(top_gap(e) for e in lists64):.2e}", flush=True)
