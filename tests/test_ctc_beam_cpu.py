"""CTC prefix beam search on the host (mrn_amd/modules/decoding.py::ctc_beam_host) against this file's own restatement of the
algorithm and against a brute force over every alignment; the (path, prob) pair through CTCLabelConverter.decode; the options and the
kernel's limits.  The restatement (reference(), plain loops, any float type) and the brute force are also what
tests/test_ctc_beam_gpu.py holds mrn_ctc_beam_decode_f32 against."""
import contextlib
import ctypes
import io
import itertools
import types

import numpy as np
import pytest


# ---- the test's own reference, written from the algorithm (never imports the code under test) ---------------------------------
def reference(x, W, K, dtype=np.float64):
    """prefix beam search of one sample x [T][C] in `dtype` arithmetic -> [(prefix, total)] in descending total"""
    f = dtype
    ninf = f(-np.inf)
    T, C = x.shape
    k = min(K, C - 1)
    beam = [((), f(0), ninf)]
    for t in range(T):
        row = x[t].astype(f)
        peak = row.max()
        lp = row - (peak + np.log(np.sum(np.exp(row - peak), dtype=f)))
        nonblank = np.arange(1, C)
        S = [int(c) for c in nonblank[np.lexsort((nonblank, -x[t, 1:].astype(np.float64)))][:k]]       # raw logit down, class up
        live = {p: j for j, (p, _, _) in enumerate(beam)}
        stay = []
        for p, pb, pnb in beam:
            total = np.logaddexp(pb, pnb)
            stay.append([p, total + lp[0], pnb + lp[p[-1]] if p and p[-1] in S else ninf])
        ext = {}
        for i, (p, pb, pnb) in enumerate(beam):
            total = np.logaddexp(pb, pnb)
            for r, c in enumerate(S):
                v = (pb if p and p[-1] == c else total) + lp[c]
                q = p + (c,)
                if q in live:
                    stay[live[q]][2] = np.logaddexp(stay[live[q]][2], v)
                else:
                    ext[(i, r)] = (q, ninf, v)
        cands = []                                                  # candidate order: entry, then stay before the ranks
        for i in range(len(beam)):
            cands.append(tuple(stay[i]))
            cands.extend(ext[(i, r)] for r in range(len(S)) if (i, r) in ext)
        totals = [np.logaddexp(pb, pnb) for _, pb, pnb in cands]
        order = sorted((n for n in range(len(cands)) if np.isfinite(totals[n])), key=lambda n: (-totals[n], n))[:W]
        beam = [cands[n] for n in order]
        assert all(isinstance(v, f) for _, pb, pnb in beam for v in (pb, pnb))
    return [(p, np.logaddexp(pb, pnb)) for p, pb, pnb in beam]


def brute_force(x):
    """log-probability of every label of x [T][C], summed over all C**T alignments in float64 -> {label tuple: log p}"""
    T, C = x.shape
    x = x.astype(np.float64)
    lp = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    mass = {}
    for align in itertools.product(range(C), repeat=T):
        label = tuple(c for n, c in enumerate(align) if c != 0 and (n == 0 or c != align[n - 1]))
        mass[label] = mass.get(label, 0.0) + float(np.exp(sum(lp[t, c] for t, c in enumerate(align))))
    return {label: float(np.log(p)) for label, p in mass.items()}


def make_logits(kind, B, T, C, seed):
    """float32 [B][T][C]: "noise" = 3 * randn; "planted" = the same with the blank raised by 2.5 sigma and, at random frames, a random
    class raised above it (labels with gaps, repeats and doubled characters)"""
    rng = np.random.default_rng(seed)
    x = 3.0 * rng.standard_normal((B, T, C))
    if kind == "planted":
        x[:, :, 0] += 7.5
        for b in range(B):
            frames = np.flatnonzero(rng.random(T) < 0.4)
            x[b, frames, rng.integers(1, C, size=frames.size)] += 15.0
    return x.astype(np.float32)


def n_best(tokens, length, score):
    """one sample's outputs -> [(prefix, score)] of the live slots"""
    return [(tuple(int(c) for c in tokens[w, :length[w]]), float(score[w])) for w in range(len(length)) if length[w] >= 0]


def ctc_converter(n_chars):
    from mrn_amd.tools.utils import CTCLabelConverter
    with contextlib.redirect_stdout(io.StringIO()):
        return CTCLabelConverter("".join(chr(0x4E00 + i) for i in range(n_chars)))


# ---- 1. exactness without pruning ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_host_equals_the_brute_force_when_nothing_is_pruned(seed):
    from mrn_amd.modules.decoding import ctc_beam_host
    x = (2.0 * np.random.default_rng(seed).standard_normal((1, 4, 3))).astype(np.float32)
    exact = brute_force(x[0])
    assert len(exact) == 15 <= 16                                   # every label of up to 4 frames over 2 classes fits the beam
    tokens, length, score, _, _ = ctc_beam_host(x, 16, 2)
    got = n_best(tokens[0], length[0], score[0])
    assert {p for p, _ in got} == set(exact) and len(got) == 15
    for p, s in got:
        assert abs(s - exact[p]) <= 1e-9, (p, s, exact[p])
    assert got[0][0] == max(exact, key=exact.get)
    assert (length[0, 15:] == -1).all() and np.isneginf(score[0, 15:]).all()


# ---- 2. the host form equals the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "planted"])
@pytest.mark.parametrize("T,C,W,K", [(9, 21, 3, 4), (31, 37, 4, 8), (31, 37, 16, 15), (31, 5, 16, 15)])
def test_host_equals_the_reference(T, C, W, K, kind):
    """both sides are float64: the same n-best lists, in order ((31, 5, 16, 15): the cut-off is clamped to the C - 1 = 4 classes)"""
    from mrn_amd.modules.decoding import ctc_beam_host
    for seed in (1000, 1001):
        x = make_logits(kind, 2, T, C, seed)
        tokens, length, score, _, _ = ctc_beam_host(x, W, K)
        for b in range(len(x)):
            want = reference(x[b], W, K)
            got = n_best(tokens[b], length[b], score[b])
            assert [p for p, _ in got] == [p for p, _ in want], (seed, b)
            assert max(abs(s - float(w)) for (_, s), (_, w) in zip(got, want)) <= 1e-9
            assert all((tokens[b, w, max(int(length[b, w]), 0):] == 0).all() for w in range(W))
            dead = length[b] < 0
            assert not dead[:len(want)].any() and dead[len(want):].all() and np.isneginf(score[b][dead]).all()


# ---- 3. path / prob go where argmax_prob_lastdim's pair goes ---------------------------------------------------------------------
def test_path_and_prob_round_trip():
    """CTCLabelConverter.decode(path) spells the best prefix -- also one with doubled characters, forced by planted logits -- and the
    cumulative product of prob is float32(exp(score))"""
    from mrn_amd.modules.decoding import ctc_beam_host
    conv = ctc_converter(33)                                        # 37 classes
    x = make_logits("planted", 3, 31, 37, 7)
    x[0] = -4.0                                                     # sample 0: "5 5 9 9 9 6" with blanks only where the label needs them
    for t, c in enumerate([5, 0, 5, 5, 9, 0, 9, 0, 9, 6]):
        x[0, t, c] = 9.0
    x[0, 10:, 0] = 9.0
    tokens, length, score, path, prob = ctc_beam_host(x, 8, 15)
    assert tuple(tokens[0, 0, :length[0, 0]]) == (5, 5, 9, 9, 9, 6)
    assert path[0].tolist() == [5, 0, 5, 9, 0, 9, 0, 9, 6] + [0] * 22
    strings = conv.decode(path, [31] * 3)
    for b in range(3):
        best = tokens[b, 0, :length[b, 0]]
        assert strings[b] == "".join(conv.character[c] for c in best)
        assert path.dtype == np.int64 and prob.dtype == np.float32
        assert np.cumprod(prob[b])[-1] == np.float32(np.exp(score[b, 0]))
        assert (prob[b, 1:] == 1).all()


# ---- 4. options and limits ---------------------------------------------------------------------------------------------------------
def test_options_and_limits():
    from mrn_amd.modules import decoding as D
    assert D.decode_options(types.SimpleNamespace()) == ("greedy", 8, 15)
    assert D.decode_options(types.SimpleNamespace(ctc_decode="beam", beam_width=4, beam_top_n=3)) == ("beam", 4, 3)
    with pytest.raises(ValueError, match="greedy.*beam"):
        D.decode_options(types.SimpleNamespace(ctc_decode="best"))
    for bad in (0, -1, 2.5, "8", True, None):
        with pytest.raises(ValueError, match="beam_width must be an integer >= 1"):
            D.decode_options(types.SimpleNamespace(beam_width=bad))
        with pytest.raises(ValueError, match="beam_top_n must be an integer >= 1"):
            D.decode_options(types.SimpleNamespace(beam_top_n=bad))
    ok = dict(prediction="CTC", T=31, C=37, W=8, K=15)
    assert D.beam_supported(**ok)
    for key, inside, outside in (("T", 512, 513), ("T", 1, 0), ("W", 16, 17), ("W", 1, 0), ("K", 15, 16), ("K", 1, 0),
                                 ("C", 65535, 65536), ("C", 2, 1)):
        assert D.beam_supported(**{**ok, key: inside}), (key, inside)
        assert not D.beam_supported(**{**ok, key: outside}), (key, outside)
    assert not D.beam_supported(**{**ok, "prediction": "Attn"})
    x = make_logits("noise", 1, 5, 4, 3)
    tokens, length, _, _, _ = D.ctc_beam_host(x, 20, 30)            # the host form has no such limits
    assert tokens.shape == (1, 20, 5) and (length[0] >= 0).sum() == 20
    with pytest.raises(ValueError, match="ctc_beam_host needs"):
        D.ctc_beam_host(x[0], 4, 4)


def test_entry_point_is_declared_exported_and_cited():
    """include/mrn_decode.h is parsed and bound like include/mrn_hip.h: the prototype there, the symbol in the library, the
    reference op site in its comment"""
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.DECODE_HEADER_PATH)
    assert list(protos) == ["mrn_ctc_beam_decode_f32"]
    ret, argtypes, argnames = protos["mrn_ctc_beam_decode_f32"]
    assert ret == "int" and argnames == ["logits", "stride_b", "stride_t", "B", "T", "C", "W", "K", "tokens", "length", "score", "path",
                                         "prob", "stream"]
    assert argtypes[:3] == ["const float*", "int64_t", "int64_t"] and argtypes[-3:] == ["int64_t*", "float*", "void*"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mrn_ctc_beam_decode_f32")
    assert not set(protos) & set(_lib.parse_header())
    bound = _lib.LIB.load().mrn_ctc_beam_decode_f32
    assert bound.restype is ctypes.c_int and len(bound.argtypes) == 14
    header = open(_lib.DECODE_HEADER_PATH).read()
    comment = header[:header.index("int mrn_ctc_beam_decode_f32(")].rsplit("/*", 1)[1]
    assert "test.py:211-219" in comment and "1 <= T <= 512" in comment
