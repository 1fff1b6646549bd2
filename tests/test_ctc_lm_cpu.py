"""The character n-gram model (mrn_amd/modules/char_lm.py) and its fusion into the host form of the CTC prefix beam search
(mrn_amd/modules/decoding.py::ctc_beam_host(lm=)): normalisation and the back-off form against the interpolated formula, the hash
table, the fused search against a brute force over every label, a planted case the model decides, the options and the entry point.
synthetic_rows(), planted_case() and collision_lm() are also what tests/test_ctc_lm_gpu.py holds mrn_ctc_beam_lm_decode_f32 against."""
import copy
import ctypes
import itertools
import types

import numpy as np
import pytest

from tests.test_ctc_beam_cpu import brute_force, ctc_converter, make_logits, n_best

DISCOUNT = 0.75


def synthetic_rows(C_lm, n_texts, seed, max_len=9):
    """texts as rows of classes 1 .. C_lm - 1: a random first class, then with probability 0.7 the class a fixed random successor
    table names, else a random one -- some n-grams frequent, most unseen"""
    rng = np.random.default_rng(seed)
    follow = rng.integers(1, C_lm, size=C_lm)
    rows = []
    for _ in range(n_texts):
        row = [int(rng.integers(1, C_lm))]
        for _ in range(int(rng.integers(0, max_len))):
            row.append(int(follow[row[-1]]) if rng.random() < 0.7 else int(rng.integers(1, C_lm)))
        rows.append(row)
    return rows


def synthetic_lm(C_lm, order, seed=5, n_texts=60):
    from mrn_amd.modules.char_lm import lm_from_rows
    return lm_from_rows(synthetic_rows(C_lm, n_texts, seed), C_lm, order, DISCOUNT)


def planted_case():
    """(x [1][4][4], lm): class 1 is certain in frame 0, classes 2 and 3 have the same logit in frame 1, then blanks; the model has
    seen "1 3" only.  Acoustically (1, 2) and (1, 3) tie bit for bit and the tie order (the lower class) picks (1, 2)"""
    from mrn_amd.modules.char_lm import lm_from_rows
    x = np.full((1, 4, 4), -6.0, dtype=np.float32)
    x[0, 0, 1] = 6.0
    x[0, 1, 2] = x[0, 1, 3] = 6.0
    x[0, 2:, 0] = 6.0
    return x, lm_from_rows([[1, 3]] * 5, 4, 3, DISCOUNT)


def collision_lm(C_lm=21, n=8):
    """an order-3 model whose table is n trigrams that all hash to one slot of a 2 n-slot table (load 0.5, a probe sequence of n),
    over the unigram arrays of a synthetic model; the trigrams start in (0, 0), (0, b) and (a, b) contexts so a decoder meets them"""
    from mrn_amd.modules.char_lm import CharLM, make_key, mix
    base = synthetic_lm(C_lm, 1)
    mask, chosen, home = 2 * n - 1, {}, None
    grams = [(0, 0, c) for c in range(1, C_lm)] + [(0, b, c) for b in range(1, C_lm) for c in range(1, C_lm)]
    grams += list(itertools.product(range(1, C_lm), repeat=3))
    by_slot = {}
    for g in grams:
        by_slot.setdefault(mix(make_key(*g)) & mask, []).append(g)
    home = max(by_slot, key=lambda s: (any(g[1] == 0 for g in by_slot[s]), len(by_slot[s])))
    for i, g in enumerate(by_slot[home][:n]):
        chosen[g] = (-0.25 * (i + 1), 0.0)
    assert len(chosen) == n
    return CharLM(3, base.uni_logp, base.uni_bow, base.unk_logp, {}, chosen)


def interpolated(rows, C_lm, order, discount, a, b, c):
    """p_order(c | a, b) by the interpolated formula evaluated directly on raw counts the test takes itself: what the stored form
    must equal.  c may be a symbol never seen anywhere (also one outside the model: it has no count either)"""
    counts = [{} for _ in range(order)]                       # level n: {context of n - 1 classes: {symbol: count}}
    for row in rows:
        padded = [0] * (order - 1) + list(row) + [0]
        for i in range(order - 1, len(padded)):
            for n in range(order):
                seen = counts[n].setdefault(tuple(padded[i - n:i]), {})
                seen[padded[i]] = seen.get(padded[i], 0) + 1
    uni = counts[0][()]
    total = sum(uni.values())
    p = max(uni.get(c, 0) - discount, 0.0) / total + discount * len(uni) / total / C_lm
    for n, ctx in ((1, (b,)), (2, (a, b))):
        seen = counts[n].get(ctx) if n < order else None
        if seen is not None:
            cnt = sum(seen.values())
            p = max(seen.get(c, 0) - discount, 0.0) / cnt + discount * len(seen) / cnt * p
    return p


# ---- 1. the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
def test_normalisation_and_the_interpolated_formula(order):
    from mrn_amd.modules.char_lm import check_char_lm, lm_from_rows
    C = 9
    rows = synthetic_rows(C, 40, seed=3)
    lm = lm_from_rows(rows, C, order, DISCOUNT)
    check_char_lm(lm)
    seen3 = sorted(lm.trigrams)[:4] if order == 3 else []
    contexts = [(0, 0), (0, rows[0][0]), tuple(rows[1][:2]) if len(rows[1]) > 1 else (0, 0)] + [g[:2] for g in seen3]
    unseen = [(a, b) for a in range(1, C) for b in range(1, C) if (a, b) not in lm.bigrams][:3] + [(C + 2, 1), (1, C + 7), (C, C)]
    assert unseen[0] not in lm.bigrams
    for a, b in contexts + unseen:
        p = [np.exp(lm.logp(a, b, c)) for c in range(C)]
        assert abs(sum(p) - 1.0) <= 1e-12, (a, b, sum(p))                       # a distribution over the model's own V symbols
        for c in range(C):
            assert abs(p[c] - interpolated(rows, C, order, DISCOUNT, a, b, c)) <= 1e-12, (a, b, c)
        # a class outside the model is scored as a never-seen symbol: every such class the same, n of them add n times that mass
        outside = np.exp(lm.logp(a, b, C))
        assert lm.logp(a, b, C + 40) == lm.logp(a, b, C) and np.isfinite(lm.logp(a, b, C))
        assert abs(outside - interpolated(rows, C, order, DISCOUNT, a, b, C)) <= 1e-12
        assert abs(sum(p) + 7 * outside - (1.0 + 7 * interpolated(rows, C, order, DISCOUNT, a, b, C))) <= 1e-12
    total = sum(len(r) + 1 for r in rows)
    seen1 = len({c for r in rows for c in r} | {0})
    assert abs(lm.unk_logp - (np.log(1.0 / C) + np.log(DISCOUNT * seen1 / total))) <= 1e-12
    if order == 1:
        assert lm.logp(3, 4, 2) == lm.logp(0, 0, 2)                               # lower orders ignore the longer context
    if order == 2:
        assert lm.logp(3, 4, 2) == lm.logp(7, 4, 2) and not lm.trigrams


def test_build_from_strings():
    from mrn_amd.modules.char_lm import build_char_lm, lm_from_rows
    conv = ctc_converter(5)                                                        # 9 classes
    ch = conv.character
    texts = [ch[4] + ch[5], ch[5] + ch[6] + ch[4], "x" + ch[4], ch[8], "[UNK]"]
    lm = build_char_lm(conv, texts, order=3)
    assert lm.dropped == 2 and lm.C_lm == 9 and lm.order == 3
    same = lm_from_rows([[4, 5], [5, 6, 4], [8]], 9, 3, 0.75)
    assert same.bigrams == lm.bigrams and same.trigrams == lm.trigrams and np.array_equal(same.uni_logp, lm.uni_logp)
    with pytest.raises(ValueError, match="none of the 2 texts"):
        build_char_lm(conv, ["xyz", "q"])
    with pytest.raises(ValueError, match="order"):
        build_char_lm(conv, texts, order=4)
    with pytest.raises(ValueError, match="sequence of str"):
        build_char_lm(conv, "abc")


# ---- 2. the table ------------------------------------------------------------------------------------------------------------------
def test_table_finds_what_is_stored_and_nothing_else():
    from mrn_amd.modules.char_lm import check_char_lm, find, make_key
    lm = synthetic_lm(21, 3)
    keys, vals, max_probe = lm.table()
    size = len(keys)
    assert size & (size - 1) == 0 and 2 * (len(lm.bigrams) + len(lm.trigrams)) <= size and keys.dtype == np.uint64
    assert vals.dtype == np.float32 and vals.shape == (size, 2) and max_probe >= 1
    longest = 0
    for gram, (logp, bow) in list(lm.bigrams.items()) + list(lm.trigrams.items()):
        s = find(keys, max_probe, make_key(*gram))
        assert s >= 0 and vals[s, 0] == np.float32(logp) and vals[s, 1] == np.float32(bow), gram
        longest = max(longest, next(p for p in range(1, max_probe + 1) if find(keys, p, make_key(*gram)) >= 0))
    assert longest == max_probe
    absent = [g for g in itertools.product(range(21), repeat=3) if g not in lm.trigrams][:500]
    assert all(find(keys, max_probe, make_key(*g)) == -1 for g in absent)
    assert all(find(keys, max_probe, make_key(b, c)) == -1 for b in range(21) for c in range(21) if (b, c) not in lm.bigrams)
    assert check_char_lm(lm) == (size, len(lm.bigrams) + len(lm.trigrams))


def test_forced_collisions_round_trip():
    from mrn_amd.modules.char_lm import build_table, check_char_lm, find, make_key, mix
    lm = collision_lm()
    keys, vals, max_probe = lm.table()
    assert len(keys) == 16 and max_probe == 8 and len({mix(make_key(*g)) & 15 for g in lm.trigrams}) == 1
    for g, (logp, _) in lm.trigrams.items():
        assert vals[find(keys, max_probe, make_key(*g)), 0] == np.float32(logp)
        assert lm.logp(*g) == logp
    check_char_lm(lm)
    rng = np.random.default_rng(0)                                                 # many keys at load 0.5
    entries = {make_key(int(a), int(b), int(c)): (float(-i), float(i)) for i, (a, b, c) in enumerate(rng.integers(0, 6000, size=(2048, 3)))}
    keys, vals, max_probe = build_table(entries, size=2 * len(entries) if len(entries) == 2048 else None)
    assert 2 * len(entries) <= len(keys)
    for key, v in entries.items():
        assert tuple(vals[find(keys, max_probe, key)]) == v
    assert int((keys != 0).sum()) == len(entries)


def test_check_rejects_every_malformation():
    from mrn_amd.modules.char_lm import CharLM, check_char_lm
    good = synthetic_lm(21, 3)
    check_char_lm(good)

    def broken(**attrs):
        lm = copy.copy(good)
        for k, v in attrs.items():
            setattr(lm, k, v)
        return lm

    n = len(good.keys)
    moved_keys = good.keys.copy()
    s = int(np.flatnonzero(moved_keys)[0])
    free = next(i for i in range(n) if moved_keys[(s + n // 2 + i) % n] == 0)
    moved_keys[(s + n // 2 + free) % n], moved_keys[s] = moved_keys[s], 0        # the key sits far behind its probe sequence
    nan_vals = good.vals.copy()
    nan_vals[int(np.flatnonzero(good.keys)[0]), 0] = np.nan
    inf_uni = good.uni_logp.copy()
    inf_uni[3] = -np.inf
    for match, lm in (("power of two", broken(keys=np.concatenate([good.keys, good.keys[:n // 2]]),
                                              vals=np.concatenate([good.vals, good.vals[:n // 2]]))),
                      ("not reachable within max_probe", broken(max_probe=0)),
                      ("not reachable within max_probe", broken(keys=moved_keys)),
                      ("non-finite", broken(vals=nan_vals)),
                      ("non-finite", broken(uni_logp=inf_uni)),
                      ("non-finite", broken(unk_logp=-np.inf)),
                      ("above 65535", CharLM(1, np.full(65536, -11.1), np.zeros(65536), -11.1)),
                      ("order 0", broken(order=0)),
                      ("order 4", broken(order=4)),
                      ("order True", broken(order=True))):
        with pytest.raises(ValueError, match=match):
            check_char_lm(lm)
    check_char_lm(CharLM(1, np.full(65535, -11.1), np.zeros(65535), -11.1))          # the largest model; an empty table


# ---- 3. the host form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "planted"])
@pytest.mark.parametrize("T,C,W,K", [(9, 21, 3, 4), (31, 37, 4, 8), (31, 37, 16, 15), (31, 5, 16, 15), (4, 3, 16, 2)])
def test_without_weights_the_host_form_is_unchanged(T, C, W, K, kind):
    from mrn_amd.modules.decoding import ctc_beam_host
    x = make_logits(kind, 2, T, C, 1000)
    plain = ctc_beam_host(x, W, K)
    assert len(plain) == 5
    for lm in (synthetic_lm(C, 3), synthetic_lm(max(C - 2, 2), 2)):
        named = ctc_beam_host(x, W, K, lm=None, lm_weight=0.7, lm_bonus=0.3)         # without a model the weights are not read
        fused = ctc_beam_host(x, W, K, lm=lm, lm_weight=0.0, lm_bonus=0.0)
        assert len(named) == 5 and len(fused) == 6
        for a, b, c in zip(plain, named, fused):
            assert a.dtype == b.dtype == c.dtype and a.tobytes() == b.tobytes() == c.tobytes()
        live = fused[1] >= 0
        assert np.array_equal(fused[5][live], fused[2][live]) and np.isneginf(fused[5][~live]).all()


def fused_brute_force(x, lm, alpha, beta):
    """{label: log p_ctc + alpha * (lm + eos) + beta * len} over every label of x [T][C]"""
    out = {}
    for label, acoustic in brute_force(x).items():
        ctx = (0, 0) + label
        lm_sum = sum(lm.logp(ctx[i], ctx[i + 1], ctx[i + 2]) for i in range(len(label))) + lm.logp(ctx[-2], ctx[-1], 0)
        out[label] = acoustic + alpha * lm_sum + beta * len(label)
    return out


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("T,C,W", [(4, 4, 128), (5, 3, 64)])
def test_host_equals_the_fused_brute_force_when_nothing_is_pruned(T, C, W, order):
    from mrn_amd.modules.decoding import ctc_beam_host
    lm = synthetic_lm(C, order, seed=11, n_texts=12)
    for seed, (alpha, beta) in enumerate([(0.5, 0.0), (1.3, 0.4), (0.8, -0.6), (3.0, 1.0)]):
        x = (2.0 * np.random.default_rng(seed).standard_normal((1, T, C))).astype(np.float32)
        exact = fused_brute_force(x[0], lm, alpha, beta)
        acoustic = brute_force(x[0])
        assert len(exact) <= W
        tokens, length, score, path, prob, fused = ctc_beam_host(x, W, C - 1, lm=lm, lm_weight=alpha, lm_bonus=beta)
        got = n_best(tokens[0], length[0], fused[0])
        assert {p for p, _ in got} == set(exact)
        best = max(exact, key=exact.get)
        assert got[0][0] == best and abs(got[0][1] - exact[best]) <= 1e-12
        assert all(abs(s - exact[p]) <= 1e-9 for p, s in got) and (np.diff(fused[0, :len(got)]) <= 0).all()
        for (p, _), s in zip(got, score[0]):
            assert abs(s - acoustic[p]) <= 1e-9                                     # score stays the acoustic log-probability
        assert prob[0, 0] == np.float32(np.exp(score[0, 0]))


def test_the_model_decides_a_planted_tie():
    from mrn_amd.modules.decoding import ctc_beam_host
    x, lm = planted_case()
    for dtype in (np.float64, np.float32):
        tokens, length, score, _, _, _ = ctc_beam_host(x, 4, 3, lm=lm, lm_weight=0.0, dtype=dtype)
        assert n_best(tokens[0], length[0], score[0])[0][0] == (1, 2)               # the acoustic tie order
        assert score[0, 0] == score[0, 1] and tuple(tokens[0, 1, :2]) == (1, 3)
        tokens, length, score, path, _, fused = ctc_beam_host(x, 4, 3, lm=lm, lm_weight=0.5, dtype=dtype)
        assert n_best(tokens[0], length[0], score[0])[0][0] == (1, 3)
        assert path[0].tolist() == [1, 3, 0, 0] and fused[0, 0] > fused[0, 1]


def test_float32_host_form_runs_in_float32():
    from mrn_amd.modules.decoding import ctc_beam_host
    x = make_logits("planted", 2, 31, 37, 5)
    lm = synthetic_lm(37, 3)
    f32 = ctc_beam_host(x, 8, 15, lm=lm, lm_weight=0.5, lm_bonus=0.1, dtype=np.float32)
    f64 = ctc_beam_host(x, 8, 15, lm=lm, lm_weight=0.5, lm_bonus=0.1)
    live = f32[1] >= 0
    assert np.array_equal(f32[5][live], f32[5][live].astype(np.float32))             # every value is a float32
    assert np.array_equal(f32[2][live], f32[2][live].astype(np.float32))
    d = np.abs(f32[5][:, 0] - f64[5][:, 0]).max()
    assert 0 < d < 1e-3
    plain32 = ctc_beam_host(x, 8, 15, dtype=np.float32)
    assert len(plain32) == 5 and 0 < np.abs(plain32[2][:, 0] - ctc_beam_host(x, 8, 15)[2][:, 0]).max() < 1e-3


# ---- 4. the surface ------------------------------------------------------------------------------------------------------------------
def test_options_and_bad_weights():
    from mrn_amd.modules import decoding as D
    lm = synthetic_lm(9, 2)
    ns = types.SimpleNamespace
    assert D.lm_options(ns(), False) == (None, 0.5, 0.0)
    assert D.lm_options(ns(ctc_decode="beam", ctc_lm=lm), False) == (lm, 0.5, 0.0)
    assert D.lm_options(ns(ctc_decode="beam", ctc_lm=lm, lm_weight=1, lm_bonus=-0.25), False) == (lm, 1.0, -0.25)
    assert D.lm_options(ns(ctc_lm=lm, lm_weight=-1), True) == (None, 0.5, 0.0)      # the attention head ignores the option
    assert D.lm_options(ns(lm_weight=-1, lm_bonus="x"), False) == (None, 0.5, 0.0)  # read only with a model
    for bad in (ns(ctc_lm=lm), ns(ctc_lm=lm, ctc_decode="greedy")):
        with pytest.raises(ValueError, match="ctc_decode='beam'"):
            D.lm_options(bad, False)
    with pytest.raises(ValueError, match="ctc_lm and lexicon"):
        D.lm_options(ns(ctc_lm=lm, ctc_decode="beam", lexicon=["a"]), False)
    with pytest.raises(ValueError, match="ctc_lm and candidates"):
        D.lm_options(ns(ctc_lm=lm, ctc_decode="beam", candidates={}), False)
    with pytest.raises(ValueError, match="must be a CharLM"):
        D.lm_options(ns(ctc_lm="model.arpa", ctc_decode="beam"), False)
    x = make_logits("noise", 1, 5, 9, 3)
    for kw in (dict(lm_weight=-0.1), dict(lm_weight=np.inf), dict(lm_weight=np.nan), dict(lm_bonus=np.inf), dict(lm_bonus=np.nan),
               dict(lm_weight="1"), dict(lm_bonus=None), dict(lm_weight=True)):
        with pytest.raises(ValueError, match="lm_weight|lm_bonus"):
            D.ctc_beam_host(x, 4, 4, lm=lm, **kw)
        with pytest.raises(ValueError, match="lm_weight|lm_bonus"):
            D.lm_options(ns(ctc_lm=lm, ctc_decode="beam", **kw), False)
    with pytest.raises(ValueError, match="dtype"):
        D.ctc_beam_host(x, 4, 4, dtype=np.float16)
    assert D.beam_lm_supported(lm)


def test_validation_refuses_the_option_combinations():
    """validation() reads the options before it touches the model or the loader"""
    from mrn_amd.test import validation
    lm = synthetic_lm(9, 2)
    conv = ctc_converter(5)
    base = dict(Prediction="CTC", batch_max_length=25)
    for keys, match in ((dict(ctc_lm=lm), "ctc_decode='beam'"), (dict(ctc_lm=lm, ctc_decode="beam", candidates={}), "ctc_lm|candidates"),
                        (dict(ctc_lm=lm, ctc_decode="beam", lexicon=["a"]), "lexicon"),
                        (dict(ctc_lm=lm, ctc_decode="beam", lm_weight=-2.0), "lm_weight")):
        with pytest.raises(ValueError, match=match):
            validation(object(), None, [], conv, types.SimpleNamespace(**base, **keys))


def test_entry_point_is_declared_exported_and_cited():
    """include/mrn_ctc_lm.h is parsed and bound like include/mrn_hip.h: the prototype there, the symbol in the library, the reference
    op site in its comment, the entry point in the README"""
    import os
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header(_lib.CTC_LM_HEADER_PATH)
    assert list(protos) == ["mrn_ctc_beam_lm_decode_f32"]
    ret, argtypes, argnames = protos["mrn_ctc_beam_lm_decode_f32"]
    beam = _lib.parse_header(_lib.DECODE_HEADER_PATH)["mrn_ctc_beam_decode_f32"]
    assert ret == "int" and argnames[:13] == beam[2][:13] and argtypes[:13] == beam[1][:13]      # the beam decoder's operands first
    assert argnames[13:] == ["lm_keys", "lm_vals", "lm_mask", "lm_max_probe", "uni_logp", "uni_bow", "C_lm", "unk_logp", "order", "alpha",
                             "beta", "fused", "stream"]
    assert argtypes[13:] == ["const void*", "const float*", "int64_t", "int", "const float*", "const float*", "int", "float", "int",
                             "float", "float", "float*", "void*"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mrn_ctc_beam_lm_decode_f32")
    others = [p for k, p in vars(_lib).items() if k.endswith("HEADER_PATH") and p != _lib.CTC_LM_HEADER_PATH]
    assert len(others) >= 8 and not any(set(protos) & set(_lib.parse_header(p)) for p in others)
    bound = _lib.LIB.load().mrn_ctc_beam_lm_decode_f32
    assert bound.restype is ctypes.c_int and len(bound.argtypes) == 26
    header = open(_lib.CTC_LM_HEADER_PATH).read()
    comment = header[:header.index("int mrn_ctc_beam_lm_decode_f32(")].rsplit("/*", 1)[1]
    assert "test.py:211-219" in comment and "1 <= T <= 512" in comment and "C_lm <= 65535" in comment and "2^26" in comment
    readme = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), os.pardir, "README.md")).read()
    assert "mrn_ctc_beam_lm_decode_f32" in readme and "include/mrn_ctc_lm.h" in readme
