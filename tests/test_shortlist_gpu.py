"""The lexicon-shortlist kernels (mrn_lexicon_shortlist_i32, csrc/lexicon_shortlist.hip) through ops.lexicon_shortlist against the numpy
host form mrn_amd/modules/decoding.py::lexicon_shortlist_host, which tests/test_shortlist_cpu.py holds to the definition.  Everything is
integer arithmetic: cand and dist are compared with ==, element for element, and every case runs the call twice, since nothing in the
result may depend on the order in which atomics land.

The shapes are the smallest at which each part can go wrong: a ragged last wave and a ragged last tile of 256 words, a batch that ends
inside a workgroup's group of 8 samples, hypotheses on both sides of the 32-token (one 32-bit word of state) and 64-token (the host's)
boundaries, word tables of one and of 255 places (eight staged chunks of 32), the largest class, more words at the cut distance than
slots."""
import numpy as np
import pytest
import torch

from tests.test_attn_lexicon_cpu import as_arrays
from tests.test_shortlist_cpu import hyp_arrays, perturbed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops as o
    from mrn_amd._lib import LIB
    LIB.load()
    return o


def recorded_calls(monkeypatch, fn):
    """(fn(), the names of the library calls it made)"""
    from mrn_amd._lib import LIB
    names, real = [], LIB.call
    monkeypatch.setattr(LIB, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.setattr(LIB, "call", real)


def check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, K, max_dist=None, launches=1):
    """the op on the device == the host form, twice over; -> the host form's (cand, dist)"""
    from mrn_amd.modules.decoding import lexicon_shortlist_host
    ref = lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, K, max_dist)
    handle = ops.upload_words(tokens, lengths, "cuda")
    args = (torch.from_numpy(hyp).cuda(), torch.from_numpy(hyp_len).cuda(), handle, K, max_dist)
    got, names = recorded_calls(monkeypatch, lambda: ops.lexicon_shortlist(*args))
    assert names.count("mrn_lexicon_shortlist_i32") == launches
    again = ops.lexicon_shortlist(*args)
    for g, a, r in zip(got, again, ref):
        assert g.is_cuda and g.dtype == torch.int32 and tuple(g.shape) == r.shape
        assert torch.equal(g, a)
        assert np.array_equal(g.cpu().numpy(), r)
    return ref


def random_case(seed, B, N, Lmax, C, Hmax, shortest=0):
    """N random words of U[shortest, Lmax] classes 4 ... C - 1 and B hypotheses: words after up to three edits, clipped to Hmax"""
    rng = np.random.default_rng(seed)
    words = [tuple(int(c) for c in rng.integers(4, C, int(rng.integers(shortest, Lmax + 1)))) for _ in range(N)]
    words[0] = tuple(int(c) for c in rng.integers(4, C, Lmax))                      # the table is Lmax wide
    hyps = [perturbed(rng, words[int(rng.integers(N))], C, int(rng.integers(0, 4)))[:Hmax] for _ in range(B)]
    return words, hyps


@pytest.mark.parametrize("B", [1, 5, 19])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1007])
def test_ragged_waves_tiles_and_sample_groups(ops, monkeypatch, N, B):
    words, hyps = random_case(100 * N + B, B, N, 12, 40, 20)
    hyp, hyp_len = hyp_arrays(hyps, junk=5)
    tokens, lengths = as_arrays(words)
    check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, min(N, 7))
    check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, 50, 4)


def test_hypothesis_lengths_at_the_state_word_boundaries(ops, monkeypatch):
    """0, 1, 31, 32, 33, 63 and 64 tokens; the first group of eight samples stays within 32 tokens (32-bit state), the second does not"""
    rng = np.random.default_rng(7)
    words, _ = random_case(7, 1, 300, 70, 12, 64, shortest=0)
    words += [(), (5,)]
    hyps = []
    for n in (0, 1, 31, 32, 5, 17, 32, 2) + (33, 63, 64, 0, 1, 64, 40, 12) + (64, 32, 0):
        base = words[int(rng.integers(len(words)))]
        hyps.append((tuple(base) + tuple(int(c) for c in rng.integers(4, 12, 70)))[:n])
    hyp, hyp_len = hyp_arrays(hyps, Hmax=64, junk=4)
    tokens, lengths = as_arrays(words)
    assert np.bincount(hyp[10]).max() >= 8                      # eight classes in 64 places: masks with several bits set
    for K, max_dist in ((10, None), (256, None), (10, 30)):
        check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, K, max_dist)


def test_long_hypotheses_are_flagged_and_finished_by_the_host_form(ops, monkeypatch):
    """65 and 300 tokens (and a length beyond Hmax, which is clipped to it) among ordinary ones: the kernel flags them, the op merges the
    host form's rows"""
    from mrn_amd._lib import call
    rng = np.random.default_rng(11)
    words, short = random_case(11, 4, 200, 30, 20, 30)
    long_ones = [tuple(int(c) for c in rng.integers(4, 20, n)) for n in (65, 300, 64, 299)]
    hyps = [short[0], long_ones[0], short[1], long_ones[1], long_ones[2], short[2], long_ones[3], short[3]]
    hyp, hyp_len = hyp_arrays(hyps, Hmax=300, junk=4)
    hyp_len[6] = 5000
    tokens, lengths = as_arrays(words)
    check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, 9)
    check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, 9, 40)
    # the kernel itself: flagged rows are all -1, the others are the host form's, and a negative length is flagged too
    from mrn_amd.modules.decoding import lexicon_shortlist_host
    B, K, N = len(hyps), 9, len(words)
    raw_len = hyp_len.copy()
    raw_len[6], raw_len[0] = 300, -1
    dev = [torch.from_numpy(a).cuda() for a in (hyp, raw_len, tokens, lengths)]
    cand, dist = torch.full((B, K), 7, dtype=torch.int32).cuda(), torch.full((B, K), 7, dtype=torch.int32).cuda()
    flag = torch.full((B,), 7, dtype=torch.int32).cuda()
    work = torch.empty(B * (1024 + (N + 15) // 16 * 16), dtype=torch.uint8).cuda()
    call("mrn_lexicon_shortlist_i32", dev[0].data_ptr(), 300, dev[1].data_ptr(), B, dev[2].data_ptr(), tokens.shape[1], dev[3].data_ptr(), N, K,
         -1, cand.data_ptr(), dist.data_ptr(), flag.data_ptr(), work.data_ptr(), work.numel(), ops._stream())
    flagged = np.array([1, 1, 0, 1, 0, 0, 1, 0], dtype=bool)
    assert np.array_equal(flag.cpu().numpy(), flagged.astype(np.int32))
    ref = lexicon_shortlist_host(hyp, raw_len, tokens, lengths, K)
    assert np.all(cand.cpu().numpy()[flagged] == -1) and np.all(dist.cpu().numpy()[flagged] == -1)
    assert np.array_equal(cand.cpu().numpy()[~flagged], ref[0][~flagged]) and np.array_equal(dist.cpu().numpy()[~flagged], ref[1][~flagged])


@pytest.mark.parametrize("Lmax", [1, 255])
def test_the_narrowest_and_the_widest_word_table(ops, monkeypatch, Lmax):
    """words of 0, 1 and Lmax classes, classes up to 65 534, a word twice, a hypothesis whose classes occur in no word"""
    rng = np.random.default_rng(Lmax)
    pool = [4, 5, 65534, 65533, 40000, 9]
    words = [(), (65534,), tuple(int(c) for c in rng.choice(pool, Lmax))]
    words += [tuple(int(c) for c in rng.choice(pool, int(rng.integers(0, Lmax + 1)))) for _ in range(80)]
    words += [words[2], words[1], ()]
    hyps = [words[2][:64], (65534,), (), (7, 7, 7), tuple(int(c) for c in rng.choice(pool, 64)), (65534, 65533, 65534, 65534, 4),
            perturbed(rng, words[2][:50], 12, 3)]
    hyp, hyp_len = hyp_arrays(hyps, junk=65534)
    tokens, lengths = as_arrays(words)
    assert tokens.shape[1] == Lmax and tokens.max() == 65534
    ref = check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, 12)
    assert ref[1][3, 0] == 3 and ref[0][2, 0] == 0 and ref[1][2, 0] == 0     # no class shared: max(3, L), least for L <= 3; () is word 0
    check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, len(words), 2)


@pytest.mark.parametrize("K", [1, 90, 100, 256])
def test_slot_counts(ops, monkeypatch, K):
    """K = 1, K = N, K > N (the tail is -1) and the largest K"""
    words, hyps = random_case(3, 6, 90, 10, 30, 12)
    hyp, hyp_len = hyp_arrays(hyps)
    ref = check(ops, monkeypatch, hyp, hyp_len, *as_arrays(words), K)
    assert np.all(ref[0][:, 90:] == -1) and np.all(ref[0][:, :min(K, 90)] >= 0)


def test_more_words_at_the_cut_distance_than_slots(ops, monkeypatch):
    """200 one-substitution variants of the hypothesis in shuffled index order, between words further away, over two tiles: the K-th and
    the (K + 1)-th word are equally far, so the tie to the lower index and the index-ordered compaction decide the row"""
    rng = np.random.default_rng(21)
    base = tuple(int(c) for c in rng.integers(4, 30, 14))
    variants = []
    for i in range(200):
        w = list(base)
        w[i % 14] = 30 + i                                                     # a class the hypothesis does not have: distance exactly 1
        variants.append(tuple(w))
    far = [tuple(int(c) for c in rng.integers(4, 30, 9)) for _ in range(330)]
    words = variants + far + [base]
    order = rng.permutation(len(words))
    words = [words[i] for i in order]
    hyps = [base, base[:13], base + (4,), far[0], ()]
    hyp, hyp_len = hyp_arrays(hyps)
    tokens, lengths = as_arrays(words)
    K = 50
    from mrn_amd.modules.decoding import lexicon_shortlist_host
    full = lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, K + 1)
    assert full[1][0, K - 1] == full[1][0, K] == 1 and full[1][0, 0] == 0          # the case proves something: the cut falls inside bin 1
    assert (np.diff(full[0][0, 1:]) > 0).all()
    for k, max_dist in ((K, None), (K, 1), (1, None), (2, None), (201, None), (202, None), (256, 1)):
        check(ops, monkeypatch, hyp, hyp_len, tokens, lengths, k, max_dist)


@pytest.mark.parametrize("max_dist", [0, 1, 3])
def test_the_cut_off(ops, monkeypatch, max_dist):
    """a sample with an exact match, samples one and three edits away, one with no word in range"""
    words, _ = random_case(5, 1, 400, 10, 25, 10, shortest=4)
    rng = np.random.default_rng(5)
    hyps = [words[7], words[300], perturbed(rng, words[9], 25, 1), perturbed(rng, words[350], 25, 3), tuple(range(100, 120)), ()]
    hyp, hyp_len = hyp_arrays(hyps)
    ref = check(ops, monkeypatch, hyp, hyp_len, *as_arrays(words), 6, max_dist)
    assert ref[1][0, 0] == 0 and np.all(ref[0][4] == -1) and np.all(ref[1][4] == -1)           # nothing within 3 of twenty unknown classes
    assert ref[1].max() <= max_dist


def test_a_table_in_chunks_of_samples(ops, monkeypatch):
    """the distance bytes of one call stay within ops.SHORTLIST_WORK_BYTES: a small budget cuts the batch into three launches"""
    words, hyps = random_case(9, 19, 500, 10, 30, 12)
    hyp, hyp_len = hyp_arrays(hyps)
    monkeypatch.setattr(ops, "SHORTLIST_WORK_BYTES", 8 * 512)
    check(ops, monkeypatch, hyp, hyp_len, *as_arrays(words), 20, launches=3)


def test_a_violated_limit_is_an_error_and_launches_nothing(ops, monkeypatch):
    from mrn_amd._lib import LIB, call
    words, hyps = random_case(2, 3, 40, 8, 30, 10)
    hyp, hyp_len = hyp_arrays(hyps)
    tokens, lengths = as_arrays(words)
    B, N, Lmax, Hmax, K = 3, 40, tokens.shape[1], hyp.shape[1], 5
    dev = [torch.from_numpy(a).cuda() for a in (hyp, hyp_len, tokens, lengths)]
    cand, dist = torch.full((B, 256), 7, dtype=torch.int32).cuda(), torch.full((B, 256), 7, dtype=torch.int32).cuda()
    flag = torch.full((B,), 7, dtype=torch.int32).cuda()
    need = LIB.load().mrn_lexicon_shortlist_work_bytes(B, N)
    work = torch.zeros(need, dtype=torch.uint8).cuda()

    def launch(**kw):
        a = dict(hyp=dev[0].data_ptr(), Hmax=Hmax, hyp_len=dev[1].data_ptr(), B=B, lex_tokens=dev[2].data_ptr(), Lmax=Lmax,
                 lex_len=dev[3].data_ptr(), N=N, K=K, max_dist=-1, cand=cand.data_ptr(), dist=dist.data_ptr(), flag=flag.data_ptr(),
                 work=work.data_ptr(), work_bytes=need)
        a.update(kw)
        call("mrn_lexicon_shortlist_i32", *a.values(), ops._stream())

    for kw, match in ((dict(K=0), "K = 0"), (dict(K=257), "K = 257"), (dict(N=0), "N = 0"), (dict(N=(1 << 20) + 1), "outside 1..2\\^20"),
                      (dict(Lmax=0), "Lmax = 0"), (dict(Lmax=256), "Lmax = 256"), (dict(Hmax=-1), "Hmax = -1"), (dict(max_dist=-2), "max_dist = -2"),
                      (dict(hyp=None), "without hypotheses"), (dict(hyp_len=None), "bad operands"), (dict(lex_tokens=None), "bad operands"),
                      (dict(lex_len=None), "bad operands"), (dict(cand=None), "bad operands"), (dict(dist=None), "bad operands"),
                      (dict(flag=None), "bad operands"), (dict(work=None), "bad operands"), (dict(work_bytes=need - 1), "workspace")):
        with pytest.raises(RuntimeError, match=match):
            launch(**kw)
    torch.cuda.synchronize()
    assert (cand == 7).all() and (dist == 7).all() and (flag == 7).all() and (work == 0).all()          # nothing was launched
    launch()                                                                                            # the same operands within the limits
    from mrn_amd.modules.decoding import lexicon_shortlist_host
    ref = lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, K)
    assert np.array_equal(cand.cpu().numpy().reshape(-1)[:B * K].reshape(B, K), ref[0]) and (flag == 0).all()
    # outside the limits the op takes the host form: no launch, the same result
    handle = ops.upload_words(tokens, lengths, "cuda")
    got, names = recorded_calls(monkeypatch, lambda: ops.lexicon_shortlist(dev[0], dev[1], handle, 300))
    wide = lexicon_shortlist_host(hyp, hyp_len, tokens, lengths, 300)
    assert not names and got[0].is_cuda and np.array_equal(got[0].cpu().numpy(), wide[0]) and np.array_equal(got[1].cpu().numpy(), wide[1])
