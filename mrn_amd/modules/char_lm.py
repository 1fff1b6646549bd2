"""A character n-gram language model for the CTC prefix beam search (pure numpy, float64: importable without a GPU).

Tokens are the CTC converter's class indices.  Class 0, the blank, never occurs in a prefix, so it doubles as the padding symbol: a
context is padded on the left with order - 1 zeros (begin of text), and a PREDICTED 0 is the end of text.  A text c_1 .. c_L is
counted as the padded row 0 .. 0 c_1 .. c_L 0; every position behind the padding is one event at every level (raw counts: the
trigram, the bigram and the unigram that end there), so the context counts of a level are the sums of its own events.

Estimate: interpolated absolute discounting with one discount D at every level,

    p_n(c | ctx) = max(cnt(ctx, c) - D, 0) / cnt(ctx) + D * N1+(ctx) / cnt(ctx) * p_{n-1}(c | ctx'),     p_n = p_{n-1} where cnt(ctx) = 0,
    p_1(c)       = max(cnt(c) - D, 0) / total + D * N1+ / total / V,

N1+(ctx) the number of distinct symbols seen behind ctx, ctx' the context without its oldest symbol, and V = C_lm the number of
predictable symbols: the classes 1 .. C_lm - 1 and the end of text.  Over those V symbols every p_n sums to one.

Stored form: back-off (ARPA) form, which evaluates to exactly the interpolated value.  Dense uni_logp [C_lm] (entry 0 = end of text)
and uni_bow [C_lm] (log of D * N1+(b) / cnt(b) of the one-symbol context b, 0 = log 1 for an unseen one; entry 0 = begin of text);
every seen bigram (b, c) stores (log p_2(c | b), bow) with bow = log of D * N1+(b, c) / cnt(b, c) of the PAIR as a context (0 where it
was never one), and every seen trigram stores (log p_3, 0).  The one pair that is a context without being an event, (0, 0) = begin of
text, is stored as a bigram too, with the log p_2(0 | 0) the back-off would have computed.

Classes outside the model.  A decoder may have more classes than the model (C > C_lm).  A class c >= C_lm is scored as a symbol of
the model that was never seen would be at the unigram level,

    unk_logp = log(1 / V) + log(D * N1+ / total),

finite, and reached through the ordinary back-off chain (no n-gram with such a class is stored, and uni_bow of such a class is 0).
The model stays a distribution over its OWN V symbols; n classes outside it add n * exp(logp(a, b, outside)) on top of the 1:
out-of-model classes are not paid for by the in-model ones.  build_char_lm's C_lm is the converter's class count, so this only
happens with a model built for a smaller character set.

Evaluation, logp(a, b, c) with a the class before b (order 3; order 2 ignores a, order 1 ignores a and b):

    trigram (a, b, c) stored          -> its logp;
    bo = bow of bigram (a, b) if stored else 0;
    bigram (b, c) stored              -> bo + its logp;
    otherwise                         -> bo + (ubow(b) + uni(c)),     uni(c) = uni_logp[c] if c < C_lm else unk_logp,
                                                                         ubow(b) = uni_bow[b] if b < C_lm else 0.

Device form, table(): one open-addressing hash table.  key = n << 60 | a << 32 | b << 16 | c, n = 2 (a = 0) or 3; 0 marks an empty
slot (no stored key is 0: n >= 2).  Values float32 (logp, bow).  size = a power of two with load <= 0.5; slot = mix(key) & (size - 1),
collisions by linear probing; max_probe = the longest probe sequence of any stored key (slots examined, the hit included), so a
lookup that has examined max_probe slots without a hit is a miss.  The hash is the splitmix64 finaliser:

    h = key;  h ^= h >> 30;  h *= 0xBF58476D1CE4E5B9;  h ^= h >> 27;  h *= 0x94D049BB133111EB;  h ^= h >> 31      (mod 2^64)

stated here (mix) and in mrn_amd/csrc/char_lm.hpp (lm_mix), the header both kernels that read the table include, nowhere else.

On an attention head (AttnLabelConverter) the same holds with class 0 = [UNK] in the blank's place: encode_texts bans it, so it never
occurs in a text and doubles as begin / end of text; [PAD], [SOS] and [EOS] never occur either and sit at the unigram floor
(modules/decoding.py, "Language-model fusion on the attention head").
"""
import numpy as np

MAX_ORDER = 3
MAX_CLASSES = 65535          # classes are 16-bit fields of a key
MAX_TABLE_SLOTS = 1 << 26
_M64 = (1 << 64) - 1


def mix(key):
    """the 64-bit hash of a key: an int -> int, a uint64 array -> uint64 array (array arithmetic wraps mod 2^64)"""
    h = np.atleast_1d(np.asarray(key, dtype=np.uint64)).copy()
    h ^= h >> np.uint64(30)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(27)
    h *= np.uint64(0x94D049BB133111EB)
    h ^= h >> np.uint64(31)
    return h if isinstance(key, np.ndarray) else int(h[0])


def make_key(*gram):
    """(b, c) or (a, b, c) -> the uint64 key as an int"""
    if len(gram) == 2:
        return 2 << 60 | gram[0] << 16 | gram[1]
    return 3 << 60 | gram[0] << 32 | gram[1] << 16 | gram[2]


def build_table(entries, size=None):
    """{key: (logp, bow)} -> (keys uint64 [size], vals float32 [size][2], max_probe).  size = the smallest power of two >= twice the
    number of keys (at least 2) unless given; keys are inserted in ascending order, so the table is a function of its contents"""
    n = len(entries)
    if size is None:
        size = 2
        while size < 2 * n:
            size *= 2
    if size < 1 or size & (size - 1) or n > size:
        raise ValueError(f"build_table: size {size} must be a power of two and hold {n} keys")
    keys = np.zeros(size, dtype=np.uint64)
    vals = np.zeros((size, 2), dtype=np.float32)
    mask, max_probe = size - 1, 0
    ordered = sorted(entries)
    if ordered and not 0 < ordered[0] <= ordered[-1] <= _M64:
        raise ValueError("build_table: a key outside 1..2^64-1")
    homes = (mix(np.array(ordered, dtype=np.uint64)) & np.uint64(mask)).tolist()
    for key, s in zip(ordered, homes):
        probes = 1
        while keys[s] != 0:
            s, probes = (s + 1) & mask, probes + 1
        keys[s] = key
        vals[s] = entries[key]
        max_probe = max(max_probe, probes)
    return keys, vals, max_probe


def find(keys, max_probe, key):
    """the slot of `key` in a table, or -1: what the kernel's bounded probe does"""
    mask = len(keys) - 1
    s = mix(key) & mask
    for _ in range(int(max_probe)):
        k = int(keys[s])
        if k == key:
            return s
        if k == 0:
            return -1
        s = (s + 1) & mask
    return -1


class CharLM:
    """the stored form: order, uni_logp / uni_bow float64 [C_lm], unk_logp, bigrams {(b, c): (logp, bow)}, trigrams {(a, b, c): (logp,
    0.0)}, and the device form built from them (keys, vals, max_probe; table()).  dropped = texts build_char_lm could not spell"""

    def __init__(self, order, uni_logp, uni_bow, unk_logp, bigrams=None, trigrams=None, dropped=0):
        self.order = order
        self.uni_logp = np.ascontiguousarray(uni_logp, dtype=np.float64)
        self.uni_bow = np.ascontiguousarray(uni_bow, dtype=np.float64)
        self.unk_logp = float(unk_logp)
        self.bigrams = dict(bigrams or {}) if order >= 2 else {}
        self.trigrams = dict(trigrams or {}) if order >= 3 else {}
        self.dropped = dropped
        entries = {make_key(*g): v for g, v in self.bigrams.items()}
        entries.update({make_key(*g): v for g, v in self.trigrams.items()})
        self.keys, self.vals, self.max_probe = build_table(entries)

    @property
    def C_lm(self):
        return len(self.uni_logp)

    def table(self):
        """(keys uint64 [size], vals float32 [size][2], max_probe)"""
        return self.keys, self.vals, self.max_probe

    def logp(self, a, b, c, dtype=np.float64):
        """log p(c | a, b) by the back-off evaluation of the module docstring; c = 0 is the end of text, a = b = 0 the begin.  In
        float32 the stored values are the table's (rounded once) and the sums are float32 sums in the kernel's order"""
        f = dtype
        C = self.C_lm
        uni = f(self.uni_logp[c]) if c < C else f(self.unk_logp)
        if self.order == 1:
            return uni
        bo = f(0)
        if self.order == 3:
            hit = self.trigrams.get((a, b, c))
            if hit is not None:
                return f(hit[0])
            ctx = self.bigrams.get((a, b))
            if ctx is not None:
                bo = f(ctx[1])
        hit = self.bigrams.get((b, c))
        if hit is not None:
            return bo + f(hit[0])
        return bo + ((f(self.uni_bow[b]) if b < C else f(0)) + uni)


def check_char_lm(lm):
    """the host check every model passes once before it is uploaded (ops.upload_char_lm): the kernel trusts the arrays, so whatever
    could send a read outside them, make a probe miss a stored key or put a non-finite number into a ranking key is a ValueError here.
    -> (size, number of stored keys)"""
    if isinstance(lm.order, bool) or not isinstance(lm.order, (int, np.integer)) or not 1 <= lm.order <= MAX_ORDER:
        raise ValueError(f"char_lm: order {lm.order!r} outside 1..{MAX_ORDER}")
    for name in ("uni_logp", "uni_bow"):
        a = getattr(lm, name)
        if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.ndim != 1 or not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"char_lm: {name} must be a contiguous one-dimensional float64 array")
    C = len(lm.uni_logp)
    if len(lm.uni_bow) != C or C < 1:
        raise ValueError(f"char_lm: uni_logp and uni_bow must have the same length >= 1, got {C} and {len(lm.uni_bow)}")
    if C > MAX_CLASSES:
        raise ValueError(f"char_lm: C_lm = {C} above {MAX_CLASSES} (classes are 16-bit fields of a key)")
    keys, vals, max_probe = lm.keys, lm.vals, lm.max_probe
    if not isinstance(keys, np.ndarray) or keys.dtype != np.uint64 or keys.ndim != 1 or not keys.flags["C_CONTIGUOUS"]:
        raise ValueError("char_lm: keys must be a contiguous one-dimensional uint64 array")
    size = len(keys)
    if size < 1 or size & (size - 1) or size > MAX_TABLE_SLOTS:
        raise ValueError(f"char_lm: table size {size} must be a power of two in 1..2^26")
    if not isinstance(vals, np.ndarray) or vals.dtype != np.float32 or vals.shape != (size, 2) or not vals.flags["C_CONTIGUOUS"]:
        raise ValueError(f"char_lm: vals must be a contiguous float32 array [{size}][2]")
    if isinstance(max_probe, bool) or not isinstance(max_probe, (int, np.integer)) or not 0 <= max_probe <= size:
        raise ValueError(f"char_lm: max_probe {max_probe!r} outside 0..{size}")
    used = np.flatnonzero(keys)
    if 2 * len(used) > size:
        raise ValueError(f"char_lm: {len(used)} keys in {size} slots, a load above 0.5")
    finite = (np.isfinite(lm.uni_logp).all() and np.isfinite(lm.uni_bow).all() and np.isfinite(vals[used]).all()
              and np.isfinite(lm.unk_logp) and np.isfinite(np.float32(lm.unk_logp))
              and np.isfinite(lm.uni_logp.astype(np.float32)).all() and np.isfinite(lm.uni_bow.astype(np.float32)).all())
    if not finite:
        raise ValueError("char_lm: non-finite log-probability or back-off weight")
    # every stored key at once (a model is checked once per validation() call: no per-key Python)
    k = keys[used]
    u = np.uint64
    n, a, b, c = k >> u(60), k >> u(32) & u(0xFFFF), k >> u(16) & u(0xFFFF), k & u(0xFFFF)
    bad = (((n != u(2)) & (n != u(3))) | ((n == u(3)) & (lm.order < 3)) | ((n == u(2)) & (a != u(0)))
           | (k != (n << u(60) | a << u(32) | b << u(16) | c)) | (np.maximum(np.maximum(a, b), c) >= u(C)))
    if bad.any():
        s = int(used[np.flatnonzero(bad)[0]])
        raise ValueError(f"char_lm: slot {s} holds {int(keys[s]):#x}, no n-gram key of an order-{lm.order} model over {C} classes")
    # key k in slot s is found by the bounded probe iff s is fewer than max_probe slots behind its home slot, no slot from the home
    # slot up to s is empty, and no earlier slot holds the same key
    home = (mix(k) & u(size - 1)).astype(np.int64)
    behind = (used - home) & (size - 1)
    empties = np.concatenate([[0], np.cumsum(keys == 0)])                   # empties[i] = empty slots in front of slot i
    end = home + behind
    between = np.where(end < size, empties[np.minimum(end, size)] - empties[home],
                       empties[size] - empties[home] + empties[np.maximum(end - size, 0)])
    lost = (behind >= max_probe) | (between != 0)
    if not lost.any() and len(np.unique(k)) != len(k):
        order_ = np.argsort(k, kind="stable")
        lost[order_[1:][k[order_][1:] == k[order_][:-1]]] = True
    if lost.any():
        s = int(used[np.flatnonzero(lost)[0]])
        raise ValueError(f"char_lm: the key {int(keys[s]):#x} in slot {s} is not reachable within max_probe = {max_probe}")
    return size, len(used)


def encode_texts(converter, texts):
    """texts -> (rows of classes, dropped): encoded as decoding.encode_lexicon encodes words; a text with a character outside
    converter.dict, or one of the [UNK] / [CTCblank] class, is dropped and counted"""
    table = converter.dict
    banned = {0, table.get("[UNK]")}
    rows, dropped = [], 0
    for text in texts:
        row = [table.get(ch) for ch in text]
        if any(c is None or c in banned for c in row):
            dropped += 1
            continue
        rows.append(row)
    return rows, dropped


def count_ngrams(rows, order):
    """rows of classes -> [counts of level 1, .., level `order`]: level n maps a context tuple of n - 1 classes to {symbol: count}"""
    levels = [{} for _ in range(order)]
    for row in rows:
        padded = [0] * (order - 1) + list(row) + [0]
        for i in range(order - 1, len(padded)):
            for n in range(1, order + 1):
                ctx = tuple(padded[i - n + 1:i])
                seen = levels[n - 1].setdefault(ctx, {})
                seen[padded[i]] = seen.get(padded[i], 0) + 1
    return levels


def lm_from_rows(rows, C_lm, order=3, discount=0.75, dropped=0):
    """rows of classes in 1 .. C_lm - 1 -> CharLM by the estimate of the module docstring"""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= order <= MAX_ORDER:
        raise ValueError(f"char_lm: order {order!r} outside 1..{MAX_ORDER}")
    if not 0.0 < discount <= 1.0:
        raise ValueError(f"char_lm: discount {discount!r} outside (0, 1]: an unseen symbol needs mass")
    if not 1 <= C_lm <= MAX_CLASSES:
        raise ValueError(f"char_lm: C_lm = {C_lm} outside 1..{MAX_CLASSES}")
    rows = [list(map(int, r)) for r in rows]
    if not rows:
        raise ValueError("char_lm: no text to count")
    if any(c < 1 or c >= C_lm for r in rows for c in r):
        raise ValueError(f"char_lm: a class outside 1..{C_lm - 1} in a text")
    D = float(discount)
    levels = count_ngrams(rows, order)
    uni = levels[0][()]
    total, V = sum(uni.values()), C_lm
    gamma1 = D * len(uni) / total
    p1 = np.full(C_lm, gamma1 / V)
    for c, n in uni.items():
        p1[c] += max(n - D, 0.0) / total
    unk_logp = np.log(1.0 / V) + np.log(gamma1)

    def gamma(level, ctx):
        seen = levels[level - 1].get(ctx)
        return None if seen is None else D * len(seen) / sum(seen.values())

    uni_bow = np.zeros(C_lm)
    p2, bigrams, trigrams = {}, {}, {}
    if order >= 2:
        for (b,), seen in levels[1].items():
            uni_bow[b] = np.log(gamma(2, (b,)))
            cnt = sum(seen.values())
            for c, n in seen.items():
                p2[(b, c)] = max(n - D, 0.0) / cnt + gamma(2, (b,)) * p1[c]
        pairs = set(p2)
        if order == 3:
            pairs |= set(levels[2])                    # (0, 0): a context that is no event
        for b, c in pairs:
            p = p2.get((b, c))
            if p is None:
                g = gamma(2, (b,))
                p = p1[c] if g is None else g * p1[c]
            g3 = gamma(3, (b, c)) if order == 3 else None
            bigrams[(b, c)] = (float(np.log(p)), 0.0 if g3 is None else float(np.log(g3)))
    if order == 3:
        for (a, b), seen in levels[2].items():
            cnt, g3 = sum(seen.values()), gamma(3, (a, b))
            for c, n in seen.items():
                lower = p2.get((b, c))
                if lower is None:
                    g = gamma(2, (b,))
                    lower = p1[c] if g is None else g * p1[c]
                trigrams[(a, b, c)] = (float(np.log(max(n - D, 0.0) / cnt + g3 * lower)), 0.0)
    return CharLM(int(order), np.log(p1), uni_bow, unk_logp, bigrams, trigrams, dropped)


def build_char_lm(converter, texts, order=3, discount=0.75):
    """texts (str) -> CharLM over the converter's classes (C_lm = len(converter.character)).  A text the converter cannot spell is
    dropped and counted (lm.dropped); nothing left is a ValueError.  Orders 1, 2 and 3"""
    if isinstance(texts, (str, bytes)) or not hasattr(texts, "__iter__"):
        raise ValueError(f"build_char_lm: texts must be a sequence of str, got {type(texts).__name__}")
    texts = list(texts)
    rows, dropped = encode_texts(converter, texts)
    if not rows:
        raise ValueError(f"build_char_lm: none of the {len(texts)} texts can be spelled with the converter's characters")
    return lm_from_rows(rows, len(converter.character), order, discount, dropped)
