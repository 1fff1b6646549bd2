"""Shared helpers for the parity tests (CPU and GPU)."""
import os

import numpy as np
import torch

from mrn_amd.tools import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def golden_state_dict(g, seed):
    """Rebuild the reference model's state_dict (key layout from the fixture, values from the generator)."""
    sd = {}
    for k, shp in zip(g["sd_keys"], g["sd_shapes"]):
        k = str(k)
        shape = tuple(int(v) for v in str(shp).split(",")) if str(shp) else ()
        sd[k] = torch.from_numpy(np.array(W.det_param(W.canonical_key(k), shape, seed)))
    return sd


def sub(t, n=4096):
    a = t.detach().cpu().double().numpy().reshape(-1)
    step = max(1, a.size // n)
    return a[::step][:n].astype(np.float32), a.mean(), np.abs(a).mean()


def assert_sub_close(g, name, t, atol=1e-4, rtol=1e-4):
    """Compare a tensor with a stored strided subsample + moments."""
    assert tuple(g[name + "/shape"]) == tuple(t.shape), (name, tuple(g[name + "/shape"]), tuple(t.shape))
    s, mean, absmean = sub(t)
    ref = g[name + "/sub"]
    err = np.abs(s - ref).max()
    tol = atol + rtol * np.abs(ref).max()
    assert err <= tol, f"{name}: max abs err {err:.3e} > tol {tol:.3e}"
    assert abs(mean - float(g[name + "/mean"])) <= atol + rtol * abs(float(g[name + "/absmean"])), name
    return err


def assert_close(name, a, b, atol=1e-4, rtol=1e-4):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    tol = atol + rtol * (np.abs(b).max() if b.size else 0.0)
    assert err <= tol, f"{name}: max abs err {err:.3e} > tol {tol:.3e}"
    return err


def det_inputs(kind, classes, B, seed, noise=False):
    """Same synthetic batch the golden generator used (tests/golden/make_golden.py: run())."""
    if noise:
        image = torch.from_numpy(W.uniform("input:image", (B, 4, 32, 256), -1.0, 1.0, seed))
    else:
        image = torch.from_numpy(W.smooth_image("input:image", (B, 4, 32, 256), seed))
    nspecial = 4 if kind in ("crnn", "svtr") else 5
    nchar = classes[-1] - nspecial
    chars = "".join(chr(0x4E00 + i) for i in range(nchar))
    lens = W.randint("label_len", (B,), 1, 26, seed)
    words = []
    for b in range(B):
        ids = W.randint(f"label_{b}", (int(lens[b]),), 0, nchar, seed)
        words.append("".join(chars[i] for i in ids))
    domain = torch.from_numpy(W.randint("domain", (B,), 0, 2, seed))
    return image, words, chars, domain


def assert_sub_l2(g, name, t, rel=0.05, q=0.99, q_atol=6e-6):
    """Robust comparison for Adam parameter deltas: elements whose gradient is ~0 get a normalised update m/sqrt(v)
    of essentially random sign, so a max-abs check is meaningless there.  Require a small relative L2 error over the
    stored subsample and a tight bound on the q-quantile of the absolute error."""
    assert tuple(g[name + "/shape"]) == tuple(t.shape), name
    s, _, _ = sub(t)
    ref = g[name + "/sub"]
    err = np.abs(s - ref)
    l2 = np.linalg.norm(s - ref) / max(np.linalg.norm(ref), 1e-30)
    assert l2 <= rel, f"{name}: relative L2 error {l2:.3e} > {rel}"
    assert np.quantile(err, q) <= q_atol, f"{name}: {q}-quantile abs err {np.quantile(err, q):.3e} > {q_atol}"
    return l2


def drop_masks(B, seed, tag, n_experts=1):
    """the DropPath draws the golden generator injected into the reference (tests/golden/make_golden.py)"""
    return [[torch.from_numpy(W.randint(f"droppath:{tag}:{e}:{k}", (B,), 0, 2, seed)).float() for k in range(22)]
            for e in range(n_experts)]


class DetLoader:
    """Deterministic stand-in for the reference's Dataset_Manager / Val_Dataset (data/data_manage.py:8-283): every batch is
    a pure function of (tag, seed, call number), so the golden generator (driving the REFERENCE learners) and the tests
    (driving the HIP learners) see byte-identical batches.  Labels are drawn over the characters set by set_characters();
    `oov` appends a character outside every dictionary to the first label of each batch (the [UNK] path)."""

    def __init__(self, B, tag, seed, noise=False, oov=False, n_valid=1):
        self.B, self.tag, self.seed, self.noise, self.oov, self.n_valid = B, tag, seed, noise, oov, n_valid
        self.chars = ""
        self.count = 0
        self.calls = []            # (method, args) log: lets tests assert how a learner drove the loader

    def set_characters(self, chars):
        self.chars = chars

    def _batch(self, n):
        name = f"{self.tag}:{n}"
        if self.noise:
            image = W.uniform(name + ":img", (self.B, 4, 32, 256), -1.0, 1.0, self.seed)
        else:
            image = W.smooth_image(name + ":img", (self.B, 4, 32, 256), self.seed)
        lens = W.randint(name + ":len", (self.B,), 1, 26, self.seed)
        labels = []
        for b in range(self.B):
            ids = W.randint(f"{name}:lab{b}", (int(lens[b]),), 0, len(self.chars), self.seed)
            labels.append("".join(self.chars[i] for i in ids))
        if self.oov:
            labels[0] = (labels[0][:24] + "é")
        return torch.from_numpy(image), labels

    # -- Dataset_Manager interface -------------------------------------------------------------------------
    def init_start(self, *a, **k):
        self.calls.append(("init_start", a))

    def get_dataset(self, taski, memory=None, index_list=None):
        self.calls.append(("get_dataset", (taski, memory, None if index_list is None else [np.asarray(i).copy() for i in index_list])))
        return index_list

    def rehearsal_prev_model(self, taski):
        self.calls.append(("rehearsal_prev_model", (taski,)))
        return self, 500

    def get_batch(self):
        self.count += 1
        return self._batch(self.count - 1)

    def get_batch2(self):
        image, labels = self.get_batch()
        index = tuple(int(v) for v in W.randint(f"{self.tag}:{self.count - 1}:dom", (self.B,), 0, 2, self.seed))
        return image, labels, [index]

    # -- Val_Dataset interface -----------------------------------------------------------------------------
    def create_dataset(self, val_data=None):
        return [self._batch(10_000 + i) for i in range(self.n_valid)]

    def create_list_dataset(self, valid_datas=None):
        return self.create_dataset()


class oracle_dtype:
    """run the CPU oracle in another floating-point precision (float64: the exact-arithmetic yardstick for conditioning
    bands): sets torch's default dtype and casts the oracle's TPS constants"""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        from oracle import mrn_oracle as O
        self.O, self.old = O, O.tps_constants
        dt = self.dtype
        O.tps_constants = lambda *a: tuple(t.to(dt) for t in self.old(*a))
        torch.set_default_dtype(dt)
        return self

    def __exit__(self, *exc):
        torch.set_default_dtype(torch.float32)
        self.O.tps_constants = self.old

    def cast(self, sd):
        return {k: (v.to(self.dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def crafted_validation_case(kind):
    """Two evaluation batches with hand-made logits for validation() (reference test.py:139-279): every scoring branch is hit --
    exact match, a wrong character (fractional normalised edit distance), an out-of-dictionary label character ([UNK] never
    counts as correct), an empty prediction, an empty ground truth and, for the attention head, predictions with an [EOS]
    (pruned there) and without one (the reference then drops the LAST character: prd[:prd.find('[EOS]')] with find = -1).
    Returns (chars, batches [(image, labels)], logits [tensor [B,T,C]]): the stub model returns logits[i] for batch i."""
    chars = "".join(chr(0x4E00 + i) for i in range(36))
    ctc = kind == "crnn"
    T, C = (63, 40) if ctc else (26, 41)
    first = 4 if ctc else 5                                  # index of chars[0] in the converters' tables

    def ids(word):
        return [first + chars.index(c) for c in word]

    def attn_row(tokens):                                    # tokens then [EOS]=3 ... ; None = no [EOS] anywhere
        return (tokens + [3] + [first] * T)[:T]

    def ctc_row(tokens):                                     # every character twice, blanks between characters, then blanks
        seq = []
        for t in tokens:
            seq += [t, t, 0]
        return (seq + [0] * T)[:T]

    w = [chars[:5], chars[3:12], chars[7:9], chars[10:14] + "é", chars[20:23], ""]
    batches, logits = [], []
    for bi in range(2):
        labels = [w[(i + 3 * bi) % len(w)] for i in range(3)] if bi == 0 else [w[3], w[4], w[5]]
        rows = []
        for si, word in enumerate(labels):
            tok = [first + chars.index(c) if c in chars else (2 if ctc else 0) for c in word]          # [UNK] = 2 (CTC) / 0 (Attn)
            case = (bi, si)
            if case == (0, 1):                               # one wrong character
                tok = tok[:2] + [first + 30] + tok[3:]
            if ctc:
                if case == (0, 2):
                    tok = []                                 # all blanks: empty prediction
                rows.append(ctc_row(tok))
            else:
                if case == (0, 2):
                    rows.append(attn_row([]))                # [EOS] first: empty prediction
                elif case == (1, 1):
                    rows.append(([first + 1, first + 2] * T)[:T])      # no [EOS] at all
                else:
                    rows.append(attn_row(tok))
        tgt = torch.tensor(rows, dtype=torch.long)           # [B,T]
        lg = torch.from_numpy(W.uniform(f"crafted:{kind}:{bi}", (len(labels), T, C), -1.0, 1.0, 77))
        lg.scatter_add_(2, tgt.unsqueeze(2), torch.full((len(labels), T, 1), 4.0))
        image = torch.zeros(len(labels), 4, 32, 256)
        batches.append((image, labels))
        logits.append(lg)
    return chars, batches, logits


def fake_text_samples(path, seed=5):
    """deterministic (images, labels) for a dataset directory path such as "rootA/Latin": RGBA uint8 crops of varying size and
    labels over a small alphabet, a few of them longer than batch_max_length (the readers must filter those out)"""
    lang = path.rstrip("/").split("/")[-1]
    n = 37 + 11 * (sum(ord(c) for c in path) % 5)
    alphabet = "abcdefghijklmnopqrstuvwxyz" + lang.lower()
    images, labels = [], []
    for i in range(n):
        name = f"fake:{path}:{i}"
        h = int(W.randint(name + ":h", (1,), 20, 41, seed)[0])
        w = int(W.randint(name + ":w", (1,), 60, 201, seed)[0])
        images.append((W.uniform(name, (h, w, 4), 0.0, 255.999, seed)).astype(np.uint8))
        L = int(W.randint(name + ":len", (1,), 1, 31, seed)[0])          # up to 30 characters: some exceed 25
        ids = W.randint(name + ":lab", (L,), 0, len(alphabet), seed)
        labels.append("".join(alphabet[j] for j in ids))
    return images, labels


def bn_bwd_reference(dz, keep, y, mean, invstd, gamma, dtype=torch.float64):
    """BatchNorm2d(train) backward with the ReLU mask, written out: the yardstick of ops.bn_bwd.  dz, y [..., C] (any leading
    dims: the rows), keep a 0/1 tensor like dz or None (no ReLU), mean / invstd / gamma [C].  Everything is cast to `dtype`
    first (float64: the reference; float32: the baseline a plain fp32 evaluation of the same formula reaches).
    -> dy, dgamma, dbeta, dres with g = dz * keep, xhat = (y - mean) * invstd,
    dy = gamma * invstd * (g - sum(g) / N - xhat * sum(g * xhat) / N), dgamma = sum(g * xhat), dbeta = sum(g), dres = g"""
    C = y.shape[-1]
    dz, y = dz.detach().to(dtype).reshape(-1, C), y.detach().to(dtype).reshape(-1, C)
    mean, invstd, gamma = mean.detach().to(dtype), invstd.detach().to(dtype), gamma.detach().to(dtype)
    g = dz if keep is None else dz * keep.detach().to(dtype).reshape(-1, C)
    n = y.shape[0]
    xhat = (y - mean) * invstd
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dy = gamma * invstd * (g - dbeta / n - xhat * (dgamma / n))
    return dy, dgamma, dbeta, g


def pack_relu_mask(z):
    """uint8 [numel / 4]: bit j of byte i is set when element 4 i + j of z (flattened) is > 0 -- the ReLU mask layout
    scale_shift_act_kernel writes for the backward pass (ops.scale_shift_act pos_mask, ops.bn_bwd zmask)"""
    pos = (z.detach().reshape(-1, 4) > 0).to(torch.uint8)
    return pos[:, 0] | (pos[:, 1] << 1) | (pos[:, 2] << 2) | (pos[:, 3] << 3)


def unpack_relu_mask(mask):
    """inverse of pack_relu_mask: bool [4 * numel]"""
    bits = torch.arange(4, device=mask.device, dtype=torch.uint8)
    return ((mask.reshape(-1, 1) >> bits) & 1).bool().reshape(-1)


def rel_err(got, ref):
    """max |got - ref| relative to max |ref| (absolute where the reference is all zero), in float64"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max())
    return float((got - ref).abs().max()) / (scale if scale > 0 else 1.0)


F32_FLOOR = 4 * 2.0 ** -24        # two fp32 roundings of the result itself: the floor under every "8 x the fp32 baseline" bound


def baseline_bound(ref64, base32, factor=8.0, extra=0.0):
    """the bound within_baseline applies: max(factor * error of the fp32 baseline, 4 * 2^-24, extra), relative to max|reference|"""
    return max(factor * rel_err(base32, ref64), F32_FLOOR, extra)


def within_baseline(name, got, ref64, base32, factor=8.0, extra=0.0):
    """kernel error <= max(factor * error of the fp32 CPU baseline, 4 * 2^-24), both relative to max|reference|; -> the ratio.
    `extra`: a relative tolerance the caller DERIVED for a known property of the kernel's formula (never a measured one), OR-ed
    into the bound"""
    err, e32 = rel_err(got, ref64), rel_err(base32, ref64)
    ratio = err / max(e32, F32_FLOOR / factor)
    print(f"{name}: kernel {err:.2e}  fp32 baseline {e32:.2e}  ratio {ratio:.2f}" + (f"  derived extra {extra:.2e}" if extra else ""))
    bound = max(factor * e32, F32_FLOOR, extra)
    assert err <= bound, (f"{name}: kernel error {err:.3e} > max({factor:g} x {e32:.3e}, {F32_FLOOR:.2e}"
                          + (f", {extra:.3e})" if extra else ")"))
    return ratio


# ---------------------------------------------------------------------------------------------------------
# written-out yardsticks of the loss / distillation / EWC / optimiser kernels (tests/test_loss_optim_*.py).  Every one casts its
# operands to `dtype` first: float64 is the reference, float32 the baseline a plain fp32 evaluation of the same formula reaches.
# ---------------------------------------------------------------------------------------------------------
def row_lse(x, dtype=torch.float64):
    """log-sum-exp of every row of x [rows, C]"""
    x = x.detach().to(dtype)
    m = x.max(1, keepdim=True).values
    return (m + torch.log(torch.exp(x - m).sum(1, keepdim=True))).squeeze(1)


def _log_softmax(x):
    m = x.max(1, keepdim=True).values
    return (x - m) - torch.log(torch.exp(x - m).sum(1, keepdim=True))


def ce_reference(logits, target, ignore_index=-100, upstream=1.0, dtype=torch.float64):
    """CrossEntropyLoss(reduction='mean', ignore_index) on logits [rows, C], target [rows] int64 -> (loss, d(upstream * loss) / dlogits).
    loss = sum over the rows with target != ignore_index of (lse - x[target]) / their number; no such row: the loss is NaN (0 / 0)
    and the gradient exactly zero, as torch has it."""
    x = logits.detach().to(dtype)
    t = target.reshape(-1)
    valid = t != ignore_index
    n = int(valid.sum())
    logp = _log_softmax(x)
    tt = torch.where(valid, t, torch.zeros_like(t)).unsqueeze(1)
    rows = -logp.gather(1, tt).squeeze(1) * valid.to(dtype)
    loss = rows.sum() / torch.tensor(float(n), dtype=dtype)
    if n == 0:
        return loss, torch.zeros_like(x)
    onehot = torch.zeros_like(x).scatter_(1, tt, 1.0)
    d = (torch.exp(logp) - onehot) * valid.to(dtype).unsqueeze(1) * (upstream / n)
    return loss, d


def kd_reference(new, old, c0, c1, T, upstream=1.0, dtype=torch.float64):
    """_KD_loss of LwF / WA on the class slice [c0, c1) of new / old [rows, C]:
    loss = -sum(softmax(old / T) * log_softmax(new / T)) / rows -> (loss, d(upstream * loss) / dnew over the full width C: zero outside
    the slice, (softmax(new / T) - softmax(old / T)) / T * upstream / rows inside)"""
    new, old = new.detach().to(dtype), old.detach().to(dtype)
    rows = new.shape[0]
    la, lb = _log_softmax(new[:, c0:c1] / T), _log_softmax(old[:, c0:c1] / T)
    pb = torch.exp(lb)
    loss = -(pb * la).sum() / rows
    d = torch.zeros_like(new)
    d[:, c0:c1] = (torch.exp(la) - pb) / T * (upstream / rows)
    return loss, d


def weight_align_reference(w, n_old, dtype=torch.float64):
    """Model.weight_align on w [rows, C]: gamma = mean ||old rows|| / mean ||new rows||, the rows from n_old on scaled by it
    -> (gamma, w aligned)"""
    w = w.detach().to(dtype)
    norms = torch.sqrt((w * w).sum(1))
    gamma = norms[:n_old].mean() / norms[n_old:].mean()
    out = w.clone()
    out[n_old:] *= gamma
    return gamma, out


def clip_reference(g, max_norm):
    """clip_grad_norm_(g, max_norm) -> (norm, coefficient, g * coefficient): coefficient = min(1, max_norm / (norm + 1e-6));
    max_norm None: no clipping, g is returned as it is"""
    if max_norm is None:
        return None, None, g
    norm = torch.sqrt((g * g).sum())
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return norm, coef, g * coef


def adam_reference(p, grads, max_norm, lr, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64):
    """len(grads) steps of clip_grad_norm_(max_norm) + torch.optim.Adam (no weight decay, no amsgrad) from zero moments
    -> dict p, g (the last gradient after clipping), m, v, norms, coefs"""
    p = p.detach().to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    norms, coefs = [], []
    for step, g in enumerate(grads, 1):
        norm, coef, g = clip_reference(g.detach().to(dtype), max_norm)
        norms.append(norm)
        coefs.append(coef)
        m = m + (g - m) * (1 - betas[0])
        v = v * betas[1] + (1 - betas[1]) * g * g
        denom = torch.sqrt(v) / (1 - betas[1] ** step) ** 0.5 + eps
        p = p - lr / (1 - betas[0] ** step) * (m / denom)
    return dict(p=p, g=g, m=m, v=v, norms=norms, coefs=coefs)


def sgd_reference(p, grads, max_norm, lr, momentum=0.0, weight_decay=0.0, dtype=torch.float64):
    """... + torch.optim.SGD (dampening 0, no Nesterov): d = g + wd * p; buf = d at the first step, momentum * buf + d afterwards;
    p -= lr * buf (momentum 0: p -= lr * d and buf stays zero) -> dict p, g, buf, norms, coefs"""
    p = p.detach().to(dtype).clone()
    buf = torch.zeros_like(p)
    norms, coefs = [], []
    for g in grads:
        norm, coef, g = clip_reference(g.detach().to(dtype), max_norm)
        norms.append(norm)
        coefs.append(coef)
        d = g + weight_decay * p
        if momentum != 0:
            buf = momentum * buf + d
            d = buf
        p = p - lr * d
    return dict(p=p, g=g, buf=buf, norms=norms, coefs=coefs)


def adadelta_reference(p, grads, max_norm, lr, rho=0.9, eps=1e-6, dtype=torch.float64):
    """... + torch.optim.Adadelta (no weight decay) -> dict p, g, sq (square_avg), acc (acc_delta), norms, coefs"""
    p = p.detach().to(dtype).clone()
    sq, acc = torch.zeros_like(p), torch.zeros_like(p)
    norms, coefs = [], []
    for g in grads:
        norm, coef, g = clip_reference(g.detach().to(dtype), max_norm)
        norms.append(norm)
        coefs.append(coef)
        sq = sq * rho + (1 - rho) * g * g
        delta = torch.sqrt(acc + eps) / torch.sqrt(sq + eps) * g
        acc = acc * rho + (1 - rho) * delta * delta
        p = p - lr * delta
    return dict(p=p, g=g, sq=sq, acc=acc, norms=norms, coefs=coefs)


def ewc_reference(grads, fisher_max, p, mean, coef, grad0, dtype=torch.float64):
    """EWC (il_modules/ewc.py): fisher = min(sum_k grads[k]^2 / len(grads), fisher_max); penalty = sum fisher * (p - mean)^2 / 2;
    grad = grad0 + coef * fisher * (p - mean) -> dict acc (the sum before finalising), fisher, penalty, grad"""
    acc = torch.zeros_like(p, dtype=dtype)
    for g in grads:
        g = g.detach().to(dtype)
        acc = acc + g * g
    fisher = torch.clamp(acc * (1.0 / len(grads)), max=fisher_max)
    d = p.detach().to(dtype) - mean.detach().to(dtype)
    penalty = (fisher * d * d).sum() / 2
    grad = grad0.detach().to(dtype) + coef * fisher * d
    return dict(acc=acc, fisher=fisher, penalty=penalty, grad=grad)


# ---------------------------------------------------------------------------------------------------------
# written-out yardsticks of the DM-Router's kernels (tests/test_router_kernels_*.py): rowops.hip, router.hip and DMRouterFn.  As above:
# operands cast to `dtype` first, float64 the reference, float32 the baseline.
# ---------------------------------------------------------------------------------------------------------
def layernorm_reference(x, gamma, beta, eps=1e-5, dy=None, dtype=torch.float64):
    """LayerNorm over the last dim of x [rows, C], two-pass: mean = sum(x) / C, var = sum((x - mean)^2) / C, rstd = 1 / sqrt(var + eps),
    xhat = (x - mean) * rstd, y = xhat * gamma + beta; with dy: dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)), g = dy * gamma,
    dgamma = sum_rows(dy * xhat), dbeta = sum_rows(dy) -> dict y, mean, rstd (, dx, dgamma, dbeta)"""
    x, gamma, beta = x.detach().to(dtype), gamma.detach().to(dtype), beta.detach().to(dtype)
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / C + eps)
    xhat = d * rstd
    out = dict(y=xhat * gamma + beta, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1))
    if dy is not None:
        dy = dy.detach().to(dtype)
        g = dy * gamma
        out["dx"] = rstd * (g - g.sum(-1, keepdim=True) / C - xhat * ((g * xhat).sum(-1, keepdim=True) / C))
        out["dgamma"] = (dy * xhat).reshape(-1, C).sum(0)
        out["dbeta"] = dy.reshape(-1, C).sum(0)
    return out


def colnorm_reference(x, gamma, beta, eps=1e-5, dy=None, dtype=torch.float64):
    """the same normalisation over the MIDDLE axis of x [B, P, W] (gamma, beta [P]): ChannelDomainGating's LayerNorm(patch) on the
    'b (d c) p' rearrangement, without the transpose -> dict y, mean [B, W], rstd [B, W] (, dx, dgamma [P], dbeta [P])"""
    r = layernorm_reference(x.detach().permute(0, 2, 1), gamma, beta, eps, None if dy is None else dy.detach().permute(0, 2, 1), dtype)
    return {k: (v.permute(0, 2, 1) if k in ("y", "dx") else v) for k, v in r.items()}


def gelu_reference(x, dtype=torch.float64):
    """nn.GELU(), the erf form: x * Phi(x), Phi(x) = (1 + erf(x / sqrt 2)) / 2"""
    x = x.detach().to(dtype)
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_grad_reference(x, dtype=torch.float64):
    """d gelu / dx = Phi(x) + x * phi(x), phi(x) = exp(-x^2 / 2) / sqrt(2 pi)"""
    x = x.detach().to(dtype)
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * (0.3989422804014327 * torch.exp(-0.5 * x * x))


def gate_tail_reference(r, w_route, b_route, beta, dw=None, dtype=torch.float64, w=None):
    """route Linear(P -> 1) over the patch axis of r [B, P, I], squeeze, softmax(beta * s): s[b][i] = sum_p Wr[p] r[b][p][i] + br,
    w = softmax(beta * s); with dw [B, I]: ds = beta * w * (dw - sum_i(dw * w)), dr[b][p][i] = Wr[p] * ds[b][i],
    dWr[p] = sum_{b,i} ds[b][i] * r[b][p][i], dbr = sum(ds) -> dict s, w, argmax (first maximum of s) (, ds, dr, dWr, dbr).
    w [B, I]: the backward formulas on THESE weights instead of the softmax (ops.gate_tail_bwd takes w as an operand; with the
    softmax's own w, sum(ds) is zero and dbr all rounding)"""
    r, Wr, br = r.detach().to(dtype), w_route.detach().to(dtype).reshape(-1), b_route.detach().to(dtype).reshape(-1)
    s = (r * Wr.view(1, -1, 1)).sum(1) + br
    m = s.max(1, keepdim=True).values
    e = torch.exp(beta * (s - m))
    soft = e / e.sum(1, keepdim=True)
    out = dict(s=s, w=soft, argmax=(s == m).to(torch.int64).argmax(1))
    w = soft if w is None else w.detach().to(dtype)
    if dw is not None:
        dw = dw.detach().to(dtype)
        ds = beta * w * (dw - (dw * w).sum(1, keepdim=True))
        out.update(ds=ds, dr=Wr.view(1, -1, 1) * ds.unsqueeze(1), dWr=(ds.unsqueeze(1) * r).sum((0, 2)), dbr=ds.sum().reshape(1))
    return out


def fanin_reference(logits, w, dout=None, dtype=torch.float64):
    """MRN fan-in: logits a list of I tensors [B, T, C_i] (C_i <= C = the last one's), each padded to C classes with ONES;
    out[b][t][c] = sum_i w[b][i] * Lpad_i[b][t][c]; with dout: dw[b][i] = sum_{t,c} dout[b][t][c] * Lpad_i[b][t][c] -> (out, dw or None)"""
    C = logits[-1].shape[-1]
    w = w.detach().to(dtype)
    pad = [torch.cat([l.detach().to(dtype), torch.ones(*l.shape[:2], C - l.shape[-1], dtype=dtype)], -1) for l in logits]
    out = sum(w[:, i].view(-1, 1, 1) * p for i, p in enumerate(pad))
    dw = None
    if dout is not None:
        dout = dout.detach().to(dtype)
        dw = torch.stack([(dout * p).sum((1, 2)) for p in pad], 1)
    return out, dw


DM_ROUTER_PARAMS = ("n_w", "n_b", "w1", "b1", "sn_w", "sn_b", "wsp", "bsp", "w2", "b2", "cn_w", "cn_b", "wch", "bch", "w3", "b3")
DM_ROUTER_GRADS = ("dx",) + tuple("d" + k for k in DM_ROUTER_PARAMS)


def dm_router_reference(x, params, dout, eps=1e-5, dtype=torch.float64, stages=None):
    """DM_Router.forward and its backward, stage by stage, on the router-internal layout x [B, P, I, C] (functional.DMRouterFn's);
    params: the 16 tensors in DMRouterFn's order (DM_ROUTER_PARAMS); dout like x.  The spatial gate mixes the tokens in the reference's
    '(d p)' order (token n = d * P + p), the channel gate normalises every (b, d, c) column over p and mixes the (d c) axis:
        xn = LN(x; n)           hpre = xn W1^T + b1        h = gelu(hpre) = [u | v]      vn = LN(v; sn)
        vp[b][n] = sum_m Wsp[n][m] vn[b][m] + bsp[n]       g = u * vp                    y = g W2^T + b2 + x
        zn = LN_p(y; cn)        zp = zn Wch^T + bch over (d c)                           z2 = y * zp      out = z2 W3^T + b3 + x
    -> (out [B, P, I, C], dict of the 17 gradients named in DM_ROUTER_GRADS); stages: a dict that receives the intermediate tensors
    (in the dtype of the evaluation)"""
    B, P, I, C = x.shape
    N = P * I
    p = {k: v.detach().to(dtype) for k, v in zip(DM_ROUTER_PARAMS, params)}
    X = x.detach().to(dtype).reshape(-1, C)
    dout = dout.detach().to(dtype).reshape(-1, C)

    def to_ref(t):                                  # rows in L2 order (b, p, d) -> [B, N, width] with n = d * P + p
        return t.reshape(B, P, I, -1).permute(0, 2, 1, 3).reshape(B, N, -1)

    def to_l2(t):
        return t.reshape(B, I, P, -1).permute(0, 2, 1, 3).reshape(B * N, -1)

    ln1 = layernorm_reference(X, p["n_w"], p["n_b"], eps, dtype=dtype)
    xn = ln1["y"]
    hpre = xn @ p["w1"].t() + p["b1"]
    h = gelu_reference(hpre, dtype)
    u, v = h[:, :C], h[:, C:]
    ln2 = layernorm_reference(v, p["sn_w"], p["sn_b"], eps, dtype=dtype)
    vn_r = to_ref(ln2["y"])                                                         # [B, N, C]
    vp_r = torch.einsum("nm,bmc->bnc", p["wsp"], vn_r) + p["bsp"].view(1, N, 1)
    vp = to_l2(vp_r)
    g = u * vp
    y = g @ p["w2"].t() + p["b2"] + X
    y3 = y.reshape(B, P, I * C)
    cn = colnorm_reference(y3, p["cn_w"], p["cn_b"], eps, dtype=dtype)
    zn = cn["y"].reshape(B * P, I * C)
    zp = (zn @ p["wch"].t() + p["bch"]).reshape(-1, C)
    z2 = y * zp
    out = z2 @ p["w3"].t() + p["b3"] + X

    G = {}
    G["dw3"], G["db3"] = dout.t() @ z2, dout.sum(0)
    dz2 = dout @ p["w3"]
    dy, dzp = dz2 * zp, (dz2 * y).reshape(B * P, I * C)
    G["dwch"], G["dbch"] = dzp.t() @ zn, dzp.sum(0)
    dzn = (dzp @ p["wch"]).reshape(B, P, I * C)
    cb = colnorm_reference(y3, p["cn_w"], p["cn_b"], eps, dzn, dtype)
    G["dcn_w"], G["dcn_b"] = cb["dgamma"], cb["dbeta"]
    dy = dy + cb["dx"].reshape(-1, C)
    G["dw2"], G["db2"] = dy.t() @ g, dy.sum(0)
    dg = dy @ p["w2"]
    du, dvp_r = dg * vp, to_ref(dg * u)
    G["dwsp"] = torch.einsum("bnc,bmc->nm", dvp_r, vn_r)
    G["dbsp"] = dvp_r.sum((0, 2))
    dvn = to_l2(torch.einsum("nm,bnc->bmc", p["wsp"], dvp_r))
    lb2 = layernorm_reference(v, p["sn_w"], p["sn_b"], eps, dvn, dtype)
    G["dsn_w"], G["dsn_b"] = lb2["dgamma"], lb2["dbeta"]
    dhpre = torch.cat([du, lb2["dx"]], 1) * gelu_grad_reference(hpre, dtype)
    G["dw1"], G["db1"] = dhpre.t() @ xn, dhpre.sum(0)
    lb1 = layernorm_reference(X, p["n_w"], p["n_b"], eps, dhpre @ p["w1"], dtype)
    G["dn_w"], G["dn_b"] = lb1["dgamma"], lb1["dbeta"]
    G["dx"] = (lb1["dx"] + dout + dy).reshape(B, P, I, C)
    if stages is not None:
        stages.update(xn=xn, hpre=hpre, vn_r=vn_r, vp=vp, g=g, y=y, zn=zn, zp=zp, z2=z2, dy=dy, dvp_r=dvp_r, dhpre=dhpre)
    return out.reshape(B, P, I, C), G


# ---------------------------------------------------------------------------------------------------------
# written-out yardsticks of the SVTR attention kernels and of one trained SVTR block (tests/test_svtr_kernels_*.py): attention.hip,
# SvtrAttentionFn and modules.svtr.Block.forward_train.  As above: operands cast to `dtype` first, float64 the reference, float32 the
# baseline.  x3=...: the baseline of a path whose products run as split-fp16 x3 -- the same formulas in float64 with every operand of
# such a product replaced by its HL32 value (hl_split) at the scale the code under test uses, and hi*hi + hi*lo + lo*hi in place of the
# product (lo*lo is what the kernels drop: a' b' - lo_a lo_b exactly, x3_matmul).  Its distance from plain float64 stands where the
# fp32 baseline's error stands in within_baseline.
# ---------------------------------------------------------------------------------------------------------
FP16_PEAK = 16384.0                # ops.FP16_WEIGHT_PEAK: the range target of every power-of-two operand scale
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def hl_parts(x, s=1.0):
    """the two halves of the HL32 value of x at scale s, as the kernels form them (csrc/hl32.hpp split_f16): t = fp32(s x),
    hi = fp16(t), lo = fp16(t - hi) (exact in fp32) -> (hi / s, lo / s) in float64.  Round to nearest even, fp16 subnormals kept,
    |t| >= 65520 overflows to inf as it does on the device."""
    s = s.detach().double() if torch.is_tensor(s) else float(s)
    t = (x.detach().double() * s).to(torch.float32)
    hi = t.to(torch.float16)
    lo = (t - hi.to(torch.float32)).to(torch.float16)
    return hi.double() / s, lo.double() / s


def hl_split(x, s=1.0):
    """CPU emulation of the HL32 value of x at scale s: (fp16(s x) + fp16(s x - fp16(s x))) / s in float64"""
    hi, lo = hl_parts(x, s)
    return hi + lo


def pow2_scale_of(x, target=FP16_PEAK):
    """the largest power of two s with s * max|x| <= target (ops.pow2_scale / mrn_pow2_finalize_f32); 1 where x is all zero"""
    m = float(x.detach().abs().max()) if x.numel() else 0.0
    if not (m > 0.0 and m < float("inf")):
        return 1.0
    return 2.0 ** float(np.floor(np.log2(np.float32(target) / np.float32(m))))


def layernorm_bound_scale(gamma, beta, C, target=FP16_PEAK):
    """the scale layernorm_fwd_operand derives from the parameters: s (sqrt(C) max|gamma| + max|beta|) <= target"""
    bound = float(np.float32(np.sqrt(np.float32(C))) * np.float32(gamma.detach().abs().max()) + np.float32(beta.detach().abs().max()))
    return 2.0 ** float(np.floor(np.log2(np.float32(target) / np.float32(bound))))


def x3_matmul(a, b, sa, sb):
    """a @ b as the split-fp16 x3 kernels form it, in float64: hi hi + hi lo + lo hi of the HL32 values of a (scale sa) and b (sb)"""
    ah, al = hl_parts(a, sa)
    bh, bl = hl_parts(b, sb)
    return (ah + al) @ (bh + bl) - al @ bl


def _heads_of(qkv, heads, dtype):
    B, N, C3 = qkv.shape
    d = C3 // 3 // heads
    x = qkv.detach().to(dtype).reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]                                  # [B, heads, N, d] each


def _tokens_of(t):
    B, h, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, h * d)


def svtr_attention_reference(qkv, mask, heads, scale, dout=None, dtype=torch.float64, mutant=None):
    """softmax(scale q k^T + mask) v per head on qkv [B, N, 3C] (q | k | v, each (head, d) innermost, d = C / heads: any head
    dimension), mask [N, N] additive (mask[query][key]) or None, and its backward, written out:
        S = scale q k^T + mask    P = exp(S - max) / l    lse = max + log l (natural log)    O = P v
        dP = dO v^T    D = rowsum(dO o O)    dS = P o (dP - D)    dq = scale dS k    dk = scale dS^T q    dv = P^T dO
    -> dict out [B, N, C], lse [B, heads, N] (, dq, dk, dv [B, N, C] with dout [B, N, C]).
    mutant: a deliberately wrong variant, for the proof that the test inputs discriminate (test_svtr_kernels_cpu.py)"""
    q, k, v = _heads_of(qkv, heads, dtype)
    if mutant == "next_head_v":
        v = torch.roll(v, -1, 1)
    S = (q @ k.transpose(-1, -2)) * scale
    m = None if mask is None else mask.detach().to(dtype)
    if m is not None:
        S = S + m
    mx = S.max(-1, keepdim=True).values
    e = torch.exp(S - mx)
    l = e.sum(-1, keepdim=True)
    P = e / l
    O = P @ v
    out = dict(out=_tokens_of(O), lse=(mx + torch.log(l)).squeeze(-1))
    if dout is None:
        return out
    B, N, C = out["out"].shape
    dO = dout.detach().to(dtype).reshape(B, N, heads, C // heads).permute(0, 2, 1, 3)
    dP = dO @ v.transpose(-1, -2)
    D = (dO * O).sum(-1, keepdim=True)
    if mutant == "no_D":
        D = torch.zeros_like(D)
    if mutant == "lse_base":                   # a backward that takes the natural lse it is handed for the base-2 one it stores
        P = torch.exp2(S * LOG2E - out["lse"].unsqueeze(-1))
    dS = P * (dP - D)
    dSk = dS
    if mutant == "mask_transposed_dkv":        # dk / dv from the probabilities of the TRANSPOSED mask (lse is the forward's)
        Pt = torch.exp((q @ k.transpose(-1, -2)) * scale + m.t() - out["lse"].unsqueeze(-1))
        dSk, P = Pt * (dP - D), Pt
    out["dq"] = _tokens_of(dS @ k) * scale
    out["dk"] = _tokens_of(dSk.transpose(-1, -2) @ q) * (1.0 if mutant == "dk_no_scale" else scale)
    out["dv"] = _tokens_of(P.transpose(-1, -2) @ dO)
    return out


X3_OPSCALE, X3_PBIAS = 64.0, 12.0          # csrc/attention.hip: OPSCALE, PBIAS of svtr_attention_x3_kernel


def svtr_attention_x3_baseline(qkv, mask, heads, scale):
    """the x3 baseline of svtr_attention_x3_kernel's output, in float64: q' = HL32(64 scale log2e q) (the factor applied in fp32, as
    the kernel does), k' = HL32(64 k), v' = HL32(64 v); base-2 scores q' k' (x3) / 4096 + log2e mask; per 32-key tile the running
    maximum m_t of the tiles so far, p = exp2(s - m_t + 12) (0 where every key so far is masked), l = sum of the UNSPLIT p,
    O = sum of HL32(p) v' (x3), every tile's share brought to the last maximum by the exact factor exp2(m_t - m_last) -> out [B, N, C]"""
    q, k, v = _heads_of(qkv, heads, torch.float32)
    qs = (q * np.float32(np.float32(scale) * np.float32(LOG2E) * np.float32(X3_OPSCALE))).double()      # already 64 x: split at scale 1
    B, h, N, d = q.shape
    S = x3_matmul(qs, k.double().transpose(-1, -2), 1.0, X3_OPSCALE) / X3_OPSCALE
    if mask is not None:
        S = S + mask.detach().double() * LOG2E
    T = (N + 31) // 32
    Sp = torch.full((B, h, N, T * 32), float("-inf"), dtype=torch.float64)
    Sp[..., :N] = S
    run = torch.cummax(Sp.view(B, h, N, T, 32).amax(-1), -1).values                      # [B, h, N, T]
    safe = torch.where(torch.isinf(run), torch.zeros_like(run), run)
    last = safe[..., -1:]
    p = torch.exp2(Sp.view(B, h, N, T, 32) - safe.unsqueeze(-1) + X3_PBIAS).to(torch.float32).double()
    w = torch.exp2(safe - last).unsqueeze(-1)                                            # exact powers in float64 up to rounding 2^-53
    l = (p * w).sum((-1, -2)).unsqueeze(-1)
    ph, pl = hl_parts(p, 1.0)
    ph, pl = (ph * w).reshape(B, h, N, T * 32)[..., :N], (pl * w).reshape(B, h, N, T * 32)[..., :N]
    vh, vl = hl_parts(v, X3_OPSCALE)
    O = ((ph + pl) @ (vh + vl) - pl @ vl) / l
    return _tokens_of(O)


SVTR_BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "mixer.qkv.weight", "mixer.qkv.bias", "mixer.proj.weight", "mixer.proj.bias",
                     "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def svtr_block_reference(x, params, drop1, drop2, mask, heads, dout, eps=1e-6, dtype=torch.float64, x3=None, mutant=None):
    """modules.svtr.Block.forward_train and its backward, stage by stage.  x, dout [B, N, C]; params: a dict under the block's
    state_dict names (SVTR_BLOCK_PARAMS; "mixer.qkv.bias" absent or None: no qkv bias); drop1 / drop2 [B]: the DropPath multipliers of
    the two branches (0 or 1 / keep) or None; mask [N, N] or None.
        y1 = LN(x; norm1)    qkv = y1 Wqkv^T + bqkv    ctx = attention(qkv)    pr = ctx Wp^T + bp    x1 = x + drop1 pr
        y2 = LN(x1; norm2)   f = y2 W1^T + b1          g = gelu(f)             o = g W2^T + b2       out = x1 + drop2 o
    -> (out [B, N, C], dict of gradients: "dx" and "d" + name for every parameter present: 12, or 13 with the qkv bias).
    x3: None, or "fused" / "separate": the x3 baseline of the default mode / of TRAIN_OPERAND_FUSION off.  The four forward Linears and
    their four data gradients are the x3 products (the weight gradients run exact at these row counts: functional.linear_wgrad takes
    the x3 path from 4096 rows); weights split at the power of two of max|W|; activations and gradients at the power of two of their
    own max ("separate"), or at what the producer hands on ("fused"): the LayerNorm bound, the scale of max|qkv| for ctx, of max|f| for
    g, of max|dg| at half the target for df.
    mutant: a deliberately wrong variant (test_svtr_kernels_cpu.py)"""
    B, N, C = x.shape
    p = {k: (None if params.get(k) is None else params[k].detach().to(dtype)) for k in SVTR_BLOCK_PARAMS}
    X, dout2 = x.detach().to(dtype).reshape(-1, C), dout.detach().to(dtype).reshape(-1, C)
    rows = lambda d: torch.ones(B * N, 1, dtype=dtype) if d is None else d.detach().to(dtype).repeat_interleave(N).view(-1, 1)
    d1, d2 = rows(drop1), rows(drop2)
    scale = (C // heads) ** -0.5

    def mm(a, w, sa=None):                          # a @ w^T
        if x3 is None:
            return a @ w.t()
        sa = pow2_scale_of(a) if (sa is None or x3 == "separate") else sa
        return x3_matmul(a, w.t(), sa, pow2_scale_of(w))

    ln1 = layernorm_reference(X, p["norm1.weight"], p["norm1.bias"], eps, dtype=dtype)
    y1 = ln1["y"]
    qkv = mm(y1, p["mixer.qkv.weight"], layernorm_bound_scale(p["norm1.weight"], p["norm1.bias"], C))
    if p["mixer.qkv.bias"] is not None:
        qkv = qkv + p["mixer.qkv.bias"]
    att = svtr_attention_reference(qkv.reshape(B, N, 3 * C), mask, heads, scale, dtype=dtype)
    ctx = att["out"].reshape(-1, C)
    pr = mm(ctx, p["mixer.proj.weight"], pow2_scale_of(qkv)) + p["mixer.proj.bias"]
    x1 = X + d1 * pr
    ln2 = layernorm_reference(x1, p["norm2.weight"], p["norm2.bias"], eps, dtype=dtype)
    y2 = ln2["y"]
    f = mm(y2, p["mlp.fc1.weight"], layernorm_bound_scale(p["norm2.weight"], p["norm2.bias"], C)) + p["mlp.fc1.bias"]
    g = gelu_reference(f, dtype)
    o = mm(g, p["mlp.fc2.weight"], pow2_scale_of(f)) + p["mlp.fc2.bias"]
    out = x1 + d2 * o

    G = {}
    do = dout2 if mutant == "no_drop_in_gradient" else d2 * dout2
    G["dmlp.fc2.weight"] = do.t() @ g
    G["dmlp.fc2.bias"] = do.reshape(C, -1).sum(1) if mutant == "fc2_bias_wrong_axis" else do.sum(0)
    dg = mm(do, p["mlp.fc2.weight"].t())
    df = dg * gelu_grad_reference(f, dtype)
    G["dmlp.fc1.weight"], G["dmlp.fc1.bias"] = df.t() @ y2, df.sum(0)
    dy2 = mm(df, p["mlp.fc1.weight"].t(), pow2_scale_of(dg, FP16_PEAK / 2))
    lb2 = layernorm_reference(x1, p["norm2.weight"], p["norm2.bias"], eps, dy2, dtype)
    G["dnorm2.weight"], G["dnorm2.bias"] = lb2["dgamma"], lb2["dbeta"]
    dln2 = lb2["dx"]
    if mutant == "ln2_no_xhat":
        gg = dy2 * p["norm2.weight"]
        dln2 = ln2["rstd"].unsqueeze(-1) * (gg - gg.sum(-1, keepdim=True) / C)
    dx1 = dout2 + dln2
    dpr = dx1 if mutant == "no_drop_in_gradient" else d1 * dx1
    G["dmixer.proj.weight"], G["dmixer.proj.bias"] = dpr.t() @ ctx, dpr.sum(0)
    dctx = mm(dpr, p["mixer.proj.weight"].t())
    ab = svtr_attention_reference(qkv.reshape(B, N, 3 * C), mask, heads, scale, dctx.reshape(B, N, C), dtype)
    dqkv = torch.cat([ab["dq"], ab["dk"], ab["dv"]], -1).reshape(-1, 3 * C)
    G["dmixer.qkv.weight"] = dqkv.t() @ y1
    if p["mixer.qkv.bias"] is not None:
        G["dmixer.qkv.bias"] = dqkv.sum(0)
    dy1 = mm(dqkv, p["mixer.qkv.weight"].t())
    lb1 = layernorm_reference(X, p["norm1.weight"], p["norm1.bias"], eps, dy1, dtype)
    G["dnorm1.weight"], G["dnorm1.bias"] = lb1["dgamma"], lb1["dbeta"]
    G["dx"] = (dx1 + lb1["dx"]).reshape(B, N, C)
    return out.reshape(B, N, C), G
