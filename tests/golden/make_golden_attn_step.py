"""Outputs of the attention head's three decoder kernels (csrc/attn_decode.hip attn_decoder_kernel, attn_greedy_kernel, attn_beam_kernel) on
the smallest shapes that reach every branch of the step they share, for tests/test_decode_attn_step_gpu.py, which demands them back bit for bit.

    python tests/golden/make_golden_attn_step.py

Needs the GPU and the built library; does not use the reference.  The fixture was recorded from the parent of the commit that moved the
step into shared helpers (its hash is stored under "parent"), so regenerate it only for a change that is MEANT to move a bit.  Inputs
come from the seeded CPU generator of mrn_amd/tools/weights.py and are not stored.  Hidden is 256 and S = 3 throughout; a case runs in
the split-fp16 x3 form and in the exact form.  Writes tests/golden/attn_step.npz.
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from mrn_amd.tools import weights as W  # noqa: E402

HID, S, SEED, SOS, EOS = 256, 3, 47, 2, 1


def u(name, shape, a=1.0):
    return torch.from_numpy(W.uniform("attn_step:" + name, shape, -a, a, SEED)).cuda()


@contextlib.contextmanager
def env(**kv):
    """the launch switches that are read per launch: set (or, with None, unset) for the block"""
    old = {k: os.environ.pop(k, None) for k in kv}
    os.environ.update({k: v for k, v in kv.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def operands(ops, tag, B, T, D, C, x3):
    """one expert's inputs and weights, the weights packed for the form; the generator leans to EOS so that beam entries finish early"""
    w = {"Hb": u(tag + "Hb", (B, T, D)), "Hproj": u(tag + "Hproj", (B, T, HID)), "eproj": u(tag + "eproj", (B, S, 4 * HID)),
         "etab": u(tag + "etab", (C, 4 * HID)), "b_h2h": u(tag + "b_h2h", (HID,), 0.1), "w_score": u(tag + "w_score", (HID,), 0.2),
         "b_hh": u(tag + "b_hh", (4 * HID,), 0.1), "b_gen": u(tag + "b_gen", (C,), 0.1)}
    w["b_gen"][EOS] += 0.75
    h2h, ih, hh = u(tag + "h2h", (HID, HID), 1 / 16), u(tag + "ih", (4 * HID, D), D ** -0.5), u(tag + "hh", (4 * HID, HID), 1 / 16)
    gen = u(tag + "gen", (C, HID), 0.25)
    if x3:
        w["w_h2h"], w["w_ih"], w["w_hh"], inv = ops.pack_decoder_x3(h2h, ih, hh, D)
        w["w_gen"], ginv = ops.pack_generator(gen, True)
        w["w_inv"] = torch.cat([inv, ginv]).contiguous()            # (the decoder reads the first three)
    else:
        w["w_h2h"], w["w_ih"], w["w_hh"] = (ops.pack_fragment_major(t).contiguous() for t in (h2h, ih, hh))
        w["w_gen"], w["w_inv"] = ops.pack_generator(gen, False)
    return w


def decoder(ops, w, state=None):
    """the teacher-forced launch with every training save (ops.attn_decoder_train) and, where given, the carried state"""
    p = ops._p
    B, T, D = w["Hb"].shape
    new = lambda *s: torch.empty(*s, device="cuda", dtype=torch.float32)  # noqa: E731
    out = {"hid": new(B, S, HID), "alpha": new(B, S, T), "gates": new(B, S, 4 * HID), "c": new(B, S, HID), "ctx": new(B, S, D),
           "hp": new(B, S, HID)}
    if state is not None:
        out["h_state"], out["c_state"] = state[0].clone(), state[1].clone()
    x3 = w["w_inv"] is not None
    ops.call("mrn_attn_decoder_fwd_x3" if x3 else "mrn_attn_decoder_fwd_f32", p(w["Hb"]), p(w["Hproj"]), p(w["eproj"]),
             w["eproj"].stride(0), w["eproj"].stride(1), p(w["w_h2h"]), p(w["b_h2h"]), p(w["w_score"]), p(w["w_ih"]), p(w["w_hh"]),
             *([p(w["w_inv"])] if x3 else []), p(w["b_hh"]), p(out["hid"]), out["hid"].stride(0), out["hid"].stride(1),
             p(out.get("h_state")), p(out.get("c_state")), p(out["alpha"]), p(out["gates"]), p(out["c"]), p(out["ctx"]), p(out["hp"]),
             B, T, D, S, HID, ops._stream())
    return out


def grouped(ops, tag, G, B, T, D, x3):
    """G experts in the grouped launch -> hid [G,B,S,H]"""
    ws = [operands(ops, f"{tag}{g}:", B, T, D, 2, x3) for g in range(G)]
    col = lambda k: [w[k] for w in ws]  # noqa: E731
    stack = lambda k: torch.stack(col(k)).contiguous()  # noqa: E731
    return ops.attn_decoder_grouped(stack("Hb"), stack("Hproj"), stack("eproj"), col("w_h2h"), col("b_h2h"), col("w_score"), col("w_ih"),
                                    col("w_hh"), col("b_hh"), HID, w_inv=col("w_inv") if x3 else None)


def greedy(ops, w, C):
    """-> logits (written with a padded row stride) and tokens"""
    B = w["Hb"].shape[0]
    out = torch.empty(B, S, C + 3, device="cuda", dtype=torch.float32)[:, :, :C]
    start = torch.tensor([SOS], dtype=torch.int64).cuda()
    logits, tokens = ops.attn_greedy_decode(w["Hb"], w["Hproj"], w["etab"], start, w["w_h2h"], w["b_h2h"], w["w_score"], w["w_ih"],
                                            w["w_hh"], w["b_hh"], w["w_gen"], w["b_gen"], HID, S, out=out, want_tokens=True,
                                            w_inv=w["w_inv"])
    return {"logits": logits.contiguous(), "tokens": tokens}


def beam(ops, w, width):
    start = torch.tensor([SOS], dtype=torch.int64).cuda()
    res = ops.attn_beam_decode(w["Hb"], w["Hproj"], w["etab"], start, w["w_h2h"], w["b_h2h"], w["w_score"], w["w_ih"], w["w_hh"],
                               w["b_hh"], w["w_gen"], w["b_gen"], HID, S, EOS, width, w_inv=w["w_inv"])
    return dict(zip(("tokens", "length", "score", "logp", "path", "prob"), res))


def run(ops):
    """every case -> {"case/output": CPU tensor}; a key "k@form" must equal the stored "k" (the same launch in another form)"""
    d = {}

    def put(case, outs, form=""):
        d.update({f"{case}/{k}{form}": v for k, v in outs.items()})
    with env(MRN_ATTN_CTX_CHUNK=None, MRN_GREEDY_VB=None):
        for x3 in (True, False):
            f = "x3" if x3 else "f32"
            # 1. single expert, saves and carried state: B = 5 ends half way through the last two-sample tile; T = 67 = 16 x 4 + 3
            w = operands(ops, "one:", 5, 67, 32, 37, x3)
            put(f"decoder_{f}", decoder(ops, w, (u("one:h", (5, HID), 0.5), u("one:c", (5, HID)))))
            # 4. greedy on the same operands, C = 37: three class tiles, the last padded
            for vb in ("2", "16"):
                with env(MRN_GREEDY_VB=vb):
                    put(f"greedy_vb{vb}_{f}", greedy(ops, w, 37))
            # 5. beam, B = 6: W = 3 (five samples per workgroup, a row unused) and W = 16 (one sample per workgroup)
            w = operands(ops, "beam:", 6, 67, 32, 37, x3)
            for width in (3, 16):
                put(f"beam_w{width}_{f}", beam(ops, w, width))
            # 2. grouped: pinned == 1, pinned == 2 (eight (group, tile) pairs), a split beyond eight groups
            for G, B in ((3, 4), (4, 4), (9, 3)):
                put(f"grouped_g{G}_{f}", {"hid": grouped(ops, f"g{G}:", G, B, 5, 32, x3)})
            # 3. two context chunks (1024 + 32) under the switch; without it the whole-context form must give the same bits
            w = operands(ops, "wide:", 3, 5, 1056, 37, x3)
            put(f"wide_decoder_{f}", decoder(ops, w))
            put(f"wide_greedy_{f}", greedy(ops, w, 37))
            with env(MRN_ATTN_CTX_CHUNK="1"):
                put(f"wide_decoder_{f}", decoder(ops, w), "@chunked")
                put(f"wide_greedy_{f}", greedy(ops, w, 37), "@chunked")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


if __name__ == "__main__":
    from mrn_amd import ops
    from mrn_amd._lib import LIB
    LIB.load()
    got = run(ops)
    d = {k: v.numpy() for k, v in got.items() if "@" not in k}
    for k, v in got.items():
        assert torch.equal(v, got[k.split("@")[0]]), k
    for k in d:
        if k.endswith("/length"):                                   # some entries finish before S, some do not
            assert (d[k] == S).any() and ((d[k] > 0) & (d[k] < S)).any(), (k, d[k])
    d["parent"] = np.array(sys.argv[1] if len(sys.argv) > 1 else
                           subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip())
    path = os.path.join(HERE, "attn_step.npz")
    np.savez_compressed(path, **d)
    print("attn_step ->", path, f"{os.path.getsize(path) / 1024:.0f} KiB, {len(d) - 1} arrays")
