"""What the evaluation forwards of Model, DERNet and MRNNet return for every second decode on the attention head (attn_beam, attn_lexicon,
attn_candidates, attn_shortlist, and none of them), and the library entry points they call, for tests/test_decode_attn_search_gpu.py.

    python tests/golden/make_golden_attn_search.py

Needs the GPU and the built library; does not use the reference.  The fixture was recorded from the parent of the commit that made one
request record (modules/decoding.py AttnSearch) of the four keywords (its hash is stored under "parent"): that commit moved Python only,
so every stored value must come back.  Regenerate it only for a change that is MEANT to move a launch or a bit.  Nets and batch are
those of tests/test_decode_attn_beam_gpu.py trba_nets() (its whole batch: one image per label, 32 x 128, batch_max_length 25), a
two-task attention DERNet on the same options and a four-expert MRNNet, all seeded by mrn_amd/tools/weights.py; nothing of them is
stored.  The requests: beam width 3, the trie of tests/test_decode_attn_lexicon_gpu.py WORDS beside it, the candidate table of
tests/test_decode_attn_candidates_gpu.py word_lists(LABELS), the shortlist of K = 3 words of tests/test_decode_shortlist_gpu.py WORDS,
and plain greedy.

The groups, and the branch of MRNNet._experts_and_gate a routed (cross=True) forward takes in each; cross=False is the newest expert's
own forward in all of them:

    model         the plain Model
    der           the DERNet
    mrn           two experts, no switch: ONE lock-step heads group (HeadsGroup.run_greedy) on one side stream -- with fewer than four
                  experts _half_groups gives a single sub-group
    mrn_inline    expert_halves = 0: the same heads group on the caller's stream
    mrn_streams   MRN_GREEDY_DECODE=stepwise: no lock-step heads; grouped backbones, then every expert's heads on a stream of its own
    mrn_loop      the same with expert_streams = False: one expert after the other, whole forwards
    mrn_halves    four experts, expert_halves = 2: two lock-step sub-groups of two on two streams (routed forward only)

Every forward runs twice, the second time recorded, so that the call list is the steady state: no packing of weights, whatever ran
before.  A key "k@request" must equal the stored "k" (the greedy logits do not depend on the request).  Writes
tests/golden/attn_search.npz.
"""
import contextlib
import functools
import io
import os
import subprocess
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.golden.make_golden_attn_step import env  # noqa: E402

WIDTH, K, L = 3, 3, 25
REQUESTS = ("greedy", "beam", "lexicon", "candidates", "shortlist")
GROUPS = ("model", "der", "mrn", "mrn_inline", "mrn_streams", "mrn_loop", "mrn_halves")
INTS, FLOATS = ("beam_path", "beam_word", "index"), ("beam_prob", "logits")


def _mrn(opt, classes, seed):
    from mrn_amd.modules.model import MRNNet
    from mrn_amd.tools import weights as Wt
    with contextlib.redirect_stdout(io.StringIO()):
        net = MRNNet(opt)
        for c in classes:
            net.update_fc(256, c)
            net.build_prediction(opt, c)
    Wt.fill_state_dict(net.state_dict(), seed=seed)
    with torch.no_grad():
        for e in net.model:
            e.Prediction.generator.weight.mul_(40.0)
    return net.cuda().eval()


@functools.lru_cache(maxsize=None)
def nets():
    """{"mrn", "model", "der", "four"} and the batch on the device: trba_nets() and two more nets built its way (seeded weights, peaked
    generators, evaluation mode)"""
    from mrn_amd.modules.model import DERNet
    from mrn_amd.tools import weights as Wt
    from tests.test_decode_attn_beam_gpu import CHARACTERS, trba_nets, trba_opt
    net, plain, image = trba_nets()
    classes = (30, 5 + len(CHARACTERS))
    opt = trba_opt()
    with contextlib.redirect_stdout(io.StringIO()):
        der = DERNet(opt)
        for c in classes:
            der.update_fc(256, c)
        der.build_prediction(opt, classes[-1])
        der.build_aux_prediction(opt, classes[-1])
    Wt.fill_state_dict(der.state_dict(), seed=13)
    with torch.no_grad():
        der.Prediction.generator.weight.mul_(40.0)
    four = _mrn(opt, (30, 36, 38, classes[-1]), 14)
    return {"mrn": net, "model": plain, "der": der.cuda().eval(), "four": four}, image.cuda()


@functools.lru_cache(maxsize=None)
def requests():
    """request name -> the keywords of an evaluation forward"""
    from mrn_amd import ops
    from mrn_amd.modules import decoding
    from mrn_amd.tools.utils import AttnLabelConverter
    from tests.test_decode_attn_beam_gpu import CHARACTERS, LABELS
    from tests.test_decode_attn_candidates_gpu import word_lists
    from tests.test_decode_attn_lexicon_gpu import WORDS as TRIE_WORDS
    from tests.test_decode_shortlist_gpu import WORDS as SHORTLIST_WORDS
    conv = AttnLabelConverter(CHARACTERS)
    tokens, lengths, _ = decoding.encode_attn_lexicon(conv, TRIE_WORDS, L)
    trie = ops.upload_trie(decoding.build_trie(tokens, lengths), "cuda")
    lists = [word_lists(LABELS)[gt] for gt in LABELS]
    table = decoding.CandidateTable(conv, lists, True, L)
    cands = ops.upload_words(table.tokens, table.lengths, "cuda", 2).with_cand(table.rows(lists), L + 1)
    tokens, lengths, _ = decoding.encode_attn_lexicon(conv, SHORTLIST_WORDS, L)
    words = ops.upload_words(tokens, lengths, "cuda", 2)
    return {"greedy": {}, "beam": {"attn_beam": WIDTH}, "lexicon": {"attn_beam": WIDTH, "attn_lexicon": trie},
            "candidates": {"attn_candidates": cands}, "shortlist": {"attn_shortlist": (words, K, None)}}


def _calls(group):
    """the forwards of a group: call name -> f(**request keywords) -> the forward's dict"""
    all_nets, image = nets()
    sos = torch.full((image.shape[0],), 2, dtype=torch.long, device=image.device)
    if group in ("model", "der"):
        return {"forward": lambda **kw: all_nets[group](image, text=sos, is_train=False, **kw)}
    net = all_nets["four" if group == "mrn_halves" else "mrn"]
    calls = {"routed": lambda **kw: net(image, True, sos, False, **kw)}
    if group != "mrn_halves":
        calls["newest"] = lambda **kw: net(image, False, sos, False, **kw)
    return calls


@contextlib.contextmanager
def _setting(group):
    """the switches of a group, put back behind it"""
    all_nets, _ = nets()
    net = all_nets["four" if group == "mrn_halves" else "mrn"]
    old = net.expert_streams, net.expert_halves
    net.expert_streams = group != "mrn_loop"
    net.expert_halves = {"mrn_inline": 0, "mrn_halves": 2}.get(group, -1)
    try:
        with env(MRN_GREEDY_DECODE="stepwise" if group in ("mrn_streams", "mrn_loop") else None, MRN_ATTN_BEAM=None):
            yield
    finally:
        net.expert_streams, net.expert_halves = old


def run(groups=GROUPS):
    """-> {"group/call/request/output": CPU tensor} and "group/call/request/calls": the list of library entry points, in order"""
    from tests.test_decode_attn_candidates_gpu import recorded_calls
    patch = types.SimpleNamespace(setattr=setattr)
    d = {}
    with torch.no_grad():
        for group in groups:
            with _setting(group):
                for call, f in _calls(group).items():
                    for name in REQUESTS:
                        kw = requests()[name]
                        f(**kw)
                        out, names = recorded_calls(patch, lambda: f(**kw))
                        out = dict(out, logits=out["logits"] if "logits" in out else out["predict"])
                        assert ("beam_path" in out) == (name != "greedy") and ("beam_word" in out) == (name not in ("greedy", "beam"))
                        for k in INTS + FLOATS:
                            if out.get(k) is not None:
                                same = k == "logits" and name != "greedy"
                                d[f"{group}/{call}/greedy/logits@{name}" if same else f"{group}/{call}/{name}/{k}"] = out[k]
                        d[f"{group}/{call}/{name}/calls"] = list(names)
    torch.cuda.synchronize()
    return {k: v if isinstance(v, list) else v.cpu() for k, v in d.items()}


if __name__ == "__main__":
    from mrn_amd._lib import LIB
    LIB.load()
    got = run()
    d = {}
    for k, v in got.items():
        if "@" in k:
            assert torch.equal(v, got[k.split("@")[0]]), k
        else:
            d[k] = np.array(v) if isinstance(v, list) else v.numpy()
    d["parent"] = np.array(sys.argv[1] if len(sys.argv) > 1 else
                           subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip())
    path = os.path.join(HERE, "attn_search.npz")
    np.savez_compressed(path, **d)
    print("attn_search ->", path, f"{os.path.getsize(path) / 1024:.0f} KiB, {len(d) - 1} arrays")
