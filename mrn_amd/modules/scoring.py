"""Which validation batches the device scorer takes, and the integer form of the strings it compares (pure Python: importable
without a GPU).

validation() (mrn_amd/test.py, reference test.py:211-265) scores strings: the greedy prediction is decoded through
converter.character, cut at "[EOS]" on the attention head, and compared with the raw label.  mrn_greedy_score_f32 scores integer
tokens instead, which gives the same numbers as long as one token is one character:

  * a class k stands for the string converter.character[k]; its CANONICAL token is converter.dict[that string].  The dict keeps
    the LAST index of a repeated character (tools/utils.py:23-27), so two classes that decode to the same character get the same
    token and compare equal, as their strings do;
  * a label character is converter.dict.get(ch, -1): a character outside the dictionary equals no prediction;
  * the classes whose string is longer than one character ("[PAD]", "[UNK]", "[SOS]") get -2: the kernel flags a sample that
    predicts one of them where it counts, and the host scores that sample on strings.  The CTC blank and [EOS] never reach the
    table: the kernel's mode drops / cuts at them.

The table is built once per validation() call and never cached on the converter: MRN rebuilds its character set for every task,
and a stale table would score silently wrong.
"""
import os

import numpy as np

from ..tools.utils import _padded_rows

SCORE_MAX_T = 512            # decoding steps mrn_greedy_score_f32 takes (static LDS: 4 samples x 512 tokens + probabilities)
SCORE_MAX_LABEL = 256        # label characters (4 columns of the edit-distance wavefront per lane)
MULTI_CHARACTER = -2
NOT_IN_DICTIONARY = -1

MODE_CTC, MODE_ATTN = 0, 1


def scoring_mode(prediction):
    return MODE_ATTN if "Attn" in prediction else MODE_CTC


def canonical_table(converter, prediction):
    """int32 [C]: per class the canonical token (>= 0) or -2 for a class that decodes to a multi-character token.  The entries of
    the CTC blank (0) and of [EOS] are their own index: the kernel never looks them up."""
    mode = scoring_mode(prediction)
    handled = {0} if mode == MODE_CTC else {converter.dict["[EOS]"]}
    table = np.empty(len(converter.character), dtype=np.int32)
    for k, s in enumerate(converter.character):
        if k in handled:
            table[k] = k
        elif len(s) != 1:
            table[k] = MULTI_CHARACTER
        else:
            table[k] = converter.dict[s]
    return table


def canonical_labels(converter, labels, width):
    """raw label strings -> (int32 [B,width] canonical tokens, -1 = character not in the dictionary or padding; int32 [B] lengths)"""
    d = converter.dict
    rows = [[d.get(ch, NOT_IN_DICTIONARY) for ch in word] for word in labels]
    index = _padded_rows(rows, width, NOT_IN_DICTIONARY).numpy().astype(np.int32)
    lengths = np.fromiter((len(r) for r in rows), dtype=np.int32, count=len(rows))
    return index, lengths


def spells_eos(converter):
    """can single-character classes spell the string "[EOS]"?  The reference cuts at prd.find("[EOS]") on the decoded STRING
    (test.py:224), so such a character set can cut before the [EOS] token; the integer form cannot see that."""
    return all(ch in converter.dict for ch in "[]EOS")


def scoring_backend():
    """MRN_VALIDATION_SCORING = device (default) | host"""
    v = os.environ.get("MRN_VALIDATION_SCORING", "device")
    if v not in ("device", "host"):
        raise ValueError(f"MRN_VALIDATION_SCORING must be 'device' or 'host', got {v!r}")
    return v


def device_scoring_supported(converter, prediction, T, Lmax):
    """does mrn_greedy_score_f32 score a batch of T decoding steps and labels of up to Lmax characters"""
    if not (1 <= T <= SCORE_MAX_T and 0 <= Lmax <= SCORE_MAX_LABEL):
        return False
    if scoring_mode(prediction) == MODE_ATTN and spells_eos(converter):
        return False
    return scoring_backend() == "device"
