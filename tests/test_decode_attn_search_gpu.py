"""The second decode of the evaluation forwards (attn_beam, attn_lexicon, attn_candidates, attn_shortlist; modules/decoding.py AttnSearch)
on Model, DERNet and MRNNet, along every branch MRNNet takes to its experts: tests/golden/attn_search.npz holds what the forwards
returned, and the library entry points they called, before the four keywords became one record (tests/golden/make_golden_attn_search.py
states the nets, the requests and the branches).  The call list and every integer output (beam_path, beam_word, index) must come back
exactly; a float output (beam_prob, the greedy logits) within the band tests/test_decode_attn_candidates_gpu.py holds a probability to,
|got - want| <= |want| * (exp(TOKEN_BAND) - 1) + 1e-37, so that an intended last-bit change in the backbone does not break this test.

The file's name puts it behind tests/test_bench_gpu.py in the suite, as tests/test_decode_attn_step_gpu.py's does: that file starts
bench.py as a child process and skips once the pytest process has initialised the GPU, which this test does."""
import os

import numpy as np
import pytest
import torch

from tests.golden.make_golden_attn_search import FLOATS, GROUPS, INTS, run
from tests.test_attn_beam_cpu import TOKEN_BAND

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", GROUPS)
def test_outputs_and_library_calls_are_the_recorded_parents(golden_dir, group):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd._lib import LIB
    LIB.load()
    ref = np.load(os.path.join(golden_dir, "attn_search.npz"))
    mine = {k for k in ref.files if k.startswith(group + "/")}
    got = run((group,))
    assert {k.split("@")[0] for k in got} == mine and any(k.endswith("/beam_word") for k in mine)
    for k, v in got.items():
        want = ref[k.split("@")[0]]
        what = k.split("@")[0].rsplit("/", 1)[1]
        if what == "calls":
            assert v == want.tolist(), f"{k}: not the library calls of parent {ref['parent']}"
        elif what in INTS:
            assert v.dtype == torch.from_numpy(want).dtype and np.array_equal(v.numpy(), want), f"{k}: differs from parent {ref['parent']}"
        else:
            assert what in FLOATS and v.dtype == torch.float32 and v.shape == want.shape, k
            err = np.abs(v.numpy().astype(np.float64) - want)
            band = np.abs(want.astype(np.float64)) * (np.exp(TOKEN_BAND) - 1) + 1e-37
            print(f"{k}: worst error {float((err / band).max()):.3f} of its band")
            assert np.all(err <= band), k
