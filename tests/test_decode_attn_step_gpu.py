"""The attention head's three decoder kernels (csrc/attn_decode.hip attn_decoder_kernel, attn_greedy_kernel, attn_beam_kernel) share one step;
tests/golden/attn_step.npz holds their outputs from before they did (tests/golden/make_golden_attn_step.py states the cases), and every
stored array must come back bit for bit: torch.equal, no tolerance.  A difference means a regrouped expression or a moved contraction.

The file's name puts it behind tests/test_bench_gpu.py in the suite, as tests/test_decode_attn_beam_gpu.py's does: that file starts
bench.py as a child process and skips once the pytest process has initialised the GPU, which this test does."""
import os

import numpy as np
import pytest
import torch

from tests.golden.make_golden_attn_step import run

pytestmark = pytest.mark.gpu


def test_every_output_is_bit_identical_to_the_recorded_parent(golden_dir):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mrn_amd import ops
    from mrn_amd._lib import LIB
    LIB.load()
    ref = np.load(os.path.join(golden_dir, "attn_step.npz"))
    got = run(ops)
    assert {k.split("@")[0] for k in got} == set(ref.files) - {"parent"}
    differ = [k for k, v in got.items() if not torch.equal(v, torch.from_numpy(ref[k.split("@")[0]]))]
    assert not differ, f"not bit-identical to parent {ref['parent']}: {differ}"
