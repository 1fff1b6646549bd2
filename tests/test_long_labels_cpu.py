"""Label lengths on the CPU: the pure-Python predicate that picks the CTC kernel and refuses widths beyond the long one, the
refusal at the loss site (before anything is allocated or launched), and the C ABI of the long kernel's entry points."""
import pytest
import torch

from mrn_amd.modules.label_length import (CTC_MAX_LABEL_LENGTH, CTC_SHORT_MAX_LABEL_LENGTH, ctc_label_length_supported,
                                          ctc_uses_long_kernel, unsupported_label_length_message)


def test_limits():
    assert CTC_SHORT_MAX_LABEL_LENGTH == 31 and CTC_MAX_LABEL_LENGTH == 255


@pytest.mark.parametrize("n,supported,long_kernel", [(0, True, False), (1, True, False), (25, True, False), (31, True, False),
                                                      (32, True, True), (48, True, True), (63, True, True), (64, True, True),
                                                      (127, True, True), (128, True, True), (255, True, True),
                                                      (256, False, False), (1000, False, False), (-1, False, False)])
def test_predicate_boundaries(n, supported, long_kernel):
    assert ctc_label_length_supported(n) is supported
    assert ctc_uses_long_kernel(n) is long_kernel


def test_refusal_message_names_the_range():
    msg = unsupported_label_length_message(256)
    assert "batch_max_length" in msg and "0..255" in msg and "got 256" in msg


def test_ctc_loss_refuses_wide_targets_before_any_launch(monkeypatch):
    from mrn_amd import ops
    calls = []
    monkeypatch.setattr(ops, "call", lambda *a: calls.append(a))
    logits = torch.zeros(2, 63, 10)
    targets = torch.ones(2, 256, dtype=torch.long)
    with pytest.raises(NotImplementedError, match=r"batch_max_length \(padded target width\) in 0\.\.255; got 256"):
        ops.ctc_loss_fwd(logits, targets, torch.tensor([3, 300], dtype=torch.int32))
    assert calls == []


def test_long_entry_points_in_the_header():
    from mrn_amd import _lib
    protos = _lib.parse_header()
    assert protos["mrn_ctc_occ_floats_long"] == ("int64_t", ["int", "int", "int"], ["B", "T", "max_target_len"])
    fwd_short, fwd_long = protos["mrn_ctc_loss_fwd_f32"], protos["mrn_ctc_loss_fwd_long_f32"]
    assert fwd_long == fwd_short                                    # the long fwd is a drop-in for the 64-state one
    ret, types, names = protos["mrn_ctc_loss_bwd_long_f32"]
    assert ret == "int" and names[:8] == ["logits", "ld", "lse", "occ", "targets", "tstride", "target_len", "max_target_len"]
    assert names[-1] == "stream" and types[names.index("max_target_len")] == "int"
