"""Label lengths the HIP path's CTC loss takes (pure Python: importable without a GPU).

The reference's CTCLoss(zero_infinity=True) (il_modules/base.py:131) has no limit on the label length, and its datasets keep every
label up to batch_max_length (data/dataset.py:78-83).  Here the CTC loss runs two kernels, chosen from the padded target width
(the converter pads to batch_max_length, so the choice needs no device-to-host sync): the 64-state kernel up to 31 characters,
the long kernel (K states per lane) up to 255.  CTC greedy decoding without a loss, the attention head and CE take any length.
"""

CTC_SHORT_MAX_LABEL_LENGTH = 31      # 2L + 1 <= 64 states: mrn_ctc_loss_fwd_f32
CTC_MAX_LABEL_LENGTH = 255           # 2L + 1 <= 511 states: mrn_ctc_loss_fwd_long_f32


def ctc_label_length_supported(batch_max_length):
    """does the CTC loss take targets padded to batch_max_length (0 .. 255)"""
    return 0 <= batch_max_length <= CTC_MAX_LABEL_LENGTH


def ctc_uses_long_kernel(batch_max_length):
    """padded widths 32 .. 255 take the long kernel; up to 31 the 64-state kernel"""
    return CTC_SHORT_MAX_LABEL_LENGTH < batch_max_length <= CTC_MAX_LABEL_LENGTH


def unsupported_label_length_message(batch_max_length):
    """the NotImplementedError text for a CTC loss over targets wider than the long kernel takes"""
    return ("HIP CTC loss supports batch_max_length (padded target width) in 0..%d; got %d (the attention head and CTC decoding "
            "without a loss take any length)" % (CTC_MAX_LABEL_LENGTH, batch_max_length))
