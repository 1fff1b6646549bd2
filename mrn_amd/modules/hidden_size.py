"""Hidden sizes the HIP path runs (pure Python: importable without a GPU).

The reference is generic in opt.hidden_size (modules/model.py: BidirectionalLSTM(..., opt.hidden_size, opt.hidden_size), nn.Linear(512,
opt.hidden_size) for SVTR, DM_Router(out_dim, 2 * out_dim, ...), DERNet.feature_dim = out_dim * len(self.model)).  Here the LSTM layer
kernels (csrc/lstm.hip, csrc/lstm_bwd.hip) are built for 128, 256 and 512 hidden units -- 8 waves of one 16-unit tile at 128, 16 waves at 256,
16 waves of two tiles each at 512 -- and with them the whole CTC family runs at those sizes: CRNN, and SVTR with its single Linear.  The
attention decoder (attn_decoder_kernel, csrc/attn_bwd.hip) is built for 256 only, so a net with the attention head runs 256 only.
"""

SUPPORTED_HIDDEN = (128, 256, 512)      # the LSTM layer kernels' instantiations; the CTC family's sizes
ATTN_HIDDEN = 256                       # the attention decoder's one size


def hidden_supported(sequence_modeling, prediction, hidden):
    """does the HIP path run a net of this SequenceModeling ("BiLSTM" / "None" / None) and Prediction ("CTC" / "Attn") at hidden_size
    `hidden`: 128, 256 and 512 with the CTC head, 256 only with the attention head"""
    if sequence_modeling not in ("BiLSTM", "None", None):
        return False
    if prediction == "CTC":
        return hidden in SUPPORTED_HIDDEN
    if prediction == "Attn":
        return hidden == ATTN_HIDDEN
    return False


def unsupported_hidden_message(sequence_modeling, prediction, hidden):
    """the NotImplementedError text for a hidden size the kernels are not built for"""
    return ("HIP path supports hidden_size in %s with the CTC head (BiLSTM or no SequenceModeling); the attention head runs %d only; "
            "SequenceModeling=%s Prediction=%s has hidden_size=%d"
            % (list(SUPPORTED_HIDDEN), ATTN_HIDDEN, sequence_modeling, prediction, hidden))


def check_hidden(sequence_modeling, prediction, hidden):
    """raise before any launch where a model learns its sizes"""
    if not hidden_supported(sequence_modeling, prediction, hidden):
        raise NotImplementedError(unsupported_hidden_message(sequence_modeling, prediction, hidden))
