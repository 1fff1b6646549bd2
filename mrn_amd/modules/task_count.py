"""Task counts the HIP path runs (pure Python: importable without a GPU).

The reference adds one frozen language expert per task to MRNNet and one extractor per task to DERNet, with no limit on how many
(modules/model.py: DM_Router(..., patch, len(self.model)), the fan-in over len(self.model) experts, DERNet.feature_dim = out_dim *
len(self.model)).  Here up to 16 tasks run on both nets.  The router kernels keep their 8-wide register form up to 8 experts and take
a 16-wide form from 9 to 16 (mrn_fanin_fwd_wide_f32 ...).  DERNet's attention head decodes over 256 * G context columns: while the
context of a 16-sample tile fits in LDS whole (G <= 7 at T = 65) the decoder runs as before, beyond that it forms and multiplies the
context in chunks of 1024 columns.
"""

MAX_TASKS = 16              # experts of MRNNet, extractors of DERNet
ROUTER_NARROW_MAX = 8       # expert counts the 8-wide router kernels take (mrn_fanin_fwd_f32 ...)


def tasks_supported(n):
    """does the HIP path run a net with n tasks (1 .. 16 experts / extractors)"""
    return 1 <= n <= MAX_TASKS


def router_uses_wide_kernels(n):
    """9 .. 16 experts take the 16-wide router kernels; up to 8 the 8-wide ones"""
    return ROUTER_NARROW_MAX < n <= MAX_TASKS


def unsupported_task_count_message(net, n):
    """the NotImplementedError text for adding a task beyond the ceiling"""
    return "HIP path supports 1..%d tasks (MRN experts / DER extractors); %s would have %d" % (MAX_TASKS, net, n)
