"""Model containers with the reference's four-stage operator API (modules/model.py): Model_Extractor (:17-101),
Model (:105-199), MRNNet (:314-496).  Same constructor arguments (`opt`), attribute names, forward signatures,
return conventions and state_dict keys; the math runs on the HIP path.

MI355X-first differences that do not change results:
  * experts write their contextual features straight into one [B, P, I, C] buffer and their logits into
    16-byte-aligned padded rows, so torch.stack / pad-with-ones / permute / contiguous / sum of
    MRNNet.cross_forward (:399-423) collapse into the DM-Router kernels plus one fan-in pass;
  * the input image is converted to NHWC once and shared by all experts.
"""
import contextlib
import copy
import os

import torch
import torch.nn as nn

from .. import ops
from ..functional import FaninFn, GateTailFn, HeightMeanFn, LinearFn, needs_grad
from ._nn import to_nhwc
from .decoding import ATTN_EOS, attn_search_request
from .dm_router import DM_Router
from .feature_extraction import ResNet_FeatureExtractor, VGG_FeatureExtractor
from .geometry import check_call, frames
from .prediction import Attention
from .sequence_modeling import BidirectionalLSTM
from .hidden_size import check_hidden
from .task_count import tasks_supported, unsupported_task_count_message
from .transformation import TPS_SpatialTransformerNetwork



# Loop B: the heads of the frozen experts (BiLSTM x 2 + attention decoder / CTC Linear: latency-bound launches of 64-192 workgroups,
# 8 ms of a TRBA x 6 step) run on a stream of their own behind their backbones, so that the NEXT batch's backbones -- issued one step
# ahead by experts_prefetch -- start as soon as this batch's backbones are done instead of queueing behind its recurrences.
# MRN_HEADS_STREAM=0/1 is the A/B switch.
HEADS_STREAM = os.environ.get("MRN_HEADS_STREAM", "1") == "1"

class Model_Extractor(nn.Module):
    def __init__(self, opt):
        super().__init__()
        check_hidden(opt.SequenceModeling, opt.Prediction, opt.hidden_size)      # (before anything is built or launched)
        self.opt = opt
        self.stages = {"Trans": opt.Transformation, "Feat": opt.FeatureExtraction, "Seq": opt.SequenceModeling,
                       "Pred": opt.Prediction}
        if opt.Transformation == "TPS":
            self.Transformation = TPS_SpatialTransformerNetwork(
                F=opt.num_fiducial, I_size=(opt.imgH, opt.imgW), I_r_size=(opt.imgH, opt.imgW),
                I_channel_num=opt.input_channel)
        else:
            print("No Transformation module specified")
        if opt.FeatureExtraction == "VGG":
            self.FeatureExtraction = VGG_FeatureExtractor(opt.input_channel, opt.output_channel)
        elif opt.FeatureExtraction == "ResNet":
            self.FeatureExtraction = ResNet_FeatureExtractor(opt.input_channel, opt.output_channel)
        elif opt.FeatureExtraction == "RCNN":
            from .feature_extraction import RCNN_FeatureExtractor
            self.FeatureExtraction = RCNN_FeatureExtractor(opt.input_channel, opt.output_channel)
        elif opt.FeatureExtraction == "SVTR":
            from .svtr import SVTR_FeatureExtractor
            self.FeatureExtraction = SVTR_FeatureExtractor(opt.input_channel, opt.output_channel)
        else:
            raise Exception("No FeatureExtraction module specified")
        self.FeatureExtraction_output = opt.output_channel
        self.AdaptiveAvgPool = nn.AdaptiveAvgPool2d((None, 1))
        if opt.SequenceModeling == "BiLSTM":
            self.SequenceModeling = nn.Sequential(
                BidirectionalLSTM(self.FeatureExtraction_output, opt.hidden_size, opt.hidden_size),
                BidirectionalLSTM(opt.hidden_size, opt.hidden_size, opt.hidden_size))
        else:
            self.SequenceModeling = nn.Sequential(nn.Linear(self.FeatureExtraction_output, opt.hidden_size))
            print("No SequenceModeling module specified")
        self.SequenceModeling_output = opt.hidden_size

    def visual(self, image):
        """Transformation + FeatureExtraction (+ the reference's permute / AdaptiveAvgPool / squeeze): [B,C,H,W] -> [B,T,C']"""
        check_call(self.stages["Trans"], self.stages["Feat"], image.shape[0], image.shape[2], image.shape[3])     # (before any launch)
        with ops.batch_counters():                           # (the train-mode BatchNorm layers' num_batches_tracked: one launch)
            if not self.stages["Trans"] == "None":
                image = self.Transformation(image)
            fmap = self.FeatureExtraction(image)             # logical [B,C,H,W], NHWC memory
        B, C, H, W = fmap.shape
        if H == 1:
            # permute(0,3,1,2) + AdaptiveAvgPool((None,1)) + squeeze(3) of the reference is the identity on [B,1,W,C]
            return to_nhwc(fmap).view(B, W, C)
        x = to_nhwc(fmap)                                    # 48- / 64-pixel inputs: the mean over the map's 2 / 3 rows
        if torch.is_grad_enabled() and x.requires_grad:
            return HeightMeanFn.apply(x)
        return ops.height_mean(x)

    def sequence(self, visual, out=None):
        """SequenceModeling stage: [B,T,C'] -> [B,T,hidden]; `out` = optional (strided) destination."""
        if self.stages["Seq"] == "BiLSTM":
            x = self.SequenceModeling[0](visual)
            return self.SequenceModeling[1](x, out=out)
        lin = self.SequenceModeling[0]
        if needs_grad(lin, visual):
            return LinearFn.apply(visual, lin.weight, lin.bias)
        return ops.linear(visual, lin.weight, lin.bias, out=out)

    def forward(self, image, out=None):
        """image [B,C,H,W] -> contextual feature [B,T,hidden]"""
        return self.sequence(self.visual(image), out=out)


class Model(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.model = Model_Extractor(opt)
        self.SequenceModeling_output = self.model.SequenceModeling_output
        self.stages = {"Pred": opt.Prediction}
        self.fc = None
        self.Prediction = None

    def reset_class(self, opt, device):
        if opt.Prediction == "CTC":
            self.Prediction = nn.Linear(self.SequenceModeling_output, opt.num_class)
        elif opt.Prediction == "Attn":
            self.Prediction = Attention(self.SequenceModeling_output, opt.hidden_size, opt.num_class,
                                        nn.Linear(opt.hidden_size, opt.num_class))
        else:
            raise Exception("Prediction is neither CTC or Attn")
        self.Prediction.to(device)

    def forward(self, image, text=None, is_train=True, feature_out=None, predict_out=None, attn_beam=None, attn_lexicon=None,
                attn_candidates=None, attn_shortlist=None, search=None, attn_lm=None):
        """attn_beam (a width; attention head, evaluation under no_grad): the dict also has beam_path / beam_prob [B,S], the best entry
        of a beam search on the same features (modules/decoding.py) -- one more launch, `predict` is still the greedy decoder's.
        attn_lexicon (the handle of ops.upload_trie, beside attn_beam): the search is walked along the lexicon's trie, and the dict
        also has beam_word [B], the lexicon index of the best entry (-1: no word of the lexicon can be spelled).  attn_candidates (the
        handle of ops.upload_words(...).with_cand(...); instead of attn_beam): every sample's candidate words are scored exactly
        (Attention.score_candidates) and the same three keys hold the best word's pair and its table index.  attn_shortlist ((the
        handle of ops.upload_words, K, max_dist or None); instead of both): the K words nearest to the greedy hypothesis (the arg-max
        of `predict`) are scored exactly (Attention.shortlist_search) and the same three keys hold the best one.  attn_lm ((the handle of
        ops.upload_char_lm, lm_weight, lm_bonus, top_n), beside attn_beam and nothing else): the beam search is fused with that
        character n-gram model and beam_path / beam_prob are those of the best entry by the fused key.  search: the five as the
        decoding.AttnSearch an MRNNet has resolved already"""
        if search is None:
            search = attn_search_request(self.stages["Pred"], is_train, attn_beam, attn_lexicon, attn_candidates, attn_shortlist, attn_lm)
        return self.heads(self.model.visual(image), text, is_train, feature_out, predict_out, search=search)

    def _second_decode(self, out, search, feat, text, logits):
        """the beam_path / beam_prob (and beam_word) of a forward's dict: `search` (a decoding.AttnSearch or None) on the features the
        greedy decode ran on; a shortlist's hypothesis is the arg-max of the greedy logits"""
        if search is not None:
            tokens = ops.argmax_lastdim(logits) if search.kind == "shortlist" else None
            out["beam_path"], out["beam_prob"], word = self.Prediction.search(search, feat, text, self.opt.batch_max_length, tokens=tokens)
            if search.has_word:
                out["beam_word"] = word
        return out

    def heads(self, visual, text=None, is_train=True, feature_out=None, predict_out=None, search=None):
        """SequenceModeling + Prediction on precomputed backbone features; search: a decoding.AttnSearch (Model.forward explains the
        keys it adds to the dict)"""
        feat = self.model.sequence(visual, out=feature_out)
        if self.stages["Pred"] == "CTC":
            if needs_grad(self.Prediction, feat):
                pred = LinearFn.apply(feat, self.Prediction.weight, self.Prediction.bias)
            else:
                pred = ops.linear(feat, self.Prediction.weight, self.Prediction.bias, out=predict_out)
        else:
            pred = self.Prediction(feat, text, is_train, batch_max_length=self.opt.batch_max_length, out=predict_out)
        return self._second_decode({"predict": pred, "feature": feat}, search, feat, text, pred)

    def update_fc(self, hidden_size, nb_classes, device=None):
        fc = nn.Linear(hidden_size, nb_classes)
        if self.fc is not None:
            nb_output = self.fc.out_features
            fc = fc.to(self.fc.weight.device)
            fc.weight.data[:nb_output] = self.fc.weight.data
            fc.bias.data[:nb_output] = self.fc.bias.data
        self.fc = fc

    def new_fc(self, hidden_size, nb_classes):
        self.fc = nn.Linear(hidden_size, nb_classes)

    def weight_align(self, increment):
        """rescale the newest `increment` rows of fc so their mean L2 norm matches the old rows' (reference :166-174)"""
        gamma = ops.weight_align_(self.fc.weight.data, increment)
        torch.autograd.graph.increment_version(self.fc.weight)      # written through a raw pointer: invalidate repacked copies
        print("alignweights,gamma=", float(gamma))
        return gamma

    def build_prediction(self, opt, num_class):
        if opt.Prediction == "CTC":
            self.Prediction = self.fc
        elif opt.Prediction == "Attn":
            self.Prediction = Attention(self.SequenceModeling_output, opt.hidden_size, num_class, self.fc)
        else:
            raise Exception("Prediction is neither CTC or Attn")

    def copy(self):
        return copy.deepcopy(self)

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        return self


class DERNet(Model):
    """Dynamically expanding network (reference modules/model.py:203-312): one Model_Extractor per task, features
    concatenated on the channel axis, main head over all of them, auxiliary head over the newest out_dim (= hidden_size)."""

    def __init__(self, opt):
        super().__init__(opt)
        self.model = nn.ModuleList()
        self.out_dim = None
        self.fc = None
        self.aux_fc = None
        self.task_sizes = []
        self.expert_grouping = True         # frozen extractors run their conv backbones in lock-step
        self.frozen_stream = True           # ... on their own HIP stream, side by side with the trained extractor's forward
        self._group = None
        self._side = None

    @property
    def feature_dim(self):
        return 0 if self.out_dim is None else self.out_dim * len(self.model)

    def _frozen_lockstep(self, image):
        """(frozen indices, BackboneGroup, SequenceGroup) when the frozen extractors can run conv backbones AND BiLSTMs in lock-step
        and occupy one contiguous channel range of the feature buffer; else None"""
        from . import expert_group
        trainable = [needs_grad(ext, image) for ext in self.model]
        frozen = [i for i, t in enumerate(trainable) if not t]
        if not (self.expert_grouping and len(frozen) >= 2):
            return None
        exts = [self.model[i] for i in frozen]
        key = tuple(id(e) for e in exts)
        if self._group is None or self._group[0] != key:
            self._group = (key, expert_group.BackboneGroup(exts), expert_group.SequenceGroup(exts))
        if not expert_group.supported(exts):
            return None
        if not (expert_group.SequenceGroup.sequence_supported(exts) and frozen == list(range(frozen[0], frozen[0] + len(frozen)))):
            return (frozen, self._group[1], None)
        return (frozen, self._group[1], self._group[2])

    def _run_frozen(self, image, frozen, bg, sg):
        """the frozen group's slices of a fresh [B,T,out_dim*N] feature buffer (current stream)"""
        with torch.no_grad():
            stack = bg.visual_all(image, as_act=True)
            _, B, _, T, _ = stack.shape
            buf = torch.empty(B, T, self.feature_dim, device=image.device, dtype=torch.float32)
            sg.sequence(stack, out=buf[:, :, frozen[0] * self.out_dim:], out_row_stride=self.feature_dim, out_group_stride=self.out_dim)
        return buf

    def frozen_prefetch(self, image):
        """Issue the FROZEN extractors' forward of a (future) batch on the side stream; pass the handle to
        forward(..., frozen=handle).  They are frozen and in eval mode (reference il_modules/der.py:101-104,137-141), so their
        features for batch n+1 do not depend on the update of batch n: only the launch order changes.  None when the frozen
        extractors cannot run in lock-step (the caller then simply does not pass a handle)."""
        check_call(self.opt.Transformation, self.opt.FeatureExtraction, image.shape[0], image.shape[2], image.shape[3])
        image = to_nhwc(image).permute(0, 3, 1, 2)
        plan = self._frozen_lockstep(image)
        if plan is None or plan[2] is None or not (self.frozen_stream and image.is_cuda):
            return None
        if self._side is None:
            self._side = ops.aux_stream(0, image.device)
        side = self._side
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            buf = self._run_frozen(image, *plan)
            done = torch.cuda.Event()
            done.record(side)
        image.record_stream(side)
        return {"buf": buf, "done": done, "batch": image.shape[0], "frozen": plan[0]}

    def _features(self, image, frozen_handle=None):
        """[B,T,out_dim*N]: frozen extractors write straight into their channel slice (no torch.cat pass); two or more
        frozen extractors of one architecture run conv backbones and BiLSTMs in lock-step (modules/expert_group.py), on a side
        stream next to the trained extractor's forward -- or earlier still, through frozen_prefetch()"""
        check_call(self.opt.Transformation, self.opt.FeatureExtraction, image.shape[0], image.shape[2], image.shape[3])
        image = to_nhwc(image).permute(0, 3, 1, 2)
        trainable = [needs_grad(ext, image) for ext in self.model]
        visuals, seq_done, buf, join = {}, set(), None, None
        if frozen_handle is not None:
            assert frozen_handle["batch"] == image.shape[0]
            buf, join, seq_done = frozen_handle["buf"], frozen_handle["done"], set(frozen_handle["frozen"])
        else:
            plan = self._frozen_lockstep(image)
            if plan is not None and plan[2] is not None:
                # the frozen group is independent of the trained extractor until the heads: its (MFMA-bound) convolutions share
                # the chip with the trained extractor's forward, whose BatchNorm / pooling passes are HBM-bound
                if self.frozen_stream and any(trainable) and image.is_cuda:
                    handle = self.frozen_prefetch(image)
                    buf, join = handle["buf"], handle["done"]
                else:
                    buf = self._run_frozen(image, *plan)
                seq_done = set(plan[0])
            elif plan is not None:
                with torch.no_grad():
                    stack = plan[1].visual_all(image)
                visuals = {i: stack[k] for k, i in enumerate(plan[0])}
        trained = {i: ext(image) for i, ext in enumerate(self.model) if trainable[i]}      # (main stream; the side stream runs)
        if join is not None:
            main = torch.cuda.current_stream()
            main.wait_event(join)
            buf.record_stream(main)
        outs = []
        for i, ext in enumerate(self.model):
            if trainable[i]:
                outs.append(trained[i])
                continue
            with torch.no_grad():
                if i not in seq_done:
                    vis = visuals[i] if i in visuals else ext.visual(image)
                    if buf is None:
                        buf = torch.empty(vis.shape[0], vis.shape[1], self.feature_dim, device=vis.device, dtype=torch.float32)
                    ext.sequence(vis, out=buf[:, :, i * self.out_dim:(i + 1) * self.out_dim])
                outs.append(buf[:, :, i * self.out_dim:(i + 1) * self.out_dim])
        return buf if not any(trainable) else torch.cat(outs, -1)

    def _head(self, head, feat, text, is_train):
        if self.stages["Pred"] == "CTC":
            if needs_grad(head, feat):
                return LinearFn.apply(feat, head.weight, head.bias)
            return ops.linear(feat, head.weight, head.bias)
        return head(feat if feat.is_contiguous() else feat.contiguous(), text, is_train, batch_max_length=self.opt.batch_max_length)

    def forward(self, image, text=None, is_train=True, frozen=None, attn_beam=None, attn_lexicon=None, attn_candidates=None,
                attn_shortlist=None, attn_lm=None):
        """frozen: optional handle of frozen_prefetch(image) (same batch); attn_beam, attn_lexicon, attn_candidates, attn_shortlist,
        attn_lm: as Model.forward (the main head's pair and beam_word)"""
        search = attn_search_request(self.stages["Pred"], is_train, attn_beam, attn_lexicon, attn_candidates, attn_shortlist, attn_lm)
        feat = self._features(image, frozen)
        logits = self._head(self.Prediction, feat, text, is_train)
        aux = self._head(self.aux_Prediction, feat[:, :, -self.out_dim:], text, is_train)
        out = {"logits": logits, "aux_logits": aux, "features": feat}
        rows = feat if search is None or feat.is_contiguous() else feat.contiguous()
        return self._second_decode(out, search, rows, text, logits)

    def update_fc(self, hidden_size, nb_classes, device=None):
        if not tasks_supported(len(self.model) + 1):
            raise NotImplementedError(unsupported_task_count_message("DERNet", len(self.model) + 1))
        check_hidden(self.opt.SequenceModeling, self.opt.Prediction, self.opt.hidden_size)
        dev = next(self.parameters()).device if len(self.model) else None
        self.model.append(Model_Extractor(self.opt))
        if len(self.model) > 1:
            self.model[-1].load_state_dict(self.model[-2].state_dict())
        if self.out_dim is None:
            self.out_dim = self.model[-1].SequenceModeling_output
        fc = nn.Linear(self.feature_dim if self.opt.Prediction == "CTC" else self.out_dim, nb_classes)
        if self.fc is not None:                       # keep the old classes' rows over the old extractors' columns
            old_w, old_b = self.fc.weight.data.cpu(), self.fc.bias.data.cpu()
            ncol = min(old_w.shape[1], self.feature_dim - self.out_dim, fc.weight.shape[1])
            fc.weight.data[:old_w.shape[0], :ncol] = old_w[:, :ncol]
            fc.bias.data[:old_b.shape[0]] = old_b
        self.fc = fc
        self.aux_fc = nn.Linear(self.out_dim, nb_classes)
        if dev is not None:
            self.to(dev)

    def build_prediction(self, opt, num_class):
        if opt.Prediction == "CTC":
            self.Prediction = self.fc
        elif opt.Prediction == "Attn":
            self.Prediction = Attention(self.feature_dim, opt.hidden_size, num_class, self.fc)
        else:
            raise Exception("Prediction is neither CTC or Attn")
        if len(self.model) > 1:
            self.Prediction.to(next(self.model[0].parameters()).device)

    def build_aux_prediction(self, opt, num_class):
        if opt.Prediction == "CTC":
            self.aux_Prediction = self.aux_fc
        elif opt.Prediction == "Attn":
            self.aux_Prediction = Attention(self.SequenceModeling_output, opt.hidden_size, num_class, self.aux_fc)
        else:
            raise Exception("Prediction is neither CTC or Attn")
        if len(self.model) > 1:
            self.aux_Prediction.to(next(self.model[0].parameters()).device)

    def freeze_conv(self):
        for p in self.model.parameters():
            p.requires_grad = False
        self.model.eval()

    def copy(self):
        group, self._group = self._group, None               # packed-weight caches / the side stream are not copied
        side, self._side = self._side, None
        try:
            return copy.deepcopy(self)
        finally:
            self._group = group
            self._side = side


class MRNNet(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.model = nn.ModuleList()
        self.out_dim = None
        self.fc = None
        self.opt = opt
        self.task_sizes = []
        self.patch = frames(opt.FeatureExtraction, opt.imgW)      # router tokens = frames of an imgW-pixel line (63 / 64 / 65 at 256)
        self.router = "dm-router"
        self.layer_num = 1
        self.beta = 1
        self.expert_streams = True          # run the frozen experts on separate HIP streams
        self.expert_grouping = True         # run the frozen experts' conv backbones in lock-step (modules/expert_group.py)
        self._stream_pool = []
        self._group = None
        self._heads = None
        self._halves = None
        # concurrent lock-step sub-groups: -1 = by backbone family (convolutional experts: ONE group; SVTR: three groups of >= 2 from six
        # experts on, two from four on), 0 = off (one group on the caller's stream), k >= 2 = exactly k
        self.expert_halves = int(os.environ.get("MRN_EXPERT_HALVES", "-1"))
        #   (measured on TRBA x 6, MI355X: 1 group 1.00, 2 halves on two streams 1.044, 3 thirds 1.015, staggered halves 1.035,
        #    halves with one high-priority stream 0.96; with the final conv kernel and the loop-B pipeline: one group on a
        #    side stream 0.992 of two halves)

    def _streams(self, n, device):
        while len(self._stream_pool) < n:
            self._stream_pool.append(ops.aux_stream(len(self._stream_pool), device))      # (process-wide: see ops.aux_stream)
        return self._stream_pool

    def _backbone_group(self):
        """BackboneGroup over the current experts when they can run in lock-step, else None (per-expert path)"""
        from . import expert_group
        if not self.expert_grouping:
            return None
        extractors = [e.model for e in self.model]
        key = tuple(id(e) for e in extractors)
        if self._group is None or self._group[0] != key:
            self._group = (key, expert_group.BackboneGroup(extractors))
        return self._group[1] if expert_group.supported(extractors) else None

    def _half_groups(self, is_train):
        """[(lo, hi, BackboneGroup, HeadsGroup)] per sub-group when the experts are split into `expert_halves` lock-step
        groups that run on separate streams, else None.  Fewer than two experts per sub-group: ONE group on one side stream,
        so that the loop-B software pipeline (experts_prefetch) still overlaps the router phase with the next batch's experts."""
        from . import expert_group
        I = len(self.model)
        k = self.expert_halves
        if k < 0:
            # default: ONE lock-step group of all experts on one side stream.  Sub-groups on separate streams (MRN_EXPERT_HALVES=2 / 3) were
            # the default while the convolution kernels left CU resources to share; the row-block Winograd kernel owns its CU (144 KiB of
            # LDS, 453 registers), so sub-groups only add tile-quantisation tails: same box 90.7 -> 89.7 ms for six TRBA experts, and every
            # launch has the GPU to itself (in-situ rate of the dominant kernel 0.25 -> 0.325 of peak).  SVTR's kernels share a CU, and its
            # experts keep their sub-groups (same box, six experts: one group 23.5-23.6 ms, three 22.4-22.6)
            svtr = I > 0 and self.model[0].model.stages.get("Feat") == "SVTR"
            k = (3 if I >= 6 else 2) if svtr else I
        if k < 2 or I < 2:
            return None
        if I < 2 * k:
            k = 1
        key = tuple(id(e) for e in self.model) + (k,)
        if self._halves is None or self._halves[0] != key:
            cuts = [I * i // k for i in range(k + 1)]
            parts = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                models = list(self.model)[lo:hi]
                parts.append((lo, hi, expert_group.BackboneGroup([m.model for m in models]), expert_group.HeadsGroup(models)))
            self._halves = (key, parts)
        return self._halves[1]

    def _heads_group(self, group, is_train):
        """HeadsGroup (SequenceModeling + Prediction of all experts in lock-step) when `group` exists and the heads allow it"""
        from .expert_group import HeadsGroup
        if group is None or not (HeadsGroup.supported(list(self.model), is_train) or self._greedy_heads(is_train)):
            return None
        if self._heads is None or self._heads[0] is not group:
            self._heads = (group, HeadsGroup(list(self.model)))
        return self._heads[1]

    @property
    def feature_dim(self):
        return 0 if self.out_dim is None else self.out_dim * len(self.model)

    def _greedy_heads(self, is_train):
        """attention experts at evaluation time decode greedily in lock-step (HeadsGroup.run_greedy: one launch for all of them) unless
        MRN_GREEDY_DECODE=stepwise asks for the per-expert step loop"""
        from .expert_group import HeadsGroup
        return (not is_train and self.opt.Prediction == "Attn" and ops.greedy_decode_mode() == "fused"
                and HeadsGroup.greedy_supported(list(self.model)))

    def _run_heads(self, hg, visual, text, is_train, feats, logits, search=None, parts=None, first=0):
        """search (a decoding.AttnSearch) with parts (a list): the list takes (first expert, path [G,B,S], prob [G,B,S], word [G,B] or
        None) of the group's second decode; for a shortlist (first expert, the group, (its features, Hproj, start and operand
        columns)), what run_search scores a candidate table with once the routing index has given the hypotheses"""
        if not self._greedy_heads(is_train):
            hg.run(visual, text, feats, logits)
        elif search is not None and search.kind == "shortlist":
            kept = []
            hg.run_greedy(visual, text, feats, logits, keep=kept)
            parts.append((first, hg, tuple(kept)))
        else:
            best = hg.run_greedy(visual, text, feats, logits, search=search)
            if search is not None:
                parts.append((first,) + best)

    def forward(self, image, cross=True, text=None, is_train=True, experts=None, attn_beam=None, attn_lexicon=None, attn_candidates=None,
                attn_shortlist=None, attn_lm=None):
        """`experts`: optional handle from experts_prefetch() -- the frozen experts' outputs for THIS batch, issued earlier.
        attn_beam (a width; attention experts, evaluation under no_grad): the dict also has beam_path / beam_prob [B,S], the best entry of
        a beam search (modules/decoding.py) of the expert the hard routing index picks for each sample, for cross=False of the newest
        expert; one more launch per heads group on the same features, `logits` is still the greedy decoder's.  attn_lexicon (the handle
        of ops.upload_trie, beside attn_beam): the search of every expert is walked along the one trie, and the dict also has beam_word
        [B], as Model.forward.  attn_candidates (the handle of ops.upload_words(...).with_cand(...); instead of attn_beam): every sample's
        candidate words are scored exactly under ALL experts in one grouped launch per heads group (a word with a class an expert lacks
        is dead for that expert) and the same three keys hold the routed expert's best word.  attn_shortlist ((the handle of
        ops.upload_words, K, max_dist or None); instead of both): the candidate table is the shortlist of the ROUTED expert's greedy
        hypothesis (the arg-max of `logits`), one table per batch, scored under all experts like attn_candidates'.  attn_lm ((the handle
        of ops.upload_char_lm, lm_weight, lm_bonus, top_n), beside attn_beam and nothing else): every expert's beam search is fused with
        the one model in the grouped launch, and the pair is the routed expert's best entry by the fused key"""
        check_call(self.opt.Transformation, self.opt.FeatureExtraction, image.shape[0], image.shape[2], image.shape[3])
        search = attn_search_request(self.opt.Prediction, is_train, attn_beam, attn_lexicon, attn_candidates, attn_shortlist, attn_lm)
        best = None
        if cross == False:  # noqa: E712  (learners pass cross positionally, exactly as in the reference)
            newest = self.model[-1](image, text, is_train, search=search)
            features, index = newest["predict"], None
            if search is not None:
                best = (newest["beam_path"], newest["beam_prob"], newest.get("beam_word"))
        elif is_train == False:  # noqa: E712
            routed = self.cross_forward_expert(image, text, is_train, search=search)
            features, index = routed[:2]
            if search is not None:
                best = routed[2]
        else:
            features, index = self.cross_forward(image, text, is_train, experts=experts)
        out = {"logits": features, "index": index, "aux_logits": None}
        if best is not None:
            out["beam_path"], out["beam_prob"] = best[:2]
            if search.has_word:
                out["beam_word"] = best[2]
        return out

    # -- shared by both routed paths -------------------------------------------------------------------
    def experts_prefetch(self, image, text=None, is_train=True):
        """Issue the FROZEN experts' forward for a batch on the side streams and return a handle for
        forward(..., experts=handle) -- or None when the experts cannot run as lock-step half-groups.

        In the router phase the experts do not depend on the router being trained, so a learner can issue batch n+1's
        expert forward before batch n's router forward / backward / Adam: the side streams then run it while the main
        stream is busy with the router.  The side streams wait only for the inputs (an event recorded after the NHWC
        conversion), every output lives in the issuing stream's allocator pool, and the consumer waits on per-half
        events, so nothing orders the prefetch behind the router work of the previous step."""
        I = len(self.model)
        check_call(self.opt.Transformation, self.opt.FeatureExtraction, image.shape[0], image.shape[2], image.shape[3])
        with torch.no_grad():
            group = self._backbone_group() if I > 1 else None
            halves = self._half_groups(is_train) if self._heads_group(group, is_train) is not None else None
            if halves is None:
                return None
            B, dev = image.shape[0], image.device
            img = to_nhwc(image).permute(0, 3, 1, 2)
            T_pred = self.patch if self.opt.Prediction == "CTC" else self.opt.batch_max_length + 1
            main = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record(main)
            # the heads on a stream of their own (see HEADS_STREAM) when the experts run as ONE lock-step group (convolutional experts;
            # measured, same box: CRNN x 3 11.23 -> 10.80 ms, TRBA x 6 unchanged -- the row-block kernel is power-bound and the
            # recurrences take their CUs from it; SVTR's three sub-groups already interleave: 21.4 -> 21.9 with six streams, not split)
            split = HEADS_STREAM and len(halves) == 1
            streams = self._streams(len(halves) * (2 if split else 1), dev)
            # the router's [B,P,I,C] feature tensor is allocated ONCE (issuing stream's pool) and every sub-group writes its experts'
            # slice of it: no concatenation launch when the router phase adopts the outputs
            feats = torch.empty(B, self.patch, I, self.out_dim, device=dev, dtype=torch.float32)
            parts = []
            for k, (lo, hi, bg, hg) in enumerate(halves):
                st = streams[k]
                sh = streams[len(halves) + k] if split else st
                st.wait_event(ready)
                with torch.cuda.stream(st):
                    visual = bg.visual_all(img, as_act=True)
                    if split:
                        grown = torch.cuda.Event()
                        grown.record(st)
                if split:
                    sh.wait_event(grown)
                    for t in (visual.f32, visual.hl):
                        if t is not None:
                            t.record_stream(sh)          # (allocated in the backbone stream's pool, read by the heads' stream)
                with torch.cuda.stream(sh):
                    lg = [ops.padded_rows(B, T_pred, e.fc.out_features, dev) for e in list(self.model)[lo:hi]]
                    self._run_heads(hg, visual, text, is_train, feats[:, :, lo:hi, :], lg)
                    done = torch.cuda.Event()
                    done.record(sh)
                for t in (img, image, text, feats):
                    if t is not None:
                        t.record_stream(st)
                        if split:
                            t.record_stream(sh)
                parts.append((lg, done))
            return {"parts": parts, "batch": B, "feats": feats}

    def _experts_and_gate(self, image, text, is_train, experts=None, search=None, parts=None):
        """search (a decoding.AttnSearch) with parts (an empty list): the list takes _run_heads' record per heads group, or per expert
        (expert, path [1,B,S], prob [1,B,S], word [1,B] or None) from its own forward.  For a shortlist nothing more is launched: the
        list takes what _shortlist_best scores the table with, _run_heads' record or (expert, None, its features [B,T,D])"""
        I = len(self.model)

        def expert_part(i, res):
            if search is not None and search.kind == "shortlist":
                parts.append((i, None, feats[:, :, i, :]))
            elif search is not None:
                word = res["beam_word"].unsqueeze(0) if search.has_word else None
                parts.append((i, res["beam_path"].unsqueeze(0), res["beam_prob"].unsqueeze(0), word))

        own = None if search is None or search.kind == "shortlist" else search      # what an expert's own forward decodes
        B = image.shape[0]
        dev = image.device
        if experts is not None:
            # outputs of experts_prefetch(): wait for the two half-groups, adopt their buffers on this stream
            assert experts["batch"] == B
            main = torch.cuda.current_stream()
            logits = []
            for lg, done in experts["parts"]:
                main.wait_event(done)
                for l in lg:
                    l.record_stream(main)
                logits += lg
            feats = experts["feats"]
            feats.record_stream(main)
            r = self.dm_router[0].forward_l2(feats)
            r = LinearFn.apply(r.view(B * self.patch, I * self.out_dim), self.channel_route.weight, self.channel_route.bias)
            return logits, r.view(B, self.patch, I)
        image = to_nhwc(image).permute(0, 3, 1, 2)          # one NHWC conversion shared by all experts
        T_pred = self.patch if self.opt.Prediction == "CTC" else self.opt.batch_max_length + 1
        feats = torch.empty(B, self.patch, I, self.out_dim, device=dev, dtype=torch.float32)
        logits = [ops.padded_rows(B, T_pred, expert.fc.out_features, dev) for expert in self.model]
        with torch.no_grad():
            group = self._backbone_group() if I > 1 else None
            heads = self._heads_group(group, is_train)
            halves = self._half_groups(is_train) if heads is not None else None
            if halves is not None:
                # two lock-step half-groups on two HIP streams: while one half's convolutions keep the matrix pipes busy,
                # the other half's HBM-bound BatchNorm / pooling passes and latency-bound recurrences share the CUs
                main = torch.cuda.current_stream()
                streams = self._streams(len(halves), dev)
                for (lo, hi, bg, hg), st in zip(halves, streams):
                    st.wait_stream(main)
                    with torch.cuda.stream(st):
                        self._run_heads(hg, bg.visual_all(image, as_act=True), text, is_train, feats[:, :, lo:hi, :], logits[lo:hi],
                                        search=search, parts=parts, first=lo)
                for st in streams[:len(halves)]:
                    main.wait_stream(st)
                    image.record_stream(st)
            elif heads is not None:
                # backbones AND heads in lock-step: one grouped launch per conv layer / Linear / recurrence, one stream
                self._run_heads(heads, group.visual_all(image, as_act=True), text, is_train, feats, logits, search=search, parts=parts)
            elif self.expert_streams and I > 1:
                # Phase 1, one stream: the conv backbones (grouped when the experts allow it, else one after the other).
                # Phase 2, one HIP stream per expert: BiLSTM / attention decoder are latency-bound launches of 16-32
                # workgroups each; the experts' recurrences run side by side instead of idling 90 % of the CUs.
                if group is not None:
                    stack = group.visual_all(image)                      # [I,B,T,C']
                    visuals = [stack[i] for i in range(I)]
                else:
                    visuals = None                                       # (SVTR: many small launches per expert -- whole
                main = torch.cuda.current_stream()                       #  experts run side by side, one stream each)
                streams = self._streams(I, dev)
                for i, expert in enumerate(self.model):
                    streams[i].wait_stream(main)
                    with torch.cuda.stream(streams[i]):
                        if visuals is None:
                            res = expert(image, text, is_train, feature_out=feats[:, :, i, :], predict_out=logits[i], search=own)
                        else:
                            res = expert.heads(visuals[i], text, is_train, feature_out=feats[:, :, i, :], predict_out=logits[i], search=own)
                            visuals[i].record_stream(streams[i])
                        expert_part(i, res)
                for st in streams[:I]:
                    main.wait_stream(st)
                    image.record_stream(st)
            else:
                for i, expert in enumerate(self.model):
                    expert_part(i, expert(image, text, is_train, feature_out=feats[:, :, i, :], predict_out=logits[i], search=own))
        r = self.dm_router[0].forward_l2(feats)               # [B,P,I,C]
        r = LinearFn.apply(r.view(B * self.patch, I * self.out_dim), self.channel_route.weight, self.channel_route.bias)
        return logits, r.view(B, self.patch, I)

    def cross_forward(self, image, text=None, is_train=True, experts=None):
        for expert in self.model:
            if torch.is_grad_enabled() and any(p.requires_grad for p in expert.parameters()):
                raise NotImplementedError("cross_forward trains the router over FROZEN experts (il_modules/mrn.py:154-157,"
                                          "285-286); unfreeze is not supported on the HIP path")
        logits, r = self._experts_and_gate(image, text, is_train, experts=experts)
        w = GateTailFn.apply(r, self.route.weight, self.route.bias, float(self.beta))
        return FaninFn.apply(w, *logits), w

    def cross_forward_expert(self, image, text=None, is_train=True, search=None):
        """-> (the routed expert's logits, the hard routing index); with search (a decoding.AttnSearch) also the routed expert's
        (path [B,S], prob [B,S], word [B] or None) as a third value"""
        with torch.no_grad():
            parts = []
            logits, r = self._experts_and_gate(image, text, is_train, search=search, parts=parts)
            _, index = ops.gate_tail_fwd(r.contiguous(), self.route.weight.view(-1), self.route.bias, float(self.beta), hard=True)
            if search is not None and search.kind == "shortlist":
                routed = ops.select_expert(logits, index)
                return routed, index, self._shortlist_best(parts, routed, index, text, search)
            best = None if search is None else self._routed(parts, index)
            routed = ops.select_expert(logits, index)
            return (routed, index) if search is None else (routed, index, best)

    @staticmethod
    def _routed(parts, index):
        """parts: (first expert, tensors [G,B,...] or None in their place) per heads group or expert, in any order -> per tensor the rows
        of the expert `index` picks for each sample, [B,...]"""
        main = torch.cuda.current_stream() if index.is_cuda else None
        parts = sorted(parts, key=lambda p: p[0])
        for part in parts:
            for t in part[1:]:
                if main is not None and t is not None:      # (decoded on a side stream that this stream has waited for)
                    t.record_stream(main)
        pick = index.view(-1).long()
        rows = torch.arange(pick.numel(), device=pick.device)
        return tuple(None if col[0] is None else torch.cat(col)[pick, rows] for col in list(zip(*parts))[1:])

    def _shortlist_best(self, records, routed, index, text, search):
        """the routed expert's (path, prob, word [B]) of the lexicon protocol: the hypotheses are the arg-max of the routed logits [B,S,C]
        before the first [EOS], their shortlist is the batch's one candidate table, and every heads group (run_search: one grouped
        launch) or expert (Attention.search) of `records` scores it on the features its greedy decode ran on"""
        L = self.opt.batch_max_length
        main = torch.cuda.current_stream() if routed.is_cuda else None
        cand, _ = ops.lexicon_shortlist(*ops.hypothesis_of_path(ops.argmax_lastdim(routed), ATTN_EOS), search.words, search.K, search.max_dist)
        scoring = search.scoring(cand, L + 1)
        parts = []
        for first, hg, kept in sorted(records, key=lambda p: p[0]):
            if hg is None:                            # one expert; kept: its features, a strided slice of the router's feature tensor
                best = self.model[first].Prediction.search(scoring, kept.contiguous(), text, L)
                parts.append((first,) + tuple(t.unsqueeze(0) for t in best))
            else:
                if main is not None:                  # (allocated on a side stream that this stream has waited for)
                    kept[0].record_stream(main)
                    kept[1].record_stream(main)
                parts.append((first,) + hg.run_search(scoring, *kept))
        return self._routed(parts, index)

    def build_fc(self, hidden_size, nb_classes):
        self.update_fc(hidden_size, nb_classes)

    def update_fc(self, hidden_size, nb_classes):
        if not tasks_supported(len(self.model) + 1):
            raise NotImplementedError(unsupported_task_count_message("MRNNet", len(self.model) + 1))
        check_hidden(self.opt.SequenceModeling, self.opt.Prediction, self.opt.hidden_size)
        dev = next(self.parameters()).device if len(self.model) else None
        self.model.append(Model(self.opt))
        self.model[-1].new_fc(hidden_size, nb_classes)
        if self.out_dim is None:
            self.out_dim = self.model[-1].SequenceModeling_output
        # the whole router is re-created for the new expert count (reference :437-452)
        self.route = nn.Linear(self.patch, 1)
        self.channel_route = nn.Linear(self.feature_dim, len(self.model))
        block = DM_Router(self.out_dim, self.out_dim * 2, self.patch, len(self.model))
        print("mlp {} has {} layers".format(block, self.layer_num))
        self.dm_router = nn.Sequential(*[block for _ in range(self.layer_num)])
        if dev is not None:
            self.to(dev)

    def build_prediction(self, opt, num_class):
        if opt.Prediction == "CTC" or opt.Prediction == "Attn":
            self.model[-1].build_prediction(opt, num_class)
            if len(self.model) > 1:
                self.model[-1].to(next(self.model[0].parameters()).device)
        else:
            raise Exception("Prediction is neither CTC or Attn")

    def copy(self):
        pool, self._stream_pool = self._stream_pool, []      # streams / packed-weight caches are not copied
        group, self._group = self._group, None
        heads, self._heads = self._heads, None
        halves, self._halves = self._halves, None
        try:
            return copy.deepcopy(self)
        finally:
            self._stream_pool = pool
            self._group = group
            self._heads = heads
            self._halves = halves

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        return self

    def softargmax1d(self, input, beta=5):
        """softmax(beta * input) over the last axis (reference :495-496).  cross_forward has it fused into the gate-tail kernel
        together with the `route` Linear; this stand-alone form runs the same kernel with a one-tap identity route."""
        shape = input.shape
        x = input.reshape(-1, 1, shape[-1])
        one = torch.ones(1, 1, device=input.device, dtype=torch.float32)
        zero = torch.zeros(1, device=input.device, dtype=torch.float32)
        return GateTailFn.apply(x, one, zero, float(beta)).view(shape)
