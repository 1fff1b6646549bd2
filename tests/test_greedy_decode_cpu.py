"""Host side of the fused greedy decoder (no kernel is launched): the LDS rule, the lock-step predicate, the fallback switch, the C ABI."""
import contextlib
import ctypes
import io
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEDY = ("mrn_attn_greedy_decode_f32", "mrn_attn_greedy_decode_x3", "mrn_attn_greedy_decode_grouped_f32",
          "mrn_attn_greedy_decode_x3_grouped")


def _source():
    """the decoders' translation unit: the shared header, then csrc/attn_decode.hip"""
    return "".join(open(os.path.join(ROOT, "mrn_amd", "csrc", f)).read() for f in ("recurrent.hpp", "attn_decode.hip"))


def test_whole_context_rule_over_widths_and_task_counts():
    """ops.attn_greedy_whole_context over DERNet's D = 256 * G and the supported widths (T = 33 ... 129): G = 7 is the widest whole-context
    tile, as for the teacher-forced decoder; off that grid the 2112 extra bytes move the crossing (D = 1856, T = 129, x3)"""
    from mrn_amd import ops
    assert ops.GREEDY_LDS_EXTRA == 4 * (16 + 2 * 16 * 16) == 2112
    for T in (17, 33, 65, 129):
        for x3 in (True, False):
            for G in range(1, 17):
                D = 256 * G
                assert ops.attn_greedy_whole_context(D, T, x3) == (G <= 7)
                assert ops.attn_greedy_whole_context(D, T, x3) == ops.attn_decoder_whole_context(D, T, x3)
                bytes_ = 4 * (2 * 16 * 260 + 16 * (D + 4) + 16 * T + 256) + (1024 if x3 else 0) + 2112
                assert ops.attn_greedy_whole_context(D, T, x3) == (bytes_ <= 160 * 1024)
    assert 4 * (2 * 16 * 260 + 16 * (1792 + 4) + 16 * 129 + 256) + 1024 + 2112 == 160640
    assert ops.attn_decoder_whole_context(1856, 129, True) and not ops.attn_greedy_whole_context(1856, 129, True)
    assert ops.attn_greedy_whole_context(1856, 129, False)          # (no 1 KiB of fp16-plane slack in the exact form)
    # the chunked form itself always fits: 1024 context columns
    assert 4 * (2 * 16 * 260 + 16 * (1024 + 4) + 16 * 129 + 256) + 1024 + 2112 <= 160 * 1024


def test_rule_matches_the_launch_helper():
    """the terms of greedy_launch's budget in csrc/attn_decode.hip (the tile of attn_tile_lds, the three decoder kernels' one definition, plus
    GREEDY_LDS_EXTRA) are the ones ops.attn_greedy_whole_context restates"""
    src = _source()
    tile = re.sub(r"\s+", " ", src[src.index("static size_t attn_tile_lds("):src.index("static dim3 attn_grid(")])
    assert "(bool x3, int dc, int T, size_t extra)" in tile
    assert "sizeof(float) * (2 * BT * HLD + BT * (dc + 4) + BT * T + HID) + (x3 ? 1024 : 0) + extra" in tile
    body = src[src.index("static int greedy_launch("):src.index("static void greedy_fill(")]
    flat = re.sub(r"\s+", " ", body)
    assert "attn_tile_lds(x3, wide ? CTX_CHUNK : D, T, GREEDY_LDS_EXTRA)" in flat and "lds <= 160 * 1024" in flat
    assert "attn_tile_lds(x3, D, T, GREEDY_LDS_EXTRA) > 160 * 1024" in flat
    assert 'getenv("MRN_ATTN_CTX_CHUNK")' in flat and 'getenv("MRN_GREEDY_VB")' in flat
    assert "static const" not in body                                # both switches are read per launch
    consts = dict(re.findall(r"(?m)^constexpr int (\w+) = ([^;]+);", src))
    assert consts["BT"].strip() == "16" and consts["NW"].strip() == "16" and consts["HID"].strip() == "256"
    assert consts["HLD"].strip() == "HID + 4" and consts["CTX_CHUNK"].strip() == "1024" and consts["MAX_GROUPS"].strip() == "8"
    assert re.sub(r"\s+", " ", consts["GREEDY_LDS_EXTRA"]).strip() == "4 * (BT + 2 * NW * BT)"


def test_decoder_kernel_is_left_alone():
    """the new kernel stands next to attn_decoder_kernel, which keeps its two template parameters"""
    src = _source()
    assert src.count("template <bool X3, bool WIDE>\n__global__ __launch_bounds__(NTH) void attn_decoder_kernel(const AttnDecGroup grp)") == 1
    assert src.count("template <bool X3, bool WIDE>\n__global__ __launch_bounds__(NTH) void attn_greedy_kernel(const GreedyGroup grp)") == 1
    assert src.index("void attn_decoder_kernel(") < src.index("void attn_greedy_kernel(") < src.index("void embed_gather_kernel(")


def _opt(trans, feat, seq, pred):
    return types.SimpleNamespace(Transformation=trans, FeatureExtraction=feat, SequenceModeling=seq, Prediction=pred, num_fiducial=20,
                                 imgH=32, imgW=256, input_channel=4, output_channel=512, hidden_size=256, batch_max_length=25)


def test_greedy_lockstep_predicate(monkeypatch):
    from mrn_amd.modules import expert_group
    from mrn_amd.modules.model import Model, MRNNet
    HG = expert_group.HeadsGroup
    with contextlib.redirect_stdout(io.StringIO()):
        trba = [Model(_opt("TPS", "ResNet", "BiLSTM", "Attn")) for _ in range(3)]
        vgg_attn = Model(_opt("None", "VGG", "BiLSTM", "Attn"))
        crnn = [Model(_opt("None", "VGG", "BiLSTM", "CTC")) for _ in range(2)]
        svtr = [Model(_opt("None", "SVTR", "None", "CTC")) for _ in range(2)]
        net = MRNNet(_opt("TPS", "ResNet", "BiLSTM", "Attn"))
        for c in (20, 30, 40):
            net.update_fc(256, c)
            net.build_prediction(net.opt, c)
    assert HG.greedy_supported(trba)
    assert not HG.supported(trba, False)                                  # run() still has no evaluation form for the attention head
    assert not HG.greedy_supported(trba[:1])                              # a single expert: nothing to group
    assert not HG.greedy_supported([trba[0], vgg_attn])                   # mixed stages
    assert not HG.greedy_supported(crnn) and HG.supported(crnn, False)    # CTC heads keep supported() / run()
    assert not HG.greedy_supported(svtr) and HG.supported(svtr, False)
    # MRNNet: the evaluation forward of attention experts takes the lock-step group unless the step loop is asked for
    monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
    assert net._greedy_heads(False) and not net._greedy_heads(True)
    group = net._backbone_group()
    assert group is not None and net._heads_group(group, False) is not None and net._heads_group(group, True) is not None
    monkeypatch.setenv("MRN_GREEDY_DECODE", "stepwise")
    assert not net._greedy_heads(False)
    assert net._heads_group(group, False) is None and net._heads_group(group, True) is not None


def test_fallback_switch_parsing(monkeypatch):
    from mrn_amd import ops
    monkeypatch.delenv("MRN_GREEDY_DECODE", raising=False)
    assert ops.greedy_decode_mode() == "fused"
    for value, mode in (("", "fused"), ("fused", "fused"), ("stepwise", "stepwise")):
        monkeypatch.setenv("MRN_GREEDY_DECODE", value)                    # read per call
        assert ops.greedy_decode_mode() == mode
    for bad in ("0", "step", "Fused"):
        monkeypatch.setenv("MRN_GREEDY_DECODE", bad)
        with pytest.raises(ValueError, match="MRN_GREEDY_DECODE"):
            ops.greedy_decode_mode()


def test_generator_stream_layout():
    """ops.pack_generator (exact form): rows zero-padded to 16, tile n's 16 KiB contiguous, element order of pack_fragment_major"""
    from mrn_amd import ops
    C = 37
    w = torch.arange(C * 256, dtype=torch.float32).view(C, 256)
    p, inv = ops.pack_generator(w, False)
    assert inv is None and tuple(p.shape) == (3, 1, 16, 4, 16, 4)        # tile, gate group, k-step, lane group, class in tile, r
    wp = torch.zeros(48, 256)
    wp[:C] = w
    for n, q, gg, col, r in ((0, 0, 0, 0, 0), (1, 3, 2, 5, 1), (2, 15, 3, 4, 3), (2, 7, 1, 5, 2)):
        assert p[n, 0, q, gg, col, r] == wp[16 * n + col, 16 * q + 4 * gg + r]
    assert torch.count_nonzero(p[2, 0, :, :, 5:, :]) == 0                 # classes 37 ... 47: padding


def test_new_entry_points_are_declared_exported_and_cited():
    from mrn_amd import _lib
    from mrn_amd.build import build_library
    build_library(verbose=False)
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER_PATH).read()
    for name in GREEDY:
        assert name in protos and hasattr(dll, name)
        ret, argtypes, argnames = protos[name]
        assert ret == "int" and argnames[-1] == "stream" and argnames[-2] == "hidden"
        for a in ("etab", "start_token", "w_gen", "b_gen", "num_class", "logits", "logits_stride_b", "logits_stride_s", "tokens_out"):
            assert a in argnames, (name, a)
        assert "eproj" not in argnames
        assert ("w_inv" in argnames) == ("x3" in name)
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "modules/prediction.py:70-86" in comment, name
    grouped = protos["mrn_attn_greedy_decode_x3_grouped"]
    assert grouped[1][grouped[2].index("num_class")] == "const int*" and grouped[1][grouped[2].index("logits")] == "const void* const*"
    assert "the C ABI (156 entry points" in open(os.path.join(ROOT, "README.md")).read() and len(protos) == 156
