"""Input geometries the HIP path runs (pure Python: importable without a GPU).

The reference ends the visual stage with permute(0,3,1,2) + AdaptiveAvgPool2d((None, 1)) (modules/model.py:59-61, 92): the final
feature map's rows are averaged into one sequence row, so any imgH trains there.  Here 32-pixel inputs (a height-1 map: the pool is
the identity) run every feature extractor; 48- and 64-pixel inputs (2- and 3-row maps) run the VGG / ResNet extractors, with or without
TPS, through the height-mean kernels (mrn_height_mean_grouped_f32).  The same two extractors run the widths 128 ... 512 in steps of
64: the sequence length -- and with it the MRN router's token count -- follows the width (frames()).  SVTR and RCNN stay at 32 x 256.
One call may hold at most MAX_CALL_PIXELS = 256 * 64 * 256 input pixels (B * imgH * imgW): beyond it the early layers' activations
pass the 2 GiB that the kernels' 32-bit byte offsets address.
"""

SUPPORTED_HEIGHTS = (32, 48, 64)
SUPPORTED_WIDTH = 256                      # the default width (every extractor; the only one for SVTR / RCNN)
SUPPORTED_WIDTHS = (128, 192, 256, 320, 384, 448, 512)
TALL_FEATURES = ("VGG", "ResNet")          # extractors that run at every supported height and width
TRANSFORMATIONS = ("None", "TPS")
MAX_CALL_PIXELS = 256 * 64 * 256           # B * imgH * imgW of the largest call (B = 256 at 64 x 256)


def geometry_supported(feature_extraction, imgH, imgW, transformation="None"):
    """does the HIP path run this stage set at imgH x imgW (VGG / ResNet: imgH 32 / 48 / 64 x imgW 128 ... 512 in steps of 64; every
    other extractor: 32 x 256)"""
    if transformation not in TRANSFORMATIONS:
        return False
    if imgH == 32 and imgW == SUPPORTED_WIDTH:
        return True
    return imgH in SUPPORTED_HEIGHTS and imgW in SUPPORTED_WIDTHS and feature_extraction in TALL_FEATURES


def frames(feature_extraction, imgW):
    """sequence length T of the visual feature (the MRN router's token count) for an imgW-pixel line: the VGG stack ends with a 2x2
    conv without padding on the imgW/4-wide map, the ResNet stack with one with padding (0, 1); SVTR keeps imgW/4 tokens"""
    if feature_extraction == "VGG":
        return imgW // 4 - 1
    if feature_extraction == "SVTR":
        return imgW // 4
    return imgW // 4 + 1


def call_in_budget(B, imgH, imgW):
    """is a call of B images of imgH x imgW within the per-call pixel budget"""
    return B * imgH * imgW <= MAX_CALL_PIXELS


def unsupported_geometry_message(transformation, feature_extraction, imgH, imgW, final_height):
    """the NotImplementedError text for an input whose final feature map the HIP path does not take"""
    return ("HIP path supports imgH in {%s} at imgW = %d for the VGG / ResNet extractors, and there every imgW in {%s} (other "
            "extractors: 32 x %d only), with at most %d pixels per call; got %s + %s at %d x %d (final feature map height %d)"
            % (", ".join(str(h) for h in SUPPORTED_HEIGHTS), SUPPORTED_WIDTH, ", ".join(str(w) for w in SUPPORTED_WIDTHS),
               SUPPORTED_WIDTH, MAX_CALL_PIXELS, transformation, feature_extraction, imgH, imgW, final_height))


def over_budget_message(B, imgH, imgW):
    """the NotImplementedError text for a call over the pixel budget"""
    return ("HIP path takes at most B * imgH * imgW = %d pixels per call (256 x 64 x 256: the early layers' activations reach the "
            "2 GiB that 32-bit byte offsets address); got B = %d at %d x %d = %d pixels -- split the batch"
            % (MAX_CALL_PIXELS, B, imgH, imgW, B * imgH * imgW))


def check_call(transformation, feature_extraction, B, imgH, imgW):
    """refuse, before any launch, an input size outside the supported set or a call over the pixel budget"""
    if not geometry_supported(feature_extraction, imgH, imgW, transformation):
        raise NotImplementedError(unsupported_geometry_message(transformation, feature_extraction, imgH, imgW, max(1, imgH // 16 - 1)))
    if not call_in_budget(B, imgH, imgW):
        raise NotImplementedError(over_budget_message(B, imgH, imgW))
