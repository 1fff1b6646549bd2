"""Input geometries the HIP path runs (pure Python: importable without a GPU).

The reference ends the visual stage with permute(0,3,1,2) + AdaptiveAvgPool2d((None, 1)) (modules/model.py:59-61, 92): the final
feature map's rows are averaged into one sequence row, so any imgH trains there.  Here 32-pixel inputs (a height-1 map: the pool is
the identity) run every feature extractor; 48- and 64-pixel inputs (2- and 3-row maps) run the VGG / ResNet extractors, with or without
TPS, through the height-mean kernels (mrn_height_mean_grouped_f32).  The width stays 256: the MRN router's sequence length (63 / 65
frames) is fixed by it.
"""

SUPPORTED_HEIGHTS = (32, 48, 64)
SUPPORTED_WIDTH = 256
TALL_FEATURES = ("VGG", "ResNet")          # extractors that run at every supported height
TRANSFORMATIONS = ("None", "TPS")


def geometry_supported(feature_extraction, imgH, imgW, transformation="None"):
    """does the HIP path run this stage set at imgH x imgW (imgW = 256; imgH 32 for every extractor, 48 / 64 for VGG / ResNet)"""
    if imgW != SUPPORTED_WIDTH or transformation not in TRANSFORMATIONS:
        return False
    if imgH == 32:
        return True
    return imgH in SUPPORTED_HEIGHTS and feature_extraction in TALL_FEATURES


def unsupported_geometry_message(transformation, feature_extraction, imgH, imgW, final_height):
    """the NotImplementedError text for an input whose final feature map the HIP path does not take"""
    return ("HIP path supports imgH in {%s} at imgW = %d for the VGG / ResNet extractors (other extractors: 32 x %d only); got "
            "%s + %s at %d x %d (final feature map height %d)"
            % (", ".join(str(h) for h in SUPPORTED_HEIGHTS), SUPPORTED_WIDTH, SUPPORTED_WIDTH, transformation, feature_extraction,
               imgH, imgW, final_height))
