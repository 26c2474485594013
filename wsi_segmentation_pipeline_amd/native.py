"""ctypes binding of libwsi_hip.so (C ABI: include/wsi_hip.h).

The product path has no CPU fallback: if the library is missing, ``load()`` raises and every caller
fails loudly.  ``build()`` compiles the library in-tree with hipcc for gfx950 (works without a GPU).
"""
import contextlib
import ctypes as C
import enum
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libwsi_hip.so')
CSRC = os.path.join(_HERE, 'csrc')

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


TRUNK_MAX_BLOCKS = 36                    # include/wsi_hip.h WSI_TRUNK_MAX_BLOCKS: residual blocks of one trunk, all stages together


def _trunk_weights(name, convs, downs, doc):
    """The ctypes mirror of a net's weight struct: one field list, `convs` convs per block and `downs` downsample slots."""
    fields = [
        ('stem_w', C.c_void_p), ('stem_b', C.c_void_p),
        ('stem_w_u8', C.c_void_p), ('stem_b_u8', C.c_void_p), ('norm', C.c_float * 6),
        ('blocks', C.c_int * 4),
        ('conv_w', C.c_void_p * (convs * TRUNK_MAX_BLOCKS)), ('conv_b', C.c_void_p * (convs * TRUNK_MAX_BLOCKS)),
        ('down_w', C.c_void_p * downs), ('down_b', C.c_void_p * downs),
        ('head_w', C.c_void_p), ('head_b', C.c_void_p), ('head_k', C.c_int),
        ('planes', C.c_int),
    ]
    return type(name, (C.Structure,), {'_fields_': fields, '__doc__': doc})


WsiTrunkWeights = _trunk_weights('WsiTrunkWeights', 2, 3, 'wsi_trunk_weights: `blocks` residual blocks per stage; layerL.B.convK at '
                                 '2 * (sum(blocks[:L-1]) + B) + (K-1); downsamples of layer2..4.')
WsiBneckWeights = _trunk_weights('WsiBneckWeights', 3, 4, 'wsi_bneck_weights: `blocks` Bottleneck blocks per stage; layerL.B.convK at '
                                 '3 * (sum(blocks[:L-1]) + B) + (K-1); downsamples of layer1..4.')


def _decoder_weights(name, convs, doc):
    """The ctypes mirror of a decoder's weight struct: one field list, `convs` conv slots."""
    fields = [
        ('conv_w', C.c_void_p * convs), ('conv_b', C.c_void_p * convs), ('cin', C.c_int * convs), ('cout', C.c_int * convs),
        ('head_w', C.c_void_p), ('head_b', C.c_void_p), ('head_cin', C.c_int), ('classes', C.c_int), ('tail_w', C.c_void_p),
    ]
    return type(name, (C.Structure,), {'_fields_': fields, '__doc__': doc})


WsiUnetDecoderWeights = _decoder_weights('WsiUnetDecoderWeights', 10, 'wsi_unet_decoder_weights: conv 2 * (L - 1) + J = decoder.layerL.block.J; '
                                         "tail_w = wsi_unet_tail_prepack's blob or NULL.")
WsiLinknetDecoderWeights = _decoder_weights('WsiLinknetDecoderWeights', 15, 'wsi_linknet_decoder_weights: conv 3 * (L - 1) + J = '
                                            "decoder.layerL.block.J; tail_w = wsi_linknet_tail_prepack's blob or NULL.")


class WsiFpnDecoderWeights(C.Structure):
    """wsi_fpn_decoder_weights: conv slots in state-dict order (conv1, p4 / p3 / p2.skip_conv, s5.block.0-2, s4.block.0-1, s3.block.0,
    s2.block.0), the GroupNorm weight / bias of the seven seg units in the same order, the head."""
    _fields_ = [
        ('conv_w', C.c_void_p * 11), ('conv_b', C.c_void_p * 11), ('cin', C.c_int * 11), ('cout', C.c_int * 11),
        ('gn_w', C.c_void_p * 7), ('gn_b', C.c_void_p * 7), ('groups', C.c_int), ('eps', C.c_float),
        ('head_w', C.c_void_p), ('head_b', C.c_void_p), ('classes', C.c_int),
    ]


class WsiPspnetDecoderWeights(C.Structure):
    """wsi_pspnet_decoder_weights: conv slot 0 = the feature-map columns of decoder.conv (1x1, BatchNorm folded), slot 1 = decoder.final_conv
    (3x3, output channels padded to one line); per pyramid stage the transposed stage conv [feat_c][feat_c / 4] with its BatchNorm scale
    folded in, its bias [feat_c / 4] and the transposed column slice of decoder.conv [feat_c / 4][512]."""
    _fields_ = [
        ('conv_w', C.c_void_p * 2), ('conv_b', C.c_void_p * 2), ('cin', C.c_int * 2), ('cout', C.c_int * 2),
        ('stage_w', C.c_void_p * 4), ('stage_b', C.c_void_p * 4), ('proj_w', C.c_void_p * 4),
        ('classes', C.c_int), ('feat_c', C.c_int),
    ]


class WsiJpegHuff(C.Structure):
    """wsi_jpeg_huff: one Huffman table in the look-up form of the entropy kernel."""
    _fields_ = [('look', C.c_uint16 * 512), ('maxcode', C.c_int32 * 18), ('valoffset', C.c_int32 * 18), ('huffval', C.c_uint8 * 256)]


class WsiJpegTables(C.Structure):
    """wsi_jpeg_tables: up to four quantisation tables (zigzag order) and the DC 0, DC 1, AC 0, AC 1 Huffman tables."""
    _fields_ = [('qt', (C.c_uint16 * 64) * 4), ('huff', WsiJpegHuff * 4), ('qt_present', C.c_uint8 * 4), ('huff_present', C.c_uint8 * 4)]


class WsiJpegTile(C.Structure):
    """wsi_jpeg_tile: the marker walk's record of one tile stream."""
    _fields_ = [('scan_off', C.c_ulonglong), ('scan_len', C.c_uint), ('status', C.c_int), ('table_set', C.c_int),
                ('width', C.c_ushort), ('height', C.c_ushort), ('restart', C.c_ushort), ('ncomp', C.c_ubyte),
                ('h', C.c_ubyte * 3), ('v', C.c_ubyte * 3), ('tq', C.c_ubyte * 3), ('td', C.c_ubyte * 3), ('ta', C.c_ubyte * 3),
                ('pad', C.c_ubyte * 6)]


class JpegStatus(enum.IntEnum):
    """include/wsi_hip.h WSI_JPEG_*: why a tile cannot go to the device (1..9, from the marker walk) or what stopped its lane (16..)."""
    OK = 0
    PROGRESSIVE = 1
    ARITHMETIC = 2
    PRECISION = 3
    COMPONENTS = 4
    SAMPLING = 5
    MULTISCAN = 6
    MALFORMED = 7
    TABLE_CAPACITY = 8
    EMPTY = 9
    BAD_CODE = 16
    COEF_OVERRUN = 17
    SHORT = 18
    EXHAUSTED = 19
    EXCESS = 20
    RANGE = 21
    GEOMETRY = 22


_vp, _i, _ll, _sz, _f, _d =C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_float, C.c_double
# name -> (restype, argtypes); must list every symbol include/wsi_hip.h declares
SIGNATURES = {
    'wsi_hip_abi_version': (_i, []),
    'wsi_pf_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'wsi_pf_pixel_index': (_ll, [_i, _i, _i, _i, _i]),
    'wsi_prepack_conv_bytes': (_sz, [_i, _i, _i, _i]),
    'wsi_prepack_conv': (_i, [_vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _vp, _vp]),
    'wsi_unet_tail_prepack_bytes': (_sz, []),
    'wsi_unet_tail_prepack': (_i, [_vp] * 10 + [_f, _vp, _vp, _i, _i, _i, _vp]),
    'wsi_unet_tail_bands': (_i, [_i, _i, _i]),
    'wsi_unet_tail_timeouts': (_i, [C.POINTER(C.c_ulonglong), _i]),
    'wsi_prepack_stem_bytes': (_sz, [_i]),
    'wsi_prepack_stem': (_i, [_vp, _vp, _vp, _vp, _vp, _f, _i, _vp, _vp]),
    'wsi_prepack_stem_u8': (_i, [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _vp, _vp]),
    'wsi_normalize_u8_lut': (_i, [_vp, _vp, _vp]),
    'wsi_stem_conv7x7_bn_relu_maxpool': (_i, [_vp, _vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp]),
    'wsi_stem_conv7x7_bn_relu_maxpool_lines96': (_i, [_vp, _vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _ll, _vp]),
    'wsi_stem_set_mode': (_i, [_i, _i]),
    'wsi_conv3x3_bn_act': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'wsi_conv3x3_bn_act_cfg': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'wsi_conv3x3s2_ds_fused': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'wsi_s2_slab_images': (_i, [_i, _i, _i, _i, _i]),
    'wsi_pf_split_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'wsi_conv3x3_bn_act_split': (_i, [_vp] * 5 + [_i] * 7 + [_vp]),
    'wsi_conv3x3_up_concat_bn_act': (_i, [_vp] * 5 + [_i] * 8 + [_vp]),
    'wsi_conv3x3s2_ds_fused_split': (_i, [_vp] * 7 + [_i] * 6 + [_vp]),
    'wsi_conv_set_mode': (_i, [_i]),
    'wsi_conv1x1_bn': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'wsi_conv1x1_bn_act': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'wsi_avgpool_fc': (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    'wsi_linear': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'wsi_pf_pack': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'wsi_pf_unpack': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'wsi_trunk_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'wsi_trunk_workspace_init': (_i, [_vp, _i, _i, _i, _i, _vp]),
    'wsi_trunk_workspace_release': (_i, [_vp]),
    'wsi_trunk_forward': (_i, [C.POINTER(WsiTrunkWeights), _vp, _vp, _ll, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    'wsi_trunk_forward_tap': (_i, [C.POINTER(WsiTrunkWeights), _vp, _vp, _ll, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    'wsi_trunk_set_chunks': (_i, [_i, _i]),
    'wsi_bneck_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'wsi_bneck_workspace_init': (_i, [_vp, _i, _i, _i, _i, _vp]),
    'wsi_bneck_forward': (_i, [C.POINTER(WsiBneckWeights), _vp, _vp, _ll, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    'wsi_bneck_forward_tap': (_i, [C.POINTER(WsiBneckWeights), _vp, _vp, _ll, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    'wsi_prof_begin': (_i, [_i]),
    'wsi_prof_end': (_i, [_vp, _vp, _vp, _i]),
    'wsi_tile_gather': (_i, [_vp, _ll, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'wsi_stitch_add': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    'wsi_stitch_add_dense': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    'wsi_softmax_threshold_argmax': (_i, [_vp, _i, _ll, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    'wsi_ring_create': (_i, [_vp, _i, _sz]),
    'wsi_ring_host_slot': (_vp, [_vp, _i]),
    'wsi_ring_wait_slot': (_i, [_vp, _i]),
    'wsi_ring_submit': (_i, [_vp, _i, _i, _i, _i, _ll, _vp, _ll]),
    'wsi_ring_fence': (_i, [_vp, _vp]),
    'wsi_ring_acquire': (_i, [_vp, _vp]),
    'wsi_ring_device': (_i, [_vp]),
    'wsi_ring_drain': (_i, [_vp]),
    'wsi_ring_destroy': (None, [_vp]),
    'wsi_resample_plan_create': (_i, [_vp, _i, _i, _i, _i]),
    'wsi_resample_plan_destroy': (None, [_vp]),
    'wsi_resample_scratch_bytes': (_sz, [_vp, _i]),
    'wsi_resample_tiles': (_i, [_vp, _vp, _ll, _i, _i, _vp, _i, _vp, _vp, _vp]),
    'wsi_find_nuclei_hsv': (_i, [_vp, _ll, _i, C.c_double, _vp, _vp]),
    'wsi_connected_components_scratch_bytes': (_sz, [_i, _i]),
    'wsi_connected_components': (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    'wsi_kmeans_points': (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    'wsi_kmeans_seed_farthest': (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    'wsi_find_nuclei_lab': (_i, [_vp, _ll, _i, _d, _vp, _vp, _vp]),
    'wsi_fill_holes_scratch_bytes': (_sz, [_i, _i]),
    'wsi_fill_holes': (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    'wsi_slic_scratch_bytes': (_sz, [_i, _i, _i]),
    'wsi_slic': (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _i, _d, _d, _i, _vp, _vp, _vp]),
    'wsi_tile_grid_candidates': (_ll, [_i, _i, _i, _i, _i, _i]),
    'wsi_tile_grid_scratch_bytes': (_sz, [_ll]),
    'wsi_tile_grid': (_i, [_i, _i, _i, _i, _i, _i, _vp, _i, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
    'wsi_exponent_span': (_i, [_vp, _ll, _vp, _vp]),
    'wsi_paint_regions': (_i, [_vp, _vp, _ll, _vp, _vp, _vp, _ll, _vp]),
    'wsi_resize_bilinear_f64': (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp]),
    'wsi_argmax_classes': (_i, [_vp, _i, _ll, _vp, _vp]),
    'wsi_morph_rect': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'wsi_bwperim': (_i, [_vp, _vp, _i, _i, _vp]),
    'wsi_tumor_bed_workspace_bytes': (_sz, [_i, _i]),
    'wsi_convex_hull_image': (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    'wsi_tumor_bed': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'wsi_hull_polygon': (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    'wsi_mask_iou_counts': (_i, [_vp, _vp, _ll, _vp, _vp]),
    'wsi_score_counts': (_i, [_vp, _vp, _vp, _ll, _vp, _vp]),
    'wsi_esp': (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    'wsi_prepack_tconv_bytes': (_sz, [_i, _i]),
    'wsi_prepack_tconv': (_i, [_vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp, _vp]),
    'wsi_linknet_tail_prepack_bytes': (_sz, []),
    'wsi_linknet_tail_prepack': (_i, [_vp] * 15 + [_f, _vp, _vp, _i, _i, _i, _i, _vp]),
    'wsi_tconv4x4s2_bn_relu': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'wsi_conv1x1_bn_relu_add': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'wsi_groupnorm_scratch_bytes': (_sz, [_i, _i, _i]),
    'wsi_groupnorm_relu_up2': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _i, _vp, _vp]),
    'wsi_fpn_merge_head_up4': (_i, [C.POINTER(C.c_void_p * 4), _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    'wsi_upsample2_nearest': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'wsi_pyramid_pool': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'wsi_pspnet_stage_project': (_i, [_vp, C.POINTER(C.c_void_p * 4), C.POINTER(C.c_void_p * 4), C.POINTER(C.c_void_p * 4), _vp, _vp, _i, _i, _vp]),
    'wsi_pyramid_expand': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'wsi_pspnet_head_up8': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'wsi_resize_nearest_f32': (_i, [_vp, _ll, _i, _i, _vp, _i, _i, _vp]),
    'wsi_tile_views_u8': (_i, [_vp, _ll, _i, _i, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    'wsi_views_f32': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    'wsi_mlp_views': (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _f, _f, _vp, _vp, _vp]),
    'wsi_stain_moments_scratch_bytes': (_sz, [_ll, _i]),
    'wsi_stain_od_moments': (_i, [_vp, _ll, _i, _i, _vp, _vp, _vp, _vp]),
    'wsi_stain_lab_moments': (_i, [_vp, _ll, _i, _i, _vp, _vp, _vp]),
    'wsi_stain_angle_hist': (_i, [_vp, _ll, _i, _i, _vp, _vp, _i, _vp, _vp]),
    'wsi_stain_conc_hist': (_i, [_vp, _ll, _i, _i, _vp, _vp, _i, _f, _vp, _vp]),
    'wsi_stain_macenko_apply': (_i, [_vp, _vp, _ll, _i, _vp, _vp, _vp, _f, _vp]),
    'wsi_stain_reinhard_apply': (_i, [_vp, _vp, _ll, _i, _vp, _vp, _vp]),
    'wsi_jpeg_tables_bytes': (_sz, []),
    'wsi_jpeg_tile_bytes': (_sz, []),
    'wsi_jpeg_parse_tables': (_i, [_vp, _sz, _vp]),
    'wsi_jpeg_walk': (_i, [_vp, _sz, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    'wsi_jpeg_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'wsi_jpeg_entropy': (_i, [_vp, _sz, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i, _vp]),
    'wsi_jpeg_reconstruct': (_i, [_vp, _sz, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _ll, _i, _i, _vp]),
    'wsi_jenc_quality_tables': (_i, [_i, _vp, _vp]),
    'wsi_jenc_std_huff': (_i, [_i, _vp, _vp, C.POINTER(_i)]),
    'wsi_jenc_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'wsi_jenc_transform': (_i, [_vp, _ll, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    'wsi_jenc_entropy_size': (_i, [_vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    'wsi_jenc_entropy_write': (_i, [_vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _i, _vp]),
    'wsi_jenc_downsample': (_i, [_vp, _ll, _i, _i, _i, _i, _vp, _ll, _vp]),
    'wsi_poly_raster': (_i, [_vp, _ll, _vp, _i, _vp, _i, _i, _ll, _i, _i, _i, _i, _vp]),
    'wsi_contour_count_workspace_bytes': (_sz, [_i, _i]),
    'wsi_contour_workspace_bytes': (_sz, [_ll]),
    'wsi_contour_count': (_i, [_vp, _i, _i, _ll, _vp, _vp, _vp, _vp]),
    'wsi_contour_build': (_i, [_vp, _i, _i, _ll, _vp, _vp, _ll, _vp, _sz, _vp]),
    'wsi_contour_ranks': (_i, [_vp, _sz, _ll, _vp]),
    'wsi_contour_order': (_i, [_vp, _sz, _ll, _i, _vp, _vp]),
    'wsi_contour_emit': (_i, [_vp, _i, _i, _ll, _vp, _sz, _ll, _i, _i, _i, _i, _i, _i, _vp, _ll, _vp, _vp, _ll, _vp]),
    'wsi_edt_workspace_bytes': (_sz, [_i, _i]),
    'wsi_edt_columns': (_i, [_vp, _i, _i, _ll, _i, _vp, _sz, _vp]),
    'wsi_edt_rows': (_i, [_vp, _sz, _i, _i, _vp, _ll, _vp]),
    'wsi_region_count_workspace_bytes': (_sz, [_i, _i]),
    'wsi_region_workspace_bytes': (_sz, [_i, _i, _ll]),
    'wsi_region_count': (_i, [_vp, _i, _i, _ll, _vp, _vp, _vp, _vp]),
    'wsi_region_runs': (_i, [_vp, _i, _i, _ll, _vp, _vp, _ll, _vp, _sz, _vp]),
    'wsi_region_link': (_i, [_vp, _sz, _i, _i, _ll, _i, _vp]),
    'wsi_region_rank': (_i, [_vp, _sz, _i, _i, _ll, _i, _vp, _vp]),
    'wsi_region_table': (_i, [_vp, _sz, _i, _i, _ll, _ll, _vp, _ll, _vp, _vp]),
    'wsi_region_paint': (_i, [_vp, _sz, _i, _i, _ll, _vp, _ll, _vp]),
    'wsi_regionhull_workspace_bytes': (_sz, [_i, _i, _ll, _ll]),
    'wsi_regionhull_rows': (_i, [_vp, _sz, _vp, _i, _i, _ll, _ll, _vp, _sz, _vp]),
    'wsi_regionhull_chains': (_i, [_vp, _sz, _i, _i, _ll, _ll, _vp, _vp]),
    'wsi_regionhull_emit': (_i, [_vp, _sz, _vp, _i, _i, _ll, _ll, _ll, _vp, _vp]),
    'wsi_regionhull_measure': (_i, [_vp, _sz, _i, _i, _ll, _ll, _vp, _ll, _vp, _vp]),
}
# the four entries of every (segmentation model, encoder block type) pair: one signature set, generated per prefix
_enc5 = C.POINTER(C.c_void_p * 5)
for _prefix, _trunk, _dec in (('wsi_unet', WsiTrunkWeights, WsiUnetDecoderWeights), ('wsi_unet_bneck', WsiBneckWeights, WsiUnetDecoderWeights),
                              ('wsi_linknet', WsiTrunkWeights, WsiLinknetDecoderWeights),
                              ('wsi_fpn', WsiTrunkWeights, WsiFpnDecoderWeights), ('wsi_fpn_bneck', WsiBneckWeights, WsiFpnDecoderWeights),
                              ('wsi_pspnet', WsiTrunkWeights, WsiPspnetDecoderWeights), ('wsi_pspnet_bneck', WsiBneckWeights, WsiPspnetDecoderWeights)):
    _wt, _dw = C.POINTER(_trunk), C.POINTER(_dec)
    SIGNATURES.update({
        _prefix + '_workspace_bytes': (_sz, [_dw, _i, _i, _i, _i]),
        _prefix + '_workspace_init': (_i, [_dw, _vp, _i, _i, _i, _i, _vp]),
        _prefix + '_forward': (_i, [_wt, _dw, _vp, _vp, _ll, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _enc5, _vp]),
        _prefix + '_decoder': (_i, [_dw, _enc5, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    })


def build(verbose=False):
    """Compile csrc/*.hip into lib/libwsi_hip.so with hipcc --offload-arch=gfx950."""
    res = subprocess.run(['make', '-C', CSRC, '-j8'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode:
        print(res.stdout)
    if res.returncode:
        raise RuntimeError('hipcc build of libwsi_hip.so failed')
    global _lib
    _lib = None
    return LIB_PATH


ABI_VERSION = 9                          # include/wsi_hip.h WSI_HIP_ABI_VERSION (tests/test_capi_symbols.py compares the two)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            '%s not found: the WSI inference path has no CPU fallback - build it first '
            '(python -c "import __graft_entry__ as g; g.build()" or make -C %s)' % (LIB_PATH, CSRC))
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lost a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.wsi_hip_abi_version() != ABI_VERSION:
        raise RuntimeError('libwsi_hip.so ABI version mismatch')
    if lib.wsi_jpeg_tables_bytes() != C.sizeof(WsiJpegTables) or lib.wsi_jpeg_tile_bytes() != C.sizeof(WsiJpegTile):
        raise RuntimeError('libwsi_hip.so wsi_jpeg_tables / wsi_jpeg_tile layout mismatch')
    _lib = lib
    return lib


class ConvMode(enum.IntFlag):
    """wsi_conv_set_mode bits: include/wsi_hip.h WSI_CONV_MODE_* (tests/test_capi_symbols.py compares the two)."""
    S2_GATHER = 0
    S2_SLAB = 1
    S2_SLAB_128 = 3
    XCD_ORDER = 8
    WIDE_FROM_256 = 16
    WIDE_NEVER = 32
    S2_ABLATE = 64
    NO_S2_SPLIT = 128
    XCD_RANGES_OFF = 256
    XCD_RANGES_L1 = 512
    L1_SLAB3 = 1024
    NO_DS_FOLD = 2048
    NO_SLAB_PAIR = 4096
    EPILOGUE_PIECES = 8192
    L1_LINES128 = 16384
    S2_NT2 = 32768
    UNET_CONCAT_PASS = 65536
    WIDE_NO_D8 = 131072
    PW_GATHER = 262144
    L1_PERSISTENT = 1048576
    UNET_NO_TAIL = 2097152
    UNET_TAIL_FORM1 = 4194304
    UNET_X0_UNFUSED = 8388608
    LINKNET_NO_TAIL = 16777216


class StemMode(enum.IntEnum):
    """wsi_stem_set_mode `fused` values: include/wsi_hip.h WSI_STEM_MODE_*."""
    UNFUSED = 0
    FUSED = 1
    FUSED_LUT = 2
    FUSED_ONE_STRIP = 3
    FUSED_STRIPS = 4


@contextlib.contextmanager
def conv_mode(flags=0, base=ConvMode.S2_SLAB):
    """Run the block under wsi_conv_set_mode(base + flags); the default mode (S2_SLAB alone) is back on exit."""
    lib = load()
    check(lib.wsi_conv_set_mode(int(base) | int(flags)), 'wsi_conv_set_mode')
    try:
        yield
    finally:
        lib.wsi_conv_set_mode(int(ConvMode.S2_SLAB))


@contextlib.contextmanager
def stem_mode(fused, rows=64):
    """Run the block under wsi_stem_set_mode(fused, rows); the default (FUSED, 64 rows) is back on exit."""
    lib = load()
    check(lib.wsi_stem_set_mode(int(fused), rows), 'wsi_stem_set_mode')
    try:
        yield
    finally:
        lib.wsi_stem_set_mode(int(StemMode.FUSED), 64)


def profiled(run, max_records=256, ms=False):
    """(what run() returns, the profiler's records of it): wsi_prof_begin(max_records), run(), wsi_prof_end.  One (kind, flops) per launch
    in launch order, (kind, flops, milliseconds) with `ms`; wsi_prof_end waits for the recorded events.  RuntimeError where the records
    filled the table (the run may have made more launches than were recorded)."""
    lib = load()
    check(lib.wsi_prof_begin(max_records), 'wsi_prof_begin')
    try:
        out = run()
    finally:
        t, kind, flops = (C.c_float * max_records)(), (C.c_int * max_records)(), (C.c_double * max_records)()
        n = lib.wsi_prof_end(t, kind, flops, max_records)
    if not 0 <= n < max_records:
        raise RuntimeError('wsi_prof_end returned %d of at most %d records' % (n, max_records))
    return out, [(kind[i], flops[i]) + ((t[i],) if ms else ()) for i in range(n)]


def check(rc, what):
    if rc != 0:
        raise RuntimeError('%s failed with code %d (see include/wsi_hip.h error conventions)' % (what, rc))
