"""ctypes binding of libgandtr_hip.so (C ABI: include/gandtr_hip.h).

The shared library is built in-tree by ``__graft_entry__.build()`` / ``make -C gandtr_amd/csrc``.  There is NO
fallback: if the library is missing the HIP path raises -- a CUDA/HIP device request never silently runs torch ops.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p

_LIB_PATH = os.environ.get("GANDTR_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgandtr_hip.so")
_lib = None

GDT_OK, GDT_ERR_INVALID, GDT_ERR_HIP, GDT_ERR_WORKSPACE, GDT_ERR_NOT_CONVERGED = 0, 1, 2, 3, 4


class ConvDesc(ctypes.Structure):
    """struct gdt_conv_desc (include/gandtr_hip.h); ``dilation`` is 1 (none) unless given."""
    _fields_ = [("cin", c_int), ("cout", c_int), ("kh", c_int), ("kw", c_int), ("stride", c_int), ("pad", c_int),
                ("pad_reflect", c_int), ("transposed", c_int), ("relu", c_int), ("out_f32_nchw", c_int),
                ("act", c_int), ("bn_eps", c_float), ("dilation", c_int), ("leaky", c_float), ("in_relu", c_int)]

    def __init__(self, *args, **kw):
        if len(args) < 13:
            kw.setdefault("dilation", 1)
        super().__init__(*args, **kw)


class ConvWeights(ctypes.Structure):
    """struct gdt_conv_weights (include/gandtr_hip.h): host fp32 arrays, all but ``weight`` may be NULL."""
    _fields_ = [("weight", c_void_p), ("bias", c_void_p), ("bn_gamma", c_void_p), ("bn_beta", c_void_p), ("bn_mean", c_void_p), ("bn_var", c_void_p)]


class PoolHeadDesc(ctypes.Structure):
    """struct gdt_pool_head_desc (include/gandtr_hip.h)."""
    _fields_ = [("kind", c_int), ("p", c_void_p), ("n_p", c_int), ("eps", c_float), ("aggregate", c_int), ("levels", c_int),
                ("rw", c_void_p), ("rb", c_void_p), ("fw", c_void_p), ("fb", c_void_p), ("eps_l2", c_float), ("attention", c_int), ("normalize_max", c_int)]


class MedianHeadDesc(ctypes.Structure):
    """struct gdt_median_head_desc (include/gandtr_hip.h)."""
    _fields_ = [("iterations", c_int), ("fw", c_void_p), ("fb", c_void_p), ("eps_l2", c_float), ("attention", c_int), ("normalize_max", c_int)]


class IngestItem(ctypes.Structure):
    """struct gdt_ingest_item (include/gandtr_hip.h)."""
    _fields_ = [("src", c_void_p), ("h", c_int), ("w", c_int), ("fx", c_int), ("fy", c_int), ("box", c_float * 4),
                ("out_w", c_int), ("out_h", c_int), ("dst_hwc", c_void_p), ("dst_chw", c_void_p)]


class CropItem(ctypes.Structure):
    """struct gdt_crop_item (include/gandtr_hip.h)."""
    _fields_ = [("src", c_void_p), ("h", c_int), ("w", c_int), ("x0", c_int), ("y0", c_int), ("cw", c_int), ("ch", c_int),
                ("flip_src", c_int), ("flip_dst", c_int), ("dst_chw", c_void_p)]


class JpegInfo(ctypes.Structure):
    """struct gdt_jpeg_info (include/gandtr_hip.h)."""
    _fields_ = [("width", c_int), ("height", c_int), ("ncomp", c_int), ("hs", c_int * 4), ("vs", c_int * 4), ("tq", c_int * 4),
                ("td", c_int * 4), ("ta", c_int * 4), ("restart_interval", c_int), ("mcus_x", c_int), ("mcus_y", c_int),
                ("blocks_per_mcu", c_int), ("nsegments", c_int), ("scan_offset", ctypes.c_ulonglong),
                ("scan_capacity", ctypes.c_ulonglong), ("quant", (ctypes.c_ushort * 64) * 4), ("huff_bits", (ctypes.c_ubyte * 17) * 4),
                ("huff_vals", (ctypes.c_ubyte * 256) * 4), ("progressive", c_int), ("comp_id", c_int * 4), ("adobe_transform", c_int)]


class JpegItem(ctypes.Structure):
    """struct gdt_jpeg_item (include/gandtr_hip.h)."""
    _fields_ = [("info", POINTER(JpegInfo)), ("scan", c_void_p), ("seg_off", POINTER(ctypes.c_uint)), ("dst_hwc", c_void_p)]


class PatchLayer(ctypes.Structure):
    """struct gdt_patch_layer (include/gandtr_hip.h): one feature map of gdt_patch_sample."""
    _fields_ = [("feat", c_void_p), ("ids", c_void_p), ("w1", c_void_p), ("b1", c_void_p), ("w2", c_void_p), ("b2", c_void_p), ("out", c_void_p),
                ("batch", c_int), ("channels", c_int), ("hw", c_int), ("patches", c_int)]


class PatchNceLayer(ctypes.Structure):
    """struct gdt_patchnce_layer (include/gandtr_hip.h): one layer of gdt_patchnce_loss."""
    _fields_ = [("q", c_void_p), ("k", c_void_p), ("row_loss", c_void_p), ("rows", c_int), ("d", c_int), ("groups", c_int)]


class MapLossPair(ctypes.Structure):
    """struct gdt_map_loss_pair (include/gandtr_hip.h): one pair of maps of gdt_map_loss."""
    _fields_ = [("a", c_void_p), ("b", c_void_p), ("target", c_float), ("kind", c_int), ("flags", c_int), ("n_images", c_int),
                ("count", ctypes.c_long), ("weight", c_double)]


PATCH_MAX_LAYERS = 16                  # GDT_PATCH_MAX_LAYERS
MAP_LOSS_MAX_PAIRS = 16                # GDT_MAP_LOSS_MAX_PAIRS

_FP = POINTER(c_float)
_IP = POINTER(c_int)

# name -> (restype, argtypes); every symbol declared in include/gandtr_hip.h
SIGNATURES = {
    "gdt_last_error": (c_char_p, []),
    "gdt_version": (c_char_p, []),
    "gdt_net_create": (c_int, [POINTER(c_void_p)]),
    "gdt_net_destroy": (None, [c_void_p]),
    "gdt_net_set_precision": (c_int, [c_void_p, c_int]),
    "gdt_net_input": (c_int, [c_void_p, c_int, _IP, _FP, _FP, _IP]),
    "gdt_net_conv": (c_int, [c_void_p, c_int, c_int, POINTER(ConvDesc), POINTER(ConvWeights), c_int, _IP]),
    "gdt_net_instance_norm": (c_int, [c_void_p, c_int, c_float, c_int, c_float, c_int, _IP]),
    "gdt_net_maxpool": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, _IP]),
    "gdt_net_resize": (c_int, [c_void_p, c_int, c_int, c_int, _IP]),
    "gdt_net_blur_resample": (c_int, [c_void_p, c_int, c_int, _IP]),
    "gdt_net_gem_l2n": (c_int, [c_void_p, c_int, c_float, c_float, c_float, _IP]),
    "gdt_net_pool_head": (c_int, [c_void_p, c_int, POINTER(PoolHeadDesc), _IP]),
    "gdt_net_median_head": (c_int, [c_void_p, c_int, POINTER(MedianHeadDesc), _IP]),
    "gdt_net_input_filter": (c_int, [c_void_p, c_int, c_float, c_float, c_float, c_float, c_float]),
    "gdt_net_output_nchw": (c_int, [c_void_p, c_int, c_void_p, _IP]),
    "gdt_net_hed_head": (c_int, [c_void_p, _IP, POINTER(c_void_p), _FP, _FP, c_float, c_int, _IP]),
    "gdt_net_rcf_head": (c_int, [c_void_p, _IP, _IP, POINTER(c_void_p), _FP, _FP, c_float, c_int, _IP]),
    "gdt_net_finalize": (c_int, [c_void_p]),
    "gdt_net_output_shape": (c_int, [c_void_p, c_int, c_int, c_int, c_int, _IP, _IP]),
    "gdt_net_num_outputs": (c_int, [c_void_p]),
    "gdt_net_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_net_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, POINTER(c_void_p),
                                c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_net_set_group_factor": (c_int, [c_void_p, c_float]),
    "gdt_plan_knob_name": (c_char_p, [c_int]),
    "gdt_plan_count_name": (c_char_p, [c_int]),
    "gdt_plan_count_more_name": (c_char_p, [c_int]),
    "gdt_net_flops": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_double)]),
    "gdt_net_set_profiling": (c_int, [c_void_p, c_int]),
    "gdt_net_profile_read": (c_int, [c_void_p, c_int, _IP, _IP, _IP, POINTER(c_double), POINTER(c_double)]),
    "gdt_net_profile_read_bytes": (c_int, [c_void_p, c_int, POINTER(c_int), POINTER(c_double)]),
    "gdt_net_num_ops": (c_int, [c_void_p]),
    "gdt_net_plan_summary": (c_int, [c_void_p, c_int, c_int, c_int, c_int, _IP, c_int]),
    "gdt_net_blur_summary": (c_int, [c_void_p, c_int, c_int, c_int, _IP, _IP]),
    "gdt_net_basic_summary": (c_int, [c_void_p, c_int, c_int, c_int, _IP]),
    "gdt_ms_aggregate": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "gdt_whiten": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gdt_whiten_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gdt_retrieval_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_retrieval_scores_ranks": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                           c_void_p]),
    "gdt_retrieval_select_negatives": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                               c_int, c_int, c_void_p]),
    "gdt_retrieval_ap_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_retrieval_average_precision": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, _IP, _IP, _IP, c_int,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gdt_retrieval_diverse_anchors_workspace_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_retrieval_diverse_anchors": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gdt_retrieval_topk_workspace_bytes": (c_int, [c_long, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_retrieval_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_int, c_long, c_int, c_void_p, c_size_t,
                                   c_void_p]),
    "gdt_retrieval_expand": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "gdt_codebook_nearest_workspace_bytes": (c_int, [c_long, c_long, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_codebook_nearest": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_codebook_aggregate_workspace_bytes": (c_int, [c_long, c_long, c_int, c_int, POINTER(c_size_t)]),
    "gdt_codebook_aggregate": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_int, c_int,
                                       c_int, c_int, c_int, c_float, c_void_p, c_size_t, c_void_p]),
    "gdt_kmeans_update_workspace_bytes": (c_int, [c_long, c_long, POINTER(c_size_t)]),
    "gdt_kmeans_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_retrieval_knn_affinity": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "gdt_retrieval_diffuse_workspace_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_retrieval_diffuse": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                      c_float, c_float, c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_retrieval_rank_scores_workspace_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "gdt_retrieval_rank_scores": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_tuple_loss_workspace_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "gdt_tuple_loss": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_size_t, c_void_p]),
    "gdt_patch_score": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gdt_patch_sample": (c_int, [POINTER(PatchLayer), c_int, c_int, c_int, c_void_p]),
    "gdt_patchnce_loss": (c_int, [POINTER(PatchNceLayer), c_int, c_float, c_float, c_void_p, c_void_p]),
    "gdt_map_loss_workspace_bytes": (c_int, [POINTER(MapLossPair), c_int, POINTER(c_size_t)]),
    "gdt_map_loss": (c_int, [POINTER(MapLossPair), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gdt_l2n_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "gdt_gem_l2n": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "gdt_rpool_regions": (c_int, [c_int, c_int, c_int, _IP, c_int, _IP]),
    "gdt_pool_regions": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_float, c_int, c_void_p, c_void_p]),
    "gdt_pool_regions_weighted": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "gdt_local_descriptors_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_local_descriptors": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gdt_net_local_head": (c_int, [c_void_p, c_int, c_float, c_int, _IP]),
    "gdt_pixel_attention_workspace_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_pixel_attention": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gdt_geometric_median_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_geometric_median": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gdt_pack_input_filter": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_void_p, c_void_p]),
    "gdt_mfma_only_tflops": (c_int, [c_int, POINTER(c_double), c_void_p]),
    "gdt_ingest_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_ingest_resize_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int, c_void_p, c_void_p,
                                     POINTER(c_float), POINTER(c_float), c_void_p, c_size_t, c_void_p]),
    "gdt_ingest_batch_workspace_bytes": (c_int, [POINTER(IngestItem), c_int, c_int, POINTER(c_size_t)]),
    "gdt_ingest_resize_u8_batch": (c_int, [POINTER(IngestItem), c_int, c_int, POINTER(c_float), POINTER(c_float), c_void_p, c_size_t,
                                           c_void_p]),
    "gdt_crop_resize_workspace_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_crop_resize_u8_batch": (c_int, [POINTER(CropItem), c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), c_void_p, c_size_t,
                                         c_void_p]),
    "gdt_jpeg_parse": (c_int, [c_void_p, c_size_t, POINTER(JpegInfo)]),
    "gdt_jpeg_extract_scan": (c_int, [c_void_p, c_size_t, POINTER(JpegInfo), c_void_p, POINTER(ctypes.c_uint)]),
    "gdt_jpeg_parse_batch": (c_int, [POINTER(c_void_p), POINTER(c_size_t), c_int, POINTER(JpegInfo), _IP, c_int]),
    "gdt_jpeg_extract_scan_batch": (c_int, [POINTER(c_void_p), POINTER(c_size_t), POINTER(JpegInfo), c_int, c_void_p, POINTER(c_size_t),
                                            POINTER(ctypes.c_uint), POINTER(c_size_t), c_int]),
    "gdt_jpeg_decode_workspace_bytes": (c_int, [POINTER(JpegItem), c_int, POINTER(c_size_t)]),
    "gdt_jpeg_decode_u8_batch": (c_int, [POINTER(JpegItem), c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_jpeg_progressive_coefficients": (c_int, [c_char_p, c_size_t, POINTER(JpegInfo), c_void_p]),
    "gdt_jpeg_progressive_coefficients_batch": (c_int, [POINTER(c_void_p), POINTER(c_size_t), POINTER(JpegInfo), c_int, c_void_p, POINTER(c_size_t),
                                                        POINTER(c_int), c_int]),
    "gdt_jpeg_decode_coef_workspace_bytes": (c_int, [POINTER(JpegInfo), c_int, POINTER(c_size_t)]),
    "gdt_jpeg_decode_coef_u8_batch": (c_int, [POINTER(JpegInfo), c_void_p, POINTER(c_size_t), POINTER(c_void_p), c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_whiten_learn_workspace_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_whiten_learn": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_int),
                                 c_void_p, c_size_t, c_void_p]),
    "gdt_pca_whiten_learn_workspace_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "gdt_pca_whiten_learn": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_int), c_void_p, c_size_t, c_void_p]),
    "gdt_pca_project_normalize_workspace_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "gdt_pca_project_normalize": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, POINTER(c_int), c_void_p, c_size_t, c_void_p]),
    "gdt_pca_covariance": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "gdt_l2n_rows_f64": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gdt_clahe_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_clahe_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_clahe_lab_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), POINTER(c_float),
                                  POINTER(c_float), c_double, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gdt_photometric_workspace_bytes": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "gdt_lab_lightness_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), c_void_p]),
    "gdt_rgb2lab_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), c_void_p]),
    "gdt_hist256_f32": (c_int, [c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p]),
    "gdt_match_channel_f32": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gdt_match_histogram_lab_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), POINTER(c_float),
                                            POINTER(c_float), c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gdt_gamma_channel_f32": (c_int, [c_void_p, c_void_p, c_int, c_long, c_double, c_void_p, c_void_p, c_void_p]),
    "gdt_gamma_equalize_lab_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), POINTER(c_float),
                                           POINTER(c_float), c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}


class HipLibraryMissing(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


def load():
    """Load (once) and return the ctypes handle; raises HipLibraryMissing when the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipLibraryMissing(
            "%s not found: the gandtr HIP path has no CPU fallback. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C gandtr_amd/csrc`." % _LIB_PATH)
    lib = ctypes.CDLL(_LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError here == ABI mismatch between header and library
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _names(fn):
    """the names ``fn(0)``, ``fn(1)``, .. up to the first NULL"""
    names = []
    while True:
        name = fn(len(names))
        if name is None:
            return tuple(names)
        names.append(name.decode())


def plan_knobs():
    """Names of the environment knobs the library reads every time it plans a geometry (gdt_plan_knob_name), in its order."""
    return _names(load().gdt_plan_knob_name)


def plan_count_names():
    """Names of the counters gdt_net_plan_summary fills (gdt_plan_count_name), in index order."""
    return _names(load().gdt_plan_count_name)


def plan_count_more_names():
    """Names of the counters gdt_net_plan_summary fills behind those (gdt_plan_count_more_name) when the array has room for them, in index order."""
    return _names(load().gdt_plan_count_more_name)


def check(rc):
    """Translate a gdt status into the exception type the reference raises for the same condition
    (ValueError for bad arguments / unsupported shapes, RuntimeError for device failures)."""
    if rc == GDT_OK:
        return
    msg = load().gdt_last_error().decode("utf8", "replace")
    if rc == GDT_ERR_INVALID:
        raise ValueError(msg)
    raise RuntimeError("gandtr_hip error %d: %s" % (rc, msg))
