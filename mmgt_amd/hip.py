"""ctypes binding of libmmgt_hip.so (include/mmgt_hip.h): the ONLY compute entry points of the product.

There is no fallback: if the library is missing or a call fails, a RuntimeError is raised.  torch is used for device
memory (the caching allocator) and the current HIP stream only.
"""
import ctypes
import os
from ctypes import c_float, c_int, c_long, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMGT_LIB") or os.path.join(_HERE, "libmmgt_hip.so")    # MMGT_LIB: a diagnostic build (make trace), tools only

F32, BF16 = 0, 1
ACT_NONE, ACT_GEGLU, ACT_SILU, ACT_RELU, ACT_QUICK_GELU, ACT_GELU, ACT_MISH = 0, 1, 2, 3, 4, 5, 6

_lib = None
DMA_LIMIT = (1 << 31) - 1        # the kernels address every operand through 32-bit LDS-DMA offsets: 2 GiB per tensor

_SIGS = {
    "mmgt_abi_version": (c_int, []),
    "mmgt_last_error": (ctypes.c_char_p, []),
    "mmgt_tune": (c_int, [ctypes.c_char_p, c_int]),
    "mmgt_tune_get": (c_int, [ctypes.c_char_p, ctypes.POINTER(c_int)]),
    "mmgt_box_calib": (c_int, [c_float, ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_void_p]),
    "mmgt_gemm16_set_trace": (None, [c_void_p]),
    "mmgt_ffn_set_trace": (None, [c_void_p]),
    "mmgt_rconv_set_trace": (None, [c_void_p]),
    "mmgt_gemm": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_float, c_void_p, c_long,
                          c_void_p, c_long, c_int, c_int, c_int, c_int, c_int, c_long, c_long, c_long, c_long, c_int,
                          c_void_p]),
    "mmgt_gemm_post": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_long, c_void_p,
                               c_long, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_conv3x3_nhwc": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                  c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_groupnorm_chunks": (c_int, [c_int]),
    "mmgt_groupnorm_nhwc": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                    c_int, c_int, c_float, c_int, c_int, c_void_p]),
    "mmgt_layernorm": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_void_p, c_long,
                               c_int, c_int, c_int, c_void_p]),
    "mmgt_attention": (c_int, [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_long, c_long, c_void_p, c_long,
                               c_long, c_long, c_void_p, c_long, c_long, c_long, c_int, c_void_p, c_void_p, c_long,
                               c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                               c_int, c_int, c_void_p]),
    "mmgt_attention_scaled": (c_int, [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_long, c_long,
                                      c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                      c_int, c_void_p]),
    "mmgt_attention_twin": (c_int, [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_long, c_long,
                                    c_void_p, c_void_p, c_long, c_long, c_long, c_int, c_void_p, c_void_p, c_long, c_long, c_long, c_long,
                                    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "mmgt_softmax_rows": (c_int, [c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_float, c_int, c_void_p]),
    "mmgt_gemm_bf16_f32": (c_int, [c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_int, c_void_p]),
    "mmgt_qk_split3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]),
    "mmgt_softmax_rows_f32_bf16": (c_int, [c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_float, c_void_p]),
    "mmgt_ncfhw_to_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "mmgt_nhwc_to_ncfhw": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int,
                                   c_int, c_void_p]),
    "mmgt_conv1x1_cat_nhwc": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "mmgt_conv_taps_gather": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_timestep_features": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_ff_fused_image_bytes": (c_int, [c_int, c_int]),
    "mmgt_ff_fused": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_long,
                              c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_rowgemm320_image_bytes": (c_long, [c_int]),
    "mmgt_rowgemm_set_trace": (None, [c_void_p]),
    "mmgt_ff_fused_po": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                                 c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_groupnorm_affine": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int,
                                      c_void_p]),
    "mmgt_rowgemm320": (c_int, [c_void_p, c_long, c_int, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                c_long, c_void_p, c_long, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_gn_silu_conv3x3_image_bytes": (c_long, [c_int, c_int]),
    "mmgt_gn_silu_conv3x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_gn_silu_conv3x3_unet_image_bytes": (c_long, [c_int, c_int]),
    "mmgt_gn_silu_conv3x3_unet": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                          c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_gn_silu_conv3x3_unet_stats_rows": (c_int, [c_int, c_int, c_int, c_int]),
    "mmgt_gn_silu_conv3x3_unet_stats": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                                c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_gn_stats_finalize_unet": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "mmgt_groupnorm_affine2": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_float, c_int, c_void_p]),
    "mmgt_gn_stats_finalize": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "mmgt_temporal_leg320_image_bytes": (c_long, []),
    "mmgt_temporal_leg320": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_int,
                                     c_void_p]),
    "mmgt_channel_norm_gelu": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p]),
    "mmgt_lerp_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_relpos_attention": (c_int, [c_void_p, c_long, c_long, c_void_p, c_long, c_long, c_void_p, c_long, c_long, c_void_p, c_long, c_long,
                                      c_void_p, c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                      c_int, c_void_p]),
    "mmgt_silu": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p]),
    "mmgt_cfg_ddim_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_float, c_float,
                                   c_float, c_float, c_float, c_void_p]),
    "mmgt_sampler_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_float,
                                  c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_void_p]),
    "mmgt_cfg_moments": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p]),
    "mmgt_known_latents": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_float, c_float, c_void_p]),
    "mmgt_mask_to_latent": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_feather_alpha": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_composite_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p]),
    "mmgt_accumulate_window": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    "mmgt_accumulate_windows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_int, c_void_p]),
    "mmgt_rotary": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p]),
    "mmgt_film_residual": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p]),
    "mmgt_mean_tokens": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_activation": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p]),
    "mmgt_smga_ddim_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_float, c_float, c_float, c_float,
                                    c_float, c_float, c_int, c_int, c_void_p]),
    "mmgt_blur_mask_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_resample_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "mmgt_window_stack": (c_int, [c_void_p, c_void_p, c_int, c_long, c_int, c_void_p]),
    "mmgt_frames_to_u8": (c_int, [c_void_p, c_void_p, c_long, c_int, c_float, c_float, c_int, c_void_p]),
    "mmgt_jpeg_dct_quant": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_jpeg_entropy": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_long, c_void_p]),
    "mmgt_jpeg_segment_stride": (c_int, [c_int, c_int, ctypes.POINTER(c_long)]),
    "mmgt_jpeg_scan": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "mmgt_jpeg_compact": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_int, c_void_p]),
    "mmgt_jpeg_qtables": (c_int, [c_int, c_void_p]),
    "mmgt_jpegdec_sizes": (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(c_int)]),
    "mmgt_jpegdec_entropy": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                     c_int, c_int, c_int, c_void_p]),
    "mmgt_jpegdec_idct": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_jpegdec_color": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_jpegprog_entropy": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_resize_u8_workspace": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_longlong)]),
    "mmgt_resize_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                               c_void_p, c_void_p, c_int, c_void_p]),
    "mmgt_gif_histogram": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_gif_index": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_gif_dither": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_int, c_int, c_void_p]),
    "mmgt_gif_dither_band": (c_int, []),
    "mmgt_gif_dither_scratch": (c_int, [c_int, c_int, c_int, ctypes.POINTER(ctypes.c_longlong)]),
    "mmgt_gif_delta": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_gif_lzw": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_long, c_void_p]),
    "mmgt_gif_strip_stride": (c_int, [c_int, c_int, ctypes.POINTER(c_long)]),
    "mmgt_gif_pack": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_long, c_long, c_void_p]),
    "mmgt_png_filter": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_png_histogram": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_longlong, ctypes.c_longlong, c_void_p]),
    "mmgt_png_deflate": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, ctypes.c_longlong,
                                 ctypes.c_longlong, c_void_p]),
    "mmgt_png_pack": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_int, c_void_p]),
    "mmgt_webp_predict": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_webp_histogram": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_longlong, ctypes.c_longlong, c_void_p]),
    "mmgt_webp_code": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int,
                               ctypes.c_longlong, ctypes.c_longlong, c_void_p]),
    "mmgt_vp8_quantiser": (c_int, [c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "mmgt_vp8_slot_bytes": (c_int, [c_int, c_int, c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]),
    "mmgt_vp8_convert": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_vp8_analyse": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_int, c_void_p]),
    "mmgt_vp8_code": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_int, c_int, c_int, c_int,
                              c_int, c_void_p]),
    "mmgt_vp8_pack": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_png_inflate": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_longlong, c_void_p]),
    "mmgt_png_unfilter": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_png_expand": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmgt_gif_unlzw": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p]),
    "mmgt_gif_compose": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_webp_decode": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p]),
    "mmgt_webp_untransform": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p]),
    "mmgt_webp_compose": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_vp8dec_parse": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p]),
    "mmgt_vp8dec_reconstruct": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p]),
    "mmgt_vp8dec_filter": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p]),
    "mmgt_vp8dec_output": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, ctypes.c_longlong, c_void_p, c_int, ctypes.c_longlong, c_void_p]),
    "mmgt_dwpose_draw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mmgt_audio_decode_mono": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_int, c_int, c_void_p]),
    "mmgt_audio_resample": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_int, c_int, c_int, c_void_p, ctypes.c_longlong, c_void_p]),
}

EXPORTS = tuple(_SIGS)


def lib():
    """Load libmmgt_hip.so once; raise loudly if it has not been built (python __graft_entry__.py / make -C mmgt_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C mmgt_amd/csrc` (hipcc, gfx950). "
                               "mmgt_amd has no non-HIP compute path.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
        for kv in filter(None, os.environ.get("MMGT_TUNE", "").split(",")):     # A/B switches for the tools: MMGT_TUNE="splitk=0,attn64=0"
            k, v = kv.split("=")
            if L.mmgt_tune(k.strip().encode(), int(v)) != 0:
                raise RuntimeError(f"MMGT_TUNE: {L.mmgt_last_error().decode()}")
    return _lib


_calls = {}


def _check(rc, what):
    _calls[what] = _calls.get(what, 0) + 1
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {lib().mmgt_last_error().decode()}")


def call_count(what):
    """How often the entry point `what` (an include/mmgt_hip.h name) has been called through this binding: lets a test assert WHICH kernel a
    dispatcher took."""
    return _calls.get(what, 0)


def tune(key, value):
    _check(lib().mmgt_tune(key.encode(), int(value)), "mmgt_tune")


def tune_get(key):
    """A host-side switch of the library's table (include/mmgt_hip.h: mmgt_tune_get)."""
    v = c_int(0)
    _check(lib().mmgt_tune_get(key.encode(), ctypes.byref(v)), "mmgt_tune_get")
    return v.value


def box_calib(warm_seconds=2.0):
    """(in-kernel MHz, TFLOP/s) of a bare 16x16x32 bf16 MFMA loop on random operands after `warm_seconds` of back-to-back launches: a
    measure of the BOX, quoted beside a step time so that lines from different boxes can be compared (include/mmgt_hip.h: mmgt_box_calib)."""
    mhz, tf = c_float(0), c_float(0)
    _check(lib().mmgt_box_calib(float(warm_seconds), ctypes.byref(mhz), ctypes.byref(tf), _stream()), "mmgt_box_calib")
    return mhz.value, tf.value


def dtype_code(dt):
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float32:
        return F32
    raise RuntimeError(f"mmgt_amd supports float32 and bfloat16 storage, got {dt}")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("mmgt_amd.hip: tensors must live on the GPU (no CPU fallback exists)")


def _f32(t, name):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
        raise RuntimeError(f"{name} must be contiguous float32")
    return t


# ------------------------------------------------------------------------------------------------------------ GEMM

def gemm(a, w, bias=None, *, out=None, residual=None, bias2=None, bias2_rows=0, row_scale=None, alpha=1.0,
         act=ACT_NONE):
    """out[M, Nout] = epilogue(a[M, K] @ w[N, K]^T).  a may be a strided 2-D view (row stride, unit column stride)."""
    _dev(a, w, bias, out, residual, bias2, row_scale)
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.is_contiguous() and a.dtype == w.dtype
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K, (a.shape, w.shape)
    n_out = N // 2 if act == ACT_GEGLU else N
    if out is None:
        out = torch.empty((M, n_out), device=a.device, dtype=a.dtype)
    assert out.shape == (M, n_out) and out.stride(1) == 1 and out.dtype == a.dtype
    if residual is not None:
        assert residual.shape == (M, n_out) and residual.stride(1) == 1 and residual.dtype == a.dtype
    lim = DMA_LIMIT                    # an operand of 2 GiB or more is worked in runs of rows
    if M * a.stride(0) * a.element_size() > lim and M > 1:
        step = max(1, lim // (a.stride(0) * a.element_size()))
        # bias2 row groups: a run must start on a group boundary -- unless ONE row serves every output row (bias2_rows >= M: the
        # time embedding / the twin CLIP vector), which every run then takes as it is
        one_row = bias2 is not None and bias2_rows >= M
        if bias2 is not None and not one_row:
            step = step // bias2_rows * bias2_rows
            if step == 0:
                raise RuntimeError("gemm: a bias2 row group exceeds the 2 GiB range of the 32-bit LDS-DMA offsets")
        assert 0 < step < M
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            if bias2 is None:
                b2, b2r = None, 0
            elif one_row:
                b2, b2r = bias2[:1], max(m1 - m0, bias2_rows)
            else:
                b2, b2r = bias2[m0 // bias2_rows:(m1 + bias2_rows - 1) // bias2_rows], bias2_rows
            gemm(a[m0:m1], w, bias, out=out[m0:m1], residual=None if residual is None else residual[m0:m1], bias2=b2, bias2_rows=b2r,
                 row_scale=None if row_scale is None else row_scale[m0:m1], alpha=alpha, act=act)
        return out
    _check(lib().mmgt_gemm(_ptr(a), a.stride(0), _ptr(w), _ptr(_f32(bias, "bias")), _ptr(_f32(bias2, "bias2")),
                           bias2_rows, _ptr(_f32(row_scale, "row_scale")), alpha, _ptr(residual),
                           residual.stride(0) if residual is not None else 0, _ptr(out), out.stride(0), M, N, K, act, 1,
                           0, 0, 0, 0, dtype_code(a.dtype), _stream()), "mmgt_gemm")
    return out


def gemm_post(a, w, bias, row_scale, alpha, bias_post, residual, out=None):
    """out = (a @ w^T + bias) * row_scale[:, None] * alpha + bias_post + residual   (see mmgt_gemm_post)."""
    _dev(a, w, bias, row_scale, bias_post, residual, out)
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.is_contiguous() and a.dtype == w.dtype
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=a.dtype)
    assert out.shape == (M, N) and residual.shape == (M, N) and residual.stride(1) == 1 and out.stride(1) == 1
    _check(lib().mmgt_gemm_post(_ptr(a), a.stride(0), _ptr(w), _ptr(_f32(bias, "bias")), _ptr(_f32(row_scale, "row_scale")),
                                alpha, _ptr(_f32(bias_post, "bias_post")), _ptr(residual), residual.stride(0), _ptr(out),
                                out.stride(0), M, N, K, dtype_code(a.dtype), _stream()), "mmgt_gemm_post")
    return out


def gemm_batched_wx(w, x, bias_unused=None, *, out):
    """out[b] (R, ldo>=Ntok) = w[R, K] @ x[b][Ntok, K]^T for every batch b: the V^T projection (keys contiguous)."""
    _dev(w, x, out)
    B, ntok, K = x.shape
    R = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and out.dim() == 3 and out.shape[0] == B and out.shape[1] == R
    assert out.stride(2) == 1
    _check(lib().mmgt_gemm(_ptr(w), K, _ptr(x), None, None, 0, None, 1.0, None, 0, _ptr(out), out.stride(1), R, ntok, K,
                           ACT_NONE, B, 0, x.stride(0), 0, out.stride(0), dtype_code(x.dtype), _stream()),
           "mmgt_gemm(batched)")
    return out


def gemm_batched(a, w, *, out):
    """out[b] (M, N) = a[b] (M, K) @ w[b] (N, K)^T for dense 3-D operands (one problem per grid.z)."""
    _dev(a, w, out)
    B, M, K = a.shape
    N = w.shape[1]
    assert a.is_contiguous() and w.is_contiguous() and out.is_contiguous() and w.shape == (B, N, K) and out.shape == (B, M, N)
    _check(lib().mmgt_gemm(_ptr(a), K, _ptr(w), None, None, 0, None, 1.0, None, 0, _ptr(out), N, M, N, K, ACT_NONE, B,
                           M * K, N * K, 0, M * N, dtype_code(a.dtype), _stream()), "mmgt_gemm(batched)")
    return out


def conv3x3(x, wp, bias=None, *, stride=1, upsample=False, bias2=None, bias2_rows=0, residual=None, act=ACT_NONE,
            x1=None, out=None, pad_high_only=False):
    """x (NB, H, W, C0) channels-last [+ x1 (NB, H, W, C1)], wp [Cout][3][3][C0+C1] -> (NB, OH, OW, Cout).
    pad_high_only (stride 2 only): zero padding after the last row / column only (the VAE encoder's downsampler).
    upsample = True: the conv sees the nearest-2x upsampled input; upsample = 2: the same result from the four-phase image
    packing.pack_conv3x3_up2(weight) ([4][Cout][2][2][C0]: four 2 x 2 convs on the stored image, 16 / 36 of the multiply-adds; bf16, bias only)."""
    _dev(x, wp, bias, bias2, residual, x1)
    assert x.dim() == 4 and x.is_contiguous() and wp.is_contiguous() and wp.dtype == x.dtype
    NB, IH, IW, C0 = x.shape
    C1 = 0 if x1 is None else x1.shape[3]
    if upsample is not True and upsample == 2:
        assert wp.dim() == 5 and wp.shape[0] == 4 and wp.shape[2:] == (2, 2, C0) and x1 is None and residual is None and bias2 is None
        assert x.dtype == torch.bfloat16 and act == ACT_NONE and stride == 1 and not pad_high_only
        cout = wp.shape[1]
        assert cout % 256 == 0 or cout % 320 == 0
    else:
        upsample = bool(upsample)
        cout = wp.shape[0]
        assert wp.numel() == cout * 9 * (C0 + C1)
    vh, vw = (IH * 2, IW * 2) if upsample else (IH, IW)
    if pad_high_only:
        assert stride == 2 and not upsample
        oh, ow = (vh - 2) // 2 + 1, (vw - 2) // 2 + 1
    else:
        oh, ow = (vh - 1) // stride + 1, (vw - 1) // stride + 1
    if out is None:
        out = torch.empty((NB, oh, ow, cout), device=x.device, dtype=x.dtype)
    assert out.shape == (NB, oh, ow, cout) and out.is_contiguous()
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous()
    # The kernels address every operand through 32-bit LDS-DMA offsets (2 GiB per tensor).  Larger tensors -- the PoseGuider and
    # VAE convs of a 96-frame 512 x 512 clip -- are worked in runs of whole images: images are independent in a conv.
    lim = DMA_LIMIT
    per_img = max(t.numel() // NB * t.element_size() for t in (x, out, x1, residual) if t is not None)
    if per_img * NB > lim and NB > 1:
        step = max(1, lim // per_img)
        for n0 in range(0, NB, step):
            n1 = min(NB, n0 + step)
            b2, b2r = None, bias2_rows
            if bias2 is not None:
                m0, m1 = n0 * oh * ow, n1 * oh * ow
                if bias2_rows >= NB * oh * ow:              # ONE row for every output row (see gemm)
                    b2, b2r = bias2[:1], max(m1 - m0, bias2_rows)
                elif m0 % bias2_rows:
                    raise RuntimeError("conv3x3: a batch split inside a bias2 row group is not supported")
                else:
                    b2 = bias2[m0 // bias2_rows:(m1 + bias2_rows - 1) // bias2_rows]
            conv3x3(x[n0:n1], wp, bias, stride=stride, upsample=upsample, bias2=b2, bias2_rows=b2r,
                    residual=None if residual is None else residual[n0:n1], act=act, x1=None if x1 is None else x1[n0:n1],
                    out=out[n0:n1], pad_high_only=pad_high_only)
        return out
    _check(lib().mmgt_conv3x3_nhwc(_ptr(x), C0, _ptr(x1), C1, NB, IH, IW, -2 if pad_high_only else stride, int(upsample), _ptr(wp),
                                   _ptr(_f32(bias, "bias")), _ptr(_f32(bias2, "bias2")), bias2_rows, _ptr(residual),
                                   _ptr(out), cout, act, dtype_code(x.dtype), _stream()), "mmgt_conv3x3_nhwc")
    return out


# ------------------------------------------------------------------------------------------------------------ norms

def groupnorm(x, gamma, beta, groups, eps, silu=False, x1=None, out=None):
    """x (NB, HW, C0) [+ x1 (NB, HW, C1)] -> (NB, HW, C0+C1), per-image GroupNorm (+ SiLU)."""
    _dev(x, gamma, beta, x1)
    assert x.dim() == 3 and x.is_contiguous()
    NB, HW, C0 = x.shape
    C1 = 0 if x1 is None else x1.shape[2]
    if x1 is not None:
        assert x1.is_contiguous() and x1.shape[:2] == x.shape[:2] and x1.dtype == x.dtype
    if out is None:
        out = torch.empty((NB, HW, C0 + C1), device=x.device, dtype=x.dtype)
    chunks = lib().mmgt_groupnorm_chunks(HW)
    ws = torch.empty((NB * chunks * groups * 2,), device=x.device, dtype=torch.float32)
    _check(lib().mmgt_groupnorm_nhwc(_ptr(x), C0, _ptr(x1), C1, _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")),
                                     _ptr(out), _ptr(ws), NB, HW, groups, eps, int(silu), dtype_code(x.dtype),
                                     _stream()), "mmgt_groupnorm_nhwc")
    return out


def groupnorm_affine(x, gamma, beta, groups, eps, x1=None):
    """x (NB, HW, C) [+ x1 (NB, HW, C1): the channel concatenation] -> (scale, shift), fp32 (NB, C + C1) each:
    GroupNorm(x | x1)[n, p, c] = (x | x1)[n, p, c] * scale[n, c] + shift[n, c].
    The statistics pass of `groupnorm` alone; `rowgemm320(pre_scale=, pre_shift=)` / `gn_silu_conv3x3_unet` apply the tables while they load x."""
    _dev(x, gamma, beta, x1)
    assert x.dim() == 3 and x.is_contiguous()
    NB, HW, C = x.shape
    C1 = 0
    if x1 is not None:
        assert x1.is_contiguous() and x1.shape[:2] == x.shape[:2] and x1.dtype == x.dtype
        C1 = x1.shape[2]
    chunks = lib().mmgt_groupnorm_chunks(HW)
    ws = torch.empty((NB * chunks * groups * 2,), device=x.device, dtype=torch.float32)
    tab = torch.empty((2, NB, C + C1), device=x.device, dtype=torch.float32)       # one allocation: the fused convs fetch scale | shift rows with one descriptor
    scale, shift = tab[0], tab[1]
    _check(lib().mmgt_groupnorm_affine2(_ptr(x), C, _ptr(x1), C1, _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), _ptr(ws), _ptr(scale),
                                        _ptr(shift), NB, HW, groups, eps, dtype_code(x.dtype), _stream()), "mmgt_groupnorm_affine2")
    return scale, shift


def gn_silu_conv3x3_unet_supported(dtype, c0, c1, cout, H, W):
    """csrc/rconv.hip: bf16, 16 x 16 pixel tiles, 64-channel phases, output blocks of 320 / 256 / 160 channels"""
    return dtype == torch.bfloat16 and c0 % 64 == 0 and c1 % 64 == 0 and c0 > 0 and cout % 160 == 0 and H % 16 == 0 and W % 16 == 0


def gn_silu_conv3x3_unet(x, scale, shift, wimg, cout, bias=None, bias2=None, b2_imgs=0, residual=None, x1=None, out=None, next_norm=None):
    """bias + bias2[n // b2_imgs] + conv3x3(silu((x | x1) * scale[n, c] + shift[n, c])) (+ residual) in one launch (csrc/rconv.hip): x (NB, H, W, C0)
    [, x1 (NB, H, W, C1)] bf16 channels-last, (scale, shift) the tables of `groupnorm_affine` (one allocation), wimg = packing.pack_rconv(weight).
    next_norm = (gamma, beta, groups, eps) of the GroupNorm that reads the result: returns (out, (scale, shift) of THAT norm) -- its statistics
    come from the launch's epilogue and a small fold (mmgt_gn_stats_finalize_unet), the pass over the tensor is not needed."""
    _dev(x, scale, shift, wimg, bias, bias2, residual, x1, out)
    assert x.dim() == 4 and x.is_contiguous()
    NB, H, W, C0 = x.shape
    C1 = 0
    if x1 is not None:
        assert x1.is_contiguous() and x1.shape[:3] == x.shape[:3] and x1.dtype == x.dtype
        C1 = x1.shape[3]
    assert gn_silu_conv3x3_unet_supported(x.dtype, C0, C1, cout, H, W)
    C = C0 + C1
    assert scale.shape == (NB, C) and shift.shape == (NB, C) and scale.dtype == torch.float32 and scale.is_contiguous() and shift.is_contiguous()
    assert shift.data_ptr() == scale.data_ptr() + 4 * NB * C, "scale and shift must be the two halves of one allocation (groupnorm_affine)"
    assert wimg.dtype == torch.uint8 and wimg.is_contiguous() and wimg.numel() == lib().mmgt_gn_silu_conv3x3_unet_image_bytes(C, cout)
    if out is None:
        out = torch.empty((NB, H, W, cout), device=x.device, dtype=x.dtype)
    assert out.shape == (NB, H, W, cout) and out.is_contiguous() and out.dtype == x.dtype
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous() and residual.dtype == x.dtype
    if bias2 is not None:
        assert bias2.dim() == 2 and bias2.shape[1] == cout and bias2.is_contiguous() and b2_imgs > 0 and (NB + b2_imgs - 1) // b2_imgs <= bias2.shape[0]
    stats = None
    if next_norm is not None:
        rows = lib().mmgt_gn_silu_conv3x3_unet_stats_rows(NB, H, W, cout)
        assert rows in (2, 4)
        ppi = (H // 16) * (W // 16) * (16 // rows)
        stats = torch.empty((3, NB * ppi, cout), device=x.device, dtype=torch.float32)
    _check(lib().mmgt_gn_silu_conv3x3_unet_stats(_ptr(x), C0, _ptr(x1), C1, _ptr(scale), _ptr(wimg), _ptr(_f32(bias, "bias")), _ptr(_f32(bias2, "bias2")),
                                                 b2_imgs, _ptr(residual), _ptr(out), _ptr(stats), NB, H, W, cout, dtype_code(x.dtype), _stream()),
           "mmgt_gn_silu_conv3x3_unet")
    if next_norm is None:
        return out
    gamma, beta, groups, eps = next_norm
    tab = torch.empty((2, NB, cout), device=x.device, dtype=torch.float32)
    _check(lib().mmgt_gn_stats_finalize_unet(_ptr(stats), _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), _ptr(tab), NB, ppi, 16 * rows, cout, groups,
                                             eps, _stream()), "mmgt_gn_stats_finalize_unet")
    return out, (tab[0], tab[1])


def gn_silu_conv3x3_supported(dtype, cin, cout, H, W, residual=False):
    """(Cin, Cout) = (128, 128), (256, 128), (256, 256: two launches on the halves of the output channels), (128, 64: no residual)"""
    return (dtype == torch.bfloat16 and ((cin, cout) in ((128, 128), (256, 128), (256, 256)) or ((cin, cout) == (128, 64) and not residual))
            and H % 16 == 0 and W % 16 == 0)


def gn_silu_conv3x3_tables(x, scale, shift, wimg, cout, bias=None, residual=None, out=None, stats=None):
    """bias + conv3x3(silu(x * scale[n, c] + shift[n, c])) (+ residual) (csrc/gnconv.hip): x (NB, H, W, Cin) bf16 channels-last, scale / shift
    (NB, Cin) fp32 (the tables of `groupnorm_affine`), wimg = packing.pack_gnconv(weight (cout, Cin, 3, 3)): one launch per 128 output channels.
    stats: or a (NB * (H / 16) * (W / 16), cout / 4, 2) fp32 tensor that receives the per-tile (sum, sum of squares) of the stored values
    (`gn_tables_from_stats` turns them into the tables of the GroupNorm that reads `out`)."""
    _dev(x, scale, shift, wimg, bias, residual, out, stats)
    assert x.dim() == 4 and x.is_contiguous()
    NB, H, W, C = x.shape
    assert gn_silu_conv3x3_supported(x.dtype, C, cout, H, W, residual is not None) and x.numel() * x.element_size() <= DMA_LIMIT
    assert scale.shape == (NB, C) and shift.shape == (NB, C) and scale.dtype == torch.float32 and shift.dtype == torch.float32
    assert scale.is_contiguous() and shift.is_contiguous()
    if shift.data_ptr() != scale.data_ptr() + 4 * NB * C:                     # the kernel wants the two tables in one allocation
        tab = torch.stack([scale, shift])
        scale, shift = tab[0], tab[1]
    cl = min(cout, 128)                                                # output channels per launch
    per = lib().mmgt_gn_silu_conv3x3_image_bytes(C, cl)
    assert wimg.dtype == torch.uint8 and wimg.is_contiguous() and wimg.numel() == per * (cout // cl)
    if out is None:
        out = torch.empty((NB, H, W, cout), device=x.device, dtype=x.dtype)
    assert out.shape == (NB, H, W, cout) and out.is_contiguous() and out.dtype == x.dtype and out.numel() * 2 <= DMA_LIMIT
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous() and residual.dtype == x.dtype
    if stats is not None:
        assert cl == 128 and stats.dtype == torch.float32 and stats.is_contiguous() and stats.shape == (NB * (H // 16) * (W // 16), cout // 4, 2)
    bias = _f32(bias, "bias")
    if bias is not None:
        assert bias.numel() >= cout
    for h in range(cout // cl):
        _check(lib().mmgt_gn_silu_conv3x3(_ptr(x), _ptr(scale), _ptr(shift), wimg.data_ptr() + h * per, None if bias is None else bias.data_ptr() + 4 * cl * h,
                                          None if residual is None else residual.data_ptr() + 2 * cl * h, out.data_ptr() + 2 * cl * h,
                                          None if stats is None else stats.data_ptr() + 4 * 64 * h,
                                          NB, H, W, C, cl, cout, dtype_code(x.dtype), _stream()), "mmgt_gn_silu_conv3x3")
    return out


def gn_tables_from_stats(stats, gamma, beta, groups, eps, NB, C):
    """(scale, shift) of GroupNorm(groups, gamma, beta, eps) over a tensor (NB, H, W, C) from the per-tile partial sums `gn_silu_conv3x3*` wrote
    while storing it (stats (NB * tiles, C / 4, 2)): one small launch instead of the statistics pass over the tensor."""
    _dev(stats, gamma, beta)
    assert stats.dim() == 3 and stats.shape[1] == C // 4 and stats.shape[2] == 2 and stats.shape[0] % NB == 0 and stats.is_contiguous()
    tab = torch.empty((2, NB, C), device=stats.device, dtype=torch.float32)
    _check(lib().mmgt_gn_stats_finalize(_ptr(stats), _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), _ptr(tab[0]), _ptr(tab[1]), NB, stats.shape[0] // NB,
                                        C, groups, eps, _stream()), "mmgt_gn_stats_finalize")
    return tab[0], tab[1]


def gn_silu_conv3x3(x, gamma, beta, groups, eps, wimg, cout, bias=None, residual=None, out=None, tables=None, want_stats=False):
    """conv3x3(silu(GroupNorm(x))) (+ residual): the statistics from `tables` (scale, shift) if the caller has them (`gn_tables_from_stats` of the
    launch that produced x), else ONE pass over x (`groupnorm_affine`); then one fused launch per 128 output channels.  x (NB, H, W, Cin) bf16
    channels-last -> (NB, H, W, cout), or (out, stats) with want_stats (stats = None where the launch cannot produce them)."""
    assert x.dim() == 4 and x.is_contiguous()
    NB, H, W, C = x.shape
    if out is None:
        out = torch.empty((NB, H, W, cout), device=x.device, dtype=x.dtype)
    stats = None
    if want_stats and cout % 128 == 0:
        stats = torch.empty((NB * (H // 16) * (W // 16), cout // 4, 2), device=x.device, dtype=torch.float32)
    step = max(1, DMA_LIMIT // (H * W * max(C, cout) * x.element_size()))       # 32-bit buffer offsets: runs of whole images below 2 GiB
    tiles = (H // 16) * (W // 16)
    for n0 in range(0, NB, step):
        n1 = min(NB, n0 + step)
        if tables is None:
            scale, shift = groupnorm_affine(x[n0:n1].view(n1 - n0, H * W, C), gamma, beta, groups, eps)
        else:
            scale, shift = tables[0][n0:n1], tables[1][n0:n1]
        gn_silu_conv3x3_tables(x[n0:n1], scale, shift, wimg, cout, bias, None if residual is None else residual[n0:n1], out[n0:n1],
                               None if stats is None else stats[n0 * tiles:n1 * tiles])
    return (out, stats) if want_stats else out


def layernorm(x, gamma, beta, eps=1e-5, pe=None, pe_div=1, pe_mod=1, out=None):
    """x (rows, C) -> LayerNorm over C (+ pe[(row // pe_div) % pe_mod] added after the affine).  With pe=None and
    pe_mod > 1, `beta` is a (>= pe_mod, C) table of beta + pe rows indexed the same way."""
    _dev(x, gamma, beta, pe)
    assert x.dim() == 2 and x.stride(1) == 1
    rows, C = x.shape
    if pe is None and pe_mod > 1:
        assert beta.dim() == 2 and beta.shape[0] >= pe_mod and beta.shape[1] == C and beta.is_contiguous()
    else:
        assert beta.numel() == C
    if out is None:
        out = torch.empty((rows, C), device=x.device, dtype=x.dtype)
    _check(lib().mmgt_layernorm(_ptr(x), x.stride(0), _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), eps,
                                _ptr(_f32(pe, "pe")), pe_div, pe_mod, _ptr(out), out.stride(0), rows, C,
                                dtype_code(x.dtype), _stream()), "mmgt_layernorm")
    return out


def channel_norm_gelu(x, gamma, beta, eps=1e-5):
    """(rows, C): per-channel normalisation over the rows + affine + GELU (wav2vec2's first conv layer)."""
    _dev(x, gamma, beta)
    assert x.dim() == 2 and x.is_contiguous()
    out = torch.empty_like(x)
    _check(lib().mmgt_channel_norm_gelu(_ptr(x), _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), _ptr(out), x.shape[0], x.shape[1], eps,
                                        dtype_code(x.dtype), _stream()), "mmgt_channel_norm_gelu")
    return out


def lerp_rows(x, rows_out):
    """(rows_in, C) -> (rows_out, C): linear interpolation along the rows, align_corners=True."""
    _dev(x)
    assert x.dim() == 2 and x.is_contiguous()
    out = torch.empty((rows_out, x.shape[1]), device=x.device, dtype=x.dtype)
    _check(lib().mmgt_lerp_rows(_ptr(x), _ptr(out), x.shape[0], rows_out, x.shape[1], dtype_code(x.dtype), _stream()), "mmgt_lerp_rows")
    return out


def ff_fused_supported(C, inner, dtype):
    return dtype == torch.bfloat16 and lib().mmgt_ff_fused_image_bytes(C, inner) > 0


def ff_fused(x, ln_gamma, ln_beta, wimg, bias2, residual, inner, eps=1e-5, out=None):
    """out = residual + bias2 + W2 . GEGLU(W1 . LN(x) + b1) in one launch (x (M, 320) bf16; wimg = packing.pack_ff_fused(...);
    ln_gamma None: x is used as it is)."""
    _dev(x, ln_gamma, ln_beta, wimg, bias2, residual)
    assert x.dim() == 2 and x.stride(1) == 1 and residual.shape == x.shape and residual.stride(1) == 1 and residual.dtype == x.dtype
    M, C = x.shape
    assert wimg.dtype == torch.uint8 and wimg.is_contiguous() and wimg.numel() == lib().mmgt_ff_fused_image_bytes(C, inner)
    if out is None:
        out = torch.empty((M, C), device=x.device, dtype=x.dtype)
    assert out.shape == (M, C) and out.stride(1) == 1 and out.dtype == x.dtype
    _check(lib().mmgt_ff_fused(_ptr(x), x.stride(0), _ptr(_f32(ln_gamma, "ln_gamma")), _ptr(_f32(ln_beta, "ln_beta")), eps, _ptr(wimg),
                               _ptr(_f32(bias2, "bias2")), _ptr(residual), residual.stride(0), _ptr(out), out.stride(0), M, C, inner,
                               dtype_code(x.dtype), _stream()), "mmgt_ff_fused")
    return out


def ff_fused_po(x, ln_gamma, ln_beta, wimg, bias2, residual, inner, wpo, bias_po, residual2, eps=1e-5, out=None):
    """`ff_fused` with the transformer block's proj_out on the end of the same launch: out = residual2 + bias_po + Wpo . hidden,
    hidden = bf16(residual + bias2 + FeedForward(LN(x))) never stored (wpo = packing.pack_ff_proj_out(proj_out.weight))."""
    _dev(x, ln_gamma, ln_beta, wimg, bias2, residual, wpo, bias_po, residual2)
    assert x.dim() == 2 and x.stride(1) == 1 and residual.shape == x.shape and residual.stride(1) == 1 and residual.dtype == x.dtype
    assert residual2.shape == x.shape and residual2.stride(1) == 1 and residual2.dtype == x.dtype
    M, C = x.shape
    assert wimg.dtype == torch.uint8 and wimg.is_contiguous() and wimg.numel() == lib().mmgt_ff_fused_image_bytes(C, inner)
    assert wpo.dtype == torch.uint8 and wpo.is_contiguous() and wpo.numel() == C * C * 2
    if out is None:
        out = torch.empty((M, C), device=x.device, dtype=x.dtype)
    assert out.shape == (M, C) and out.stride(1) == 1 and out.dtype == x.dtype
    _check(lib().mmgt_ff_fused_po(_ptr(x), x.stride(0), _ptr(_f32(ln_gamma, "ln_gamma")), _ptr(_f32(ln_beta, "ln_beta")), eps, _ptr(wimg),
                                  _ptr(_f32(bias2, "bias2")), _ptr(residual), residual.stride(0), _ptr(wpo), _ptr(_f32(bias_po, "bias_po")),
                                  _ptr(residual2), residual2.stride(0), _ptr(out), out.stride(0), M, C, inner, dtype_code(x.dtype), _stream()),
           "mmgt_ff_fused_po")
    return out


def rowgemm320_supported(dtype, K, N):
    return dtype == torch.bfloat16 and K == 320 and lib().mmgt_rowgemm320_image_bytes(N) > 0


def rowgemm320(x, wimg, N, bias=None, *, ln_gamma=None, ln_beta=None, pe_div=0, pe_mod=0, eps=1e-5, residual=None, bias2=None,
               bias2_rows=0, n1=None, out=None, out_t=None, n_tok=0, pre_scale=None, pre_shift=None, pre_rows=0, pre_silu=False):
    """[LayerNorm ->] Linear of the 320-channel level in one launch that reads x once (csrc/rowgemm.hip).  x (M, 320) bf16, wimg =
    packing.pack_rowgemm(W (N, 320)).  Columns [0, n1) -> out (M, n1) row-major (+ residual, n1 == N only), columns [n1, N) ->
    out_t (M / n_tok, N - n1, npad) transposed per batch of n_tok rows (the V^T operand of `attention(v_transposed=True)`).
    ln_beta (pe_mod, 320) fp32: row (m / pe_div) % pe_mod.  pre_scale / pre_shift (M / pre_rows, 320) fp32 instead of a LayerNorm:
    x * scale[m / pre_rows] + shift[m / pre_rows] (`groupnorm_affine`; pre_silu: SiLU behind it).  Returns (out, out_t)."""
    _dev(x, wimg, bias, ln_gamma, ln_beta, residual, bias2, out, out_t, pre_scale, pre_shift)
    norm = 1 if ln_gamma is not None else 0
    if pre_scale is not None:
        assert ln_gamma is None and pre_rows > 0 and x.shape[0] % pre_rows == 0
        assert pre_scale.shape == pre_shift.shape == (x.shape[0] // pre_rows, 320) and pre_scale.is_contiguous() and pre_shift.is_contiguous()
        norm, ln_gamma, ln_beta, pe_div, pe_mod = (3 if pre_silu else 2), pre_scale, pre_shift, pre_rows, x.shape[0] // pre_rows
    assert x.dim() == 2 and x.shape[1] == 320 and x.stride(1) == 1 and x.dtype == torch.bfloat16
    M = x.shape[0]
    n1 = N if n1 is None else n1
    assert wimg.dtype == torch.uint8 and wimg.is_contiguous() and wimg.numel() == lib().mmgt_rowgemm320_image_bytes(N)
    if n1 and out is None:
        out = torch.empty((M, n1), device=x.device, dtype=x.dtype)
    npad = 0
    if n1 < N:
        assert n_tok > 0 and M % n_tok == 0
        if out_t is None:
            out_t = torch.empty((M // n_tok, N - n1, (n_tok + 7) // 8 * 8), device=x.device, dtype=x.dtype)
        assert out_t.dtype == x.dtype and out_t.is_contiguous() and out_t.shape[:2] == (M // n_tok, N - n1)
        npad = out_t.shape[2]
    if out is not None:
        assert out.shape == (M, n1) and out.stride(1) == 1 and out.dtype == x.dtype
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1 and residual.dtype == x.dtype
    if ln_beta is not None:
        assert ln_beta.is_contiguous() and ln_beta.numel() >= 320 * max(pe_mod, 1)
    if bias2 is not None:
        assert bias2.dim() == 2 and bias2.shape[1] == N and bias2.is_contiguous() and (M + bias2_rows - 1) // bias2_rows <= bias2.shape[0]
    _check(lib().mmgt_rowgemm320(_ptr(x), x.stride(0), norm, _ptr(_f32(ln_gamma, "ln_gamma")), _ptr(_f32(ln_beta, "ln_beta")), pe_div, pe_mod,
                                 eps, _ptr(wimg), _ptr(_f32(bias, "bias")), _ptr(_f32(bias2, "bias2")), bias2_rows, _ptr(residual),
                                 0 if residual is None else residual.stride(0), _ptr(out), 0 if out is None else out.stride(0), n1,
                                 _ptr(out_t), n_tok, npad, M, N, dtype_code(x.dtype), _stream()), "mmgt_rowgemm320")
    return out, out_t


def temporal_leg320_supported(dtype, C, heads, frames, n_pix, batch=1):
    """What csrc/tleg.hip is built for: bf16, 8 heads of 40, windows of 24 or 12 frames, whole 4-wave tasks, a tensor a buffer resource
    can address (2 GiB) -- a caller with any other shape takes the three-launch path."""
    return dtype == torch.bfloat16 and C == 320 and heads == 8 and frames in (12, 24) and n_pix % (4 * 48 // frames) == 0 and \
        batch * frames * n_pix * 640 < (1 << 31)


def temporal_leg320(x, ln_gamma, beta_pe, wimg, bias_o, batch, frames, n_pix, scale, eps=1e-5, out=None):
    """x + to_out(temporal attention(LayerNorm(x) + pe)) of a level-0 motion-module attention block in ONE launch (csrc/tleg.hip).  x (batch *
    frames * n_pix, 320) bf16 rows (batch, frame, pixel); beta_pe (>= frames, 320) fp32 = LayerNorm bias + pe rows; wimg = packing.pack_tleg."""
    _dev(x, ln_gamma, beta_pe, wimg, bias_o, out)
    if not (x.dim() == 2 and temporal_leg320_supported(x.dtype, x.shape[1], 8, frames, n_pix, batch)):
        raise RuntimeError(f"temporal_leg320: unsupported shape (dtype {x.dtype}, {tuple(x.shape)}, {frames} frames x {n_pix} pixels x batch {batch}): "
                           "8 heads of 40 channels, 12 or 24 frames, bf16, < 2 GiB")
    assert x.dim() == 2 and x.shape == (batch * frames * n_pix, 320) and x.is_contiguous() and x.dtype == torch.bfloat16
    assert wimg.dtype == torch.uint8 and wimg.is_contiguous() and wimg.numel() == lib().mmgt_temporal_leg320_image_bytes()
    assert beta_pe.dim() == 2 and beta_pe.shape[1] == 320 and beta_pe.shape[0] >= frames
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.is_contiguous() and out.dtype == x.dtype
    _check(lib().mmgt_temporal_leg320(_ptr(x), _ptr(out), _ptr(_f32(ln_gamma, "ln_gamma")), _ptr(_f32(beta_pe, "beta_pe")), beta_pe.shape[0],
                                      _ptr(wimg), _ptr(_f32(bias_o, "bias_o")), batch, frames, n_pix, scale, eps, dtype_code(x.dtype), _stream()),
           "mmgt_temporal_leg320")
    return out


# ------------------------------------------------------------------------------------------------------------ attention

def attention(q, k, v, out, *, batch, heads, hd, nq, nk, scale, q_str, k_str, v_str, o_str, bdiv=1, v_transposed=False,
              k2=None, v2=None, k2_str=(0, 0), v2_str=(0, 0), k2_bdiv=1, nk2=0, seg2_first_batch=0, out_scale=None, out_scale_heads=0,
              twin_out=None):
    """Raw strided attention (see include/mmgt_hip.h).  *_str = (batch stride 0, batch stride 1, token stride).
    out_scale (groups, batch * nq) fp32 + out_scale_heads: the output rows of head group g = head // out_scale_heads are multiplied by
    out_scale[g] (mmgt_attention_scaled: single key segment, row-major V)."""
    _dev(q, k, v, out, k2, v2, out_scale, twin_out)
    if twin_out is not None:
        # every batch entry reads (k2, v2); twin_out (out's strides) receives the attention over (k, v) alone (mmgt_attention_twin)
        assert k2 is not None and v_transposed and seg2_first_batch == 0 and out_scale is None and twin_out.dtype == out.dtype
        _check(lib().mmgt_attention_twin(_ptr(q), q_str[0], q_str[1], q_str[2], _ptr(k), k_str[0], k_str[1], k_str[2], _ptr(v),
                                         v_str[0], v_str[1], v_str[2], _ptr(out), _ptr(twin_out), o_str[0], o_str[1], o_str[2], bdiv,
                                         _ptr(k2), _ptr(v2), k2_str[0], k2_str[1], v2_str[0], v2_str[1], k2_bdiv, nk2, batch, heads, hd,
                                         nq, nk, scale, dtype_code(q.dtype), _stream()), "mmgt_attention_twin")
        return out
    if out_scale is not None:
        assert k2 is None and not v_transposed and bdiv == 1 and out_scale_heads > 0 and heads % out_scale_heads == 0
        assert out_scale.dtype == torch.float32 and out_scale.dim() == 2 and out_scale.stride(1) == 1
        assert out_scale.shape == (heads // out_scale_heads, batch * nq)
        _check(lib().mmgt_attention_scaled(_ptr(q), q_str[0], q_str[1], q_str[2], _ptr(k), k_str[0], k_str[1], k_str[2], _ptr(v),
                                           v_str[0], v_str[1], v_str[2], _ptr(out), o_str[0], o_str[1], o_str[2], _ptr(out_scale),
                                           out_scale.stride(0), out_scale_heads, batch, heads, hd, nq, nk, scale, dtype_code(q.dtype),
                                           _stream()), "mmgt_attention_scaled")
        return out
    _check(lib().mmgt_attention(_ptr(q), q_str[0], q_str[1], q_str[2], _ptr(k), k_str[0], k_str[1], k_str[2], _ptr(v),
                                v_str[0], v_str[1], v_str[2], _ptr(out), o_str[0], o_str[1], o_str[2], bdiv, _ptr(k2),
                                _ptr(v2), k2_str[0], k2_str[1], v2_str[0], v2_str[1], k2_bdiv, nk2, seg2_first_batch,
                                batch, heads, hd, nq, nk, scale, int(v_transposed), dtype_code(q.dtype), _stream()),
           "mmgt_attention")
    return out


def relpos_attention(q, k, v, out, x, grep_w, grep_b, grep_a, tab, *, batch, heads, T, scale, q_str, k_str, v_str, o_str, x_str, hd=64):
    """WavLM's attention with the gated relative-position bias (see include/mmgt_hip.h).  *_str = (batch stride, row stride) in
    elements; head h at column h * 64.  x: the LayerNorm output the gate is computed from; grep_w (8, 64), grep_b (8,), grep_a (heads,),
    tab (heads, 2T - 1): fp32."""
    _dev(q, k, v, out, x, grep_w, grep_b, grep_a, tab)
    assert q.dtype == k.dtype == v.dtype == out.dtype == x.dtype
    assert tuple(tab.shape) == (heads, 2 * T - 1) and grep_w.numel() == 8 * 64 and grep_b.numel() == 8 and grep_a.numel() == heads
    _check(lib().mmgt_relpos_attention(_ptr(q), q_str[0], q_str[1], _ptr(k), k_str[0], k_str[1], _ptr(v), v_str[0], v_str[1],
                                       _ptr(out), o_str[0], o_str[1], _ptr(x), x_str[0], x_str[1], _ptr(_f32(grep_w, "grep_w")),
                                       _ptr(_f32(grep_b, "grep_b")), _ptr(_f32(grep_a, "grep_a")), _ptr(_f32(tab, "tab")), batch, heads, hd,
                                       T, scale, dtype_code(q.dtype), _stream()), "mmgt_relpos_attention")
    return out


def softmax_rows(x, scale=1.0, out=None):
    _dev(x)
    assert x.dim() == 2 and x.stride(1) == 1
    if out is None:
        out = torch.empty_like(x)
    _check(lib().mmgt_softmax_rows(_ptr(x), x.stride(0), _ptr(out), out.stride(0), x.shape[0], x.shape[1], scale,
                                   dtype_code(x.dtype), _stream()), "mmgt_softmax_rows")
    return out


def softmax_rows_f32_bf16(x, scale, out):
    """fp32 logits (rows, cols) -> bf16 probabilities, one pass (cols a multiple of 256, <= 8192)."""
    _dev(x, out)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    assert out.shape == x.shape and out.stride(1) == 1 and out.dtype == torch.bfloat16
    _check(lib().mmgt_softmax_rows_f32_bf16(_ptr(x), x.stride(0), _ptr(out), out.stride(0), x.shape[0], x.shape[1], scale, _stream()),
           "mmgt_softmax_rows_f32_bf16")
    return out


def gemm_bf16_f32(a, w, out=None):
    """out fp32 (M, N) = a bf16 (M, K) @ w bf16 (N, K)^T: the raw fp32 accumulators of the bf16 MFMA path (K % 64 == 0, N % 8 == 0)."""
    _dev(a, w, out)
    assert a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1] and a.stride(1) == 1 and w.stride(1) == 1
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32)
    assert out.shape == (M, N) and out.dtype == torch.float32 and out.stride(1) == 1
    _check(lib().mmgt_gemm_bf16_f32(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(out), out.stride(0), M, N, K, _stream()),
           "mmgt_gemm_bf16_f32")
    return out


def qk_split3(qk, bias_q, bias_k, out=None):
    """qk fp32 (rows, 4C) = [t Wq_hi^T | t Wq_lo^T | t Wk_hi^T | t Wk_lo^T] -> (Qp, Kp) bf16 (rows, 3C): [q_hi|q_hi|q_lo], [k_hi|k_lo|k_hi]
    with q = qk0 + qk1 + bias_q, k = qk2 + qk3 + bias_k (so that Qp . Kp = q . k to ~17 bits on the bf16 MFMA path).  out = (Qp, Kp): write
    into these contiguous bf16 (rows, 3C) tensors."""
    _dev(qk, bias_q, bias_k, *(out or ()))
    assert qk.dim() == 2 and qk.is_contiguous() and qk.dtype == torch.float32 and qk.shape[1] % 16 == 0
    rows, C = qk.shape[0], qk.shape[1] // 4
    assert bias_q.shape == (C,) and bias_k.shape == (C,) and bias_q.dtype == torch.float32 and bias_k.dtype == torch.float32
    if out is None:
        out = (torch.empty((rows, 3 * C), device=qk.device, dtype=torch.bfloat16), torch.empty((rows, 3 * C), device=qk.device, dtype=torch.bfloat16))
    Qp, Kp = out
    for t in out:
        assert t.shape == (rows, 3 * C) and t.dtype == torch.bfloat16 and t.is_contiguous()
    _check(lib().mmgt_qk_split3(_ptr(qk), _ptr(bias_q), _ptr(bias_k), _ptr(Qp), _ptr(Kp), rows, C, _stream()), "mmgt_qk_split3")
    return Qp, Kp


# ------------------------------------------------------------------------------------------------------------ plumbing

def ncfhw_to_nhwc(x, cpad, dtype, scale=1.0, out=None):
    """(B, C, F, H, W) fp32 -> (B*F, H, W, cpad) channels-last `dtype` (times `scale`), zero padded channels."""
    _dev(x, out)
    assert x.dim() == 5 and x.dtype == torch.float32 and x.is_contiguous()
    B, C, F, H, W = x.shape
    if out is None:
        out = torch.empty((B * F, H, W, cpad), device=x.device, dtype=dtype)
    assert out.shape == (B * F, H, W, cpad) and out.dtype == dtype and out.is_contiguous()
    _check(lib().mmgt_ncfhw_to_nhwc(_ptr(x), _ptr(out), B, C, F, H, W, cpad, scale, dtype_code(dtype), _stream()),
           "mmgt_ncfhw_to_nhwc")
    return out


def nhwc_to_ncfhw(x, B, C, scale=1.0, shift=0.0, clamp01=False, out=None):
    """(B*F, H, W, cpad) -> (B, C, F, H, W) fp32 (first C channels), out = clamp(x * scale + shift)."""
    _dev(x, out)
    assert x.dim() == 4 and x.is_contiguous()
    BF, H, W, cpad = x.shape
    F = BF // B
    if out is None:
        out = torch.empty((B, C, F, H, W), device=x.device, dtype=torch.float32)
    assert out.shape == (B, C, F, H, W) and out.dtype == torch.float32 and out.is_contiguous()
    _check(lib().mmgt_nhwc_to_ncfhw(_ptr(x), _ptr(out), B, C, F, H, W, cpad, scale, shift, int(clamp01),
                                    dtype_code(x.dtype), _stream()),
           "mmgt_nhwc_to_ncfhw")
    return out


def conv1x1_cat_supported(dtype, c0, c1, cout):
    return dtype == torch.bfloat16 and c0 % 64 == 0 and c1 % 64 == 0 and c0 > 0 and c1 > 0 and (cout % 256 == 0 or cout % 320 == 0)


def conv1x1_cat(x0, x1, w, bias=None, residual=None, out=None):
    """bias + [x0 | x1] . w^T (+ residual): x0 (rows, C0), x1 (rows, C1) bf16, w (Cout, C0 + C1) -> (rows, Cout), one launch (csrc/gemm16.hip's conv
    gather over two sources with one tap): a resnet's conv_shortcut over the skip concatenation."""
    _dev(x0, x1, w, bias, residual, out)
    assert x0.dim() == 2 and x1.dim() == 2 and x0.shape[0] == x1.shape[0] and x0.is_contiguous() and x1.is_contiguous() and w.is_contiguous()
    rows, c0, c1, cout = x0.shape[0], x0.shape[1], x1.shape[1], w.shape[0]
    assert conv1x1_cat_supported(x0.dtype, c0, c1, cout) and w.shape == (cout, c0 + c1) and w.dtype == x0.dtype == x1.dtype
    if out is None:
        out = torch.empty((rows, cout), device=x0.device, dtype=x0.dtype)
    assert out.shape == (rows, cout) and out.is_contiguous()
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous() and residual.dtype == x0.dtype
    _check(lib().mmgt_conv1x1_cat_nhwc(_ptr(x0), c0, _ptr(x1), c1, rows, _ptr(w), _ptr(_f32(bias, "bias")), _ptr(residual), _ptr(out), cout,
                                       dtype_code(x0.dtype), _stream()), "mmgt_conv1x1_cat_nhwc")
    return out


def conv_taps_gather(y, bias, NB, H, W, out=None):
    """y (NB * H * W, ldY >= 36) bf16 = the per-pixel products of a 4-channel 3 x 3 conv (column 4 tap + o: packing.pack_conv_taps) -> (NB, H, W, 8) bf16:
    channels 0 .. 3 = bias + the sum over the taps of the neighbour pixels' products, 4 .. 7 zero."""
    _dev(y, bias, out)
    assert y.dim() == 2 and y.shape[0] == NB * H * W and y.shape[1] >= 36 and y.stride(1) == 1 and y.dtype == torch.bfloat16
    if out is None:
        out = torch.empty((NB, H, W, 8), device=y.device, dtype=y.dtype)
    assert out.shape == (NB, H, W, 8) and out.dtype == y.dtype and out.is_contiguous()
    _check(lib().mmgt_conv_taps_gather(_ptr(y), y.stride(0), _ptr(_f32(bias, "bias")), _ptr(out), NB, H, W, dtype_code(y.dtype), _stream()),
           "mmgt_conv_taps_gather")
    return out


def timestep_features(timesteps, dim, dtype, out=None):
    _dev(timesteps, out)
    assert timesteps.dtype == torch.float32 and timesteps.dim() == 1 and timesteps.is_contiguous()
    if out is None:
        out = torch.empty((timesteps.shape[0], dim), device=timesteps.device, dtype=dtype)
    assert out.shape == (timesteps.shape[0], dim) and out.dtype == dtype and out.is_contiguous()
    _check(lib().mmgt_timestep_features(_ptr(timesteps), _ptr(out), timesteps.shape[0], dim, dtype_code(dtype),
                                        _stream()), "mmgt_timestep_features")
    return out


def silu(x, out=None):
    _dev(x, out)
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
    _check(lib().mmgt_silu(_ptr(x), _ptr(out), x.numel(), dtype_code(x.dtype), _stream()), "mmgt_silu")
    return out


def cfg_ddim_step(pred_sum, counter, latents, guidance, sa_t, sb_t, sa_p, sb_p, out=None):
    """latents (1, C, F, H, W) fp32; pred_sum (2, C, F, H, W) fp32; counter (F,) fp32 -> new latents.  The kernel takes latents.numel() as
    the stride between the two CFG rows of pred_sum and indexes counter by frame: any other shape is refused before the launch."""
    _dev(pred_sum, counter, latents, out)
    assert latents.dtype == torch.float32 and latents.is_contiguous() and pred_sum.is_contiguous()
    if latents.dim() != 5 or latents.shape[0] != 1:
        raise RuntimeError(f"cfg_ddim_step: latents must be (1, C, F, H, W), got {tuple(latents.shape)}")
    if pred_sum.dtype != torch.float32 or tuple(pred_sum.shape) != (2,) + tuple(latents.shape[1:]):
        raise RuntimeError(f"cfg_ddim_step: pred_sum must be float32 {(2,) + tuple(latents.shape[1:])}, got {pred_sum.dtype} {tuple(pred_sum.shape)}")
    _, C, F, H, W = latents.shape
    if counter.numel() != F:
        raise RuntimeError(f"cfg_ddim_step: counter has {counter.numel()} entries for {F} frames")
    if out is None:
        out = torch.empty_like(latents)
    assert out.shape == latents.shape and out.dtype == torch.float32 and out.is_contiguous()
    _check(lib().mmgt_cfg_ddim_step(_ptr(pred_sum), _ptr(_f32(counter, "counter")), _ptr(latents), _ptr(out),
                                    latents.numel(), F, H * W, guidance, sa_t, sb_t, sa_p, sb_p, _stream()),
           "mmgt_cfg_ddim_step")
    return out


MOMENT_PARTIAL_ROWS = 512          # rows of per-workgroup partial sums that mmgt_cfg_moments never exceeds (include/mmgt_hip.h)


def _cfg_shapes(what, pred_sum, counter, lat_shape):
    """the refusals of `cfg_ddim_step` for the entries of csrc/sampler.hip: pred_sum float32 (2, C, F, H, W) for latents (1, C, F, H, W), counter
    float32 (F,).  -> (n, F, hw)"""
    if len(lat_shape) != 5 or lat_shape[0] != 1:
        raise RuntimeError(f"{what}: latents must be (1, C, F, H, W), got {tuple(lat_shape)}")
    if pred_sum.dtype != torch.float32 or tuple(pred_sum.shape) != (2,) + tuple(lat_shape[1:]) or not pred_sum.is_contiguous():
        raise RuntimeError(f"{what}: pred_sum must be contiguous float32 {(2,) + tuple(lat_shape[1:])}, got {pred_sum.dtype} {tuple(pred_sum.shape)}")
    _, C, F, H, W = lat_shape
    if counter.numel() != F:
        raise RuntimeError(f"{what}: counter has {counter.numel()} entries for {F} frames")
    _f32(counter, "counter")
    return C * F * H * W, F, H * W


def cfg_moments(pred_sum, counter, guidance, out=None):
    """pred_sum (2, C, F, H, W) fp32, counter (F,) fp32 -> fp64 (4,) on the device: (sum v_c, sum v_c^2, sum v_g, sum v_g^2) over the C F H W elements
    of v_c = pred_sum[1] / counter and v_g = v_u + guidance (v_c - v_u), in a fixed order (bit-equal from launch to launch).  No host sync."""
    _dev(pred_sum, counter, out)
    if pred_sum.dim() != 5:
        raise RuntimeError(f"cfg_moments: pred_sum must be (2, C, F, H, W), got {tuple(pred_sum.shape)}")
    n, F, hw = _cfg_shapes("cfg_moments", pred_sum, counter, (1,) + tuple(pred_sum.shape[1:]))
    if out is None:
        out = torch.empty((4,), device=pred_sum.device, dtype=torch.float64)
    if out.dtype != torch.float64 or tuple(out.shape) != (4,) or not out.is_contiguous():
        raise RuntimeError(f"cfg_moments: out must be contiguous float64 (4,), got {out.dtype} {tuple(out.shape)}")
    part = torch.empty((MOMENT_PARTIAL_ROWS, 4), device=pred_sum.device, dtype=torch.float64)
    _check(lib().mmgt_cfg_moments(_ptr(pred_sum), _ptr(counter), n, F, hw, guidance, _ptr(part), MOMENT_PARTIAL_ROWS, _ptr(out), _stream()),
           "mmgt_cfg_moments")
    return out


def sampler_step(pred_sum, counter, latents, guidance, sa_t, sb_t, k_x, k_0, k_1, k_v, k_z, *, rescale=0.0, moments=None, prev_x0=None, noise=None,
                 x0_out=None, out=None):
    """The general update behind the window accumulation (include/mmgt_hip.h: mmgt_sampler_step): latents (1, C, F, H, W) fp32, pred_sum and counter as
    for `cfg_ddim_step`; prev_x0 / noise / x0_out None or latents' shape -> new latents.
        v = rho (v_u + guidance (v_c - v_u));  x0 = sa_t x - sb_t v;  new = k_x x + k_0 x0 + k_1 prev_x0 + k_v v + k_z noise;  x0_out = x0
    rescale > 0: rho from `moments` (fp64 (4,) of `cfg_moments`; computed here when None).  Every refusal is raised before anything is launched."""
    _dev(pred_sum, counter, latents, moments, prev_x0, noise, x0_out, out)
    n, F, hw = _cfg_shapes("sampler_step", pred_sum, counter, tuple(latents.shape))
    if latents.dtype != torch.float32 or not latents.is_contiguous():
        raise RuntimeError(f"sampler_step: latents must be contiguous float32, got {latents.dtype}")
    if not 0.0 <= float(rescale) <= 1.0:
        raise RuntimeError(f"sampler_step: rescale must lie in [0, 1], got {rescale}")
    if out is None:
        out = torch.empty_like(latents)
    for name, t in (("prev_x0", prev_x0), ("noise", noise), ("x0_out", x0_out), ("out", out)):
        if t is not None and (t.shape != latents.shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"sampler_step: {name} must be contiguous float32 {tuple(latents.shape)} like latents, got {t.dtype} {tuple(t.shape)}")
    if k_1 != 0.0 and prev_x0 is None:
        raise RuntimeError("sampler_step: k_1 != 0 (a second-order step) needs prev_x0")
    if k_z != 0.0 and noise is None:
        raise RuntimeError("sampler_step: k_z != 0 (eta > 0) needs noise")
    if x0_out is not None and any(t is not None and t.data_ptr() == x0_out.data_ptr() for t in (prev_x0, out, latents)):
        raise RuntimeError("sampler_step: x0_out must be a buffer of its own (not prev_x0, latents or out)")
    if moments is not None and (moments.dtype != torch.float64 or tuple(moments.shape) != (4,) or not moments.is_contiguous()):
        raise RuntimeError(f"sampler_step: moments must be contiguous float64 (4,), got {moments.dtype} {tuple(moments.shape)}")
    if rescale > 0.0 and moments is None:
        moments = cfg_moments(pred_sum, counter, guidance)
    # a tensor whose coefficient is zero is not handed over: its term is skipped, whatever an unused buffer holds
    _check(lib().mmgt_sampler_step(_ptr(pred_sum), _ptr(counter), _ptr(latents), _ptr(prev_x0 if k_1 != 0.0 else None),
                                   _ptr(noise if k_z != 0.0 else None), _ptr(moments if rescale > 0.0 else None),
                                   _ptr(out), _ptr(x0_out), n, F, hw, guidance, rescale, sa_t, sb_t, k_x, k_0, k_1, k_v, k_z, _stream()),
           "mmgt_sampler_step")
    return out


# ------------------------------------------------------------------------------------------------------------ re-voicing a clip (csrc/vid2vid.hip)

MASK_GROW_MAX, FEATHER_MAX = 8, 32


def known_latents(x0, z, sa, sb, x=None, mask=None, out=None):
    """The noised known clip, and with x / mask the kept-region blend (include/mmgt_hip.h: mmgt_known_latents).  x0, z, x, out: contiguous fp32
    (1, C, F, h, w); mask: contiguous fp32 (F, h, w), 1 = take x, 0 = take known = sa x0 + sb z.  out may be x.  Every refusal is raised before
    anything is launched."""
    _dev(x0, z, x, mask, out)
    if x0.dim() != 5 or x0.shape[0] != 1:
        raise RuntimeError(f"known_latents: x0 must be (1, C, F, h, w), got {tuple(x0.shape)}")
    if (x is None) != (mask is None):
        raise RuntimeError("known_latents: x and mask come together (the blend needs both, the plain noising neither)")
    if out is None:
        out = torch.empty_like(x0)
    for name, t in (("x0", x0), ("z", z), ("x", x), ("out", out)):
        if t is not None and (t.shape != x0.shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"known_latents: {name} must be contiguous float32 {tuple(x0.shape)}, got {t.dtype} {tuple(t.shape)}")
    _, C, F, h, w = x0.shape
    if mask is not None and (tuple(mask.shape) != (F, h, w) or mask.dtype != torch.float32 or not mask.is_contiguous()):
        raise RuntimeError(f"known_latents: mask must be contiguous float32 {(F, h, w)}, got {mask.dtype} {tuple(mask.shape)}")
    if out.data_ptr() in (x0.data_ptr(), z.data_ptr()):
        raise RuntimeError("known_latents: out may be x, not x0 or z")
    _check(lib().mmgt_known_latents(_ptr(x0), _ptr(z), _ptr(x), _ptr(mask), _ptr(out), x0.numel(), F, h * w, float(sa), float(sb), _stream()),
           "mmgt_known_latents")
    return out


def mask_to_latent(mask_u8, grow=1):
    """Pixel mask uint8 (L, H, W), H and W multiples of 8 -> cell mask fp32 (L, H / 8, W / 8) of 0 / 1: 1 iff a pixel >= 128 lies in a cell within
    Chebyshev distance `grow` (0 .. 8)."""
    _dev(mask_u8)
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3 or not mask_u8.is_contiguous():
        raise RuntimeError(f"mask_to_latent: the mask must be contiguous uint8 (L, H, W), got {mask_u8.dtype} {tuple(mask_u8.shape)}")
    L, H, W = mask_u8.shape
    if L < 1 or H < 8 or W < 8 or H % 8 or W % 8:
        raise RuntimeError(f"mask_to_latent: H and W must be multiples of 8 (the VAE's cell), got {H} x {W}")
    if int(grow) != grow or not 0 <= grow <= MASK_GROW_MAX:
        raise RuntimeError(f"mask_to_latent: grow must be an integer in 0 .. {MASK_GROW_MAX}, got {grow}")
    out = torch.empty((L, H // 8, W // 8), device=mask_u8.device, dtype=torch.float32)
    _check(lib().mmgt_mask_to_latent(_ptr(mask_u8), _ptr(out), L, H, W, int(grow), _stream()), "mmgt_mask_to_latent")
    return out


def feather_alpha(cells, r=8):
    """Cell mask fp32 (L, h, w) -> paste-back alpha uint8 (L, 8 h, 8 w): the mask repeated x 8 and box-averaged over (2 r + 1)^2 pixels with edge
    replication, in integers (include/mmgt_hip.h: mmgt_feather_alpha); r in 0 .. 32."""
    _dev(cells)
    if cells.dtype != torch.float32 or cells.dim() != 3 or not cells.is_contiguous() or cells.numel() == 0:
        raise RuntimeError(f"feather_alpha: the cell mask must be contiguous float32 (L, h, w), got {cells.dtype} {tuple(cells.shape)}")
    if int(r) != r or not 0 <= r <= FEATHER_MAX:
        raise RuntimeError(f"feather_alpha: the radius must be an integer in 0 .. {FEATHER_MAX}, got {r}")
    L, h, w = cells.shape
    out = torch.empty((L, 8 * h, 8 * w), device=cells.device, dtype=torch.uint8)
    _check(lib().mmgt_feather_alpha(_ptr(cells), _ptr(out), L, h, w, int(r), _stream()), "mmgt_feather_alpha")
    return out


def composite_u8(gen, orig, alpha, out=None):
    """gen, orig uint8 (L, H, W, 3), alpha uint8 (L, H, W) -> uint8 (L, H, W, 3): every byte (g a + o (255 - a) + 127) / 255."""
    _dev(gen, orig, alpha, out)
    if gen.dtype != torch.uint8 or gen.dim() != 4 or gen.shape[3] != 3 or not gen.is_contiguous() or gen.numel() == 0:
        raise RuntimeError(f"composite_u8: gen must be contiguous uint8 (L, H, W, 3), got {gen.dtype} {tuple(gen.shape)}")
    if out is None:
        out = torch.empty_like(gen)
    for name, t in (("orig", orig), ("out", out)):
        if t.dtype != torch.uint8 or t.shape != gen.shape or not t.is_contiguous():
            raise RuntimeError(f"composite_u8: {name} must be contiguous uint8 {tuple(gen.shape)} like gen, got {t.dtype} {tuple(t.shape)}")
    if alpha.dtype != torch.uint8 or tuple(alpha.shape) != tuple(gen.shape[:3]) or not alpha.is_contiguous():
        raise RuntimeError(f"composite_u8: alpha must be contiguous uint8 {tuple(gen.shape[:3])}, got {alpha.dtype} {tuple(alpha.shape)}")
    if out.data_ptr() in (gen.data_ptr(), orig.data_ptr(), alpha.data_ptr()):
        raise RuntimeError("composite_u8: out must be a buffer of its own")
    _check(lib().mmgt_composite_u8(_ptr(gen), _ptr(orig), _ptr(alpha), _ptr(out), alpha.numel(), _stream()), "mmgt_composite_u8")
    return out


def _accumulate_operands(what, pred, pred_sum, counter, idx, weights, C, B, Fw, rows, row0):
    """The refusals shared by the two window accumulations, raised before anything is launched -> (F, hw).  weights may be None."""
    _dev(pred, pred_sum, counter, idx, weights)
    if rows not in (1, 2) or row0 not in (0, 1) or row0 + rows > 2:
        raise RuntimeError(f"{what}: CFG rows: rows must be 2 (row0 = 0), or 1 with row0 in (0, 1); got rows={rows}, row0={row0}")
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"{what}: pred must be float32 or bfloat16, got {pred.dtype}")
    if idx.dtype != torch.int32 or not idx.is_contiguous():
        raise RuntimeError(f"{what}: idx must be contiguous int32, got {idx.dtype}")
    if pred.dim() != 4 or not pred.is_contiguous() or pred.shape[0] != rows * B * Fw or pred.shape[3] < C:
        raise RuntimeError(f"{what}: pred must be contiguous ({rows * B * Fw}, h, w, cpad >= {C}) for rows={rows}, {B} window(s) of {Fw} frames, "
                           f"got {tuple(pred.shape)}")
    if pred_sum.dtype != torch.float32 or counter.dtype != torch.float32:
        raise RuntimeError(f"{what}: pred_sum must be float32 and counter must be float32, got {pred_sum.dtype} and {counter.dtype}")
    if pred_sum.dim() != 5 or not pred_sum.is_contiguous() or pred_sum.shape[0] != 2 or pred_sum.shape[1] != C:
        raise RuntimeError(f"{what}: pred_sum must be contiguous (2, C, F, h, w) with C = {C} channels, got {tuple(pred_sum.shape)}")
    F, hw = pred_sum.shape[2], pred.shape[1] * pred.shape[2]
    if pred_sum.shape[3] * pred_sum.shape[4] != hw:
        raise RuntimeError(f"{what}: pred has {hw} pixels per frame, pred_sum {pred_sum.shape[3] * pred_sum.shape[4]}")
    if counter.numel() != F or not counter.is_contiguous():
        raise RuntimeError(f"{what}: counter must be contiguous with one entry per frame: counter has {counter.numel()} entries for {F} frames")
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (Fw,) or not weights.is_contiguous()):
        raise RuntimeError(f"{what}: weights must be contiguous float32 ({Fw},), one per window position, got {weights.dtype} {tuple(weights.shape)}")
    if not 0 < Fw <= F:
        raise RuntimeError(f"{what}: a window of {Fw} frames in a clip of {F}")
    return F, hw


def accumulate_window(pred, pred_sum, counter, idx, C, rows=2, row0=0, bump_counter=True, weights=None):
    """One window into the overlap average (include/mmgt_hip.h: mmgt_accumulate_window).  pred ((rows*Fw), h, w, cpad) channels-last; pred_sum
    (2, C, F, h, w) fp32: CFG rows [row0, row0 + rows) at frames idx (int32 (Fw,) on the device) = fmaf(weights[j], pred, pred_sum);
    counter[idx[j]] += weights[j] when bump_counter.  weights fp32 (Fw,) on the device, or None for 1 everywhere (the same bits as ones)."""
    what = "accumulate_window"
    if idx.dim() != 1:
        raise RuntimeError(f"{what}: idx must be (Fw,), got {tuple(idx.shape)}")
    Fw = idx.numel()
    if Fw > 256:
        raise RuntimeError(f"{what}: a window of {Fw} frames (1 .. 256)")
    F, hw = _accumulate_operands(what, pred, pred_sum, counter, idx, weights, C, 1, Fw, rows, row0)
    _check(lib().mmgt_accumulate_window(_ptr(pred), _ptr(pred_sum), _ptr(counter), _ptr(idx), _ptr(weights), Fw, F, C, pred.shape[3], hw, rows, row0,
                                        int(bool(bump_counter)), dtype_code(pred.dtype), _stream()), "mmgt_accumulate_window")


def accumulate_windows(pred, pred_sum, counter, idx, C, rows=2, row0=0, weights=None):
    """The B windows of one sampler group in one launch (include/mmgt_hip.h: mmgt_accumulate_windows): pred ((rows*B*Fw), h, w, cpad) channels-last
    in CFG row major order [uncond w0 .. uncond w(B-1), cond w0 .. cond w(B-1)], idx (B, Fw) int32 on the device.  Added window by window in list
    order, counter collecting every covering window's weight: bitwise what B calls of `accumulate_window` on the windows' slices give."""
    what = "accumulate_windows"
    if idx.dim() != 2:
        raise RuntimeError(f"{what}: idx must be (B, Fw), got {tuple(idx.shape)}")
    B, Fw = idx.shape
    if not 1 <= B <= 256:
        raise RuntimeError(f"{what}: {B} windows in a group (1 .. 256)")
    F, hw = _accumulate_operands(what, pred, pred_sum, counter, idx, weights, C, B, Fw, rows, row0)
    if F > 65535:
        raise RuntimeError(f"{what}: {F} frames (the launch has one grid row per frame, up to 65535)")
    _check(lib().mmgt_accumulate_windows(_ptr(pred), _ptr(pred_sum), _ptr(counter), _ptr(idx), _ptr(weights), B, Fw, F, C, pred.shape[3], hw, rows,
                                         row0, dtype_code(pred.dtype), _stream()), "mmgt_accumulate_windows")


# ------------------------------------------------------------------------------------------------------------ SMGA glue

def rotary(x, cos_sin, seq):
    """x (rows, dim) -> rotated pairs, angle table cos_sin (>= seq, dim/2, 2) fp32 indexed by row % seq."""
    _dev(x, cos_sin)
    assert x.dim() == 2 and x.is_contiguous() and cos_sin.is_contiguous() and cos_sin.shape[0] >= seq
    out = torch.empty_like(x)
    _check(lib().mmgt_rotary(_ptr(x), _ptr(_f32(cos_sin, "cos_sin")), _ptr(out), x.shape[0], x.shape[1], seq, dtype_code(x.dtype),
                             _stream()), "mmgt_rotary")
    return out


def film_residual(x, scale_shift, rows_per_batch, res=None, res2=None):
    """res (+ res2) + (scale + 1) * x + shift; scale_shift: fp32 (B, >= 2 dim) view with unit column stride, [scale | shift] per row."""
    _dev(x, scale_shift, res, res2)
    assert x.dim() == 2 and x.is_contiguous() and scale_shift.dtype == torch.float32 and scale_shift.stride(1) == 1
    assert scale_shift.shape[1] >= 2 * x.shape[1] and scale_shift.shape[0] * rows_per_batch >= x.shape[0]
    for r in (res, res2):
        assert r is None or (r.shape == x.shape and r.is_contiguous() and r.dtype == x.dtype)
    out = torch.empty_like(x)
    _check(lib().mmgt_film_residual(_ptr(x), _ptr(scale_shift), scale_shift.stride(0), _ptr(res), _ptr(res2), _ptr(out), x.shape[0],
                                    x.shape[1], rows_per_batch, dtype_code(x.dtype), _stream()), "mmgt_film_residual")
    return out


def mean_tokens(x):
    """(B, T, C) -> fp32 (B, C)."""
    _dev(x)
    assert x.dim() == 3 and x.is_contiguous()
    out = torch.empty((x.shape[0], x.shape[2]), device=x.device, dtype=torch.float32)
    _check(lib().mmgt_mean_tokens(_ptr(x), _ptr(out), x.shape[0], x.shape[1], x.shape[2], dtype_code(x.dtype), _stream()),
           "mmgt_mean_tokens")
    return out


def activation(x, act):
    _dev(x)
    assert x.is_contiguous()
    out = torch.empty_like(x)
    _check(lib().mmgt_activation(_ptr(x), _ptr(out), x.numel(), act, dtype_code(x.dtype), _stream()), "mmgt_activation")
    return out


def smga_ddim_step(pred_uncond, pred_cond, x, noise, guidance, sqrt_recip, sqrt_recipm1, sqrt_next, c, sigma, last):
    _dev(pred_uncond, pred_cond, x, noise)
    assert pred_uncond.is_contiguous() and pred_cond.is_contiguous() and pred_uncond.dtype == pred_cond.dtype
    assert x.dtype == torch.float32 and x.is_contiguous() and pred_uncond.numel() == x.numel() == pred_cond.numel()
    out = torch.empty_like(x)
    _check(lib().mmgt_smga_ddim_step(_ptr(pred_uncond), _ptr(pred_cond), _ptr(x), _ptr(_f32(noise, "noise")), _ptr(out), x.numel(),
                                     guidance, sqrt_recip, sqrt_recipm1, sqrt_next, c, sigma, int(last),
                                     dtype_code(pred_uncond.dtype), _stream()), "mmgt_smga_ddim_step")
    return out


# ------------------------------------------------------------------------------------------------------------ conditioning / output

def blur_mask_u8(masks, ksize):
    """(L, H, W) uint8 -> (L, 64, 64) uint8 (see mmgt_blur_mask_u8)."""
    _dev(masks)
    assert masks.dtype == torch.uint8 and masks.dim() == 3 and masks.is_contiguous()
    out = torch.empty((masks.shape[0], 64, 64), device=masks.device, dtype=torch.uint8)
    _check(lib().mmgt_blur_mask_u8(_ptr(masks), _ptr(out), masks.shape[0], masks.shape[1], masks.shape[2], ksize, _stream()),
           "mmgt_blur_mask_u8")
    return out


def resample_u8(x, D, bounds, coeffs, as_float=True):
    """(L, S, S) uint8 -> (L, D, D) float32 in [0, 1] (or uint8) with PIL's integer coefficient tables (int32 device tensors)."""
    _dev(x, bounds, coeffs)
    assert x.dtype == torch.uint8 and x.dim() == 3 and x.shape[1] == x.shape[2] and x.is_contiguous()
    assert bounds.dtype == torch.int32 and coeffs.dtype == torch.int32 and bounds.shape == (D, 2) and coeffs.shape[0] == D
    out = torch.empty((x.shape[0], D, D), device=x.device, dtype=torch.float32 if as_float else torch.uint8)
    _check(lib().mmgt_resample_u8(_ptr(x), _ptr(out) if as_float else None, None if as_float else _ptr(out), x.shape[0], x.shape[1], D,
                                  _ptr(bounds), _ptr(coeffs), coeffs.shape[1], _stream()), "mmgt_resample_u8")
    return out


def resize_u8_workspace(n, Hs, Ws, Hd, Wd, C):
    """Bytes of the uint8 intermediate a resize_u8 call of that shape needs (0 unless both sizes change)."""
    b = ctypes.c_longlong(0)
    _check(lib().mmgt_resize_u8_workspace(int(n), int(Hs), int(Ws), int(Hd), int(Wd), int(C), ctypes.byref(b)), "mmgt_resize_u8_workspace")
    return b.value


def resize_u8(x, Hd, Wd, tables_x=None, tables_y=None, lut=None, out=None, tmp=None):
    """(n, Hs, Ws, C) uint8 frames, C = 1 or 3 -> PIL's Image.resize((Wd, Hd)) of every frame (see mmgt_resize_u8).  tables_x / tables_y are the
    (bounds (D, 2), kk (D, ksize)) int32 device tensors of conditioning.pil_resample_tables for the axis that changes.  Without `lut` the result is
    (n, Hd, Wd, C) uint8; with lut (C, 256) float32 it is (C, n, Hd, Wd) float32 = lut[c][value].  `out` / `tmp` (uint8, at least the workspace
    size) to write into the caller's buffers."""
    _dev(x, lut, out, tmp)
    if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError(f"resize_u8: expected contiguous uint8 (n, H, W, C) frames, got {x.dtype} {tuple(x.shape)}")
    n, Hs, Ws, C = x.shape
    Hd, Wd = int(Hd), int(Wd)
    ws = resize_u8_workspace(n, Hs, Ws, Hd, Wd, C)                   # checks the shape
    args = []
    for name, tabs, S, D in (("tables_x", tables_x, Ws, Wd), ("tables_y", tables_y, Hs, Hd)):
        if S == D:
            args += [None, None, 0]
            continue
        if tabs is None:
            raise RuntimeError(f"resize_u8: {name} is needed ({S} -> {D})")
        b, k = tabs
        _dev(b, k)
        if b.dtype != torch.int32 or k.dtype != torch.int32 or tuple(b.shape) != (D, 2) or k.dim() != 2 or k.shape[0] != D or \
                not b.is_contiguous() or not k.is_contiguous():
            raise RuntimeError(f"resize_u8: {name} must be contiguous int32 bounds ({D}, 2) and weights ({D}, ksize)")
        args += [_ptr(b), _ptr(k), k.shape[1]]
    if lut is not None and (lut.dtype != torch.float32 or tuple(lut.shape) != (C, 256) or not lut.is_contiguous()):
        raise RuntimeError(f"resize_u8: lut must be contiguous float32 ({C}, 256)")
    shape, dtype = ((n, Hd, Wd, C), torch.uint8) if lut is None else ((C, n, Hd, Wd), torch.float32)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=dtype)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
        raise RuntimeError(f"resize_u8: out must be contiguous {dtype} {shape}")
    if ws and tmp is None:
        tmp = torch.empty((ws,), device=x.device, dtype=torch.uint8)
    elif ws and (tmp.dtype != torch.uint8 or tmp.numel() < ws or not tmp.is_contiguous()):
        raise RuntimeError(f"resize_u8: tmp must be contiguous uint8 of at least {ws} bytes")
    _check(lib().mmgt_resize_u8(_ptr(x), _ptr(tmp) if ws else None, _ptr(out) if lut is None else None, None if lut is None else _ptr(out), _ptr(lut),
                                n, Hs, Ws, Hd, Wd, C, *args, _stream()), "mmgt_resize_u8")
    return out


def window_stack(x, half=2):
    """(L, ...) float32 -> (L, 2 half + 1, ...)."""
    _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    L = x.shape[0]
    D = x.numel() // L
    out = torch.empty((L, 2 * half + 1) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    _check(lib().mmgt_window_stack(_ptr(x), _ptr(out), L, D, half, _stream()), "mmgt_window_stack")
    return out


def frames_to_u8(x, scale=0.5, shift=0.5):
    """channels-last (N, H, W, cpad) -> (N, H, W, 3) uint8 = trunc(clamp(x * scale + shift, 0, 1) * 255)."""
    _dev(x)
    assert x.dim() == 4 and x.is_contiguous()
    out = torch.empty(tuple(x.shape[:3]) + (3,), device=x.device, dtype=torch.uint8)
    _check(lib().mmgt_frames_to_u8(_ptr(x), _ptr(out), x.shape[0] * x.shape[1] * x.shape[2], x.shape[3], scale, shift,
                                   dtype_code(x.dtype), _stream()), "mmgt_frames_to_u8")
    return out


# ------------------------------------------------------------------------------------------------------------ Motion-JPEG (csrc/mjpeg.hip)

JPEG_SUBSAMPLING = {"4:2:0": 420, "4:4:4": 444}


def _jpeg_ss(subsampling):
    """"4:2:0" / "4:4:4" -> the library's code; anything else goes through as an int (or 0) so that the library refuses it with its message."""
    if subsampling in JPEG_SUBSAMPLING:
        return JPEG_SUBSAMPLING[subsampling]
    return subsampling if isinstance(subsampling, int) else 0


def jpeg_geometry(H, W, subsampling):
    """(mcu_rows, mcu_cols, blocks per MCU) of an H x W frame."""
    side, bpm = (16, 6) if _jpeg_ss(subsampling) == 420 else (8, 3)
    return -(-H // side), -(-W // side), bpm


def jpeg_qtables(quality):
    """The (luminance, chrominance) quantiser tables of `quality` as 2 x 64 bytes in zigzag order: what the kernel divides by."""
    buf = ctypes.create_string_buffer(128)
    _check(lib().mmgt_jpeg_qtables(int(quality), buf), "mmgt_jpeg_qtables")
    return buf.raw[:64], buf.raw[64:]


def jpeg_segment_stride(W, subsampling):
    """Bytes that one MCU row's entropy-coded segment cannot exceed, whatever the input (csrc/mjpeg.hip states the bound)."""
    v = c_long(0)
    _check(lib().mmgt_jpeg_segment_stride(int(W), _jpeg_ss(subsampling), ctypes.byref(v)), "mmgt_jpeg_segment_stride")
    return v.value


def jpeg_dct_quant(frames, quality=90, subsampling="4:2:0"):
    """(n, H, W, 3) uint8 RGB -> (n, mcu_rows, mcu_cols, blocks per MCU, 64) int16 quantised DCT coefficients in zigzag order."""
    _dev(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise RuntimeError("jpeg_dct_quant: frames must be contiguous uint8 (n, H, W, 3)")
    n, H, W, _ = frames.shape
    out = torch.empty((n,) + jpeg_geometry(H, W, subsampling) + (64,), device=frames.device, dtype=torch.int16)
    _check(lib().mmgt_jpeg_dct_quant(_ptr(frames), _ptr(out), n, H, W, _jpeg_ss(subsampling), int(quality), _stream()), "mmgt_jpeg_dct_quant")
    return out


def jpeg_entropy(coef, H, W, subsampling="4:2:0", out=None):
    """Coefficients of jpeg_dct_quant -> (segs (n * mcu_rows, stride) uint8, sizes (n * mcu_rows,) int32): one entropy-coded segment per
    (frame, MCU row); only the first sizes[s] bytes of a row of `segs` are written.  `out` = (segs, sizes) to write into."""
    _dev(coef)
    assert coef.dtype == torch.int16 and coef.dim() == 5 and coef.is_contiguous()
    n, rows = coef.shape[0], coef.shape[1]
    stride = jpeg_segment_stride(W, subsampling)
    if out is None:
        out = (torch.empty((n * rows, stride), device=coef.device, dtype=torch.uint8),
               torch.empty((n * rows,), device=coef.device, dtype=torch.int32))
    segs, sizes = out
    assert segs.shape == (n * rows, stride) and segs.dtype == torch.uint8 and segs.is_contiguous() and sizes.shape == (n * rows,)
    assert tuple(coef.shape[1:4]) == jpeg_geometry(H, W, subsampling)
    _check(lib().mmgt_jpeg_entropy(_ptr(coef), _ptr(segs), _ptr(sizes), n, H, W, _jpeg_ss(subsampling), stride, _stream()), "mmgt_jpeg_entropy")
    return segs, sizes


def jpeg_compact(segs, sizes, mcu_rows):
    """-> (data uint8 on the device, offsets int64 (nseg + 1,) on the HOST): frame f's scan data with its RSTm / EOI markers is
    data[offsets[f * mcu_rows]:offsets[(f + 1) * mcu_rows]].  One small D2H copy (the offsets) sizes the buffer."""
    _dev(segs, sizes)
    nseg = sizes.shape[0]
    offsets = torch.empty((nseg + 1,), device=segs.device, dtype=torch.int64)
    _check(lib().mmgt_jpeg_scan(_ptr(sizes), _ptr(offsets), nseg, _stream()), "mmgt_jpeg_scan")
    host = offsets.cpu()
    total = int(host[-1])
    data = torch.empty((total,), device=segs.device, dtype=torch.uint8)
    _check(lib().mmgt_jpeg_compact(_ptr(segs), segs.shape[1], _ptr(sizes), _ptr(offsets), _ptr(data), total, nseg, int(mcu_rows), _stream()),
           "mmgt_jpeg_compact")
    return data, host


# ------------------------------------------------------------------------------------------------------------ JPEG input (csrc/jpegdec.hip)


def jpegdec_sizes(H, W, ncomp, hs, vs):
    """(blocks per frame over all component planes, int32 words of one frame's table block); the library refuses geometry it does not decode."""
    fb, ti = ctypes.c_longlong(0), c_int(0)
    _check(lib().mmgt_jpegdec_sizes(int(H), int(W), int(ncomp), int(hs), int(vs), ctypes.byref(fb), ctypes.byref(ti)), "mmgt_jpegdec_sizes")
    return fb.value, ti.value


def jpegdec_entropy(data, offsets, seginfo, tables, n, H, W, ncomp, hs, vs):
    """Restart segments -> (coef (n, frame_blocks, 64) int16 in natural order, status (nseg,) int32): include/mmgt_hip.h states the operands."""
    _dev(data, offsets, seginfo, tables)
    fb, ti = jpegdec_sizes(H, W, ncomp, hs, vs)
    nseg = seginfo.shape[0]
    if (data.dtype != torch.uint8 or data.dim() != 1 or offsets.dtype != torch.int64 or offsets.shape != (nseg + 1,) or seginfo.dtype != torch.int32
            or seginfo.shape != (nseg, 3) or tables.dtype != torch.int32 or tables.shape != (n, ti)
            or not all(t.is_contiguous() for t in (data, offsets, seginfo, tables))):
        raise RuntimeError("jpegdec_entropy: expected data uint8 (bytes,), offsets int64 (nseg + 1,), seginfo int32 (nseg, 3), tables int32 "
                           f"(n, {ti}), all contiguous")
    coef = torch.empty((n, fb, 64), device=data.device, dtype=torch.int16)
    status = torch.empty((nseg,), device=data.device, dtype=torch.int32)
    _check(lib().mmgt_jpegdec_entropy(_ptr(data), data.numel(), _ptr(offsets), _ptr(seginfo), _ptr(tables), _ptr(coef), _ptr(status), n, nseg,
                                      H, W, ncomp, hs, vs, _stream()), "mmgt_jpegdec_entropy")
    return coef, status


def jpegprog_entropy(data, offsets, seginfo, scaninfo, huff, coef, status, H, W, ncomp, hs, vs, zero_fill):
    """One dependency level of a progressive batch (csrc/jpegprog.hip): its restart segments into coef (n, frame_blocks, 64) int16, which the
    first level's call (zero_fill) clears first and later ones refine; status (nseg,) int32.  include/mmgt_hip.h states the operands."""
    _dev(data, offsets, seginfo, scaninfo, huff, coef, status)
    fb, _ = jpegdec_sizes(H, W, ncomp, hs, vs)
    nseg, n = seginfo.shape[0], coef.shape[0]
    if (data.dtype != torch.uint8 or data.dim() != 1 or offsets.dtype != torch.int64 or offsets.shape != (nseg + 1,) or seginfo.dtype != torch.int32
            or seginfo.shape != (nseg, 3) or scaninfo.dtype != torch.int32 or scaninfo.dim() != 2 or scaninfo.shape[1] != 16
            or huff.dtype != torch.int32 or huff.dim() != 2 or huff.shape[1] != 307 or coef.dtype != torch.int16 or coef.shape != (n, fb, 64)
            or status.dtype != torch.int32 or status.shape != (nseg,)
            or not all(t.is_contiguous() for t in (data, offsets, seginfo, scaninfo, huff, coef, status))):
        raise RuntimeError("jpegprog_entropy: expected data uint8 (bytes,), offsets int64 (nseg + 1,), seginfo int32 (nseg, 3), scaninfo int32 "
                           f"(nscan, 16), huff int32 (nhuff, 307), coef int16 (n, {fb}, 64), status int32 (nseg,), all contiguous")
    _check(lib().mmgt_jpegprog_entropy(_ptr(data), data.numel(), _ptr(offsets), _ptr(seginfo), _ptr(scaninfo), _ptr(huff), _ptr(coef), _ptr(status),
                                       n, nseg, scaninfo.shape[0], huff.shape[0], H, W, ncomp, hs, vs, int(bool(zero_fill)), _stream()),
           "mmgt_jpegprog_entropy")


def jpegdec_idct(coef, tables, H, W, ncomp, hs, vs):
    """Coefficients of jpegdec_entropy -> (n, frame_blocks * 64) uint8 component planes."""
    _dev(coef, tables)
    fb, ti = jpegdec_sizes(H, W, ncomp, hs, vs)
    n = coef.shape[0]
    if (coef.dtype != torch.int16 or coef.shape != (n, fb, 64) or tables.dtype != torch.int32 or tables.shape != (n, ti)
            or not coef.is_contiguous() or not tables.is_contiguous()):
        raise RuntimeError(f"jpegdec_idct: expected coef int16 (n, {fb}, 64) and tables int32 (n, {ti}), contiguous")
    planes = torch.empty((n, fb * 64), device=coef.device, dtype=torch.uint8)
    _check(lib().mmgt_jpegdec_idct(_ptr(coef), _ptr(tables), _ptr(planes), n, H, W, ncomp, hs, vs, _stream()), "mmgt_jpegdec_idct")
    return planes


def jpegdec_color(planes, H, W, ncomp, hs, vs, out=None):
    """Component planes of jpegdec_idct -> (n, H, W, 3) uint8 RGB (`out` to write into)."""
    _dev(planes)
    fb, _ = jpegdec_sizes(H, W, ncomp, hs, vs)
    n = planes.shape[0]
    if planes.dtype != torch.uint8 or planes.shape != (n, fb * 64) or not planes.is_contiguous():
        raise RuntimeError(f"jpegdec_color: expected planes uint8 (n, {fb * 64}), contiguous")
    if out is None:
        out = torch.empty((n, H, W, 3), device=planes.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or out.shape != (n, H, W, 3) or not out.is_contiguous() or out.device != planes.device:
        raise RuntimeError(f"jpegdec_color: out must be contiguous uint8 ({n}, {H}, {W}, 3) on {planes.device}")
    _check(lib().mmgt_jpegdec_color(_ptr(planes), _ptr(out), n, H, W, ncomp, hs, vs, _stream()), "mmgt_jpegdec_color")
    return out


# ------------------------------------------------------------------------------------------------------------ GIF (csrc/gif.hip)

GIF_BINS = 32768


def _rgb_frames(frames, what):
    _dev(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise RuntimeError(f"{what}: frames must be contiguous uint8 (n, H, W, 3)")
    return frames.shape[:3]


def gif_histogram(frames):
    """(n, H, W, 3) uint8 RGB -> (32768,) pixels per 5-bit-per-channel bin (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3) of the whole clip, on the
    device.  The counts are uint32 held in an int32 tensor: read them with .cpu().numpy().view(numpy.uint32)."""
    n, H, W = _rgb_frames(frames, "gif_histogram")
    hist = torch.zeros((GIF_BINS,), device=frames.device, dtype=torch.int32)
    _check(lib().mmgt_gif_histogram(_ptr(frames), _ptr(hist), n, H, W, _stream()), "mmgt_gif_histogram")
    return hist


def gif_index(frames, lut):
    """idx (n, H, W) uint8 = lut[bin(pixel)]; lut (32768,) uint8 on the device."""
    n, H, W = _rgb_frames(frames, "gif_index")
    _dev(lut)
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (GIF_BINS,) or not lut.is_contiguous():
        raise RuntimeError("gif_index: lut must be contiguous uint8 (32768,)")
    idx = torch.empty((n, H, W), device=frames.device, dtype=torch.uint8)
    _check(lib().mmgt_gif_index(_ptr(frames), _ptr(lut), _ptr(idx), n, H, W, _stream()), "mmgt_gif_index")
    return idx


def gif_dither_band():
    """Rows of one band of mmgt_gif_dither (csrc/gif_dither_core.h: GDI_BAND): a taller frame passes a row of errors from band to band."""
    return lib().mmgt_gif_dither_band()


def gif_dither_scratch_bytes(n, H, W):
    """Bytes of scratch that gif_dither needs for n frames of H x W: the carry rows, none for frames of a single band."""
    v = ctypes.c_longlong(0)
    _check(lib().mmgt_gif_dither_scratch(int(n), int(H), int(W), ctypes.byref(v)), "mmgt_gif_dither_scratch")
    return v.value


def gif_dither(frames, lut, palette, out=None, scratch=None):
    """idx (n, H, W) uint8 under Floyd-Steinberg error diffusion against `palette` (256, 3) uint8 (csrc/gif_dither_core.h states the rule); lut as
    for gif_index.  `out` (n, H, W) uint8 contiguous (any alignment) and `scratch` uint8 (>= gif_dither_scratch_bytes, contents irrelevant) to write
    into."""
    n, H, W = _rgb_frames(frames, "gif_dither")
    _dev(lut, palette, out, scratch)
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (GIF_BINS,) or not lut.is_contiguous():
        raise RuntimeError("gif_dither: lut must be contiguous uint8 (32768,)")
    if palette.dtype != torch.uint8 or tuple(palette.shape) != (256, 3) or not palette.is_contiguous():
        raise RuntimeError("gif_dither: palette must be contiguous uint8 (256, 3)")
    if out is None:
        out = torch.empty((n, H, W), device=frames.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W) or not out.is_contiguous():
        raise RuntimeError(f"gif_dither: out must be contiguous uint8 ({n}, {H}, {W})")
    if scratch is None:
        scratch = torch.empty((max(4, gif_dither_scratch_bytes(n, H, W)),), device=frames.device, dtype=torch.uint8)
    if scratch.dtype != torch.uint8 or scratch.dim() != 1 or not scratch.is_contiguous():
        raise RuntimeError("gif_dither: scratch must be contiguous uint8 (bytes,)")
    _check(lib().mmgt_gif_dither(_ptr(frames), _ptr(lut), _ptr(palette), _ptr(out), _ptr(scratch), scratch.numel(), n, H, W, _stream()),
           "mmgt_gif_dither")
    return out


def gif_delta(idx, prev=None, out=None):
    """Frame differencing of an index map (n, H, W) uint8: 255 where a pixel equals the frame before, else the index.  Frame 0 is compared with
    `prev` (H, W), the last frame of the part of the clip before this one, or copied if there is none."""
    _dev(idx, prev, out)
    if idx.dtype != torch.uint8 or idx.dim() != 3 or not idx.is_contiguous():
        raise RuntimeError("gif_delta: idx must be contiguous uint8 (n, H, W)")
    n, H, W = idx.shape
    if prev is not None and (prev.dtype != torch.uint8 or tuple(prev.shape) != (H, W) or not prev.is_contiguous()):
        raise RuntimeError(f"gif_delta: prev must be contiguous uint8 ({H}, {W})")
    if out is None:
        out = torch.empty_like(idx)
    if out.dtype != torch.uint8 or out.shape != idx.shape or not out.is_contiguous():
        raise RuntimeError(f"gif_delta: out must be contiguous uint8 {tuple(idx.shape)}")
    _check(lib().mmgt_gif_delta(_ptr(idx), _ptr(prev), _ptr(out), n, H, W, _stream()), "mmgt_gif_delta")
    return out


def gif_strip_stride(W, strip_rows):
    """Bytes that the LZW bit string of one strip of `strip_rows` rows cannot exceed, whatever the indices (csrc/gif.hip states the bound)."""
    v = c_long(0)
    _check(lib().mmgt_gif_strip_stride(int(W), int(strip_rows), ctypes.byref(v)), "mmgt_gif_strip_stride")
    return v.value


def gif_packed_stride(strips, out_stride):
    """Bytes that one frame's data sub-blocks cannot exceed: its slots' bytes, a length byte per 255 of them and the terminator, rounded up to 16."""
    b = int(strips) * int(out_stride)
    return (b + -(-b // 255) + 1 + 15) // 16 * 16


def gif_lzw(idx, strip_rows, out=None):
    """idx (n, H, W) uint8 -> (out (n * strips, stride) uint8, bits (n, strips) int64): the LZW bit string of every (frame, strip), LSB-first, and
    its length; only the first ceil(bits / 32) words of a row of `out` are written.  `out` = (out, bits) to write into."""
    _dev(idx)
    if idx.dtype != torch.uint8 or idx.dim() != 3 or not idx.is_contiguous():
        raise RuntimeError("gif_lzw: idx must be contiguous uint8 (n, H, W)")
    n, H, W = idx.shape
    stride = gif_strip_stride(W, strip_rows)
    strips = -(-H // int(strip_rows))
    if out is None:
        out = (torch.empty((n * strips, stride), device=idx.device, dtype=torch.uint8),
               torch.empty((n, strips), device=idx.device, dtype=torch.int64))
    slots, bits = out
    assert slots.dim() == 2 and slots.shape[0] == n * strips and slots.dtype == torch.uint8 and slots.stride(1) == 1
    assert bits.shape == (n, strips) and bits.dtype == torch.int64 and bits.is_contiguous()
    _check(lib().mmgt_gif_lzw(_ptr(idx), _ptr(slots), _ptr(bits), n, H, W, int(strip_rows), slots.stride(0), _stream()), "mmgt_gif_lzw")
    return slots, bits


def gif_pack(slots, bits, out=None):
    """The strips of gif_lzw -> (packed (n, packed_stride) uint8, sizes (n,) int32): frame f's GIF data sub-blocks with their 0x00 terminator are
    packed[f, :sizes[f]].  `out` = (packed, sizes) to write into."""
    _dev(slots, bits)
    n, strips = bits.shape
    if out is None:
        out = (torch.empty((n, gif_packed_stride(strips, slots.stride(0))), device=slots.device, dtype=torch.uint8),
               torch.empty((n,), device=slots.device, dtype=torch.int32))
    packed, sizes = out
    assert packed.dim() == 2 and packed.shape[0] == n and packed.dtype == torch.uint8 and packed.stride(1) == 1
    assert sizes.shape == (n,) and sizes.dtype == torch.int32
    _check(lib().mmgt_gif_pack(_ptr(slots), _ptr(bits), _ptr(packed), _ptr(sizes), n, strips, slots.stride(0), packed.stride(0), _stream()),
           "mmgt_gif_pack")
    return packed, sizes


# ------------------------------------------------------------------------------------------------------------ PNG (csrc/png.hip)

PNG_SYMS = 286
PNG_HEADER_BYTES = 576              # MMGT_PNG_HEADER_BYTES: room for the longest dynamic-Huffman block header


def png_filter(frames, out=None):
    """(n, H, W, 3) uint8 RGB -> (filt (n, H, 1 + 3 W) uint8, sums (n, H, 2) int64): every scanline's filter type byte and filtered bytes, and the
    two sums of which the host makes the row's Adler-32 (see mmgt_png_filter).  `out` = (filt, sums) to write into."""
    n, H, W = _rgb_frames(frames, "png_filter")
    if out is None:
        out = (torch.empty((n, H, 1 + 3 * W), device=frames.device, dtype=torch.uint8),
               torch.empty((n, H, 2), device=frames.device, dtype=torch.int64))
    filt, sums = out
    assert filt.shape == (n, H, 1 + 3 * W) and filt.dtype == torch.uint8 and filt.is_contiguous()
    assert sums.shape == (n, H, 2) and sums.dtype == torch.int64 and sums.is_contiguous()
    _check(lib().mmgt_png_filter(_ptr(frames), _ptr(filt), _ptr(sums), n, H, W, _stream()), "mmgt_png_filter")
    return filt, sums


def _png_data(data, strip_bytes, what):
    _dev(data)
    if data.dtype != torch.uint8 or data.dim() != 2 or not data.is_contiguous() or data.shape[0] < 1 or data.shape[1] < 1 or int(strip_bytes) < 1:
        raise RuntimeError(f"{what}: data must be contiguous uint8 (n, frame_bytes), strip_bytes at least 1")
    n, frame_bytes = data.shape
    return n, frame_bytes, -(-frame_bytes // int(strip_bytes))


def png_histogram(data, strip_bytes, out=None):
    """data (n, frame_bytes) uint8, any bytes -> (n, strips, 286): how often each literal/length symbol occurs in the tokens of every strip of
    strip_bytes bytes (see mmgt_png_histogram).  The counts are uint32 held in an int32 tensor."""
    n, frame_bytes, strips = _png_data(data, strip_bytes, "png_histogram")
    if out is None:
        out = torch.empty((n, strips, PNG_SYMS), device=data.device, dtype=torch.int32)
    assert out.shape == (n, strips, PNG_SYMS) and out.dtype == torch.int32 and out.is_contiguous()
    _check(lib().mmgt_png_histogram(_ptr(data), _ptr(out), n, frame_bytes, int(strip_bytes), _stream()), "mmgt_png_histogram")
    return out


def _slot_offsets(want_bits):
    """Bit counts, one per slot -> word offsets (slots + 1,) int64 of slots that hold them, each a whole number of 32-bit words."""
    import numpy as np
    w = np.asarray(want_bits, np.int64).reshape(-1)
    return np.concatenate([[0], np.cumsum((w + 31) // 32)]).astype(np.int64)


def _pack_slots(slots, want_bits, out):
    """Slots laid out by _slot_offsets(want_bits), want_bits (n, k) -> (packed (bytes,) uint8, out_off (n + 1,) host int64): frame f's k slots joined
    bit by bit and padded with zero bits to a byte are packed[out_off[f]:out_off[f + 1]] (mmgt_png_pack)."""
    import numpy as np
    _dev(slots)
    w = np.asarray(want_bits, np.int64)
    n, k = w.shape
    off = _slot_offsets(w)
    bit_off = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(w, axis=1)], axis=1)
    out_off = np.concatenate([[0], np.cumsum((bit_off[:, -1] + 7) // 8)]).astype(np.int64)
    if out is None:
        out = torch.empty((int(out_off[-1]),), device=slots.device, dtype=torch.uint8)
    assert slots.dim() == 1 and slots.numel() >= int(off[-1]) and slots.dtype == torch.int32 and slots.is_contiguous()
    assert out.dim() == 1 and out.numel() >= int(out_off[-1]) and out.dtype == torch.uint8 and out.is_contiguous()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(slots.device)
    for f0 in range(0, n, 65535):                                  # the launch's grid holds a frame per y index
        f1 = min(n, f0 + 65535)
        d_off, d_bit, d_out = up(off[f0 * k:f1 * k + 1]), up(bit_off[f0:f1]), up(out_off[f0:f1 + 1])                                # alive until launched
        _check(lib().mmgt_png_pack(_ptr(slots), _ptr(d_off), slots.numel(), _ptr(d_bit), _ptr(out), _ptr(d_out), out.numel(), f1 - f0, k,
                                   _stream()), "mmgt_png_pack")
    return out, out_off


def png_slot_offsets(want_bits):
    """Exact bit counts (n, strips) -> word offsets (n * strips + 1,) int64 of slots that hold them, each a whole number of 32-bit words."""
    import numpy as np
    w = np.asarray(want_bits, np.int64)
    if w.size == 0 or (w < 1).any():
        raise RuntimeError("png: every strip holds at least one bit")
    return _slot_offsets(w)


def png_deflate(data, strip_bytes, codes, headers, header_bits, want_bits, out=None):
    """Codes every strip of data (n, frame_bytes) into its slot: host arrays codes (n, strips, 286) uint32, headers (n, strips, PNG_HEADER_BYTES)
    uint8, header_bits (n, strips) int32 and want_bits (n, strips) int64, the bit count of each strip that sizes and places its slot
    (png_slot_offsets) -> (slots (words,) int32, bits (n, strips) int64 as the device counted them).  `out` = (slots, bits) to write into."""
    import numpy as np
    n, frame_bytes, strips = _png_data(data, strip_bytes, "png_deflate")
    codes, headers = np.ascontiguousarray(codes, np.uint32), np.ascontiguousarray(headers, np.uint8)
    header_bits, off = np.ascontiguousarray(header_bits, np.int32), png_slot_offsets(want_bits)
    if codes.shape != (n, strips, PNG_SYMS) or headers.shape != (n, strips, PNG_HEADER_BYTES) or header_bits.shape != (n, strips) or \
            off.size != n * strips + 1 or header_bits.min() < 0 or header_bits.max() > 8 * PNG_HEADER_BYTES:
        raise RuntimeError(f"png_deflate: tables do not match {n} x {strips} strips")
    up = lambda a, dt: torch.from_numpy(a.view(dt)).to(data.device)
    if out is None:
        out = (torch.empty((int(off[-1]),), device=data.device, dtype=torch.int32),
               torch.empty((n, strips), device=data.device, dtype=torch.int64))
    slots, bits = out
    assert slots.dim() == 1 and slots.numel() >= int(off[-1]) and slots.dtype == torch.int32 and slots.is_contiguous()
    assert bits.shape == (n, strips) and bits.dtype == torch.int64 and bits.is_contiguous()
    codes, headers, header_bits, off = up(codes, np.int32), up(headers, np.uint8), up(header_bits, np.int32), up(off, np.int64)    # alive until launched
    _check(lib().mmgt_png_deflate(_ptr(data), _ptr(codes), _ptr(headers), _ptr(header_bits), _ptr(slots), _ptr(off), slots.numel(), _ptr(bits), n,
                                  frame_bytes, int(strip_bytes), _stream()), "mmgt_png_deflate")
    return slots, bits


def png_pack(slots, want_bits, out=None):
    """The slots of png_deflate, laid out by the same want_bits (n, strips) -> (packed (bytes,) uint8, out_off (n + 1,) host int64): frame f's
    deflate stream, its strips joined bit by bit, is packed[out_off[f]:out_off[f + 1]].  `out` = packed to write into."""
    png_slot_offsets(want_bits)                                    # PNG's rule for the counts
    return _pack_slots(slots, want_bits, out)


# ------------------------------------------------------------------------------------------------------------ WebP lossless (csrc/webp.hip)

WEBP_PREDICTOR_BITS = 4             # WP_PREDICTOR_BITS: blocks of 16 x 16 pixels choose a predictor mode
WEBP_HIST_WORDS = 793               # MMGT_WEBP_HIST_WORDS: green + length [280], red [256], blue [256], matches
WEBP_CODE_WORDS = 792               # a frame's code tables: green + length, red, blue


def webp_predict(frames, out=None):
    """(n, H, W, 3) uint8 RGB -> (modes (n, bh, bw) uint8, res (n, H, W) int32): every 16 x 16 block's predictor mode and the residuals as ARGB
    words (see mmgt_webp_predict).  `out` = (modes, res) to write into."""
    n, H, W = _rgb_frames(frames, "webp_predict")
    B = 1 << WEBP_PREDICTOR_BITS
    bh, bw = -(-H // B), -(-W // B)
    if out is None:
        out = (torch.empty((n, bh, bw), device=frames.device, dtype=torch.uint8), torch.empty((n, H, W), device=frames.device, dtype=torch.int32))
    modes, res = out
    assert modes.shape == (n, bh, bw) and modes.dtype == torch.uint8 and modes.is_contiguous()
    assert res.shape == (n, H, W) and res.dtype == torch.int32 and res.is_contiguous()
    _check(lib().mmgt_webp_predict(_ptr(frames), _ptr(modes), _ptr(res), n, H, W, _stream()), "mmgt_webp_predict")
    return modes, res


def _webp_data(data, strip_px, what):
    _dev(data)
    if data.dtype != torch.int32 or data.dim() != 2 or not data.is_contiguous() or data.shape[0] < 1 or data.shape[1] < 1 or int(strip_px) < 1:
        raise RuntimeError(f"{what}: data must be contiguous int32 (n, frame_px), strip_px at least 1")
    n, frame_px = data.shape
    return n, frame_px, -(-frame_px // int(strip_px))


def webp_histogram(data, strip_px, out=None):
    """data (n, frame_px) int32, any words -> (n, strips, 793): how often each green / length, red and blue symbol occurs in the tokens of every
    strip of strip_px pixels, and its matches (see mmgt_webp_histogram).  The counts are uint32 held in an int32 tensor."""
    n, frame_px, strips = _webp_data(data, strip_px, "webp_histogram")
    if out is None:
        out = torch.empty((n, strips, WEBP_HIST_WORDS), device=data.device, dtype=torch.int32)
    assert out.shape == (n, strips, WEBP_HIST_WORDS) and out.dtype == torch.int32 and out.is_contiguous()
    _check(lib().mmgt_webp_histogram(_ptr(data), _ptr(out), n, frame_px, int(strip_px), _stream()), "mmgt_webp_histogram")
    return out


def webp_slot_offsets(want_bits):
    """Exact bit counts (n, 1 + strips), a frame's header first -> word offsets (n * (1 + strips) + 1,) int64 of slots that hold them, each a whole
    number of 32-bit words.  A strip may hold no bit at all (every symbol the only one of its alphabet); a header never does."""
    import numpy as np
    w = np.asarray(want_bits, np.int64)
    if w.ndim != 2 or w.shape[1] < 2 or w.shape[0] < 1 or (w < 0).any() or (w[:, 0] < 1).any():
        raise RuntimeError("webp: bit counts are (n, 1 + strips), none negative, every header at least one bit")
    return _slot_offsets(w)


def webp_code(data, strip_px, codes, headers, want_bits, out=None):
    """Codes every strip of data (n, frame_px) into its slot and copies the frames' headers into theirs: host arrays codes (n, 792) uint32, headers =
    n byte strings (a frame's header bits, LSB-first) and want_bits (n, 1 + strips) int64, the bit count of each header and strip that sizes and
    places its slot (webp_slot_offsets) -> (slots (words,) int32, bits (n, strips) int64 as the device counted them).  `out` = (slots, bits)."""
    import numpy as np
    n, frame_px, strips = _webp_data(data, strip_px, "webp_code")
    codes, want = np.ascontiguousarray(codes, np.uint32), np.asarray(want_bits, np.int64)
    if codes.shape != (n, WEBP_CODE_WORDS) or want.shape != (n, strips + 1) or len(headers) != n:
        raise RuntimeError(f"webp_code: tables do not match {n} x {strips} strips")
    off = webp_slot_offsets(want)
    hwords = (want[:, 0] + 31) // 32
    if any(len(h) > 4 * int(k) for h, k in zip(headers, hwords)):
        raise RuntimeError("webp_code: a header is longer than its bit count")
    hoff = np.concatenate([[0], np.cumsum(hwords)]).astype(np.int64)
    hbuf = np.zeros(4 * int(hoff[-1]), np.uint8)
    for f, h in enumerate(headers):
        hbuf[4 * hoff[f]:4 * hoff[f] + len(h)] = np.frombuffer(h, np.uint8)
    up = lambda a, dt: torch.from_numpy(a.view(dt)).to(data.device)
    if out is None:
        out = (torch.empty((max(1, int(off[-1])),), device=data.device, dtype=torch.int32),
               torch.empty((n, strips), device=data.device, dtype=torch.int64))
    slots, bits = out
    assert slots.dim() == 1 and slots.numel() >= int(off[-1]) and slots.dtype == torch.int32 and slots.is_contiguous()
    assert bits.shape == (n, strips) and bits.dtype == torch.int64 and bits.is_contiguous()
    codes, hbuf, d_hoff, d_off = up(codes, np.int32), up(hbuf, np.int32), up(hoff, np.int64), up(off, np.int64)      # alive until launched
    _check(lib().mmgt_webp_code(_ptr(data), _ptr(codes), _ptr(hbuf), _ptr(d_hoff), hbuf.numel(), _ptr(slots), _ptr(d_off), slots.numel(), _ptr(bits),
                                n, frame_px, int(strip_px), _stream()), "mmgt_webp_code")
    return slots, bits


def webp_pack(slots, want_bits, out=None):
    """The slots of webp_code, laid out by the same want_bits (n, 1 + strips) -> (packed (bytes,) uint8, out_off (n + 1,) host int64): frame f's VP8L
    payload, its header and strips joined bit by bit and padded with zero bits to a byte, is packed[out_off[f]:out_off[f + 1]].  The join is
    mmgt_png_pack's, with the header as one more slot.  `out` = packed to write into."""
    webp_slot_offsets(want_bits)                                   # WebP's rule for the counts
    return _pack_slots(slots, want_bits, out)


# ------------------------------------------------------------------------------------------------------------ WebP lossy (csrc/vp8.hip)

VP8_MAX_SIDE = 16383                # V8_MAX_SIDE: the frame header's 14-bit sizes
VP8_MB_BLOCKS = 25                  # a macroblock's blocks of 16 levels: 16 luma, 4 U, 4 V, Y2


def vp8_quantiser(quality):
    """quality 0 .. 100 -> (the quantiser index 0 .. 127, the default loop filter level of that index) (see mmgt_vp8_quantiser)."""
    q, level = c_int(0), c_int(0)
    _check(lib().mmgt_vp8_quantiser(int(quality), ctypes.byref(q), ctypes.byref(level)), "mmgt_vp8_quantiser")
    return q.value, level.value


def vp8_slot_bytes(H, W, partitions):
    """(worst-case bytes of a first partition, of a token partition) of an H x W frame (see mmgt_vp8_slot_bytes)."""
    first, token = ctypes.c_longlong(0), ctypes.c_longlong(0)
    _check(lib().mmgt_vp8_slot_bytes(int(H), int(W), int(partitions), ctypes.byref(first), ctypes.byref(token)), "mmgt_vp8_slot_bytes")
    return first.value, token.value


def _vp8_planes(n, H, W, device):
    mbh, mbw = -(-H // 16), -(-W // 16)
    return tuple(torch.empty((n, s * mbh, s * mbw), device=device, dtype=torch.uint8) for s in (16, 8, 8))


def _vp8_check_planes(planes, n, H, W, what):
    mbh, mbw = -(-H // 16), -(-W // 16)
    _dev(*planes)
    for p, s in zip(planes, (16, 8, 8)):
        if p.shape != (n, s * mbh, s * mbw) or p.dtype != torch.uint8 or not p.is_contiguous():
            raise RuntimeError(f"{what}: planes must be contiguous uint8 ({n}, 16 mbh, 16 mbw), ({n}, 8 mbh, 8 mbw) twice")


def vp8_convert(frames, out=None):
    """(n, H, W, 3) uint8 RGB -> (Y, U, V) of the frames padded to whole macroblocks (see mmgt_vp8_convert).  `out` = the planes to write into."""
    n, H, W = _rgb_frames(frames, "vp8_convert")
    if out is None:
        out = _vp8_planes(n, H, W, frames.device)
    if min(n, H, W) >= 1 and max(H, W) <= VP8_MAX_SIDE:
        _vp8_check_planes(out, n, H, W, "vp8_convert")
    _check(lib().mmgt_vp8_convert(_ptr(frames), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), n, H, W, _stream()), "mmgt_vp8_convert")
    return out


def vp8_analyse(planes, H, W, q, out=None):
    """The planes of vp8_convert -> (recon (Y, U, V), levels (n, mbh, mbw, 25, 16) int16, modes (n, mbh, mbw, 2) uint8, nz (n, mbh, mbw) int32 masks,
    skipped (n,) int32) (see mmgt_vp8_analyse).  `out` = the same tuple to write into."""
    n, H, W = planes[0].shape[0], int(H), int(W)
    _vp8_check_planes(planes, n, H, W, "vp8_analyse")
    mbh, mbw = -(-H // 16), -(-W // 16)
    dev = planes[0].device
    if out is None:
        out = (_vp8_planes(n, H, W, dev), torch.empty((n, mbh, mbw, VP8_MB_BLOCKS, 16), device=dev, dtype=torch.int16),
               torch.empty((n, mbh, mbw, 2), device=dev, dtype=torch.uint8), torch.empty((n, mbh, mbw), device=dev, dtype=torch.int32),
               torch.empty((n,), device=dev, dtype=torch.int32))
    recon, levels, modes, nz, skipped = out
    _vp8_check_planes(recon, n, H, W, "vp8_analyse")
    assert levels.shape == (n, mbh, mbw, VP8_MB_BLOCKS, 16) and levels.dtype == torch.int16 and levels.is_contiguous()
    assert modes.shape == (n, mbh, mbw, 2) and modes.dtype == torch.uint8 and modes.is_contiguous()
    assert nz.shape == (n, mbh, mbw) and nz.dtype == torch.int32 and nz.is_contiguous()
    assert skipped.shape == (n,) and skipped.dtype == torch.int32 and skipped.is_contiguous()
    _check(lib().mmgt_vp8_analyse(_ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), _ptr(recon[0]), _ptr(recon[1]), _ptr(recon[2]), _ptr(levels),
                                  _ptr(modes), _ptr(nz), _ptr(skipped), n, H, W, int(q), _stream()), "mmgt_vp8_analyse")
    return out


def vp8_code(levels, nz, modes, skipped, H, W, q, partitions, filter_level, out=None):
    """The outputs of vp8_analyse -> (slots (bytes,) uint8, counts (n, 1 + partitions) int64): every partition coded into its worst-case slot and its
    byte count (see mmgt_vp8_code and vp8_slot_bytes for the layout).  `out` = (slots, counts) to write into."""
    _dev(levels, nz, modes, skipped)
    n, H, W, partitions = levels.shape[0], int(H), int(W), int(partitions)
    per_frame = 1
    if partitions in (1, 2, 4, 8) and min(H, W) >= 1 and max(H, W) <= VP8_MAX_SIDE:
        first, token = vp8_slot_bytes(H, W, partitions)
        per_frame = first + partitions * token
    if out is None:
        out = (torch.empty((n * per_frame,), device=levels.device, dtype=torch.uint8),
               torch.empty((n, 1 + max(1, partitions)), device=levels.device, dtype=torch.int64))
    slots, counts = out
    assert slots.dim() == 1 and slots.dtype == torch.uint8 and slots.is_contiguous()
    assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= n * (1 + max(1, partitions))
    _check(lib().mmgt_vp8_code(_ptr(levels), _ptr(nz), _ptr(modes), _ptr(skipped), _ptr(slots), slots.numel(), _ptr(counts), n, H, W, int(q),
                               partitions, int(filter_level), _stream()), "mmgt_vp8_code")
    return slots, counts


def vp8_pack(slots, counts, H, W, partitions, out=None):
    """The slots and counts of vp8_code -> (packed (bytes,) uint8, out_off (n + 1,) host int64): frame f's 'VP8 ' payload is
    packed[out_off[f]:out_off[f + 1]] (see mmgt_vp8_pack).  The counts are read back to place the frames.  `out` = packed to write into."""
    import numpy as np
    _dev(slots, counts)
    partitions = int(partitions)
    c = counts.cpu().numpy()
    n = c.shape[0]
    if (c < 0).any():
        raise RuntimeError(f"vp8_pack: partition {tuple(np.argwhere(c < 0)[0])} did not fit its slot (mmgt_vp8_code)")
    if (c[:, 0] >= 1 << 19).any():
        raise RuntimeError(f"vp8_pack: a first partition of {int(c[:, 0].max())} bytes passes the frame tag's 19 bits")
    out_off = np.concatenate([[0], np.cumsum(10 + 3 * (partitions - 1) + c.sum(1))]).astype(np.int64)
    if out is None:
        out = torch.empty((int(out_off[-1]),), device=slots.device, dtype=torch.uint8)
    assert out.dim() == 1 and out.numel() >= int(out_off[-1]) and out.dtype == torch.uint8 and out.is_contiguous()
    d_off = torch.from_numpy(out_off).to(slots.device)                                                                              # alive until launched
    _check(lib().mmgt_vp8_pack(_ptr(slots), slots.numel(), _ptr(counts), _ptr(out), _ptr(d_off), out.numel(), n, int(H), int(W), partitions,
                               _stream()), "mmgt_vp8_pack")
    return out, out_off


# ------------------------------------------------------------------------------------------------------------ PNG input (csrc/pngdec.hip)

_PNGDEC_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def pngdec_stride(W, colour_type, depth):
    """Bytes of one filtered scanline: the filter type byte and ceil(W * bits per pixel / 8)."""
    if colour_type not in _PNGDEC_CHANNELS:
        raise RuntimeError(f"pngdec: colour type {colour_type} is outside the range (0, 2, 3, 4, 6)")
    return 1 + (int(W) * _PNGDEC_CHANNELS[colour_type] * int(depth) + 7) // 8


def _status_words(status, n, device, what):
    if status is None:
        status = torch.empty((n,), device=device, dtype=torch.int32)
    if status.dtype != torch.int32 or tuple(status.shape) != (n,) or not status.is_contiguous() or status.device != device:
        raise RuntimeError(f"{what}: status must be contiguous int32 ({n},) on {device}")
    return status


def png_inflate(data, offsets, frame_bytes, out=None):
    """Raw deflate streams data[offsets[f]:offsets[f + 1]] (data uint8, a multiple of 16 bytes; offsets int64 (n + 1,)) -> (filt (n, frame_bytes)
    uint8, status (n,) int32): include/mmgt_hip.h states the operands.  `out` = (filt, status) to write into, either may be None."""
    _dev(data, offsets)
    n = offsets.numel() - 1
    if (data.dtype != torch.uint8 or data.dim() != 1 or offsets.dtype != torch.int64 or offsets.dim() != 1 or n < 1
            or not data.is_contiguous() or not offsets.is_contiguous()):
        raise RuntimeError("png_inflate: expected data uint8 (bytes,) and offsets int64 (n + 1,), n >= 1, both contiguous")
    filt, status = out if out is not None else (None, None)
    if filt is None:
        filt = torch.empty((n, int(frame_bytes)), device=data.device, dtype=torch.uint8)
    if filt.dtype != torch.uint8 or tuple(filt.shape) != (n, int(frame_bytes)) or not filt.is_contiguous() or filt.device != data.device:
        raise RuntimeError(f"png_inflate: filt must be contiguous uint8 ({n}, {int(frame_bytes)}) on {data.device}")
    status = _status_words(status, n, data.device, "png_inflate")
    _check(lib().mmgt_png_inflate(_ptr(data), data.numel(), _ptr(offsets), _ptr(filt), _ptr(status), n, int(frame_bytes), _stream()), "mmgt_png_inflate")
    return filt, status


def png_unfilter(filt, H, W, colour_type, depth, out=None):
    """Filtered scanlines (n, H * stride) uint8, reconstructed IN PLACE -> (sums (n, H, 2) int64, status (n,) int32): the two sums of which the
    host makes each row's Adler-32, over the bytes as they were (see mmgt_png_unfilter).  `out` = (sums, status) to write into, either may be None."""
    _dev(filt)
    H, W = int(H), int(W)
    stride = pngdec_stride(W, colour_type, depth)
    n = filt.shape[0]
    if filt.dtype != torch.uint8 or tuple(filt.shape) != (n, H * stride) or not filt.is_contiguous() or n < 1:
        raise RuntimeError(f"png_unfilter: expected filt uint8 (n, {H * stride}), contiguous")
    sums, status = out if out is not None else (None, None)
    if sums is None:
        sums = torch.empty((n, H, 2), device=filt.device, dtype=torch.int64)
    if sums.dtype != torch.int64 or tuple(sums.shape) != (n, H, 2) or not sums.is_contiguous() or sums.device != filt.device:
        raise RuntimeError(f"png_unfilter: sums must be contiguous int64 ({n}, {H}, 2) on {filt.device}")
    status = _status_words(status, n, filt.device, "png_unfilter")
    _check(lib().mmgt_png_unfilter(_ptr(filt), _ptr(sums), _ptr(status), n, H, W, int(colour_type), int(depth), _stream()), "mmgt_png_unfilter")
    return sums, status


def png_expand(filt, H, W, colour_type, depth, palette=None, plte_len=None, out=None):
    """Reconstructed scanlines (n, H * stride) -> (pixels (n, H, W, 3) uint8 RGB, status (n,) int32); colour type 3 takes palette (n, 256, 3) uint8 and
    plte_len (n,) int32.  `out` = (pixels, status) to write into, either may be None."""
    _dev(filt, palette, plte_len)
    H, W = int(H), int(W)
    stride = pngdec_stride(W, colour_type, depth)
    n = filt.shape[0]
    if filt.dtype != torch.uint8 or tuple(filt.shape) != (n, H * stride) or not filt.is_contiguous() or n < 1:
        raise RuntimeError(f"png_expand: expected filt uint8 (n, {H * stride}), contiguous")
    if int(colour_type) == 3 and (palette is None or plte_len is None or palette.dtype != torch.uint8 or tuple(palette.shape) != (n, 256, 3)
                                  or plte_len.dtype != torch.int32 or tuple(plte_len.shape) != (n,) or not palette.is_contiguous()
                                  or not plte_len.is_contiguous()):
        raise RuntimeError(f"png_expand: colour type 3 needs palette uint8 ({n}, 256, 3) and plte_len int32 ({n},), contiguous")
    pixels, status = out if out is not None else (None, None)
    if pixels is None:
        pixels = torch.empty((n, H, W, 3), device=filt.device, dtype=torch.uint8)
    if pixels.dtype != torch.uint8 or tuple(pixels.shape) != (n, H, W, 3) or not pixels.is_contiguous() or pixels.device != filt.device:
        raise RuntimeError(f"png_expand: out must be contiguous uint8 ({n}, {H}, {W}, 3) on {filt.device}")
    status = _status_words(status, n, filt.device, "png_expand")
    _check(lib().mmgt_png_expand(_ptr(filt), _ptr(palette), _ptr(plte_len), _ptr(pixels), _ptr(status), n, H, W, int(colour_type), int(depth),
                                 _stream()), "mmgt_png_expand")
    return pixels, status


# ------------------------------------------------------------------------------------------------------------ GIF input (csrc/gifdec.hip)

GIFDEC_TAB = 16                     # long long words per frame row (csrc/gifdec_core.h: GD_TAB)


def _gif_tab(tab, what):
    if tab.dtype != torch.int64 or tab.dim() != 2 or tab.shape[1] != GIFDEC_TAB or tab.shape[0] < 1 or not tab.is_contiguous():
        raise RuntimeError(f"{what}: expected tab int64 (n, {GIFDEC_TAB}), n >= 1, contiguous")
    return tab.shape[0]


def gif_unlzw(data, tab, idx_bytes, out=None):
    """The LZW code streams of n frames (data uint8, a multiple of 16 bytes; tab int64 (n, 16), one row per frame: include/mmgt_hip.h) -> (idx
    (idx_bytes,) uint8: every frame's palette indices in stream order at its row's offset, status (n,) int32).  `out` = (idx, status) to write into,
    either may be None."""
    _dev(data, tab)
    n = _gif_tab(tab, "gif_unlzw")
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise RuntimeError("gif_unlzw: expected data uint8 (bytes,), contiguous")
    idx, status = out if out is not None else (None, None)
    if idx is None:
        idx = torch.empty((int(idx_bytes),), device=data.device, dtype=torch.uint8)
    if idx.dtype != torch.uint8 or tuple(idx.shape) != (int(idx_bytes),) or not idx.is_contiguous() or idx.device != data.device:
        raise RuntimeError(f"gif_unlzw: idx must be contiguous uint8 ({int(idx_bytes)},) on {data.device}")
    status = _status_words(status, n, data.device, "gif_unlzw")
    _check(lib().mmgt_gif_unlzw(_ptr(data), data.numel(), _ptr(tab), _ptr(idx), idx.numel(), _ptr(status), n, _stream()), "mmgt_gif_unlzw")
    return idx, status


def gif_compose(tab, idx, palette, carry, H, W, out=None):
    """The chunk's frames composed on the H x W canvas: tab int64 (n, 16), idx uint8 (bytes,) as gif_unlzw wrote it, palette uint8 (n, 256, 3), carry
    uint8 (2, H, W, 3) (read unless tab[0] is the file's first frame, written at the end) -> (n, H, W, 3) uint8 RGB.  `out`: a tensor to write into."""
    _dev(tab, idx, palette, carry)
    n, H, W = _gif_tab(tab, "gif_compose"), int(H), int(W)
    if idx.dtype != torch.uint8 or idx.dim() != 1 or not idx.is_contiguous():
        raise RuntimeError("gif_compose: expected idx uint8 (bytes,), contiguous")
    if palette.dtype != torch.uint8 or tuple(palette.shape) != (n, 256, 3) or not palette.is_contiguous():
        raise RuntimeError(f"gif_compose: expected palette uint8 ({n}, 256, 3), contiguous")
    if carry.dtype != torch.uint8 or tuple(carry.shape) != (2, H, W, 3) or not carry.is_contiguous():
        raise RuntimeError(f"gif_compose: expected carry uint8 (2, {H}, {W}, 3), contiguous")
    if out is None:
        out = torch.empty((n, H, W, 3), device=idx.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous() or out.device != idx.device:
        raise RuntimeError(f"gif_compose: out must be contiguous uint8 ({n}, {H}, {W}, 3) on {idx.device}")
    _check(lib().mmgt_gif_compose(_ptr(tab), _ptr(idx), idx.numel(), _ptr(palette), _ptr(carry), _ptr(out), n, H, W, _stream()), "mmgt_gif_compose")
    return out


# ------------------------------------------------------------------------------------------------------------ WebP lossless input (csrc/webpdec.hip)

WEBPDEC_TAB = 16                    # long long words per frame row (csrc/webpdec_core.h: WD_TAB)
WEBPDEC_GROUP_WORDS = 14768 // 4    # scratch words of one prefix-code group (csrc/webpdec_core.h: sizeof(WdGroup) / 4)


def _webp_tab(tab, what):
    if tab.dtype != torch.int64 or tab.dim() != 2 or tab.shape[1] != WEBPDEC_TAB or tab.shape[0] < 1 or not tab.is_contiguous():
        raise RuntimeError(f"{what}: expected tab int64 (n, {WEBPDEC_TAB}), n >= 1, contiguous")
    return tab.shape[0]


def _webp_words(t, name, what):
    if t.dtype != torch.int32 or t.dim() != 1 or t.numel() < 1 or not t.is_contiguous():
        raise RuntimeError(f"{what}: expected {name} int32 (words,), contiguous")


def webp_decode(data, tab, scratch, out=None):
    """The VP8L streams of n frames (data uint8, a multiple of 16 bytes; tab int64 (n, 16), one row per frame: include/mmgt_hip.h) -> every frame's
    scratch words (header block, sub-images, entropy-coded main image) in scratch int32 (words,) at its row's offset, and status (n,) int32, which
    is returned (negative: minus the scratch words the frame needs for its prefix-code groups).  `out`: the status tensor to write into."""
    _dev(data, tab, scratch)
    n = _webp_tab(tab, "webp_decode")
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise RuntimeError("webp_decode: expected data uint8 (bytes,), contiguous")
    _webp_words(scratch, "scratch", "webp_decode")
    status = _status_words(out, n, data.device, "webp_decode")
    _check(lib().mmgt_webp_decode(_ptr(data), data.numel(), _ptr(tab), _ptr(scratch), scratch.numel(), _ptr(status), n, _stream()), "mmgt_webp_decode")
    return status


def webp_untransform(tab, scratch, argb_words=None, out=None):
    """Every frame's transforms undone in its own order: scratch as webp_decode left it (it is used up) -> (argb int32 (words,): the ARGB words of
    each frame's own rectangle at its row's offset, status (n,) int32).  `out` = (argb, status) to write into, either may be None; without an argb
    tensor, argb_words says how many words to allocate."""
    _dev(tab, scratch)
    n = _webp_tab(tab, "webp_untransform")
    _webp_words(scratch, "scratch", "webp_untransform")
    argb, status = out if out is not None else (None, None)
    if argb is None:
        argb = torch.empty((int(argb_words),), device=scratch.device, dtype=torch.int32)
    _webp_words(argb, "argb", "webp_untransform")
    status = _status_words(status, n, scratch.device, "webp_untransform")
    _check(lib().mmgt_webp_untransform(_ptr(tab), _ptr(scratch), scratch.numel(), _ptr(argb), argb.numel(), _ptr(status), n, _stream()),
           "mmgt_webp_untransform")
    return argb, status


def webp_compose(tab, argb, carry, H, W, out=None):
    """The call's frames composed on the H x W canvas: tab int64 (n, 16), argb int32 (words,) as webp_untransform wrote it, carry int32 (H, W), the
    RGBA canvas (read unless tab[0] is its file's first frame, written at the end) -> (n, H, W, 3) uint8 RGB.  `out`: a tensor to write into."""
    _dev(tab, argb, carry)
    n, H, W = _webp_tab(tab, "webp_compose"), int(H), int(W)
    _webp_words(argb, "argb", "webp_compose")
    if carry.dtype != torch.int32 or tuple(carry.shape) != (H, W) or not carry.is_contiguous():
        raise RuntimeError(f"webp_compose: expected carry int32 ({H}, {W}), contiguous")
    if out is None:
        out = torch.empty((n, H, W, 3), device=argb.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous() or out.device != argb.device:
        raise RuntimeError(f"webp_compose: out must be contiguous uint8 ({n}, {H}, {W}, 3) on {argb.device}")
    _check(lib().mmgt_webp_compose(_ptr(tab), _ptr(argb), argb.numel(), _ptr(carry), _ptr(out), n, H, W, _stream()), "mmgt_webp_compose")
    return out


# --------------------------------------------------------------------------------------------------------------- WebP lossy input (csrc/vp8dec.hip)

VP8DEC_TAB = 8                      # long long words per frame row (csrc/vp8dec_core.h: V8D_TAB)


def _vp8dec_tab(tab, what):
    if tab.dtype != torch.int64 or tab.dim() != 2 or tab.shape[1] != VP8DEC_TAB or tab.shape[0] < 1 or not tab.is_contiguous():
        raise RuntimeError(f"{what}: expected tab int64 (n, {VP8DEC_TAB}), n >= 1, contiguous")
    return tab.shape[0]


def vp8dec_parse(data, tab, scratch, out=None):
    """The `VP8 ` payloads of n frames (data uint8, a multiple of 16 bytes; tab int64 (n, 8), one row per frame: include/mmgt_hip.h) -> every
    frame's header block, macroblock modes and dequantised coefficients in scratch int32 (words,) at its row's offset, and status (n,) int32, which
    is returned.  `out`: the status tensor to write into."""
    _dev(data, tab, scratch)
    n = _vp8dec_tab(tab, "vp8dec_parse")
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise RuntimeError("vp8dec_parse: expected data uint8 (bytes,), contiguous")
    _webp_words(scratch, "scratch", "vp8dec_parse")
    status = _status_words(out, n, data.device, "vp8dec_parse")
    _check(lib().mmgt_vp8dec_parse(_ptr(data), data.numel(), _ptr(tab), _ptr(scratch), scratch.numel(), _ptr(status), n, _stream()), "mmgt_vp8dec_parse")
    return status


def vp8dec_reconstruct(tab, scratch, out=None):
    """Every parsed frame's prediction plus residual -> its unfiltered planes in scratch; status (n,) int32 is returned."""
    _dev(tab, scratch)
    n = _vp8dec_tab(tab, "vp8dec_reconstruct")
    _webp_words(scratch, "scratch", "vp8dec_reconstruct")
    status = _status_words(out, n, scratch.device, "vp8dec_reconstruct")
    _check(lib().mmgt_vp8dec_reconstruct(_ptr(tab), _ptr(scratch), scratch.numel(), _ptr(status), n, _stream()), "mmgt_vp8dec_reconstruct")
    return status


def vp8dec_filter(tab, scratch, out=None):
    """Every reconstructed frame's loop filter, in place in scratch; status (n,) int32 is returned."""
    _dev(tab, scratch)
    n = _vp8dec_tab(tab, "vp8dec_filter")
    _webp_words(scratch, "scratch", "vp8dec_filter")
    status = _status_words(out, n, scratch.device, "vp8dec_filter")
    _check(lib().mmgt_vp8dec_filter(_ptr(tab), _ptr(scratch), scratch.numel(), _ptr(status), n, _stream()), "mmgt_vp8dec_filter")
    return status


def vp8dec_output(tab, scratch, argb, max_pixels, out=None):
    """Every frame's planes -> the ARGB words (alpha 255) of its rectangle in argb int32 (words,) at its row's offset, as webp_compose takes them;
    max_pixels: the largest W * H among the rows.  status (n,) int32 is returned."""
    _dev(tab, scratch, argb)
    n = _vp8dec_tab(tab, "vp8dec_output")
    _webp_words(scratch, "scratch", "vp8dec_output")
    _webp_words(argb, "argb", "vp8dec_output")
    status = _status_words(out, n, scratch.device, "vp8dec_output")
    _check(lib().mmgt_vp8dec_output(_ptr(tab), _ptr(scratch), scratch.numel(), _ptr(argb), argb.numel(), _ptr(status), n, int(max_pixels), _stream()),
           "mmgt_vp8dec_output")
    return status


def dwpose_draw(kp, H=512, W=512):
    """SMGA's normalised key points (L, 402) or (L, 134, 3) fp32 -> (pose (L, H, W, 3), hands, lips, face (L, H, W)) uint8: the reference's
    pose_vid_generator frames drawn on the device (see mmgt_dwpose_draw)."""
    _dev(kp)
    kp = kp.reshape(kp.shape[0], 134, 3)
    assert kp.dtype == torch.float32 and kp.is_contiguous()
    L = kp.shape[0]
    pose = torch.empty((L, H, W, 3), device=kp.device, dtype=torch.uint8)
    hands, lips, face = (torch.empty((L, H, W), device=kp.device, dtype=torch.uint8) for _ in range(3))
    _check(lib().mmgt_dwpose_draw(_ptr(kp), _ptr(pose), _ptr(hands), _ptr(lips), _ptr(face), L, H, W, _stream()), "mmgt_dwpose_draw")
    return pose, hands, lips, face


# ----------------------------------------------------------------------------------------------------- audio input

AUDIO_SAMPLE_BYTES = (1, 2, 3, 4, 4, 8)          # csrc/audio_core.h: U8, S16, S24, S32, F32, F64


def audio_decode_mono(raw, n_frames, channels, fmt, out=None):
    """The interleaved little-endian frames at the start of raw uint8 (bytes,) -- a view at any byte offset will do -- as (n_frames,) fp32 mono
    (include/mmgt_hip.h: mmgt_audio_decode_mono).  `out`: the tensor to write into."""
    _dev(raw, out)
    need = int(n_frames) * int(channels) * AUDIO_SAMPLE_BYTES[fmt] if 0 <= fmt < 6 else 0
    if raw.dtype != torch.uint8 or raw.dim() != 1 or not raw.is_contiguous() or raw.numel() < need:
        raise RuntimeError(f"audio_decode_mono: expected raw uint8 (bytes,), contiguous, of at least {need} bytes")
    if out is None:
        out = torch.empty((int(n_frames),), device=raw.device, dtype=torch.float32)
    if _f32(out, "audio_decode_mono: out").shape != (int(n_frames),):
        raise RuntimeError(f"audio_decode_mono: out must hold ({int(n_frames)},) floats")
    _check(lib().mmgt_audio_decode_mono(_ptr(raw), _ptr(out), int(n_frames), int(channels), int(fmt), _stream()), "mmgt_audio_decode_mono")
    return out


def audio_resample(x, taps, up, down, half, out=None):
    """x (n_in,) fp32 through the polyphase FIR whose phase-major table is taps (up * (2 * half // up + 1),) fp32 -> (ceil(n_in * up / down),) fp32
    (include/mmgt_hip.h: mmgt_audio_resample).  `out`: the tensor to write into."""
    _dev(x, taps, out)
    _f32(x, "audio_resample: x"), _f32(taps, "audio_resample: taps")
    n_in = x.numel()
    n_out = -(-n_in * int(up) // int(down))
    if x.dim() != 1 or taps.dim() != 1 or taps.numel() != int(up) * (2 * int(half) // int(up) + 1):
        raise RuntimeError(f"audio_resample: x must be 1-D and taps hold up * (2 * half // up + 1) = {int(up) * (2 * int(half) // int(up) + 1)} floats")
    if out is None:
        out = torch.empty((n_out,), device=x.device, dtype=torch.float32)
    if _f32(out, "audio_resample: out").shape != (n_out,):
        raise RuntimeError(f"audio_resample: out must hold ({n_out},) floats")
    _check(lib().mmgt_audio_resample(_ptr(x), n_in, _ptr(taps), int(up), int(down), int(half), _ptr(out), n_out, _stream()), "mmgt_audio_resample")
    return out
