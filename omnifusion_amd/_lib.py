"""ctypes loader of libomnifusion_hip.so — the ONLY compute path of this package.

There is no CPU / PyTorch fallback: if the HIP library is missing or fails to load,
importing the operators raises (the product path must fail loudly, never silently run
something else).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OMNI_LIB_VARIANT") or os.path.join(_HERE, "csrc", "libomnifusion_hip.so")    # (OMNI_LIB_VARIANT: tools/ only — a variant build of the library for same-box A/B timings)
LIB_PATH_DEBUG = os.path.join(_HERE, "csrc", "libomnifusion_hip_dbg.so")     # tools/ only: ablation switches + micro-benchmarks

OMNI_OK, OMNI_ERR_INVALID, OMNI_ERR_HIP, OMNI_ERR_UNSUPPORTED = 0, 1, 2, 3
LAYOUT_BCHWN, LAYOUT_BNCHW, LAYOUT_BNHWC, LAYOUT_BCHNW = 0, 1, 2, 3
F32, F16 = 0, 1

_lib = None


class OmniLibraryMissing(ImportError):
    pass


# every symbol include/omnifusion.h declares (tests/test_boundary.py parses the header and
# checks this list against it and against the built library)
EXPORTS = [
    "omni_version", "omni_last_error", "omni_set_option", "omni_get_option", "omni_num_patches", "omni_patch_centers",
    "omni_geometry_create", "omni_geometry_destroy", "omni_geometry_cache_clear", "omni_geometry_cache_size",
    "omni_equi2pers", "omni_equi2pers_aux", "omni_pers2equi", "omni_pers2equi_conf", "omni_patches_to_planar",
    "omni_equi2pers_g", "omni_pers2equi_g", "omni_equi2pers_bwd", "omni_pers2equi_bwd",
    "omni_conv2d_nhwc_f32", "omni_stem_f32", "omni_maxpool3x3s2_f32", "omni_upsample_bilinear_f32",
    "omni_add_hw_f32", "omni_add_period_f32", "omni_token_pack_f32", "omni_layernorm512_f32",
    "omni_attention_f32", "omni_heads_f32", "omni_mlp_points_f32",
    "omni_conv2d_nhwc_f16x3_ws", "omni_conv2d_sh_f16x3_ws", "omni_conv2d_sh_f16x3_post_ws", "omni_gemm_rows_sh_f16x3", "omni_gemm_rows_ln_sh_f16x3", "omni_gemm_rows_pack", "omni_conv3x3_up2_sh_f16x3", "omni_conv3x3_up2_heads_sh_f16x3", "omni_conv3x3_up2_heads_sh_f16x1", "omni_up2_heads_scratch_bytes", "omni_heads_pack_f16x3", "omni_sh_from_f32", "omni_sh_to_f32", "omni_sh_overflow",
    "omni_stem_sh", "omni_stem_sh_f16x3", "omni_stem_sh_f16x1", "omni_maxpool3x3s2_sh", "omni_upsample_bilinear_sh", "omni_up2_tapsum_sh", "omni_add_hw_sh", "omni_add_period_sh", "omni_layernorm512_sh", "omni_gemm_sh_f16x3_ln512_ws", "omni_gemm_rows_slices_sh_f16x3", "omni_gemm_rows_ln_parts_sh_f16x3", "omni_splitk_reduce_ln512", "omni_wino_input_sh", "omni_conv3x3_wino_sh_f16x3", "omni_attention_qkv_sh",
    "omni_conv2d_splitk_plan", "omni_conv2d_sh_plan", "omni_conv2d_nhwc_f32_ws",
    "omni_masked_median_f32", "omni_depth_metrics_f32",
    "omni_png_info", "omni_png_decode", "omni_png_decode_batch", "omni_zlib_inflate", "omni_png_checksums",
    "omni_preprocess_rgb_u8", "omni_preprocess_depth_u16", "omni_berhu_workspace_bytes", "omni_berhu_loss_f32", "omni_berhu_grad_f32",
    "omni_pointcloud_ply_f32",
    "omni_dibr_workspace_bytes", "omni_splat_render_f32", "omni_dibr_f32",
    "omni_splat_render_wt_f32", "omni_dibr_wt_f32", "omni_dibr_bwd_workspace_bytes", "omni_splat_render_bwd_f32", "omni_dibr_bwd_f32",
    "omni_ssim_f32", "omni_photometric_workspace_bytes", "omni_photometric_grad_scratch_bytes", "omni_photometric_loss_f32",
    "omni_photometric_grad_f32",
    "omni_freeview_rotations", "omni_freeview_equi2pers_f32", "omni_freeview_pers2equi_f32", "omni_freeview_merge_f32",
    "omni_freeview_bwd_workspace_bytes", "omni_freeview_equi2pers_bwd_f32", "omni_freeview_pers2equi_bwd_f32", "omni_freeview_merge_bwd_f32",
    "omni_semantic_workspace_bytes", "omni_semantic_step_f32", "omni_semantic_grad_f32", "omni_confusion_matrix_i64",
    "omni_depth_normals_f32", "omni_sobel_f32", "omni_l1_workspace_bytes", "omni_l1_loss_f32", "omni_l1_grad_f32",
    "omni_geometry_terms_workspace_bytes", "omni_geometry_terms_f32", "omni_geometry_terms_grad_f32",
    "omni_image_diff_f32", "omni_image_diff_norm_f32", "omni_vertex_diff_norm_f32",
    "omni_guided_smoothness_workspace_bytes", "omni_guided_smoothness_f32", "omni_guided_smoothness_grad_f32",
    "omni_depth_smoothness_workspace_bytes", "omni_depth_smoothness_f32", "omni_depth_smoothness_grad_f32",
    "omni_chamfer_workspace_bytes", "omni_chamfer_nn_f32", "omni_chamfer_grad_f32",
    "omni_augment_rgb_u8", "omni_augment_depth_u16", "omni_augment_planes",
    "omni_planefit_workspace_bytes", "omni_planefit_normals_f32", "omni_planefit_normals_grad_f32", "omni_planefit_loss_f32",
    "omni_planefit_loss_grad_f32",
    "omni_conv2d_bwd_workspace_bytes", "omni_conv2d_bwd_epilogue_f32", "omni_conv2d_bwd_data_f16x3", "omni_conv2d_bwd_weight_f16x3",
    "omni_conv2d_split_weights_f16x3",
    "omni_batchnorm_workspace_bytes", "omni_batchnorm_fwd_f32", "omni_batchnorm_bwd_f32",
    "omni_layernorm_bwd_workspace_bytes", "omni_layernorm_fwd_f32", "omni_layernorm_bwd_f32",
    "omni_attention_bwd_workspace_bytes", "omni_attention_bwd_f32", "omni_gelu_fwd_f32", "omni_gelu_bwd_f32",
    "omni_stem_conv_fwd_f32", "omni_stem_conv_bwd_workspace_bytes", "omni_stem_conv_bwd_weight_f32", "omni_maxpool3x3s2_bwd_f32",
    "omni_upsample_bilinear2x_bwd_f32",
]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OmniLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -m omnifusion_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no fallback path.")
    # The library and PyTorch must share ONE HIP runtime (device pointers and streams cross the
    # boundary).  Both name libamdhip64.so.7; importing torch first makes the dynamic loader bind
    # our DT_NEEDED entry to the copy torch already mapped (loading /opt/rocm's copy first leaves
    # two runtimes in the process and the second one sees no device).
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    lib.omni_last_error.restype = ctypes.c_char_p
    lib.omni_version.restype = ctypes.c_int
    lib.omni_up2_heads_scratch_bytes.restype = ctypes.c_size_t
    lib.omni_dibr_workspace_bytes.restype = ctypes.c_size_t
    lib.omni_splat_render_f32.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_float] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    lib.omni_dibr_f32.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 2 + \
        [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.omni_splat_render_wt_f32.argtypes = [vp] * 3 + [cf] + [vp] * 3 + [ci] * 4 + [vp] * 2
    lib.omni_dibr_wt_f32.argtypes = [vp] * 4 + [ci, cf, ci] + [vp] * 3 + [ci] * 4 + [vp] * 2
    lib.omni_dibr_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.omni_splat_render_bwd_f32.argtypes = [vp] * 6 + [cf] + [vp] * 3 + [ci] * 4 + [vp] * 2
    lib.omni_dibr_bwd_f32.argtypes = [vp] * 7 + [ci, cf, ci] + [vp] * 2 + [ci] * 4 + [vp] * 2
    lib.omni_ssim_f32.argtypes = [vp] * 2 + [ci] * 5 + [vp, ci, vp, vp]
    lib.omni_photometric_workspace_bytes.restype = ctypes.c_size_t
    lib.omni_photometric_grad_scratch_bytes.restype = ctypes.c_size_t
    lib.omni_photometric_loss_f32.argtypes = [vp, vp, vp, ci, vp, ci] + [ci] * 5 + [vp, ci, cf] + [vp] * 3
    lib.omni_photometric_grad_f32.argtypes = [vp, vp, vp, ci, vp, ci] + [ci] * 5 + [vp, ci, cf] + [vp] * 5
    lib.omni_freeview_rotations.argtypes = [vp, vp, ci, vp, vp]
    lib.omni_freeview_equi2pers_f32.argtypes = [vp] * 3 + [ci] * 7 + [cf, cf, ci, vp]
    lib.omni_freeview_pers2equi_f32.argtypes = [vp] * 4 + [ci] * 6 + [cf, cf, vp]
    lib.omni_freeview_merge_f32.argtypes = [vp] * 4 + [ci] * 7 + [cf, cf, vp]
    lib.omni_freeview_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.omni_freeview_bwd_workspace_bytes.argtypes = [ci] * 5
    lib.omni_freeview_equi2pers_bwd_f32.argtypes = [vp] * 3 + [ci] * 7 + [cf, cf, ci, vp, vp]
    lib.omni_freeview_pers2equi_bwd_f32.argtypes = [vp] * 3 + [ci] * 6 + [cf, cf, vp, vp]
    lib.omni_freeview_merge_bwd_f32.argtypes = [vp] * 3 + [ci] * 7 + [cf, cf, vp, vp]
    sz, i64 = ctypes.c_size_t, ctypes.c_int64
    lib.omni_semantic_workspace_bytes.restype = sz
    lib.omni_semantic_workspace_bytes.argtypes = [sz]
    lib.omni_semantic_step_f32.argtypes = [vp, vp, ci, ci, sz, i64, ci] + [vp] * 5
    lib.omni_semantic_grad_f32.argtypes = [vp, vp, ci, ci, sz, i64] + [vp] * 4
    lib.omni_confusion_matrix_i64.argtypes = [vp, vp, sz, ci] + [vp] * 3
    lib.omni_depth_normals_f32.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    lib.omni_sobel_f32.argtypes = [vp] + [ci] * 4 + [vp] * 3
    lib.omni_l1_workspace_bytes.restype = sz
    lib.omni_l1_workspace_bytes.argtypes = [ci]
    lib.omni_l1_loss_f32.argtypes = [vp] * 3 + [ci, ci, sz, ci] + [vp] * 3
    lib.omni_l1_grad_f32.argtypes = [vp] * 3 + [ci, ci, sz, ci] + [vp] * 4
    lib.omni_geometry_terms_workspace_bytes.restype = sz
    lib.omni_geometry_terms_workspace_bytes.argtypes = [ci] * 3
    lib.omni_geometry_terms_f32.argtypes = [vp] * 4 + [ci] * 5 + [vp] * 3
    lib.omni_geometry_terms_grad_f32.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 5
    lib.omni_image_diff_f32.argtypes = [vp] + [ci] * 5 + [vp] * 2
    lib.omni_image_diff_norm_f32.argtypes = [vp] + [ci] * 4 + [vp] * 2
    lib.omni_vertex_diff_norm_f32.argtypes = [vp] + [ci] * 3 + [vp] * 2
    lib.omni_guided_smoothness_workspace_bytes.restype = sz
    lib.omni_guided_smoothness_workspace_bytes.argtypes = [sz]
    lib.omni_guided_smoothness_f32.argtypes = [vp] * 4 + [sz] + [vp] * 3
    lib.omni_guided_smoothness_grad_f32.argtypes = [vp] * 3 + [sz] + [vp] * 4
    lib.omni_depth_smoothness_workspace_bytes.restype = sz
    lib.omni_depth_smoothness_workspace_bytes.argtypes = [ci] * 3
    lib.omni_depth_smoothness_f32.argtypes = [vp] * 5 + [ci] * 4 + [vp] * 3
    lib.omni_depth_smoothness_grad_f32.argtypes = [vp] * 5 + [ci] * 4 + [vp] * 4
    lib.omni_chamfer_workspace_bytes.restype = sz
    lib.omni_chamfer_workspace_bytes.argtypes = [ci] * 4
    lib.omni_chamfer_nn_f32.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 5
    lib.omni_chamfer_grad_f32.argtypes = [vp] * 6 + [ci] * 4 + [vp] * 4
    lib.omni_augment_rgb_u8.argtypes = [vp] * 4 + [ci] * 5 + [vp]
    lib.omni_augment_depth_u16.argtypes = [vp] * 4 + [ci] * 5 + [cf, cf, vp]
    lib.omni_augment_planes.argtypes = [vp, vp, ci, vp, vp] + [ci] * 6 + [vp]
    lib.omni_planefit_workspace_bytes.restype = sz
    lib.omni_planefit_workspace_bytes.argtypes = [ci] * 3
    lib.omni_planefit_normals_f32.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    lib.omni_planefit_normals_grad_f32.argtypes = [vp] * 3 + [ci] * 3 + [vp] * 3
    lib.omni_planefit_loss_f32.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 3
    lib.omni_planefit_loss_grad_f32.argtypes = [vp] * 4 + [ci] * 4 + [vp] * 4
    lib.omni_conv2d_bwd_workspace_bytes.restype = sz
    lib.omni_conv2d_bwd_workspace_bytes.argtypes = [ci] * 10
    lib.omni_conv2d_bwd_epilogue_f32.argtypes = [vp] * 5 + [ctypes.c_longlong, ci, ci, vp, sz, vp]
    lib.omni_conv2d_bwd_data_f16x3.argtypes = [vp] * 5 + [ci] * 10 + [vp, sz, vp]
    lib.omni_conv2d_bwd_weight_f16x3.argtypes = [vp] * 5 + [ci] * 10 + [vp, sz, vp]
    lib.omni_conv2d_split_weights_f16x3.argtypes = [vp, vp, ci, ci, vp]
    cd = ctypes.c_double
    lib.omni_batchnorm_workspace_bytes.restype = sz
    lib.omni_batchnorm_workspace_bytes.argtypes = [ctypes.c_longlong, ci]
    lib.omni_batchnorm_fwd_f32.argtypes = [vp] * 8 + [ctypes.c_longlong, ci, ci, cd, cd, ci, vp, sz, vp]
    lib.omni_batchnorm_bwd_f32.argtypes = [vp] * 9 + [ctypes.c_longlong, ci, ci, ci, vp, sz, vp]
    ll = ctypes.c_longlong
    lib.omni_layernorm_bwd_workspace_bytes.restype = sz
    lib.omni_layernorm_bwd_workspace_bytes.argtypes = [ll, ci]
    lib.omni_layernorm_fwd_f32.argtypes = [vp] * 4 + [ll, ci, cf, vp]
    lib.omni_layernorm_bwd_f32.argtypes = [vp] * 6 + [ll, ci, cf, vp, sz, vp]
    lib.omni_attention_bwd_workspace_bytes.restype = sz
    lib.omni_attention_bwd_workspace_bytes.argtypes = [ci, ci]
    lib.omni_attention_bwd_f32.argtypes = [vp] * 5 + [ci, ci, vp, sz, vp]
    lib.omni_gelu_fwd_f32.argtypes = [vp, vp, ll, vp]
    lib.omni_gelu_bwd_f32.argtypes = [vp] * 3 + [ll, vp]
    lib.omni_stem_conv_fwd_f32.argtypes = [vp] * 4 + [ci] * 3 + [vp]
    lib.omni_stem_conv_bwd_workspace_bytes.restype = sz
    lib.omni_stem_conv_bwd_workspace_bytes.argtypes = [ci] * 3
    lib.omni_stem_conv_bwd_weight_f32.argtypes = [vp] * 4 + [ci] * 3 + [vp, sz, vp]
    lib.omni_maxpool3x3s2_bwd_f32.argtypes = [vp] * 3 + [ci] * 4 + [vp]
    lib.omni_upsample_bilinear2x_bwd_f32.argtypes = [vp, vp] + [ci] * 4 + [vp]
    lib.omni_conv2d_sh_plan.argtypes = [ci] * 13 + [ctypes.POINTER(ci), ci]
    for name in EXPORTS:
        getattr(lib, name)          # AttributeError here = header/library mismatch
    _lib = lib
    return lib


def load_debug():
    """The DEBUG build of the library (python -m omnifusion_amd.build --debug): same entry points plus the
    result-changing ablation switches (OMNI_*_DBG) and the omni_debug_* micro-benchmarks.  tools/ only — nothing under
    omnifusion_amd/ or tests/ loads it."""
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH_DEBUG):
        raise OmniLibraryMissing(f"{LIB_PATH_DEBUG} not found: python -m omnifusion_amd.build --debug")
    lib = ctypes.CDLL(LIB_PATH_DEBUG)
    lib.omni_last_error.restype = ctypes.c_char_p
    return lib


def set_option(name, value):
    check(load().omni_set_option(name.encode(), int(value)), "set_option")


def get_option(name):
    v = ctypes.c_int(0)
    check(load().omni_get_option(name.encode(), ctypes.byref(v)), "get_option")
    return v.value


CALL_LOG = None          # tools/fwd.py --labels: a list that receives the label of every library call (profiles/ label their kernel rows with it)


def check(status, what=""):
    """Map C-ABI status codes to the exceptions the Python boundary promises
    (SURVEY.md §8b 'Errors'): ValueError for bad arguments, RuntimeError for HIP errors."""
    if CALL_LOG is not None:
        CALL_LOG.append(what)
    if status == OMNI_OK:
        return
    msg = load().omni_last_error().decode(errors="replace")
    if status == OMNI_ERR_INVALID:
        raise ValueError(f"{what}: {msg}")
    if status == OMNI_ERR_UNSUPPORTED:
        raise NotImplementedError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg}")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream_of(t):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def dtype_code(t):
    import torch
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise ValueError(f"unsupported dtype {t.dtype}: the HIP path stores float32 or float16")
