"""ctypes loader of libomnifusion_hip.so — the ONLY compute path of this package.

There is no CPU / PyTorch fallback: if the HIP library is missing or fails to load,
importing the operators raises (the product path must fail loudly, never silently run
something else).
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OMNI_LIB_VARIANT") or os.path.join(_HERE, "csrc", "libomnifusion_hip.so")    # (OMNI_LIB_VARIANT: tools/ only — a variant build of the library for same-box A/B timings)
LIB_PATH_DEBUG = os.path.join(_HERE, "csrc", "libomnifusion_hip_dbg.so")     # tools/ only: ablation switches + micro-benchmarks

OMNI_OK, OMNI_ERR_INVALID, OMNI_ERR_HIP, OMNI_ERR_UNSUPPORTED = 0, 1, 2, 3
LAYOUT_BCHWN, LAYOUT_BNCHW, LAYOUT_BNHWC, LAYOUT_BCHNW = 0, 1, 2, 3
F32, F16 = 0, 1

_lib = None


class OmniLibraryMissing(ImportError):
    pass


# The whole C ABI: one line per prototype of include/omnifusion.h, in header order — name, return type, parameter types.
# A letter is a type and a number after it repeats it ("p3ii" = five parameters: three pointers, two ints).  `p` is every
# pointer, out-parameters and omni_stream_t included; `s` is const char*.  tests/test_boundary.py parses the header and
# holds this table to it, type by type.
_CTYPE = {"v": None, "p": ctypes.c_void_p, "s": ctypes.c_char_p, "i": ctypes.c_int, "z": ctypes.c_size_t, "l": ctypes.c_longlong,
          "q": ctypes.c_int64, "f": ctypes.c_float, "d": ctypes.c_double}
_TABLE = """
omni_version i
omni_last_error s
omni_set_option i si
omni_get_option i sp
omni_num_patches i i
omni_patch_centers i iip
omni_geometry_create i piffi4p
omni_geometry_destroy v p
omni_geometry_cache_clear v
omni_geometry_cache_size i
omni_equi2pers i ppi8ffip
omni_equi2pers_aux i ppi3ffp
omni_pers2equi i ppi8ffip
omni_patches_to_planar i ppi6p
omni_pers2equi_conf i p3i7ffip
omni_equi2pers_g i p3i4p
omni_pers2equi_g i p3i4p
omni_equi2pers_bwd i ppi8ffip
omni_pers2equi_bwd i ppi8ffip
omni_conv2d_nhwc_f32 i p6i11p
omni_conv2d_splitk_plan i lii
omni_conv2d_nhwc_f32_ws i p6i12pzp
omni_conv2d_nhwc_f16x3_ws i p6i12pzp
omni_conv2d_nhwc_f16x1_ws i p6i12pzp
omni_conv2d_sh_f16x3_ws i p6i13pzp
omni_conv2d_sh_plan i i13pi
omni_gemm_rows_sh_f16x3 i p5i5p
omni_gemm_rows_pack i ppiip
omni_gemm_rows_ln_sh_f16x3 i p3fp4i4p
omni_conv3x3_up2_sh_f16x3 i p4i7p
omni_up2_heads_scratch_bytes z ii
omni_conv3x3_up2_heads_sh_f16x3 i p4ffpzppi3p
omni_conv3x3_up2_heads_sh_f16x1 i p4ffpzppi3p
omni_heads_pack_f16x3 i pp
omni_conv2d_sh_f16x3_post_ws i p6i13pzpzp
omni_wino_input_sh i ppi4p
omni_conv3x3_wino_sh_f16x3 i p5i8pzp
omni_sh_from_f32 i ppzp
omni_sh_to_f32 i ppzp
omni_sh_overflow i pi
omni_stem_f32 i p4iip
omni_maxpool3x3s2_f32 i ppi4p
omni_upsample_bilinear_f32 i ppi6p
omni_add_hw_f32 i ppi3p
omni_add_period_f32 i ppzzp
omni_stem_sh i p4iip
omni_stem_sh_f16x3 i p4iip
omni_stem_sh_f16x1 i p4iip
omni_maxpool3x3s2_sh i ppi4p
omni_upsample_bilinear_sh i ppi6p
omni_up2_tapsum_sh i p3i5p
omni_conv3x3_up2_taps_sh_f16x3 i p4i7p
omni_add_hw_sh i ppi3p
omni_add_period_sh i ppzzp
omni_layernorm512_sh i p4ifp
omni_gemm_rows_slices_sh_f16x3 i p3i4p
omni_gemm_rows_ln_parts_sh_f16x3 i pip5fp3i4p
omni_splitk_reduce_ln512 i pip5fpiip
omni_gemm_sh_f16x3_ln512_ws i p7fpi4pzp
omni_attention_qkv_sh i ppiip
omni_token_pack_f32 i p3i4p
omni_layernorm512_f32 i p4ifp
omni_attention_f32 i p3iip
omni_heads_f32 i ppffppi3p
omni_mlp_points_f32 i p7i3p
omni_masked_median_f32 i ppzp3
omni_depth_metrics_f32 i p5zp3
omni_semantic_workspace_bytes z z
omni_semantic_step_f32 i ppiizqip5
omni_semantic_grad_f32 i ppiizqp4
omni_confusion_matrix_i64 i ppzip3
omni_preprocess_rgb_u8 i ppi5p
omni_preprocess_depth_u16 i p3i5ffp
omni_augment_rgb_u8 i p4i5p
omni_augment_depth_u16 i p4i5ffp
omni_augment_planes i ppippi6p
omni_png_info i pzp4
omni_png_decode i pzpi3
omni_png_decode_batch i p3i5
omni_zlib_inflate i pzpzpp
omni_png_checksums i pzpp
omni_berhu_workspace_bytes z i
omni_berhu_loss_f32 i p4izp3
omni_berhu_grad_f32 i p4izp4
omni_pointcloud_ply_f32 i p3i3p
omni_dibr_workspace_bytes z i4
omni_splat_render_f32 i p3fppi4pp
omni_dibr_f32 i p4ifippi4pp
omni_splat_render_wt_f32 i p3fp3i4pp
omni_dibr_wt_f32 i p4ifip3i4pp
omni_dibr_bwd_workspace_bytes z i4
omni_splat_render_bwd_f32 i p6fp3i4pp
omni_dibr_bwd_f32 i p7ifippi4pp
omni_ssim_f32 i ppi5pipp
omni_photometric_workspace_bytes z i4
omni_photometric_grad_scratch_bytes z i4
omni_photometric_loss_f32 i p3ipi6pifp3
omni_photometric_grad_f32 i p3ipi6pifp5
omni_freeview_rotations i ppipp
omni_freeview_equi2pers_f32 i p3i7ffip
omni_freeview_pers2equi_f32 i p4i6ffp
omni_freeview_merge_f32 i p4i7ffp
omni_freeview_bwd_workspace_bytes z i5
omni_freeview_equi2pers_bwd_f32 i p3i7ffipp
omni_freeview_pers2equi_bwd_f32 i p3i6ffpp
omni_freeview_merge_bwd_f32 i p3i7ffpp
omni_depth_normals_f32 i ppi3pp
omni_sobel_f32 i pi4p3
omni_l1_workspace_bytes z i
omni_l1_loss_f32 i p3iizip3
omni_l1_grad_f32 i p3iizip4
omni_geometry_terms_workspace_bytes z i3
omni_geometry_terms_f32 i p4i5p3
omni_geometry_terms_grad_f32 i p4i4p5
omni_planefit_workspace_bytes z i3
omni_planefit_normals_f32 i ppi3pp
omni_planefit_normals_grad_f32 i p3i3p3
omni_planefit_loss_f32 i p4i4p3
omni_planefit_loss_grad_f32 i p4i4p4
omni_image_diff_f32 i pi5pp
omni_image_diff_norm_f32 i pi4pp
omni_vertex_diff_norm_f32 i pi3pp
omni_guided_smoothness_workspace_bytes z z
omni_guided_smoothness_f32 i p4zp3
omni_guided_smoothness_grad_f32 i p3zp4
omni_depth_smoothness_workspace_bytes z i3
omni_depth_smoothness_f32 i p5i4p3
omni_depth_smoothness_grad_f32 i p5i4p4
omni_chamfer_workspace_bytes z i4
omni_chamfer_nn_f32 i p4i4p5
omni_chamfer_grad_f32 i p6i4p4
omni_conv2d_bwd_workspace_bytes z i10
omni_conv2d_bwd_epilogue_f32 i p5liipzp
omni_conv2d_bwd_data_f16x3 i p5i10pzp
omni_conv2d_bwd_weight_f16x3 i p5i10pzp
omni_conv2d_split_weights_f16x3 i ppiip
omni_conv2d_bwd_data_f16x1 i p5i10pzp
omni_conv2d_bwd_weight_f16x1 i p5i10pzp
omni_conv2d_split_weights_f16x1 i ppiip
omni_batchnorm_workspace_bytes z li
omni_batchnorm_fwd_f32 i p8liiddipzp
omni_batchnorm_bwd_f32 i p9li3pzp
omni_syncbn_stats_f32 i pplipzp
omni_syncbn_fwd_apply_f32 i p5ip4liddip
omni_syncbn_bwd_reduce_f32 i p8liipzp
omni_syncbn_bwd_apply_f32 i p6ippliip
omni_layernorm_bwd_workspace_bytes z li
omni_layernorm_fwd_f32 i p4lifp
omni_layernorm_bwd_f32 i p6lifpzp
omni_attention_bwd_workspace_bytes z ii
omni_attention_bwd_f32 i p5iipzp
omni_gelu_fwd_f32 i pplp
omni_gelu_bwd_f32 i p3lp
omni_stem_conv_fwd_f32 i p4i3p
omni_stem_conv_bwd_workspace_bytes z i3
omni_stem_conv_bwd_weight_f32 i p4i3pzp
omni_maxpool3x3s2_bwd_f32 i p3i4p
omni_upsample_bilinear2x_bwd_f32 i ppi4p
omni_depth_heads_fwd_f32 i p7i4p
omni_depth_heads_bwd_workspace_bytes z i3
omni_depth_heads_bwd_f32 i p9i4pzp
omni_adamw_grad_sqnorm_f32 i pipipp
omni_adamw_prepare_f32 i pipidip3
omni_adamw_apply_f32 i p4ipipip
omni_point_conv_fwd_f32 i p4i5p
omni_point_conv_bwd_workspace_bytes z i4
omni_point_conv_bwd_f32 i p7i5pzp
"""


def _signature(ret, params=""):
    params = re.sub(r"([a-z])(\d+)", lambda m: m[1] * int(m[2]), params)
    return _CTYPE[ret], tuple(_CTYPE[c] for c in params)


# name -> (restype, argtypes) of every exported function; EXPORTS: their names
SIGNATURES = {name: _signature(*sig) for name, *sig in map(str.split, _TABLE.strip().splitlines())}
EXPORTS = list(SIGNATURES)


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
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = restype, argtypes
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
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


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
