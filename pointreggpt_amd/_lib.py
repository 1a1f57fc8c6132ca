"""ctypes binding of libprg_hip.so (include/prg.h).  No CPU fallback: if the library is missing or a call
fails this raises — the product path never routes around the HIP kernels."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("PRG_HIP_LIB", _HERE / "libprg_hip.so"))

PRG_F32, PRG_BF16, PRG_MXFP8, PRG_F16X3 = 0, 1, 2, 3


class PrgError(RuntimeError):
    pass


class UnetConfigC(C.Structure):
    _fields_ = [("dim", C.c_int32), ("n_levels", C.c_int32), ("dim_mults", C.c_int32 * 8),
                ("in_channels", C.c_int32), ("conditional", C.c_int32), ("param_cond_dim", C.c_int32),
                ("groups", C.c_int32), ("sigmoid_out", C.c_int32)]


class StepC(C.Structure):
    _fields_ = [("t", C.c_int32), ("clip_pred", C.c_int32), ("c_x0", C.c_float), ("c_x", C.c_float),
                ("c_eps", C.c_float), ("sigma", C.c_float), ("sqrt_recip", C.c_float),
                ("sqrt_recipm1", C.c_float)]


class ConvFusedC(C.Structure):
    """prg_conv_fused (include/prg.h): the arguments of prg_debug_conv_fused."""
    _fields_ = ([(n, C.c_void_p) for n in ("x0", "x1", "w", "bias", "pro_a", "pro_b", "residual", "res_a", "res_b", "fold_acc",
                                           "fold_p", "fold_q", "gamma", "beta", "out", "sums", "acc_raw", "coef_a", "coef_b")] +
                [(n, C.c_int32) for n in ("B", "C0", "C1", "Cout", "H", "W", "K", "groups", "prologue", "residual_mode",
                                          "in_place", "stats", "nsplit", "acc_done", "stats_pass", "storage",
                                          "family", "th", "tw", "bm", "bn", "nslabs")] +
                [("slabs", C.c_void_p)])


CF_PRO_NONE, CF_PRO_TABLES, CF_PRO_FOLD = 0, 1, 2
CF_RES_NONE, CF_RES_ADD, CF_RES_TABLES, CF_RES_FOLD = 0, 1, 2, 3
CF_STATS_OFF, CF_STATS_SLABS, CF_STATS_ACC = 0, 1, 2
CF_STORE_BF16, CF_STORE_F16X3, CF_STORE_F32 = 0, 1, 2
CF_MAX_SLABS = 1024
# ConvFamily (csrc/conv_choose.h), as prg_conv_fused.family reports it
CONV_FAMILIES = ("none", "igemm", "halo", "mx_halo", "c64", "ws", "w256", "w256mx", "split_halo", "split_ws", "split_p64", "split_w512",
                 "split_igemm")


class GnFoldC(C.Structure):
    """prg_gn_fold (include/prg.h): the arguments of prg_debug_gn_fold."""
    _fields_ = ([(n, C.c_void_p) for n in ("acc", "p", "q", "entries", "flat", "ss_a", "ss_b", "row", "pq", "zero_out", "x", "residual",
                                           "out", "coef_a", "coef_b")] +
                [(n, C.c_int64) for n in ("ss_a_stride", "ss_a_floats", "ss_b_stride", "ss_b_floats", "row_stride", "flat_floats",
                                          "zero_words")] +
                [(n, C.c_int32) for n in ("B", "C", "HW", "groups", "pq_per_image", "n_entries", "use_entry", "ss_total", "output",
                                          "in_place")])


GF_NONE, GF_TABLES, GF_APPLY = 0, 1, 2

_P, _I, _F, _L = C.c_void_p, C.c_int, C.c_float, C.c_int64

# name -> (restype, argtypes): every symbol include/prg.h declares
PROTOTYPES = {
    "prg_abi_version": (C.c_int, []),
    "prg_last_error": (C.c_char_p, []),
    "prg_device_info": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
    "prg_depth2pc": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _P]),
    "prg_pc2depth": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "prg_project_points_zbuffer": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P]),
    "prg_pose_candidate_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "prg_pose_candidate_counts": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _F, _P, _P, C.c_size_t, _P]),
    "prg_reproject_zbuffer": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P]),
    "prg_unproject_f64": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _P]),
    "prg_depth_augment": (C.c_int, [_P, _P, _I, _I, _I, _P]),
    "prg_apply_mask": (C.c_int, [_P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _P]),
    "prg_occlusion_filter": (C.c_int, [_P, _P, _P, _I, _I, _I, _F, _P]),
    "prg_overlap_counts": (C.c_int, [_P, _P, _I, _L, C.c_double, _P, _P]),
    "prg_overlap_counts_indexed": (C.c_int, [_P, _P, _I, _P, _I, _L, C.c_double, _P, _P]),
    "prg_nearest_ragged_f64": (C.c_int, [_P, _P, _I, _L, _P, _P, _P]),
    "prg_radius_pairs_workspace_bytes": (C.c_size_t, [_L]),
    "prg_radius_count_ragged_f64": (C.c_int, [_P, _P, _I, _L, _L, C.c_double, _P, _P, C.c_size_t, _P]),
    "prg_radius_fill_ragged_f64": (C.c_int, [_P, _P, _I, _L, C.c_double, _P, _L, _P, _P]),
    "prg_radius_select_ragged_f64": (C.c_int, [_P, _P, _I, _L, _P, _P, _L, _I, _P, _P, _P, _P, _P]),
    "prg_normals_ragged_f64": (C.c_int, [_P, _P, _I, _P, _P, _P, _P, _L, _I, _P, _I, _P, _P, _P, _P]),
    "prg_patch_tables_ragged": (C.c_int, [_P, _P, _P, _I, _L, _L, _I, _P, _P, _P, _P, _P, _P]),
    "prg_patch_overlap_ragged_f64": (C.c_int, [_P, _P, _I, _P, _P, _L, _I, C.c_double, _P, _L, _L, _P, _P, _P]),
    "prg_patch_corr_labels_f64": (C.c_int, [_P, _L, _P, _L, _I, _P, _L, C.c_double, _P, _P]),
    "prg_voxel_grid_workspace_bytes": (C.c_size_t, [_L, _I]),
    "prg_voxel_grid_ragged": (C.c_int, [_P, _P, _P, _I, _L, C.c_double, _P, _P, _P, _P, C.c_size_t, _P]),
    "prg_merge_memory_f64": (C.c_int, [_P, _P, _L, _P, _P, _I, _I, _P, _P, _P, _P]),
    "prg_rigid_crop_ragged_f64": (C.c_int, [_P, _P, _P, _I, _L, _P, _P, _P, _P, _P, _P, _P]),
    "prg_augment_ragged_f64": (C.c_int, [_P, _P, _I, _L, _P, _P, _P, C.c_uint32, _P, _L, C.c_double, _P, _L, _P, _P, _P]),
    "prg_unet_param_count": (_L, [C.POINTER(UnetConfigC)]),
    "prg_unet_create": (C.c_int, [C.POINTER(UnetConfigC), _P, _L, _I, C.POINTER(_P)]),
    "prg_unet_destroy": (C.c_int, [_P]),
    "prg_unet_reserve": (C.c_int, [_P, _I, _I]),
    "prg_unet_set_time_freqs": (C.c_int, [_P, _P, _I]),
    "prg_unet_forward": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _P]),
    "prg_maskunet_forward": (C.c_int, [_P, _P, _P, _I, _I, _P]),
    "prg_debug_conv3x3": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "prg_debug_block_pair": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "prg_debug_upsample_conv3x3": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "prg_debug_conv4x4s2": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "prg_debug_conv": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "prg_debug_upsample_conv": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "prg_debug_attention_core": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "prg_debug_layernorm": (C.c_int, [_P, _P, _P, _P, _L, _I, _I, _P]),
    "prg_debug_linear_attention_block": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _P]),
    "prg_debug_resblock_tail": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "prg_debug_conv_fused": (C.c_int, [C.POINTER(ConvFusedC), _P]),
    "prg_debug_conv_choice": (C.c_int, [_P, _P, _P, _P]),
    "prg_debug_gn_stats": (C.c_int, [_P, _P, C.POINTER(_I), _I, _I, _I, _I, _I, _P]),
    "prg_debug_gn_coeff": (C.c_int, [_P, _I, _P, _P, _P, _L, _L, _P, _L, _L, C.POINTER(_I), _L, _P, _P, _I, _I, _I, _I, _P]),
    "prg_debug_gn_fold": (C.c_int, [C.POINTER(GnFoldC), _P]),
    "prg_debug_affine_silu": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "prg_debug_linear": (C.c_int, [_P, _I, _I, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "prg_debug_sinusoidal": (C.c_int, [_P, _P, _P, _I, _I, _I, _P]),
    "prg_debug_weight_arena": (C.c_int, [C.POINTER(UnetConfigC), _P, _L, _I, _I, _I, _P, _L, C.POINTER(_L)]),
    "prg_debug_pack_conv": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _P, _L, C.POINTER(_L)]),
    "prg_unet_set_taps": (C.c_int, [_P, _I]),
    "prg_unet_get_tap": (C.c_int, [_P, C.c_char_p, _P, _L, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _P]),
    "prg_sampler_create": (C.c_int, [_P, C.POINTER(StepC), _I, _I, _I, C.POINTER(_P)]),
    "prg_sampler_destroy": (C.c_int, [_P]),
    "prg_sampler_set_graph": (C.c_int, [_P, _I]),
    "prg_sampler_run": (C.c_int, [_P, _P, _P, _P, _L, _P, _P, _P]),
    "prg_sampler_set_profile": (C.c_int, [_P, _I]),
    "prg_sampler_get_profile": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(_L), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]),
    "prg_sampler_get_profile_bytes": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "prg_sampler_get_profile_executed": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "prg_sampler_get_profile_step": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(_L)]),
    "prg_debug_sampler_step": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _P]),
    "prg_debug_sampler_step_keep": (C.c_int, [_P, _P, _P, _P, _P, _F, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _P]),
    "prg_debug_sampler_step_objective": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _F, _F, _F, _P, C.c_int, C.c_int, C.c_int,
                                                   C.POINTER(C.c_float), _P]),
    "prg_sampler_set_keep": (C.c_int, [_P, _P, _I]),
    "prg_sampler_set_objective": (C.c_int, [_P, _I, _P, _P, _I]),
    "prg_sampler_set_keep_draws": (C.c_int, [_P, _P, _L]),
    "prg_sampler_get_profile_shapes": (C.c_int, [_P, _P, _I, C.POINTER(C.c_int32)]),
    "prg_validate_workspace_bytes": (C.c_size_t, [_I, _I]),
    "prg_q_sample": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _I, _I, _P, _P, _P]),
    "prg_diffusion_loss": (C.c_int, [_P, _P, _P, _P, C.c_uint32, _P, _P, _P, _I, _I, _I, _I, _P, C.c_size_t, _P, _P]),
    "prg_mask_metrics": (C.c_int, [_P, _P, _P, _P, _F, _F, _I, _I, _P, C.c_size_t, _P, _P, _P]),
    "prg_host_crop_aabb": (C.c_int, [_P, _L, _P, _P, _P, C.POINTER(_L)]),
    "prg_host_voxel_down_sample": (C.c_int, [_P, _L, C.c_double, _P, C.POINTER(_L)]),
    "prg_host_write_ply": (C.c_int, [C.c_char_p, _P, _L]),
    "prg_pool_create": (C.c_int, [_I, C.POINTER(_P)]),
    "prg_pool_destroy": (C.c_int, [_P]),
    "prg_pool_wait": (C.c_int, [_P, C.POINTER(_L)]),
    "prg_pool_submit_cloud": (C.c_int, [_P, C.c_char_p, _P, _L, _P, _P, _I, _P, _P, C.c_double, _P]),
    "prg_pool_submit_image": (C.c_int, [_P, C.c_char_p, _P, _I, _I, _I]),
    "prg_pool_submit_text": (C.c_int, [_P, C.c_char_p, _P, _I, _I]),
}

_lib = None


def load():
    """dlopen the HIP library and attach prototypes.  Raises PrgError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch's wheel carries its own libamdhip64: import it FIRST so this library binds to the HIP runtime torch already
    # initialised (loading /opt/rocm's copy first leaves the process with two runtimes, one of which sees no device)
    import torch  # noqa: F401
    if not LIB_PATH.exists():
        raise PrgError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"or `make -C pointreggpt_amd/csrc` (there is no CPU fallback)")
    try:
        lib = C.CDLL(str(LIB_PATH))
    except OSError as e:  # missing ROCm runtime etc.
        raise PrgError(f"cannot load {LIB_PATH}: {e}") from e
    # PRG_HIP_LIB_ALLOW_MISSING=1 (diagnostics only, with PRG_HIP_LIB=<an older build>: same-box A/B against a previous round's
    # library, tools/gpu_r5_call2.sh): entry points that library predates are skipped; calling one fails at the call site
    lenient = os.environ.get("PRG_HIP_LIB_ALLOW_MISSING", "0") not in ("", "0") and bool(os.environ.get("PRG_HIP_LIB"))
    for name, (res, args) in PROTOTYPES.items():
        if lenient and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)   # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.prg_abi_version() != 1:
        raise PrgError(f"ABI version mismatch: library {lib.prg_abi_version()}, binding 1")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().prg_last_error()
        raise PrgError(f"{what or 'libprg_hip'} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a contiguous torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor must be contiguous"
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise PrgError("no HIP device visible: pointreggpt_amd has no CPU path")
