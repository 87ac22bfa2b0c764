"""ctypes binding of libmimo_hip.so (C ABI declared in include/mimo_hip.h).

The library is the product: there is no CPU or eager-PyTorch fallback.  If the
shared object is missing, importing the binding raises with build instructions.
"""
from __future__ import annotations

import ctypes as C
import os

# torch must be imported before libmimo_hip.so is dlopen'ed: the PyTorch-ROCm wheel bundles its own
# libamdhip64.so.7; loading ours first would bind the process to /opt/rocm's copy (same SONAME) and
# leave torch and the engine on mismatched HIP runtimes ("no ROCm-capable device is detected").
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIMO_HIP_LIB: another build of the same library (A/B runs of two builds on one GPU box)
LIB_PATH = os.environ.get("MIMO_HIP_LIB") or os.path.join(_HERE, "libmimo_hip.so")


class MimoHipError(RuntimeError):
    pass


class MimoConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("num_subnetworks", C.c_int32),
        ("filter_base_count", C.c_int32), ("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("encoder_dropout_rate", C.c_float), ("core_dropout_rate", C.c_float), ("decoder_dropout_rate", C.c_float),
        ("bn_eps", C.c_float), ("bn_momentum", C.c_float), ("loss_kind", C.c_int32),
        ("eps_min", C.c_float), ("eps_max", C.c_float), ("device", C.c_int32), ("precision", C.c_int32),
        ("inference_only", C.c_int32), ("center_dropout_rate", C.c_float), ("final_dropout_rate", C.c_float),
        ("norm_kind", C.c_int32), ("act_kind", C.c_int32), ("up_kind", C.c_int32),
    ]


class ForwardArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("stride_n", C.c_int64), ("stride_s", C.c_int64), ("perm", C.c_void_p),
        ("training", C.c_int32), ("drop_masks", C.POINTER(C.c_void_p)), ("out", C.c_void_p),
        ("elem_masks", C.POINTER(C.c_void_p)), ("no_grad", C.c_int32), ("param_version", C.c_int64),
        ("rng_sites", C.POINTER(C.c_uint8)), ("rng_seed", C.c_uint64), ("rng_offset", C.c_uint64),
        ("x_rows", C.c_int64),
    ]


class BnReluBackwardArgs(C.Structure):
    """mimo_op_bn_relu_backward_args (include/mimo_hip.h)"""
    _fields_ = [
        ("kind", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32), ("c_p", C.c_int32),
        ("training", C.c_int32), ("split_out", C.c_int32), ("precision", C.c_int32),
        ("da", C.c_void_p), ("ldda", C.c_int32),
        ("dxpad", C.c_void_p), ("ldp", C.c_int32), ("choff", C.c_int32),
        ("skip", C.c_void_p), ("ldsk", C.c_int32), ("skoff", C.c_int32),
        ("head_w", C.c_void_p), ("head_out", C.c_void_p), ("head_dout", C.c_void_p), ("head_dloss", C.c_void_p),
        ("head_label", C.c_void_p), ("head_mask", C.c_void_p), ("head_perm", C.c_void_p),
        ("head_co", C.c_int32), ("head_subnetworks", C.c_int32), ("head_s", C.c_int32), ("loss_kind", C.c_int32),
        ("eps_min", C.c_float), ("eps_max", C.c_float),
        ("z", C.c_void_p), ("ldz", C.c_int32),
        ("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p), ("mask", C.c_void_p),
        ("dz", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("dbias", C.c_void_p),
        ("c1", C.c_void_p), ("c2", C.c_void_p), ("head_dw", C.c_void_p), ("head_db", C.c_void_p),
        ("absmax", C.c_void_p), ("absmax_capacity", C.c_int32), ("absmax_n", C.POINTER(C.c_int32)),
        ("status", C.POINTER(C.c_int32)),
    ]


class HeadBackwardArgs(C.Structure):
    """mimo_op_head_backward_args (include/mimo_hip.h)"""
    _fields_ = [
        ("a", C.c_void_p), ("lda", C.c_int32), ("w", C.c_void_p),
        ("c", C.c_int32), ("c_p", C.c_int32), ("co", C.c_int32), ("n", C.c_int32), ("subnetworks", C.c_int32), ("s", C.c_int32),
        ("hw", C.c_int64),
        ("out", C.c_void_p), ("dout", C.c_void_p), ("dloss", C.c_void_p), ("label", C.c_void_p), ("mask", C.c_void_p),
        ("perm", C.c_void_p), ("loss_kind", C.c_int32), ("eps_min", C.c_float), ("eps_max", C.c_float),
        ("in_scale", C.c_void_p), ("in_shift", C.c_void_p), ("precision", C.c_int32),
        ("da", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p),
    ]


class BnStatsArgs(C.Structure):
    """mimo_op_bn_stats_args (include/mimo_hip.h)"""
    _fields_ = [
        ("partial", C.c_void_p), ("rows", C.c_int32), ("cout_pad", C.c_int32), ("c", C.c_int32), ("c_p", C.c_int32),
        ("training", C.c_int32), ("route", C.c_int32), ("count", C.c_int64),
        ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
        ("momentum", C.c_float), ("eps", C.c_float),
        ("mean", C.c_void_p), ("invstd", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
        ("status", C.POINTER(C.c_int32)),
    ]


class BnReluForwardArgs(C.Structure):
    """mimo_op_bn_relu_forward_args (include/mimo_hip.h)"""
    _fields_ = [
        ("z", C.c_void_p), ("ldz", C.c_int32), ("scale", C.c_void_p), ("shift", C.c_void_p), ("mask", C.c_void_p),
        ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32), ("c_p", C.c_int32), ("precision", C.c_int32),
        ("z_fp32", C.c_int32),
        ("a", C.c_void_p), ("lda", C.c_int32), ("pool", C.c_void_p), ("ldpool", C.c_int32), ("status", C.POINTER(C.c_int32)),
    ]


class HeadForwardArgs(C.Structure):
    """mimo_op_head_forward_args (include/mimo_hip.h)"""
    _fields_ = [
        ("a", C.c_void_p), ("lda", C.c_int32), ("w", C.c_void_p), ("bias", C.c_void_p),
        ("c", C.c_int32), ("co", C.c_int32), ("n", C.c_int32), ("subnetworks", C.c_int32), ("s", C.c_int32), ("hw", C.c_int32),
        ("in_scale", C.c_void_p), ("in_shift", C.c_void_p), ("precision", C.c_int32),
        ("out", C.c_void_p), ("status", C.POINTER(C.c_int32)),
    ]


class MonitorPanel(C.Structure):
    """mimo_monitor_panel (include/mimo_hip.h)"""
    _fields_ = [
        ("src", C.c_void_p), ("mask", C.c_void_p),
        ("n", C.c_int32), ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("mc", C.c_int32),
        ("channel", C.c_int32), ("count", C.c_int32), ("nrow", C.c_int32), ("padding", C.c_int32), ("flags", C.c_int32),
        ("vmin", C.c_float), ("vmax", C.c_float), ("lut", C.c_void_p), ("out_offset", C.c_int64),
    ]


class GatherField(C.Structure):
    """mimo_gather_field (include/mimo_hip.h)"""
    _fields_ = [("src", C.c_void_p), ("lut", C.c_void_p), ("dst", C.c_void_p), ("c", C.c_int32), ("reserved", C.c_int32)]


class StitchField(C.Structure):
    """mimo_stitch_field (include/mimo_hip.h)"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("c", C.c_int32), ("reserved", C.c_int32)]


LOSS_KINDS = {"laplace_nll": 0, "gaussian_nll": 1}
# "bf16-mixed" / "16-mixed": Lightning's names for bf16 / fp16 autocast training — here 16-bit storage + operands
PRECISIONS = {"fp32": 0, "split16": 1, "bf16": 2, "bf16-mixed": 3, "16-mixed": 4}
WINDOWS = {"uniform": 0, "linear": 1, "crop": 2}  # MIMO_WINDOW_*

_lib = None

_P, _I, _L, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
_SIGNATURES = {
    "mimo_last_error": (C.c_char_p, []),
    "mimo_version": (C.c_int, []),
    "mimo_plan_create": (C.c_int, [C.POINTER(MimoConfig), C.POINTER(_P)]),
    "mimo_plan_destroy": (None, [_P]),
    "mimo_plan_workspace_bytes": (C.c_size_t, [_P]),
    "mimo_plan_num_tensors": (C.c_int, [_P]),
    "mimo_plan_tensor_info": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int, C.POINTER(_L), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(_L)]),
    "mimo_plan_param_floats": (_L, [_P]),
    "mimo_plan_buffer_floats": (_L, [_P]),
    "mimo_plan_bind": (C.c_int, [_P, _P, _P, _P]),
    "mimo_plan_dropout_mask": (C.c_int, [_P, C.c_int, _P, _P]),
    "mimo_plan_status": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32, _P]),
    "mimo_plan_num_double_convs": (C.c_int, [_P]),
    "mimo_plan_double_conv_channels": (C.c_int, [_P, C.c_int]),
    "mimo_forward": (C.c_int, [_P, C.POINTER(ForwardArgs), _P]),
    "mimo_draw_permutations": (C.c_int, [_P, _P, _I, _I, _I, _I, C.c_uint64, C.c_uint64, _P]),
    "mimo_loss_forward": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "mimo_backward": (C.c_int, [_P, _P, _P, _P, _P]),
    "mimo_backward_stage": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "mimo_backward_stage_async": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_void_p)]),
    "mimo_plan_encoder_param_floats": (_L, [_P]),
    "mimo_input_gradient": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "mimo_input_gradient_mc": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "mimo_fgsm_perturb": (C.c_int, [_P, _P, _L, C.POINTER(_F), C.c_int, _F, _F, _P, _P]),
    "mimo_pgd_step": (C.c_int, [_P, _P, _P, _L, C.POINTER(_F), C.POINTER(_F), C.c_int, _F, _F, _P]),
    "mimo_pgd_init": (C.c_int, [_P, _L, C.POINTER(_F), C.c_int, _F, _F, C.c_uint64, C.c_uint64, _P, _P]),
    "mimo_plan_num_backward_stages": (C.c_int, [_P]),
    "mimo_plan_backward_stage_range": (C.c_int, [_P, C.c_int, C.POINTER(_L), C.POINTER(_L)]),
    "mimo_plan_profile": (C.c_int, [_P, C.c_int]),
    "mimo_plan_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(_L), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double)]),
    "mimo_plan_profile_read_tier": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mimo_plan_profile_read_kind_tier": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "mimo_adam_step": (C.c_int, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _F, _P]),
    "mimo_adam_step_amp": (C.c_int, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _P, _F, _P, _P, _P]),
    "mimo_grad_clip_scratch_bytes": (C.c_size_t, []),
    "mimo_adam_step_clipped": (C.c_int, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _P, _F, _P, _P, _I, _F, _P, _P, _P]),
    "mimo_uncertainties": (C.c_int, [_P, _P, _I, _I, _I, _L, _I, _P, _P, _P, _P]),
    "mimo_evidential_forward": (C.c_int, [_P, _P, _P, _I, _L, _P, _P, _P]),
    "mimo_evidential_backward": (C.c_int, [_P, _P, _P, _P, _P, _I, _L, _P, _P]),
    "mimo_evidential_uncertainties": (C.c_int, [_P, _I, _L, _P, _P, _P, _P]),
    "mimo_evidential_loss_gradient": (C.c_int, [_P, _P, _P, _I, _L, _F, _P, _P]),
    "mimo_evidential_step": (C.c_int, [_P, _P, _P, _I, _L, _P, _P, _P, _P, _P, _I, _P]),
    "mimo_evidential_loss_gradient_dev": (C.c_int, [_P, _P, _P, _I, _L, _F, _P, _P, _P]),
    "mimo_validation_epilogue": (C.c_int, [_P, _P, _P, _I, _I, _I, _L, _I, _F, _F, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mimo_loss_buffer_step": (C.c_int, [_P, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    "mimo_training_epilogue": (C.c_int, [_P, _P, _P, _I, _I, _I, _L, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mimo_eval_workspace_bytes": (C.c_size_t, []),
    "mimo_eval_accumulate": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _L, _I, _F, _F, _P, _I, _P, _P, _P]),
    "mimo_eval_select": (C.c_int, [_P, _L, _P, _I, _P, _P]),
    "mimo_eval_interval_sums": (C.c_int, [_P, _L, _I, _I, _P, _P, _P]),
    "mimo_eval_accumulate_sources": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _L, _I, _F, _F, _P, _I, _P, _P, _P, _P]),
    "mimo_eval_select_by": (C.c_int, [_P, _I, _L, _P, _I, _P, _P]),
    "mimo_eval_interval_sums_by": (C.c_int, [_P, _I, _P, _I, _L, _I, _I, _P, _P, _P]),
    "mimo_score_workspace_bytes": (C.c_size_t, []),
    "mimo_score_accumulate": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _L, _I, _F, _F, _P, _I, _P, _P, _P, _P, _P]),
    "mimo_score_accumulate_evidential": (C.c_int, [_P, _P, _P, _I, _L, _P, _I, _P, _P, _P, _P, _P]),
    "mimo_score_finalize": (C.c_int, [_P, _I, _P, _P]),
    "mimo_op_conv3x3_forward": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_conv3x3_dgrad": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_conv3x3_wgrad": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_maxpool2x2": (C.c_int, [_P, _P, _I, _I, _I, _I, _P]),
    "mimo_op_upsample_cat": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_fold_slice": (C.c_int, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_pool_backward": (C.c_int, [_P, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_up_backward": (C.c_int, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_bn_relu_backward": (C.c_int, [C.POINTER(BnReluBackwardArgs), _P]),
    "mimo_op_head_backward": (C.c_int, [C.POINTER(HeadBackwardArgs), _P]),
    "mimo_op_bn_stats": (C.c_int, [C.POINTER(BnStatsArgs), _P]),
    "mimo_op_bn_relu_forward": (C.c_int, [C.POINTER(BnReluForwardArgs), _P]),
    "mimo_op_maxpool2x2_ex": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_upsample_cat_ex": (C.c_int, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_op_head_forward": (C.c_int, [C.POINTER(HeadForwardArgs), _P]),
    "mimo_op_loss_forward": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _P, _P]),
    "mimo_op_pack_input": (C.c_int, [_P, _L, _L, _L, _P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "mimo_op_unpack_dx": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "mimo_op_fold_image_grad": (C.c_int, [_P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "mimo_op_fold_image_grad_mc": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "mimo_monitor_grid_shape": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mimo_monitor_scratch_bytes": (C.c_size_t, [C.c_int]),
    "mimo_monitor_grids": (C.c_int, [C.POINTER(MonitorPanel), C.c_int, _P, _P, _P]),
    "mimo_dataset_gather": (C.c_int, [C.POINTER(GatherField), C.c_int, _P, _P, _L, _I, _I, _I, _P]),
    "mimo_scene_gather_tiles": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mimo_scene_stitch": (C.c_int, [C.POINTER(StitchField), C.c_int, _I, _I, _I, _I, _I, _I, _I, _P]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load():
    """Load the shared library (once) and attach argument/return types."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MimoHipError(
            f"{LIB_PATH} not found: build it with `make` (hipcc --offload-arch=gfx950) or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().mimo_last_error()
        raise MimoHipError(f"{what or 'libmimo_hip'} failed (status {rc}): {msg.decode() if msg else '?'}")


def ptr(t) -> int:
    """Raw device pointer of a torch tensor (or 0 for None)."""
    return 0 if t is None else t.data_ptr()


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
