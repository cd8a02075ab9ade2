"""ctypes binding of `libi2v_hip.so` (C ABI: `include/i2v_hip.h`).

The product path has NO fallback: `load()` raises if the HIP library is missing or is not the
gfx950 build.  (`bind()` only attaches prototypes to an already opened library; the planner unit
tests use it for their host simulation of the ABI.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libi2v_hip.so")
HIP_BACKEND = b"hip:gfx950"


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("src", "dst", "cin", "cout", "kh", "kw", "stride", "pad", "relu", "residual")]


class PoolDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("src", "dst", "k", "stride", "pad")]


class Conv3dDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("src", "dst", "cin", "cout", "kt", "kh", "kw", "stride_t", "stride", "pad_t", "pad", "dil_t",
                 "relu", "residual")]


class AttnDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("theta", "phi", "g", "dst")] + [("scale", C.c_float)]


class SeDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("src", "dst", "residual", "C", "rd", "relu")]


class Pool3dDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("src", "dst", "kt", "k", "stride_t", "stride", "pad_t", "pad")]


class I2VError(RuntimeError):
    pass


_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
_PROTOS = {
    "i2v_create": ([_I, C.POINTER(_P)], _I),
    "i2v_destroy": ([_P], _I),
    "i2v_last_error": ([], C.c_char_p),
    "i2v_abi_version": ([], _I),
    "i2v_backend": ([], C.c_char_p),
    "i2v_backend_stat": ([C.c_char_p], C.c_longlong),
    "i2v_net_create": ([_P, C.POINTER(_I)], _I),
    "i2v_net_destroy": ([_P, _I], _I),
    "i2v_net_add_buffer": ([_P, _I, _I, _I, _I, C.POINTER(_I)], _I),
    "i2v_net_add_tensor": ([_P, _I, _I, _I, _I, _I, C.POINTER(_I)], _I),
    "i2v_net_set_input": ([_P, _I, _I], _I),
    "i2v_net_set_relu_gain": ([_P, _I, _I, _F], _I),
    "i2v_net_add_conv": ([_P, _I, C.POINTER(ConvDesc), _P, _P, _P], _I),
    "i2v_net_add_conv_grouped": ([_P, _I, C.POINTER(ConvDesc), _I, _P, _P, _P], _I),
    "i2v_net_add_conv_depthwise": ([_P, _I, C.POINTER(ConvDesc), _P, _P, _P], _I),
    "i2v_net_add_maxpool": ([_P, _I, C.POINTER(PoolDesc)], _I),
    "i2v_net_add_conv_preact": ([_P, _I, C.POINTER(ConvDesc), _P, _P, _P, _P, _P], _I),
    "i2v_net_add_avgpool": ([_P, _I, C.POINTER(PoolDesc)], _I),
    "i2v_net_add_buffer3d": ([_P, _I, _I, _I, _I, _I, C.POINTER(_I)], _I),
    "i2v_net_add_conv3d": ([_P, _I, C.POINTER(Conv3dDesc), _P, _P, _P], _I),
    "i2v_net_add_maxpool3d": ([_P, _I, C.POINTER(Pool3dDesc)], _I),
    "i2v_net_add_attention": ([_P, _I, C.POINTER(AttnDesc)], _I),
    "i2v_net_add_se": ([_P, _I, C.POINTER(SeDesc), _P, _P, _P, _P], _I),
    "i2v_net_tensor_frames": ([_P, _I, _I, C.POINTER(_I)], _I),
    "i2v_net_plan": ([_P, _I, C.POINTER(_I), _I, _I], _I),
    "i2v_net_workspace_bytes": ([_P, _I], C.c_size_t),
    "i2v_net_fusion_info": ([_P, _I, _P], _I),
    "i2v_net_scpair_info": ([_P, _I, _P], _I),
    "i2v_net_forward": ([_P, _I, _P, _I, _P], _I),
    "i2v_net_hook_info": ([_P, _I, _I, C.POINTER(_P), C.POINTER(_L), C.POINTER(_P), C.POINTER(_L),
                           C.POINTER(_L), C.POINTER(C.c_int32)], _I),
    "i2v_net_backward": ([_P, _I, _P, _I, _P], _I),
    "i2v_net_read_tensor": ([_P, _I, _I, _I, _P, _I, _P], _I),
    "i2v_timing_enable": ([_P, _I], _I),
    "i2v_timing_collect": ([_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_L), _I], _I),
    "i2v_timing_collect_ex": ([_P, C.POINTER(C.c_double), _I, _I], _I),
    "i2v_clip_from_u8_f32": ([_P, _P, _I, _I, _I, _I, _P], _I),
    "i2v_clip_resize_crop_u8_f32": ([_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P], _I),
    "i2v_frames_from_video_f32": ([_P, _P, _P, _I, _I, _I, _I, _P], _I),
    "i2v_compose_f32": ([_P, _P, _P, _I, _I, _I, _I, _F, _I, _P], _I),
    "i2v_cossim_scratch_bytes": ([_L, _I], C.c_size_t),
    "i2v_cossim_fwd_bwd_f32": ([_P, _L, _P, _L, _L, _I, _P, _I, _F, _I, _I, _P, _P, _L, _P, _P], _I),
    "i2v_std_fwd_bwd_f32": ([_P, _L, _L, _I, _I, _I, _P, _P, _L, _P, _P], _I),
    "i2v_std_reduce_f32": ([_P, _L, _L, _I, _P, _P], _I),
    "i2v_std_grad_f32": ([_P, _L, _L, _I, _L, _I, _I, _P, _P, _L, _P, _P], _I),
    "i2v_adam_step_f32": ([_P, _P, _P, _P, _P, _L, _I, _F, C.c_double, C.c_double, C.c_double, C.c_double, _I, _P], _I),
    "i2v_sign_step_f32": ([_P, _P, _P, _L, _L, _F, _F, _P], _I),
    "i2v_sign_step_delta_f32": ([_P, _P, _L, _F, _P], _I),
    "i2v_sign_step_delta_gx_f32": ([_P, _P, _P, _L, _F, _F, _P], _I),
    "i2v_ilaf_reduce_f32": ([_P, _L, _P, _P, _L, _I, _P, _P], _I),
    "i2v_ilaf_grad_f32": ([_P, _L, _P, _P, _L, _I, C.c_double, _I, _I, _P, _P, _L, _P, _P], _I),
    "i2v_ilaf_scratch_bytes": ([_L, _I, _I], C.c_size_t),
    "i2v_ilaf_reduce_seg_f32": ([_P, _L, _P, _P, _L, _I, _I, _P, _P], _I),
    "i2v_ilaf_grad_seg_f32": ([_P, _L, _P, _P, _L, _I, _I, _P, _I, _I, _P, _P, _L, _P, _P], _I),
    "i2v_tap_distance_f32": ([_P, _L, _P, _L, _I, _I, C.c_double, _I, _I, _P, _P, _L, _P, _P], _I),
    "i2v_head_scratch_bytes": ([_I, _I], C.c_size_t),
    "i2v_head_ce_f32": ([_P, _L, _I, _I, _I, _I, _P, _P, _I, _P, _F, _I, _I, _P, _P, _P, _L, _P, _P], _I),
    "i2v_clip_resample_crop_u8_f32": ([_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P], _I),
    "i2v_tt_grad_mix_f32": ([_P, _P, _P, _P, _I, _L, _I, _I, _F, _P], _I),
    "i2v_resample_nearest_f32": ([_P, _P, _L, _I, _I, _I, _I, _P, _P, _P], _I),
    "i2v_resample_nearest_bwd_f32": ([_P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _P, _P], _I),
    "i2v_dwconv1d_f32": ([_P, _P, _L, _I, _L, _P, _I, _P], _I),
    "i2v_tap_scratch_bytes": ([_L], _L),
    "i2v_tap_perts_f32": ([_P, _P, _P, _I, _I, _I, _I, _I, _P], _I),
    "i2v_tap_sign_abs_f32": ([_P, _P, _P, _L, _P, _P], _I),
    "i2v_tap_grad_f32": ([_P, _P, _P, _I, _I, _I, _I, _I, _F, _P], _I),
    "i2v_grad_post_scratch_bytes": ([_I, _I, _I, _I, _I, _I], _L),
    "i2v_grad_post_f32": ([_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P], _I),
    "i2v_head_pool_f32": ([_P, _L, _I, _I, _I, _I, _I, _I, _P, _P], _I),
    "i2v_head_logits_ce_f32": ([_I, _I, _P, _P, _I, _P, _F, _P, _P, _P, _P], _I),
    "i2v_head_grad_f32": ([_P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P, _P], _I),
    "i2v_aens_coeffs_f32": ([_P, _P, _F, _I, _P], _I),
    "i2v_aens_reduce_f32": ([_P, _P, _I, _I, _P, _P, _P], _I),
}
EXPORTS = tuple(_PROTOS)
# The ragged clip transform (`include/i2v_loader.h`): a header of its own, outside the ABI the planner's host simulation implements,
# so bound only on the product library.
_LOADER_PROTOS = {
    "i2v_clip_gather_scratch_bytes": ([_I, _I, _I, _I], _L),
    "i2v_clip_gather_resize_crop_u8_f32": ([_P, _L, _P, _P, _I, _I, _P, _I, _P, _I, _I, _I, _P, _P, _L, _P], _I),
}
LOADER_EXPORTS = tuple(_LOADER_PROTOS)


def _net_protos(fam, config):
    """The seven entries every transformer family has (`include/i2v_<fam>.h`): create, destroy, workspace_bytes, forward, backward,
    hook_info and read_hook, with the family's config struct."""
    return {
        f"i2v_{fam}_create": ([_I, C.POINTER(config), C.POINTER(_P), _I, C.POINTER(C.c_int32), _I, _I, C.POINTER(_P)], _I),
        f"i2v_{fam}_destroy": ([_P], _I),
        f"i2v_{fam}_workspace_bytes": ([_P], _L),
        f"i2v_{fam}_forward": ([_P, _P, _I, _P], _I),
        f"i2v_{fam}_backward": ([_P, _P, _I, _P], _I),
        f"i2v_{fam}_hook_info": ([_P, _I, C.POINTER(_P), C.POINTER(_L), C.POINTER(_P), C.POINTER(_L), C.POINTER(_L)], _I),
        f"i2v_{fam}_read_hook": ([_P, _I, _I, _P, _I, _P], _I),
    }


class VitConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("img", "patch", "in_chans", "dim", "heads", "mlp", "blocks")] + [("ln_eps", C.c_float)]


# The ViT surrogate (`include/i2v_vit.h`): like the loader, a header of its own outside the host simulation's ABI.
_VIT_PROTOS = {
    **_net_protos("vit", VitConfig),
    "i2v_vit_create_ex": ([_I, C.POINTER(VitConfig), _I, C.POINTER(_P), _I, C.POINTER(C.c_int32), _I, _I, C.POINTER(_P)], _I),
    "i2v_vit_linear_f32": ([_P, _I, _I, _P, _P, _I, _P, _P, _P, _P], _I),
    "i2v_vit_linear_bwd_f32": ([_P, _I, _I, _P, _I, _P, _P, _P], _I),
    "i2v_vit_layernorm_f32": ([_P, _L, _I, _P, _P, _F, _P, _P, _P, _P], _I),
    "i2v_vit_layernorm_bwd_f32": ([_P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _P], _I),
    "i2v_vit_probs_ld": ([_I], _I),
    "i2v_vit_attention_f32": ([_P, _I, _I, _I, _I, _F, _P, _P, _P], _I),
    "i2v_vit_attention_bwd_f32": ([_P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P], _I),
    "i2v_vit_embed_f32": ([_P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P], _I),
    "i2v_vit_embed_bwd_f32": ([_P, _I, _I, _I, _I, _P, _I, _P, _P, _I, _P], _I),
    "i2v_vit_embed_ex_f32": ([_P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P], _I),
    "i2v_vit_embed_bwd_ex_f32": ([_P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _I, _P], _I),
}
VIT_EXPORTS = tuple(_VIT_PROTOS)


class SwinConfig(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("img", "patch", "in_chans", "dim", "window", "stages")]
                + [("depths", C.c_int32 * 4), ("heads", C.c_int32 * 4), ("ln_eps", C.c_float)])


# The Swin surrogates (`include/i2v_swin.h`): a header of its own as well, bound on the product library only.
_SWIN_PROTOS = {
    **_net_protos("swin", SwinConfig),
    "i2v_swin_window_attention_f32": ([_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P], _I),
    "i2v_swin_window_attention_bwd_f32": ([_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P], _I),
    "i2v_swin_merge_f32": ([_P, _I, _I, _I, _I, _P, _P], _I),
    "i2v_swin_merge_bwd_f32": ([_P, _I, _I, _I, _I, _P, _I, _P], _I),
    "i2v_swin_embed_f32": ([_P, _I, _I, _I, _I, _P, _P, _P, _P, _F, _I, _P, _P, _P, _P, _P, _P], _I),
    "i2v_swin_embed_bwd_f32": ([_P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P], _I),
}
SWIN_EXPORTS = tuple(_SWIN_PROTOS)


class ConvNextConfig(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("img", "patch", "in_chans", "dim", "stages")] + [("depths", C.c_int32 * 4), ("ln_eps", C.c_float)])


# The ConvNeXt surrogates (`include/i2v_convnext.h`): a header of its own, bound on the product library only -- except the depthwise
# launch on its own, `i2v_convnext_dw_f32`, which the host simulation exports as well (the same operations as scalar host code).
_CONVNEXT_PROTOS = {
    **_net_protos("convnext", ConvNextConfig),
    "i2v_convnext_dw_f32": ([_P, _P, _P, _P, _P, _I, _I, _I, _I, _P], _I),
}
CONVNEXT_EXPORTS = tuple(_CONVNEXT_PROTOS)
CONVNEXT_NODE_PROTOS = {"i2v_convnext_dw_f32": _CONVNEXT_PROTOS["i2v_convnext_dw_f32"]}


class MixerConfig(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("img", "patch", "in_chans", "dim", "blocks", "tokens_hidden", "mlp", "kind")] + [("ln_eps", C.c_float)])


# The all-MLP surrogates, MLP-Mixer and ResMLP (`include/i2v_mixer.h`): a header of its own, kept apart from EXPORTS.  The host
# simulation exports all of it: the planner runs there on scalar restatements, and so does the token-mixing launch on its own.
_MIXER_PROTOS = {
    **_net_protos("mixer", MixerConfig),
    "i2v_mixer_tokens_f32": ([_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P], _I),
    "i2v_mixer_tokens_bwd_f32": ([_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P], _I),
}
MIXER_EXPORTS = tuple(_MIXER_PROTOS)
MIXER_NODE_PROTOS = {k: _MIXER_PROTOS[k] for k in ("i2v_mixer_tokens_f32", "i2v_mixer_tokens_bwd_f32")}


class CaitConfig(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("img", "patch", "in_chans", "dim", "heads", "mlp", "blocks")] + [("ln_eps", C.c_float)])


# The CaiT surrogates (`include/i2v_cait.h`): a header of its own, kept apart from EXPORTS.  The host simulation exports all of it: the
# planner runs there on scalar restatements, and so do the two talking-heads attention entries on their own.
_CAIT_PROTOS = {
    **_net_protos("cait", CaitConfig),
    "i2v_cait_attention_f32": ([_P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P], _I),
    "i2v_cait_attention_bwd_f32": ([_P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P], _I),
    "i2v_cait_add_pos_f32": ([_P, _P, _I, _I, _I, _P], _I),
}
CAIT_EXPORTS = tuple(_CAIT_PROTOS)


class ConvitConfig(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("img", "patch", "in_chans", "dim", "heads", "mlp", "blocks", "local_blocks")] + [("ln_eps", C.c_float)])


# The ConViT surrogates (`include/i2v_convit.h`): a header of its own, kept apart from EXPORTS.  The host simulation exports all of it:
# the planner runs there on scalar restatements, and so do the two gated positional attention entries on their own.
_CONVIT_PROTOS = {
    **_net_protos("convit", ConvitConfig),
    "i2v_convit_attention_f32": ([_P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P], _I),
    "i2v_convit_attention_bwd_f32": ([_P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P], _I),
    "i2v_convit_join_cls_f32": ([_P, _P, _P, _I, _I, _I, _P], _I),
    "i2v_convit_join_cls_bwd_f32": ([_P, _P, _P, _I, _I, _I, _P], _I),
}
CONVIT_EXPORTS = tuple(_CONVIT_PROTOS)


class XcitConfig(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("img", "in_chans", "dim", "heads", "mlp", "blocks")] + [("ln_eps", C.c_float)])


# The XCiT surrogates (`include/i2v_xcit.h`): a header of its own, kept apart from EXPORTS.  The host simulation exports all of it: the
# planner runs there on scalar restatements, and so do the kernel entries on their own -- cross-covariance attention forward and
# backward, the depthwise 3 x 3 launch, and the stem's gather / scatter pair.
_XCIT_PROTOS = {
    **_net_protos("xcit", XcitConfig),
    "i2v_xcit_attention_f32": ([_P, _I, _I, _I, _I, _P, _P, _P, _P, _P], _I),
    "i2v_xcit_attention_bwd_f32": ([_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P], _I),
    "i2v_xcit_dw3_f32": ([_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "i2v_xcit_stem_gather_f32": ([_P, _P, _I, _I, _I, _I, _I, _P], _I),
    "i2v_xcit_stem_scatter_f32": ([_P, _P, _P, _I, _I, _I, _I, _I, _I, _P], _I),
}
XCIT_EXPORTS = tuple(_XCIT_PROTOS)


class TwinsConfig(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("img", "in_chans", "patch", "stages", "window")]
                + [(n, C.c_int32 * 4) for n in ("dims", "heads", "mlp", "depths", "sr")] + [("ln_eps", C.c_float), ("pe_eps", C.c_float)])


# The Twins surrogates (`include/i2v_twins.h`): a header of its own, kept apart from EXPORTS.  The host simulation exports all of it: the
# planner runs there on scalar restatements, and so do the kernel entries on their own -- sub-sampled attention forward and backward,
# the block gather / scatter pair, and window attention at shift 0 without a table (which the host simulation has in no other form).
_TWINS_PROTOS = {
    **_net_protos("twins", TwinsConfig),
    "i2v_twins_attention_f32": ([_P, _P, _I, _I, _I, _I, _I, _F, _P, _P], _I),
    "i2v_twins_attention_bwd_f32": ([_P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P], _I),
    "i2v_twins_block_gather_f32": ([_P, _P, _I, _I, _I, _I, _I, _P], _I),
    "i2v_twins_block_scatter_f32": ([_P, _P, _I, _I, _I, _I, _I, _I, _P], _I),
    "i2v_twins_window_attention_f32": ([_P, _I, _I, _I, _I, _I, _I, _P, _P, _P], _I),
    "i2v_twins_window_attention_bwd_f32": ([_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P], _I),
}
TWINS_EXPORTS = tuple(_TWINS_PROTOS)


class BeitConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("img", "patch", "in_chans", "dim", "heads", "mlp", "blocks")] + [("ln_eps", C.c_float)]


# The BEiT surrogates (`include/i2v_beit.h`): a header of its own, kept apart from EXPORTS.  The host simulation exports all of it: the
# planner runs there on scalar restatements, and so do the two attention entries and the bias add on their own.
_BEIT_PROTOS = {
    **_net_protos("beit", BeitConfig),
    "i2v_beit_attention_f32": ([_P, _P, _I, _I, _I, _I, _F, _P, _P], _I),
    "i2v_beit_attention_bwd_f32": ([_P, _P, _P, _I, _I, _I, _I, _F, _P, _P], _I),
    "i2v_beit_bias_add_f32": ([_P, _P, _I, _L, _P], _I),
}
BEIT_EXPORTS = tuple(_BEIT_PROTOS)


class PitConfig(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("img", "patch", "stride", "in_chans", "prefix")]
                + [(n, C.c_int32 * 3) for n in ("dims", "heads", "depths")] + [("ln_eps", C.c_float)])


# The PiT surrogates (`include/i2v_pit.h`): a header of its own, kept apart from EXPORTS.  The host simulation exports all of it: the
# planner runs there on scalar restatements, and so do the kernel entries on their own -- streaming attention forward and backward, the
# pooling convolution pair and the overlapping patch gather / scatter pair.
_PIT_PROTOS = {
    **_net_protos("pit", PitConfig),
    "i2v_pit_attention_f32": ([_P, _I, _I, _I, _I, _F, _P, _P, _P], _I),
    "i2v_pit_attention_bwd_f32": ([_P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P], _I),
    "i2v_pit_pool_f32": ([_P, _P, _P, _I, _I, _I, _I, _P, _P], _I),
    "i2v_pit_pool_bwd_f32": ([_P, _P, _I, _I, _I, _I, _I, _P, _P], _I),
    "i2v_pit_patch_gather_f32": ([_P, _I, _I, _I, _I, _I, _P, _P], _I),
    "i2v_pit_patch_scatter_f32": ([_P, _I, _I, _I, _I, _I, _I, _P, _P], _I),
}
PIT_EXPORTS = tuple(_PIT_PROTOS)


class CoatConfig(C.Structure):
    _fields_ = ([("img", C.c_int32), ("in_chans", C.c_int32), ("dims", C.c_int32 * 4), ("heads", C.c_int32), ("depths", C.c_int32 * 4),
                 ("mlp_ratios", C.c_int32 * 4)] + [(n, C.c_int32) for n in ("win3", "win5", "win7")] + [("ln_eps", C.c_float)])


# The CoaT-Lite surrogates (`include/i2v_coat.h`): a header of its own, kept apart from EXPORTS.  The host simulation exports all of it:
# the planner runs there on scalar restatements, and so do the kernel entries on their own -- factorized attention forward and backward,
# the per-channel-window depthwise convolution pair and the cell gather / scatter pair behind a class row.
_COAT_PROTOS = {
    **_net_protos("coat", CoatConfig),
    "i2v_coat_factor_attention_f32": ([_P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P], _I),
    "i2v_coat_factor_attention_bwd_f32": ([_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P], _I),
    "i2v_coat_dwmix_f32": ([_P, _L, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P], _I),
    "i2v_coat_dwmix_bwd_f32": ([_P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P], _I),
    "i2v_coat_cell_gather_f32": ([_P, _I, _I, _I, _I, _I, _P, _P], _I),
    "i2v_coat_cell_scatter_f32": ([_P, _I, _I, _I, _I, _I, _I, _P, _P], _I),
}
COAT_EXPORTS = tuple(_COAT_PROTOS)


class TntConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("img", "in_chans", "dim", "in_dim", "heads", "in_heads", "mlp_ratio", "blocks")] + [("ln_eps", C.c_float)]


# The TNT surrogates (`include/i2v_tnt.h`): a header of its own, kept apart from EXPORTS.  The host simulation exports all of it: the
# planner runs there on scalar restatements, and so do the kernel entries on their own -- the batched short-sequence attention forward
# and backward, the workgroup's share of sequences, and the pixel gather / scatter pair.
_TNT_PROTOS = {
    **_net_protos("tnt", TntConfig),
    "i2v_tnt_attention_f32": ([_P, _L, _I, _I, _I, _F, _P, _P], _I),
    "i2v_tnt_attention_bwd_f32": ([_P, _P, _L, _I, _I, _I, _F, _P, _P], _I),
    "i2v_tnt_attention_group": ([_I, _I, _I], _I),
    "i2v_tnt_pixel_gather_f32": ([_P, _I, _I, _I, _P, _P], _I),
    "i2v_tnt_pixel_scatter_f32": ([_P, _I, _I, _I, _I, _P, _P], _I),
}
TNT_EXPORTS = tuple(_TNT_PROTOS)


class XfGemmDesc(C.Structure):
    _fields_ = ([("A", _P)] + [(n, _L) for n in ("a_bo", "a_bi", "a_sm", "a_sk")] + [("B", _P)] + [(n, _L) for n in ("b_bo", "b_bi", "b_sk", "b_sn")]
                + [("C", _P)] + [(n, _L) for n in ("c_bo", "c_bi", "c_sm")] + [(n, _P) for n in ("bias", "R", "C2", "H")]
                + [(n, C.c_int32) for n in ("M", "N", "K", "batch", "nb_in")] + [("alpha", _F), ("mode", C.c_int32)])


# The shared transformer launches on their own (`include/i2v_xf_launch.h`): a header of its own, kept apart from EXPORTS.  The host
# simulation exports XF_HOST_PROTOS -- the launches that have a scalar restatement; the softmax pair is the device library's alone.
_XF_PROTOS = {
    "i2v_xf_gemm_f32": ([C.POINTER(XfGemmDesc), _P], _I),
    "i2v_xf_layernorm_f32": ([_P, _L, _I, _P, _P, _F, _P, _P, _P, _P], _I),
    "i2v_xf_layernorm_bwd_f32": ([_P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _P], _I),
    "i2v_xf_patchify_f32": ([_P, _P, _I, _I, _I, _I, _I, _P, _I, _P], _I),
    "i2v_xf_softmax_f32": ([_P, _L, _I, _I, _P], _I),
    "i2v_xf_softmax_bwd_f32": ([_P, _P, _L, _I, _I, _F, _P], _I),
}
XF_EXPORTS = tuple(_XF_PROTOS)
XF_HOST_PROTOS = {k: v for k, v in _XF_PROTOS.items() if "softmax" not in k}


class NlAct(C.Structure):
    _fields_ = [("p", _P), ("nstride", _L), ("T", C.c_int32), ("HW", C.c_int32)]


class NlGemmDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("form", "clips", "Cc", "M", "N")] + [("A", NlAct), ("B", NlAct), ("C", _P), ("c_nstride", _L),
                ("c_T", C.c_int32), ("c_HW", C.c_int32), ("D", _P), ("Din", _P), ("scale", _F), ("accumulate", C.c_int32),
                ("ksplit", C.c_int32), ("part", _P)])


class NlAddMaskDesc(C.Structure):
    _fields_ = [("out", _P), ("out_nstride", _L), ("a", _P * 3), ("a_nstride", _L * 3), ("mask", _P), ("mask_nstride", _L), ("gate", _P),
                ("gate_stride", C.c_int32), ("N", C.c_int32), ("C", C.c_int32), ("HW", C.c_int32), ("gain", _F)]


# The non-local block's launches and the gated add on their own (`include/i2v_nl_launch.h`): a header of its own, kept apart from
# EXPORTS.  Every build exports them: the host simulation runs their scalar twins.
_NL_PROTOS = {
    "i2v_nl_gemm_f32": ([C.POINTER(NlGemmDesc), _P], _I),
    "i2v_nl_softmax_rows_f32": ([_P, _P, _L, _I, _I, _P], _I),
    "i2v_nl_addmask_f32": ([C.POINTER(NlAddMaskDesc), _P], _I),
}
NL_EXPORTS = tuple(_NL_PROTOS)


class ConvAuxDesc(C.Structure):
    _fields_ = ([("src", _P), ("src_nstride", _L), ("dst", _P), ("dst_nstride", _L), ("plan_src", _P), ("filter", _P), ("shift", _P),
                 ("gate_out", _P), ("gate", _P), ("mask", _P), ("mask_nstride", _L), ("gate_out_stride", C.c_int32), ("gate_stride", C.c_int32)]
                + [(n, C.c_int32) for n in ("N", "C", "H", "W", "stride", "backward", "relu", "groups", "k")])


class ConvAuxPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("waves", "rows", "pitch", "lds_bytes", "v4")]


class SeLaunchDesc(C.Structure):
    _fields_ = ([("x", _P), ("x_nstride", _L), ("g", _P), ("g_nstride", _L), ("r", _P), ("r_nstride", _L), ("dst", _P), ("dst_nstride", _L)]
                + [(n, _P) for n in ("w1", "b1", "w2", "b2", "m", "h", "s", "t", "dmh")] + [("gate_out", _P), ("gate_out_stride", C.c_int32)]
                + [(n, C.c_int32) for n in ("N", "C", "rd", "HW", "relu", "backward", "launches")])


# The grouped, depthwise and squeeze-and-excitation launches on their own (`include/i2v_conv_aux_launch.h`): a header of its own, kept
# apart from EXPORTS.  The host simulation exports CONV_AUX_HOST_PROTOS: the packers and the node's scalar twin; the two convolution
# kernels are the device library's alone.
_CONV_AUX_PROTOS = {
    "i2v_gconv_f32": ([C.POINTER(ConvAuxDesc), C.POINTER(ConvAuxPlan), _P], _I),
    "i2v_dwconv_f32": ([C.POINTER(ConvAuxDesc), C.POINTER(ConvAuxPlan), _P], _I),
    "i2v_gconv_pack_f32": ([_P, _I, _I, _I, _I, _I, _P, _P, _P], _I),
    "i2v_dwconv_pack_f32": ([_P, _I, _I, _I, _I, _I, _P, _P], _I),
    "i2v_se_f32": ([C.POINTER(SeLaunchDesc), _P], _I),
}
CONV_AUX_EXPORTS = tuple(_CONV_AUX_PROTOS)
CONV_AUX_HOST_PROTOS = {k: v for k, v in _CONV_AUX_PROTOS.items() if k not in ("i2v_gconv_f32", "i2v_dwconv_f32")}


# The 8-bit export and the per-frame quality figures (`include/i2v_quality.h`): a header of its own, kept apart from EXPORTS.  Every build
# exports them: the host simulation runs their scalar twins.
_QUALITY_PROTOS = {
    "i2v_clip_to_u8": ([_P, _P, _I, _P, _I, _I, _I, _I, _P], _I),
    "i2v_clip_quality_scratch_bytes": ([_L, _I, _I], C.c_size_t),
    "i2v_clip_quality_tile": ([C.POINTER(_I), C.POINTER(_I)], None),
    "i2v_clip_quality_u8": ([_P, _P, _P, _L, _I, _I, _P, _L, _P], _I),
    "i2v_clip_quality_f32": ([_P, _P, _P, _I, _I, _I, _I, _P, _L, _P], _I),
}
QUALITY_EXPORTS = tuple(_QUALITY_PROTOS)


# The transformer families by the word in their entry names (`i2v_<word>_*`)
FAMILY_PROTOS = {"vit": _VIT_PROTOS, "swin": _SWIN_PROTOS, "convnext": _CONVNEXT_PROTOS, "mixer": _MIXER_PROTOS, "cait": _CAIT_PROTOS,
                 "convit": _CONVIT_PROTOS, "xcit": _XCIT_PROTOS, "twins": _TWINS_PROTOS, "beit": _BEIT_PROTOS, "pit": _PIT_PROTOS, "coat": _COAT_PROTOS,
                 "tnt": _TNT_PROTOS}


def family_config(word):
    """The config struct of a transformer family: the one `_net_protos` gave its `i2v_<word>_create` a pointer to."""
    argtypes = FAMILY_PROTOS[word][f"i2v_{word}_create"][0]
    return next(a._type_ for a in argtypes if isinstance(getattr(a, "_type_", None), type) and issubclass(a._type_, C.Structure))


def bind(cdll, protos=_PROTOS):
    for name, (args, res) in protos.items():
        fn = getattr(cdll, name)
        fn.argtypes, fn.restype = args, res
    return cdll


_lib = None


def load():
    """Open the gfx950 library or fail loudly -- there is no CPU path in the product."""
    global _lib
    if _lib is None:
        # $I2V_LIB: another BUILD of the same gfx950 library (developer A/B of compile-time kernel switches); it must still answer hip:gfx950
        path = os.environ.get("I2V_LIB") or LIB_PATH
        if not os.path.exists(path):
            raise I2VError(f"{path} not found: build it with `python __graft_entry__.py` "
                           "(hipcc --offload-arch=gfx950); the attack engine has no CPU fallback")
        lib = bind(C.CDLL(path))
        if lib.i2v_backend() != HIP_BACKEND:
            raise I2VError(f"{path} reports backend {lib.i2v_backend()!r}, expected {HIP_BACKEND!r}")
        for protos in (_LOADER_PROTOS, *FAMILY_PROTOS.values(), _XF_PROTOS, _NL_PROTOS, _CONV_AUX_PROTOS, _QUALITY_PROTOS):
            bind(lib, protos)
        _lib = lib
    return _lib


def check(capi, status):
    if status != 0:
        raise I2VError(capi.i2v_last_error().decode())
