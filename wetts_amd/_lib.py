"""ctypes binding of libwetts_hip.so (include/wetts_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a call fails, this
module raises.  torch is imported first so that the process-wide HIP runtime is the one PyTorch
already loaded (both are `libamdhip64.so.7`; the dynamic linker then resolves our NEEDED entry
to the loaded image and device pointers / streams are shared).
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libwetts_hip.so")

MAX_STAGES = 8
MAX_RB_KERNELS = 8
MAX_RB_DILATIONS = 8


class WettsError(RuntimeError):
    pass


ABI_VERSION = 12  # WETTS_ABI_VERSION of include/wetts_hip.h this binding was written against


class Config(C.Structure):
    """Mirror of wetts_config_t."""
    _fields_ = [
        ("n_vocab", C.c_int32),
        ("inter_channels", C.c_int32),
        ("hidden_channels", C.c_int32),
        ("filter_channels", C.c_int32),
        ("n_heads", C.c_int32),
        ("n_layers", C.c_int32),
        ("kernel_size", C.c_int32),
        ("window_size", C.c_int32),
        ("resblock", C.c_int32),
        ("n_resblock_kernels", C.c_int32),
        ("resblock_kernel_sizes", C.c_int32 * MAX_RB_KERNELS),
        ("n_resblock_dilations", C.c_int32),
        ("resblock_dilation_sizes", (C.c_int32 * MAX_RB_DILATIONS) * MAX_RB_KERNELS),
        ("n_upsamples", C.c_int32),
        ("upsample_rates", C.c_int32 * MAX_STAGES),
        ("upsample_kernel_sizes", C.c_int32 * MAX_STAGES),
        ("upsample_initial_channel", C.c_int32),
        ("n_speakers", C.c_int32),
        ("gin_channels", C.c_int32),
        ("use_sdp", C.c_int32),
        ("flow_n_flows", C.c_int32),
        ("flow_wn_layers", C.c_int32),
        ("flow_kernel_size", C.c_int32),
        ("sdp_n_flows", C.c_int32),
        ("dp_filter_channels", C.c_int32),
        ("vocoder_type", C.c_int32),
        ("vocos_channels", C.c_int32),
        ("vocos_h_channels", C.c_int32),
        ("vocos_num_layers", C.c_int32),
        ("istft_n_fft", C.c_int32),
        ("istft_hop_length", C.c_int32),
        ("istft_win_length", C.c_int32),
        ("transformer_flows", C.c_int32),
        ("use_spk_conditioned_encoder", C.c_int32),
        ("is_onnx", C.c_int32),
        ("reserved", C.c_int32 * 6),
    ]


_P = C.c_void_p
_I32 = C.c_int32
_I64 = C.c_int64
_F = C.c_float
_D = C.c_double
_CFG = C.POINTER(Config)


class FrontendConfig(C.Structure):
    """Mirror of wetts_frontend_config_t."""
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "hidden_size", "num_layers", "num_heads", "intermediate_size",
                                          "max_position_embeddings", "type_vocab_size")] + \
               [("layer_norm_eps", C.c_float)] + \
               [(n, C.c_int32) for n in ("transform_heads", "transform_ff", "num_polyphones", "num_prosody")]


_FCFG = C.POINTER(FrontendConfig)

WAVLM_MAX_CONV = 8


class WavLMConfig(C.Structure):
    """Mirror of wetts_wavlm_config_t."""
    _fields_ = [("num_conv_layers", C.c_int32), ("conv_dim", C.c_int32 * WAVLM_MAX_CONV),
                ("conv_kernel", C.c_int32 * WAVLM_MAX_CONV), ("conv_stride", C.c_int32 * WAVLM_MAX_CONV)] + \
               [(n, C.c_int32) for n in ("hidden_size", "num_layers", "num_heads", "intermediate_size", "pos_kernel",
                                          "pos_groups", "num_buckets", "max_bucket_distance")] + \
               [("layer_norm_eps", C.c_float)]


_WCFG = C.POINTER(WavLMConfig)

# name -> (restype, argtypes); must list every symbol include/wetts_hip.h declares
SIGNATURES = {
    "wetts_abi_version": (_I32, []),
    "wetts_last_error": (C.c_char_p, []),
    "wetts_blob_num_tensors": (_I32, [_CFG]),
    "wetts_blob_tensor_info": (_I32, [_CFG, _I32, C.c_char_p, C.c_size_t, C.POINTER(_I64),
                                      C.POINTER(_I64), C.POINTER(_I64 * 4)]),
    "wetts_blob_numel": (_I64, [_CFG]),
    "wetts_create": (_I32, [_CFG, _P, _I64, _P, C.POINTER(_P)]),
    "wetts_destroy": (None, [_P]),
    "wetts_hop_length": (_I32, [_P]),
    "wetts_get_blob": (_I32, [_P, _P, _I64, _P]),
    "wetts_workspace_bytes": (_I64, [_P, _I32, _I32, _I32]),
    "wetts_speaker_embedding": (_I32, [_P, _P, _I32, _P, _P]),
    "wetts_text_encoder": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _I64, _P]),
    "wetts_duration_sdp": (_I32, [_P, _P, _P, _P, _P, _F, _I32, _I32, _P, _P, _P, _I64, _P]),
    "wetts_duration_dp": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P, _I64, _P]),
    "wetts_durations_to_lengths": (_I32, [_P, _P, _F, _I32, _I32, _P, _P, _P, _P, _P]),
    "wetts_set_status_word": (_I32, [_P, _P, _P]),
    "wetts_set_seed": (_I32, [_P, C.c_uint64]),
    "wetts_randn": (_I32, [_P, _I64, C.c_uint64, C.c_uint64, _P]),
    "wetts_rand": (_I32, [_P, _I64, C.c_uint64, C.c_uint64, _P]),
    "wetts_slice_ids": (_I32, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "wetts_slice_segments": (_I32, [_P, _I64, _I64, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "wetts_kl_loss": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _F, _P, _P, _P, _P]),
    "wetts_l1_loss": (_I32, [_P, _P, _I32, _I64, _F, _P, _P, _P, _P]),
    "wetts_duration_blob_num_tensors": (_I32, [_CFG]),
    "wetts_duration_blob_tensor_info": (_I32, [_CFG, _I32, C.c_char_p, C.c_size_t, C.POINTER(_I64), C.POINTER(_I64),
                                               C.POINTER(_I64 * 4)]),
    "wetts_duration_blob_numel": (_I64, [_CFG]),
    "wetts_load_duration_posterior": (_I32, [_P, _P, _I64, _P]),
    "wetts_duration_loss_workspace_bytes": (_I64, [_P, _I32, _I32]),
    "wetts_duration_sdp_forward": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                          _I64, _P]),
    "wetts_duration_reduce": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "wetts_duration_dp_loss": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P]),
    "wetts_duration_logw_target": (_I32, [_P, _P, _I32, _I32, _P, _P]),
    "wetts_duration_affine_forward": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P]),
    "wetts_duration_spline_forward": (_I32, [_P, _I32, _P, _P, _F, _I32, _I32, _F, _P, _P]),
    "wetts_duration_dequant_log": (_I32, [_P, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "wetts_duration_pre": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "wetts_duration_loss_total": (_I32, [_P, _P, _I32, _I32, _F, _P, _P, _P]),
    "wetts_stft_basis_numel": (_I64, [_I32, _I32]),
    "wetts_stft_basis": (_I32, [_I32, _I32, _P, _I64, _P]),
    "wetts_spectrogram": (_I32, [_P, _P, _I32, _I64, _I32, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "wetts_spec_to_mel": (_I32, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "wetts_mask_rows": (_I32, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "wetts_length_regulate": (_I32, [_P, _P, _P, _P, _P, _P, _I64, _I64, _F, _I32, _I32, _I32,
                                     _P, _P, _P, _P, _P, _P, _P]),
    "wetts_flow_reverse": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P, _I64, _P]),
    "wetts_posterior_blob_num_tensors": (_I32, [_CFG, _I32]),
    "wetts_posterior_blob_tensor_info": (_I32, [_CFG, _I32, _I32, C.c_char_p, C.c_size_t, C.POINTER(_I64),
                                                C.POINTER(_I64), C.POINTER(_I64 * 4)]),
    "wetts_posterior_blob_numel": (_I64, [_CFG, _I32]),
    "wetts_load_posterior_encoder": (_I32, [_P, _I32, _P, _I64, _P]),
    "wetts_posterior_workspace_bytes": (_I64, [_P, _I32, _I32]),
    "wetts_posterior_encoder": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P]),
    "wetts_flow_forward": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P, _I64, _P]),
    "wetts_hifigan": (_I32, [_P, _P, _I64, _I64, _P, _I64, _P, _I32, _I32, _P, _P, _I64, _P]),
    "wetts_hifigan_ragged_supported": (_I32, [_P]),
    "wetts_hifigan_ragged": (_I32, [_P, _P, _I64, _I64, _P, _P, _I32, _I32, _P, _P, _I64, _P]),
    "wetts_set_decoder_precision": (_I32, [_P, _I32]),
    "wetts_set_flow_precision": (_I32, [_P, _I32]),
    "wetts_set_istft_mode": (_I32, [_P, _I32]),
    "wetts_get_istft_mode": (_I32, [_P]),
    "wetts_dynamic_quant_conv1d": (_I32, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "wetts_mas": (_I32, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _I64, _P]),
    "wetts_align_scores": (_I32, [_P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "wetts_align_lengths": (_I32, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "wetts_path_to_durations": (_I32, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    "wetts_counts_to_lengths": (_I32, [_P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "wetts_audio_to_int16": (_I32, [_P, _P, _I32, _I64, _P, _P]),
    "wetts_infer_workspace_bytes": (_I64, [_P, _I32, _I32, _I32]),
    "wetts_infer": (_I32, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _I32, _I32, _I32, _P, _P,
                           C.POINTER(_I32), _P, _I64, _P]),
    "wetts_hifigan_cost": (_I32, [_CFG, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "wetts_set_mrf_timing": (_I32, [_P, _I32]),
    "wetts_read_mrf_timing": (_I32, [_P, C.POINTER(C.c_double), C.POINTER(_I64), C.POINTER(_I32)]),
    "wetts_read_mrf_bytes": (_I32, [_P, C.POINTER(C.c_double)]),
    "wetts_profile_hifigan": (_I32, [_P, _P, _I64, _I64, _P, _I32, _I32, _P, _P, _I64, _P,
                                     C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(_I32)]),
    "wetts_disc_blob_num_tensors": (_I32, []),
    "wetts_disc_blob_tensor_info": (_I32, [_I32, C.c_char_p, C.c_size_t, C.POINTER(_I64), C.POINTER(_I64),
                                           C.POINTER(_I64 * 4)]),
    "wetts_disc_blob_numel": (_I64, []),
    "wetts_disc_create": (_I32, [_P, _I64, _P, C.POINTER(_P)]),
    "wetts_disc_destroy": (None, [_P]),
    "wetts_disc_fmap_shape": (_I32, [_I32, _I32, _I32, C.POINTER(_I64 * 4)]),
    "wetts_disc_forward": (_I32, [_P, _P, _P, _I32, _I32, C.POINTER(_P), _P]),
    "wetts_disc_fold_conv0": (_I32, [_P, _I32, _P, _I32, _I32, _P, _P]),
    "wetts_disc_strided_conv": (_I32, [_P, _I32, _I32, _P, _I64, _I32, _P, _P]),
    "wetts_disc_conv_post": (_I32, [_P, _I32, _P, _I32, _I32, _P, _P]),
    "wetts_disc_grouped_conv": (_I32, [_P, _I32, _P, _I32, _I32, _P, _P]),
    "wetts_disc_losses": (_I32, [_I32, _I32, C.POINTER(_P), C.POINTER(_P), C.POINTER(_I64), C.POINTER(_I64),
                                 C.POINTER(_I64), _I32, _F, _P, _P, _P, _P, _P, _P]),
    "wetts_mrd_blob_num_tensors": (_I32, []),
    "wetts_mrd_blob_tensor_info": (_I32, [_I32, C.c_char_p, C.c_size_t, C.POINTER(_I64), C.POINTER(_I64),
                                          C.POINTER(_I64 * 4)]),
    "wetts_mrd_blob_numel": (_I64, []),
    "wetts_mrd_create": (_I32, [_P, _I64, _P, C.POINTER(_P)]),
    "wetts_mrd_destroy": (None, [_P]),
    "wetts_mrd_fmap_shape": (_I32, [_I32, _I32, _I32, C.POINTER(_I64 * 4)]),
    "wetts_mrd_workspace_bytes": (_I64, [_I32, _I32]),
    "wetts_mrd_forward": (_I32, [_P, _P, _P, _I32, _I32, C.POINTER(_P), _P, _I64, _P]),
    "wetts_mrd_normalize": (_I32, [_P, _I32, _I32, _P, _P]),
    "wetts_mrd_spectrogram": (_I32, [_P, _I32, _P, _I32, _I32, _P, _P]),
    "wetts_mrd_band_conv": (_I32, [_P, _I32, _I32, _P, _I32, _I32, _P, _P]),
    "wetts_mrd_conv_post": (_I32, [_P, _I32, _P, _I32, _I32, _P, _P]),
    "wetts_mrd_band_width": (_I32, [_I32, _I32, _I32]),
    "wetts_durdisc_blob_num_tensors": (_I32, [_I32, _I32, _I32, _I32]),
    "wetts_durdisc_blob_tensor_info": (_I32, [_I32, _I32, _I32, _I32, _I32, C.c_char_p, C.c_size_t, C.POINTER(_I64),
                                              C.POINTER(_I64), C.POINTER(_I64 * 4)]),
    "wetts_durdisc_blob_numel": (_I64, [_I32, _I32, _I32, _I32]),
    "wetts_durdisc_create": (_I32, [_I32, _I32, _I32, _I32, _P, _I64, _P, C.POINTER(_P)]),
    "wetts_durdisc_destroy": (None, [_P]),
    "wetts_durdisc_workspace_bytes": (_I64, [_P, _I32, _I32]),
    "wetts_durdisc_forward": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _P, _I64, _P]),
    "wetts_durdisc_layer": (_I32, [_P, _I32, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "wetts_durdisc_row_means": (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "wetts_frontend_blob_num_tensors": (_I32, [_FCFG]),
    "wetts_frontend_blob_tensor_info": (_I32, [_FCFG, _I32, C.c_char_p, C.c_size_t, C.POINTER(_I64), C.POINTER(_I64),
                                               C.POINTER(_I64 * 4)]),
    "wetts_frontend_blob_numel": (_I64, [_FCFG]),
    "wetts_frontend_create": (_I32, [_FCFG, _P, _I64, _P, C.POINTER(_P)]),
    "wetts_frontend_destroy": (None, [_P]),
    "wetts_frontend_workspace_bytes": (_I64, [_P, _I32, _I32]),
    "wetts_frontend_forward": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    "wetts_frontend_embed": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P]),
    "wetts_frontend_linear": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "wetts_frontend_add_layer_norm": (_I32, [_P, _P, _P, _P, _F, _I32, _I32, _P, _P]),
    "wetts_frontend_attention": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "wetts_frontend_heads": (_I32, [_P, _P, _P, _I32, _I32, _P, _P, _P]),
    "wetts_frontend_layer": (_I32, [_P, _I32, _P, _P, _I32, _I32, _P, _P]),
    "wetts_frontend_decide": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "wetts_frontend_score_workspace_bytes": (_I64, [_P, _I32, _I32]),
    "wetts_frontend_score": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P]),
    "wetts_frontend_score_heads": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P]),
    "wetts_frontend_trainable_span": (_I32, [_FCFG, C.POINTER(_I64), C.POINTER(_I64)]),
    "wetts_frontend_train_workspace_bytes": (_I64, [_P, _I32, _I32]),
    "wetts_frontend_grad": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _D, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P]),
    "wetts_frontend_adamw_step": (_I32, [_P, _P, _P, _P, _D, _D, _D, _D, _D, _D, _D, _P]),
    "wetts_frontend_adamw": (_I32, [_P, _P, _P, _P, _I64, _D, _D, _D, _D, _D, _D, _D, _P]),
    "wetts_frontend_read_weights": (_I32, [_P, _I64, _I64, _P, _P]),
    "wetts_frontend_linear_dgrad": (_I32, [_P, _I64, _P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "wetts_frontend_linear_wgrad_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "wetts_frontend_linear_wgrad": (_I32, [_P, _I64, _P, _I32, _I32, _I32, _P, _P, _P, _I64, _P]),
    "wetts_frontend_layer_norm_backward": (_I32, [_P, _P, _P, _F, _I32, _I32, _P, _P, _P, _P, _I64, _P]),
    "wetts_frontend_attention_backward": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _I64, _P]),
    "wetts_frontend_ce_backward": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _D, _P, _P]),
    "wetts_frontend_set_precision": (_I32, [_P, _I32]),
    "wetts_frontend_get_precision": (_I32, [_P]),
    "wetts_frontend_linear16_form": (_I32, [_I32, _I32]),
    "wetts_frontend_linear16_workspace_bytes": (_I64, [_I32, _I32]),
    "wetts_frontend_linear16": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _I64, _P]),
    "wetts_wavlm_bucket": (_I32, [_I32, _I32, _I32]),
    "wetts_wavlm_num_frames": (_I64, [_WCFG, _I64]),
    "wetts_wavlm_blob_num_tensors": (_I32, [_WCFG]),
    "wetts_wavlm_blob_tensor_info": (_I32, [_WCFG, _I32, C.c_char_p, C.c_size_t, C.POINTER(_I64), C.POINTER(_I64),
                                            C.POINTER(_I64 * 4)]),
    "wetts_wavlm_blob_numel": (_I64, [_WCFG]),
    "wetts_wavlm_create": (_I32, [_WCFG, _P, _I64, _P, C.POINTER(_P)]),
    "wetts_wavlm_destroy": (None, [_P]),
    "wetts_wavlm_workspace_bytes": (_I64, [_P, _I32, _I64]),
    "wetts_wavlm_forward": (_I32, [_P, _P, _I64, _I32, _I64, _P, _P, _I64, _P]),
    "wetts_wavlm_resample": (_I32, [_P, _I64, _I32, _I64, _I32, _I32, _I32, _P, _I32, _P, _I64, _P, _P]),
    "wetts_wavlm_conv0": (_I32, [_P, _P, _I64, _I32, _I64, _P, _P]),
    "wetts_wavlm_conv": (_I32, [_P, _I32, _P, _I32, _I64, _P, _P]),
    "wetts_wavlm_project": (_I32, [_P, _P, _I32, _P, _P, _P]),
    "wetts_wavlm_pos_conv": (_I32, [_P, _P, _I32, _I32, _P, _P]),
    "wetts_wavlm_attention": (_I32, [_P, _I32, _P, _P, _I32, _I32, _P, _P, _P]),
    "wetts_wavlm_layer_workspace_bytes": (_I64, [_P, _I32, _I32]),
    "wetts_wavlm_layer": (_I32, [_P, _I32, _P, _I32, _I32, _P, _P, _P]),
    "wetts_wavlm_disc_blob_num_tensors": (_I32, [_I32, _I32, _I32]),
    "wetts_wavlm_disc_blob_tensor_info": (_I32, [_I32, _I32, _I32, _I32, C.c_char_p, C.c_size_t, C.POINTER(_I64),
                                                 C.POINTER(_I64), C.POINTER(_I64 * 4)]),
    "wetts_wavlm_disc_blob_numel": (_I64, [_I32, _I32, _I32]),
    "wetts_wavlm_disc_create": (_I32, [_I32, _I32, _I32, _P, _I64, _P, C.POINTER(_P)]),
    "wetts_wavlm_disc_destroy": (None, [_P]),
    "wetts_wavlm_disc_workspace_bytes": (_I64, [_P, _I32, _I32]),
    "wetts_wavlm_disc_forward": (_I32, [_P, _P, _I64, _I32, _I32, _P, _P, _P]),
    "wetts_wavlm_disc_pre": (_I32, [_P, _P, _I64, _I32, _I32, _P, _P]),
    "wetts_wavlm_disc_convs": (_I32, [_P, _P, _I32, _I32, _P, _P, _P]),
    "wetts_conv16": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _F,
                            _P]),
    "wetts_conv16_wn_gate": (_I32, [_P, _P, _P, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    "wetts_conv16_wn_update": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    "wetts_wn16_gate": (_I32, [_P, _P, _I64, _I32, _I32, _P]),
    "wetts_wn16_update": (_I32, [_P, _P, _P, _P, _I32, _I32, _I64, _I32, _I32, _P]),
    "wetts_conv16_post": (_I32, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "wetts_resblock16": (_I32, [_I32, _I32, _I32, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                                C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), _P, _P, _P, _I32, _I32, _I32, _I32, _F,
                                _I32, _P]),
}

# WETTS_CONV16_* flags of wetts_conv16
CONV16_F16, CONV16_TRANSPOSED, CONV16_LRELU, CONV16_ACCUM, CONV16_BASIC, CONV16_TAG = 1, 2, 4, 8, 16, 32

# WETTS_STATUS_* bits of include/wetts_hip.h
STATUS_SPLINE_DOMAIN, STATUS_PHONE_ID_RANGE, STATUS_SPEAKER_ID_RANGE, STATUS_DURATION_NONFINITE = 1, 2, 4, 8
STATUS_ALIGN_TEXT_LONGER, STATUS_DURATION_NEGATIVE, STATUS_SEGMENT_LONGER = 16, 32, 64
STATUS_TOKEN_ID_RANGE, STATUS_TYPE_ID_RANGE = 128, 256
STATUS_LABEL_RANGE, STATUS_LABEL_AT_PAD = 512, 1024

_lib = None


def load():
    """Loads (once) and returns the CDLL.  Raises WettsError if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WettsError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `python -m wetts_amd.build`). "
            "There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError => header / library mismatch, fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.wetts_abi_version() != ABI_VERSION:
        raise WettsError("libwetts_hip.so ABI version mismatch")
    _lib = lib
    return lib


def last_error():
    return load().wetts_last_error().decode(errors="replace")


def check(rc, what):
    if rc != 0:
        raise WettsError(f"{what} failed (code {rc}): {last_error()}")


def ptr(t):
    """Device (or host) address of a torch tensor / None."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def current_stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
