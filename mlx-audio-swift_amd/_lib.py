"""ctypes binding of libmi_speech.so (include/mi_speech.h).  Fails loudly when the library is
missing - there is no fallback path."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIS_LIB_PATH: load a diagnostics build of the same library instead (e.g. `make timing`, tools/attn_phases.py)
LIB_PATH = os.environ.get("MIS_LIB_PATH") or os.path.join(_HERE, "libmi_speech.so")

MIS_OK = 0
STATUS_NAMES = {0: "ok", 1: "modelNotInitialized", 2: "generationFailed", 3: "invalidInput",
                4: "audioDecodingFailed", 5: "audioEncodingFailed", 6: "cancelled", 7: "device"}
MIS_F32, MIS_F16, MIS_BF16, MIS_I32 = 0, 1, 2, 3
EVENT_TOKEN, EVENT_INFO, EVENT_AUDIO = 0, 1, 2


class SnacConfigC(C.Structure):
    _fields_ = [("sampling_rate", C.c_int32), ("latent_dim", C.c_int32), ("decoder_dim", C.c_int32),
                ("n_decoder_rates", C.c_int32), ("decoder_rates", C.c_int32 * 8), ("codebook_size", C.c_int32),
                ("codebook_dim", C.c_int32), ("n_codebooks", C.c_int32), ("vq_strides", C.c_int32 * 8),
                ("noise", C.c_int32), ("depthwise", C.c_int32), ("attn_window_size", C.c_int32)]


class LmConfigC(C.Structure):
    _fields_ = [("hidden_size", C.c_int32), ("num_hidden_layers", C.c_int32), ("intermediate_size", C.c_int32),
                ("num_attention_heads", C.c_int32), ("num_key_value_heads", C.c_int32), ("head_dim", C.c_int32),
                ("vocab_size", C.c_int32), ("rms_norm_eps", C.c_float), ("rope_theta", C.c_float),
                ("rope_factor", C.c_float), ("rope_low_freq_factor", C.c_float), ("rope_high_freq_factor", C.c_float),
                ("rope_original_max_pos", C.c_float), ("tie_word_embeddings", C.c_int32), ("sample_rate", C.c_int32),
                ("qk_norm", C.c_int32), ("rope_plain", C.c_int32), ("rope_ops_in_dtype", C.c_int32),
                ("start_of_speech_id", C.c_int32), ("end_of_speech_id", C.c_int32), ("audio_token_offset", C.c_int32),
                ("start_of_ai_id", C.c_int32), ("codec_chunk_groups", C.c_int32)]


class GenParamsC(C.Structure):
    _fields_ = [("max_tokens", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float),
                ("repetition_penalty", C.c_float), ("repetition_context", C.c_int32), ("seed", C.c_uint64),
                ("frame_constrained", C.c_int32), ("row_offset", C.c_int64),
                ("sampler_flavor", C.c_int32), ("reserved", C.c_int32)]


class GenInfoC(C.Structure):
    _fields_ = [("prompt_token_count", C.c_int32), ("generation_token_count", C.c_int32),
                ("prefill_time", C.c_double), ("generate_time", C.c_double), ("tokens_per_second", C.c_double),
                ("peak_memory_gb", C.c_double)]


class SopranoConfigC(C.Structure):
    _fields_ = [("lm", LmConfigC), ("decoder_num_layers", C.c_int32), ("decoder_dim", C.c_int32),
                ("decoder_intermediate_dim", C.c_int32), ("hop_length", C.c_int32), ("n_fft", C.c_int32),
                ("upscale", C.c_int32), ("input_kernel", C.c_int32), ("dw_kernel", C.c_int32),
                ("token_size", C.c_int32), ("stop_token_id", C.c_int32)]


class Qwen3TTSConfigC(C.Structure):
    _fields_ = [("talker", LmConfigC), ("predictor", LmConfigC), ("num_code_groups", C.c_int32),
                ("text_hidden_size", C.c_int32), ("text_vocab_size", C.c_int32), ("codec_eos_token_id", C.c_int32),
                ("tts_pad_token_id", C.c_int32),
                ("dec_latent_dim", C.c_int32), ("dec_codebook_dim", C.c_int32), ("dec_codebook_size", C.c_int32),
                ("dec_decoder_dim", C.c_int32), ("dec_hidden_size", C.c_int32), ("dec_intermediate_size", C.c_int32),
                ("dec_head_dim", C.c_int32), ("dec_num_heads", C.c_int32), ("dec_num_layers", C.c_int32),
                ("dec_num_kv_heads", C.c_int32), ("dec_num_quantizers", C.c_int32), ("dec_num_semantic_quantizers", C.c_int32),
                ("dec_rms_norm_eps", C.c_float), ("dec_rope_theta", C.c_float),
                ("n_upsample_rates", C.c_int32), ("upsample_rates", C.c_int32 * 8),
                ("n_upsampling_ratios", C.c_int32), ("upsampling_ratios", C.c_int32 * 8), ("sample_rate", C.c_int32)]


class Qwen3TTSReferenceConfigC(C.Structure):
    _fields_ = [("spk_mel_dim", C.c_int32), ("spk_enc_dim", C.c_int32), ("spk_n_blocks", C.c_int32),
                ("spk_channels", C.c_int32 * 8), ("spk_kernel_sizes", C.c_int32 * 8), ("spk_dilations", C.c_int32 * 8),
                ("spk_attention_channels", C.c_int32), ("spk_res2net_scale", C.c_int32), ("spk_se_channels", C.c_int32),
                ("spk_sample_rate", C.c_int32),
                ("enc_audio_channels", C.c_int32), ("enc_num_filters", C.c_int32), ("enc_kernel_size", C.c_int32),
                ("enc_last_kernel_size", C.c_int32), ("enc_residual_kernel_size", C.c_int32),
                ("enc_num_residual_layers", C.c_int32), ("enc_dilation_growth_rate", C.c_int32), ("enc_compress", C.c_int32),
                ("enc_n_ratios", C.c_int32), ("enc_upsampling_ratios", C.c_int32 * 8),
                ("enc_use_causal_conv", C.c_int32), ("enc_use_conv_shortcut", C.c_int32),
                ("enc_hidden_size", C.c_int32), ("enc_num_layers", C.c_int32), ("enc_num_heads", C.c_int32),
                ("enc_intermediate_size", C.c_int32),
                ("enc_codebook_dim", C.c_int32), ("enc_codebook_size", C.c_int32), ("enc_num_quantizers", C.c_int32),
                ("enc_valid_num_quantizers", C.c_int32), ("enc_sampling_rate", C.c_int32),
                ("enc_rope_theta", C.c_float), ("enc_frame_rate", C.c_float), ("enc_norm_eps", C.c_float)]


class Qwen3TTSParamsC(C.Structure):
    _fields_ = [("max_frames", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32),
                ("repetition_penalty", C.c_float), ("min_p", C.c_float), ("seed", C.c_uint64), ("row_offset", C.c_int64)]


class DacConfigC(C.Structure):
    _fields_ = [("latent_dim", C.c_int32), ("decoder_dim", C.c_int32), ("n_decoder_rates", C.c_int32),
                ("decoder_rates", C.c_int32 * 8), ("n_codebooks", C.c_int32), ("codebook_size", C.c_int32),
                ("codebook_dim", C.c_int32), ("sample_rate", C.c_int32)]


class MimiConfigC(C.Structure):
    _fields_ = [("channels", C.c_int32), ("sample_rate", C.c_int32), ("frame_rate", C.c_float),
                ("dimension", C.c_int32), ("n_filters", C.c_int32), ("n_residual_layers", C.c_int32), ("n_ratios", C.c_int32),
                ("ratios", C.c_int32 * 8), ("kernel_size", C.c_int32), ("residual_kernel_size", C.c_int32),
                ("last_kernel_size", C.c_int32), ("dilation_base", C.c_int32), ("compress", C.c_int32),
                ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("dim_feedforward", C.c_int32), ("context", C.c_int32),
                ("max_period", C.c_float), ("norm_eps", C.c_float),
                ("num_quantizers", C.c_int32), ("bins", C.c_int32), ("quantizer_dim", C.c_int32)]


class MarvisConfigC(C.Structure):
    _fields_ = [("backbone", LmConfigC), ("decoder", LmConfigC), ("text_vocab_size", C.c_int32), ("audio_vocab_size", C.c_int32),
                ("audio_num_codebooks", C.c_int32)]


class MarvisParamsC(C.Structure):
    _fields_ = [("max_frames", C.c_int32), ("codebooks", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float),
                ("seed", C.c_uint64), ("row_offset", C.c_int64)]


class EncodecConfigC(C.Structure):
    _fields_ = [("audio_channels", C.c_int32), ("num_filters", C.c_int32), ("kernel_size", C.c_int32),
                ("num_residual_layers", C.c_int32), ("dilation_growth_rate", C.c_int32), ("codebook_size", C.c_int32),
                ("codebook_dim", C.c_int32), ("hidden_size", C.c_int32), ("num_lstm_layers", C.c_int32),
                ("residual_kernel_size", C.c_int32), ("use_causal_conv", C.c_int32), ("pad_reflect", C.c_int32),
                ("last_kernel_size", C.c_int32), ("compress", C.c_int32), ("use_conv_shortcut", C.c_int32),
                ("trim_right_ratio", C.c_float), ("n_upsampling_ratios", C.c_int32), ("upsampling_ratios", C.c_int32 * 8),
                ("n_quantizers", C.c_int32), ("sampling_rate", C.c_int32), ("group_norm", C.c_int32),
                ("normalize", C.c_int32)]


class MelConfigC(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_fft", C.c_int32), ("hop_length", C.c_int32), ("n_mels", C.c_int32),
                ("window", C.c_int32), ("mel_scale", C.c_int32), ("slaney_norm", C.c_int32), ("drop_last_frame", C.c_int32)]


class WhisperConfigC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "num_mel_bins", "d_model", "encoder_layers",
                                         "encoder_attention_heads", "encoder_ffn_dim", "max_source_positions",
                                         "decoder_layers", "decoder_attention_heads", "decoder_ffn_dim",
                                         "max_target_positions")]


class MoonshineConfigC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("vocab_size", "hidden_size", "intermediate_size", "encoder_num_hidden_layers",
                                          "decoder_num_hidden_layers", "encoder_num_attention_heads", "decoder_num_attention_heads",
                                          "encoder_num_key_value_heads", "decoder_num_key_value_heads", "encoder_hidden_act",
                                          "decoder_hidden_act", "max_position_embeddings", "attention_bias")]
                + [("partial_rotary_factor", C.c_float), ("rope_theta", C.c_float)]
                + [(n, C.c_int32) for n in ("bos_token_id", "eos_token_id", "decoder_start_token_id", "tie_word_embeddings")])


class SmartTurnConfigC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_mel_bins", "max_source_positions", "d_model", "encoder_attention_heads", "encoder_layers",
                                          "encoder_ffn_dim", "k_proj_bias", "sampling_rate", "max_audio_seconds", "n_fft", "hop_length",
                                          "normalize_audio")]
                + [("threshold", C.c_float)])


class EcapaLidConfigC(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("channels", C.c_int32), ("kernel_sizes", C.c_int32 * 5), ("dilations", C.c_int32 * 5),
                ("attention_channels", C.c_int32), ("res2net_scale", C.c_int32), ("se_channels", C.c_int32),
                ("embedding_dim", C.c_int32), ("classifier_hidden_dim", C.c_int32), ("num_classes", C.c_int32),
                ("max_batch", C.c_int32), ("max_samples", C.c_int32)]


class FsmnVadConfigC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("input_dim", "input_affine_dim", "fsmn_layers", "linear_dim", "proj_dim", "lorder", "rorder",
                                          "lstride", "rstride", "output_affine_dim", "output_dim", "sample_rate", "n_mels", "frame_length",
                                          "frame_shift", "lfr_m", "lfr_n", "n_sil")]
                + [("sil_pdf_ids", C.c_int32 * 16), ("max_batch", C.c_int32), ("chunk_frames", C.c_int32)])


class SenseVoiceConfigC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "input_size", "output_size", "attention_heads", "linear_units", "num_blocks", "tp_blocks",
                                         "kernel_size", "sanm_shift", "normalize_before", "sample_rate", "n_mels", "frame_length", "frame_shift",
                                         "lfr_m", "lfr_n", "window_hann", "max_batch", "max_seconds", "head_rows")]


class SileroVadBranchConfigC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sample_rate", "filter_length", "hop_length", "pad", "cutoff", "context_size", "chunk_size")]


class SileroVadConfigC(C.Structure):
    _fields_ = [("branch16k", SileroVadBranchConfigC), ("branch8k", SileroVadBranchConfigC), ("max_batch", C.c_int32),
                ("max_chunks", C.c_int32)]


class BigVGANConfigC(C.Structure):
    _fields_ = [("num_mels", C.c_int32), ("n_upsamples", C.c_int32), ("upsample_rates", C.c_int32 * 8),
                ("n_upsample_kernel_sizes", C.c_int32), ("upsample_kernel_sizes", C.c_int32 * 8), ("upsample_initial_channel", C.c_int32),
                ("resblock", C.c_int32), ("n_resblock_kernels", C.c_int32), ("resblock_kernel_sizes", C.c_int32 * 8),
                ("n_resblock_dilations", C.c_int32 * 8), ("resblock_dilation_sizes", (C.c_int32 * 8) * 8), ("activation", C.c_int32),
                ("snake_logscale", C.c_int32), ("use_bias_at_final", C.c_int32), ("use_tanh_at_final", C.c_int32),
                ("max_batch", C.c_int32), ("max_frames", C.c_int32)]


class MossFormer2ConfigC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("sample_rate", "win_len", "win_inc", "fft_len", "num_mels", "win_hann", "in_channels",
                                          "out_channels", "out_channels_final", "num_blocks", "max_batch")]
                + [("preemphasis", C.c_float), ("max_samples", C.c_int64)])


class DeepFilterNetConfigC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("sample_rate", "fft_size", "hop_size", "nb_erb", "nb_df", "df_order", "df_lookahead", "conv_lookahead",
                                          "conv_ch", "emb_hidden_dim", "df_hidden_dim", "lsnr_max", "lsnr_min", "emb_num_layers",
                                          "df_num_layers", "linear_groups", "enc_linear_groups")]
                + [("conv_kernel", C.c_int32 * 2), ("convt_kernel", C.c_int32 * 2), ("conv_kernel_inp", C.c_int32 * 2),
                   ("df_pathway_kernel_size_t", C.c_int32), ("gru_kr", C.c_int32), ("max_batch", C.c_int32), ("norm_alpha", C.c_float),
                   ("erb_widths", C.c_int32 * 128), ("max_samples", C.c_int64)])


class LasrConfigC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads",
                                          "intermediate_size", "hidden_act", "conv_kernel_size", "convolution_bias", "num_mel_bins",
                                          "subsampling_conv_channels", "subsampling_conv_kernel_size", "subsampling_conv_stride",
                                          "attention_bias", "rope_type", "pad_token_id", "max_batch", "max_seconds")]
                + [("layer_norm_eps", C.c_float), ("rope_theta", C.c_float), ("conv_residual_weights", C.c_float * 2),
                   ("feed_forward_residual_weights", C.c_float * 2)])


class SortformerConfigC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("hidden_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "intermediate_size",
                                          "num_mel_bins", "conv_kernel_size", "subsampling_factor", "subsampling_conv_channels",
                                          "subsampling_conv_kernel_size", "subsampling_conv_stride", "attention_bias", "scale_input",
                                          "tf_d_model", "encoder_layers", "encoder_attention_heads", "encoder_ffn_dim", "max_source_positions",
                                          "k_proj_bias", "num_speakers", "fc_d_model", "tf_d_model_modules", "sampling_rate", "hop_length",
                                          "n_fft", "win_length", "max_batch", "max_seconds")]
                + [("layer_norm_eps", C.c_float), ("preemphasis", C.c_float)])


class SttParamsC(C.Structure):
    _fields_ = [("max_tokens", C.c_int32), ("temperature", C.c_float), ("seed", C.c_uint64), ("eot_id", C.c_int32),
                ("timestamp_begin", C.c_int32), ("suppress", C.c_void_p), ("n_suppress", C.c_int32),
                ("begin_suppress", C.c_void_p), ("n_begin_suppress", C.c_int32), ("row_offset", C.c_int64)]


class GroupTimingC(C.Structure):
    _fields_ = [("n_shards", C.c_int32), ("generate_ms", C.c_double), ("slowest_shard_ms", C.c_double), ("gather_ms", C.c_double)]


class TimingC(C.Structure):
    _fields_ = [("prefill_ms", C.c_double), ("decode_ms", C.c_double), ("codec_ms", C.c_double),
                ("step_ms_avg", C.c_double), ("steps", C.c_int32), ("gemm_probe_ms", C.c_double),
                ("gemm_probe_bytes", C.c_double), ("hbm_bytes_per_step", C.c_double)]


EVENT_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64)

_P = C.c_void_p
# name -> (restype, argtypes): every symbol include/mi_speech.h declares
SYMBOLS = {
    "mis_last_error": (C.c_char_p, []),
    "mis_abi_version": (C.c_int, []),
    "mis_free": (None, [_P]),
    "mis_device_count": (C.c_int, []),
    "mis_orpheus_deinterleave": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, _P, _P, _P]),
    "mis_speech_parse_output": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mis_orpheus_parse_output": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, _P, _P]),
    "mis_snac_load": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "mis_snac_create": (C.c_int, [C.POINTER(SnacConfigC), C.c_int, C.POINTER(_P)]),
    "mis_snac_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_snac_finalize": (C.c_int, [_P]),
    "mis_snac_destroy": (None, [_P]),
    "mis_snac_num_samples": (C.c_int64, [_P, C.c_int]),
    "mis_snac_noise_len": (C.c_int64, [_P, C.c_int, C.c_int]),
    "mis_snac_set_noise": (C.c_int, [_P, C.c_int, C.c_uint64]),
    "mis_snac_decode": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.POINTER(_P), _P]),
    "mis_snac_padded_length": (C.c_int64, [_P, C.c_int64]),
    "mis_snac_encode": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P, _P]),
    "mis_snac_debug_tap": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "mis_tts_load": (C.c_int, [C.c_char_p, _P, C.c_int, C.POINTER(_P)]),
    "mis_tts_create": (C.c_int, [C.POINTER(LmConfigC), _P, C.c_int, C.POINTER(_P)]),
    "mis_tts_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_lm_prefill": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "mis_tts_native_quant_bits": (C.c_int, [_P, C.c_int]),
    "mis_tts_init_synthetic_quantized": (C.c_int, [_P, C.c_uint64, C.c_int]),
    "mis_tts_set_tensor_quantized": (C.c_int, [_P, C.c_char_p, _P, _P, _P, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mis_tts_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_tts_finalize": (C.c_int, [_P]),
    "mis_tts_destroy": (None, [_P]),
    "mis_lm_reset": (C.c_int, [_P, C.c_int, C.c_int]),
    "mis_lm_forward": (C.c_int, [_P, _P, _P, _P]),
    "mis_lm_forward_hidden": (C.c_int, [_P, _P, _P, _P, _P]),
    "mis_sample_logits": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.POINTER(GenParamsC), C.c_int,
                                    C.c_int, C.c_int, _P]),
    "mis_tts_generate": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(GenParamsC), C.POINTER(_P), C.POINTER(_P),
                                   C.POINTER(C.c_int64), _P, C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_tts_generate_device": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(GenParamsC), C.POINTER(_P), _P, C.c_int64,
                                          _P, _P]),
    "mis_tts_generate_stream": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(GenParamsC), C.POINTER(_P), EVENT_CB, _P, _P]),
    "mis_tts_set_profiling": (C.c_int, [_P, C.c_int]),
    "mis_tts_last_timing": (C.c_int, [_P, C.POINTER(TimingC)]),
    "mis_tts_time_gemm": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mis_shard_rows": (None, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mis_tts_group_create": (C.c_int, [C.POINTER(_P), C.c_int, C.POINTER(_P)]),
    "mis_tts_group_destroy": (None, [_P]),
    "mis_tts_group_size": (C.c_int, [_P]),
    "mis_tts_group_generate": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(GenParamsC), C.POINTER(_P), C.POINTER(C.c_int64), _P,
                                         C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_tts_group_generate_device": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(GenParamsC), C.POINTER(_P), C.c_int64, _P, _P]),
    "mis_tts_group_last_timing": (C.c_int, [_P, C.POINTER(GroupTimingC)]),
    "mis_comm_unique_id": (C.c_int, [_P]),
    "mis_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "mis_comm_destroy": (None, [_P]),
    "mis_comm_all_gather_pcm": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, _P, C.POINTER(C.c_double)]),
    "mis_mel_num_frames": (C.c_int64, [C.POINTER(MelConfigC), C.c_int64]),
    "mis_mel_spectrogram": (C.c_int, [C.c_int, C.POINTER(MelConfigC), _P, C.c_int, C.c_int64, _P, C.POINTER(C.c_int64)]),
    "mis_whisper_encoder_features": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int64, C.c_int, _P]),
    "mis_whisper_create": (C.c_int, [C.POINTER(WhisperConfigC), C.c_int, C.POINTER(_P)]),
    "mis_whisper_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_whisper_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_whisper_set_tensor_quantized": (C.c_int, [_P, C.c_char_p, _P, _P, _P, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mis_whisper_native_quant_bits": (C.c_int, [_P, C.c_int, C.c_int]),
    "mis_whisper_init_synthetic_quantized": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_int]),
    "mis_whisper_finalize": (C.c_int, [_P]),
    "mis_whisper_destroy": (None, [_P]),
    "mis_whisper_encode": (C.c_int, [_P, _P, C.c_int, _P]),
    "mis_whisper_decoder_reset": (C.c_int, [_P]),
    "mis_whisper_decoder_forward": (C.c_int, [_P, _P, _P, _P]),
    "mis_stt_whisper_generate": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int, C.POINTER(SttParamsC),
                                           C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_stt_whisper_generate_stream": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int, C.POINTER(SttParamsC), EVENT_CB, _P, _P,
                                                  C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_soprano_create": (C.c_int, [C.POINTER(SopranoConfigC), C.c_int, C.POINTER(_P)]),
    "mis_soprano_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_soprano_set_tensor_quantized": (C.c_int, [_P, C.c_char_p, _P, _P, _P, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mis_soprano_finalize": (C.c_int, [_P]),
    "mis_soprano_destroy": (None, [_P]),
    "mis_soprano_lm": (_P, [_P]),
    "mis_soprano_lm_path": (C.c_int32, [_P]),
    "mis_soprano_num_samples": (C.c_int64, [_P, C.c_int]),
    "mis_soprano_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "mis_soprano_generate": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(GenParamsC), C.POINTER(_P), C.POINTER(C.c_int64),
                                       _P, C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_soprano_generate_stream": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(GenParamsC), EVENT_CB, _P, _P]),
    "mis_qwen3tts_create": (C.c_int, [C.POINTER(Qwen3TTSConfigC), C.c_int, C.POINTER(_P)]),
    "mis_qwen3tts_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_qwen3tts_set_tensor_quantized": (C.c_int, [_P, C.c_char_p, _P, _P, _P, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mis_qwen3tts_finalize": (C.c_int, [_P]),
    "mis_qwen3tts_destroy": (None, [_P]),
    "mis_qwen3tts_talker": (_P, [_P]),
    "mis_qwen3tts_samples_per_frame": (C.c_int, [_P]),
    "mis_qwen3tts_num_code_groups": (C.c_int, [_P]),
    "mis_qwen3tts_group_generate": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.POINTER(Qwen3TTSParamsC), _P,
                                              C.POINTER(_P), C.POINTER(C.c_int64), _P, C.POINTER(_P), C.POINTER(C.c_int64), _P,
                                              C.c_int, EVENT_CB, _P, _P]),
    "mis_moonshine_create": (C.c_int, [C.POINTER(MoonshineConfigC), C.c_int, C.POINTER(_P)]),
    "mis_moonshine_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_moonshine_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_moonshine_finalize": (C.c_int, [_P]),
    "mis_moonshine_destroy": (None, [_P]),
    "mis_moonshine_frames": (C.c_int, [_P, _P, C.c_int, _P]),
    "mis_moonshine_encode": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P]),
    "mis_moonshine_decoder_reset": (C.c_int, [_P, C.c_int]),
    "mis_moonshine_decoder_forward": (C.c_int, [_P, _P, _P]),
    "mis_moonshine_launches_per_step": (C.c_int, [_P]),
    "mis_stt_moonshine_generate": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.POINTER(SttParamsC), C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_smartturn_create": (C.c_int, [C.POINTER(SmartTurnConfigC), C.c_int, C.POINTER(_P)]),
    "mis_smartturn_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_smartturn_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_smartturn_finalize": (C.c_int, [_P]),
    "mis_smartturn_destroy": (None, [_P]),
    "mis_smartturn_launches": (C.c_int, [_P]),
    "mis_smartturn_predict": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_float, _P, _P, _P]),
    "mis_smartturn_forward_features": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mis_ecapa_lid_create": (C.c_int, [C.POINTER(EcapaLidConfigC), C.c_int, C.POINTER(_P)]),
    "mis_ecapa_lid_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_ecapa_lid_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_ecapa_lid_finalize": (C.c_int, [_P]),
    "mis_ecapa_lid_destroy": (None, [_P]),
    "mis_ecapa_lid_launches": (C.c_int, [_P]),
    "mis_ecapa_lid_predict": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, _P, _P, _P, _P]),
    "mis_ecapa_lid_forward_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "mis_ecapa_lid_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_fsmn_vad_create": (C.c_int, [C.POINTER(FsmnVadConfigC), C.c_int, C.POINTER(_P)]),
    "mis_fsmn_vad_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_fsmn_vad_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_fsmn_vad_finalize": (C.c_int, [_P]),
    "mis_fsmn_vad_destroy": (None, [_P]),
    "mis_fsmn_vad_launches": (C.c_int, [_P]),
    "mis_fsmn_vad_frames": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mis_fsmn_vad_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int]),
    "mis_fsmn_vad_forward_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "mis_fsmn_vad_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int]),
    "mis_fsmn_vad_detect_raw": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int, _P, C.c_int]),
    "mis_fsmn_vad_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_sensevoice_create": (C.c_int, [C.POINTER(SenseVoiceConfigC), C.c_int, C.POINTER(_P)]),
    "mis_sensevoice_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_sensevoice_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_sensevoice_finalize": (C.c_int, [_P]),
    "mis_sensevoice_destroy": (None, [_P]),
    "mis_sensevoice_launches": (C.c_int, [_P]),
    "mis_sensevoice_frames": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mis_sensevoice_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int]),
    "mis_sensevoice_forward_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_sensevoice_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, _P]),
    "mis_stt_sensevoice_generate": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, _P, C.c_int64, _P, _P]),
    "mis_sensevoice_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_silero_vad_create": (C.c_int, [C.POINTER(SileroVadConfigC), C.c_int, C.POINTER(_P)]),
    "mis_silero_vad_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_silero_vad_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_silero_vad_finalize": (C.c_int, [_P]),
    "mis_silero_vad_destroy": (None, [_P]),
    "mis_silero_vad_launches": (C.c_int, [_P]),
    "mis_silero_vad_chunks": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "mis_silero_vad_predict": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, _P, C.c_int, _P, _P]),
    "mis_silero_vad_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "mis_silero_vad_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_bigvgan_create": (C.c_int, [C.POINTER(BigVGANConfigC), C.c_int, C.POINTER(_P)]),
    "mis_bigvgan_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_bigvgan_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_bigvgan_finalize": (C.c_int, [_P]),
    "mis_bigvgan_destroy": (None, [_P]),
    "mis_bigvgan_hop": (C.c_int, [_P]),
    "mis_bigvgan_launches": (C.c_int, [_P]),
    "mis_bigvgan_decode": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P]),
    "mis_bigvgan_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_mossformer2_create": (C.c_int, [C.POINTER(MossFormer2ConfigC), C.c_int, C.POINTER(_P)]),
    "mis_mossformer2_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_mossformer2_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_mossformer2_finalize": (C.c_int, [_P]),
    "mis_mossformer2_destroy": (None, [_P]),
    "mis_mossformer2_launches": (C.c_int, [_P]),
    "mis_mossformer2_frames": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mis_mossformer2_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int]),
    "mis_mossformer2_mask_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "mis_mossformer2_mask": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int]),
    "mis_mossformer2_enhance": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int64, _P]),
    "mis_mossformer2_synthesize": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int, _P, C.c_int64, _P]),
    "mis_mossformer2_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_deepfilternet_create": (C.c_int, [C.POINTER(DeepFilterNetConfigC), C.c_int, C.POINTER(_P)]),
    "mis_deepfilternet_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_deepfilternet_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_deepfilternet_finalize": (C.c_int, [_P]),
    "mis_deepfilternet_destroy": (None, [_P]),
    "mis_deepfilternet_launches": (C.c_int, [_P]),
    "mis_deepfilternet_frames": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mis_deepfilternet_enhance": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, C.c_int]),
    "mis_deepfilternet_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_deepfilternet_stream_create": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "mis_deepfilternet_stream_destroy": (None, [_P]),
    "mis_deepfilternet_stream_reset": (C.c_int, [_P, C.c_int]),
    "mis_deepfilternet_stream_feed": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int, _P]),
    "mis_deepfilternet_stream_launches": (C.c_int, [_P]),
    "mis_deepfilternet_stream_hops_seen": (C.c_int64, [_P, C.c_int]),
    "mis_lasr_create": (C.c_int, [C.POINTER(LasrConfigC), C.c_int, C.POINTER(_P)]),
    "mis_lasr_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_lasr_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_lasr_finalize": (C.c_int, [_P]),
    "mis_lasr_destroy": (None, [_P]),
    "mis_lasr_launches": (C.c_int, [_P]),
    "mis_lasr_frames": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "mis_lasr_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P]),
    "mis_lasr_forward_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "mis_lasr_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P]),
    "mis_stt_lasr_generate": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, _P, C.c_int64, _P]),
    "mis_lasr_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_sortformer_create": (C.c_int, [C.POINTER(SortformerConfigC), C.c_int, C.POINTER(_P)]),
    "mis_sortformer_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_sortformer_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_sortformer_finalize": (C.c_int, [_P]),
    "mis_sortformer_destroy": (None, [_P]),
    "mis_sortformer_launches": (C.c_int, [_P]),
    "mis_sortformer_frames": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "mis_sortformer_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    "mis_sortformer_forward_features": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "mis_sortformer_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    "mis_sortformer_pre_encode": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "mis_sortformer_encode_embeddings": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "mis_sortformer_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P]),
    "mis_whisper_group_generate": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int64, _P, C.c_int, C.POINTER(SttParamsC),
                                             C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_soprano_group_generate": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.POINTER(GenParamsC), C.POINTER(_P), C.POINTER(C.c_int64),
                                             _P, C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_qwen3tts_generate_codes": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.POINTER(Qwen3TTSParamsC), _P,
                                              C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    "mis_qwen3tts_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "mis_qwen3tts_set_stream_exact": (C.c_int, [_P, C.c_int]),
    "mis_qwen3tts_decode_stream_begin": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "mis_qwen3tts_decode_stream_step": (C.c_int, [_P, _P, C.c_int, _P]),
    "mis_qwen3tts_decode_stream_end": (C.c_int, [_P]),
    "mis_qwen3tts_decoder_tap": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int64)]),
    "mis_qwen3tts_generate": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.POINTER(Qwen3TTSParamsC), _P,
                                        C.POINTER(_P), C.POINTER(C.c_int64), _P, C.POINTER(_P), C.POINTER(C.c_int64), _P,
                                        C.c_int, EVENT_CB, _P, _P]),
    "mis_qwen3tts_enable_reference": (C.c_int, [_P, C.POINTER(Qwen3TTSReferenceConfigC)]),
    "mis_qwen3tts_speaker_embedding": (C.c_int, [_P, _P, C.c_int64, _P]),
    "mis_qwen3tts_encode_audio": (C.c_int, [_P, _P, C.c_int64, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mis_qwen3tts_reference_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.c_int, _P, C.c_int64, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int64)]),
    "mis_qwen3tts_add_reference": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mis_qwen3tts_clear_references": (C.c_int, [_P]),
    "mis_qwen3tts_sample_logits": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, _P, C.POINTER(Qwen3TTSParamsC), C.c_int, C.c_int,
                                             C.c_int, C.c_int, _P]),
    "mis_dac_create": (C.c_int, [C.POINTER(DacConfigC), C.c_int, C.POINTER(_P)]),
    "mis_dac_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_dac_finalize": (C.c_int, [_P]),
    "mis_dac_destroy": (None, [_P]),
    "mis_dac_num_samples": (C.c_int64, [_P, C.c_int]),
    "mis_dac_padded_length": (C.c_int64, [_P, C.c_int64]),
    "mis_dac_encode": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, _P, _P]),
    "mis_dac_decode_codes": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "mis_dac_debug_tap": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "mis_mel_stream_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "mis_mel_stream_process": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mis_mel_stream_flush": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mis_mel_stream_reset": (C.c_int, [_P]),
    "mis_mel_stream_total_frames": (C.c_int64, [_P]),
    "mis_mel_stream_destroy": (None, [_P]),
    "mis_encodec_create": (C.c_int, [C.POINTER(EncodecConfigC), C.c_int, C.POINTER(_P)]),
    "mis_encodec_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_encodec_finalize": (C.c_int, [_P]),
    "mis_encodec_destroy": (None, [_P]),
    "mis_encodec_hop_length": (C.c_int, [_P]),
    "mis_encodec_decode_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_encodec_debug_tap": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int64)]),
    "mis_encodec_has_encoder": (C.c_int, [_P]),
    "mis_encodec_encode_num_frames": (C.c_int64, [_P, C.c_int64]),
    "mis_encodec_encode_frame": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, _P, _P]),
    "mis_mimi_202407": (None, [C.c_int, C.POINTER(MimiConfigC)]),
    "mis_mimi_create": (C.c_int, [C.POINTER(MimiConfigC), C.c_int, C.POINTER(_P)]),
    "mis_mimi_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_mimi_finalize": (C.c_int, [_P]),
    "mis_mimi_destroy": (None, [_P]),
    "mis_mimi_num_samples": (C.c_int64, [_P, C.c_int]),
    "mis_mimi_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "mis_mimi_encode_num_frames": (C.c_int64, [_P, C.c_int64]),
    "mis_mimi_encode": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, _P]),
    "mis_mimi_decode_stream_begin": (C.c_int, [_P, C.c_int]),
    "mis_mimi_decode_stream_step": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "mis_mimi_decode_stream_end": (C.c_int, [_P]),
    "mis_marvis_create": (C.c_int, [C.POINTER(MarvisConfigC), C.c_int, C.POINTER(_P)]),
    "mis_marvis_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "mis_marvis_set_tensor_quantized": (C.c_int, [_P, C.c_char_p, _P, _P, _P, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mis_marvis_init_synthetic": (C.c_int, [_P, C.c_uint64]),
    "mis_marvis_init_synthetic_quantized": (C.c_int, [_P, C.c_uint64, C.c_int]),
    "mis_marvis_finalize": (C.c_int, [_P]),
    "mis_marvis_destroy": (None, [_P]),
    "mis_marvis_backbone": (_P, [_P]),
    "mis_marvis_decoder": (_P, [_P]),
    "mis_marvis_launches_per_frame": (C.c_int, [_P]),
    "mis_marvis_generate_codes": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(MarvisParamsC), _P, C.POINTER(_P),
                                            C.POINTER(C.c_int64), _P]),
    "mis_marvis_generate": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(MarvisParamsC), _P, C.POINTER(_P),
                                      C.POINTER(C.c_int64), _P, C.POINTER(_P), C.POINTER(C.c_int64), _P, C.c_int, _P, _P, _P]),
}

class AttnDebugArgsC(C.Structure):
    """mis_debug_attn_args (include/mi_speech_debug.h): one launch_attn_decode call on host data"""
    _fields_ = ([(n, C.c_int32) for n in ("batch", "Mpad", "S", "Nqkv", "H", "Hkv", "D", "Smax", "cache_rows", "append_only", "first_schedule",
                                          "cross", "cross_len", "out_ld", "rope_in_dtype", "qp_S", "qp_KT")] +
                [(n, C.c_float) for n in ("scale", "qk_eps", "qp_eps")] +
                [(n, _P) for n in ("qkv_part", "pos", "active", "rope_cos", "rope_sin", "qnorm_w", "knorm_w", "qp_w", "qp_bias", "qp_slabs",
                                   "qp_h_in", "qp_lnw", "qp_lnb", "kcache", "vtcache", "kcache_out", "vtcache_out", "out", "qp_h_out", "report")])


class CodecGemmDebugArgsC(C.Structure):
    """mis_debug_codec_gemm_args (include/mi_speech_debug.h): one launch_gemm call on host data"""
    _fields_ = ([(n, C.c_int32) for n in ("mode", "snake", "batch", "use_pack", "M", "K", "N", "Tin", "Tout", "s", "pad", "Cin", "ldx", "ldy",
                                          "x_lo", "dup_bias_n0", "split_k_ok", "taps", "dil", "noise_rng")] +
                [("noise_key", C.c_uint64), ("row_offset", C.c_int64)] +
                [(n, _P) for n in ("AT", "bias", "X", "R", "scale", "noise", "alpha", "ralpha", "row_ids", "Y", "report")])


# diagnostics / test scaffolding: include/mi_speech_debug.h (not part of the product surface)
DEBUG_SYMBOLS = {
    "mis_debug_launch_floor": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "mis_debug_occupy_cus": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double]),
    "mis_debug_occupy_wait": (C.c_int, []),
    "mis_debug_device_cus": (C.c_int32, [C.c_int]),
    "mis_debug_sampler_failures": (C.c_int32, []),
    "mis_debug_choose_split": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mis_debug_gemm_skinny": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                        C.c_int64, _P]),
    "mis_debug_gemm_skinny_q": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, _P, C.c_int64, _P]),
    "mis_debug_gemm_pf": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "mis_debug_attn_decode": (C.c_int, [C.c_int, C.POINTER(AttnDebugArgsC)]),
    "mis_debug_codec_gemm": (C.c_int, [C.c_int, C.POINTER(CodecGemmDebugArgsC)]),
    "mis_debug_codec_final": (C.c_int, [C.c_int, _P, _P, C.c_float, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, _P]),
    "mis_debug_codec_hist": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_codec_embed": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, _P]),
    "mis_debug_codec_dw7": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_codec_vq_nearest": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_gemm_big": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_enc_layernorm": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_float, _P, _P]),
    "mis_debug_enc_im2col3": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_enc_scatter_kv": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_enc_attn_prefill": (C.c_int, [C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_whisper_embed_ln": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_whisper_suppress": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int]),
    "mis_debug_lm_embed_rmsnorm": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _P, _P]),
    "mis_debug_lm_glue": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_float, _P, _P]),
    "mis_debug_gemm_skinny_norm_ok": (C.c_int32, [C.c_int] * 8),
    "mis_debug_gemm_skinny_norm": (C.c_int, [C.c_int, _P, _P, C.c_int, _P, _P, _P, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int,
                                             _P, C.c_int64, _P, _P, _P]),
    "mis_debug_pf_rows": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int64,
                                    C.c_int, C.c_float, _P, _P, _P, _P]),
    "mis_debug_prefill_feed": (C.c_int, [C.c_int, _P, _P, C.c_int, _P, C.c_int, _P, _P]),
    "mis_debug_convert_to_bf16": (C.c_int, [C.c_int, _P, C.c_int, C.c_int64, _P]),
    "mis_debug_dequant_affine": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_token_engine": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_double)]),
    "mis_debug_whisper_weight_bytes": (C.c_int64, [_P]),
    "mis_debug_mimi_decoder_tap": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int64)]),
    "mis_debug_marvis_forced_logits": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(MarvisParamsC), _P, C.c_int, _P, _P, _P]),
    "mis_debug_marvis_sample_logits": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint64, C.c_int64, C.c_int,
                                                 C.c_int, C.c_int, _P]),
    "mis_debug_moonshine_stem_tap": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, _P, C.c_int64, _P]),
    "mis_debug_moonshine_conv1": (C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_moonshine_groupnorm": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "mis_debug_moonshine_rope": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_moonshine_attn": (C.c_int, [C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_int, _P, _P,
                                           C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "mis_debug_moonshine_gemv": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_moonshine_embed": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_moonshine_argmax_embed": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, _P]),
    "mis_debug_smartturn_tap": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "mis_debug_smartturn_timing": (C.c_int, [_P, _P]),
    "mis_debug_ecapa_lid_timing": (C.c_int, [_P, _P]),
    "mis_debug_lasr_timing": (C.c_int, [_P, _P]),
    "mis_debug_lasr_gemm": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, _P, C.c_float, C.c_float, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, _P, _P, _P]),
    "mis_debug_lasr_ln": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_float, _P, C.c_int, _P]),
    "mis_debug_lasr_rope": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_lasr_attn": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "mis_debug_lasr_glu_dwconv": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_lasr_im2col": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_lasr_pack": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_lasr_argmax": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, _P]),
    "mis_debug_lasr_collapse": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_fsmn_vad_timing": (C.c_int, [_P, _P]),
    "mis_debug_sensevoice_timing": (C.c_int, [_P, _P]),
    "mis_debug_sensevoice_attn": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "mis_debug_sensevoice_head_argmax": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "mis_debug_silero_vad_timing": (C.c_int, [_P, _P]),
    "mis_debug_mossformer2_timing": (C.c_int, [_P, _P]),
    "mis_debug_deepfilternet_timing": (C.c_int, [_P, _P]),
    "mis_debug_deepfilternet_stream_timing": (C.c_int, [_P, _P]),
    "mis_debug_deepfilternet_stream_gru_step_frames": (C.c_int, [_P, C.c_int]),
    "mis_debug_bigvgan_timing": (C.c_int, [_P, _P]),
    "mis_debug_bigvgan_aa_act": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int64, _P, _P, _P]),
    "mis_debug_sortformer_timing": (C.c_int, [_P, _P]),
    "mis_debug_sortformer_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P,
                                            _P, C.c_int, C.c_float, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "mis_debug_sortformer_attn": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P,
                                            _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mis_debug_sortformer_conv0": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_sortformer_stats": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_float, _P]),
    "mis_debug_sortformer_ln": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_float, _P, C.c_int, C.c_int, _P]),
    "mis_debug_sortformer_intake": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "mis_debug_sortformer_glu_dwconv": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mis_debug_sortformer_peak": (C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int, C.c_int, _P]),
    "mis_debug_encodec_encode_tap": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, _P, C.c_int64, _P, C.POINTER(C.c_int32),
                                               C.POINTER(C.c_int64)]),
    "mis_debug_marvis_rope_tables": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _P, _P]),
}

_lib = None


class MisLibraryMissing(RuntimeError):
    pass


def lib():
    """The loaded shared library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MisLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        try:        # if torch is installed, let ITS bundled ROCm runtime load first (one libamdhip64 per process)
            import torch  # noqa: F401
        except Exception:
            pass
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(DEBUG_SYMBOLS.items()):
            fn = getattr(l, name)          # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def last_error() -> str:
    m = lib().mis_last_error()
    return m.decode("utf-8", "replace") if m else ""
