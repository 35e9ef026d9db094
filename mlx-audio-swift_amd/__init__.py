"""mlx-audio-swift_amd: MI355X-native (gfx950) engine for the TTS generate()/generateStream() + neural
codec hot path of Blaizzy/mlx-audio-swift.

The product is `libmi_speech.so` (hand-written HIP kernels behind the C ABI of include/mi_speech.h,
sources in csrc/).  This package is the host-side mirror of the reference's protocol surface for that
path, written in Python because no Swift toolchain exists in the build image (INTEGRATION.md holds
the Swift shim a maintainer would add):

    codecs.SNAC            <-> class SNAC : AudioCodecModel       (MLXAudioCodecs/SNAC/SNACDecoder.swift)
    codecs.DescriptDAC     <-> class DescriptDAC (decode side)         (MLXAudioCodecs/Descript/DescriptDAC.swift)
    codecs.Encodec         <-> class Encodec (encode and decode)       (MLXAudioCodecs/Encodec/Encodec.swift)
    codecs.Mimi            <-> class Mimi : AudioCodecModel + MimiStreamingDecoder  (MLXAudioCodecs/Mimi/Mimi.swift)
    codecs.BigVGAN         <-> class BigVGAN : AudioDecoderModel (mel -> waveform vocoder)  (MLXAudioCodecs/BigVGAN/BigVGAN.swift)
    tts.LlamaTTSModel      <-> class LlamaTTSModel : SpeechGenerationModel  (MLXAudioTTS/Models/Llama/LlamaTTS.swift)
    soprano.SopranoModel   <-> class SopranoModel : SpeechGenerationModel  (MLXAudioTTS/Models/Soprano/Soprano.swift)
    qwen3tts.Qwen3TTSModel <-> class Qwen3TTSModel : SpeechGenerationModel  (MLXAudioTTS/Models/Qwen3TTS/Qwen3TTS.swift)
    marvis.MarvisTTSModel  <-> class MarvisTTSModel : SpeechGenerationModel  (MLXAudioTTS/Models/Marvis/MarvisTTSModel.swift)
    stt.WhisperModel       <-> class WhisperModel : STTGenerationModel   (MLXAudioSTT/Models/Whisper/WhisperModel.swift)
    moonshine.MoonshineModel <-> class MoonshineModel : STTGenerationModel (MLXAudioSTT/Models/Moonshine/MoonshineModel.swift)
    smartturn.SmartTurnModel <-> class SmartTurnModel (endpoint detection)  (MLXAudioVAD/Models/SmartTurn/SmartTurn.swift)
    lid.EcapaTdnnLID         <-> class EcapaTdnn (spoken language identification)  (MLXAudioLID/Models/EcapaTdnn/EcapaTdnnLID.swift)
    vad.FSMNVAD              <-> class FSMNVAD (voice activity detection)  (MLXAudioVAD/Models/FSMNVAD/FSMNVAD.swift)
    vad.SileroVAD            <-> class SileroVAD (voice activity detection) (MLXAudioVAD/Models/SileroVAD/SileroVAD.swift)
    vad.segment_speech       <-> func segmentSpeech (VAD -> STT chunker)    (MLXAudioVAD/SpeechSegmenter.swift)
    sortformer.SortformerModel <-> class SortformerModel (speaker diarization)  (MLXAudioVAD/Models/Sortformer/Sortformer.swift)
    sts.MossFormer2SE        <-> class MossFormer2SEModel : STSModel (speech enhancement)  (MLXAudioSTS/Models/MossFormer2SE)
    sts.DeepFilterNet        <-> class DeepFilterNetModel : STSModel (speech enhancement)  (MLXAudioSTS/Models/DeepFilterNet)
    sts.DeepFilterNetStreamer <-> class DeepFilterNetStreamer (hop-by-hop enhancement)  (DeepFilterNet/DeepFilterNetStreamer.swift)
    dsp.*                  <-> computeMelSpectrogram (MLXAudioCore/DSP.swift) / WhisperAudio.encoderFeatures
    generation.*           <-> AudioGeneration / AudioGenerationInfo / AudioGenerationError /
                               GenerateParameters                (MLXAudioCore/Generation/GenerationTypes.swift)

There is NO CPU fallback: importing works anywhere (so that the C ABI can be inspected), but every
compute entry point raises if the HIP library or a GPU is missing.
"""
from . import _lib  # noqa: F401
from .generation import (AudioGenerationError, AudioGenerationInfo, GenerateParameters, TokenEvent, InfoEvent,  # noqa: F401
                         AudioEvent)
from .codecs import SNAC, SNACConfig, DescriptDAC, DescriptDACConfig, Encodec, EncodecConfig  # noqa: F401
from .codecs import EncodecEncodedAudio, preprocess_encodec_audio  # noqa: F401
from .codecs import Mimi, MimiConfig, MimiStreamingDecoder, mimi_sanitize  # noqa: F401
from .codecs import BigVGAN, BigVGANConfig, bigvgan_sanitize, bigvgan_expected_shapes, bigvgan_aa_act  # noqa: F401
from .tts import (LlamaTTSModel, LlamaTTSConfiguration, OrpheusTokens, VyvoTokens, interleave_snac_codes,  # noqa: F401
                  orpheus_prompt_rows, padded_prompt_batch)
from .orpheus import deinterleave, parse_output  # noqa: F401
from .soprano import SopranoModel, SopranoConfiguration  # noqa: F401
from .qwen3tts import (Qwen3TTSModel, Qwen3TTSConfiguration, Qwen3TTSDecoderConfiguration, Qwen3TTSGenerateParameters,  # noqa: F401
                       PreparedPrompt)
from .marvis import (MarvisTTSModel, CSMModelArgs, CSMLlamaConfiguration, MarvisGenerateParameters, QualityLevel,  # noqa: F401
                     marvis_sanitize, marvis_checkpoint_plan, tokenize_text_segment, tokenize_audio, tokenize_segment, text_pieces)
from . import dsp  # noqa: F401
from .stt import WhisperModel, WhisperConfig, STTGenerateParameters, STTOutput  # noqa: F401
from .moonshine import (MoonshineModel, MoonshineConfig, MoonshineTokenizer, moonshine_sanitize, moonshine_frames,  # noqa: F401
                        moonshine_rotary_dim)
from .smartturn import (SmartTurnModel, SmartTurnConfig, SmartTurnEncoderConfig, SmartTurnProcessorConfig,  # noqa: F401
                        SmartTurnEndpointOutput, smart_turn_sanitize, smart_turn_expected_keys, smart_turn_read_directory)
from .lid import (EcapaTdnnLID, EcapaTdnnConfig, LanguagePrediction, LIDOutput, LIDError, ecapa_lid_sanitize,  # noqa: F401
                  ecapa_lid_expected_shapes, ecapa_lid_labels, ecapa_lid_read_directory)
from .lasr import (LasrCTCModel, LasrCTCConfig, LasrEncoderConfig, SentencePieceTokenizer, lasr_sanitize, lasr_expected_keys,  # noqa: F401
                   greedy_ctc_tokens)
from .sensevoice import (SenseVoiceModel, SenseVoiceConfig, SenseVoiceEncoderConfig, SenseVoiceFrontendConfig,  # noqa: F401
                         SenseVoiceTokenizer, sensevoice_sanitize, sensevoice_expected_keys, sensevoice_expected_shapes,
                         sensevoice_check_weights, sensevoice_layer_prefixes, sensevoice_read_directory, read_sentencepiece_pieces)
from .vad import (FSMNVAD, FSMNVADConfig, FSMNVADEncoderConfig, fsmn_vad_sanitize, fsmn_vad_expected_shapes,  # noqa: F401
                  fsmn_vad_check_weights, fsmn_vad_read_directory, fsmn_vad_read_cmvn, fsmn_vad_postprocess, parse_kaldi_cmvn,
                  chunks_from_segments, merge_runs, SileroVAD, SileroVADConfig, SileroVADBranchConfig, SileroVADError,
                  SileroVADStreamingState, SpeechSegmentConfig, silero_vad_sanitize, silero_vad_expected_shapes, silero_vad_check_weights,
                  silero_vad_read_directory, silero_vad_probs_to_timestamps, silero_vad_chunk_samples, speech_runs_from_probs,
                  detect_speech_runs, segment_speech)
from .sts import (MossFormer2SE, MossFormer2SEConfig, MossFormer2SEError, STSModelError, mossformer2_sanitize,  # noqa: F401
                  mossformer2_normalized_key, mossformer2_expected_shapes, mossformer2_check_weights, resolve_sts_model_type,
                  load_sts_model, DeepFilterNet, DeepFilterNetConfig, DeepFilterNetError, deepfilternet_expected_shapes,
                  deepfilternet_synthetic_weights, compute_norm_alpha, libdf_erb_band_widths, DeepFilterNetStreamingConfig,
                  DeepFilterNetStreamer, deepfilternet_enhance_streaming, deepfilternet_stream_chunks,
                  deepfilternet_stream_check_served)
from .sortformer import (SortformerModel, SortformerConfig, FCEncoderConfig, TFEncoderConfig, ModulesConfig, ProcessorConfig,  # noqa: F401
                         DiarizationSegment, DiarizationOutput, StreamingState, sortformer_sanitize, sortformer_expected_keys,
                         preds_to_segments, trim_silence, maybe_compress_state)

__all__ = ["SNAC", "SNACConfig", "LlamaTTSModel", "LlamaTTSConfiguration", "OrpheusTokens", "GenerateParameters",
           "AudioGenerationError", "AudioGenerationInfo", "TokenEvent", "InfoEvent", "AudioEvent", "deinterleave",
           "parse_output"]
