"""fluidaudio_amd — MI355X-native replacement for FluidAudio's host-side hot path
(STFT->mel featurizer, argmax + CTC greedy collapse, centroid-linkage AHC, VBx) behind the
reference's own interfaces.  All arithmetic runs in csrc/libfluidaudio_hip.so (hand-written HIP
for gfx950) through the C ABI of include/fluidaudio_hip.h; there is no CPU fallback.
"""
from ._lib import (AHC_MODE_AUTO, AHC_MODE_EXACT, AHC_MODE_REFERENCE_ORDER, ALLOCATION_FAILURE, INVALID_ARGUMENT, RUNTIME_ERROR, SUCCESS, Context, FluidAudioHipError, build, default_context, lib)  # noqa: F401
from .aed import (AED_END_CAP, AED_END_EOS, AED_FEED_SEQUENCE, AED_FEED_TOKEN, AED_MODEL_CANARY, AED_MODEL_COHERE, AED_RUNNING, AedConfig, AedDecodeState,  # noqa: F401
                  AedResult, AedWindows, MergedTokens, cross_attention_mask as aed_cross_attention_mask, encoder_context as aed_encoder_context,
                  encoder_valid_frames as aed_encoder_valid_frames, merge_token_streams as aed_merge_token_streams, merge_token_windows as aed_merge_token_windows,
                  merge_token_windows_dev as aed_merge_token_windows_dev, plan_windows as aed_plan_windows)
from .ahc import AHCClustering, check_dendrogram, cut, fastcluster_compute_centroid_linkage, linkage, linkage_batch  # noqa: F401
from .beam import ARPAError, ARPALanguageModel, CtcVocabulary, ctc_beam_search, ctc_beam_search_ids_batch  # noqa: F401
from .ctc import (LogitsArgmax, ctc_greedy_decode, ctc_greedy_ids_batch, ctc_greedy_rows, ctc_greedy_ids_dev, ctc_log_probs_dev,  # noqa: F401
                  decode_ctc_token_ids)
from .der import DERResult, DERSpeakerSegment, compute_der, compute_der_batch, segments_from_timed, segments_from_timeline  # noqa: F401
from .kws import KWS_DETECTION_DTYPE, KWS_WINDOW_DTYPE, adjusted_threshold, score_windows, spot_keywords_batch  # noqa: F401
from . import vocab_rescore  # noqa: F401
from .embedding import EmbeddingConfig, EmbeddingPlan, plan_embeddings, span_inputs, weight_resample  # noqa: F401
from .formats import AudioWAV, RTTMParser, RTTMParserError, TimedSpeakerSegment, export_embeddings_json  # noqa: F401
from .fsmn_vad import (fsmn_vad_config, fsmn_vad_frame_count, fsmn_vad_gather_silence_dev,  # noqa: F401
                       fsmn_vad_pack_feats_dev, fsmn_vad_pack_waveforms, fsmn_vad_pack_waveforms_dev, fsmn_vad_plan_chunks, fsmn_vad_segments,
                       fsmn_vad_segments_dev)
from .kmeans import KMeansClustering, SeededRNG, SpeakerCountConstraints  # noqa: F401
from .mel import AudioMelSpectrogram, LuxTtsMelExtractor, MelPlan, UnifiedMelExtractor  # noqa: F401
from .paraformer import (PARAFORMER_SPAN_DTYPE, CifResult, ParaformerConfig, TimestampedSegment, cif_batch, cif_batch_dev, decode_tokens,  # noqa: F401
                         keep_table, segments_from_spans, timestamps_batch, timestamps_batch_dev)
from .pipeline import (ClusteringResult, OfflineClusteringConfig, cluster_embeddings, cluster_embeddings_batch, cluster_embeddings_stagewise, diarize_segments,  # noqa: F401
                       extract_embeddings, select_training_embeddings, span_embedder)
from .online import (ONLINE_PACK_REPEAT, ONLINE_PACK_ZERO_TAIL, ONLINE_RUN_DTYPE, ONLINE_SEGMENT_DTYPE, OnlineChunkConfig, chunk_finish as online_chunk_finish,
                     chunk_plan as online_chunk_plan, pack_waveforms as online_pack_waveforms, EMBEDDING_SIZE, SPEAKER_ASSIGNMENT_DTYPE, SPEAKER_KINDS, SPEAKER_PAIR_DTYPE, Speaker, SpeakerDatabase, SpeakerDbConfig,
                     cosine_distance as speaker_cosine_distance, l2_normalize as speaker_l2_normalize, validate_embedding as speaker_validate_embedding)  # noqa: F401
from .pool import Pool, device_count  # noqa: F401
from .reconstruct import (OfflineReconstruction, ReconstructionConfig, SegmentationOutput, chunk_assignments, finalize_segments,  # noqa: F401
                          powerset_decode)
from .post import (ConstrainedClusterAssignment, HungarianAssignment, assign_embeddings, centroid_scores,  # noqa: F401
                   compute_centroids)
from .resample import linear_resample, poly_taps, resample_poly  # noqa: F401
from .sharding import gather_ragged_int32, shard_offsets, shard_range  # noqa: F401
from .sortformer import OfflineSortformerConfig, OfflineSortformerDiarizer, offline_windows, pack_windows, stitch, stitcher_alignment  # noqa: F401
from .sortformer_stream import (SORTFORMER_STREAM_PRESETS, SORTFORMER_STREAM_STATUS, SortformerStreamConfig, SortformerStreamSnapshot,  # noqa: F401
                                SortformerStreamState, SortformerStreamUpdate, chunk_plan as sortformer_stream_chunk_plan, file_chunks as sortformer_stream_file_chunks,
                                pack_chunks as sortformer_stream_pack_chunks)
from .rnnt import (RNNT_BIAS_DEFAULT_BOOST, RNNT_BIAS_MAX_BOOST, RNNT_BIAS_MAX_FORM, RnntBias, RnntConfig, VocabularyTerm,  # noqa: F401
                   bias_build as rnnt_bias_build, bias_candidates as rnnt_bias_candidates, bias_effective_boost as rnnt_bias_effective_boost,
                   decode_logits as rnnt_decode_logits, fold as rnnt_fold)
from .rnnt_stream import (RNNT_STREAM_CLASS_LANG_TAG, RNNT_STREAM_CLASS_LEXICAL, RNNT_STREAM_STATUS, SECONDS_PER_ENCODER_FRAME,  # noqa: F401
                          RnntStreamConfig, RnntStreamSnapshot, RnntStreamState, RnntStreamTracked, rms as rnnt_stream_rms, seconds as rnnt_stream_seconds,
                          token_classes as rnnt_stream_token_classes)
from .tdt import (Language, Script, TdtConfig, TdtDurationMapping, TdtFrameNavigation, decode_logits as tdt_decode_logits,  # noqa: F401
                  decode_logits_lang as tdt_decode_logits_lang, decode_tables as tdt_decode_tables, matches as tdt_matches,
                  token_classes as tdt_token_classes, topk_rows as tdt_topk_rows)
from .tdt_merge import (MERGE_NO_SEAM, MergedWindows, merge_capacity, merge_route_name, merge_windows, merge_windows_dev,  # noqa: F401
                        splice_safe_table, case_canon_table)
from .tdt_plan import (TDT_SPAN_DTYPE, TDT_WINDOW_DTYPE, PlannedWindows, TdtWindowPlanner, pack_windows as tdt_pack_windows,  # noqa: F401
                       pack_windows_dev as tdt_pack_windows_dev, plan_windows as tdt_plan_windows, plan_windows_dev as tdt_plan_windows_dev,
                       speech_gate as tdt_speech_gate, speech_gate_dev as tdt_speech_gate_dev, window_config as tdt_window_config,
                       window_count_bound as tdt_window_count_bound, window_layout as tdt_window_layout)
from .timeline import DiarizerSegment, DiarizerTimeline, DiarizerTimelineConfig, timeline_segments  # noqa: F401
from .vad import (VAD_SEGMENT_DTYPE, VAD_STREAM_EVENT_DTYPE, VAD_STREAM_STATE_DTYPE, gather_segments, gather_segments_dev, initial_stream_states,  # noqa: F401
                  pack_chunks, pack_chunks_dev, segment_speech_batch, segment_speech_batch_dev, stream_advance, stream_advance_dev, vad_config)
from .vbx import VBxClustering, VBxOutput  # noqa: F401
from .wer import (EDIT_COUNTS_DTYPE, CorpusErrorRate, WERAndCER, WERMetrics, edit_distance_batch, edit_distance_batch_dev, levenshtein_distance,  # noqa: F401
                  wer_and_cer_batch, wer_metrics_batch)

__version__ = "0.1.0"
