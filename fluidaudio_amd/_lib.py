"""ctypes binding of libfluidaudio_hip.so (the C ABI declared in include/fluidaudio_hip.h).

There is no CPU fallback: if the HIP library is missing or no GPU is visible, the product
path raises.  (The oracle under oracle/ is test infrastructure and is never imported here.)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("FLUIDAUDIO_HIP_LIBRARY") or os.path.join(CSRC, "libfluidaudio_hip.so")   # the override is for kernel experiments (scripts/)

SUCCESS, INVALID_ARGUMENT, INDEX_OVERFLOW, OUTPUT_TOO_SMALL, ALLOCATION_FAILURE, RUNTIME_ERROR, UNKNOWN_ERROR = 0, 1, 2, 3, 4, 5, 255
STATUS_NAMES = {0: "SUCCESS", 1: "INVALID_ARGUMENT", 2: "INDEX_OVERFLOW", 3: "OUTPUT_TOO_SMALL",
                4: "ALLOCATION_FAILURE", 5: "RUNTIME_ERROR", 255: "UNKNOWN_ERROR"}

MEL_FLOOR_ADDITIVE, MEL_FLOOR_CLAMPED = 0, 1
MEL_PAD_CENTER, MEL_PAD_PREPADDED, MEL_PAD_LEGACY = 0, 1, 2
MEL_LAYOUT_MEL_MAJOR, MEL_LAYOUT_FRAME_MAJOR = 0, 1
MEL_CENTER_ZERO, MEL_CENTER_REFLECT = 0, 1
MEL_SCALE_SLANEY, MEL_SCALE_HTK_NONORM = 0, 1
MEL_TAIL_ZERO, MEL_TAIL_REPLICATE = 0, 1
DTYPE_F32, DTYPE_F16 = 0, 1
AHC_MODE_AUTO, AHC_MODE_EXACT, AHC_MODE_REFERENCE_ORDER = 0, 1, 2
FAULT_VBX, FAULT_THREAD_START, FAULT_DEVBUF_MALLOC, FAULT_WS_MALLOC, FAULT_AHC = 0, 1, 2, 3, 4   # fa_debug_inject_fault sites (tests)

# Every symbol include/fluidaudio_hip.h + include/FastClusterWrapper.h declare (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = [
    "fa_version", "fa_debug_inject_fault", "fa_debug_set_switch", "fa_debug_hooks_enabled", "fa_debug_ahc_adopted", "fa_debug_ahc_spec_hits", "fa_ctx_set_timing", "fa_ctx_last_device_ms", "fa_debug_sclk_mhz", "fa_ctc_beam_plan", "fa_host_alloc", "fa_host_free", "fa_ctx_create", "fa_ctx_destroy", "fa_ctx_synchronize", "fa_ctx_stream", "fa_ctx_last_error",
    "fa_ctx_set_workspace_limit", "fa_ctx_set_workspace_cap", "fa_ctx_trim", "fa_ctx_workspace_bytes", "fa_ctx_reserve",
    "fa_mel_default_config", "fa_mel_num_frames", "fa_mel_padded_frames", "fa_mel_plan_create", "fa_mel_plan_destroy",
    "fa_mel_plan_utt_stride", "fa_mel_plan_frame_stride", "fa_mel_plan_total_frames", "fa_mel_execute_dev",
    "fa_mel_batch", "fa_mel_hann_window", "fa_mel_filterbank", "fa_mel_normalize_per_feature_dev",
    "fa_ctc_greedy_batch_dev", "fa_ctc_greedy_batch", "fa_ctc_greedy_rows_dev", "fa_ctc_greedy_rows", "fa_ctc_log_softmax_batch_dev",
    "fa_tdt_default_config", "fa_tdt_initial_time_index", "fa_tdt_navigation_state", "fa_tdt_final_time_jump",
    "fa_tdt_map_duration_bin", "fa_tdt_clamp_probability", "fa_tdt_greedy_tables_dev", "fa_tdt_greedy_logits_dev",
    "fa_tdt_token_classes", "fa_tdt_topk_rows_dev", "fa_tdt_greedy_logits_lang_dev",
    "fastcluster_compute_centroid_linkage", "fa_ahc_linkage", "fa_ahc_linkage_batch", "fa_ahc_row_minima", "fa_ahc_cluster", "fa_ahc_cut",
    "fa_vbx_speaker_count", "fa_vbx_refine",
    "fa_vbx_shard_slices", "fa_vbx_shard_range", "fa_vbx_shard_chunk_doubles", "fa_vbx_shard_create", "fa_vbx_shard_destroy",
    "fa_vbx_shard_frames", "fa_vbx_shard_begin", "fa_vbx_shard_iterate", "fa_vbx_shard_finish_iteration", "fa_vbx_shard_result",
    "fa_vbx_weighted_centroids", "fa_assign_cosine", "fa_centroid_scores", "fa_constrained_assign",
    "fa_offline_cluster_default_config", "fa_offline_cluster", "fa_offline_cluster_ex", "fa_offline_cluster_batch", "fa_offline_cluster_batch_dev",
    "fa_arpa_parse", "fa_arpa_destroy", "fa_arpa_unigram_count", "fa_arpa_bigram_context_count", "fa_arpa_score",
    "fa_ctc_vocab_create", "fa_ctc_vocab_destroy", "fa_ctc_beam_search_batch_dev", "fa_ctc_beam_search_batch",
    "fa_wav_pcm16_size", "fa_wav_encode_pcm16", "fa_wav_decode", "fa_rttm_parse", "fa_rttm_format", "fa_export_embeddings_json",
    "fa_seeded_rng_next", "fa_seeded_rng_below", "fa_kmeans_cluster", "fa_kmeans_cluster_ninit", "fa_speaker_constraints_resolve",
    "fa_resample_linear_frames", "fa_resample_linear", "fa_resample_poly_frames", "fa_resample_poly_taps", "fa_resample_poly", "fa_resample_poly_dev", "fa_debug_resample_route",
    "fa_device_count", "fa_pool_create", "fa_pool_destroy", "fa_pool_size", "fa_pool_context", "fa_ctx_device", "fa_pool_acquire", "fa_pool_release",
    "fa_mel_batch_sharded", "fa_ctc_greedy_batch_sharded", "fa_ahc_linkage_many",
    "fa_powerset_decode_dev", "fa_powerset_decode", "fa_offline_chunk_assignments", "fa_reconstruct_default_config",
    "fa_offline_reconstruct", "fa_offline_reconstruct_dev", "fa_segments_finalize",
    "fa_embedding_default_config", "fa_embedding_plan", "fa_embedding_plan_dev", "fa_embedding_windows_dev", "fa_embedding_span_inputs",
    "fa_embedding_span_inputs_dev", "fa_weight_resample", "fa_weight_resample_dev",
    "fa_sortformer_offline_default_config", "fa_sortformer_offline_windows", "fa_sortformer_pack_windows_dev", "fa_sortformer_stitch_dev",
    "fa_sortformer_stitcher_alignment", "fa_timeline_default_config", "fa_timeline_segments_dev", "fa_timeline_segments",
    "fa_der_default_config", "fa_der_score_batch",
    "fa_edit_distance_batch", "fa_edit_distance_batch_dev",
    "fa_kws_adjusted_threshold", "fa_ctc_kws_spot_batch_dev", "fa_ctc_kws_spot_batch", "fa_ctc_kws_score_windows_dev", "fa_ctc_kws_score_windows",
    "fa_paraformer_cif_default_config", "fa_paraformer_cif_dev", "fa_paraformer_cif", "fa_paraformer_timestamps_dev", "fa_paraformer_timestamps",
    "fa_tdt_merge_default_config", "fa_tdt_merge_windows_dev", "fa_tdt_merge_windows",
    "fa_vad_default_config", "fa_vad_chunk_count", "fa_vad_segments_dev", "fa_vad_segments", "fa_vad_pack_chunks_dev", "fa_vad_pack_chunks",
    "fa_vad_gather_segments_dev", "fa_vad_gather_segments", "fa_vad_stream_advance_dev", "fa_vad_stream_advance",
    "fa_fsmn_vad_default_config", "fa_fsmn_vad_frame_count", "fa_fsmn_vad_plan_chunks", "fa_fsmn_vad_pack_waveforms_dev", "fa_fsmn_vad_pack_waveforms",
    "fa_fsmn_vad_pack_feats_dev", "fa_fsmn_vad_gather_silence_dev", "fa_fsmn_vad_segments_dev", "fa_fsmn_vad_segments",
    "fa_tdt_window_default_config", "fa_tdt_window_layout", "fa_tdt_window_count_bound", "fa_tdt_plan_windows_dev", "fa_tdt_plan_windows",
    "fa_tdt_pack_windows_dev", "fa_tdt_pack_windows", "fa_tdt_speech_gate_dev", "fa_tdt_speech_gate",
    "fa_rnnt_bias_effective_boost", "fa_rnnt_bias_build", "fa_rnnt_bias_candidates", "fa_rnnt_default_config", "fa_rnnt_greedy_logits_dev",
    "fa_speaker_l2_normalize", "fa_speaker_cosine_distance", "fa_speaker_validate_embedding", "fa_speaker_db_default_config", "fa_speaker_db_create", "fa_speaker_db_destroy", "fa_speaker_db_assign_dev", "fa_speaker_db_distances_dev",
    "fa_speaker_db_mergeable_pairs_dev", "fa_speaker_db_assign", "fa_speaker_db_distances", "fa_speaker_db_mergeable_pairs", "fa_speaker_db_upsert", "fa_speaker_db_get", "fa_speaker_db_ids", "fa_speaker_db_count", "fa_speaker_db_remove",
    "fa_speaker_db_remove_inactive", "fa_speaker_db_set_permanent", "fa_speaker_db_reset",
    "fa_online_chunk_default_config", "fa_online_chunk_plan_dev", "fa_online_chunk_plan", "fa_online_pack_waveforms_dev", "fa_online_chunk_finish_dev",
    "fa_aed_default_config", "fa_aed_max_out", "fa_aed_state_bytes", "fa_aed_begin_dev", "fa_aed_step_dev", "fa_aed_finish_dev", "fa_aed_finish", "fa_aed_cross_mask_dev",
    "fa_aed_encoder_valid_frames", "fa_aed_encoder_context_dev", "fa_aed_gather_hidden_dev", "fa_aed_plan_windows", "fa_aed_merge_windows_dev", "fa_aed_merge_windows",
    "fa_sortformer_stream_default_config", "fa_sortformer_stream_preset_config", "fa_sortformer_stream_geometry", "fa_sortformer_stream_pop_out_length", "fa_sortformer_stream_create",
    "fa_sortformer_stream_destroy", "fa_sortformer_stream_inputs", "fa_sortformer_stream_get", "fa_sortformer_stream_set", "fa_sortformer_stream_reset", "fa_sortformer_stream_update_dev",
    "fa_sortformer_stream_update", "fa_sortformer_stream_chunk_plan", "fa_sortformer_stream_file_chunks", "fa_sortformer_stream_pack_chunks_dev",
    "fa_rnnt_stream_default_config", "fa_rnnt_stream_geometry", "fa_rnnt_stream_rms", "fa_rnnt_stream_create", "fa_rnnt_stream_destroy", "fa_rnnt_stream_reset", "fa_rnnt_stream_get",
    "fa_rnnt_stream_set", "fa_rnnt_stream_gate_dev", "fa_rnnt_stream_mel_inputs_dev", "fa_rnnt_stream_advance_dev", "fa_rnnt_stream_track_dev", "fa_rnnt_stream_finalize_dev",
    "fa_rnnt_stream_merge_rescued_dev", "fa_rnnt_stream_gate", "fa_rnnt_stream_track", "fa_rnnt_stream_merge_rescued",
    "fa_vocab_rescore_default_config", "fa_vocab_rescore_boost", "fa_vocab_rescore_build", "fa_vocab_rescore_candidates", "fa_vocab_rescore_decide_dev",
    "fa_vocab_rescore_decide",
]


class FluidAudioHipError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: {STATUS_NAMES.get(status, status)}" + (f" ({detail})" if detail else ""))


class MelConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_mels", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32),
                ("win", C.c_int32), ("preemph", C.c_float), ("pad_to", C.c_int32), ("log_floor", C.c_float),
                ("floor_mode", C.c_int32), ("window_periodic", C.c_int32), ("padding_mode", C.c_int32),
                ("layout", C.c_int32), ("power", C.c_float), ("center_pad", C.c_int32), ("mel_scale", C.c_int32),
                ("tail_mode", C.c_int32), ("filterbank", C.c_void_p)]


class TdtConfig(C.Structure):
    _fields_ = [("blank_id", C.c_int32), ("max_symbols_per_step", C.c_int32), ("max_tokens_per_chunk", C.c_int32),
                ("consecutive_blank_limit", C.c_int32), ("n_duration_bins", C.c_int32), ("duration_bins", C.c_int32 * 8)]


class AhcStats(C.Structure):
    _fields_ = [("merges", C.c_int64), ("rounds", C.c_int64), ("rescans", C.c_int64), ("exact_fallback", C.c_int64),
                ("init_ms", C.c_double), ("merge_ms", C.c_double), ("total_ms", C.c_double), ("windows", C.c_int64), ("reference_order", C.c_int64), ("handed_over_at", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OfflineClusterConfig(C.Structure):
    _fields_ = [("clustering_threshold", C.c_double), ("warm_start_fa", C.c_double), ("warm_start_fb", C.c_double),
                ("max_vbx_iterations", C.c_int32), ("convergence_tolerance", C.c_double), ("constrained_assignment", C.c_int32),
                ("num_speakers", C.c_int64), ("min_speakers", C.c_int64), ("max_speakers", C.c_int64), ("ahc_mode", C.c_int32)]


class OfflineClusterInfo(C.Structure):
    _fields_ = [("training_rows", C.c_int64), ("initial_clusters", C.c_int32), ("vbx_iterations", C.c_int32),
                ("was_adjusted", C.c_int32), ("constrained", C.c_int32), ("vbx_degraded", C.c_int32), ("ahc_degraded", C.c_int32),
                ("inputs_s", C.c_double), ("ahc_s", C.c_double),
                ("vbx_s", C.c_double), ("assign_s", C.c_double), ("total_s", C.c_double), ("ahc", AhcStats)]


class ReconstructConfig(C.Structure):
    _fields_ = [("window_duration", C.c_double), ("frame_duration", C.c_double), ("min_duration_on", C.c_double),
                ("min_duration_off", C.c_double), ("min_segment_duration", C.c_double), ("min_gap_duration", C.c_double),
                ("exclusive", C.c_int32), ("zero_vote_enabled", C.c_int32), ("zero_vote_min_duration", C.c_double)]


class ReconstructInfo(C.Structure):
    _fields_ = [("total_frames", C.c_int64), ("raw_segments", C.c_int64), ("frame_duration", C.c_double),
                ("zero_vote_run_count", C.c_int64), ("zero_vote_runs", C.c_void_p), ("zero_vote_capacity", C.c_int64),
                ("speaker_counts", C.c_void_p), ("speaker_counts_capacity", C.c_int64), ("frame_capacity", C.c_int64),
                ("frame_clusters", C.c_void_p), ("frame_averages", C.c_void_p), ("expected_count_sums", C.c_void_p), ("frame_slots", C.c_int32)]


class EmbeddingConfig(C.Structure):
    _fields_ = [("window_duration", C.c_double), ("sample_rate", C.c_int32), ("samples_per_window", C.c_int32), ("overlap_threshold", C.c_float),
                ("exclude_overlap", C.c_int32), ("min_segment_duration", C.c_double), ("batch_size", C.c_int32), ("skip_enabled", C.c_int32),
                ("skip_threshold", C.c_float), ("weight_frames", C.c_int32), ("frame_duration", C.c_double)]


class EmbeddingInfo(C.Structure):
    _fields_ = [("planned_chunks", C.c_int64), ("batches", C.c_int64), ("jobs", C.c_int64), ("runs", C.c_int64), ("evaluated_masks", C.c_int64),
                ("empty_masks", C.c_int64), ("fallback_masks", C.c_int64), ("skipped_embeddings", C.c_int64), ("frame_duration", C.c_double),
                ("min_frames", C.c_int32), ("samples_per_window", C.c_int32), ("batch_size", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SortformerOfflineConfig(C.Structure):
    _fields_ = [("window_output_frames", C.c_int32), ("subsampling", C.c_int32), ("speakers", C.c_int32), ("n_mels", C.c_int32),
                ("overlap_output_frames", C.c_int32)]


class SortformerWindow(C.Structure):
    _fields_ = [("recording", C.c_int32), ("valid_mel", C.c_int32), ("valid_out", C.c_int32), ("first", C.c_int32),
                ("mel_start", C.c_int64), ("g_start", C.c_int64)]


class TimelineConfig(C.Structure):
    _fields_ = [("onset_threshold", C.c_float), ("offset_threshold", C.c_float), ("onset_pad_frames", C.c_int32),
                ("offset_pad_frames", C.c_int32), ("min_frames_on", C.c_int32), ("min_frames_off", C.c_int32),
                ("frame_duration", C.c_float), ("speakers", C.c_int32), ("activity_type", C.c_int32)]


class DiarizerSegmentRecord(C.Structure):
    _fields_ = [("recording", C.c_int32), ("speaker", C.c_int32), ("start_frame", C.c_int64), ("end_frame", C.c_int64),
                ("activity", C.c_float), ("finalized", C.c_int32)]


class DerSegment(C.Structure):
    _fields_ = [("label", C.c_int32), ("reserved", C.c_int32), ("start", C.c_double), ("end", C.c_double)]


class DerConfig(C.Structure):
    _fields_ = [("frame_step", C.c_double), ("collar", C.c_double)]


class DerCounts(C.Structure):
    _fields_ = [("frames", C.c_int64), ("miss", C.c_int64), ("false_alarm", C.c_int64), ("confusion", C.c_int64), ("ref", C.c_int64),
                ("ref_labels", C.c_int32), ("hyp_labels", C.c_int32)]


class EditCounts(C.Structure):
    _fields_ = [("total", C.c_int32), ("insertions", C.c_int32), ("deletions", C.c_int32), ("substitutions", C.c_int32),
                ("hyp_len", C.c_int32), ("ref_len", C.c_int32)]


class KwsDetection(C.Structure):
    _fields_ = [("utterance", C.c_int32), ("keyword", C.c_int32), ("score", C.c_float), ("start_frame", C.c_int32), ("end_frame", C.c_int32)]


class KwsWindow(C.Structure):
    _fields_ = [("utterance", C.c_int32), ("keyword", C.c_int32), ("start_frame", C.c_int32), ("end_frame", C.c_int32)]


class VrCandidate(C.Structure):                                        # fa_vr_candidate
    _fields_ = [(n, C.c_int32) for n in ("utterance", "term", "first_word", "span_len", "origin", "form")] + [("similarity", C.c_float)]


class VrBoostConfig(C.Structure):                                      # fa_vr_boost_config
    _fields_ = [("use_adaptive_thresholds", C.c_int32), ("reference_token_count", C.c_int32), ("short_term_taper_pivot", C.c_int32),
                ("short_term_taper_exponent", C.c_float)]


class VrDecideConfig(C.Structure):                                     # fa_vr_decide_config
    _fields_ = [("frame_duration", C.c_double), ("margin_seconds", C.c_double), ("cbw", C.c_float), ("blank_id", C.c_int32), ("boost", VrBoostConfig)]


class VrVerdict(C.Structure):                                          # fa_vr_verdict
    _fields_ = [(n, C.c_float) for n in ("term_score", "original_score", "boost", "boosted_score")] + \
               [(n, C.c_int32) for n in ("alt_won", "compared", "should_replace", "outcome", "start_frame", "end_frame")]


class ParaformerCifConfig(C.Structure):
    _fields_ = [("threshold", C.c_float), ("tail_threshold", C.c_float), ("max_tokens", C.c_int32), ("enc_frames", C.c_int32)]


class ParaformerSpan(C.Structure):
    _fields_ = [("utterance", C.c_int32), ("token_index", C.c_int32), ("start", C.c_double), ("end", C.c_double)]


class TdtMergeConfig(C.Structure):
    _fields_ = [("frame_seconds", C.c_double), ("overlap_seconds", C.c_double)]


class VadSegmentationConfig(C.Structure):
    _fields_ = [("default_threshold", C.c_float), ("reserved0", C.c_int32), ("min_speech_duration", C.c_double), ("min_silence_duration", C.c_double),
                ("max_speech_duration", C.c_double), ("speech_padding", C.c_double), ("silence_threshold_for_split", C.c_float),
                ("has_negative_threshold", C.c_int32), ("negative_threshold", C.c_float), ("negative_threshold_offset", C.c_float),
                ("min_silence_at_max_speech", C.c_double), ("use_max_possible_silence_at_max_speech", C.c_int32), ("reserved1", C.c_int32)]


class VadSegmentRecord(C.Structure):
    _fields_ = [("recording", C.c_int32), ("reserved", C.c_int32), ("start_sample", C.c_int64), ("end_sample", C.c_int64),
                ("start_time", C.c_double), ("end_time", C.c_double)]


class VadStreamStateRecord(C.Structure):
    _fields_ = [("triggered", C.c_int32), ("has_temp_end", C.c_int32), ("temp_end_sample", C.c_int64), ("processed_samples", C.c_int64)]


class VadStreamEventRecord(C.Structure):
    _fields_ = [("stream", C.c_int32), ("chunk", C.c_int32), ("kind", C.c_int32), ("reserved", C.c_int32), ("sample_index", C.c_int64), ("time", C.c_double)]


class FsmnVadConfig(C.Structure):                                      # fa_fsmn_vad_config
    _fields_ = [("silence_threshold", C.c_float)] + [(n, C.c_int32) for n in ("window_frames", "sil_to_speech_frames", "speech_to_sil_frames", "max_end_silence_frames",
                                                                                "lookback_frames", "lookahead_frames", "max_segment_frames", "frame_ms")]


class FsmnVadChunkRecord(C.Structure):                                 # fa_fsmn_vad_chunk
    _fields_ = [("recording", C.c_int32), ("bucket", C.c_int32), ("start_sample", C.c_int64), ("end_sample", C.c_int64), ("frames", C.c_int32), ("keep_from", C.c_int32),
                ("first_frame", C.c_int64)]


class FsmnVadSegmentRecord(C.Structure):                               # fa_fsmn_vad_segment
    _fields_ = [("recording", C.c_int32), ("reason", C.c_int32), ("start_frame", C.c_int32), ("end_frame", C.c_int32), ("start_ms", C.c_int64), ("end_ms", C.c_int64)]


class TdtWindowConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("frame_samples", C.c_int32), ("mel_hop", C.c_int32), ("max_model_samples", C.c_int32), ("overlap_seconds", C.c_double),
                ("mel_chunk_context", C.c_int32), ("silence_aligned", C.c_int32), ("warmup_prefix_frames", C.c_int32), ("end_aligned", C.c_int32)]


class TdtWindowRecord(C.Structure):
    _fields_ = [("recording", C.c_int32), ("use_warmup_prefix", C.c_int32), ("is_last", C.c_int32), ("emit_after_frame", C.c_int32),
                ("global_frame_offset", C.c_int32), ("context_frames", C.c_int32), ("actual_audio_frames", C.c_int32), ("reserved", C.c_int32),
                ("chunk_start", C.c_int64), ("warmup_samples", C.c_int64), ("context_samples", C.c_int64), ("context_start", C.c_int64), ("length", C.c_int64)]


class TdtSpanRecord(C.Structure):
    _fields_ = [("recording", C.c_int32), ("reserved", C.c_int32), ("from_sample", C.c_int64), ("to_sample", C.c_int64)]


RESAMPLE_ROUTE_KINDS = ("DECIM", "INTERP", "ROWS", "LDS", "SIMPLE")    # FA_RESAMPLE_ROUTE_*


class RnntConfig(C.Structure):                                         # fa_rnnt_config
    _fields_ = [("blank_id", C.c_int32), ("eou_id", C.c_int32), ("max_symbols_per_step", C.c_int32)]


class SpeakerDbConfig(C.Structure):                                    # fa_speaker_db_config
    _fields_ = [("speaker_threshold", C.c_float), ("embedding_threshold", C.c_float), ("min_speech_duration", C.c_float), ("ema_alpha", C.c_float),
                ("validate_min_magnitude", C.c_float), ("max_speakers", C.c_int32), ("raw_capacity", C.c_int32)]


class OnlineChunkConfig(C.Structure):                                  # fa_online_chunk_config
    _fields_ = [("frames", C.c_int32), ("chunk_samples", C.c_int32), ("min_active_frames", C.c_float), ("min_speech_duration", C.c_float),
                ("validate_min_magnitude", C.c_float), ("reserved", C.c_int32), ("frame_step", C.c_double)]


class SpeakerInfo(C.Structure):                                        # fa_speaker_info
    _fields_ = [("id", C.c_int32), ("slot", C.c_int32), ("raw_count", C.c_int32), ("update_count", C.c_int32), ("is_permanent", C.c_int32),
                ("duration", C.c_float), ("created_tick", C.c_int64), ("updated_tick", C.c_int64)]


class SpeakerAssignment(C.Structure):                                  # fa_speaker_assignment
    _fields_ = [("id", C.c_int32), ("slot", C.c_int32), ("kind", C.c_int32), ("distance", C.c_float)]


class SpeakerPair(C.Structure):                                        # fa_speaker_pair
    _fields_ = [("source_id", C.c_int32), ("destination_id", C.c_int32), ("source_slot", C.c_int32), ("destination_slot", C.c_int32), ("distance", C.c_float)]


class OnlineRun(C.Structure):                                          # fa_online_run
    _fields_ = [("stream", C.c_int32), ("chunk", C.c_int32), ("local_speaker", C.c_int32)]


class OnlineSegment(C.Structure):                                      # fa_online_segment
    _fields_ = [("stream", C.c_int32), ("chunk", C.c_int32), ("local_speaker", C.c_int32), ("id", C.c_int32), ("start_frame", C.c_int32), ("end_frame", C.c_int32),
                ("start", C.c_float), ("end", C.c_float), ("quality", C.c_float)]


class AedConfig(C.Structure):                                          # fa_aed_config
    _fields_ = [("mode", C.c_int32), ("vocab", C.c_int32), ("eos_id", C.c_int32), ("max_seq", C.c_int32), ("max_new", C.c_int32), ("no_repeat_ngram", C.c_int32),
                ("repetition_penalty", C.c_float), ("window_tokens", C.c_int32), ("min_match", C.c_int32), ("reserved", C.c_int32), ("chunk_samples", C.c_int64),
                ("hop_samples", C.c_int64)]


class SortformerStreamConfig(C.Structure):                             # fa_sortformer_stream_config
    _fields_ = [(n, C.c_int32) for n in ("speakers", "d_model", "chunk_len", "chunk_left_context", "chunk_right_context", "fifo_len", "spkcache_len", "spkcache_update_period",
                                         "sil_frames_per_spk", "max_index", "max_chunk_frames", "subsampling", "n_mels", "reserved")] + \
               [(n, C.c_float) for n in ("silence_threshold", "pred_score_threshold", "scores_boost_latest", "strong_boost_rate", "weak_boost_rate", "min_pos_scores_rate")]


class SortformerStreamGeometry(C.Structure):                           # fa_sortformer_stream_geometry_info
    _fields_ = [(n, C.c_int32) for n in ("chunk_len", "spkcache_len", "spkcache_update_period", "max_pop", "score_rows", "out_rows", "chunk_mel_frames", "spkcache_len_per_spk",
                                         "strong_boost_per_spk", "weak_boost_per_spk", "min_pos_scores_per_spk", "lds_bytes")]


class SortformerStreamInfo(C.Structure):                               # fa_sortformer_stream_info
    _fields_ = [(n, C.c_int32) for n in ("spkcache_length", "fifo_length", "spkcache_preds_present", "fifo_preds_present", "silence_frame_count", "reserved")]


class SortformerChunk(C.Structure):                                    # fa_sortformer_chunk
    _fields_ = [("ready", C.c_int32), ("chunk_length", C.c_int32), ("left_offset", C.c_int32), ("right_offset", C.c_int32), ("start_frame", C.c_int64), ("rows", C.c_int64),
                ("new_start_feat", C.c_int64), ("frames_to_drop", C.c_int64)]


class RnntStreamConfig(C.Structure):                                   # fa_rnnt_stream_config
    _fields_ = [(n, C.c_int32) for n in ("window_samples", "close_silent_windows", "pre_roll_windows", "min_speech_windows", "max_span_samples", "open_slack_frames",
                                         "close_slack_frames", "vad_hangover_chunks", "mel_features", "pre_encode_cache", "total_mel_frames", "reserved")] + \
               [(n, C.c_float) for n in ("rescue_rms_threshold", "vad_rms_threshold")]


class RnntStreamInfo(C.Structure):                                     # fa_rnnt_stream_info
    _fields_ = [(n, C.c_int32) for n in ("frame_cursor", "span_open", "span_start_frame", "span_last_speech_frame", "span_speech_windows", "span_pre_roll_frames",
                                         "silent_window_run", "span_overflowed", "span_samples", "pre_roll_samples", "vad_consecutive_low_chunks", "vad_skip_count",
                                         "absolute_frame_base", "detected_blank_spans", "blank_rescues", "mel_cache_frames")]


class RnntStreamRequest(C.Structure):                                  # fa_rnnt_stream_request
    _fields_ = [(n, C.c_int32) for n in ("stream", "span_start_frame", "span_end_frame", "speech_windows", "audio_samples", "decode_chunks", "status", "reserved")] + \
               [("audio_offset", C.c_int64)]


class RnntStreamGeometry(C.Structure):                                 # fa_rnnt_stream_geometry_info
    _fields_ = [(n, C.c_int32) for n in ("span_capacity", "pre_roll_capacity", "mel_cache_capacity", "reserved")]


class ExportEmbedding(C.Structure):                                    # fa_export_embedding
    _fields_ = [("chunk_index", C.c_int32), ("speaker_index", C.c_int32), ("start_frame", C.c_int32), ("end_frame", C.c_int32),
                ("start_time", C.c_double), ("end_time", C.c_double)]


class ResampleRoute(C.Structure):                                     # fa_resample_route (fa_debug_resample_route: tests)
    _fields_ = [("lo", C.c_int64), ("hi", C.c_int64), ("split", C.c_int64), ("count", C.c_int64), ("kind", C.c_int32), ("wide", C.c_int32),
                ("tile_rows", C.c_int32), ("wide_waves", C.c_int32), ("nv", C.c_int32), ("share", C.c_int32), ("groups", C.c_int32)]


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into csrc/libfluidaudio_hip.so (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", CSRC, "-j8", "all"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libfluidaudio_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the product path)")
    try:
        # torch's wheel bundles its own ROCm runtime: when libfluidaudio_hip.so pulls /opt/rocm's libamdhip64 into the process
        # FIRST, a later `import torch` sees no device (measured on the MI355X box).  Loading torch first makes both use one runtime.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32, f64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t
    L.fa_version.restype = C.c_char_p
    L.fa_debug_inject_fault.argtypes = [i32, i32]
    L.fa_debug_inject_fault.restype = None
    L.fa_debug_set_switch.argtypes = [C.c_char_p, C.c_char_p]
    L.fa_debug_hooks_enabled.restype = i32
    L.fa_debug_ahc_adopted.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.fa_debug_ahc_spec_hits.argtypes = [vp, vp]
    L.fa_ctx_set_timing.argtypes = [vp, i32]
    L.fa_ctx_last_device_ms.argtypes = [vp]
    L.fa_ctx_last_device_ms.restype = f64
    L.fa_debug_sclk_mhz.argtypes = [vp, i32, vp]
    L.fa_ctc_beam_plan.argtypes = [i32, i32, i32, i32, i32, i32, vp]
    L.fa_host_alloc.argtypes = [sz]
    L.fa_host_alloc.restype = vp
    L.fa_host_free.argtypes = [vp]
    L.fa_host_free.restype = None
    L.fa_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.fa_ctx_destroy.argtypes = [vp]
    L.fa_ctx_destroy.restype = None
    L.fa_ctx_synchronize.argtypes = [vp]
    L.fa_ctx_stream.argtypes = [vp]
    L.fa_ctx_stream.restype = vp
    L.fa_ctx_last_error.argtypes = [vp]
    L.fa_ctx_set_workspace_limit.argtypes = [vp, sz]
    L.fa_ctx_set_workspace_cap.argtypes = [vp, sz]
    L.fa_ctx_trim.argtypes = [vp]
    L.fa_ctx_workspace_bytes.argtypes = [vp]
    L.fa_ctx_workspace_bytes.restype = sz
    L.fa_ctx_reserve.argtypes = [vp, sz, sz, i32]
    L.fa_ctx_last_error.restype = C.c_char_p
    L.fa_mel_default_config.argtypes = [C.POINTER(MelConfig)]
    L.fa_mel_default_config.restype = None
    L.fa_mel_num_frames.argtypes = [C.POINTER(MelConfig), i64]
    L.fa_mel_num_frames.restype = i32
    L.fa_mel_padded_frames.argtypes = [C.POINTER(MelConfig), i32]
    L.fa_mel_padded_frames.restype = i32
    L.fa_mel_plan_create.argtypes = [vp, C.POINTER(MelConfig), vp, i32, vp, i32, C.POINTER(vp)]
    L.fa_mel_plan_destroy.argtypes = [vp]
    L.fa_mel_plan_destroy.restype = None
    L.fa_mel_plan_utt_stride.argtypes = [vp]
    L.fa_mel_plan_utt_stride.restype = i64
    L.fa_mel_plan_frame_stride.argtypes = [vp]
    L.fa_mel_plan_frame_stride.restype = i32
    L.fa_mel_plan_total_frames.argtypes = [vp]
    L.fa_mel_plan_total_frames.restype = i64
    L.fa_mel_execute_dev.argtypes = [vp, vp, vp, vp, vp]
    L.fa_mel_batch.argtypes = [vp, C.POINTER(MelConfig), vp, vp, i32, vp, vp, i32, vp, vp]
    L.fa_mel_hann_window.argtypes = [C.POINTER(MelConfig), vp]
    L.fa_mel_normalize_per_feature_dev.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.fa_mel_filterbank.argtypes = [C.POINTER(MelConfig), vp]
    L.fa_ctc_greedy_batch_dev.argtypes = [vp, vp, i32, i32, i32, i32, i64, i64, vp, i32, vp, vp, vp]
    L.fa_ctc_log_softmax_batch_dev.argtypes = [vp, vp, i32, i32, i32, i32, i64, i64, f32, f32, i32, vp]
    L.fa_ctc_greedy_batch.argtypes = [vp, vp, i32, i32, i32, i32, i64, i64, vp, i32, vp, vp, vp]
    L.fa_ctc_greedy_rows_dev.argtypes = [vp, vp, vp, i64, vp, i32, i32, vp, vp, vp]
    L.fa_ctc_greedy_rows.argtypes = [vp, vp, vp, i64, vp, i32, i32, vp, vp, vp]
    L.fa_tdt_default_config.argtypes = [C.POINTER(TdtConfig)]
    L.fa_tdt_default_config.restype = None
    L.fa_tdt_initial_time_index.argtypes = [i32, i32, i32]
    L.fa_tdt_initial_time_index.restype = i32
    L.fa_tdt_navigation_state.argtypes = [i32, i32, i32] + [C.POINTER(i32)] * 4
    L.fa_tdt_navigation_state.restype = None
    L.fa_tdt_final_time_jump.argtypes = [i32, i32, i32, C.POINTER(i32)]
    L.fa_tdt_final_time_jump.restype = i32
    L.fa_tdt_map_duration_bin.argtypes = [C.POINTER(TdtConfig), i32, C.POINTER(i32)]
    L.fa_tdt_clamp_probability.argtypes = [f32]
    L.fa_tdt_clamp_probability.restype = f32
    L.fa_tdt_greedy_tables_dev.argtypes = [vp, C.POINTER(TdtConfig), vp, vp, vp, i32, i32, i32] + [vp] * 6 + [i32] + [vp] * 8
    L.fa_tdt_greedy_logits_dev.argtypes = [vp, C.POINTER(TdtConfig), vp, i32, i32, i32, i32, i32, i64] + [vp] * 6 + [i32] + [vp] * 8
    L.fa_tdt_token_classes.argtypes = [vp, vp, i32, vp, i32, vp]
    L.fa_tdt_topk_rows_dev.argtypes = [vp, vp, i32, i64, i32, i64, i32, vp, vp, vp]
    L.fa_tdt_greedy_logits_lang_dev.argtypes = L.fa_tdt_greedy_logits_dev.argtypes + [vp, i32, i32, i32, vp, vp]
    L.fastcluster_compute_centroid_linkage.argtypes = [vp, sz, sz, vp, sz]
    L.fastcluster_compute_centroid_linkage.restype = C.c_int
    L.fa_ahc_linkage.argtypes = [vp, vp, sz, sz, vp, sz, i32, i32, C.POINTER(AhcStats)]
    L.fa_ahc_linkage_batch.argtypes = [vp, i32, vp, vp, sz, vp, i32, i32, vp, vp]
    L.fa_ahc_row_minima.argtypes = [vp, vp, sz, sz, sz, sz, vp, vp, i32]
    L.fa_ahc_cluster.argtypes = [vp, vp, sz, sz, f64, i32, vp, C.POINTER(AhcStats)]
    L.fa_ahc_cut.argtypes = [vp, sz, f64, vp]
    L.fa_vbx_speaker_count.argtypes = [vp, i64]
    L.fa_vbx_speaker_count.restype = i32
    L.fa_vbx_refine.argtypes = [vp, vp, i64, i32, vp, vp, f64, f64, i32, f64, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.fa_vbx_shard_slices.argtypes = []
    L.fa_vbx_shard_slices.restype = i32
    L.fa_vbx_shard_range.argtypes = [i64, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    L.fa_vbx_shard_range.restype = None
    L.fa_vbx_shard_chunk_doubles.argtypes = [i32, i32, i32]
    L.fa_vbx_shard_chunk_doubles.restype = i64
    L.fa_vbx_shard_create.argtypes = [vp, vp, i64, i32, vp, i32, vp, f64, f64, i32, i32, C.POINTER(vp)]
    L.fa_vbx_shard_destroy.argtypes = [vp]
    L.fa_vbx_shard_destroy.restype = None
    L.fa_vbx_shard_frames.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.fa_vbx_shard_frames.restype = None
    L.fa_vbx_shard_begin.argtypes = [vp, vp]
    L.fa_vbx_shard_iterate.argtypes = [vp, vp, vp]
    L.fa_vbx_shard_finish_iteration.argtypes = [vp, vp, C.POINTER(f64)]
    L.fa_vbx_shard_result.argtypes = [vp, vp, vp, vp]
    L.fa_vbx_weighted_centroids.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, vp, C.POINTER(i32)]
    L.fa_assign_cosine.argtypes = [vp, vp, i64, i32, vp, i32, vp]
    L.fa_centroid_scores.argtypes = [vp, vp, i64, i32, vp, i32, vp]
    L.fa_constrained_assign.argtypes = [vp, vp, i64, i32, vp, vp]
    L.fa_offline_cluster_default_config.argtypes = [C.POINTER(OfflineClusterConfig)]
    L.fa_offline_cluster_default_config.restype = None
    L.fa_offline_cluster.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp, C.POINTER(OfflineClusterConfig), i32, vp, vp, i32,
                                     C.POINTER(i32), C.POINTER(OfflineClusterInfo)]
    L.fa_offline_cluster_ex.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp, C.POINTER(OfflineClusterConfig), i32, vp, vp, i32,
                                        C.POINTER(i32), C.POINTER(OfflineClusterInfo), vp, vp, vp]
    u64 = C.c_uint64
    L.fa_arpa_parse.argtypes = [vp, C.c_char_p, i64, C.POINTER(vp)]
    L.fa_arpa_destroy.argtypes = [vp]
    L.fa_arpa_destroy.restype = None
    L.fa_arpa_unigram_count.argtypes = [vp]
    L.fa_arpa_unigram_count.restype = i64
    L.fa_arpa_bigram_context_count.argtypes = [vp]
    L.fa_arpa_bigram_context_count.restype = i64
    L.fa_arpa_score.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(f32)]
    L.fa_ctc_vocab_create.argtypes = [vp, vp, vp, i32, i32, C.POINTER(vp)]
    L.fa_ctc_vocab_destroy.argtypes = [vp]
    L.fa_ctc_vocab_destroy.restype = None
    L.fa_ctc_beam_search_batch_dev.argtypes = [vp, vp, i32, i32, i32, i64, i64, vp, vp, vp, i32, f32, f32, i32, i32, vp, vp, vp]
    L.fa_ctc_beam_search_batch.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, f32, f32, i32, i32, vp, vp, vp]
    L.fa_wav_pcm16_size.argtypes = [i64]
    L.fa_wav_pcm16_size.restype = i64
    L.fa_wav_encode_pcm16.argtypes = [vp, vp, i64, f64, i32, vp, i64, C.POINTER(i64)]
    L.fa_wav_decode.argtypes = [vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]
    L.fa_rttm_parse.argtypes = [C.c_char_p, i64, i32, vp, i64, C.POINTER(i64), C.c_char_p, i64]
    L.fa_rttm_format.argtypes = [vp, i64, C.c_char_p, C.c_char_p, i64]
    L.fa_rttm_format.restype = i64
    L.fa_export_embeddings_json.argtypes = [vp, i64, vp, i32, vp, i32, vp, i64, C.c_char_p, i64]
    L.fa_export_embeddings_json.restype = i64
    L.fa_seeded_rng_next.argtypes = [C.POINTER(u64)]
    L.fa_seeded_rng_next.restype = u64
    L.fa_seeded_rng_below.argtypes = [C.POINTER(u64), u64]
    L.fa_seeded_rng_below.restype = u64
    L.fa_kmeans_cluster.argtypes = [vp, vp, i64, i32, i32, i32, u64, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.fa_kmeans_cluster_ninit.argtypes = [vp, vp, i64, i32, i32, i32, i32, u64, vp, vp, C.POINTER(i32), C.POINTER(i32), vp]
    L.fa_speaker_constraints_resolve.argtypes = [i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64 * 3)]
    L.fa_speaker_constraints_resolve.restype = None
    L.fa_resample_linear_frames.argtypes = [i64, f64, f64]
    L.fa_resample_linear_frames.restype = i64
    L.fa_resample_linear.argtypes = [vp, vp, i32, i64, f64, f64, vp, i64, C.POINTER(i64)]
    L.fa_resample_poly_frames.argtypes = [i64, i32, i32]
    L.fa_resample_poly_frames.restype = i64
    L.fa_resample_poly_taps.argtypes = [i32, i32, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.fa_resample_poly.argtypes = [vp, vp, i64, i32, i32, vp, i64, C.POINTER(i64)]
    L.fa_resample_poly_dev.argtypes = [vp, vp, i64, i32, i32, vp, i64, C.POINTER(i64)]
    L.fa_debug_resample_route.argtypes = [vp, vp, i64, i32, i32, vp, C.POINTER(ResampleRoute)]
    L.fa_offline_cluster_batch.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, C.POINTER(OfflineClusterConfig), vp, vp, i32, vp, vp, vp]
    L.fa_offline_cluster_batch_dev.argtypes = L.fa_offline_cluster_batch.argtypes
    L.fa_device_count.argtypes = [C.POINTER(i32)]
    L.fa_pool_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.fa_pool_destroy.argtypes = [vp]
    L.fa_pool_destroy.restype = None
    L.fa_pool_size.argtypes = [vp]
    L.fa_pool_size.restype = i32
    L.fa_pool_context.argtypes = [vp, i32]
    L.fa_pool_context.restype = vp
    L.fa_ctx_device.argtypes = [vp]
    L.fa_ctx_device.restype = i32
    L.fa_pool_acquire.argtypes = [vp, C.POINTER(vp)]
    L.fa_pool_release.argtypes = [vp, vp]
    L.fa_pool_release.restype = None
    L.fa_mel_batch_sharded.argtypes = [vp, C.POINTER(MelConfig), vp, vp, i32, vp, vp, i32, vp, vp]
    L.fa_ctc_greedy_batch_sharded.argtypes = [vp, vp, i32, i32, i32, i32, i64, i64, vp, i32, vp, vp, vp]
    L.fa_ahc_linkage_many.argtypes = [vp, i32, vp, vp, sz, vp, i32, vp, vp]
    L.fa_powerset_decode_dev.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    L.fa_powerset_decode.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    L.fa_offline_chunk_assignments.argtypes = [i64, vp, vp, vp, i32, i32, i32, vp]
    L.fa_reconstruct_default_config.argtypes = [C.POINTER(ReconstructConfig)]
    L.fa_reconstruct_default_config.restype = None
    L.fa_offline_reconstruct.argtypes = [vp, C.POINTER(ReconstructConfig), vp, i64, i32, i32, vp, i64, vp, i32, vp, i64, vp, i64,
                                         C.POINTER(i64), C.POINTER(ReconstructInfo)]
    L.fa_offline_reconstruct_dev.argtypes = L.fa_offline_reconstruct.argtypes
    L.fa_segments_finalize.argtypes = [C.POINTER(ReconstructConfig), vp, i64, vp, i64, C.POINTER(i64)]
    L.fa_embedding_default_config.argtypes = [C.POINTER(EmbeddingConfig)]
    L.fa_embedding_default_config.restype = None
    L.fa_embedding_plan.argtypes = [vp, C.POINTER(EmbeddingConfig), vp, i64, i32, i32, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(EmbeddingInfo)]
    L.fa_embedding_plan_dev.argtypes = L.fa_embedding_plan.argtypes
    L.fa_embedding_windows_dev.argtypes = [vp, vp, i64, vp, i64, i32, vp]
    L.fa_embedding_span_inputs.argtypes = [vp, C.POINTER(EmbeddingConfig), vp, i64, vp, i64, vp, vp, vp]
    L.fa_embedding_span_inputs_dev.argtypes = L.fa_embedding_span_inputs.argtypes
    L.fa_weight_resample.argtypes = [vp, vp, i64, i32, i32, vp]
    L.fa_weight_resample_dev.argtypes = L.fa_weight_resample.argtypes
    L.fa_sortformer_offline_default_config.argtypes = [C.POINTER(SortformerOfflineConfig)]
    L.fa_sortformer_offline_default_config.restype = None
    L.fa_sortformer_offline_windows.argtypes = [C.POINTER(SortformerOfflineConfig), vp, i32, vp, i64, C.POINTER(i64), vp, vp]
    L.fa_sortformer_pack_windows_dev.argtypes = [vp, C.POINTER(SortformerOfflineConfig), vp, i32, i64, i64, vp, i32, i64, vp, vp]
    L.fa_sortformer_stitch_dev.argtypes = [vp, C.POINTER(SortformerOfflineConfig), vp, vp, i32, i64, vp, vp]
    L.fa_sortformer_stitcher_alignment.argtypes = [vp, vp, i64, i32, vp]
    L.fa_timeline_default_config.argtypes = [C.POINTER(TimelineConfig)]
    L.fa_timeline_default_config.restype = None
    L.fa_timeline_segments_dev.argtypes = [vp, C.POINTER(TimelineConfig), vp, vp, vp, vp, i32, i32, vp, i64, C.POINTER(i64), vp]
    L.fa_timeline_segments.argtypes = L.fa_timeline_segments_dev.argtypes
    L.fa_der_default_config.argtypes = [C.POINTER(DerConfig)]
    L.fa_der_default_config.restype = None
    L.fa_der_score_batch.argtypes = [vp, C.POINTER(DerConfig), vp, vp, vp, vp, i32, vp, vp, vp, vp, i64]
    L.fa_edit_distance_batch.argtypes = [vp, vp, vp, vp, vp, i64, vp]
    L.fa_edit_distance_batch_dev.argtypes = L.fa_edit_distance_batch.argtypes
    L.fa_kws_adjusted_threshold.argtypes = [i32, f32, i32]
    L.fa_kws_adjusted_threshold.restype = f32
    L.fa_ctc_kws_spot_batch_dev.argtypes = [vp, vp, i32, i32, i32, i64, i64, vp, vp, vp, i32, vp, i32, i32, vp, i64, C.POINTER(i64), vp]
    L.fa_ctc_kws_spot_batch.argtypes = L.fa_ctc_kws_spot_batch_dev.argtypes
    L.fa_ctc_kws_score_windows_dev.argtypes = [vp, vp, i32, i32, i32, i64, i64, vp, vp, vp, i32, vp, i64, i32, vp]
    L.fa_ctc_kws_score_windows.argtypes = L.fa_ctc_kws_score_windows_dev.argtypes
    L.fa_paraformer_cif_default_config.argtypes = [C.POINTER(ParaformerCifConfig)]
    L.fa_paraformer_cif_default_config.restype = None
    L.fa_paraformer_cif_dev.argtypes = [vp, C.POINTER(ParaformerCifConfig), vp, i32, i32, i32, i32, i64, i64, vp, i64, vp, vp, vp, vp, vp, vp]
    L.fa_paraformer_cif.argtypes = L.fa_paraformer_cif_dev.argtypes
    L.fa_paraformer_timestamps_dev.argtypes = [vp, C.POINTER(ParaformerCifConfig), vp, i64, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i64, C.POINTER(i64), vp]
    L.fa_paraformer_timestamps.argtypes = L.fa_paraformer_timestamps_dev.argtypes
    L.fa_tdt_merge_default_config.argtypes = [C.POINTER(TdtMergeConfig)]
    L.fa_tdt_merge_default_config.restype = None
    L.fa_tdt_merge_windows_dev.argtypes = [vp, C.POINTER(TdtMergeConfig), vp, vp, vp, vp, vp, i32, vp, i64, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fa_tdt_merge_windows.argtypes = L.fa_tdt_merge_windows_dev.argtypes
    L.fa_vad_default_config.argtypes = [C.POINTER(VadSegmentationConfig)]
    L.fa_vad_default_config.restype = None
    L.fa_vad_chunk_count.argtypes = [i64]
    L.fa_vad_chunk_count.restype = i64
    L.fa_vad_segments_dev.argtypes = [vp, C.POINTER(VadSegmentationConfig), vp, vp, vp, i32, vp, i64, C.POINTER(i64), vp]
    L.fa_vad_segments.argtypes = L.fa_vad_segments_dev.argtypes
    L.fa_vad_pack_chunks_dev.argtypes = [vp, vp, vp, i32, vp, i64, vp]
    L.fa_vad_pack_chunks.argtypes = L.fa_vad_pack_chunks_dev.argtypes
    L.fa_vad_gather_segments_dev.argtypes = [vp, vp, vp, i32, vp, i64, vp, i64, vp]
    L.fa_vad_gather_segments.argtypes = L.fa_vad_gather_segments_dev.argtypes
    L.fa_vad_stream_advance_dev.argtypes = [vp, C.POINTER(VadSegmentationConfig), vp, vp, vp, i32, i32, vp, i32, i32, vp, i64, C.POINTER(i64)]
    L.fa_vad_stream_advance.argtypes = L.fa_vad_stream_advance_dev.argtypes
    fc = C.POINTER(FsmnVadConfig)
    L.fa_fsmn_vad_default_config.argtypes = [fc]
    L.fa_fsmn_vad_default_config.restype = None
    L.fa_fsmn_vad_frame_count.argtypes = [i64]
    L.fa_fsmn_vad_frame_count.restype = i64
    L.fa_fsmn_vad_plan_chunks.argtypes = [vp, i32, vp, i64, C.POINTER(i64), vp, vp]
    L.fa_fsmn_vad_pack_waveforms_dev.argtypes = [vp, vp, vp, i32, vp, i64, vp, i64, i64]
    L.fa_fsmn_vad_pack_waveforms.argtypes = L.fa_fsmn_vad_pack_waveforms_dev.argtypes
    L.fa_fsmn_vad_pack_feats_dev.argtypes = [vp, vp, i32, i64, vp, i64, i32, vp]
    L.fa_fsmn_vad_gather_silence_dev.argtypes = [vp, vp, i32, i32, i32, vp, i64, vp, i32, vp, i64]
    L.fa_fsmn_vad_segments_dev.argtypes = [vp, fc, vp, vp, i32, vp, i64, C.POINTER(i64), vp]
    L.fa_fsmn_vad_segments.argtypes = L.fa_fsmn_vad_segments_dev.argtypes
    L.fa_tdt_window_default_config.argtypes = [C.POINTER(TdtWindowConfig)]
    L.fa_tdt_window_default_config.restype = None
    L.fa_tdt_window_layout.argtypes = [C.POINTER(TdtWindowConfig)] + [C.POINTER(i64)] * 4
    L.fa_tdt_window_count_bound.argtypes = [C.POINTER(TdtWindowConfig), i64]
    L.fa_tdt_window_count_bound.restype = i64
    L.fa_tdt_plan_windows_dev.argtypes = [vp, C.POINTER(TdtWindowConfig), vp, vp, i32, vp, i64, vp] + [vp] * 5 + [vp, vp]
    L.fa_tdt_plan_windows.argtypes = L.fa_tdt_plan_windows_dev.argtypes
    L.fa_tdt_pack_windows_dev.argtypes = [vp, C.POINTER(TdtWindowConfig), vp, vp, i32, vp, i64, vp, i64, vp]
    L.fa_tdt_pack_windows.argtypes = L.fa_tdt_pack_windows_dev.argtypes
    L.fa_tdt_speech_gate_dev.argtypes = [vp, C.POINTER(TdtWindowConfig), vp, vp, i32, vp, vp, vp, i64, vp, vp, vp]
    L.fa_tdt_speech_gate.argtypes = L.fa_tdt_speech_gate_dev.argtypes
    L.fa_vocab_rescore_default_config.argtypes = [vp]
    L.fa_vocab_rescore_default_config.restype = None
    L.fa_vocab_rescore_boost.argtypes = [f32, i32, vp]
    L.fa_vocab_rescore_boost.restype = f32
    L.fa_vocab_rescore_build.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, i64, C.POINTER(i64), vp, i64]
    L.fa_vocab_rescore_candidates.argtypes = [vp, vp, i64, vp, i32, vp, vp, vp, f32, vp, i64, C.POINTER(i64), vp]
    L.fa_vocab_rescore_decide_dev.argtypes = [vp, vp, i32, i32, i32, i64, i64, vp, vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fa_vocab_rescore_decide.argtypes = L.fa_vocab_rescore_decide_dev.argtypes
    L.fa_rnnt_bias_effective_boost.argtypes = [i32, f32, f32]
    L.fa_rnnt_bias_effective_boost.restype = f32
    L.fa_rnnt_bias_build.argtypes = [vp, i32, vp, vp, i32, vp, i64, C.POINTER(i64), C.POINTER(i32)]
    L.fa_rnnt_bias_candidates.argtypes = [vp, i64, vp, i32, vp, vp, i32, C.POINTER(i32)]
    L.fa_rnnt_default_config.argtypes = [C.POINTER(RnntConfig)]
    L.fa_rnnt_default_config.restype = None
    L.fa_rnnt_greedy_logits_dev.argtypes = [vp, C.POINTER(RnntConfig), vp, i32, i32, i32, i32, i32, i64, vp, vp, vp, i64, i32, vp, vp, i32] + [vp] * 7
    L.fa_speaker_l2_normalize.argtypes = [vp, vp]
    L.fa_speaker_cosine_distance.argtypes = [vp, vp]
    L.fa_speaker_cosine_distance.restype = f32
    L.fa_speaker_validate_embedding.argtypes = [vp, f32]
    L.fa_speaker_db_default_config.argtypes = [C.POINTER(SpeakerDbConfig)]
    L.fa_speaker_db_default_config.restype = None
    L.fa_speaker_db_create.argtypes = [vp, C.POINTER(SpeakerDbConfig), i32, C.POINTER(vp)]
    L.fa_speaker_db_destroy.argtypes = [vp]
    L.fa_speaker_db_destroy.restype = None
    L.fa_speaker_db_assign_dev.argtypes = [vp, vp, vp, vp, vp, i32, i64, vp]
    L.fa_speaker_db_distances_dev.argtypes = [vp, vp, vp, i32, vp, vp]
    L.fa_speaker_db_mergeable_pairs_dev.argtypes = [vp, vp, f32, i32, vp, i32, vp]
    L.fa_speaker_db_assign.argtypes = L.fa_speaker_db_assign_dev.argtypes
    L.fa_speaker_db_distances.argtypes = L.fa_speaker_db_distances_dev.argtypes
    L.fa_speaker_db_mergeable_pairs.argtypes = L.fa_speaker_db_mergeable_pairs_dev.argtypes
    L.fa_speaker_db_upsert.argtypes = [vp, vp, i32, C.POINTER(SpeakerInfo), vp, vp]
    L.fa_speaker_db_get.argtypes = [vp, vp, i32, i32, C.POINTER(SpeakerInfo), vp, vp, i32]
    L.fa_speaker_db_ids.argtypes = [vp, vp, i32, vp, C.POINTER(i32)]
    L.fa_speaker_db_count.argtypes = [vp, vp, vp]
    L.fa_speaker_db_remove.argtypes = [vp, vp, i32, i32, i32]
    L.fa_speaker_db_remove_inactive.argtypes = [vp, vp, i32, i64, i32]
    L.fa_speaker_db_set_permanent.argtypes = [vp, vp, i32, i32, i32]
    L.fa_speaker_db_reset.argtypes = [vp, vp, i32, i32]
    L.fa_online_chunk_default_config.argtypes = [C.POINTER(OnlineChunkConfig)]
    L.fa_online_chunk_default_config.restype = None
    L.fa_online_chunk_plan_dev.argtypes = [vp, C.POINTER(OnlineChunkConfig), vp, vp, i32, i32, vp, vp, i32, vp, vp]
    L.fa_online_chunk_plan.argtypes = [vp, C.POINTER(OnlineChunkConfig), vp, vp, i32, i32, vp, vp, i32, C.POINTER(i32), vp]
    L.fa_online_pack_waveforms_dev.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    L.fa_online_chunk_finish_dev.argtypes = [vp, C.POINTER(OnlineChunkConfig), vp, vp, vp, vp, vp, i32, i64, vp, i64, C.POINTER(i64), vp, vp]
    ac = C.POINTER(AedConfig)
    L.fa_aed_default_config.argtypes = [ac, i32]
    L.fa_aed_default_config.restype = None
    L.fa_aed_max_out.argtypes = [ac]
    L.fa_aed_max_out.restype = i32
    L.fa_aed_state_bytes.argtypes = [ac, i32]
    L.fa_aed_state_bytes.restype = i64
    L.fa_aed_begin_dev.argtypes = [vp, ac, i32, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp]
    L.fa_aed_step_dev.argtypes = [vp, ac, i32, vp, vp, i32, i64, vp, vp, vp, i32, vp, vp]
    L.fa_aed_finish_dev.argtypes = [vp, ac, i32, vp, i32, vp, vp, vp, vp]
    L.fa_aed_finish.argtypes = L.fa_aed_finish_dev.argtypes
    L.fa_aed_cross_mask_dev.argtypes = [vp, vp, i32, i32, i32, vp]
    L.fa_aed_encoder_valid_frames.argtypes = [i64, i32, i32, i32]
    L.fa_aed_encoder_valid_frames.restype = i32
    L.fa_aed_encoder_context_dev.argtypes = [vp, vp, i32, i32, i32, i32, i64, i64, i64, vp, vp, vp]
    L.fa_aed_gather_hidden_dev.argtypes = [vp, ac, i32, vp, vp, i32, i32, i32, i64, i64, i64, vp]
    L.fa_aed_plan_windows.argtypes = [ac, vp, i64, vp, vp, vp, i64, C.POINTER(i64)]
    L.fa_aed_merge_windows_dev.argtypes = [vp, ac, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.fa_aed_merge_windows.argtypes = L.fa_aed_merge_windows_dev.argtypes
    sc = C.POINTER(SortformerStreamConfig)
    L.fa_sortformer_stream_default_config.argtypes = [sc]
    L.fa_sortformer_stream_default_config.restype = None
    L.fa_sortformer_stream_preset_config.argtypes = [i32, sc]
    L.fa_sortformer_stream_geometry.argtypes = [sc, C.POINTER(SortformerStreamGeometry)]
    L.fa_sortformer_stream_pop_out_length.argtypes = [sc, i32]
    L.fa_sortformer_stream_pop_out_length.restype = i32
    L.fa_sortformer_stream_create.argtypes = [vp, sc, i32, C.POINTER(vp)]
    L.fa_sortformer_stream_destroy.argtypes = [vp]
    L.fa_sortformer_stream_destroy.restype = None
    L.fa_sortformer_stream_inputs.argtypes = [vp, vp] + [C.POINTER(vp)] * 4
    L.fa_sortformer_stream_get.argtypes = [vp, vp, i32, C.POINTER(SortformerStreamInfo), vp, vp, vp, vp, vp]
    L.fa_sortformer_stream_set.argtypes = L.fa_sortformer_stream_get.argtypes
    L.fa_sortformer_stream_reset.argtypes = [vp, vp, i32]
    L.fa_sortformer_stream_update_dev.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fa_sortformer_stream_update.argtypes = L.fa_sortformer_stream_update_dev.argtypes
    L.fa_sortformer_stream_chunk_plan.argtypes = [sc, vp, vp, i32, vp]
    L.fa_sortformer_stream_file_chunks.argtypes = [sc, i64, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.fa_sortformer_stream_pack_chunks_dev.argtypes = [vp, sc, vp, vp, vp, i32, vp]
    rc = C.POINTER(RnntStreamConfig)
    L.fa_rnnt_stream_default_config.argtypes = [rc]
    L.fa_rnnt_stream_default_config.restype = None
    L.fa_rnnt_stream_geometry.argtypes = [rc, C.POINTER(RnntStreamGeometry)]
    L.fa_rnnt_stream_rms.argtypes = [vp, i64, i32, C.POINTER(f32)]
    L.fa_rnnt_stream_create.argtypes = [vp, rc, i32, C.POINTER(vp)]
    L.fa_rnnt_stream_destroy.argtypes = [vp]
    L.fa_rnnt_stream_destroy.restype = None
    L.fa_rnnt_stream_reset.argtypes = [vp, vp, i32]
    L.fa_rnnt_stream_get.argtypes = [vp, vp, i32, C.POINTER(RnntStreamInfo), vp, vp, vp]
    L.fa_rnnt_stream_set.argtypes = L.fa_rnnt_stream_get.argtypes
    L.fa_rnnt_stream_gate_dev.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.fa_rnnt_stream_gate.argtypes = L.fa_rnnt_stream_gate_dev.argtypes
    L.fa_rnnt_stream_mel_inputs_dev.argtypes = [vp, vp, vp, i32, i64, i64, i64, vp, vp, i32, vp, vp]
    L.fa_rnnt_stream_advance_dev.argtypes = [vp, vp, vp, vp, i32, vp, i32]
    L.fa_rnnt_stream_track_dev.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, i32, i32, vp, i32, vp, i64, vp, vp]
    L.fa_rnnt_stream_track.argtypes = L.fa_rnnt_stream_track_dev.argtypes
    L.fa_rnnt_stream_finalize_dev.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, i32, i32, vp, i32, vp, i64, vp, vp]
    L.fa_rnnt_stream_merge_rescued_dev.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp]
    L.fa_rnnt_stream_merge_rescued.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp]
    _lib = L
    return L


class Context:
    """fa_ctx: one device + one stream + cached workspaces (one per host thread)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        st = lib().fa_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h))
        if st != SUCCESS:
            raise FluidAudioHipError(st, "fa_ctx_create", "no usable MI355X visible" if st == RUNTIME_ERROR else "")
        self.device = device

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return lib().fa_ctx_stream(self._h) or 0

    def synchronize(self):
        self.check(lib().fa_ctx_synchronize(self._h), "fa_ctx_synchronize")

    @contextlib.contextmanager
    def torch_ordered(self, enabled: bool = True):
        """Stream ordering for the `*_dev` entries called with torch tensors: the context's stream first waits for
        everything already enqueued on torch's current stream (producers of the inputs, `.contiguous()` copies), and
        torch's current stream afterwards waits for what the body enqueued on the context's stream — so later torch ops
        (and the caching allocator's reuse of freed blocks) are ordered behind the kernels.  Two event record/wait pairs,
        no host synchronisation.  `enabled=False`: the caller orders the streams itself (bench.py's timed loop)."""
        if not enabled:
            yield
            return
        import torch
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream()
            own = torch.cuda.ExternalStream(self.stream, device=self.device)
        if cur.cuda_stream == own.cuda_stream:
            yield
            return
        own.wait_stream(cur)
        try:
            yield
        finally:
            cur.wait_stream(own)

    def last_error(self) -> str:
        return (lib().fa_ctx_last_error(self._h) or b"").decode()

    # workspace policy (include/fluidaudio_hip.h): what the context may keep cached between calls / may take at all
    def set_workspace_limit(self, nbytes: int):
        self.check(lib().fa_ctx_set_workspace_limit(self._h, nbytes), "fa_ctx_set_workspace_limit")

    def set_workspace_cap(self, nbytes: int | None):
        self.check(lib().fa_ctx_set_workspace_cap(self._h, (1 << 64) - 1 if nbytes is None else nbytes), "fa_ctx_set_workspace_cap")

    def trim(self):
        self.check(lib().fa_ctx_trim(self._h), "fa_ctx_trim")

    def workspace_bytes(self) -> int:
        return int(lib().fa_ctx_workspace_bytes(self._h))

    def reserve(self, n_max: int, d: int, recordings: int = 1):
        """Take the linkage workspace of `recordings` problems of up to n_max x d now (server start-up), not inside the first request."""
        self.check(lib().fa_ctx_reserve(self._h, int(n_max), int(d), int(recordings)), "fa_ctx_reserve")

    def check(self, status: int, where: str):
        if status != SUCCESS:
            raise FluidAudioHipError(status, where, self.last_error())

    def ahc_adopted(self):
        """What the filter-based rounds adopted at the last hand-over of AUTO's tie route on this context (fa_debug_ahc_adopted; recorded while
        FA_AHC_RO_HANDOVER_AT is set): dict of row, kind, eps and per-slot arrays node, d1, nn, nnnode, e2 — or None when nothing was recorded."""
        import numpy as np
        row, kind, eps, slots = C.c_int64(), C.c_int32(), C.c_double(), C.c_size_t()
        f = lib().fa_debug_ahc_adopted
        self.check(f(self._h, C.byref(row), C.byref(kind), C.byref(eps), C.byref(slots), 0, None, None, None, None, None), "fa_debug_ahc_adopted")
        if row.value < 0:
            return None
        n = slots.value
        a = {"node": np.zeros(n, np.int32), "d1": np.zeros(n), "nn": np.zeros(n, np.int32), "nnnode": np.zeros(n, np.int32), "e2": np.zeros(n)}
        self.check(f(self._h, C.byref(row), C.byref(kind), C.byref(eps), C.byref(slots), n, *(a[k].ctypes.data for k in ("node", "d1", "nn", "nnnode", "e2"))),
                   "fa_debug_ahc_adopted")
        return dict(row=row.value, kind=kind.value, eps=eps.value, **a)

    def ahc_spec_hits(self) -> int:
        """Speculated merges the filter-based rounds committed in their last run on this context (fa_debug_ahc_spec_hits): 0 for the one-merge round
        (FA_AHC_SPEC=0), -1 when nothing was recorded."""
        v = C.c_int64()
        self.check(lib().fa_debug_ahc_spec_hits(self._h, C.byref(v)), "fa_debug_ahc_spec_hits")
        return v.value

    def sclk_mhz(self, spin_us: int = 200) -> float:
        """The shader clock right now (fa_debug_sclk_mhz): latency-bound legs print it next to their timing."""
        v = C.c_double()
        self.check(lib().fa_debug_sclk_mhz(self._h, spin_us, C.byref(v)), "fa_debug_sclk_mhz")
        return v.value

    def close(self):
        if self._h:
            lib().fa_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pinned_array(shape, dtype):
    """numpy array over page-locked host memory from fa_host_alloc (freed when the array and its views are gone)."""
    import numpy as np
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    p = lib().fa_host_alloc(max(n * dt.itemsize, 1))
    if not p:
        raise MemoryError("fa_host_alloc failed")

    class _Owner:
        def __init__(self, ptr):
            self.ptr = ptr

        def __del__(self):
            lib().fa_host_free(self.ptr)

    buf = (C.c_char * max(n * dt.itemsize, 1)).from_address(p)
    buf._owner = _Owner(p)
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)


_default_ctx: dict[int, Context] = {}


def default_context(device: int | None = None) -> Context:
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("FLUIDAUDIO_HIP_USE_LOCAL_RANK") else 0
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
