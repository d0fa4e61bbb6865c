/*
 * fluidaudio_hip.h — C ABI of libfluidaudio_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the host arithmetic of FluidInference/FluidAudio
 * (paths below are relative to the reference's Sources/ directory).
 * Plain pointers and sizes only; no exception crosses this boundary; every entry
 * returns an fa_status whose numbering equals fastcluster_wrapper_status
 * (FastClusterWrapper/include/FastClusterWrapper.h:11-19).
 *
 * Naming: entries ending in _dev take DEVICE pointers and enqueue work on the
 * context's stream without synchronising; the un-suffixed entries take HOST
 * pointers, copy in/out and return when the result is in the caller's buffer
 * (the calling convention of the Swift seams they replace).
 */
#ifndef FLUIDAUDIO_HIP_H
#define FLUIDAUDIO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FA_SUCCESS = 0,
    FA_INVALID_ARGUMENT = 1,
    FA_INDEX_OVERFLOW = 2,
    FA_OUTPUT_TOO_SMALL = 3,
    FA_ALLOCATION_FAILURE = 4,
    FA_RUNTIME_ERROR = 5, /* HIP errors, NaN distances, unsupported-on-device conditions */
    FA_UNKNOWN_ERROR = 255
} fa_status;

/* ------------------------------------------------------------------ context -------- */
/* One context = one device + one stream + cached workspaces.  A context is NOT
 * thread-safe; use one per host thread (the reference's AudioMelSpectrogram is likewise
 * one-instance-per-thread, FluidAudio/Shared/AudioMelSpectrogram.swift:48-57). */
typedef struct fa_ctx fa_ctx;

/* stream: a hipStream_t to enqueue on, or NULL to let the context create its own. */
fa_status fa_ctx_create(int device, void *stream, fa_ctx **out);
void fa_ctx_destroy(fa_ctx *ctx);
fa_status fa_ctx_synchronize(fa_ctx *ctx);
/* The hipStream_t every _dev entry of this context enqueues on (for events / stream-ordered callers). */
void *fa_ctx_stream(const fa_ctx *ctx);
/* Page-locked host memory (hipHostMalloc).  Optional: every host-pointer entry accepts ordinary memory; buffers from
 * fa_host_alloc are moved by DMA at the full PCIe rate and let fa_mel_batch overlap its uploads with its downloads. */
void *fa_host_alloc(size_t bytes);
void fa_host_free(void *p);
/* Workspace policy.  A context keeps its linkage workspace (N^2 * 8 B: 15 GB at 43 200 rows, 20 GB at 50 000) and its scratch buffer
 * between calls, because the first call at a new size pays 0.4 - 2.5 s of hipMalloc.
 *   fa_ctx_set_workspace_limit : a cached linkage workspace larger than `bytes` is released when the call that used it returns
 *                                (0 = never keep one).  Default: keep (or the value of FLUIDAUDIO_HIP_WORKSPACE_LIMIT).
 *   fa_ctx_set_workspace_cap   : a linkage call never takes more than `bytes` of workspace.  A problem whose N x N matrix exceeds the cap
 *                                (or HBM, or 196 608 points) runs in the matrix-free mode — O(N d) memory like the reference, the same
 *                                dendrogram, ~5x slower per merge; when even that exceeds the cap the call fails with FA_ALLOCATION_FAILURE
 *                                (the reference's status for std::bad_alloc, FastClusterWrapper.cpp:236-238; AHCClustering degrades to
 *                                singletons).  Default: no cap — hipMalloc decides.
 *   fa_ctx_trim                : releases everything cached now.
 *   fa_ctx_workspace_bytes     : bytes cached right now.
 *   fa_ctx_reserve             : takes the workspace of `recordings` linkage problems of up to n_max points x d dimensions NOW (one
 *                                recording: fa_ahc_linkage / fa_offline_cluster; several: the batched entries, whose problems share one
 *                                allocation), so that a server pays the hipMalloc (0.3 - 6 s for 15 GB, depending on the box) at start-up
 *                                and not inside its first request.  Subject to the cap; kept between calls like any workspace within the limit.
 * Independently of these, a context whose workspace allocation fails first releases the idle caches of the OTHER contexts on the
 * same device and retries, so a pool of contexts on one GPU re-allocates under pressure instead of failing. */
fa_status fa_ctx_set_workspace_limit(fa_ctx *ctx, size_t bytes);
fa_status fa_ctx_set_workspace_cap(fa_ctx *ctx, size_t bytes);
fa_status fa_ctx_trim(fa_ctx *ctx);
size_t fa_ctx_workspace_bytes(const fa_ctx *ctx);
fa_status fa_ctx_reserve(fa_ctx *ctx, size_t n_max, size_t d, int32_t recordings);
/* Last error text recorded on this context ("" if none). */
const char *fa_ctx_last_error(const fa_ctx *ctx);
/* Library build identification, e.g. "fluidaudio_hip 0.1 gfx950". */
const char *fa_version(void);

/* Environment.  The library reads the process environment ONCE (at the first context or switch lookup) and never again:
 *   FLUIDAUDIO_HIP_DEVICES / FLUIDAUDIO_HIP_DEVICE   device set behind the context-free drop-in symbol (fa_pool, below)
 *   FLUIDAUDIO_HIP_WORKSPACE_LIMIT                   default of fa_ctx_set_workspace_limit, bytes
 *   FLUIDAUDIO_HIP_DEBUG_HOOKS=1                     lets fa_debug_inject_fault / fa_debug_set_switch act (tests); without it both are inert
 * ROUTE switches — each forces one of the routes the dispatch chooses between by problem shape, so that every route can be tested on any
 * input; results are identical on every route (that is what the tests check), only the speed differs:
 *   FA_AHC_CPT=1|2|4, FA_AHC_UNI_CPT=1|2|4   slots per thread of the round kernel (single problem / uniform batch)
 *   FA_AHC_NO_SINGLE_BLOCK                   problems of <= 512 points through the multi-block chain
 *   FA_AHC_NO_UNIFORM, FA_AHC_IN_FLIGHT, FA_AHC_UNI_GROUPS=1..4, FA_AHC_UNI_WAVES=6|8   how a batch of problems is laid over launches / streams
 *   FA_AHC_RO_NO_MATRIX                      the reference-order run without the N x N filter matrix (O(N d) memory, like the reference)
 *   FA_AHC_RO_NO_HANDOVER                    AUTO's tie route stays in reference order to the last row (no hand-over to the rounds once the ties have stopped)
 *   FA_AHC_RO_HANDOVER_AT=row                AUTO's tie route hands over at the first replay boundary with >= row rows done, whatever the ties did before
 *                                            (the other conditions stay: no tie above height 0 seen, no exact re-scan pending); fa_debug_ahc_adopted
 *                                            records what the rounds adopt there
 *   FA_AHC_RO_REPLAY_PAIRS=k                 (scan, select) launch pairs per graph replay of the reference-order run (default min(256, N rounded up
 *                                            to 4)); a positive multiple of 4, anything else fails a call that runs in reference order with
 *                                            INVALID_ARGUMENT.  4: a hand-over lands within 4 rows of any chosen row
 *   FA_AHC_DEBUG                             one line of statistics per linkage call on stderr
 *   FA_AHC_SPEC=0                            the one-merge round instead of the speculative one (two merges per launch where the next was foreseen)
 *   FA_AHC_SYNC_DRIVE                        the round replays of one problem one at a time, each of the full length and each state read before the next is
 *                                            enqueued (no replay queued ahead, no shorter replays towards the end)
 *   FA_MEL_GENERIC, FA_MEL_SLICE_MB=n        the generic mel kernel; slice size of host-pointer batches
 *   FA_VBX_NO_TILED                          the untiled VBx iteration
 *   FA_RESAMPLE_SIMPLE, _NO_DECIM, _NO_DECIM_TILES, _NO_ROWS, _NO_WIDE, FA_RESAMPLE_WIDE=rows:waves (16:8, 16:10, 32:8, 32:10)   polyphase kernel family
 *   FA_KWS_ARENA=records                     the candidate arena of a word-spotting call (never less than one job can need): a small one forces the
 *                                            passes that walk overflowed jobs again
 *   FA_TDT_MERGE_LDS_SIDE=tokens             the longest overlap side a seam of fa_tdt_merge_windows keeps in LDS (at most 128, the default): a
 *                                            small one sends short sides through the workspace route
 *   FA_VR_ARENA=records                      the survivor arena of fa_vocab_rescore_candidates: a small one forces the second walk
 * fa_debug_set_switch(name, value): value NULL = unset.  Changes what the NEXT calls see (process-wide; not for use while calls are in flight
 * on other threads).  RUNTIME_ERROR without FLUIDAUDIO_HIP_DEBUG_HOOKS=1, INVALID_ARGUMENT for an unknown name. */
fa_status fa_debug_set_switch(const char *name, const char *value);
int32_t fa_debug_hooks_enabled(void);
/* Test hook: the state the filter-based rounds adopted at the last hand-over of AUTO's tie route on this context, recorded only while
 * FA_AHC_RO_HANDOVER_AT is set (one synchronisation and a copy of O(slots) values per hand-over; nothing without the switch).
 * *row: dendrogram rows done at the hand-over (-1: none recorded, or the last tie route run under the switch did not hand over),
 * *kind: what was pending at that replay boundary (0: a merge decided, its row not yet written; 1: a re-scan), *eps: the bound of
 * |matrix entry - exact squared distance| the rounds certify with, *slots: matrix slots.  The arrays (nullable) take the first min(capacity, slots) slots: node id (INT32_MAX: empty slot),
 * the row record (d1: smallest entry over the other live slots, nn: its slot, lowest on ties, nnnode: that slot's node id) and e2 (smallest
 * entry other than column nn).  RUNTIME_ERROR without FLUIDAUDIO_HIP_DEBUG_HOOKS=1. */
fa_status fa_debug_ahc_adopted(const fa_ctx *ctx, int64_t *row, int32_t *kind, double *eps, size_t *slots, size_t capacity, int32_t *node, double *d1,
                               int32_t *nn, int32_t *nnnode, double *e2);
/* Test hook: how many speculated merges the filter-based rounds committed in their last run on this context (the speculative round, FA_AHC_SPEC: a
 * launch that merges a pair also evaluates the merge most likely to follow; the next launch commits it when its records certify exactly that merge).
 * 0 when the run used the one-merge round, -1 when nothing was recorded.  RUNTIME_ERROR without FLUIDAUDIO_HIP_DEBUG_HOOKS=1. */
fa_status fa_debug_ahc_spec_hits(const fa_ctx *ctx, int64_t *hits);
/* Test hook: the next `count` passes through `site` fail the way the real failure would (count 0 disarms).  Process-wide; one relaxed
 * atomic load on the paths that carry a site.  Inert unless the process was started with FLUIDAUDIO_HIP_DEBUG_HOOKS=1.  Used by the
 * fault-injection tests of the degrade contracts:
 *   FA_FAULT_VBX            fa::vbx_run_dev returns RUNTIME_ERROR  -> VBxClustering.refine's catch block (VBxClustering.swift:136-141)
 *   FA_FAULT_THREAD_START   no host thread to be had (std::system_error) -> the share runs on the calling thread
 *   FA_FAULT_DEVBUF_MALLOC  the first hipMalloc of a cached-buffer request fails -> idle caches of the device released, retried; the retry
 *                           is a pass too, so count 2 fails one request for good -> the entry returns ALLOCATION_FAILURE
 *   FA_FAULT_WS_MALLOC      the first hipMalloc of a linkage workspace fails     -> the same
 *   FA_FAULT_AHC            the linkage of fa_offline_cluster fails -> singletons (AHCClustering.swift:52-55) */
enum { FA_FAULT_VBX = 0, FA_FAULT_THREAD_START = 1, FA_FAULT_DEVBUF_MALLOC = 2, FA_FAULT_WS_MALLOC = 3, FA_FAULT_AHC = 4, FA_FAULT_SITES = 5 };
void fa_debug_inject_fault(int32_t site, int32_t count);
/* Measurement support.  fa_ctx_set_timing(1): entries that support it (fa_ctc_beam_search_batch_dev, fa_edit_distance_batch(_dev), fa_paraformer_cif(_dev), fa_paraformer_timestamps(_dev), fa_tdt_merge_windows(_dev)) bracket the DEVICE work of a call —
 * behind its allocations — with two events on the context's stream; fa_ctx_last_device_ms returns that time (< 0: none recorded), so a
 * caller can tell kernel time from host-side allocation time.  fa_debug_sclk_mhz: the shader clock right now (one wavefront counts
 * s_memtime cycles over spin_us microseconds of the constant 100 MHz s_memrealtime counter). */
fa_status fa_ctx_set_timing(fa_ctx *ctx, int32_t enable);
double fa_ctx_last_device_ms(const fa_ctx *ctx);
fa_status fa_debug_sclk_mhz(fa_ctx *ctx, int32_t spin_us, double *mhz);

/* ------------------------------------------------------------------ mel ------------- */
/* Replaces AudioMelSpectrogram (FluidAudio/Shared/AudioMelSpectrogram.swift):
 *   ctor parameters :59-70, computeFlat :185-292, computeFlatTransposed :325-456,
 *   compute (legacy) :132-178. */
enum { FA_MEL_FLOOR_ADDITIVE = 0, FA_MEL_FLOOR_CLAMPED = 1 };              /* LogFloorMode :24-27 */
enum { FA_MEL_PAD_CENTER = 0, FA_MEL_PAD_PREPADDED = 1, FA_MEL_PAD_LEGACY = 2 }; /* PaddingMode :19-22; LEGACY = compute() */
enum { FA_MEL_LAYOUT_MEL_MAJOR = 0,   /* [n_mels, frames]  computeFlat  (mel[m*stride + t]) */
       FA_MEL_LAYOUT_FRAME_MAJOR = 1  /* [frames, n_mels]  computeFlatTransposed (mel[t*n_mels + m]) */ };

typedef struct {
    int32_t sample_rate;     /* 16000 */
    int32_t n_mels;          /* 128   (1..256) */
    int32_t n_fft;           /* 512   (any power of two 64..2048: LS-EEND uses nextPow2(winLength), LSEENDTypes.swift:55-57;
                                       the batched NeMo configuration n_fft = 512 takes the tuned kernels) */
    int32_t hop;             /* 160 */
    int32_t win;             /* 400   (<= n_fft) */
    float preemph;           /* 0.97 */
    int32_t pad_to;          /* 0 (treated as 1, :72) */
    float log_floor;         /* 2^-24 */
    int32_t floor_mode;      /* FA_MEL_FLOOR_* */
    int32_t window_periodic; /* 0 symmetric / 1 periodic (:553-562) */
    int32_t padding_mode;    /* FA_MEL_PAD_* */
    int32_t layout;          /* FA_MEL_LAYOUT_* */
    /* Extensions beyond AudioMelSpectrogram (fa_mel_default_config sets the values that reproduce it): the torchaudio-
     * flavoured front end of LuxTtsMelExtractor.extract (FluidAudio/TTS/LuxTts/LuxTtsMelExtractor.swift:52-132), the
     * reference's only mel path with a golden vector in its tests. */
    float power;             /* 2 = power spectrum (:459-481; 0 is read as 2), 1 = magnitude (LuxTts :90-96) */
    int32_t center_pad;      /* FA_MEL_CENTER_* ; only meaningful with FA_MEL_PAD_CENTER */
    int32_t mel_scale;       /* FA_MEL_SCALE_* */
    int32_t tail_mode;       /* FA_MEL_TAIL_* */
    const float *filterbank; /* optional HOST table [n_mels][n_fft/2 + 1] that replaces the built-in bank; NULL = mel_scale */
} fa_mel_config;
enum { FA_MEL_CENTER_ZERO = 0,     /* zero padding of n_fft/2 (:206-217) */
       FA_MEL_CENTER_REFLECT = 1   /* torch pad_mode="reflect" (LuxTts :58-66) */ };
enum { FA_MEL_SCALE_SLANEY = 0,    /* Slaney scale, area-normalised triangles (:564-642) */
       FA_MEL_SCALE_HTK_NONORM = 1 /* torchaudio melscale_fbanks(norm: nil, mel_scale: "htk") (LuxTts :160-189) */ };
enum { FA_MEL_TAIL_ZERO = 0,       /* frames past the signal see zeros (truncated windows, :412) */
       FA_MEL_TAIL_REPLICATE = 1   /* frames >= the signal's own frame count repeat its last frame (lhotse alignment, LuxTts :124-128) */ };

void fa_mel_default_config(fa_mel_config *cfg);
/* Frame count T the reference would emit for n_samples (:192-197, :335-347, :133); 0 when its guard fires. */
int32_t fa_mel_num_frames(const fa_mel_config *cfg, int64_t n_samples);
/* ceil(T / pad_to) * pad_to (:204, :354). */
int32_t fa_mel_padded_frames(const fa_mel_config *cfg, int32_t frames);

/* A plan fixes the batch geometry (utterance offsets), the tables (Hann window, Slaney
 * filterbank in sparse form) and the launch grid; executing it is a pure kernel launch. */
typedef struct fa_mel_plan fa_mel_plan;

/* offsets: HOST array of B+1 sample offsets into the packed pcm buffer (utterance b is
 *          pcm[offsets[b] .. offsets[b+1])).
 * expected_frames: HOST array of B frame-count overrides (expectedFrameCount, :329,:347)
 *          or NULL.
 * frame_stride: allocated frames per utterance in the output (>= padded frames of every
 *          utterance); 0 = use the largest padded frame count in the batch.
 * Output addressing: utterance b starts at mel + b * fa_mel_plan_utt_stride(plan);
 *   MEL_MAJOR  : mel[b][m][t] at m*frame_stride + t     FRAME_MAJOR: mel[b][t][m] at t*n_mels + m
 * Frames t >= T(b) inside the allocation are written as 0 (padValue, :39). */
fa_status fa_mel_plan_create(fa_ctx *ctx, const fa_mel_config *cfg, const int64_t *offsets, int32_t batch,
                             const int32_t *expected_frames, int32_t frame_stride, fa_mel_plan **out);
void fa_mel_plan_destroy(fa_mel_plan *plan);
int64_t fa_mel_plan_utt_stride(const fa_mel_plan *plan);   /* floats per utterance in the output */
int32_t fa_mel_plan_frame_stride(const fa_mel_plan *plan);
int64_t fa_mel_plan_total_frames(const fa_mel_plan *plan); /* sum of T(b) */

/* d_pcm: device float[offsets[B]]; d_last_samples: device float[B] (lastAudioSample, :186) or NULL = 0;
 * d_mel: device float[B * utt_stride]; d_mel_lengths: device int32[B] (melLength) or NULL. */
fa_status fa_mel_execute_dev(fa_mel_plan *plan, const float *d_pcm, const float *d_last_samples,
                             float *d_mel, int32_t *d_mel_lengths);

/* Host-buffer convenience (the shape of a loop of computeFlat calls): copies pcm in, runs
 * the plan, copies mel (+lengths) out, synchronises.  When pcm AND mel are page-locked (fa_host_alloc) the batch is
 * processed in ~64 MB slices whose uploads overlap the downloads of the slices before them (both PCIe directions busy). */
fa_status fa_mel_batch(fa_ctx *ctx, const fa_mel_config *cfg, const float *pcm, const int64_t *offsets,
                       int32_t batch, const float *last_samples, const int32_t *expected_frames,
                       int32_t frame_stride, float *mel, int32_t *mel_lengths);

/* NeMo per_feature normalisation as applied by UnifiedMelExtractor.normalizePerFeature
 * (FluidAudio/ASR/Parakeet/Unified/UnifiedMelExtractor.swift:91-113), in place on a MEL_MAJOR tensor
 * d_mel[batch][n_mels][frame_stride]: per (utterance, mel) row, over the first valid_frames[b] frames, subtract the mean
 * and divide by (unbiased std + 1e-5); frames valid..frames-1 become 0.  valid_frames[b] = min(validCount / hop, T) is
 * the caller's (:66). */
fa_status fa_mel_normalize_per_feature_dev(fa_ctx *ctx, float *d_mel, int32_t batch, int32_t n_mels, int32_t frame_stride,
                                           int32_t frames, const int32_t *d_valid_frames);

/* Host copies of the tables (createHannWindow :553-562, createMelFilterbank :564-642). */
fa_status fa_mel_hann_window(const fa_mel_config *cfg, float *out /* win */);
fa_status fa_mel_filterbank(const fa_mel_config *cfg, float *out /* n_mels * (n_fft/2+1) */);

/* ------------------------------------------------------------------ argmax / CTC ---- */
/* Replaces LogitsArgmax.argmaxPerFrame (FluidAudio/ASR/Shared/LogitsArgmax.swift:16-55) and the
 * greedy collapse of ctcGreedyDecode (FluidAudio/ASR/Parakeet/SlidingWindow/CTC/CtcDecoder.swift:15-36,
 * 45-70; FluidAudio/ASR/SenseVoice/SenseVoiceManager.swift:119-126). */
enum { FA_DTYPE_F32 = 0, FA_DTYPE_F16 = 1 };

/* logits: batch matrices, matrix b at element offset b*matrix_stride, row t at t*row_stride,
 *         `vocab` valid elements per row (padding columns are never read).
 * valid_frames: int32[batch] (frames to decode per matrix, <= frames) or NULL = all.
 * frame_ids (optional): int32[batch * frames] per-frame argmax (argmaxPerFrame output).
 * token_ids: int32[batch * frames] collapsed ids (first token_lens[b] valid per matrix).
 * Ties -> lowest index; NaN never wins; an all-NaN/-inf row yields 0. */
fa_status fa_ctc_greedy_batch_dev(fa_ctx *ctx, const void *d_logits, int32_t dtype, int32_t batch, int32_t frames,
                                  int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                                  const int32_t *d_valid_frames, int32_t blank_id, int32_t *d_frame_ids,
                                  int32_t *d_token_ids, int32_t *d_token_lens);
fa_status fa_ctc_greedy_batch(fa_ctx *ctx, const void *logits, int32_t dtype, int32_t batch, int32_t frames,
                              int32_t vocab, int64_t row_stride, int64_t matrix_stride,
                              const int32_t *valid_frames, int32_t blank_id, int32_t *frame_ids,
                              int32_t *token_ids, int32_t *token_lens);

/* ctcGreedyDecode(logProbs: [[Float]], ...) — the array-of-arrays overload (CtcDecoder.swift:15-36), whose semantics differ from the
 * [1, T, V] overload above (:45-70) in three ways, all mirrored here:
 *   - the scan is seeded with frame[0] (:25), so a frame whose element 0 is NaN decodes to index 0;
 *   - every frame has its own length (:26): row r is values[row_offsets[r] .. row_offsets[r+1]);
 *   - an empty frame is skipped before `prev` is updated (:23): `a, [], a` collapses to ONE a.
 * utt_rows: int64[batch+1] row ranges of the utterances (NULL with batch == 1: all rows are one utterance).
 * frame_ids (optional): int32[total_rows], -1 for an empty frame.  token_ids: int32[total_rows]; utterance u writes its
 * token_lens[u] ids from token_ids[utt_rows[u]].  fp32 only ([[Float]]). */
fa_status fa_ctc_greedy_rows_dev(fa_ctx *ctx, const float *d_values, const int64_t *d_row_offsets, int64_t total_rows,
                                 const int64_t *d_utt_rows, int32_t batch, int32_t blank_id, int32_t *d_frame_ids,
                                 int32_t *d_token_ids, int32_t *d_token_lens);
fa_status fa_ctc_greedy_rows(fa_ctx *ctx, const float *values, const int64_t *row_offsets, int64_t total_rows,
                             const int64_t *utt_rows, int32_t batch, int32_t blank_id, int32_t *frame_ids,
                             int32_t *token_ids, int32_t *token_lens);

/* Per-frame log-softmax with temperature and blank bias: CtcKeywordSpotter.makeLogProbs / logSoftmax
 * (FluidAudio/ASR/Parakeet/SlidingWindow/CustomVocabulary/WordSpotting/CtcKeywordSpotter+Inference.swift:350-431).
 * DEVICE pointers; logits addressed like fa_ctc_greedy_batch_dev; d_log_probs: float[batch][frames][vocab] contiguous.
 * blank_bias is subtracted from column blank_id when != 0 (:397-399); temperature divides the logits when != 1 (:412). */
fa_status fa_ctc_log_softmax_batch_dev(fa_ctx *ctx, const void *d_logits, int32_t dtype, int32_t batch, int32_t frames,
                                       int32_t vocab, int64_t row_stride, int64_t matrix_stride, float temperature,
                                       float blank_bias, int32_t blank_id, float *d_log_probs);

/* CTC word spotting (CTC-WS, arXiv:2406.07096) over such log-probabilities, batched over utterances: CtcDPAlgorithm.fillDPTable,
 * ctcWordSpotMultiple, ctcWordSpotConstrained and nonWildcardCount (…/WordSpotting/CtcDPAlgorithm.swift:121-392) and the per-term loop
 * of CtcKeywordSpotter.spotKeywordsFromLogProbs (…/WordSpotting/CtcKeywordSpotter.swift:191-254).  Scores and frames are the
 * reference's bit for bit.  Not covered: the tokenizer, minTermLength (a text property: leave such terms out), NaN log-probabilities.
 * A keyword is a run of token ids; FA_KWS_WILDCARD matches any frame at no cost, any other id outside [0, vocab) can never match
 * (it emits -FLT_MAX), a blank id outside [0, vocab) emits 0.  A keyword of more than FA_KWS_MAX_TOKENS tokens is INVALID_ARGUMENT. */
typedef struct { int32_t utterance, keyword; float score; int32_t start_frame, end_frame; } fa_kws_detection;
typedef struct { int32_t utterance, keyword, start_frame, end_frame; } fa_kws_window;
enum { FA_KWS_WILDCARD = -1, FA_KWS_MAX_TOKENS = 127 };
/* The threshold of a term (CtcKeywordSpotter.swift:217-222): base - Float(max(0, token_count - 3)) * 1.0, or -15.0 without a base. */
float fa_kws_adjusted_threshold(int32_t has_base, float base, int32_t token_count);
/* ctcWordSpotMultiple for every (utterance, keyword) pair.  The log-probs are addressed like the logits of fa_ctc_greedy_batch_dev
 * (a DEVICE pointer read in stream order for _dev, a HOST pointer otherwise); everything else is HOST memory.  valid_frames
 * int32[batch] (nullable: all frames).  Keyword k is keyword_tokens[keyword_offsets[k] .. keyword_offsets[k + 1]); an empty one
 * contributes nothing.  min_scores float[keywords] are the thresholds as ctcWordSpotMultiple takes them (NULL: -15 for all).
 * The records come ordered by utterance, then keyword, then as the reference's array holds them (by start frame after the merge).
 * dets HOST [capacity]; *count is set even when dets is NULL (SUCCESS) or too small (OUTPUT_TOO_SMALL, the first `capacity` records
 * are written); utterance_counts HOST int64[batch] (nullable).  Argument errors are answered before any device work.
 * Synchronous.  Device scratch is O(pairs + capacity) records; only candidate records come back over PCIe. */
fa_status fa_ctc_kws_spot_batch_dev(fa_ctx *ctx, const float *d_log_probs, int32_t batch, int32_t frames, int32_t vocab,
                                    int64_t row_stride, int64_t matrix_stride, const int32_t *valid_frames,
                                    const int32_t *keyword_tokens, const int64_t *keyword_offsets, int32_t keywords,
                                    const float *min_scores, int32_t blank_id, int32_t merge_overlap, fa_kws_detection *dets,
                                    int64_t capacity, int64_t *count, int64_t *utterance_counts);
fa_status fa_ctc_kws_spot_batch(fa_ctx *ctx, const float *log_probs, int32_t batch, int32_t frames, int32_t vocab,
                                int64_t row_stride, int64_t matrix_stride, const int32_t *valid_frames,
                                const int32_t *keyword_tokens, const int64_t *keyword_offsets, int32_t keywords,
                                const float *min_scores, int32_t blank_id, int32_t merge_overlap, fa_kws_detection *dets,
                                int64_t capacity, int64_t *count, int64_t *utterance_counts);
/* ctcWordSpotConstrained for n_windows (utterance, keyword, [start_frame, end_frame)) windows: out[w] answers windows[w], frames in
 * the utterance's coordinates; (-inf, clampedStart, clampedStart) for an empty keyword, an empty window or one shorter than the
 * keyword.  A window's utterance or keyword outside the batch is INVALID_ARGUMENT.  _dev: the log-probs are a DEVICE pointer; otherwise a
 * HOST pointer.  One host synchronisation behind the uploads. */
fa_status fa_ctc_kws_score_windows_dev(fa_ctx *ctx, const float *d_log_probs, int32_t batch, int32_t frames, int32_t vocab,
                                       int64_t row_stride, int64_t matrix_stride, const int32_t *valid_frames,
                                       const int32_t *keyword_tokens, const int64_t *keyword_offsets, int32_t keywords,
                                       const fa_kws_window *windows, int64_t n_windows, int32_t blank_id, fa_kws_detection *out);
fa_status fa_ctc_kws_score_windows(fa_ctx *ctx, const float *log_probs, int32_t batch, int32_t frames, int32_t vocab,
                                   int64_t row_stride, int64_t matrix_stride, const int32_t *valid_frames,
                                   const int32_t *keyword_tokens, const int64_t *keyword_offsets, int32_t keywords,
                                   const fa_kws_window *windows, int64_t n_windows, int32_t blank_id, fa_kws_detection *out);

/* The vocabulary rescorer's term-centric path (…/CustomVocabulary/Rescorer/VocabularyRescorer+TokenRescoring.swift:693-1034, :272-307,
 * +TokenEvaluation.swift:29-173, :319-377, +Utilities.swift:8-17, :43-62, :87-96, :321-339, VocabularyRescorer.swift:111-129): candidate
 * discovery by string similarity on the device, the CTC verdicts through the window kernels above, the arbitration on the host.
 * Similarities are the reference's fp32 values bit for bit.  The caller's: normalizeForSimilarity and the split into Characters (a word
 * or a form is a row of int32 symbols, any injective numbering of the Characters with FA_VR_SPACE for the space), both tokenizers,
 * buildWordTimings, the stopword lists (two flag bits per word), preserveCapitalization and the rebuilt text, the evidence records' UTF-8
 * ranges and reason strings.  Not covered: the word-centric path, collectSpotterAnchoredCandidates (this library behaves as
 * spotterRescueEnabled = false does; fa_vocab_rescore_decide takes candidate records from anywhere), the "No tokenizer" branch. */
enum { FA_VR_SPACE = 32, FA_VR_MAX_FORM = 64, FA_VR_MAX_ALPHABET = 1024 };
enum { FA_VR_ORIGIN_MULTI_WORD = 1, FA_VR_ORIGIN_SINGLE_WORD = 2 };
enum { FA_VR_WORD_STOPWORD = 1, FA_VR_WORD_MULTI_WORD_STOPWORD = 2 };
enum { FA_VR_APPLIED = 1, FA_VR_SUPERSEDED = 2, FA_VR_REJECTED = 3, FA_VR_UNAVAILABLE = 4 };
/* term: the term's index in the build's input; form: the index among the term's kept forms (the matched alias; 0 is the canonical form
 * where that is kept), -1 where no form was better than similarity 0 */
typedef struct { int32_t utterance, term, first_word, span_len, origin, form; float similarity; } fa_vr_candidate;
typedef struct {
    int32_t use_adaptive_thresholds;     /* 1 */
    int32_t reference_token_count;       /* 3 */
    int32_t short_term_taper_pivot;      /* 1: no taper */
    float short_term_taper_exponent;     /* 2.0 */
} fa_vr_boost_config;
typedef struct {
    double frame_duration;               /* seconds per CTC frame; > 0 (0.08) */
    double margin_seconds;               /* 0.10 */
    float cbw;                           /* 3.0 */
    int32_t blank_id;                    /* 1024 */
    fa_vr_boost_config boost;
} fa_vr_decide_config;
/* term_score: the better of the term's tokens and its alternative tokens (alt_won) in the window [start_frame, end_frame); compared = 0:
 * the phrase has no tokens (or the term none), nothing is replaced, original_score = -inf, boost = 0, boosted_score = term_score.
 * Non-finite scores are reported as they are. */
typedef struct {
    float term_score, original_score, boost, boosted_score;
    int32_t alt_won, compared, should_replace, outcome, start_frame, end_frame;
} fa_vr_verdict;
void fa_vocab_rescore_default_config(fa_vr_decide_config *cfg);
/* adaptiveCbw; log2 and pow are evaluated in fp64 and rounded once to fp32, the arithmetic round them is the reference's fp32.  cfg NULL: the defaults. */
float fa_vocab_rescore_boost(float cbw, int32_t token_count, const fa_vr_boost_config *cfg);
/* The vocabulary as a position-independent blob of int32 words.  HOST memory only.  Term t: char_counts[t] = vocabTerm.count,
 * min_similarities[t] (below 0: none; the array NULL: none at all), and the rows [term_rows[t], term_rows[t + 1]) of the ragged table
 * symbols / row_offsets as its forms in buildNormalizedForms' order, the canonical one first (it may be empty).  Empty forms and later
 * duplicates are dropped; a term with char_count < min_term_length or without a form left is skipped.  A form of more than
 * FA_VR_MAX_FORM symbols, or FA_VR_MAX_ALPHABET - 1 or more distinct symbols, is INVALID_ARGUMENT.  *words_needed is set;
 * capacity_words 0 only asks for it, a smaller buffer than needed is OUTPUT_TOO_SMALL.  text (nullable) [text_capacity] receives the
 * reason of a refusal. */
fa_status fa_vocab_rescore_build(const int32_t *char_counts, const float *min_similarities, const int64_t *term_rows, const int64_t *row_offsets,
                                 const int32_t *symbols, int32_t terms, int32_t min_term_length, int32_t *blob, int64_t capacity_words,
                                 int64_t *words_needed, char *text, int64_t text_capacity);
/* The two loops of :755-1033 for every (utterance, term).  Everything is HOST memory; the blob is checked whole before it is uploaded.
 * Utterance u has the words [utterance_offsets[u], utterance_offsets[u + 1]); word w the symbols [word_offsets[w], word_offsets[w + 1])
 * of word_symbols (rows back to back in word order; a row may be empty) and the flag byte word_flags[w] (FA_VR_WORD_*).  The records
 * come in the reference's append order: utterance, term, multi-word before single-word, multi-word by span length then start,
 * single-word by word.  The capacity contract is fa_ctc_kws_spot_batch's: *count is always set, utterance_counts int64[batch]
 * (nullable), OUTPUT_TOO_SMALL writes the first `capacity` records.  One host synchronisation, unless the survivors overflow the
 * device arena (65536 records or `capacity`, whichever is more; FA_VR_ARENA=records for tests): then the walk runs once more with room
 * for the count it reported. */
fa_status fa_vocab_rescore_candidates(fa_ctx *ctx, const int32_t *blob, int64_t blob_words, const int64_t *utterance_offsets, int32_t batch,
                                      const int64_t *word_offsets, const int32_t *word_symbols, const uint8_t *word_flags, float min_similarity,
                                      fa_vr_candidate *candidates, int64_t capacity, int64_t *count, int64_t *utterance_counts);
/* evaluateCTCMatch for every candidate, then arbitratePendingReplacements per utterance.  The log-probs are addressed like
 * fa_ctc_kws_score_windows(_dev)'s; everything else is HOST memory.  candidates [n_candidates] in the order the arbitration takes as
 * candidate order; word times fp64 per word of the utterance_offsets table; term t has the tokens
 * term_tokens[term_token_offsets[t] ..) and the alternative tokens alt_tokens[alt_token_offsets[t] ..) (alt_token_offsets NULL or an
 * empty row: none); candidate c the original phrase's tokens phrase_tokens[phrase_token_offsets[c] ..).  occupied (nullable): a byte per
 * word, non-zero for an index that is taken before the pass.  verdicts [n_candidates]; applied [n_candidates] receives, utterance after
 * utterance, the indices of the applied candidates in application order, applied_counts int64[batch] how many each utterance has (both
 * nullable).  The three scores of every candidate go through one batched call of the window kernels. */
fa_status fa_vocab_rescore_decide_dev(fa_ctx *ctx, const float *d_log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride,
                                      int64_t matrix_stride, const int32_t *valid_frames, const fa_vr_decide_config *cfg,
                                      const fa_vr_candidate *candidates, int64_t n_candidates, const int64_t *utterance_offsets,
                                      const double *word_starts, const double *word_ends, int32_t terms, const int32_t *term_tokens,
                                      const int64_t *term_token_offsets, const int32_t *alt_tokens, const int64_t *alt_token_offsets,
                                      const int32_t *phrase_tokens, const int64_t *phrase_token_offsets, const uint8_t *occupied,
                                      fa_vr_verdict *verdicts, int32_t *applied, int64_t *applied_counts);
fa_status fa_vocab_rescore_decide(fa_ctx *ctx, const float *log_probs, int32_t batch, int32_t frames, int32_t vocab, int64_t row_stride,
                                  int64_t matrix_stride, const int32_t *valid_frames, const fa_vr_decide_config *cfg,
                                  const fa_vr_candidate *candidates, int64_t n_candidates, const int64_t *utterance_offsets,
                                  const double *word_starts, const double *word_ends, int32_t terms, const int32_t *term_tokens,
                                  const int64_t *term_token_offsets, const int32_t *alt_tokens, const int64_t *alt_token_offsets,
                                  const int32_t *phrase_tokens, const int64_t *phrase_token_offsets, const uint8_t *occupied,
                                  fa_vr_verdict *verdicts, int32_t *applied, int64_t *applied_counts);

/* ------------------------------------------------------------------ TDT ------------- */
/* Control flow of TdtDecoderV3.decodeWithTimings (FluidAudio/ASR/Parakeet/SlidingWindow/TDT/Decoder/TdtDecoderV3.swift:103-607)
 * and its helpers (TdtFrameNavigation.swift:20-105, TdtDurationMapping.swift:17-31, TdtConfig.swift:13-26).  The decoder
 * LSTM and joint network are CoreML models outside the reference tree: token parity is UNPINNED; the device entry
 * replays the loop over tables of the joint's decisions indexed by (decoder steps taken u, encoder frame t). */
typedef struct {
    int32_t blank_id;                /* 8192 */
    int32_t max_symbols_per_step;    /* 10 */
    int32_t max_tokens_per_chunk;    /* 150 */
    int32_t consecutive_blank_limit; /* 5 */
    int32_t n_duration_bins;         /* 5 (<= 8) */
    int32_t duration_bins[8];        /* 0 1 2 3 4 */
} fa_tdt_config;
void fa_tdt_default_config(fa_tdt_config *cfg);
/* calculateInitialTimeIndices (TdtFrameNavigation.swift:20-49); has_time_jump == 0 <=> timeJump == nil */
int32_t fa_tdt_initial_time_index(int32_t has_time_jump, int32_t time_jump, int32_t context_frame_adjustment);
/* initializeNavigationState (:59-78) */
void fa_tdt_navigation_state(int32_t time_indices, int32_t encoder_sequence_length, int32_t actual_audio_frames,
                             int32_t *effective_length, int32_t *safe_time_indices, int32_t *last_timestep, int32_t *active);
/* calculateFinalTimeJump (:91-105); *has_value == 0 <=> nil (last chunk) */
int32_t fa_tdt_final_time_jump(int32_t current_time_indices, int32_t effective_length, int32_t is_last_chunk, int32_t *has_value);
/* mapDurationBin (TdtDurationMapping.swift:17-22): RUNTIME_ERROR when out of range */
fa_status fa_tdt_map_duration_bin(const fa_tdt_config *cfg, int32_t bin_index, int32_t *duration);
/* clampProbability (:28-31) */
float fa_tdt_clamp_probability(float value);
/* Batched greedy walk, one chunk per table set.  DEVICE pointers.  d_tok/d_bin/d_prob: [batch][U][T] joint decisions;
 * per chunk: d_enc_len (encoderSequenceLength), d_audio_frames (NULL = enc_len), d_t0 (initial time index, NULL = 0),
 * d_is_last (NULL = 0), d_global_offset (NULL = 0), d_emit_after (emitTokensAfterGlobalFrame, NULL or < 0 = nil).
 * Outputs per chunk: up to max_out (token, global timestamp, duration, confidence), their count, the final time index
 * (INT32_MIN when the reference returns before touching timeJump), decoder steps taken, and a status (RUNTIME_ERROR for
 * a duration bin out of range, OUTPUT_TOO_SMALL when U or max_out is exhausted). */
fa_status fa_tdt_greedy_tables_dev(fa_ctx *ctx, const fa_tdt_config *cfg, const int32_t *d_tok, const int32_t *d_bin,
                                   const float *d_prob, int32_t batch, int32_t U, int32_t T, const int32_t *d_enc_len,
                                   const int32_t *d_audio_frames, const int32_t *d_t0, const int32_t *d_is_last,
                                   const int32_t *d_global_offset, const int32_t *d_emit_after, int32_t max_out,
                                   int32_t *d_out_tok, int32_t *d_out_time, int32_t *d_out_dur, float *d_out_conf,
                                   int32_t *d_out_count, int32_t *d_final_time, int32_t *d_final_u, int32_t *d_status);

/* The same walk with the joint decisions computed on the fly from joint LOGITS: d_logits[batch][U][T][row_stride] (fp32 or
 * fp16), token logits in [0, vocab_with_blank), the n_duration_bins duration logits right behind them.  Per visited (u, t):
 * token = first-index argmax of the token logits (the tie / NaN rule of LogitsArgmax.argmaxPerFrame), probability = its
 * softmax probability, duration bin = first-index argmax of the duration logits — what the reference's JointDecision model
 * returns (TdtModelInference.swift:84-188).  One workgroup per chunk reads only the rows on the greedy path.  The joint /
 * decoder networks are not in the reference tree: token parity UNPINNED. */
fa_status fa_tdt_greedy_logits_dev(fa_ctx *ctx, const fa_tdt_config *cfg, const void *d_logits, int32_t dtype, int32_t batch,
                                   int32_t U, int32_t T, int32_t vocab_with_blank, int64_t row_stride, const int32_t *d_enc_len,
                                   const int32_t *d_audio_frames, const int32_t *d_t0, const int32_t *d_is_last,
                                   const int32_t *d_global_offset, const int32_t *d_emit_after, int32_t max_out,
                                   int32_t *d_out_tok, int32_t *d_out_time, int32_t *d_out_dur, float *d_out_conf,
                                   int32_t *d_out_count, int32_t *d_final_time, int32_t *d_final_u, int32_t *d_status);

/* ---- language-aware decoding: transcribe(..., language:) (TdtDecoderV3.swift:284-299, 371-387, 635-703;
 * Shared/TokenLanguageFilter.swift:81-186).  One byte of class bits per token: */
#define FA_TDT_CLASS_LATIN_OK 1     /* TokenLanguageFilter.matches(text, .latin) */
#define FA_TDT_CLASS_CYRILLIC_OK 2  /* ... .cyrillic */
#define FA_TDT_CLASS_GREEK_OK 4     /* ... .greek */
#define FA_TDT_CLASS_IN_VOCAB 8     /* vocabulary[id] exists */
#define FA_TDT_CLASS_BLOCKLISTED 16 /* the id is on the caller's blocklist (the reference's englishBlocklistIds, French only) */
enum { FA_TDT_SCRIPT_LATIN = 0, FA_TDT_SCRIPT_CYRILLIC = 1, FA_TDT_SCRIPT_GREEK = 2 };
#define FA_TDT_ROUTE_SCRIPT_SWAP 1     /* the script filter replaced the joint's winner */
#define FA_TDT_ROUTE_BLOCKLIST_SWAP 2  /* the blocklist pass replaced the (possibly already replaced) label */
#define FA_TDT_MAX_TOP_K 64            /* the reference's joint hands back K = 64 candidates */
/* The class bytes of a vocabulary.  HOST pointers, no context, no GPU.  utf8_tokens[i]: the NUL-terminated UTF-8 text of token i;
 * NULL, or present[i] == 0 where present is not NULL, leaves IN_VOCAB clear (the script bits are then those of the empty text).
 * matches (TokenLanguageFilter.swift:81-134): every U+2581 scalar is stripped, an empty remainder matches every script, the rest
 * is checked scalar by scalar against the script's ranges.  INVALID_ARGUMENT for text that is not UTF-8 (overlong forms,
 * surrogates and scalars above U+10FFFF included) and for a blocklist id outside [0, vocab_with_blank). */
fa_status fa_tdt_token_classes(const char *const *utf8_tokens, const int32_t *present, int32_t vocab_with_blank,
                               const int32_t *blocklist_ids, int32_t n_block, uint8_t *classes);
/* What the joint's two top-K outputs hold, as THIS LIBRARY defines them (CoreML's order among equal logits is unspecified):
 * per row the min(K, vocab_with_blank) tokens in order of descending key, then ascending id; key = the logit widened to float32,
 * NaN counting as -inf; comparison by value (-0.0 == +0.0).  d_rows[R][row_stride] (fp32 / fp16), 1 <= K <= 64.  d_ids and
 * d_logits [R][K] (the reported logit is the widened value, NaN reported as -inf; unused slots: id -1, logit -inf), d_counts [R]
 * (NULL: not wanted).  One wavefront per row. */
fa_status fa_tdt_topk_rows_dev(fa_ctx *ctx, const void *d_rows, int32_t dtype, int64_t R, int32_t vocab_with_blank,
                               int64_t row_stride, int32_t K, int32_t *d_ids, float *d_logits, int32_t *d_counts);
/* fa_tdt_greedy_logits_dev with the reference's language mode at the main-loop and the blank-advance decisions (never in the
 * last-chunk flush, :602-605).  d_classes[vocab_with_blank]: the bytes of fa_tdt_token_classes on the device; script: FA_TDT_SCRIPT_*.
 * Script filter (:676-703): a non-blank winner that is IN_VOCAB and does not match the script is replaced by the first entry of
 * the row's top-K list (fa_tdt_topk_rows_dev's definition, K = top_k) that is IN_VOCAB and matches; blank is a legal candidate;
 * confidence = clamp(exp(x_best - M) / sum over the list of exp(x_j - M)), 0 where the list's maximum M is not finite.
 * Blocklist (:635-667), when use_blocklist != 0, on the possibly replaced label: a non-blank BLOCKLISTED label is replaced by the
 * first list entry that is not blank, not BLOCKLISTED, IN_VOCAB and LATIN_OK, with the same confidence formula.  Without such an
 * entry a filter changes nothing.  Duration, blank test, inner loop and emission follow on the filtered label.
 * d_out_route[batch][max_out]: FA_TDT_ROUTE_* bits per emitted token; d_swap_counts[batch][2]: decisions whose label the script
 * filter / the blocklist replaced, emitted or not.  INVALID_ARGUMENT (nothing launched, nothing written) for script or top_k out
 * of range or a NULL d_classes / d_swap_counts. */
fa_status fa_tdt_greedy_logits_lang_dev(fa_ctx *ctx, const fa_tdt_config *cfg, const void *d_logits, int32_t dtype, int32_t batch,
                                        int32_t U, int32_t T, int32_t vocab_with_blank, int64_t row_stride, const int32_t *d_enc_len,
                                        const int32_t *d_audio_frames, const int32_t *d_t0, const int32_t *d_is_last,
                                        const int32_t *d_global_offset, const int32_t *d_emit_after, int32_t max_out,
                                        int32_t *d_out_tok, int32_t *d_out_time, int32_t *d_out_dur, float *d_out_conf,
                                        int32_t *d_out_count, int32_t *d_final_time, int32_t *d_final_u, int32_t *d_status,
                                        const uint8_t *d_classes, int32_t script, int32_t use_blocklist, int32_t top_k,
                                        int32_t *d_out_route, int32_t *d_swap_counts);

/* ------------------------------------------------------------------ streaming RNN-T ------------- */
/* The streaming ASR path: the greedy loop of RnntDecoder.decodeWithEOU (ASR/Parakeet/Streaming/RnntDecoder.swift:73-127; the
 * Nemotron managers run the same loop behind a speculative scan, StreamingNemotronMultilingualAsrManager+Decode.swift:189-251,
 * 278-440) and the decode-time hotword biasing of Streaming/Nemotron/NemotronVocabularyBias.swift:55-340, 465-498.
 *
 * ---- the bias tables (HOST pointers, no context, no GPU).  Lower-casing + NFC and the letter-count guard of usableSurfaces
 * (:203-212, it counts grapheme clusters) are the CALLER's; everything below works on Unicode scalars. */
#define FA_RNNT_BIAS_DEFAULT_BOOST 4.5f /* NemotronVocabularyBias.defaultBoost (:90) */
#define FA_RNNT_BIAS_MAX_BOOST 6.0f     /* NemotronVocabularyBias.maxBoost (:98) */
#define FA_RNNT_BIAS_MAX_FORM 256       /* the longest piece form, in scalars, a table may hold */
/* effectiveBoost (:196-199): the weight when one is set and <= FA_RNNT_BIAS_MAX_BOOST, default_boost otherwise. */
float fa_rnnt_bias_effective_boost(int32_t has_weight, float weight, float default_boost);
/* init (:126-182) as one position-independent blob of int32 words, to be uploaded as it is (layout: csrc/rnnt_bias_core.h).
 * folded_pieces[vocab]: the folded piece of every token id as NUL-terminated UTF-8, NULL: the id has no piece; a piece that starts
 * with '<' and ends with '>' never enters the index or the tail (:147-156).  folded_surfaces[n_surfaces] with boosts[n_surfaces]
 * > 0: the folded surfaces (texts and aliases) that passed the caller's guards.  The library takes pieceForm (:233-250: split at
 * White_Space scalars, U+2581 in front of every word unless the first scalar is CJK, :219-228), builds the trie (:160-175) and
 * stores with every node the list accumulate (:310-339) gives from its depth for every entry under it: every vocabulary piece
 * equal to a prefix of the rest of the form, never the bare marker, from depth 0 of an anchored form only after two letters, all
 * ids of one folded piece together; one entry per id with the strongest boost, ascending id.  The root's list is
 * freshStartCandidates.  *tail_cap: the longest form in scalars.
 * capacity_words == 0 asks for *words_needed only; a smaller capacity than needed: OUTPUT_TOO_SMALL.  No surface, or none with a
 * scalar besides white space: SUCCESS with *words_needed = 0 and *tail_cap = 0 — decode without a bias.  INVALID_ARGUMENT: text
 * that is not UTF-8 (as in fa_tdt_token_classes), a boost <= 0 or NaN, a form above FA_RNNT_BIAS_MAX_FORM scalars, NULL outputs. */
fa_status fa_rnnt_bias_build(const char *const *folded_pieces, int32_t vocab, const char *const *folded_surfaces, const float *boosts,
                             int32_t n_surfaces, int32_t *blob, int64_t capacity_words, int64_t *words_needed, int32_t *tail_cap);
/* candidates() (:280-306) after observe (:254-261) of observed[n_observed] from a reset match state: ids ascending, one entry per
 * id with the strongest boost; ids without a piece leave the state alone.  Walks blob[words] through the accessors the kernel
 * uses: the header and every offset are checked, a malformed or truncated blob is INVALID_ARGUMENT and is never read out of
 * bounds.  *count is the number of candidates; more than capacity: OUTPUT_TOO_SMALL, nothing written but *count. */
fa_status fa_rnnt_bias_candidates(const int32_t *blob, int64_t words, const int32_t *observed, int32_t n_observed, int32_t *ids,
                                  float *boosts, int32_t capacity, int32_t *count);

typedef struct {
    int32_t blank_id;
    int32_t eou_id;               /* the end-of-utterance token (RnntDecoder.swift:32), -1: none */
    int32_t max_symbols_per_step; /* 10 */
} fa_rnnt_config;
/* blank_id 1024 (NemotronStreamingConfig.swift:45), eou_id -1, max_symbols_per_step 10. */
void fa_rnnt_default_config(fa_rnnt_config *cfg);
/* The greedy walk for a batch of streams, one wavefront per stream.  d_logits[batch][U][T][row_stride] (fp32 / fp16): the joint
 * logits for (u = decoder steps taken so far in this chunk, t = encoder frame), u as in fa_tdt_greedy_logits_dev; only the rows on
 * the greedy path are read.  d_frames[batch] = validOutLen, d_skip[batch] = skipFrames (NULL: 0): maxT = min(frames, T), start =
 * min(skip, maxT) (:85-88).  For t in start ..< maxT up to max_symbols_per_step decisions at row (u, t): blank goes to the next
 * frame, eou_id sets d_eou and ends the stream, any other token is emitted with its chunk-local frame t, observed by the bias,
 * and followed by ++u (:98-123).  A decision needed at u >= U ends the stream with OUTPUT_TOO_SMALL; a token beyond max_out is
 * counted, not stored, and leaves OUTPUT_TOO_SMALL — as in the TDT walk.
 * A decision: plain = the first-index argmax of the vocab_with_blank logits (LogitsArgmax's rule: fp16 widened, NaN never wins,
 * nothing above -inf gives 0).  With d_bias (the blob on the device, bias_words words, tail_cap as fa_rnnt_bias_build returned
 * it), pickBiased (:482-498): over the depth-0 candidates and those of every live partial match with id < vocab_with_blank,
 * score = float32(logit[id] + boost); the best candidate replaces plain — blank included — only where its score is strictly
 * above logit[plain]; NaN on either side never flips.  TIE ORDER: the reference iterates a Swift Dictionary, whose order is
 * unspecified; THIS LIBRARY defines: the highest score, then the lowest token id.
 * d_out_plain[batch][max_out]: the displaced plain argmax where the bias flipped the emitted token, -1 otherwise (the reference's
 * FLUIDAUDIO_BIAS_LOG trace, :342-349, 500-511).
 * Match state: d_tail[batch][tail_cap] / d_tail_len[batch], the last folded scalars emitted (:254-261), read at entry and written
 * back at exit: two calls over a split chunk equal one call, and d_tail_len = 0 is resetMatchState (:265-268).
 * d_status[b]: INVALID_ARGUMENT (no walk, no token) where the blob's magic, version, vocab or tail_cap do not match the arguments;
 * RUNTIME_ERROR where an offset or length inside the blob leaves bias_words — the kernel checks each before it forms an address.
 * INVALID_ARGUMENT with nothing launched: NULL ctx / cfg / d_logits / d_frames / d_out_count / d_final_u / d_eou / d_status (and
 * the three token outputs where max_out > 0); batch, U, T or vocab_with_blank <= 0; row_stride < vocab_with_blank; max_out < 0;
 * tail_cap outside [0, FA_RNNT_BIAS_MAX_FORM]; a dtype that is neither; d_bias with a NULL d_tail or d_tail_len.
 * The decoder / joint networks are not in the reference tree: token parity against the models is UNPINNED; the matcher is pinned
 * by the reference's NemotronVocabularyBiasTests. */
fa_status fa_rnnt_greedy_logits_dev(fa_ctx *ctx, const fa_rnnt_config *cfg, const void *d_logits, int32_t dtype, int32_t batch,
                                    int32_t U, int32_t T, int32_t vocab_with_blank, int64_t row_stride, const int32_t *d_frames,
                                    const int32_t *d_skip, const int32_t *d_bias, int64_t bias_words, int32_t tail_cap,
                                    int32_t *d_tail, int32_t *d_tail_len, int32_t max_out, int32_t *d_out_tok,
                                    int32_t *d_out_frame, int32_t *d_out_plain, int32_t *d_out_count, int32_t *d_final_u,
                                    int32_t *d_eou, int32_t *d_status);

/* ------------------------------------------------------------------ AED greedy decoding ------ */
/* The host loop around the attention encoder-decoder models: Cohere Transcribe (FluidAudio/ASR/Cohere/CoherePipeline.swift:525-959)
 * and Canary (FluidAudio/ASR/Canary/CanaryManager.swift:50-275).  The networks, the mel front end, tokenizers, detokenisation and
 * CanaryKeywordBooster stay the caller's.  Every output is an integer or an exactly rounded fp32: the repetition penalty is ONE
 * IEEE fp32 divide or multiply per penalised id (the unit is built without contraction, denormals kept).
 * LIBRARY'S OWN DEFINITION: a NaN logit never wins (NaN logits are outside the reference's contract); the argmax is the lowest
 * index among the largest values, 0 where no value qualifies. */
enum { FA_AED_MODEL_COHERE = 0, FA_AED_MODEL_CANARY = 1 };
enum { FA_AED_FEED_TOKEN = 0, FA_AED_FEED_SEQUENCE = 1 };
enum { FA_AED_RUNNING = 0, FA_AED_END_EOS = 1, FA_AED_END_CAP = 2 };
/* The limits keep a step's LDS (one bit per id, two words per history position) within 48 KiB. */
enum { FA_AED_MAX_VOCAB = 1 << 18, FA_AED_MAX_SEQ = 2048, FA_AED_MAX_WINDOW_TOKENS = 64 };
typedef struct {
    int32_t mode;                /* FA_AED_FEED_TOKEN (Cohere: one token per step, prompt fed step by step) / FA_AED_FEED_SEQUENCE (Canary) */
    int32_t vocab;               /* 16384 */
    int32_t eos_id;              /* 3 */
    int32_t max_seq;             /* CohereAsrConfig.maxSeqLen 108 / CanaryConfig.maxDecoderSteps 128 (S) */
    int32_t max_new;             /* maxNewTokens 108; unused by the sequence feed */
    int32_t no_repeat_ngram;     /* 3; <= 0: off (Canary: 0) */
    float repetition_penalty;    /* 1.1; 1: off (Canary: 1) */
    int32_t window_tokens;       /* mergeTokenStreams windowTokens 32, 1 ... FA_AED_MAX_WINDOW_TOKENS */
    int32_t min_match;           /* minMatch 4 */
    int32_t reserved;
    int64_t chunk_samples;       /* 560000 (35 s) / 240000 (15 s) */
    int64_t hop_samples;         /* 480000 / 192000 */
} fa_aed_config;
/* model: FA_AED_MODEL_COHERE or FA_AED_MODEL_CANARY (anything else: Cohere). */
void fa_aed_default_config(fa_aed_config *cfg, int32_t model);
/* Output tokens an utterance can emit: token feed min(max_new + 1, max_seq) (the reference's loop emits up to max_new + 1 when
 * max_seq does not bind), sequence feed max_seq.  0 for a config the step entries refuse. */
int32_t fa_aed_max_out(const fa_aed_config *cfg);
/* Bytes of the caller-owned DEVICE buffer holding the state of `batch` utterances (history of consumed tokens, its length, the
 * step, the current input token, the output tokens and their count, the end reason); 0 for a refused config or batch < 1. */
int64_t fa_aed_state_bytes(const fa_aed_config *cfg, int32_t batch);
/* Starts `batch` utterances.  d_prompts DEVICE int32[batch][prompt_stride]; prompt_lens HOST int32[batch], each 1 ... min(prompt_stride,
 * max_seq) (P < 1 is refused; a sequence-feed prompt of max_seq tokens ends at once with FA_AED_END_CAP).  Token feed writes
 * d_input_id[b] = prompt[0], d_position_id[b] = 0 and, with d_self_mask, the static self-attention mask row of step 0
 * ([batch][max_seq], mask_dtype FA_DTYPE_F32 or FA_DTYPE_F16 bits: 0 up to and including the step, -1e4 / 0xF0E2 beyond;
 * buildSelfAttentionMask :817-849 — the dynamic variant is step + 1 zeros, sized by the caller from d_position_id).  Sequence
 * feed writes d_input_ids int32[batch][max_seq] (prompt, then 0) and d_decoder_mask float[batch][max_seq] (1 / 0).  The arrays of
 * the other feed may be NULL.  One synchronisation (the prompt lengths are uploaded). */
fa_status fa_aed_begin_dev(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, const int32_t *d_prompts, int32_t prompt_stride,
                           const int32_t *prompt_lens, void *d_state, int32_t *d_input_id, int32_t *d_position_id, void *d_self_mask,
                           int32_t mask_dtype, int32_t *d_input_ids, float *d_decoder_mask);
/* One decode step for the whole batch: ONE launch, no allocation, no synchronisation.  d_logits [batch] rows of `vocab` logits
 * (fp32 / fp16, widened exactly), row b at element b * row_stride; the row is read once and never written; padding is never read;
 * rows of finished utterances are never read and none of their outputs is touched.
 * Token feed (CoherePipeline.swift:728-803): at step s the history holds the tokens consumed at steps 0 .. s-1 (NOT the current
 * input), the decision is the first-index argmax after applyRepetitionPenalty (:924-935: each distinct in-range history id once,
 * v >= 0 ? v / p : v * p; skipped for p == 1 or an empty history) and then applyNoRepeatNgram (:937-959: n = 1 bans every history
 * id, n >= 2 bans what followed each earlier occurrence of the last n-1 tokens, -1e9 overriding the penalty), the current input
 * is appended to the history AFTER the decision.  For s < P-1 the decision is discarded (the row is not read).  From s >= P-1 EOS
 * ends the utterance (nothing appended), any other token is appended to the output and becomes the next input.  The loop ends after
 * step min(max_new + P, max_seq) - 1 (FA_AED_END_CAP).  An utterance that goes on gets d_input_id, d_position_id and, with
 * d_self_mask, its mask row for the next step.
 * Sequence feed (CanaryManager.swift:212-275): plain argmax with strict '>' from -greatestFiniteMagnitude (an all -inf row yields
 * 0); EOS ends; otherwise the token is appended, d_input_ids[b][pos] = token, d_decoder_mask[b][pos] = 1, ++pos; pos == max_seq
 * ends with FA_AED_END_CAP. */
fa_status fa_aed_step_dev(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, void *d_state, const void *d_logits, int32_t dtype,
                          int64_t row_stride, int32_t *d_input_id, int32_t *d_position_id, void *d_self_mask, int32_t mask_dtype,
                          int32_t *d_input_ids, float *d_decoder_mask);
/* What the state holds now.  tokens int32[batch][max_out] (max_out >= fa_aed_max_out, else OUTPUT_TOO_SMALL; the tail of a row is
 * 0), counts, reasons (FA_AED_*), steps (token feed: the next step; sequence feed: pos) int32[batch]; reasons / steps nullable.
 * _dev: DEVICE outputs, no synchronisation.  Host form: HOST outputs, one synchronisation. */
fa_status fa_aed_finish_dev(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, const void *d_state, int32_t max_out, int32_t *d_tokens,
                            int32_t *d_counts, int32_t *d_reasons, int32_t *d_steps);
fa_status fa_aed_finish(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, const void *d_state, int32_t max_out, int32_t *tokens,
                        int32_t *counts, int32_t *reasons, int32_t *steps);
/* buildCrossAttentionMask (:851-876): d_mask [batch][encoder_seq_len], 0 below valid and -1e4 (fp32) / 0xF0E2 (fp16 bits) from it,
 * d_valid DEVICE int32[batch] clamped to [0, encoder_seq_len]. */
fa_status fa_aed_cross_mask_dev(fa_ctx *ctx, const int32_t *d_valid, int32_t batch, int32_t encoder_seq_len, int32_t mask_dtype, void *d_mask);
/* encoderValidFrames (:670-676): ceil(feature_length * encoder_frames / mel_frames) through fp64, clamped to [1, encoder_seq_len];
 * the reference's frame counts are 3500 and 438.  0 for mel_frames < 1 or a negative argument. */
int32_t fa_aed_encoder_valid_frames(int64_t feature_length, int32_t encoder_seq_len, int32_t mel_frames, int32_t encoder_frames);
/* makeDecoderContext (CanaryManager.swift:187-209): d_enc [batch][D][T] (fp32 / fp16) at element strides (stride_b, stride_d,
 * stride_t; the time stride of a row may be padded, T = 188 in 192) -> d_emb float[batch][T][D] dense and d_mask float[batch][T]:
 * 1.0 below min(max(len, 1), T), else 0.0; d_len DEVICE int32[batch]. */
fa_status fa_aed_encoder_context_dev(fa_ctx *ctx, const void *d_enc, int32_t dtype, int32_t batch, int32_t D, int32_t T, int64_t stride_b,
                                     int64_t stride_d, int64_t stride_t, const int32_t *d_len, float *d_emb, float *d_mask);
/* The hidden-row gather of :251-256: row pos - 1 (pos from the sequence-feed state) of d_dec [batch][S][D] at element strides
 * -> d_hidden float[batch][D]; rows of finished utterances are not touched. */
fa_status fa_aed_gather_hidden_dev(fa_ctx *ctx, const fa_aed_config *cfg, int32_t batch, const void *d_state, const void *d_dec, int32_t dtype,
                                   int32_t S, int32_t D, int64_t stride_b, int64_t stride_s, int64_t stride_d, float *d_hidden);
/* The window loop of transcribeLong (CoherePipeline.swift:525-572, CanaryManager.swift:50-71) for n recordings of `samples` samples:
 * at most one chunk is one window, otherwise windows start every hop and a tail of at most chunk - hop samples after the first
 * window is dropped.  window_range int64[n + 1]; starts / lens int64[capacity] (nullable: count only); *count is always set;
 * OUTPUT_TOO_SMALL when the windows do not fit `capacity`.  No context, no device. */
fa_status fa_aed_plan_windows(const fa_aed_config *cfg, const int64_t *samples, int64_t n, int64_t *window_range, int64_t *starts, int64_t *lens,
                              int64_t capacity, int64_t *count);
/* mergeTokenStreams (CoherePipeline.swift:592-634 = CanaryManager.swift:92-130) folded over each recording's windows, one
 * wavefront per recording.  tokens: flat int32 ids (DEVICE for _dev), window w = [window_offsets[w], window_offsets[w + 1]);
 * recording r owns windows [recording_range[r], recording_range[r + 1]) and the output slice [out_range[r], out_range[r + 1]),
 * which must hold the sum of its windows' tokens (else OUTPUT_TOO_SMALL).  The three offset arrays are HOST int64.  Per seam the
 * longest common substring of the last / first window_tokens tokens (the reference's strict '>' in row-major order: the longest run,
 * then the lowest row, then the lowest column); below min_match a plain concatenation; an empty side returns the other.
 * out_counts HOST int32[n]; seam_best_len / seam_best_send HOST int32[windows] (nullable; 0 where a side was empty).
 * cfg nullable (32, 4).  One synchronisation. */
fa_status fa_aed_merge_windows_dev(fa_ctx *ctx, const fa_aed_config *cfg, const int32_t *d_tokens, const int64_t *window_offsets,
                                   const int64_t *recording_range, int64_t n_recordings, int32_t *d_out, const int64_t *out_range,
                                   int32_t *out_counts, int32_t *seam_best_len, int32_t *seam_best_send);
fa_status fa_aed_merge_windows(fa_ctx *ctx, const fa_aed_config *cfg, const int32_t *tokens, const int64_t *window_offsets,
                               const int64_t *recording_range, int64_t n_recordings, int32_t *out, const int64_t *out_range,
                               int32_t *out_counts, int32_t *seam_best_len, int32_t *seam_best_send);

/* ------------------------------------------------------------------ AHC ------------- */
/* Exact signature + status contract of the reference FFI
 * (FastClusterWrapper/include/FastClusterWrapper.h:35-41, FastClusterWrapper.cpp:196-244):
 * HOST pointers, row-major data, SciPy-format dendrogram rows in merge order.  Declared with
 * the reference's own names in include/FastClusterWrapper.h (included here):
 *   fastcluster_wrapper_status fastcluster_compute_centroid_linkage(const double *data,
 *       size_t pointCount, size_t dimension, double *dendrogramOut, size_t dendrogramLength); */
#include "FastClusterWrapper.h"

typedef struct {
    int64_t merges;        /* N-1 */
    int64_t rounds;        /* select/apply kernel pairs executed */
    int64_t rescans;       /* lazy row re-scans; in a reference-order run through the matrix filter: + the rows whose candidates were too many for
                            * one wavefront and were scanned again with exact sums */
    int64_t exact_fallback;/* 1 if the Lance-Williams filter hit an ambiguity and the run switched to exact rows */
    double init_ms, merge_ms, total_ms; /* device time (hipEvent) */
    int64_t windows;       /* rounds in which several pairs fell inside the rounding bound and were re-evaluated exactly */
    int64_t reference_order; /* 1 if the run met an EXACT tie at the minimum (or was asked to) and was computed in the reference's own
                              * selection order (binary heap + index-ordered scans, fastcluster_internal.hpp:778-935,1625-1800):
                              * row for row the reference's output on tied input; `rounds` then counts its scans */
    int64_t handed_over_at;  /* AUTO's tie route: rows computed in reference order before the rest of the problem went back to the filter-based rounds
                              * (ties at distance 0 only — duplicates — that had stopped); 0: not handed over, -1: handed over, met a tie, recomputed */
} fa_ahc_stats;

enum { FA_AHC_MODE_AUTO = 0,   /* Lance-Williams filter + exact re-verification; an exact tie at the minimum (or a window overflowing
                                * with near-ties) re-runs the problem in reference order: the dendrogram is the reference's row for row */
       FA_AHC_MODE_EXACT = 1,  /* every matrix entry is the reference's sequential fp64 sum; ties in (value, row, column) order */
       FA_AHC_MODE_REFERENCE_ORDER = 2 };/* the reference's selection order from the start (what AUTO falls back to): ~12 us per merge at 43 200 points with the
                                         * distance matrix as the filter of its scans, 25-28 us matrix-free (no N x N workspace to be had, or FA_AHC_RO_NO_MATRIX set) */

/* Same computation with an explicit context; data/dendrogram are HOST pointers unless
 * device_pointers != 0.  stats may be NULL. */
fa_status fa_ahc_linkage(fa_ctx *ctx, const double *data, size_t n, size_t d, double *dendrogram,
                         size_t dendrogram_len, int32_t mode, int32_t device_pointers, fa_ahc_stats *stats);

/* `count` independent problems (one per recording) of dimension d in ONE call: the serial merge chains advance together —
 * one launch is one round of every unfinished problem — so many medium-sized recordings fill the machine that a single chain
 * leaves idle.  data / dendrograms: HOST arrays of `count` pointers (to host buffers, or to device buffers when
 * device_pointers != 0); n: HOST array of row counts; statuses (nullable): per-problem status with the contract of the
 * reference symbol; stats (nullable): `count` entries (init_ms / merge_ms are those of the whole batch).  Returns the
 * first per-problem failure.  Every dendrogram equals the one fa_ahc_linkage produces for that problem alone. */
fa_status fa_ahc_linkage_batch(fa_ctx *ctx, int32_t count, const double *const *data, const size_t *n, size_t d,
                               double *const *dendrograms, int32_t mode, int32_t device_pointers, fa_ahc_stats *stats,
                               int32_t *statuses);

/* Nearest other point of rows [row0, row1) among all n rows of x (n x d, row-major fp64): mins[i - row0] = the reference's
 * distance (sequential sum of squared differences, FastClusterWrapper.cpp:45-52; the SQUARED distance like the linkage uses
 * before its final sqrt), args[i - row0] = its index (lowest on ties).  The start-up table of the linkage
 * (fastcluster_internal.hpp:1653-1678) in a form that shards by rows across GPUs: every rank holds all of x (all-gather),
 * computes its slab, and the (min, arg) pairs are gathered (fluidaudio_amd/sharding.py::row_minima_sharded). */
fa_status fa_ahc_row_minima(fa_ctx *ctx, const double *x, size_t n, size_t d, size_t row0, size_t row1, double *mins, int32_t *args,
                            int32_t device_pointers);

/* AHCClustering.cluster (FluidAudio/Diarizer/Offline/Clustering/AHCClustering.swift:20-67): L2-normalise
 * (:70-105), linkage, threshold clamp (:112-121), top-down cut (:124-197), relabel (:200-210).
 * x: HOST double[n*d]; labels: HOST int32[n].  On linkage failure labels = 0..n-1 (:52-55) and
 * the failing status is returned. */
fa_status fa_ahc_cluster(fa_ctx *ctx, const double *x, size_t n, size_t d, double threshold, int32_t mode,
                         int32_t *labels, fa_ahc_stats *stats);
/* The cut alone (:124-210) on a host dendrogram. */
fa_status fa_ahc_cut(const double *dendrogram, size_t n, double threshold, int32_t *labels);

/* ------------------------------------------------------------------ VBx ------------- */
/* VBxClustering.refine / runVBx (FluidAudio/Diarizer/Offline/Clustering/VBxClustering.swift:41-165,167-664).
 * HOST pointers.  rho: double[T*D]; initial: int32[T] AHC labels; phi: double[D].
 * gamma: double[T*S] out, pi: double[S] out, hard: int32[T] out (argmax, first max :144-146),
 * elbos: double[max_iter] out, n_iters out.  S = number of distinct labels in `initial`
 * (returned through n_speakers; gamma/pi must be sized for it — query with fa_vbx_speaker_count). */
int32_t fa_vbx_speaker_count(const int32_t *initial, int64_t T);
fa_status fa_vbx_refine(fa_ctx *ctx, const double *rho, int64_t T, int32_t D, const int32_t *initial,
                        const double *phi, double Fa, double Fb, int32_t max_iter, double epsilon,
                        double *gamma, double *pi, int32_t *hard, double *elbos, int32_t *n_iters,
                        int32_t *n_speakers);

/* The same iteration loop (VBxClustering.swift:301-661) sharded over the frame axis, one fa_vbx_shard per device.
 * Everything that crosses frames is one record per slice of the frame axis (fa_vbx_shard_slices() = 64 slices of ceil(T / 64) frames:
 * [S][D + 1] doubles = sum_t gamma[t][s] (rho[t][:], 1), then the slice's sum of the per-frame log-likelihoods); a device holds
 * 64 / world consecutive slices = the frames fa_vbx_shard_range() names (world must divide 64).  Protocol, identical on every rank:
 *     begin(chunk)  ->  all-gather the chunks in rank order into `full`
 *     repeat up to max_iter times { iterate(full, chunk) -> all-gather -> finish_iteration(full, &elbo); stop when |elbo - previous| < epsilon (:653-659) }
 *     result(...)
 * Every rank evaluates speaker statistics, pi and the ELBO from the same gathered records: same decisions everywhere, no other
 * collective.  The records of a slice are computed exactly as fa_vbx_refine computes them on one device, so the sharded run equals
 * fa_vbx_refine bit for bit at every world size.  rho_local / labels_local: HOST, the frames of fa_vbx_shard_range(); phi HOST [D];
 * chunk / full: DEVICE double[fa_vbx_shard_chunk_doubles(S, D, world)] / [... (S, D, 1)] (the caller's collective library moves them;
 * both calls that write a chunk return with it complete); S = number of distinct labels of the WHOLE problem. */
typedef struct fa_vbx_shard fa_vbx_shard;
int32_t fa_vbx_shard_slices(void);
void fa_vbx_shard_range(int64_t T_total, int32_t rank, int32_t world, int64_t *t_lo, int64_t *t_hi);
int64_t fa_vbx_shard_chunk_doubles(int32_t S, int32_t D, int32_t world);
fa_status fa_vbx_shard_create(fa_ctx *ctx, const double *rho_local, int64_t T_total, int32_t D, const int32_t *labels_local, int32_t S,
                              const double *phi, double Fa, double Fb, int32_t rank, int32_t world, fa_vbx_shard **out);
void fa_vbx_shard_destroy(fa_vbx_shard *shard);
void fa_vbx_shard_frames(const fa_vbx_shard *shard, int64_t *t_lo, int64_t *t_hi);
fa_status fa_vbx_shard_begin(fa_vbx_shard *shard, double *d_chunk);
fa_status fa_vbx_shard_iterate(fa_vbx_shard *shard, const double *d_full, double *d_chunk);
fa_status fa_vbx_shard_finish_iteration(fa_vbx_shard *shard, const double *d_full, double *elbo);
/* HOST outputs (each may be NULL): gamma_local double[frames held * S], pi double[S], hard_local int32[frames held]. */
fa_status fa_vbx_shard_result(fa_vbx_shard *shard, double *gamma_local, double *pi, int32_t *hard_local);

/* ------------------------------------------------------------------ post-VBx -------- */
/* OfflineDiarizerManager.computeCentroids (FluidAudio/Diarizer/Offline/Core/OfflineDiarizerManager.swift:613-691) and
 * assignEmbeddings (:789-822).  HOST pointers, fp64.
 * emb: double[n*d]; gamma: double[n*S]; pi: double[S].  Speakers with pi > 1e-7 are kept: map[s] = row of `centroids`
 * (or -1), *n_centroids = number kept; centroids must hold S*d doubles.  Summation order = the reference's. */
fa_status fa_vbx_weighted_centroids(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, const double *gamma,
                                    const double *pi, int32_t S, double *centroids, int32_t *map, int32_t *n_centroids);
/* out[i] = argmax_k cosine(emb_i, centroid_k), first maximum; K == 0 -> all 0 (:795-797). */
fa_status fa_assign_cosine(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, const double *centroids, int32_t K,
                           int32_t *out);
/* centroidScores (:789-798): scores[i*K + k] = cosine(emb_i, centroid_k). */
fa_status fa_centroid_scores(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, const double *centroids, int32_t K,
                             double *scores);
/* ConstrainedClusterAssignment.assign (FluidAudio/Diarizer/Offline/Clustering/ConstrainedClusterAssignment.swift:20-42):
 * per chunk, HungarianAssignment.maxScoreAssignment (FluidAudio/Diarizer/HungarianAssignment.swift:67-97) — distinct
 * local speakers of a chunk get distinct clusters, maximising the total score; -2 = slot dropped (more speakers than
 * clusters).  scores: double[n*K]; chunk_indices: int32[n]; out: int32[n].  At most 256 rows per chunk / clusters. */
fa_status fa_constrained_assign(fa_ctx *ctx, const double *scores, int64_t n, int32_t K, const int32_t *chunk_indices,
                                int32_t *out);

/* ------------------------------------------------------------------ the clustering stage, composed ---- */
/* OfflineDiarizerManager.cluster (FluidAudio/Diarizer/Offline/Core/OfflineDiarizerManager.swift:270-375) on precomputed
 * embeddings as ONE call whose intermediates never leave HBM: selectTrainingEmbeddings (:591-611) -> AHCClustering.cluster
 * (:301-306) -> VBxClustering.refineWithConstraints (:308-333) -> computeCentroids / computeCentroidsFromClusters (:613-740)
 * -> constrained per-chunk assignment or cosine argmax of every embedding (:345-375, :789-822).  Config defaults =
 * OfflineDiarizerTypes.swift:155-163,189-192. */
typedef struct {
    double clustering_threshold;     /* 0.6 */
    double warm_start_fa;            /* 0.07 */
    double warm_start_fb;            /* 0.8 */
    int32_t max_vbx_iterations;      /* 20 */
    double convergence_tolerance;    /* 1e-4 */
    int32_t constrained_assignment;  /* 1 */
    int64_t num_speakers;            /* -1 = nil */
    int64_t min_speakers;            /* -1 = nil */
    int64_t max_speakers;            /* -1 = nil */
    int32_t ahc_mode;                /* FA_AHC_MODE_AUTO */
} fa_offline_cluster_config;
typedef struct {
    int64_t training_rows;           /* rows that passed selectTrainingEmbeddings */
    int32_t initial_clusters;        /* distinct AHC labels */
    int32_t vbx_iterations;
    int32_t was_adjusted;            /* the K-Means fallback replaced the VBx posteriors (VBxOutput.wasAdjusted) */
    int32_t constrained;             /* the constrained per-chunk assignment was used */
    int32_t vbx_degraded;            /* VBx failed: gamma = one-hot AHC labels, pi = 1/S, no ELBOs, the stage went on (VBxClustering.swift:136-141) */
    int32_t ahc_degraded;            /* the linkage failed: every training row its own cluster (AHCClustering.swift:52-55) */
    double inputs_s, ahc_s, vbx_s, assign_s, total_s;   /* host wall-clock per stage (copies included) */
    fa_ahc_stats ahc;
} fa_offline_cluster_info;
void fa_offline_cluster_default_config(fa_offline_cluster_config *cfg);
/* embeddings: float[n*d] (the 256-d speaker embeddings, widened to fp64 on the device like :286); rho: double[n*rho_dim]
 * PLDA features (rho_dim == 0: no VBx, centroids come from the AHC labels); chunk_indices: HOST int32[n] (needed when
 * constrained_assignment != 0); phi: HOST double[rho_dim].  embeddings / rho are HOST pointers unless device_pointers != 0.
 * labels: HOST int32[n] out (-2 = slot dropped by the constrained assignment); centroids: HOST double[max_centroids*d] out or
 * NULL; *n_centroids out; info may be NULL.  n == 0 -> INVALID_ARGUMENT (the reference throws noSpeechDetected, :281-283).
 * STREAM CONTRACT of device_pointers != 0: the stage reads embeddings / rho on the context's stream, and all it waits for is that stream.
 * The inputs must therefore be complete on, or ordered before, the context's stream when the call is made: produced on that stream,
 * or on another one that the caller has synchronised or made the context's stream wait for (an event recorded behind the producer and
 * hipStreamWaitEvent on fa_ctx_stream(ctx)).  The context's stream is non-blocking: nothing orders it against another stream by itself. */
fa_status fa_offline_cluster(fa_ctx *ctx, const float *embeddings, int64_t n, int32_t d, const double *rho, int32_t rho_dim,
                             const int32_t *chunk_indices, const double *phi, const fa_offline_cluster_config *config,
                             int32_t device_pointers, int32_t *labels, double *centroids, int32_t max_centroids,
                             int32_t *n_centroids, fa_offline_cluster_info *info);
/* The same call with copies of the stage's intermediates (verification at full size: bench.py and the 8 h digest test compare them
 * with the CPU side): ahc_labels HOST int32[training rows] = AHCClustering.cluster's labels (AHCClustering.swift:20-67), vbx_hard
 * HOST int32[training rows] = argmax of the VBx posteriors (VBxClustering.swift:144-146), elbos HOST double[max_vbx_iterations]
 * (info->vbx_iterations of them are written).  Each may be NULL.  device_pointers != 0: fa_offline_cluster's stream contract. */
fa_status fa_offline_cluster_ex(fa_ctx *ctx, const float *embeddings, int64_t n, int32_t d, const double *rho, int32_t rho_dim,
                                const int32_t *chunk_indices, const double *phi, const fa_offline_cluster_config *config,
                                int32_t device_pointers, int32_t *labels, double *centroids, int32_t max_centroids,
                                int32_t *n_centroids, fa_offline_cluster_info *info, int32_t *ahc_labels, int32_t *vbx_hard,
                                double *elbos);
/* `count` recordings through the same stage in ONE call: inputs and training rows of every recording are prepared, the merge
 * chains of all of them advance together (fa_ahc_linkage_batch's round launches: a single chain leaves most of the machine
 * idle), then every recording is cut / refined / assigned.  HOST pointers; all recordings share d, rho_dim, phi and config.
 * embeddings / rho / chunk_indices / labels / centroids: arrays of `count` pointers (rho and centroids may be NULL as in the
 * single call); n, n_centroids, infos (nullable), statuses (nullable): `count` entries.  Per recording the results equal
 * fa_offline_cluster's bit for bit; a failing recording does not stop the others; the first failure is returned.
 * infos[r].*_s of a batch are wall-clock marks of the shared phases, not per-recording costs. */
fa_status fa_offline_cluster_batch(fa_ctx *ctx, int32_t count, const float *const *embeddings, const int64_t *n, int32_t d,
                                   const double *const *rho, int32_t rho_dim, const int32_t *const *chunk_indices, const double *phi,
                                   const fa_offline_cluster_config *config, int32_t *const *labels, double *const *centroids,
                                   int32_t max_centroids, int32_t *n_centroids, fa_offline_cluster_info *infos, int32_t *statuses);
/* The same with the recordings' inputs RESIDENT on the context's device (what device_pointers = 1 is to fa_offline_cluster): d_embeddings[r] /
 * d_rho[r] are DEVICE pointers (the arrays of pointers themselves, n, chunk_indices[r], phi, labels[r], centroids[r] stay on the host).  The call
 * waits for the context's stream first (the inputs' producer), nothing is uploaded.  Results equal fa_offline_cluster_batch's bit for bit.
 * fa_offline_cluster's stream contract holds for every d_embeddings[r] / d_rho[r]: complete on, or ordered before, the context's stream. */
fa_status fa_offline_cluster_batch_dev(fa_ctx *ctx, int32_t count, const float *const *d_embeddings, const int64_t *n, int32_t d,
                                       const double *const *d_rho, int32_t rho_dim, const int32_t *const *chunk_indices, const double *phi,
                                       const fa_offline_cluster_config *config, int32_t *const *labels, double *const *centroids,
                                       int32_t max_centroids, int32_t *n_centroids, fa_offline_cluster_info *infos, int32_t *statuses);


/* ------------------------------------------------ speaker-count constraints + K-Means fallback ------ */
/* KMeansClustering.SeededRNG.next (FluidAudio/Diarizer/Offline/Clustering/KMeansClustering.swift:212-223) and the Swift
 * standard library's RandomNumberGenerator.next(upperBound:) over it (Lemire's method; the draw behind shuffle(using:) and
 * randomElement(using:)).  Pure host functions. */
uint64_t fa_seeded_rng_next(uint64_t *state);
uint64_t fa_seeded_rng_below(uint64_t *state, uint64_t upper_bound);
/* KMeansClustering.clusterWithCentroids (:39-91): unit-normalise, centroids = first k of a seeded shuffle, Lloyd iterations
 * until the assignment repeats or max_iterations; empty clusters re-seeded from a random embedding.  HOST pointers:
 * emb double[n*d] -> labels int32[n], centroids double[min(k,n)*d] (nullable), *out_k = centroid rows written (0 for the
 * degenerate returns: d == 0 or num_clusters <= 0 -> all labels 0; n <= k -> labels 0..n-1 and the raw embeddings). */
fa_status fa_kmeans_cluster(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, int32_t num_clusters, int32_t max_iterations,
                            uint64_t seed, int32_t *labels, double *centroids, int32_t *out_k, int32_t *out_iterations);
/* KMeansClustering.clusterWithCentroidsNInit (:99-129): seeds base_seed + 0..n_init-1, lowest inertia wins (first on ties).
 * All runs advance together on the device.  best_run / inertias[n_init] nullable. */
fa_status fa_kmeans_cluster_ninit(fa_ctx *ctx, const double *emb, int64_t n, int32_t d, int32_t num_clusters, int32_t max_iterations,
                                  int32_t n_init, uint64_t base_seed, int32_t *labels, double *centroids, int32_t *out_k,
                                  int32_t *best_run, double *inertias);
/* SpeakerCountConstraints.resolve (FluidAudio/Diarizer/Offline/Clustering/SpeakerCountConstraints.swift:25-62).  A null
 * pointer is Swift's nil.  out = { numSpeakers or -1 for nil, minSpeakers, maxSpeakers }. */
void fa_speaker_constraints_resolve(int64_t num_embeddings, const int64_t *num_speakers, const int64_t *min_speakers,
                                    const int64_t *max_speakers, int64_t out[3]);

/* ------------------------------------------------------------------ CTC beam search + ARPA LM ------ */
/* ARPALanguageModel (FluidAudio/ASR/Parakeet/SlidingWindow/CTC/ARPALanguageModel.swift:16-104): unigrams and bigrams of a
 * plain-text ARPA file (tab-separated fields, log10 -> natural log in float); higher orders ignored, malformed lines
 * skipped.  Words are keyed by a 64-bit polynomial hash of their bytes plus their length.  Parsing and fa_arpa_score are
 * host code (ctx may be NULL); the tables move to the device on the first search. */
typedef struct fa_arpa_lm fa_arpa_lm;
fa_status fa_arpa_parse(fa_ctx *ctx, const char *text, int64_t len, fa_arpa_lm **out);
void fa_arpa_destroy(fa_arpa_lm *lm);
int64_t fa_arpa_unigram_count(const fa_arpa_lm *lm);          /* lm.unigrams.count */
int64_t fa_arpa_bigram_context_count(const fa_arpa_lm *lm);   /* lm.bigrams.count (context words) */
/* ARPALanguageModel.score(word:prev:) (:98-103); prev may be NULL (nil).  Pure host function on the same tables. */
fa_status fa_arpa_score(const fa_arpa_lm *lm, const char *word, const char *prev, float *out);

/* The token vocabulary ([Int: String]) as the device needs it for word tracking: SentencePiece word-boundary flag and the
 * hash pair of the piece.  ids[i] -> pieces[i] (UTF-8); ids not listed decode to "". */
typedef struct fa_ctc_vocab fa_ctc_vocab;
fa_status fa_ctc_vocab_create(fa_ctx *ctx, const int32_t *ids, const char *const *pieces, int32_t n, int32_t vocab_size,
                              fa_ctc_vocab **out);
void fa_ctc_vocab_destroy(fa_ctc_vocab *vocab);

/* ctcBeamSearch (FluidAudio/ASR/Parakeet/SlidingWindow/CTC/CtcDecoder.swift:118-241) for a batch of [frames, vocab] float
 * log-probability matrices: one workgroup per utterance.  lm / vocabulary may be NULL (no rescoring).  beam_width <= 128,
 * token_candidates <= 64.  tokens: int32[batch][frames] (best prefix, lens[b] entries used), scores: total of the winner
 * (nullable).  The string form is decodeCtcTokenIds over tokens.  DEVICE pointers, synchronous. */
fa_status fa_ctc_beam_search_batch_dev(fa_ctx *ctx, const float *d_log_probs, int32_t batch, int32_t frames, int32_t vocab,
                                       int64_t row_stride, int64_t matrix_stride, const int32_t *d_valid_frames,
                                       const fa_ctc_vocab *vocabulary, fa_arpa_lm *lm, int32_t beam_width, float lm_weight,
                                       float word_bonus, int32_t blank_id, int32_t token_candidates, int32_t *d_tokens,
                                       int32_t *d_lens, float *d_scores);
/* Same with HOST pointers and contiguous matrices. */
/* What a search of these shapes launches: out = { trie slots per utterance, utterances per launch (the ~2 GiB arena cap), launches,
 * extension keys per thread of the ctc_beam_kernel instance (8 / 20 / 32) }.  Host only. */
fa_status fa_ctc_beam_plan(int32_t batch, int32_t frames, int32_t vocab, int32_t beam_width, int32_t blank_id, int32_t token_candidates,
                           int64_t out[4]);
fa_status fa_ctc_beam_search_batch(fa_ctx *ctx, const float *log_probs, int32_t batch, int32_t frames, int32_t vocab,
                                   const int32_t *valid_frames, const fa_ctc_vocab *vocabulary, fa_arpa_lm *lm,
                                   int32_t beam_width, float lm_weight, float word_bonus, int32_t blank_id,
                                   int32_t token_candidates, int32_t *tokens, int32_t *lens, float *scores);

/* ------------------------------------------------------------------ wire formats ------ */
/* AudioWAV.data (FluidAudio/Shared/AudioConverter.swift:474-532): float samples -> peak normalisation (normalize != 0 and
 * max |x| > 0) -> clamp to [-1, 1] -> Int16(x * 32767) -> 16-bit PCM mono RIFF/WAVE (44-byte header + 2 n bytes).  HOST
 * pointers; the sample pass runs on the device and is bit-identical to the reference's Float arithmetic. */
int64_t fa_wav_pcm16_size(int64_t n_samples);
fa_status fa_wav_encode_pcm16(fa_ctx *ctx, const float *samples, int64_t n, double sample_rate, int32_t normalize, uint8_t *out,
                              int64_t out_capacity, int64_t *out_len);
/* Extension (the reference reads audio through AVFoundation): RIFF/WAVE reader for 16-bit PCM and 32-bit float data,
 * interleaved float output; out may be NULL to query frames / channels / sample_rate.  Pure host function. */
fa_status fa_wav_decode(const uint8_t *data, int64_t len, float *out, int64_t out_capacity, int64_t *frames, int32_t *channels,
                        int32_t *sample_rate);

typedef struct fa_rttm_segment {   /* TimedSpeakerSegment as the RTTM loaders fill it */
    float start_seconds, end_seconds, quality;
    char speaker_id[64];
} fa_rttm_segment;
/* RTTMParser.loadSegments (FluidAudioCLI/Utils/RTTMParser.swift:22-63; strict = 1: blank and '#' lines skipped, any other
 * malformed line is an error reported in bad_line, result sorted by start time) or the benchmark loader
 * (FluidAudioCLI/Commands/SortformerBenchmark.swift:681-731; strict = 0: malformed lines skipped, file order kept).
 * Pure host function; *count receives the number of segments even when out is NULL / too small. */
fa_status fa_rttm_parse(const char *text, int64_t len, int32_t strict, fa_rttm_segment *out, int64_t out_capacity, int64_t *count,
                        char *bad_line, int64_t bad_line_capacity);
/* Extension: one "SPEAKER <file> 1 <start> <duration> <NA> <NA> <speaker> <NA> <NA>" line per segment; returns the text
 * length and writes it (NUL-terminated) when out_capacity is larger; -1 when the text could not be built (host allocation failed). */
int64_t fa_rttm_format(const fa_rttm_segment *segs, int64_t n, const char *file_id, char *out, int64_t out_capacity);

typedef struct fa_export_embedding {   /* TimedEmbedding fields of the export payload */
    int32_t chunk_index, speaker_index, start_frame, end_frame;
    double start_time, end_time;
} fa_export_embedding;
/* OfflineDiarizerManager.exportEmbeddings (FluidAudio/Diarizer/Offline/Core/OfflineDiarizerManager.swift:913-955): JSON
 * array of {chunkIndex, speakerIndex, startFrame, endFrame, startTime, endTime, embedding256, rho128, cluster}; cluster = -1
 * past the end of assignments.  Numbers are printed in their shortest round-trip form.  Returns the text length (-1: host allocation failed). */
int64_t fa_export_embeddings_json(const fa_export_embedding *items, int64_t n, const float *embedding256, int32_t emb_dim,
                                  const double *rho128, int32_t rho_dim, const int32_t *assignments, int64_t n_assignments,
                                  char *out, int64_t out_capacity);

/* ------------------------------------------------------------------ speaker segments ------ */
/* The powerset decode of OfflineSegmentationProcessor (FluidAudio/Diarizer/Offline/Segmentation/OfflineSegmentationProcessor.swift:316-409):
 * logits float[chunks][frames][classes] -> weights float[chunks][frames][3], 1.0 for each local speaker of powerset[min(argmax, 7)]
 * (table :15-24: [] [0] [1] [2] [0,1] [0,2] [1,2] [0,1,2]) and 0 otherwise, bit-exact; the argmax is the first strict maximum
 * seeded at -FLT_MAX (NaN never wins, an all-NaN / all--inf row is class 0).  log_probs float[chunks][frames][classes] (nullable)
 * = logits - logSumExp(logits) in fp32 (VDSPOperations.swift:142-155; informational, the reference's vvexpf is closed source).
 * _dev: DEVICE pointers, enqueued on the context's stream (no synchronisation); otherwise HOST pointers. */
fa_status fa_powerset_decode_dev(fa_ctx *ctx, const float *d_logits, int64_t chunks, int32_t frames, int32_t classes, float *d_weights,
                                 float *d_log_probs);
fa_status fa_powerset_decode(fa_ctx *ctx, const float *logits, int64_t chunks, int32_t frames, int32_t classes, float *weights,
                             float *log_probs);
/* OfflineDiarizerManager.buildChunkAssignments (FluidAudio/Diarizer/Offline/Core/OfflineDiarizerManager.swift:885-911): hard
 * int32[chunks][speakers] = -2, then for every embedding i in order hard[chunk_indices[i]][speaker_indices[i]] = labels[i] when the
 * chunk, the speaker and the label (< cluster_count) are in range; a later embedding overwrites an earlier one.  Pure host function. */
fa_status fa_offline_chunk_assignments(int64_t n, const int32_t *chunk_indices, const int32_t *speaker_indices, const int32_t *labels,
                                       int32_t cluster_count, int32_t chunks, int32_t speakers, int32_t *hard);
/* OfflineReconstruction (FluidAudio/Diarizer/Offline/Utils/OfflineReconstruction.swift:24-237, 359-496).  Defaults =
 * OfflineDiarizerTypes.swift:46-55, 97-103, 204-214, 232-247. */
typedef struct {
    double window_duration;          /* 10.0: start of a chunk without an offset = index * window_duration (:498-507) */
    double frame_duration;           /* 0 = window_duration / frames (OfflineSegmentationProcessor.swift:286) */
    double min_duration_on;          /* 0 (segmentation.minDurationOn) */
    double min_duration_off;         /* 0 (segmentation.minDurationOff) */
    double min_segment_duration;     /* 1.0 */
    double min_gap_duration;         /* 0.1 */
    int32_t exclusive;               /* 1: excludeOverlaps (:359-398) */
    int32_t zero_vote_enabled;       /* 0: the zero-vote re-embed pass (host side: the caller embeds the runs, see overrides) */
    double zero_vote_min_duration;   /* 0.4 */
} fa_reconstruct_config;
void fa_reconstruct_default_config(fa_reconstruct_config *cfg);
typedef struct {
    /* out */
    int64_t total_frames;            /* global frames (:37-47) */
    int64_t raw_segments;            /* segments before merge / sanitize */
    double frame_duration;           /* the frame duration used */
    int64_t zero_vote_run_count;     /* runs found (when zero_vote_runs is set), also those that did not fit */
    /* in: optional HOST buffers the call fills (NULL: not wanted) */
    int64_t *zero_vote_runs;         /* int64[2 * zero_vote_capacity]: [first, end) frames of each zero-vote run of at least
                                        cfg->zero_vote_min_duration (ZeroVoteReembedder.detectRuns, ZeroVoteReembedder.swift:42-79) */
    int64_t zero_vote_capacity;
    int32_t *speaker_counts;         /* int32[speaker_counts_capacity]: speakerCountPerFrame (:145-156), written when it holds total_frames */
    int64_t speaker_counts_capacity;
    /* the per-frame decision in fp64 (verification of the summation order), written when frame_capacity >= total_frames; each may be NULL */
    int64_t frame_capacity;
    int32_t *frame_clusters;         /* int32[frame_capacity * slots]: each frame's active clusters by rank (overrides applied), -1 past them */
    double *frame_averages;          /* double[frame_capacity * slots]: their activation averages sum / count (:107-143), 0 past them */
    double *expected_count_sums;     /* double[frame_capacity]: the fp64 sum of expectedCount over the frame's chunk frames (:90-94) */
    int32_t frame_slots;             /* out: slots = max(min(max(clusters, 1), speakers), 1) */
} fa_reconstruct_info;
/* buildSegments -> mergeSegments -> sanitize on the device (the merge / sanitize pass over the raw segments is host code in the same call).
 * weights float[chunks][frames][speakers] per-speaker activity (fa_powerset_decode's output, or any finite values: a non-finite one is
 * INVALID_ARGUMENT, the reference traps); offsets double[n_offsets] chunk start times in seconds (chunks past n_offsets start at
 * index * window_duration); hard int32[chunks][speakers] cluster per local speaker (fa_offline_chunk_assignments; values outside
 * [0, max(clusters, 1)) count as none; NULL: none); clusters = centroids.count.  overrides int64[n_overrides][3] = (first frame, end
 * frame, cluster): those frames' clusters become [cluster], applied in order (the zero-vote re-embed assignments, :249-298).
 * out: fa_rttm_segment[capacity], speaker_id "S<k+1>"; *count is set even when out is NULL (SUCCESS) or too small (OUTPUT_TOO_SMALL).
 * Raw segments that close at the same frame are taken in increasing cluster index (the reference uses Dictionary order, which is
 * hash-seeded); a segment open after the last frame closes at frame total_frames.  Empty input (chunks or frames 0, frame
 * duration <= 0) -> 0 segments.  weights: HOST pointer; _dev: DEVICE pointer on the context's device, read in stream order.
 * The other pointers are HOST pointers; the call is synchronous. */
fa_status fa_offline_reconstruct(fa_ctx *ctx, const fa_reconstruct_config *cfg, const float *weights, int64_t chunks, int32_t frames,
                                 int32_t speakers, const double *offsets, int64_t n_offsets, const int32_t *hard, int32_t clusters,
                                 const int64_t *overrides, int64_t n_overrides, fa_rttm_segment *out, int64_t capacity, int64_t *count,
                                 fa_reconstruct_info *info);
fa_status fa_offline_reconstruct_dev(fa_ctx *ctx, const fa_reconstruct_config *cfg, const float *d_weights, int64_t chunks, int32_t frames,
                                     int32_t speakers, const double *offsets, int64_t n_offsets, const int32_t *hard, int32_t clusters,
                                     const int64_t *overrides, int64_t n_overrides, fa_rttm_segment *out, int64_t capacity,
                                     int64_t *count, fa_reconstruct_info *info);
/* mergeSegments (:431-463; same speaker and start - previous end <= max(min_gap_duration, min_duration_off), quality blended by
 * duration) -> sanitize (:481-496; drop shorter than max(min_segment_duration, min_duration_on), then excludeOverlaps when exclusive)
 * over raw segments in their raw order.  Pure host function; *count as fa_offline_reconstruct's. */
fa_status fa_segments_finalize(const fa_reconstruct_config *cfg, const fa_rttm_segment *raw, int64_t n, fa_rttm_segment *out,
                               int64_t capacity, int64_t *count);

/* ------------------------------------------------------------------ embedding inputs ------ */
/* OfflineEmbeddingExtractor.extractEmbeddings (FluidAudio/Diarizer/Offline/Extraction/OfflineEmbeddingExtractor.swift:177-711) up to the
 * networks: which (chunk, local speaker) pairs get an embedding, each one's mask resampled to the embedding model's weight length
 * (WeightInterpolation.swift:19-116), the fbank windows, and the TimedEmbedding metadata.  The networks (fbank, embedding, PLDA) are the
 * caller's.  Defaults = OfflineDiarizerTypes.swift:46-55, 82-105, 297-303, 348-353. */
typedef struct {
    double window_duration;          /* 10.0: offset of a chunk without a finite offset = index * window_duration (:197-202, :658-661) */
    int32_t sample_rate;             /* 16000 */
    int32_t samples_per_window;      /* 0 = Int(sample_rate * window_duration) */
    float overlap_threshold;         /* 1e-3: a speaker is active in a frame above this (:303) */
    int32_t exclude_overlap;         /* 1: the clean mask zeroes frames with more than one active speaker */
    double min_segment_duration;     /* 1.0: minFrames = max(1, ceil(min_segment_duration / frame_duration)) */
    int32_t batch_size;              /* 32: fbank batches of clamp(batch_size, 1, 32) planned chunks (:162) */
    int32_t skip_enabled;            /* 0: EmbeddingSkipStrategy.none; 1: maskSimilarity(skip_threshold) */
    float skip_threshold;            /* 0.95 */
    int32_t weight_frames;           /* 589: the embedding model's weight length */
    double frame_duration;           /* 0 = window_duration / frames */
} fa_embedding_config;
void fa_embedding_default_config(fa_embedding_config *cfg);
typedef struct {
    int64_t planned_chunks;          /* chunks whose window holds audio: the fbank windows */
    int64_t batches;                 /* fbank batches */
    int64_t jobs;                    /* valid masks = embeddings (records) */
    int64_t runs;                    /* embedding-model runs (jobs - skipped) */
    int64_t evaluated_masks;         /* the reference's counters (:713-735) */
    int64_t empty_masks;
    int64_t fallback_masks;          /* base mask used because the clean one was shorter than minFrames (also counted when then empty) */
    int64_t skipped_embeddings;
    double frame_duration;           /* the frame duration used */
    int32_t min_frames;
    int32_t samples_per_window;
    int32_t batch_size;              /* the clamped batch size */
} fa_embedding_info;
/* weights float[chunks][frames][speakers] (fa_powerset_decode's output or soft weights); offsets double[n_offsets] chunk starts in seconds;
 * total_samples = the audio's length.  A chunk is planned when start = clamp(round-half-away(offset * rate), 0, total) < min(start +
 * samples_per_window, total).  Per planned chunk and speaker (in this order): baseSum <= 0, cleanSum < Float(frames) * 0.2 and a zero
 * sum of the resampled mask make the mask empty; cleanSum >= Float(minFrames) picks the clean mask, otherwise the base one.  Every sum and
 * dot product is sequential in frame order in fp32 (exact, hence the reference's bits, for 0/1 weights; pinned to the restatement for soft
 * weights).  Departure: a non-finite weight in a planned chunk is INVALID_ARGUMENT (the reference would feed NaN to the model).
 * Outputs, capacity chunks * speakers rows each, in the reference's order (chunk-major, speaker-minor):
 *   records       HOST fa_export_embedding[jobs]: chunk, speaker, first / last active frame, start / end time (fp64, no FMA)
 *   run_of_job    HOST int32[jobs]: the model run whose embedding the job carries (its own, or a cached one under maskSimilarity)
 *   window_of_run HOST int32[runs]: the planned window (index into window_start) each run's fbank input comes from
 *   window_start  HOST int64[planned_chunks] (nullable): first sample of each planned window; window_chunk HOST int32[...] (nullable): its chunk
 *   run_weights   float[runs][weight_frames]: the model's weights input; mask_rows (nullable) float[jobs][frames]: the chosen masks
 *                 before resampling (TimedEmbedding.frameWeights)
 * _dev: weights, run_weights and mask_rows are DEVICE pointers on the context's device, read / written in stream order; otherwise HOST
 * pointers.  Both calls are synchronous for the counts in info. */
fa_status fa_embedding_plan(fa_ctx *ctx, const fa_embedding_config *cfg, const float *weights, int64_t chunks, int32_t frames, int32_t speakers,
                            const double *offsets, int64_t n_offsets, int64_t total_samples, fa_export_embedding *records, int32_t *run_of_job,
                            int32_t *window_of_run, int64_t *window_start, int32_t *window_chunk, float *run_weights, float *mask_rows,
                            fa_embedding_info *info);
fa_status fa_embedding_plan_dev(fa_ctx *ctx, const fa_embedding_config *cfg, const float *d_weights, int64_t chunks, int32_t frames,
                                int32_t speakers, const double *offsets, int64_t n_offsets, int64_t total_samples, fa_export_embedding *records,
                                int32_t *run_of_job, int32_t *window_of_run, int64_t *window_start, int32_t *window_chunk, float *d_run_weights,
                                float *d_mask_rows, fa_embedding_info *info);
/* The fbank windows of `count` planned windows (a range of window_start, HOST int64[count]): d_out float[count][samples_per_window] =
 * audio[start : min(start + samples_per_window, total_samples)] followed by zeros (:807-832, AudioSampleSource.swift:23-39).  d_audio,
 * d_out: DEVICE pointers.  Synchronous (the host starts are staged in the call). */
fa_status fa_embedding_windows_dev(fa_ctx *ctx, const float *d_audio, int64_t total_samples, const int64_t *window_start, int64_t count,
                                   int32_t samples_per_window, float *d_out);
/* embedSpan's inputs (:243-297) for n spans double[n][2] (start, end seconds, HOST): startSample = max(0, round(start * rate)), endSample
 * = min(total, round(end * rate)), len = min(endSample - startSample, samples_per_window); windows float[n][samples_per_window] = the span's
 * samples then zeros, weights float[n][weight_frames] = 1 for the first max(1, min(W, round(len / samples_per_window * W))) frames.
 * statuses HOST fa_status[n]: INVALID_ARGUMENT for an empty or non-finite span (its rows are zeros).  _dev: audio, windows, weights are
 * DEVICE pointers; otherwise HOST pointers.  Synchronous. */
fa_status fa_embedding_span_inputs(fa_ctx *ctx, const fa_embedding_config *cfg, const float *audio, int64_t total_samples, const double *spans,
                                   int64_t n, float *windows, float *weights, fa_status *statuses);
fa_status fa_embedding_span_inputs_dev(fa_ctx *ctx, const fa_embedding_config *cfg, const float *d_audio, int64_t total_samples,
                                       const double *spans, int64_t n, float *d_windows, float *d_weights, fa_status *statuses);
/* WeightInterpolation.resample2D (:19-116): rows float[rows][in_frames] -> float[rows][out_frames], bit-exact (identity when the lengths
 * agree; nothing is written when a length is 0).  _dev: DEVICE pointers, enqueued on the context's stream; otherwise HOST pointers. */
fa_status fa_weight_resample(fa_ctx *ctx, const float *in, int64_t rows, int32_t in_frames, int32_t out_frames, float *out);
fa_status fa_weight_resample_dev(fa_ctx *ctx, const float *d_in, int64_t rows, int32_t in_frames, int32_t out_frames, float *d_out);

/* ------------------------------------------------------------------ offline Sortformer ------ */
/* OfflineSortformerDiarizer.processComplete (FluidAudio/Diarizer/Sortformer/Offline/OfflineSortformerDiarizer.swift:279-375) around its
 * network: window geometry, the model's inputs, and the stitching of the windows' speaker columns into one global timeline
 * (SortformerSpeakerStitcher.swift:27-77).  The network is the caller's; it runs between pack and stitch.  Defaults = :14-43. */
typedef struct {
    int32_t window_output_frames;    /* 384 */
    int32_t subsampling;             /* 8 mel frames per output frame */
    int32_t speakers;                /* 4 */
    int32_t n_mels;                  /* 128 */
    int32_t overlap_output_frames;   /* 100; used as max(0, min(overlap, window - 1)) (:303) */
} fa_sortformer_offline_config;
void fa_sortformer_offline_default_config(fa_sortformer_offline_config *cfg);
typedef struct {
    int32_t recording;               /* index into the batch */
    int32_t valid_mel;               /* mel frames of the window that hold data (the model's mel_length) */
    int32_t valid_out;               /* min(window, ceil(valid_mel / subsampling)) */
    int32_t first;                   /* 1 for a recording's first window */
    int64_t mel_start;               /* first mel frame */
    int64_t g_start;                 /* first output frame on the recording's timeline: mel_start / subsampling */
} fa_sortformer_window;
/* The loop of :303-363 for `batch` recordings of n_mel_frames[b] mel frames: windows start every (window - overlap) * subsampling mel
 * frames while the start lies inside the recording, and the first window shorter than window * subsampling is the last (a recording
 * whose last full window ends exactly at its tail gets one more, short, window inside it).  total_out[batch] (nullable) =
 * ceil(n_mel_frames / subsampling); window_range[batch + 1] (nullable) = the first window of each recording, then the count.
 * windows[capacity] in recording order; *count is set even when windows is NULL (SUCCESS) or too small (OUTPUT_TOO_SMALL).
 * Pure host function. */
fa_status fa_sortformer_offline_windows(const fa_sortformer_offline_config *cfg, const int64_t *n_mel_frames, int32_t batch,
                                        fa_sortformer_window *windows, int64_t capacity, int64_t *count, int64_t *total_out,
                                        int64_t *window_range);
/* The model's inputs (:98-119) for every window of the batch: d_out float[windows][n_mels][window * subsampling] with the tail past
 * valid_mel zero-filled, d_mel_length int32[windows].  d_mel is the batch's mel on the device in either layout the mel plan writes:
 * FA_MEL_LAYOUT_MEL_MAJOR recording b at d_mel + b * rec_stride as [n_mels][frame_stride], FA_MEL_LAYOUT_FRAME_MAJOR as
 * [frames][n_mels] (frame_stride unused).  `windows` must be the count fa_sortformer_offline_windows gives for the same lengths.
 * n_mel_frames: HOST pointer; the call returns when the kernel has finished (the staged window table lives for the call). */
fa_status fa_sortformer_pack_windows_dev(fa_ctx *ctx, const fa_sortformer_offline_config *cfg, const float *d_mel, int32_t layout,
                                         int64_t rec_stride, int64_t frame_stride, const int64_t *n_mel_frames, int32_t batch,
                                         int64_t windows, float *d_out, int32_t *d_mel_length);
/* :321-358 for every recording: d_preds float[windows][window][speakers] (the model's output, in window order) -> d_global
 * float[sum total_out][speakers], the recordings' timelines one after the other, and d_mapping int32[windows][speakers],
 * mapping[window column] = global column.  Bit for bit the reference's arithmetic: each correlation is a sequential fp32 chain in frame
 * order (multiply, then add; terms whose global value equals 0 skipped), the bijections are tried in the reference's enumeration order,
 * the strictly greatest score wins and the first enumerated wins ties, NaN never wins.  1 to 4 speakers (INVALID_ARGUMENT above).
 * With 2 * overlap <= window (the default geometry) the windows' correlations and the merge run in parallel; any other geometry runs
 * window by window in one workgroup per recording, which gives the same bits and is slow.  Synchronous like the pack. */
fa_status fa_sortformer_stitch_dev(fa_ctx *ctx, const fa_sortformer_offline_config *cfg, const float *d_preds, const int64_t *n_mel_frames,
                                   int32_t batch, int64_t windows, float *d_global, int32_t *d_mapping);
/* SortformerSpeakerStitcher.alignment on HOST arrays float[frames][speakers]: mapping int32[speakers]; identity when frames <= 0. */
fa_status fa_sortformer_stitcher_alignment(const float *global, const float *window, int64_t frames, int32_t speakers, int32_t *mapping);

/* ------------------------------------------------------------------ diarizer timeline ------ */
/* DiarizerTimeline (FluidAudio/Diarizer/DiarizerTimeline.swift), the segment detection shared by Sortformer (offline and streaming)
 * and LS-EEND.  DiarizerTimelineConfig (:9-164); the seconds initialiser's Int(round(x / frameDuration)) lives in the wrappers. */
enum { FA_ACTIVITY_SIGMOIDS = 0, FA_ACTIVITY_LOGITS = 1 };
typedef struct {
    float onset_threshold;           /* 0.5: silent -> speaking when activity > onset */
    float offset_threshold;          /* 0.5: speaking stays speaking while activity >= offset */
    int32_t onset_pad_frames;        /* 0 */
    int32_t offset_pad_frames;       /* 0 */
    int32_t min_frames_on;           /* 0 */
    int32_t min_frames_off;          /* 0 */
    float frame_duration;            /* 0.08 s; segment times are Float(frame) * frame_duration in the wrappers */
    int32_t speakers;                /* 4; any value >= 1 */
    int32_t activity_type;           /* FA_ACTIVITY_SIGMOIDS.  FA_ACTIVITY_LOGITS is INVALID_ARGUMENT: it goes through the platform's log,
                                        and no caller in the reference selects it */
} fa_timeline_config;
void fa_timeline_default_config(fa_timeline_config *cfg);   /* DiarizerTimelineConfig.sortformerDefault */
typedef struct {
    int32_t recording, speaker;
    int64_t start_frame, end_frame;  /* a start before frame 0 (onset padding) is kept, as the reference keeps it */
    float activity;                  /* activitySum / Float(activeFrameCount), 0 for no frames */
    int32_t finalized;               /* bit 0: DiarizerSegment.isFinalized; bit 1: held in the speaker's finalized list after the call
                                        (3 finalized, 2 tentative moved there by finalize() when is_complete, 0 tentative) */
} fa_diarizer_segment;
/* rebuild(finalizedPredictions:tentativePredictions:keepingSpeakers:false,isComplete:) (:945-1003, 1169-1336) for `batch` recordings:
 * finalized float[sum finalized_frames][speakers] and tentative float[sum tentative_frames][speakers], the recordings one after the
 * other (tentative and tentative_frames may be NULL: none).  The records come ordered by recording, then speaker, then as the speaker's
 * lists hold them after the call (the finalized list, then the tentative one).  Every activity sum is the reference's sequential fp32
 * chain.  Not covered: addChunk's state across calls, maxStoredFrames, speaker names and snapshots.
 * segs HOST fa_diarizer_segment[capacity]; *count is set even when segs is NULL (SUCCESS) or too small (OUTPUT_TOO_SMALL, the first
 * `capacity` records are written); recording_counts HOST int64[batch] (nullable).  _dev: the predictions are DEVICE pointers read in
 * stream order; otherwise HOST pointers.  Synchronous: one host synchronisation for the raw run count, one for the segment counts,
 * then the copy of the records. */
fa_status fa_timeline_segments_dev(fa_ctx *ctx, const fa_timeline_config *cfg, const float *d_finalized, const int64_t *finalized_frames,
                                   const float *d_tentative, const int64_t *tentative_frames, int32_t batch, int32_t is_complete,
                                   fa_diarizer_segment *segs, int64_t capacity, int64_t *count, int64_t *recording_counts);
fa_status fa_timeline_segments(fa_ctx *ctx, const fa_timeline_config *cfg, const float *finalized, const int64_t *finalized_frames,
                               const float *tentative, const int64_t *tentative_frames, int32_t batch, int32_t is_complete,
                               fa_diarizer_segment *segs, int64_t capacity, int64_t *count, int64_t *recording_counts);

/* ------------------------------------------------------------------ diarization error rate ------ */
/* DiarizationDER.compute (FluidAudio/Diarizer/DiarizationDER.swift:52-231) with the integer Kuhn-Munkres it calls
 * (Diarizer/HungarianAssignment.swift:8-61), for `batch` (reference, hypothesis) pairs in one call: the frame-wise score the
 * reference's Sortformer and LS-EEND benchmarks print.  Every quantity is an integer count; the wrappers form the seconds and the
 * rate with the reference's expressions (:160-164).
 * A segment's label is its speaker's index BY FIRST APPEARANCE on its side of its recording (the wrappers number the strings); a
 * side holds at most FA_DER_MAX_LABELS labels (AMI has 5 speakers, VoxConverse at most 21).  A segment with end <= start is never
 * rasterised, but its label and its end count (:67-80).  Negative starts clip to frame 0. */
enum { FA_DER_MAX_LABELS = 64 };
typedef struct {
    int32_t label;                   /* 0 ... FA_DER_MAX_LABELS - 1 */
    int32_t reserved;
    double start, end;               /* seconds; finite */
} fa_der_segment;
typedef struct {
    double frame_step;               /* 0.01 s: the analysis grid; > 0 and finite */
    double collar;                   /* 0: the full width dropped around every reference boundary; >= 0 and finite */
} fa_der_config;
void fa_der_default_config(fa_der_config *cfg);
typedef struct {
    int64_t frames;                  /* Int(ceil(maxEnd / frameStep)) + 1; 0 for a pair without any label */
    int64_t miss, false_alarm, confusion, ref;   /* frames; seconds are Double(count) * frameStep */
    int32_t ref_labels, hyp_labels;  /* R, H */
} fa_der_counts;
/* HOST pointers.  ref_segs / hyp_segs hold the recordings' segments one after the other: recording b's are
 * [ref_range[b], ref_range[b + 1]) and [hyp_range[b], hyp_range[b + 1]).  counts HOST [batch].  mapping HOST int32: recording b's
 * hypothesis label h maps to reference label mapping[mapping_range[b] + h], or to -1 (no partner, or no overlap with it); the
 * range must hold hyp_labels entries (OUTPUT_TOO_SMALL otherwise) and what it holds beyond them is set to -1.  overlap (nullable)
 * HOST int64[overlap_capacity]: the [hyp_labels][ref_labels] tables of overlapping frames, counted before the collar, recording
 * after recording (OUTPUT_TOO_SMALL when they do not fit).
 * INVALID_ARGUMENT — decided before any device work — for a non-finite time, a label outside 0 ... 63, frame_step <= 0 or
 * non-finite, collar < 0 or non-finite; INDEX_OVERFLOW for a recording of 2^31 frames or more.  Everything between the upload of
 * the segments and the download of the counts stays on the device; one host synchronisation. */
fa_status fa_der_score_batch(fa_ctx *ctx, const fa_der_config *cfg, const fa_der_segment *ref_segs, const int64_t *ref_range,
                             const fa_der_segment *hyp_segs, const int64_t *hyp_range, int32_t batch, fa_der_counts *counts,
                             int32_t *mapping, const int64_t *mapping_range, int64_t *overlap, int64_t overlap_capacity);

/* ------------------------------------------------------------------ word / character error rate ------ */
/* WERCalculator.editDistance (FluidAudioCLI/Utils/WERCalculator.swift:178-239) for n_pairs (hypothesis, reference) pairs of symbol
 * sequences in one call: the Levenshtein distance and the insertion / deletion / substitution counts of the reference's traceback
 * (a match first, then a substitution, a deletion, an insertion).  The total is StringUtils.levenshteinDistance
 * (FluidAudio/Shared/StringUtils.swift:12-40) and the CLI's levenshteinDistance.  Integers only: a symbol is any int32 (the wrappers
 * number words and characters by first appearance) and is compared for equality.  The wrappers form the rates with the reference's
 * expressions (Double(total) / Double(ref_len), 0 for an empty reference). */
typedef struct {
    int32_t total;                   /* the edit distance = insertions + deletions + substitutions */
    int32_t insertions, deletions, substitutions;
    int32_t hyp_len, ref_len;        /* m, n */
} fa_edit_counts;
/* hyp / ref hold the pairs' sequences one after the other: pair k's are hyp[hyp_range[k] ... hyp_range[k + 1]) and
 * ref[ref_range[k] ... ref_range[k + 1]).  The ranges (n_pairs + 1 entries each) and out [n_pairs] are HOST memory; hyp and ref are
 * HOST pointers, for _dev DEVICE pointers on the context's device read in stream order.  The results come in input order.
 * INVALID_ARGUMENT for a null or descending range, a negative range start or n_pairs < 0, INDEX_OVERFLOW for a side longer than
 * INT32_MAX or 2^31 - 1 pairs or more — decided from the ranges alone, before any device work.  n_pairs == 0: SUCCESS, nothing is
 * written.  Pairs with an empty side are answered on the host; one host synchronisation per call. */
fa_status fa_edit_distance_batch(fa_ctx *ctx, const int32_t *hyp, const int64_t *hyp_range, const int32_t *ref, const int64_t *ref_range,
                                 int64_t n_pairs, fa_edit_counts *out);
fa_status fa_edit_distance_batch_dev(fa_ctx *ctx, const int32_t *d_hyp, const int64_t *hyp_range, const int32_t *d_ref, const int64_t *ref_range,
                                     int64_t n_pairs, fa_edit_counts *out);

/* ------------------------------------------------------------------ Paraformer: CIF, token timestamps ------ */
/* The host loop between Paraformer's networks, batched over utterances: ParaformerCif.integrateAndFireWithFireFrames
 * (FluidAudio/ASR/Paraformer/ParaformerCif.swift:19-50) with the decoder's input packing of ParaformerManager.runDecoder
 * (ParaformerManager.swift:416-448, rows(of:) :465-486), and the raw token spans of decodeWithTimestamps (:134-226).  Every fp32
 * chain is evaluated in the reference's order and the time arithmetic is fp64: the outputs are the reference's bit for bit.
 * The networks (preprocessor, encoder, CifAlphas, decoder) and the vocabulary are the caller's.  The reference has no unit test of
 * these routines: parity is pinned by the restatement of tests/paraformer_restatement.py. */
typedef struct {
    float threshold;                 /* ParaformerConfig.cifThreshold */
    float tail_threshold;            /* ParaformerConfig.cifTailThreshold: the alpha of the tail frame */
    int32_t max_tokens;              /* ParaformerConfig.decoderMaxTokens: rows of ac, columns of token_ids */
    int32_t enc_frames;              /* ParaformerConfig.decoderEncFrames: rows of enc_packed */
} fa_paraformer_cif_config;
void fa_paraformer_cif_default_config(fa_paraformer_cif_config *cfg);   /* 1.0, 0.45, 128, 512 */
/* enc: batch matrices addressed like the logits of fa_ctc_greedy_batch_dev (dtype FA_DTYPE_F32 or FA_DTYPE_F16, widened on load; `dim`
 * elements of a row are read, never the padding).  alphas float[batch][alpha_stride].  valid_frames HOST int32[batch] (nullable: all
 * frames; clamped to [0, frames] — the caller clamps to decoderEncFrames as transcribe does).  cfg nullable: the defaults.
 * Per utterance, over t = 0 ... T with the tail frame (alpha = tail_threshold, a zero row) at t = T: at most one fire per frame,
 * alphas above the threshold fire on consecutive frames, T == 0 yields no token.
 * ac float[batch][max_tokens][dim]: the first min(L, max_tokens) tokens, zeros behind them.  enc_packed (nullable)
 * float[batch][enc_frames][dim]: rows below min(T, enc_frames) widened, zeros behind them.  token_counts HOST int32[batch]:
 * min(L, max_tokens); fire_counts HOST int32[batch]: L; fire_frames HOST int32[batch][frames + 1]: all L fire frames, -1 behind them.
 * _dev: enc, alphas, ac, enc_packed are DEVICE pointers, read and written in stream order; otherwise HOST pointers.  INVALID_ARGUMENT
 * for a NULL pointer, a negative size, a stride below its row, a dtype or config out of range; INDEX_OVERFLOW for a batch of more than
 * INT32_MAX frames or tokens — decided before any device work, nothing written.  batch == 0: SUCCESS.  One host synchronisation. */
fa_status fa_paraformer_cif_dev(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const void *d_enc, int32_t dtype, int32_t batch,
                                int32_t frames, int32_t dim, int64_t row_stride, int64_t matrix_stride, const float *d_alphas,
                                int64_t alpha_stride, const int32_t *valid_frames, float *d_ac, float *d_enc_packed,
                                int32_t *token_counts, int32_t *fire_counts, int32_t *fire_frames);
fa_status fa_paraformer_cif(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const void *enc, int32_t dtype, int32_t batch,
                            int32_t frames, int32_t dim, int64_t row_stride, int64_t matrix_stride, const float *alphas,
                            int64_t alpha_stride, const int32_t *valid_frames, float *ac, float *enc_packed, int32_t *token_counts,
                            int32_t *fire_counts, int32_t *fire_frames);
/* A raw span of decodeWithTimestamps (its `raw` array, :203-226): token_index is the position of the token in the utterance's row of
 * token_ids; the text and the merge of BPE pieces (:228-256) are the wrappers'. */
typedef struct { int32_t utterance, token_index; double start, end; } fa_paraformer_span;
/* alphas and valid_frames as above (only tail_threshold and max_tokens of cfg matter).  token_ids int32[batch][max_tokens]: the argmax
 * of the decoder's logits; token_counts HOST int32[batch], each in [0, max_tokens].  keep HOST uint8[vocab]: 0 for the ids the
 * reference drops (:146-156: blank, <s>, </s>, ids without a vocabulary entry, empty strings); an id outside [0, vocab) is dropped.
 * audio: the utterances' 16 kHz samples one after the other, utterance b at audio_offsets[b] ... audio_offsets[b + 1] (HOST
 * int64[batch + 1]); finite samples (the reference sorts them: the order of NaN is unspecified there; here such input ends without a
 * fault).  spans HOST [capacity], by utterance and token; *count is set even when spans is NULL (SUCCESS) or too small
 * (OUTPUT_TOO_SMALL, the first `capacity` records are written); utterance_counts HOST int64[batch] (nullable).  An utterance without a
 * kept token or with fewer than two fires yields none.  _dev: alphas, token_ids and audio are DEVICE pointers.  Argument errors as
 * above; one host synchronisation behind the uploads. */
fa_status fa_paraformer_timestamps_dev(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const float *d_alphas, int64_t alpha_stride,
                                       int32_t batch, int32_t frames, const int32_t *valid_frames, const int32_t *d_token_ids,
                                       const int32_t *token_counts, const uint8_t *keep, int32_t vocab, const float *d_audio,
                                       const int64_t *audio_offsets, fa_paraformer_span *spans, int64_t capacity, int64_t *count,
                                       int64_t *utterance_counts);
fa_status fa_paraformer_timestamps(fa_ctx *ctx, const fa_paraformer_cif_config *cfg, const float *alphas, int64_t alpha_stride,
                                   int32_t batch, int32_t frames, const int32_t *valid_frames, const int32_t *token_ids,
                                   const int32_t *token_counts, const uint8_t *keep, int32_t vocab, const float *audio,
                                   const int64_t *audio_offsets, fa_paraformer_span *spans, int64_t capacity, int64_t *count,
                                   int64_t *utterance_counts);

/* ------------------------------------------------------------------ TDT long-form: merging the windows' tokens ------ */
/* What ChunkProcessor does with the tokens of a recording's overlapping windows (FluidAudio/ASR/Parakeet/SlidingWindow/TDT/
 * ChunkProcessor.swift): merged = w[0]; merged = mergeChunks(merged, w[k]) for every further window (:952-1219 with tokensMatch,
 * tokenIdsMatch, mergeUsingMatches, wordInitialIndex, popSeamWord, mergeByMidpoint; SequenceMatcher.findContiguousMatches and
 * findLongestCommonSubsequence, TokenDeduplication/SequenceMatcher.swift:127-225), then enforceMonotonicTimestamps (:843-855) —
 * batched over recordings, one wavefront per recording, on the arrays the greedy walk leaves on the device.  Integer rules and the
 * reference's own fp64 time expressions, evaluated without contraction: the merged stream is the reference's bit for bit (pinned by
 * its 17 literal mergeTokenWindowsForTesting cases).  OUT OF SCOPE: collapseSeamWordDuplicates (Unicode strings), repairSeamGaps
 * (needs the networks), the planning of chunk starts, the streaming removeDuplicateTokenSequence. */
typedef struct {
    double frame_seconds;            /* ASRConstants.secondsPerEncoderFrame */
    double overlap_seconds;          /* ChunkProcessor.overlapSeconds */
} fa_tdt_merge_config;
void fa_tdt_merge_default_config(fa_tdt_merge_config *cfg);   /* Double(1280) / Double(16000), 2.0 */
/* A seam's route: base strategy | tail handling << 4; FA_TDT_MERGE_NO_SEAM for a recording's first window and for seams not done. */
#define FA_TDT_MERGE_EMPTY 0            /* a side without tokens (:958-959) */
#define FA_TDT_MERGE_CONCAT 1           /* left ends before right starts (:976-978) */
#define FA_TDT_MERGE_CONTIGUOUS 2       /* the longest contiguous run holds minimumPairs (:1015-1024) */
#define FA_TDT_MERGE_LCS 3              /* the LCS fallback (:1026-1050) */
#define FA_TDT_MERGE_MIDPOINT 4         /* mergeByMidpoint (:993-997, :1033-1037) */
#define FA_TDT_MERGE_TAIL_VERBATIM 0    /* right's tail as it is */
#define FA_TDT_MERGE_TAIL_ADOPT_RIGHT 1 /* the seam word popped, right's segmentation of it adopted (:1123-1128) */
#define FA_TDT_MERGE_TAIL_KEEP_LEFT 2   /* left keeps its word, right resumes at its next word-initial piece (:1129-1146) */
#define FA_TDT_MERGE_NO_SEAM (-1)
/* d_tok, d_time, d_dur, d_conf [windows][max_out] and d_count [windows]: what fa_tdt_greedy_tables_dev / fa_tdt_greedy_logits_dev
 * wrote (global timestamps); min(count, max_out) tokens of a window are used, a negative count as 0.  window_range HOST
 * int64[n_recordings + 1]: recording r owns the windows [window_range[r], window_range[r + 1]), in order; windows without tokens are
 * legal anywhere.  cfg nullable: the defaults.
 * splice_safe HOST uint8[vocab] (nullable = spliceSafeTokenIds == nil, the legacy splices; an all-zero table is the EMPTY set, which
 * is not the same) and case_canon HOST int32[vocab] (nullable = caseVariantIds == nil; -1: no entry): the tables the reference
 * builds from its vocabulary (spliceSafeTokenIds, caseVariantCanonicalIds) stay the caller's.  An id outside [0, vocab) is unsafe and
 * has no entry.
 * Outputs are flat: recording r's merged stream goes to [out_range[r], out_range[r + 1]) of d_out_tok / d_out_time / d_out_dur /
 * d_out_conf (out_range HOST int64[n_recordings + 1]); out_counts HOST int32[n_recordings]: its length; statuses HOST
 * int32[n_recordings]: FA_SUCCESS, or FA_OUTPUT_TOO_SMALL for a recording whose slice ran out (its count is 0, its slice unspecified;
 * the other recordings are untouched by it).  A merge emits a token of the right window at most twice (a right-side gap adopted, then
 * the seam word spliced again from its start), so |w0| + 2 sum_{k >= 1} |wk| tokens are always enough.  seam_routes (nullable) HOST
 * int32, indexed like the windows: entries [window_range[0], window_range[n_recordings]) are written.
 * _dev: the window arrays and the four output arrays are DEVICE pointers on the context's device, read and written in stream order;
 * otherwise HOST pointers.  INVALID_ARGUMENT for a NULL or descending range, a range starting below 0, a missing array, a negative
 * size, a frame that is not positive or an overlap that is negative (or either not finite); INDEX_OVERFLOW for a slice longer than
 * INT32_MAX or 2^31 - 1 recordings or more — decided before any device work, nothing written.  n_recordings == 0: SUCCESS.  One host
 * synchronisation per call; fa_ctx_set_timing brackets the kernel.  Overlap sides of any length are served (beyond 128 tokens a
 * side through a workspace of (largest slice) x max_out bits per wavefront in flight: ALLOCATION_FAILURE when that cannot be had). */
fa_status fa_tdt_merge_windows_dev(fa_ctx *ctx, const fa_tdt_merge_config *cfg, const int32_t *d_tok, const int32_t *d_time,
                                   const int32_t *d_dur, const float *d_conf, const int32_t *d_count, int32_t max_out,
                                   const int64_t *window_range, int64_t n_recordings, const uint8_t *splice_safe,
                                   const int32_t *case_canon, int32_t vocab, int32_t *d_out_tok, int32_t *d_out_time,
                                   int32_t *d_out_dur, float *d_out_conf, const int64_t *out_range, int32_t *out_counts,
                                   int32_t *statuses, int32_t *seam_routes);
fa_status fa_tdt_merge_windows(fa_ctx *ctx, const fa_tdt_merge_config *cfg, const int32_t *tok, const int32_t *time,
                               const int32_t *dur, const float *conf, const int32_t *count, int32_t max_out,
                               const int64_t *window_range, int64_t n_recordings, const uint8_t *splice_safe,
                               const int32_t *case_canon, int32_t vocab, int32_t *out_tok, int32_t *out_time, int32_t *out_dur,
                               float *out_conf, const int64_t *out_range, int32_t *out_counts, int32_t *statuses,
                               int32_t *seam_routes);

/* ------------------------------------------------------------------ VAD: speech segments, model rows, streaming events ------ */
/* The host arithmetic round the Silero network (FluidAudio/VAD), batched over recordings: segmentSpeech(from:totalSamples:config:)
 * with detectSpeechSampleRanges (VadManager+SpeechSegmentation.swift:22-51, 71-234), the model's input rows of processAudioSamples /
 * processChunk (VadManager.swift:162-206, 352-376), the audio of segmentSpeechAudio (:55-67) and streamingStateMachine
 * (VadManager+Streaming.swift:31-107).  Integers, fp32 comparisons and fp64 divisions in the reference's order: the outputs are the
 * reference's bit for bit (pinned by its VadSegmentationTests / VadStreamingTests through tests/vad_restatement.py).  Frames are
 * chunks of 4096 samples at 16 kHz; a model row is 64 context samples and 4096 chunk samples.  OUT OF SCOPE: the Silero network and its
 * LSTM state (the caller's), isSilentAudio.  FSMN-VAD (VAD/Fsmn/) has the section after this one.
 * Conventions of the four entries: cfg nullable = the defaults; _dev takes DEVICE pointers where it says so and reads them in stream
 * order; *count is set even when the output is NULL (SUCCESS) or too small (OUTPUT_TOO_SMALL, the first `capacity` records written);
 * every refusal is decided before any device work; batch == 0: SUCCESS; one host synchronisation unless stated otherwise. */
typedef struct {
    float default_threshold;                          /* VadConfig.defaultThreshold */
    int32_t reserved0;
    double min_speech_duration, min_silence_duration, max_speech_duration, speech_padding;   /* seconds; max_speech_duration may be +inf */
    float silence_threshold_for_split;
    int32_t has_negative_threshold;                   /* negativeThreshold != nil */
    float negative_threshold;
    float negative_threshold_offset;
    double min_silence_at_max_speech;
    int32_t use_max_possible_silence_at_max_speech;
    int32_t reserved1;
} fa_vad_segmentation_config;
void fa_vad_default_config(fa_vad_segmentation_config *cfg);   /* 0.85; 0.15, 0.75, 14.0, 0.1; 0.3; nil, 0.15; 0.098; true */
typedef struct { int32_t recording, reserved; int64_t start_sample, end_sample; double start_time, end_time; } fa_vad_segment;
/* probs float[sum frames]: recording b's probabilities at frame_range[b] ... frame_range[b + 1] (HOST int64[batch + 1]);
 * total_samples HOST int64[batch].  A recording without frames or with total_samples <= 0 yields nothing; NaN probabilities are in
 * neither class.  segs HOST [capacity], by recording and time: the times are Double(sample) / 16000.0.  recording_counts HOST
 * int64[batch] (nullable).  INVALID_ARGUMENT for the reference's preconditions on the config, a NaN duration, a duration whose
 * sample count does not fit int64 (Swift traps there), a NULL, descending or negative range; INDEX_OVERFLOW for a recording of 2^31
 * frames or more.  _dev: probs is a DEVICE pointer. */
fa_status fa_vad_segments_dev(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *d_probs, const int64_t *frame_range,
                              const int64_t *total_samples, int32_t batch, fa_vad_segment *segs, int64_t capacity, int64_t *count,
                              int64_t *recording_counts);
fa_status fa_vad_segments(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *probs, const int64_t *frame_range,
                          const int64_t *total_samples, int32_t batch, fa_vad_segment *segs, int64_t capacity, int64_t *count,
                          int64_t *recording_counts);
int64_t fa_vad_chunk_count(int64_t samples);          /* ceil(samples / 4096); 0 for samples <= 0 */
/* audio: the recordings' samples one after the other, recording b at audio_offsets[b] ... audio_offsets[b + 1] (HOST
 * int64[batch + 1]).  rows float[row_capacity][4160]: recording b's fa_vad_chunk_count rows from chunk_range[b] on (HOST
 * int64[batch + 1], written whenever the offsets are sound).  A row is the last 64 samples of the padded chunk before it (zeros
 * for a recording's first) and the chunk, a short one filled with its last sample; samples are copied as bits.  OUTPUT_TOO_SMALL
 * when row_capacity is below chunk_range[batch]: nothing is packed.  _dev: audio and rows are DEVICE pointers and the entry does NOT
 * synchronise. */
fa_status fa_vad_pack_chunks_dev(fa_ctx *ctx, const float *d_audio, const int64_t *audio_offsets, int32_t batch, float *d_rows,
                                 int64_t row_capacity, int64_t *chunk_range);
fa_status fa_vad_pack_chunks(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, int32_t batch, float *rows,
                             int64_t row_capacity, int64_t *chunk_range);
/* The speech audio of every segment, packed: segment i goes to out[out_range[i] ... out_range[i + 1]) (HOST int64[n_segments + 1],
 * written whenever the arguments are sound).  The bounds are the reference's Int(start_time * 16000.0) and Int(end_time * 16000.0),
 * clamped to the recording — NOT start_sample / end_sample, from which the trip through fp64 seconds can differ by one.  segs HOST
 * (the records of fa_vad_segments, or hand-made times).  INVALID_ARGUMENT for a recording outside the batch or a time that does not
 * fit int64; OUTPUT_TOO_SMALL when out_capacity is below out_range[n_segments]: nothing is copied.  _dev: audio and out are DEVICE
 * pointers. */
fa_status fa_vad_gather_segments_dev(fa_ctx *ctx, const float *d_audio, const int64_t *audio_offsets, int32_t batch,
                                     const fa_vad_segment *segs, int64_t n_segments, float *d_out, int64_t out_capacity,
                                     int64_t *out_range);
fa_status fa_vad_gather_segments(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, int32_t batch,
                                 const fa_vad_segment *segs, int64_t n_segments, float *out, int64_t out_capacity, int64_t *out_range);
typedef struct { int32_t triggered, has_temp_end; int64_t temp_end_sample, processed_samples; } fa_vad_stream_state;
#define FA_VAD_SPEECH_START 0
#define FA_VAD_SPEECH_END 1
typedef struct { int32_t stream, chunk, kind, reserved; int64_t sample_index; double time; } fa_vad_stream_event;
/* `streams` state machines advanced by chunk_counts[s] (HOST int32[streams], each in [0, max_chunks]) chunks each: probs
 * float[streams][max_chunks], chunk_samples int32[streams][max_chunks] (nullable: 4096 each).  states HOST [streams], in and out.
 * events HOST [capacity], by stream and chunk, at most one per chunk; time is NaN unless return_seconds, else
 * (seconds * 10^time_resolution).rounded() / 10^time_resolution (halves away from zero).  INVALID_ARGUMENT for a time_resolution
 * outside 0 ... 22, where the power is not exact.  _dev: probs and chunk_samples are DEVICE pointers. */
fa_status fa_vad_stream_advance_dev(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *d_probs, const int32_t *chunk_counts,
                                    const int32_t *d_chunk_samples, int32_t streams, int32_t max_chunks, fa_vad_stream_state *states,
                                    int32_t return_seconds, int32_t time_resolution, fa_vad_stream_event *events, int64_t capacity,
                                    int64_t *count);
fa_status fa_vad_stream_advance(fa_ctx *ctx, const fa_vad_segmentation_config *cfg, const float *probs, const int32_t *chunk_counts,
                                const int32_t *chunk_samples, int32_t streams, int32_t max_chunks, fa_vad_stream_state *states,
                                int32_t return_seconds, int32_t time_resolution, fa_vad_stream_event *events, int64_t capacity,
                                int64_t *count);

/* ------------------------------------------------------------------ FSMN-VAD: chunk schedule, model rows, segments ------ */
/* The host arithmetic round the two networks of FsmnVadManager (FluidAudio/VAD/Fsmn/FsmnVadManager.swift), batched over recordings:
 * the chunk schedule of concatenateChunks (:91-109) with lfrFrameCount (:113-117), the rows of chunkSilence (:119-155: the scaled
 * waveform, the zero-padded bucket of features, column 0 of the scores onto the recording's frame grid) and decide (:159-201).
 * Integers and one fp32 comparison per frame: the outputs are the reference's, quirks included (tests/fsmn_vad_restatement.py restates
 * the lines; with equal thresholds a window count of exactly that value flips preSpeech on every frame, and the segment behind a
 * maximal-length close starts inside the one before it).  Frames are 10 ms of 16 kHz audio.  OUT OF SCOPE: the preprocessor and the
 * scorer (the caller's), detect(audioURL:)'s file reading and resampling (fa_resample_poly), isSilentAudio.
 * The conventions are those stated above fa_vad_segmentation_config. */
typedef struct {
    float silence_threshold;                          /* a frame is speech when p <= threshold: a NaN is not speech */
    int32_t window_frames;                            /* 1 ... 64 */
    int32_t sil_to_speech_frames, speech_to_sil_frames;   /* window counts, each 0 ... window_frames */
    int32_t max_end_silence_frames;                   /* >= 1 */
    int32_t lookback_frames, lookahead_frames;        /* >= 0 */
    int32_t max_segment_frames;                       /* >= 1 */
    int32_t frame_ms;                                 /* >= 1 */
} fa_fsmn_vad_config;
void fa_fsmn_vad_default_config(fa_fsmn_vad_config *cfg);     /* 0.2; 20, 15, 15; 80; 20, 10; 6000; 10 */
/* bucket: the first of 512 / 1024 / 2048 / 3072 that holds `frames`.  keep_from: 0 for a recording's first chunk, else 2 (the frames
 * computed against replicate padding).  first_frame: the frame of the recording at which the chunk's first kept frame lands. */
typedef struct { int32_t recording, bucket; int64_t start_sample, end_sample; int32_t frames, keep_from; int64_t first_frame; } fa_fsmn_vad_chunk;
#define FA_FSMN_VAD_END_SILENCE 0
#define FA_FSMN_VAD_MAX_LENGTH 1
#define FA_FSMN_VAD_END_OF_AUDIO 2
typedef struct { int32_t recording, reason; int32_t start_frame, end_frame; int64_t start_ms, end_ms; } fa_fsmn_vad_segment;
int64_t fa_fsmn_vad_frame_count(int64_t samples);     /* lfrFrameCount: 0 below 400 samples, else max(0, (samples - 400) / 160 - 1) */
/* The chunks of every recording (no context, no device).  total_samples HOST int64[batch]; chunks HOST [capacity] (nullable), by
 * recording and time; chunk_range and frame_range HOST int64[batch + 1], written before the capacity is judged: recording b's chunks
 * and the frames of its concatenated probabilities.  A chunk whose frames do not exceed keep_from is dropped and ends its recording,
 * as the reference's loop ends; samples <= 0 plan nothing.  INVALID_ARGUMENT for a negative count or a missing array. */
fa_status fa_fsmn_vad_plan_chunks(const int64_t *total_samples, int32_t batch, fa_fsmn_vad_chunk *chunks, int64_t capacity, int64_t *count,
                                  int64_t *chunk_range, int64_t *frame_range);
/* rows float[row_capacity][row_stride]: row c is audio[start_sample ... end_sample) of chunk c's recording times 32768.0f (one fp32
 * multiply), zeros up to row_stride.  audio_offsets HOST int64[batch + 1] as for fa_vad_pack_chunks; chunks HOST [n_chunks].
 * INVALID_ARGUMENT for a chunk outside its recording or longer than row_stride; OUTPUT_TOO_SMALL when row_capacity is below n_chunks:
 * nothing is written.  _dev: audio and rows are DEVICE pointers and the entry does NOT synchronise. */
fa_status fa_fsmn_vad_pack_waveforms_dev(fa_ctx *ctx, const float *d_audio, const int64_t *audio_offsets, int32_t batch,
                                         const fa_fsmn_vad_chunk *chunks, int64_t n_chunks, float *d_rows, int64_t row_stride,
                                         int64_t row_capacity);
fa_status fa_fsmn_vad_pack_waveforms(fa_ctx *ctx, const float *audio, const int64_t *audio_offsets, int32_t batch,
                                     const fa_fsmn_vad_chunk *chunks, int64_t n_chunks, float *rows, int64_t row_stride,
                                     int64_t row_capacity);
/* The scorer's input: d_feats [n_chunks][feat_stride][400] (dtype FA_DTYPE_F32 or FA_DTYPE_F16, widened exactly) -> d_out
 * float[n_chunks][bucket][400]; a chunk's first `frames` rows are copied, the others are zero.  INVALID_ARGUMENT for a chunk with more
 * frames than bucket or feat_stride.  DEVICE pointers; the entry does NOT synchronise. */
fa_status fa_fsmn_vad_pack_feats_dev(fa_ctx *ctx, const void *d_feats, int32_t dtype, int64_t feat_stride, const fa_fsmn_vad_chunk *chunks,
                                     int64_t n_chunks, int32_t bucket, float *d_out);
/* Column 0 of d_scores [n_chunks][bucket][vocab] (fp32 or fp16) for frames keep_from ..< frames of every chunk ->
 * d_silence[frame_range[recording] + first_frame + (i - keep_from)]: the strided gather and the concatenation in one pass.
 * frame_range HOST int64[batch + 1] (fa_fsmn_vad_plan_chunks'); INVALID_ARGUMENT for a chunk that ends beyond its recording's frames,
 * OUTPUT_TOO_SMALL when silence_capacity is below frame_range[batch].  DEVICE pointers; the entry does NOT synchronise. */
fa_status fa_fsmn_vad_gather_silence_dev(fa_ctx *ctx, const void *d_scores, int32_t dtype, int32_t bucket, int32_t vocab,
                                         const fa_fsmn_vad_chunk *chunks, int64_t n_chunks, const int64_t *frame_range, int32_t batch,
                                         float *d_silence, int64_t silence_capacity);
/* decide.  probs float[sum frames]: the silence probabilities, recording b's at frame_range[b] ... frame_range[b + 1] (HOST
 * int64[batch + 1]).  segs HOST [capacity], by recording and time; reason: FA_FSMN_VAD_END_SILENCE (the end is the closing frame -
 * max_end_silence_frames + lookahead_frames, not clamped), _MAX_LENGTH, _END_OF_AUDIO (the end is the frame count); the milliseconds
 * are frames * frame_ms.  recording_counts HOST int64[batch] (nullable).  INVALID_ARGUMENT for a config outside the bounds stated at
 * its fields, a NaN threshold, a NULL, descending or negative range; INDEX_OVERFLOW for a recording of 2^31 frames or more (or whose
 * frames plus the look-ahead reach 2^31).  _dev: probs is a DEVICE pointer. */
fa_status fa_fsmn_vad_segments_dev(fa_ctx *ctx, const fa_fsmn_vad_config *cfg, const float *d_probs, const int64_t *frame_range,
                                   int32_t batch, fa_fsmn_vad_segment *segs, int64_t capacity, int64_t *count, int64_t *recording_counts);
fa_status fa_fsmn_vad_segments(fa_ctx *ctx, const fa_fsmn_vad_config *cfg, const float *probs, const int64_t *frame_range, int32_t batch,
                               fa_fsmn_vad_segment *segs, int64_t capacity, int64_t *count, int64_t *recording_counts);

/* ------------------------------------------------------------------ TDT long-form: planning the windows ------ */
/* What ChunkProcessor decides from the audio before any network runs (FluidAudio/ASR/Parakeet/SlidingWindow/TDT/
 * ChunkProcessor.swift), batched over recordings: speechEndSamples :112-128, the chunk starts (chunkStarts :163-177, regularChunkStarts
 * :179-187, silenceAlignedChunkStarts :189-268 with bestBoundaryCandidate, the two threshold tests, wouldCompressSpeechTail,
 * shouldUseWarmupPrefix and boundaryEnergyScore :270-396), the window loop of process (:501-507, 520-565, 577, 626-636;
 * DualDecodeArbitration.decodeOneChunk :359-402 is the same arithmetic with mel context 0) with lastChunkWarmupSamples :85-102, the
 * preprocessor's rows (padAudioIfNeeded, AsrManager+Pipeline.swift:153-156), and the half of the seam-gap repair that reads audio
 * (adaptiveSpeechRmsThreshold :1245-1276, speechLikeSeconds :1518-1534).  Every energy is the reference's `sum += sample * sample` in
 * fp32, in order, one rounded product and one rounded addition per sample; integers, fp32 and fp64 results are the reference's bit for
 * bit (pinned by its ChunkProcessorTests, EndAlignedFinalWindowTests and SeamGapRepairTests through tests/tdt_plan_restatement.py).
 * OUT OF SCOPE: the networks, the arbitration between the decodes (it compares confidences), finding the seam gaps from the tokens,
 * the re-decoding and collapseSeamWordDuplicates.
 * The four combinations in use: the default path (mel_chunk_context 1, regular starts, end_aligned = supportsSuppressedPrefix); v3
 * no-mel and arbitration path A (mel_chunk_context 0, silence_aligned 1, warmup_prefix_frames 0, end_aligned 1); path B (as A with
 * warmup_prefix_frames 7); path C (mel_chunk_context 0, regular starts, end_aligned 1).  The reference's literals (the ratios 0.05,
 * 0.35 and 0.8, the quiet threshold 0.003, the spans of 4.0 s, 0.5 s and 0.2 s, the window of sampleRate / 50 samples, the six-frame
 * minimal overlap, the gate's 0.0005, 0.008, 0.3 and 0.75) stay literals, derived from the geometry as the reference derives them.
 * Conventions: cfg nullable = the defaults; every refusal below is decided before any device work and writes nothing unless stated;
 * batch == 0: SUCCESS.  INVALID_ARGUMENT for: a NULL audio_offsets or output range, offsets that start below 0 or descend, a missing
 * array that would be read or written, a negative size; a geometry with sample_rate, frame_samples, mel_hop or max_model_samples
 * below 1, warmup_prefix_frames below 0, an overlap that is not finite, negative, or whose sample count does not fit int32; a chunk
 * that does not exceed the six-frame minimal overlap, or a chunk with its mel context longer than max_model_samples (a row could not
 * hold a window), or a warm-up prefix as long as a chunk; a search radius above 63 frames (4 s hold 64 frames or more) or a look-ahead
 * of more than 64 windows (the kernels' limits).  INDEX_OVERFLOW for a recording of 2^31 - 2 frames or more, or a call whose window
 * bound exceeds INT32_MAX. */
typedef struct {
    int32_t sample_rate;             /* ASRConstants.sampleRate 16000 */
    int32_t frame_samples;           /* ASRConstants.samplesPerEncoderFrame 1280 */
    int32_t mel_hop;                 /* ASRConstants.melHopSize 160 */
    int32_t max_model_samples;       /* ASRConstants.maxModelSamples 240000 */
    double overlap_seconds;          /* ChunkProcessor.overlapSeconds 2.0 */
    int32_t mel_chunk_context;       /* 1 */
    int32_t silence_aligned;         /* 0; preferSilenceAlignment */
    int32_t warmup_prefix_frames;    /* 0; a value above 0 selects the aligned starts too (:169) and lets a boundary ask for the prefix */
    int32_t end_aligned;             /* 1; supportsSuppressedPrefix(modelVersion) */
} fa_tdt_window_config;
void fa_tdt_window_default_config(fa_tdt_window_config *cfg);
/* chunkLayout (:48-75, :140-161) with cfg->warmup_prefix_frames as the prefix; every output is nullable.  Host only.  With the
 * defaults 238 080 / 206 080 / 1 280 / 0; with the mel context off 239 360 / 207 360 / 0 / 0. */
fa_status fa_tdt_window_layout(const fa_tdt_window_config *cfg, int64_t *chunk_samples, int64_t *stride_samples,
                               int64_t *mel_context_samples, int64_t *warmup_prefix_samples);
/* The most windows a recording of `samples` samples can get; 0 for samples <= 0, -1 for a refused geometry.  The list of starts holds
 * 1 + (samples - 1) / stride entries, ascending and below `samples`.  Regular starts are every multiple of the stride below `samples`:
 * a step beyond the list ends the loop.  Aligned starts can lie in front of their targets, so the loop may step on beyond the list,
 * by the stride each time and below `samples`: at most (samples - 1) / stride further windows. */
int64_t fa_tdt_window_count_bound(const fa_tdt_window_config *cfg, int64_t samples);
typedef struct {
    int32_t recording;
    int32_t use_warmup_prefix;       /* the start's ChunkStartDecision.useWarmupPrefix */
    int32_t is_last;
    int32_t emit_after_frame;        /* emitTokensAfterFrame; -1: nil */
    int32_t global_frame_offset;     /* (warmup > 0 ? contextStart : chunkStart) / frame_samples */
    int32_t context_frames;          /* contextSamples / frame_samples: contextFrameAdjustment */
    int32_t actual_audio_frames;     /* calculateEncoderFrames(length - contextSamples) */
    int32_t reserved;
    int64_t chunk_start, warmup_samples, context_samples, context_start;
    int64_t length;                  /* audioEnd - contextStart: the preprocessor's originalLength */
} fa_tdt_window;
/* audio: the recordings' samples one after the other, recording b at audio_offsets[b] ... audio_offsets[b + 1] (HOST int64[batch + 1];
 * no alignment of a recording's first sample is assumed).  windows HOST [capacity] (nullable with capacity 0: the count alone), by
 * recording and in a recording's order; window_range HOST int64[batch + 1]: recording b owns [window_range[b], window_range[b + 1]) —
 * the array fa_tdt_merge_windows takes.  The same windows as the five int32 arrays fa_tdt_greedy_tables_dev, fa_tdt_greedy_logits_dev
 * and fa_tdt_greedy_logits_lang_dev read, each [capacity] and nullable: audio_frames (actual_audio_frames), t0
 * (fa_tdt_initial_time_index(0, 0, context_frames); a window with a suppressed prefix has no context and starts at 0, its
 * initialTimeIndexOverride), is_last, global_offset, emit_after.  speech_end HOST int64[batch] (nullable): speechEndSamples, or the
 * recording's length where end_aligned is 0.  statuses HOST int32[batch] (nullable): FA_INVALID_ARGUMENT for a recording in which
 * the in-order sum of squares over a window [f F - F, f F + F) (F = frame_samples, clipped to the recording) is not finite for some
 * frame f — a NaN or an infinity among the samples, or squares that overflow; Swift's sorted() has no answer for such scores — which
 * gets zero windows and leaves the other recordings untouched.  Rounded addition of non-negative terms is monotone, so with every
 * such sum finite every energy the reference takes is finite.  A recording of 0 samples gets zero windows.
 * OUTPUT_TOO_SMALL when capacity is below window_range[batch]: window_range, speech_end and statuses are written, no window is.
 * _dev: audio and the five arrays are DEVICE pointers, read and written in stream order; otherwise HOST pointers.  One host
 * synchronisation per call. */
fa_status fa_tdt_plan_windows_dev(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *d_audio, const int64_t *audio_offsets,
                                  int32_t batch, fa_tdt_window *windows, int64_t capacity, int64_t *window_range,
                                  int32_t *d_audio_frames, int32_t *d_t0, int32_t *d_is_last, int32_t *d_global_offset,
                                  int32_t *d_emit_after, int64_t *speech_end, int32_t *statuses);
fa_status fa_tdt_plan_windows(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets,
                              int32_t batch, fa_tdt_window *windows, int64_t capacity, int64_t *window_range, int32_t *audio_frames,
                              int32_t *t0, int32_t *is_last, int32_t *global_offset, int32_t *emit_after, int64_t *speech_end,
                              int32_t *statuses);
/* The preprocessor's rows: rows float[row_capacity][max_model_samples], row i the `length` samples of windows[i] from context_start
 * of its recording, copied as bits, zeros behind them; lengths int32[n_windows] (nullable): the lengths, what fa_mel_plan_create /
 * fa_mel_execute_dev take beside the rows.  windows HOST [n_windows], the records of fa_tdt_plan_windows or hand-made ones:
 * INVALID_ARGUMENT for a recording outside the batch, a window outside its recording or longer than a row; OUTPUT_TOO_SMALL when
 * row_capacity is below n_windows (nothing is packed).  _dev: audio, rows and lengths are DEVICE pointers and the entry does NOT
 * synchronise (the windows travel in the launches' arguments); otherwise HOST pointers and one synchronisation. */
fa_status fa_tdt_pack_windows_dev(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *d_audio, const int64_t *audio_offsets,
                                  int32_t batch, const fa_tdt_window *windows, int64_t n_windows, float *d_rows, int64_t row_capacity,
                                  int32_t *d_lengths);
fa_status fa_tdt_pack_windows(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets,
                              int32_t batch, const fa_tdt_window *windows, int64_t n_windows, float *rows, int64_t row_capacity,
                              int32_t *lengths);
typedef struct { int32_t recording, reserved; int64_t from_sample, to_sample; } fa_tdt_span;
/* The speech-energy gate of the seam-gap repair.  thresholds HOST float[batch] (nullable): adaptiveSpeechRmsThreshold of every
 * recording — the frames from offset 0 on, those whose sum is exactly 0 left out, the element at min(count - 1, Int(Double(count) *
 * 0.75)) of the ascending RMS values by exact selection, times 0.3, clamped to [0.0005, 0.008]; 0.008 when no frame is left.
 * spans HOST [n_spans]: for span i span_frames[i] (HOST int64, nullable) counts the frames from_sample + k F, whole ones below
 * to_sample, whose RMS is above (strictly) the threshold of the span's recording — override_thresholds[recording] (HOST
 * float[batch]) when that array is given, the computed one otherwise — and span_seconds[i] (HOST double, nullable) is Double(frames)
 * * (Double(frame_samples) / Double(sample_rate)).  statuses as in fa_tdt_plan_windows: a refused recording has threshold NaN, its
 * spans 0 frames.  INVALID_ARGUMENT for a span whose recording is outside the batch or whose from_sample is below 0 or to_sample
 * beyond the recording (the reference would read past the audio).  _dev: audio is a DEVICE pointer.  One synchronisation. */
fa_status fa_tdt_speech_gate_dev(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *d_audio, const int64_t *audio_offsets,
                                 int32_t batch, const float *override_thresholds, float *thresholds, const fa_tdt_span *spans,
                                 int64_t n_spans, int64_t *span_frames, double *span_seconds, int32_t *statuses);
fa_status fa_tdt_speech_gate(fa_ctx *ctx, const fa_tdt_window_config *cfg, const float *audio, const int64_t *audio_offsets,
                             int32_t batch, const float *override_thresholds, float *thresholds, const fa_tdt_span *spans,
                             int64_t n_spans, int64_t *span_frames, double *span_seconds, int32_t *statuses);

/* ------------------------------------------------------------------ online diarizer: the speaker database ------ */
/* SpeakerManager (FluidAudio/Diarizer/Clustering/SpeakerManager.swift:135-212, 282-328, 411-492, 552-628, SpeakerTypes.swift:36-162,
 * 213-217, SpeakerOperations.swift:62-126, VDSPOperations.swift:12-23) as device-resident state, batched over independent streams (one
 * SpeakerManager per stream).  Embeddings are 256 floats (SpeakerManager.embeddingSize); nothing else is accepted.
 *
 * The fp32 arithmetic is this library's DEFINITION — vDSP_dotpr / vDSP_svesq specify no summation order, so Accelerate's bits are out of
 * reach and a decision within an ulp of a threshold may differ from a Mac:
 *   dot256(a, b)  64 lanes, lane l holding dimensions 4l .. 4l+3 with the partial ((a0 b0 + a1 b1) + a2 b2) + a3 b3, every product and sum
 *                 rounded on its own (no FMA); then p[l] = p[l] + p[l ^ off] for off = 32, 16, 8, 4, 2, 1
 *   sumsq(a) = dot256(a, a);  l2Normalize: norm = max(sqrtf(sumsq), 1e-12f), scale = 1 / norm, out = a * scale
 *   cosineDistance: SpeakerOperations.swift:62-101 on those sums (infinity when a sum of squares is <= 0, the unit shortcut within 1e-3
 *                 of 1, the clamp, 1 - s)
 *   the mean of the raw embeddings: per dimension a sequential fp32 sum from the oldest raw to the newest from 0.0f, then / Float(count)
 * Host and kernels share one statement of it (csrc/speaker_db_core.h).
 *
 * Where this library departs from the reference:
 *   ids            int32 counting from 1 per stream, 0 = none; names and non-numeric ids stay with the caller
 *   Date()         a caller-supplied int64 tick per call;  UUID segment ids: dropped
 *   search order   Dictionary iteration is unspecified; here slots in ascending order, a tie on the minimum distance to the lowest slot
 *   a new speaker  goes to the lowest free slot; with none free the item gets kind FULL, id 0, and the state is unchanged (the reference
 *                  is unbounded)
 *   a non-finite embedding  kind INVALID (the reference creates a NaN speaker: NaN never compares below the minimum)
 *   upsert         takes at most raw_capacity raw embeddings (the reference keeps what it is given until the next update)
 * Out of scope: mergeSpeaker, mergeWith and initializeKnownSpeakers(mode: .merge) — they order raw embeddings by wall-clock timestamp,
 * and a caller does them with get + upsert; removeRawEmbedding; names, Codable, SendableSpeaker; the unused
 * SpeakerUtilities.shouldAssignSpeaker heuristics; `confidence`, which assignSpeaker ignores.
 *
 * State per stream and slot (max_speakers slots, 1 .. 64), all in device memory: the current embedding, a ring of raw_capacity raw
 * embeddings (50 is the reference's), duration, update count, created and updated tick, id, live and permanent flags; per stream next_id. */
typedef struct fa_speaker_db fa_speaker_db;
typedef struct {
    float speaker_threshold;       /* 0.65: below it an embedding belongs to the closest speaker */
    float embedding_threshold;     /* 0.45: below it the speaker's embedding is updated as well */
    float min_speech_duration;     /* 1.0 s: shorter speech creates no speaker */
    float ema_alpha;               /* 0.9 (SpeakerManager.swift:452) */
    float validate_min_magnitude;  /* negative: off (plain SpeakerManager); 0.1: DiarizerManager's validateEmbedding before every assignment */
    int32_t max_speakers;          /* slots per stream, 1 .. 64 (default 16) */
    int32_t raw_capacity;          /* raw embeddings kept per speaker (50) */
} fa_speaker_db_config;
/* The path assignSpeaker took for an item. */
enum { FA_SPEAKER_SKIPPED = 0, FA_SPEAKER_UPDATED = 1, FA_SPEAKER_DURATION_ONLY = 2, FA_SPEAKER_LOW_ENERGY = 3, FA_SPEAKER_CREATED = 4,
       FA_SPEAKER_TOO_SHORT = 5, FA_SPEAKER_INVALID = 6, FA_SPEAKER_FULL = 7 };
typedef struct { int32_t id, slot, kind; float distance; } fa_speaker_assignment;   /* id 0 / slot -1: none; distance: to the closest speaker (+inf: none) */
typedef struct { int32_t source_id, destination_id, source_slot, destination_slot; float distance; } fa_speaker_pair;
typedef struct {
    int32_t id, slot, raw_count, update_count, is_permanent;
    float duration;
    int64_t created_tick, updated_tick;
} fa_speaker_info;
/* The arithmetic on its own, on HOST arrays of 256 floats, without a context or a device: VDSPOperations.l2Normalize,
 * SpeakerUtilities.cosineDistance (+inf for a NULL pointer) and validateEmbedding (1: the magnitude is above min_magnitude and every
 * element finite). */
fa_status fa_speaker_l2_normalize(const float *embedding, float *out);
float fa_speaker_cosine_distance(const float *a, const float *b);
int32_t fa_speaker_validate_embedding(const float *embedding, float min_magnitude);
void fa_speaker_db_default_config(fa_speaker_db_config *cfg);
/* INVALID_ARGUMENT, with nothing allocated or launched, for NULL pointers, streams < 1, max_speakers outside 1 .. 64, raw_capacity < 1.
 * The database belongs to the context's device; every later call takes a context of that device and is ordered by that context's stream. */
fa_status fa_speaker_db_create(fa_ctx *ctx, const fa_speaker_db_config *cfg, int32_t streams, fa_speaker_db **out);
void fa_speaker_db_destroy(fa_speaker_db *db);
/* assignSpeaker for `per` items of every stream.  DEVICE pointers: d_embeddings float[streams][per][256] (16-byte aligned), d_durations
 * float[streams][per], d_skip int32[streams][per] (nullable; non-zero: the item is not looked at, id 0, kind SKIPPED),
 * d_out fa_speaker_assignment[streams][per].  Within a stream the items are taken in index order, each seeing the database the previous
 * one left; streams are independent.  Per item:
 *   1. every element finite, and with validate_min_magnitude >= 0 sqrtf(sumsq(e)) > validate_min_magnitude; else INVALID
 *   2. n = l2Normalize(e);  3. the strict minimum d of cosineDistance(n, current[slot]) over the live slots (+inf with none)
 *   4. a slot found and d < speaker_threshold: d < embedding_threshold -> updateMainEmbedding when sumsq(n) > 0.01 (UPDATED), nothing at
 *      all otherwise (LOW_ENERGY); else duration += and the tick (DURATION_ONLY)
 *   5. else duration >= min_speech_duration: a new speaker with id next_id++ (CREATED; FULL without a free slot); 6. else TOO_SHORT
 * updateMainEmbedding: m = l2Normalize(n); raw = l2Normalize(m) (RawEmbedding.init normalises again); raw's own sumsq > 0.01 check; the
 * oldest raw dropped from a full ring, raw appended; current = l2Normalize(mean of raws); current = alpha current + (1 - alpha) m with
 * 1 - alpha in fp32; current = l2Normalize(current); the duration added, the tick set, the update count incremented.
 * One wavefront per stream.  Enqueued on the context's stream; no synchronisation. */
fa_status fa_speaker_db_assign_dev(fa_ctx *ctx, fa_speaker_db *db, const float *d_embeddings, const float *d_durations, const int32_t *d_skip,
                                   int32_t per, int64_t tick, fa_speaker_assignment *d_out);
/* findSpeaker / findMatchingSpeakers: d_dist float[streams][per][max_speakers] the cosine distance of query (stream, i) — NOT normalised,
 * as in the reference — to every slot, +inf on a dead one; d_best_slot int32[streams][per] (nullable) the strict minimum's slot, -1
 * with none.  The `<= threshold` filter and the ascending sort (ties by slot) are the caller's.  DEVICE pointers; no synchronisation. */
fa_status fa_speaker_db_distances_dev(fa_ctx *ctx, fa_speaker_db *db, const float *d_queries, int32_t per, float *d_dist, int32_t *d_best_slot);
/* findMergeablePairs: per stream the pairs i < j of live slots in slot order with distance < threshold, both-permanent pairs left out
 * on request; the lower slot is the destination unless the higher one is permanent (:318-323).  d_pairs [streams][capacity], d_counts
 * int32[streams] the pairs found (records beyond capacity are not written).  DEVICE pointers; no synchronisation. */
fa_status fa_speaker_db_mergeable_pairs_dev(fa_ctx *ctx, fa_speaker_db *db, float threshold, int32_t exclude_if_both_permanent,
                                            fa_speaker_pair *d_pairs, int32_t capacity, int32_t *d_counts);
/* The three above on HOST arrays of the same shapes: copied to the device, run, copied back; one synchronisation.  With fewer than
 * `capacity` pairs in a stream the records behind its count are unspecified. */
fa_status fa_speaker_db_assign(fa_ctx *ctx, fa_speaker_db *db, const float *embeddings, const float *durations, const int32_t *skip, int32_t per,
                               int64_t tick, fa_speaker_assignment *out);
fa_status fa_speaker_db_distances(fa_ctx *ctx, fa_speaker_db *db, const float *queries, int32_t per, float *dist, int32_t *best_slot);
fa_status fa_speaker_db_mergeable_pairs(fa_ctx *ctx, fa_speaker_db *db, float threshold, int32_t exclude_if_both_permanent, fa_speaker_pair *pairs,
                                        int32_t capacity, int32_t *counts);
/* The management entries take HOST pointers, wait for the context's stream and return with their effect complete.
 * upsert (upsertSpeaker :552-606): info->id >= 1; an existing id has its current embedding overwritten WITHOUT normalising, duration,
 * raws, update count and updated tick replaced, permanence only ever set, the created tick kept; a new id goes to the lowest free slot
 * through Speaker.init's l2Normalize, and next_id is raised above it.  raws float[info->raw_count][256], oldest first, stored as they are
 * (RawEmbedding.init's normalisation is the caller's).  OUTPUT_TOO_SMALL with no free slot.  info->slot is ignored. */
fa_status fa_speaker_db_upsert(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, const fa_speaker_info *info, const float *current, const float *raws);
/* getSpeaker: *info (id 0, slot -1 when there is no such speaker), current float[256] (nullable), raws float[raw_rows][256] (nullable)
 * the first min(raw_count, raw_rows) raw embeddings, oldest first. */
fa_status fa_speaker_db_get(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, fa_speaker_info *info, float *current, float *raws,
                            int32_t raw_rows);
/* the stream's ids in slot order: ids int32[max_speakers] */
fa_status fa_speaker_db_ids(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t *ids, int32_t *count);
/* speakerCount of every stream: counts int32[streams] */
fa_status fa_speaker_db_count(fa_ctx *ctx, fa_speaker_db *db, int32_t *counts);
/* removeSpeaker, removeSpeakersInactive(since:) (updated tick < since_tick), makeSpeakerPermanent / revokePermanence, reset (:610-628:
 * next_id becomes 1, or one above the largest id kept).  stream -1 in remove_inactive and reset: every stream. */
fa_status fa_speaker_db_remove(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, int32_t keep_if_permanent);
fa_status fa_speaker_db_remove_inactive(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int64_t since_tick, int32_t keep_if_permanent);
fa_status fa_speaker_db_set_permanent(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t id, int32_t permanent);
fa_status fa_speaker_db_reset(fa_ctx *ctx, fa_speaker_db *db, int32_t stream, int32_t keep_if_permanent);

/* ---- online diarizer: around the networks (DiarizerManager.processChunkWithSpeakerTracking, Diarizer/Core/DiarizerManager.swift:255-531;
 * EmbeddingExtractor.getEmbeddings, Diarizer/Extraction/EmbeddingExtractor.swift:60-199), batched over streams and chunks.  The segmentation
 * and embedding networks stay the caller's; weights float[streams][chunks][frames][3] is what fa_powerset_decode_dev leaves (or soft weights). */
typedef struct {
    int32_t frames;              /* 589 */
    int32_t chunk_samples;       /* 160 000; the constants 80 000 / 160 000 of numMasksInChunk scale as chunk_samples / 2 and chunk_samples */
    float min_active_frames;     /* 10.0 (DiarizerConfig.minActiveFramesCount) */
    float min_speech_duration;   /* 1.0 s (DiarizerConfig.minSpeechDuration): shorter runs give no segment */
    float validate_min_magnitude;/* 0.1: validateEmbedding before the assignment */
    int32_t reserved;
    double frame_step;           /* 0.016875 s (SegmentationProcessor.swift:224-239) */
} fa_online_chunk_config;
typedef struct { int32_t stream, chunk, local_speaker; } fa_online_run;
typedef struct { int32_t stream, chunk, local_speaker, id, start_frame, end_frame; float start, end, quality; } fa_online_segment;
enum { FA_ONLINE_PACK_ZERO_TAIL = 0, FA_ONLINE_PACK_REPEAT = 1 };
void fa_online_chunk_default_config(fa_online_chunk_config *cfg);
/* Before the embedding network.  DEVICE pointers.  d_activities float[streams][chunks][3]: calculateSpeakerActivities, a sequential fp32 sum
 * over the frames.  The clean mask of a speaker is weight * (row sum < 2.0 ? 1 : 0) (:321-333); it runs the model when its sequential sum is
 * not below min_active_frames (EmbeddingExtractor :71-77).  d_runs [run_capacity]: the (stream, chunk, speaker) triples that run, in that
 * order, compacted; d_run_count int32[1] how many there are (beyond run_capacity nothing is written); d_mask_rows float[run_capacity][frames]:
 * per run row[i] = mask[i % numMasksInChunk] with numMasksInChunk = min((frames * samples + chunk_samples / 2) / chunk_samples, frames) in
 * integers, an all-zero row when it is 0 (:63-66, 154-199).  d_samples_in_chunk int32[streams][chunks], NULL: chunk_samples everywhere.
 * _dev does not synchronise; fa_online_chunk_plan is the same with run_count a HOST int32 and one synchronisation.  INVALID_ARGUMENT with
 * nothing launched for NULL pointers, non-positive counts or frames < 1. */
fa_status fa_online_chunk_plan_dev(fa_ctx *ctx, const fa_online_chunk_config *cfg, const float *d_weights, const int32_t *d_samples_in_chunk,
                                   int32_t streams, int32_t chunks, float *d_activities, fa_online_run *d_runs, int32_t run_capacity,
                                   int32_t *d_run_count, float *d_mask_rows);
fa_status fa_online_chunk_plan(fa_ctx *ctx, const fa_online_chunk_config *cfg, const float *d_weights, const int32_t *d_samples_in_chunk,
                               int32_t streams, int32_t chunks, float *d_activities, fa_online_run *d_runs, int32_t run_capacity,
                               int32_t *run_count, float *d_mask_rows);
/* Ragged audio -> d_out float[rows][chunk_samples] (16-byte aligned): row r takes min(d_lengths[r], chunk_samples) samples from
 * d_audio + d_offsets[r]; ZERO_TAIL: zeros behind them (DiarizerManager :266-303); REPEAT: out[i] = in[i % n], what the doubling loop of
 * fillWaveformBuffer (:118-151) leaves; n = 0 leaves zeros.  DEVICE pointers, no synchronisation. */
fa_status fa_online_pack_waveforms_dev(fa_ctx *ctx, const float *d_audio, const int64_t *d_offsets, const int32_t *d_lengths, int32_t rows,
                                       int32_t chunk_samples, int32_t mode, float *d_out);
/* Behind the embedding network: the gate, the assignment into `db` and the timed segments, for db's streams and `chunks` chunks of each; the
 * database carries across the chunks of a stream in order.  d_weights, d_activities (of the plan), d_embeddings float[streams][chunks][3][256]
 * (zeros where no model ran; 16-byte aligned) are DEVICE pointers; chunk_offsets HOST double[streams][chunks] seconds.
 *   gate (:351-378)  activity > min_active_frames, else SKIPPED; then validateEmbedding (INVALID) and assignSpeaker with
 *                    duration = Float(activity) * Float(frame_step); db's thresholds, this config's validate_min_magnitude
 *   segments (:415-531)  speakers with activity < min_active_frames or without an id give none (a speaker exactly at the minimum passes
 *                    here and not the gate: the reference's); per frame the threshold is 0.15 when another speaker exceeds 0.3, else 0.3;
 *                    a run is kept when Float(end - start) >= min_speech_duration with times offset + Double(frame) * frame_step in fp64;
 *                    quality = min(1, sqrtf(sumsq(embedding)) / 10) * (activity / Float(end_frame - start_frame))
 * segments HOST [capacity]: ordered by stream, then chunk, within a chunk by start time (ties: the lower local speaker, then the earlier
 * frame; Swift's sort leaves ties open).  *count: all segments; OUTPUT_TOO_SMALL when it exceeds capacity (the database is updated and
 * count set all the same).  chunk_counts HOST int32[streams][chunks] (nullable).  d_assignments DEVICE fa_speaker_assignment
 * [streams][chunks][3].  One synchronisation. */
fa_status fa_online_chunk_finish_dev(fa_ctx *ctx, const fa_online_chunk_config *cfg, fa_speaker_db *db, const float *d_weights,
                                     const float *d_activities, const float *d_embeddings, const double *chunk_offsets, int32_t chunks,
                                     int64_t tick, fa_online_segment *segments, int64_t capacity, int64_t *count, int32_t *chunk_counts,
                                     fa_speaker_assignment *d_assignments);

/* ------------------------------------------------------------------ streaming Sortformer: FIFO and speaker cache ------ */
/* The state streaming Sortformer carries between chunks (Sources/FluidAudio/Diarizer/Sortformer/SortformerStateUpdater.swift:31-578,
 * driven by SortformerDiarizer.swift:514-578, 933-979 and SortformerTypes.swift:264-385) as device-resident state, batched over streams:
 * the FIFO of recent embeddings, the speaker cache with its compression, the silence profile.  One stream is one
 * SortformerStreamingState; the network stays the caller's and reads the state's slabs in place.
 *
 * Everything behind the base scores is IEEE fp32 add / multiply / divide (unfused) and comparisons, in the reference's order, and equals
 * the reference bit for bit given the same base scores.  The base scores themselves go through logf / log1pf, which no two libraries
 * round alike (the reference's are vForce's): they are the library's own, and fa_sortformer_stream_update_dev hands them out.
 * The library's own definitions beside the reference:
 *   refusals     the reference throws for short preds or a short chunk; here a per-stream status, the stream's state unchanged, the
 *                other streams advanced.  A negative core count, an operand outside its array, and a pred that is NaN or outside
 *                [0, 1] among the rows the update reads are refused as well (the reference traps or carries the NaN into the cache)
 *   max_index    a config whose live permuted indices could reach the sentinel is refused at creation
 *   d_model      a multiple of 4 (16-byte accesses) */
typedef struct fa_sortformer_stream fa_sortformer_stream;
typedef struct {
    int32_t speakers;                 /* 1 .. 4 (4) */
    int32_t d_model;                  /* preEncoderDims (512); a multiple of 4 */
    int32_t chunk_len;                /* 6; clamped to >= 1 */
    int32_t chunk_left_context;       /* 1 */
    int32_t chunk_right_context;      /* 7 */
    int32_t fifo_len;                 /* 40 */
    int32_t spkcache_len;             /* 188; clamped to >= (1 + sil_frames_per_spk) * speakers */
    int32_t spkcache_update_period;   /* 31; clamped to chunk_len .. fifo_len + chunk_len */
    int32_t sil_frames_per_spk;       /* 3 */
    int32_t max_index;                /* 99999: the sentinel of a disabled slot */
    int32_t max_chunk_frames;         /* rows of one chunk's embeddings: chunk_len + both contexts (14) */
    int32_t subsampling;              /* 8 mel frames per model frame */
    int32_t n_mels;                   /* 128 */
    int32_t reserved;
    float silence_threshold;          /* 0.2 */
    float pred_score_threshold;       /* 0.25 */
    float scores_boost_latest;        /* 0.05 */
    float strong_boost_rate;          /* 0.75 */
    float weak_boost_rate;            /* 1.5 */
    float min_pos_scores_rate;        /* 0.5 */
} fa_sortformer_stream_config;
/* SortformerConfig.default (= fastV2 = fastV2_1), balancedV2(_1), highContextV2(_1), efficientV2_1 (SortformerTypes.swift:121-216) */
enum { FA_SORTFORMER_STREAM_PRESET_DEFAULT = 0, FA_SORTFORMER_STREAM_PRESET_BALANCED = 1, FA_SORTFORMER_STREAM_PRESET_HIGH_CONTEXT = 2,
       FA_SORTFORMER_STREAM_PRESET_EFFICIENT = 3 };
/* Per-stream status of an update.  OK: advanced.  INACTIVE: d_active was 0, nothing looked at.  Every other one: refused, state unchanged. */
enum { FA_SORTFORMER_STREAM_OK = 0, FA_SORTFORMER_STREAM_INACTIVE = 1, FA_SORTFORMER_STREAM_SHORT_PREDS_FIFO = 2, FA_SORTFORMER_STREAM_SHORT_CHUNK = 3,
       FA_SORTFORMER_STREAM_SHORT_PREDS_CHUNK = 4, FA_SORTFORMER_STREAM_SHORT_PREDS_TENTATIVE = 5, FA_SORTFORMER_STREAM_NEGATIVE_CORE = 6,
       FA_SORTFORMER_STREAM_BAD_PRED = 7, FA_SORTFORMER_STREAM_BAD_OPERAND = 8 };
typedef struct {   /* what the clamped config comes to */
    int32_t chunk_len, spkcache_len, spkcache_update_period;   /* after the clamps */
    int32_t max_pop;            /* rows one pop can take */
    int32_t score_rows;         /* spkcache_len + max_pop: the row stride of d_log_scores */
    int32_t out_rows;           /* = max_chunk_frames: the row stride of d_confirmed and d_tentative */
    int32_t chunk_mel_frames;   /* (chunk_len + both contexts) * subsampling: the rows of one packed chunk */
    int32_t spkcache_len_per_spk, strong_boost_per_spk, weak_boost_per_spk, min_pos_scores_per_spk;   /* :229-232, Int(Float(x) * rate) */
    int32_t lds_bytes;          /* of the control kernel */
} fa_sortformer_stream_geometry_info;
typedef struct { int32_t spkcache_length, fifo_length, spkcache_preds_present, fifo_preds_present, silence_frame_count, reserved; } fa_sortformer_stream_info;
typedef struct {   /* one chunk of mel frames for the network */
    int32_t ready;              /* 0: not enough frames yet (the other fields 0, new_start_feat = start_feat) */
    int32_t chunk_length;       /* the network's length input */
    int32_t left_offset, right_offset;   /* mel frames of context in the chunk */
    int64_t start_frame;        /* the chunk's first frame in the buffer */
    int64_t rows;               /* frames copied (= chunk_length while streaming) */
    int64_t new_start_feat;     /* startFeat afterwards */
    int64_t frames_to_drop;     /* frames to remove from the buffer's front afterwards */
} fa_sortformer_chunk;
void fa_sortformer_stream_default_config(fa_sortformer_stream_config *cfg);
fa_status fa_sortformer_stream_preset_config(int32_t preset, fa_sortformer_stream_config *cfg);
/* The clamps applied and the derived integers; INVALID_ARGUMENT for a config fa_sortformer_stream_create refuses.  Pure host functions.
 * pop_out_length: min(max(period, context - fifo_len), context) for a context above fifo_len, 0 otherwise, -1 for an unsound config. */
fa_status fa_sortformer_stream_geometry(const fa_sortformer_stream_config *cfg, fa_sortformer_stream_geometry_info *out);
int32_t fa_sortformer_stream_pop_out_length(const fa_sortformer_stream_config *cfg, int32_t context_length);
/* INVALID_ARGUMENT, with nothing allocated or launched, for NULL pointers, streams outside 1 .. 65535, speakers outside 1 .. 4, a d_model
 * that is no multiple of 4, negative lengths, rates outside [0, 1024], a pred_score_threshold outside (0, 1), a config where
 * speakers * (spkcache_len + max_pop + sil_frames_per_spk) reaches max_index, or one whose scored rows exceed the control kernel's LDS.
 * Every stream starts empty (SortformerStreamingState.init).  The state belongs to the context's device. */
fa_status fa_sortformer_stream_create(fa_ctx *ctx, const fa_sortformer_stream_config *cfg, int32_t streams, fa_sortformer_stream **out);
void fa_sortformer_stream_destroy(fa_sortformer_stream *st);
/* What the batched network reads in place: float[streams][spkcache_len][d_model], int32[streams], float[streams][fifo_len][d_model],
 * int32[streams]; rows past a length are zero.  The four DEVICE pointers are fixed for the state's lifetime (a caller may capture its
 * model call in a graph).  Any of the four may be NULL. */
fa_status fa_sortformer_stream_inputs(fa_ctx *ctx, fa_sortformer_stream *st, float **d_spkcache, int32_t **d_spkcache_lengths, float **d_fifo,
                                      int32_t **d_fifo_lengths);
/* One stream's whole state to and from HOST arrays (session restore): spkcache float[spkcache_len][d_model], spkcache_preds
 * float[spkcache_len][speakers], fifo float[fifo_len][d_model], fifo_preds float[fifo_len][speakers], mean_silence float[d_model]; rows past a
 * length are zero, preds that are absent read as zeros.  get: any array may be NULL; waits for the context's stream.  set: takes the rows
 * of the lengths; INVALID_ARGUMENT for lengths outside the slabs, a FIFO with rows but no preds, preds outside [0, 1].  reset =
 * cleanup() for one stream, or for all with stream -1; enqueued on the context's stream. */
fa_status fa_sortformer_stream_get(fa_ctx *ctx, fa_sortformer_stream *st, int32_t stream, fa_sortformer_stream_info *info, float *spkcache,
                                   float *spkcache_preds, float *fifo, float *fifo_preds, float *mean_silence);
fa_status fa_sortformer_stream_set(fa_ctx *ctx, fa_sortformer_stream *st, int32_t stream, const fa_sortformer_stream_info *info, const float *spkcache,
                                   const float *spkcache_preds, const float *fifo, const float *fifo_preds, const float *mean_silence);
fa_status fa_sortformer_stream_reset(fa_ctx *ctx, fa_sortformer_stream *st, int32_t stream);
/* streamingUpdate (:31-165) for every stream in one call.  DEVICE pointers: d_chunk_embs [streams][max_chunk_frames][d_model] (16-byte
 * aligned; emb_dtype FA_DTYPE_F32 or FA_DTYPE_F16, widened on load), d_emb_len int32[streams] the rows of each chunk, d_preds
 * float[streams][pred_stride][speakers] with d_pred_rows int32[streams] valid rows, d_left / d_right int32[streams] the context rows of
 * this chunk, d_active int32[streams] (nullable; 0: the stream is not looked at).  Out: d_confirmed and d_tentative
 * float[streams][max_chunk_frames][speakers], d_counts int32[streams][2] their rows, d_status int32[streams], d_log_scores (nullable)
 * float[streams][score_rows][speakers]: the base scores (getLogPredScores) of the rows a compression scored, the cache's rows first;
 * rows of a stream that did not compress are left untouched.
 *   per stream: validate (FIFO rows, rc >= 0, core = emb_len - lc - rc >= 0, chunk and tentative rows at spkcacheLength + fifoLength + lc,
 *   every pred read in [0, 1]) before the first write; the FIFO's preds replaced from this call's; the core rows appended; if
 *   core + fifoLength > fifo_len: pop min(max(period, context - fifo_len), context) rows, the silence profile over them in frame order
 *   ((mean * n + x) / (n + 1), unfused), the rows appended to the speaker cache, and beyond spkcache_len the first-overflow
 *   initialisation and compressSpkcache (:220-305): base scores, disableLowScores, the latest rows' boost, the strong and the weak boost as
 *   "the first min(k, frames) in the order (score descending, frame ascending)", the +inf placeholder rows, the global selection as "the
 *   first spkcache_len in the order (score descending, permuted index ascending)", then the gather through scratch.
 * Four launches whatever the streams do, nothing allocated, nothing waited for. */
fa_status fa_sortformer_stream_update_dev(fa_ctx *ctx, fa_sortformer_stream *st, const void *d_chunk_embs, int32_t emb_dtype, const int32_t *d_emb_len,
                                          const float *d_preds, int32_t pred_stride, const int32_t *d_pred_rows, const int32_t *d_left, const int32_t *d_right,
                                          const int32_t *d_active, float *d_confirmed, float *d_tentative, int32_t *d_counts, int32_t *d_status,
                                          float *d_log_scores);
/* the same on HOST arrays: staged, run, copied back, one synchronisation; rows past a stream's counts are left untouched */
fa_status fa_sortformer_stream_update(fa_ctx *ctx, fa_sortformer_stream *st, const void *chunk_embs, int32_t emb_dtype, const int32_t *emb_len,
                                      const float *preds, int32_t pred_stride, const int32_t *pred_rows, const int32_t *left, const int32_t *right,
                                      const int32_t *active, float *confirmed, float *tentative, int32_t *counts, int32_t *status, float *log_scores);
/* getNextChunkFeaturesLocked (SortformerDiarizer.swift:933-979) for `streams` buffers of feat_frames[b] mel frames whose next core starts
 * at start_feat[b]: out[streams].  Pure host function. */
fa_status fa_sortformer_stream_chunk_plan(const fa_sortformer_stream_config *cfg, const int64_t *feat_frames, const int64_t *start_feat, int32_t streams,
                                          fa_sortformer_chunk *out);
/* SortformerFeatureLoader (SortformerTypes.swift:347-383) for a file of feat_length frames whose mel is valid up to feat_seq_length: every
 * chunk next() returns, chunk_length clamped by feat_seq_length; *num_chunks (nullable) = max(0, (feat_length - rc) / chunk).  *count is
 * set even when chunks is too small (OUTPUT_TOO_SMALL).  Pure host function. */
fa_status fa_sortformer_stream_file_chunks(const fa_sortformer_stream_config *cfg, int64_t feat_length, int64_t feat_seq_length, fa_sortformer_chunk *chunks,
                                           int64_t capacity, int64_t *count, int64_t *num_chunks);
/* The network's chunk rows: d_rows float[streams][chunk_mel_frames * n_mels], row b the chunk's `rows` frames from start_frame of stream
 * b's frame-major buffer (d_mel + stream_offsets[b] * n_mels floats; stream_offsets and chunks HOST [streams]), copied as bits, zeros
 * behind them; a stream that is not ready gets a row of zeros.  The row copy is the TDT planner's (the records travel in the launches'
 * arguments): no synchronisation. */
fa_status fa_sortformer_stream_pack_chunks_dev(fa_ctx *ctx, const fa_sortformer_stream_config *cfg, const float *d_mel, const int64_t *stream_offsets,
                                               const fa_sortformer_chunk *chunks, int32_t streams, float *d_rows);

/* ------------------------------------------------------------------ Nemotron streaming session: gate, mel cache, blank-span rescue ------ */
/* What a Nemotron streaming session does around its networks and its decode walk (fa_rnnt_greedy_logits_dev), as device-resident state
 * batched over streams: the VAD-gated skip with hangover (StreamingNemotronMultilingualAsrManager+Pipeline.swift:78-104, +Buffers.swift:35-63),
 * the mel cache in front of the encoder's input (+Buffers.swift:140-210) and the blank-span rescue's bookkeeping (+BlankRescue.swift:
 * the span machine :70-119, the closing test :123-164, the padded span audio :243-251, the staged tokens' filter, clamp and merge :264-354).
 * The networks, the rescue decode itself and the tokenizer stay the caller's.  Call order per chunk: gate, mel_inputs, the encoder,
 * fa_rnnt_greedy_logits_dev, advance, track, the rescue decode of the requests, merge_rescued.
 * The library's own definitions beside the reference:
 *   times     every startTime of this path is Double(frame) * 0.08, so the reference's comparisons on seconds are comparisons on the
 *             int32 frames kept here: f >= start - 1 && f <= last + 5, and > for the insert index
 *   RMS       vDSP_rmsqv's summation order is unspecified; the order here is rnnt_stream_core.h's: element i belongs to lane (i / 4) % 64
 *             (of wavefront (i / 256) % 4 for the gate's chunk), a lane adds its squares in ascending i with a fused multiply-add, six
 *             butterfly steps (xor 32, 16, 8, 4, 2, 1), the gate's four wavefront sums added in ascending order, one IEEE divide by n,
 *             one correctly rounded square root; silent = rms < threshold
 *   closures  the closures of one chunk are judged against the live timings of that chunk and merged afterwards (the reference rescues
 *             inside the window loop); equal, because rescued frames are clamped to last + 1 and the next span's test starts at
 *             start' - 1 >= last + 2.  merge_rescued runs before the next chunk's track. */
typedef struct fa_rnnt_stream fa_rnnt_stream;
typedef struct {
    int32_t window_samples;           /* 1280 = one encoder frame; a multiple of 4 in 4 .. 8192 */
    int32_t close_silent_windows;     /* 2; 1 .. 1024 */
    int32_t pre_roll_windows;         /* 3; 0 .. 64 */
    int32_t min_speech_windows;       /* 2; 0 .. 2^20 */
    int32_t max_span_samples;         /* 240000 = 15 s; 1 .. 2^24 */
    int32_t open_slack_frames;        /* 1; 0 .. close_silent_windows - 1 (see closures above) */
    int32_t close_slack_frames;       /* 5; 0 .. 2^20 */
    int32_t vad_hangover_chunks;      /* 2; 1 .. 2^20 */
    int32_t mel_features;             /* 128; 1 .. 4096 */
    int32_t pre_encode_cache;         /* 9; 0 .. 64 */
    int32_t total_mel_frames;         /* the encoder's frame axis: required, pre_encode_cache (at least 1) .. 65536 */
    int32_t reserved;
    float rescue_rms_threshold;       /* 0.0025; 0 disables span tracking; finite, >= 0 */
    float vad_rms_threshold;          /* 0 = the gate is off (the reference's default); in [0, 1) */
} fa_rnnt_stream_config;
/* Per-stream (and per-request) status.  OK: done.  INACTIVE: d_active was 0, nothing looked at.  BAD_OPERAND: a count outside its array
 * or a stream outside the state, nothing written.  OUTPUT_TOO_SMALL: a request without a record or without room in the arena, or a
 * merge beyond the live capacity.  NO_LEXICAL (requests of merge_rescued): the staged tokens held no lexical one, nothing committed. */
enum { FA_RNNT_STREAM_OK = 0, FA_RNNT_STREAM_INACTIVE = 1, FA_RNNT_STREAM_BAD_OPERAND = 2, FA_RNNT_STREAM_OUTPUT_TOO_SMALL = 3, FA_RNNT_STREAM_NO_LEXICAL = 4 };
/* the class byte of a vocabulary id */
enum { FA_RNNT_STREAM_CLASS_LEXICAL = 1, FA_RNNT_STREAM_CLASS_LANG_TAG = 2 };
typedef struct {   /* one stream's scalars (get / set) */
    int32_t frame_cursor;                    /* rescueFrameCursor */
    int32_t span_open, span_start_frame, span_last_speech_frame, span_speech_windows, span_pre_roll_frames, silent_window_run, span_overflowed;
    int32_t span_samples;                    /* rescueSpanAudio.count */
    int32_t pre_roll_samples;                /* rescuePreRollTail.count */
    int32_t vad_consecutive_low_chunks, vad_skip_count, absolute_frame_base;
    int32_t detected_blank_spans, blank_rescues;
    int32_t mel_cache_frames;                /* 0: no cache yet */
} fa_rnnt_stream_info;
typedef struct {   /* one rescue request */
    int32_t stream;
    int32_t span_start_frame;                /* start - preRoll */
    int32_t span_end_frame;                  /* lastSpeech + 1 */
    int32_t speech_windows;
    int32_t audio_samples;                   /* the span's samples */
    int32_t decode_chunks;                   /* ceil(audio_samples / rescue_chunk_samples) + 1 */
    int32_t status;                          /* OK, or OUTPUT_TOO_SMALL: no room in the arena (audio_offset -1) */
    int32_t reserved;
    int64_t audio_offset;                    /* floats into the arena: decode_chunks * rescue_chunk_samples floats, zeros behind the span */
} fa_rnnt_stream_request;
typedef struct {   /* what the config comes to */
    int32_t span_capacity;                   /* floats of one stream's span slab: max_span_samples rounded up to whole windows, plus one window */
    int32_t pre_roll_capacity;               /* floats of one stream's pre-roll ring */
    int32_t mel_cache_capacity;              /* floats of one stream's mel cache: mel_features * pre_encode_cache */
    int32_t reserved;
} fa_rnnt_stream_geometry_info;
void fa_rnnt_stream_default_config(fa_rnnt_stream_config *cfg);   /* the table above; total_mel_frames 0: the caller's */
fa_status fa_rnnt_stream_geometry(const fa_rnnt_stream_config *cfg, fa_rnnt_stream_geometry_info *out);   /* pure host function */
/* The host's emulation of the kernels' RMS order over x[n]: a window's (gate 0: one wavefront) or the gate's chunk (gate 1: four).  Bit-equal
 * to d_rms and to the windows' decisions.  Pure host function. */
fa_status fa_rnnt_stream_rms(const float *x, int64_t n, int32_t gate, float *rms);
/* INVALID_ARGUMENT, with a text that names the bound and nothing allocated, for NULL pointers, streams outside 1 .. 65535 and every
 * field outside the limits above.  Every stream starts as resetStates() leaves it. */
fa_status fa_rnnt_stream_create(fa_ctx *ctx, const fa_rnnt_stream_config *cfg, int32_t streams, fa_rnnt_stream **out);
void fa_rnnt_stream_destroy(fa_rnnt_stream *st);
/* resetRescueState plus the gate's counters, the frame base and the mel cache, for one stream or (stream -1) all; enqueued. */
fa_status fa_rnnt_stream_reset(fa_ctx *ctx, fa_rnnt_stream *st, int32_t stream);
/* One stream's whole state to and from HOST arrays (session restore): span_audio float[span_capacity], pre_roll float[pre_roll_capacity]
 * oldest window first, mel_cache float[mel_features][pre_encode_cache]; the floats past a count are zero.  get: any array may be NULL;
 * waits for the context's stream.  set: INVALID_ARGUMENT for counts outside their slabs or no whole windows, or a missing array. */
fa_status fa_rnnt_stream_get(fa_ctx *ctx, fa_rnnt_stream *st, int32_t stream, fa_rnnt_stream_info *info, float *span_audio, float *pre_roll, float *mel_cache);
fa_status fa_rnnt_stream_set(fa_ctx *ctx, fa_rnnt_stream *st, int32_t stream, const fa_rnnt_stream_info *info, const float *span_audio, const float *pre_roll,
                             const float *mel_cache);
/* The device steps.  DEVICE pointers; every stream in a fixed number of launches, nothing allocated, nothing waited for.  d_active
 * int32[streams] is nullable (0: the stream is not touched, its status INACTIVE).
 * gate (Pipeline.swift:86-104): d_chunks float[streams][chunk_samples] (chunk_samples >= 0; an empty chunk is silent).  Out: d_rms
 * float[streams] (0 while the gate is off), d_skip int32[streams] (1: the chunk skips the encoder; the stream's skip count and frame base
 * have advanced), d_run_list int32[streams] the active streams that run, ascending, with *d_run_count, d_status int32[streams].  2 launches. */
fa_status fa_rnnt_stream_gate_dev(fa_ctx *ctx, fa_rnnt_stream *st, const float *d_chunks, int32_t chunk_samples, const int32_t *d_active, float *d_rms,
                                  int32_t *d_skip, int32_t *d_run_list, int32_t *d_run_count, int32_t *d_status);
/* mel_inputs (prependMelCachePure / extractMelCachePure) for the *d_count (at most max_count) distinct streams of d_streams: d_mel holds
 * element (b, f, t) of the chunk's mel at b * stream_stride + f * row_stride + t * frame_stride floats; d_rows
 * float[max_count][mel_features][total_mel_frames], row k of stream d_streams[k]: its cache, the chunk's first min(chunk_frames,
 * total - pre) frames from column pre on, zeros elsewhere; then the cache becomes the chunk's last min(pre, chunk_frames) frames.
 * d_status int32[max_count] per listed slot.  2 launches. */
fa_status fa_rnnt_stream_mel_inputs_dev(fa_ctx *ctx, fa_rnnt_stream *st, const float *d_mel, int32_t chunk_frames, int64_t stream_stride, int64_t row_stride,
                                        int64_t frame_stride, const int32_t *d_streams, const int32_t *d_count, int32_t max_count, float *d_rows, int32_t *d_status);
/* absoluteFrameBase += the encoder's frames for the listed streams (Pipeline.swift:347, 575): d_frames int32[max_count] per slot, or
 * NULL for `frames` everywhere.  1 launch. */
fa_status fa_rnnt_stream_advance_dev(fa_ctx *ctx, fa_rnnt_stream *st, const int32_t *d_streams, const int32_t *d_count, int32_t max_count, const int32_t *d_frames,
                                     int32_t frames);
/* track (updateRescueSpans + closeSpanAndMaybeRescue's test): the chunk rows of gate, and the live timed tokens d_tok_frame / d_tok_id
 * int32[streams][token_capacity] with d_tok_count int32[streams]; d_class uint8[vocab] (ids outside it have no class).  Walks
 * chunk_samples / window_samples windows, advances the cursor, and leaves one request per closed span that emitted no lexical token:
 * d_requests[request_capacity] in stream order, the span's audio in d_arena float[arena_capacity] (16-byte aligned) padded with zeros to
 * decode_chunks chunks of rescue_chunk_samples (a multiple of 4), *d_request_count = the requests found, whatever fitted.  A request
 * past request_capacity has no record; one whose padded audio ends past arena_capacity has status OUTPUT_TOO_SMALL and no audio; the
 * stream's status is OUTPUT_TOO_SMALL then.  3 launches.  finalize (finalizeRescueSpanIfNeeded) closes the open span of the listed
 * streams the same way, requests in list order, d_status per listed slot. */
fa_status fa_rnnt_stream_track_dev(fa_ctx *ctx, fa_rnnt_stream *st, const float *d_chunks, int32_t chunk_samples, const int32_t *d_active, const int32_t *d_tok_frame,
                                   const int32_t *d_tok_id, const int32_t *d_tok_count, int32_t token_capacity, const uint8_t *d_class, int32_t vocab,
                                   int32_t rescue_chunk_samples, fa_rnnt_stream_request *d_requests, int32_t request_capacity, float *d_arena, int64_t arena_capacity,
                                   int32_t *d_request_count, int32_t *d_status);
fa_status fa_rnnt_stream_finalize_dev(fa_ctx *ctx, fa_rnnt_stream *st, const int32_t *d_streams, const int32_t *d_count, int32_t max_count, const int32_t *d_tok_frame,
                                      const int32_t *d_tok_id, const int32_t *d_tok_count, int32_t token_capacity, const uint8_t *d_class, int32_t vocab,
                                      int32_t rescue_chunk_samples, fa_rnnt_stream_request *d_requests, int32_t request_capacity, float *d_arena, int64_t arena_capacity,
                                      int32_t *d_request_count, int32_t *d_status);
/* merge_rescued (:264-354) for the first min(*d_request_count, request_capacity) requests, in request order within a stream: request r's
 * staged ids d_staged_ids int32[request_capacity][staged_capacity] (d_staged_id_count[r] of them, language tags included) and absolute
 * frames d_staged_frames (d_staged_frame_count[r], one per id that is no tag); the live d_live_ids int32[streams][live_capacity] with
 * d_live_id_count, and the timed d_live_frames / d_live_timed_ids (nullable) int32[streams][live_capacity] with d_live_timed_count.
 * Tags dropped, frames above span_end_frame clamped to it, committed only with a lexical id, inserted in place; the stream's rescued
 * count bumped.  d_request_status int32[request_capacity].  2 launches. */
fa_status fa_rnnt_stream_merge_rescued_dev(fa_ctx *ctx, fa_rnnt_stream *st, const fa_rnnt_stream_request *d_requests, const int32_t *d_request_count,
                                           int32_t request_capacity, const int32_t *d_staged_ids, const int32_t *d_staged_frames, const int32_t *d_staged_id_count,
                                           const int32_t *d_staged_frame_count, int32_t staged_capacity, int32_t *d_live_ids, int32_t *d_live_frames,
                                           int32_t *d_live_timed_ids, int32_t *d_live_id_count, int32_t *d_live_timed_count, int32_t live_capacity,
                                           const uint8_t *d_class, int32_t vocab, int32_t *d_request_status);
/* The same on HOST arrays: staged, run, copied back, one synchronisation.  track: *request_count is what was found; the records and the
 * arena come back whole. */
fa_status fa_rnnt_stream_gate(fa_ctx *ctx, fa_rnnt_stream *st, const float *chunks, int32_t chunk_samples, const int32_t *active, float *rms, int32_t *skip,
                              int32_t *run_list, int32_t *run_count, int32_t *status);
fa_status fa_rnnt_stream_track(fa_ctx *ctx, fa_rnnt_stream *st, const float *chunks, int32_t chunk_samples, const int32_t *active, const int32_t *tok_frame,
                               const int32_t *tok_id, const int32_t *tok_count, int32_t token_capacity, const uint8_t *class_of, int32_t vocab,
                               int32_t rescue_chunk_samples, fa_rnnt_stream_request *requests, int32_t request_capacity, float *arena, int64_t arena_capacity,
                               int32_t *request_count, int32_t *status);
fa_status fa_rnnt_stream_merge_rescued(fa_ctx *ctx, fa_rnnt_stream *st, const fa_rnnt_stream_request *requests, int32_t request_count, const int32_t *staged_ids,
                                       const int32_t *staged_frames, const int32_t *staged_id_count, const int32_t *staged_frame_count, int32_t staged_capacity,
                                       int32_t *live_ids, int32_t *live_frames, int32_t *live_timed_ids, int32_t *live_id_count, int32_t *live_timed_count,
                                       int32_t live_capacity, const uint8_t *class_of, int32_t vocab, int32_t *request_status);

/* ------------------------------------------------------------------ resampling ------ */
/* AudioConverter.linearResample (FluidAudio/Shared/AudioConverter.swift:388-442): planar float[channels][frames] ->
 * mono mix (weight 1/channels) -> linear interpolation to out_rate.  HOST pointers.  Bit-exact restatement. */
int64_t fa_resample_linear_frames(int64_t frames, double in_rate, double out_rate);
fa_status fa_resample_linear(fa_ctx *ctx, const float *planar, int32_t channels, int64_t frames, double in_rate,
                             double out_rate, float *out, int64_t out_capacity, int64_t *out_frames);
/* EXTENSION (parity unpinned: the reference delegates to Apple's closed-source AVAudioConverter, :299-370):
 * rational polyphase FIR resampler, Kaiser(5.0) windowed sinc, half length 10*max(up,down), output length
 * ceil(frames*up/down) — the specification of scipy.signal.resample_poly.  up/down are reduced by their gcd. */
int64_t fa_resample_poly_frames(int64_t frames, int32_t up, int32_t down);
fa_status fa_resample_poly_taps(int32_t up, int32_t down, float *taps, int64_t capacity, int64_t *n_taps, int64_t *pre_remove);
fa_status fa_resample_poly(fa_ctx *ctx, const float *x, int64_t frames, int32_t up, int32_t down, float *out,
                           int64_t out_capacity, int64_t *out_frames);
/* The same on device-resident buffers, enqueued on the context's stream: d_x float[frames] ->
 * d_y float[fa_resample_poly_frames(frames, up, down)].  A context keeps the plan of its last (up, down) pair (taps and
 * tables on the device): the first call of a pair builds it and synchronises the stream, a repeated call does neither. */
fa_status fa_resample_poly_dev(fa_ctx *ctx, const float *d_x, int64_t frames, int32_t up, int32_t down, float *d_y,
                               int64_t out_capacity, int64_t *out_frames);
/* Test hook: which kernel family a fa_resample_poly_dev call with these arguments would take.  It gets or builds the context's plan for the pair
 * exactly as the call would (the first time for a pair: taps and tables go to the device and the stream is synchronised), reads the same
 * FA_RESAMPLE_* switches and launches no kernel; d_x and d_y are looked at as addresses only.  One family serves the interior outputs [lo, hi),
 * the one-thread-per-output kernel the edges [0, lo) and [hi, n_out):
 *   DECIM   integer decimation: LDS tiles on [lo, split), the register-tiled kernel on [split, hi)
 *   INTERP  `count` threads of the register-tiled interpolation kernel from phase cycle `split` on
 *   ROWS    `count` tiles of a row kernel — wide: a persistent one (tile_rows 16 / 32, wide_waves wavefronts), else the 64-row kernel —
 *           with windows of nv 16-byte reads shared by `share` phases, in `groups` phase groups (these six are 0 for the other kinds)
 *   LDS     the LDS-staged kernel on every output;  SIMPLE: nothing but edges (frames == 0 reports SIMPLE and builds no plan)
 * RUNTIME_ERROR without FLUIDAUDIO_HIP_DEBUG_HOOKS=1; INVALID_ARGUMENT for a NULL ctx / out, frames < 0, up < 1 or down < 1. */
enum { FA_RESAMPLE_ROUTE_DECIM = 0, FA_RESAMPLE_ROUTE_INTERP = 1, FA_RESAMPLE_ROUTE_ROWS = 2, FA_RESAMPLE_ROUTE_LDS = 3, FA_RESAMPLE_ROUTE_SIMPLE = 4 };
typedef struct {
    int64_t lo, hi, split, count;
    int32_t kind;
    int32_t wide, tile_rows, wide_waves, nv, share, groups;
} fa_resample_route;
fa_status fa_debug_resample_route(fa_ctx *ctx, const float *d_x, int64_t frames, int32_t up, int32_t down, const float *d_y, fa_resample_route *out);

/* ------------------------------------------------------------------ device set ------ */
/* Multi-GPU for a single-process host (the reference has no multi-device notion; SURVEY §8e: utterances, logit matrices and
 * recordings are independent units, nothing is exchanged).  A pool holds one context per listed device; listing a device
 * twice gives two contexts (two streams) on it.  devices == NULL / n_devices == 0: every visible device.
 *   * fa_pool_acquire blocks until a context is free and hands it to the calling thread; fa_pool_release returns it.
 *     The context-free drop-in symbol fastcluster_compute_centroid_linkage does exactly this on a default pool built from
 *     FLUIDAUDIO_HIP_DEVICES="0,1,.." (default: all devices; FLUIDAUDIO_HIP_DEVICE=<one id> is still honoured), so concurrent
 *     AHCClustering.cluster calls (FluidAudio/Diarizer/Offline/Core/OfflineDiarizerManager.swift:270) run on different GPUs.
 *   * the _sharded / _many entries split ONE host-pointer call across all contexts of the pool (contiguous utterance ranges
 *     balanced by samples; matrices by count; recordings dealt longest-first), one host thread per context, results written
 *     straight into the caller's buffers with the geometry of the unsharded entry; they return the first failure. */
typedef struct fa_pool fa_pool;
fa_status fa_device_count(int32_t *count);
fa_status fa_pool_create(const int32_t *devices, int32_t n_devices, fa_pool **out);
void fa_pool_destroy(fa_pool *pool);
int32_t fa_pool_size(const fa_pool *pool);
fa_ctx *fa_pool_context(fa_pool *pool, int32_t index);   /* the pool keeps ownership */
int32_t fa_ctx_device(const fa_ctx *ctx);
fa_status fa_pool_acquire(fa_pool *pool, fa_ctx **ctx);
void fa_pool_release(fa_pool *pool, fa_ctx *ctx);
fa_status fa_mel_batch_sharded(fa_pool *pool, const fa_mel_config *cfg, const float *pcm, const int64_t *offsets, int32_t batch,
                               const float *last_samples, const int32_t *expected_frames, int32_t frame_stride, float *mel,
                               int32_t *mel_lengths);
fa_status fa_ctc_greedy_batch_sharded(fa_pool *pool, const void *logits, int32_t dtype, int32_t batch, int32_t frames, int32_t vocab,
                                      int64_t row_stride, int64_t matrix_stride, const int32_t *valid_frames, int32_t blank_id,
                                      int32_t *frame_ids, int32_t *token_ids, int32_t *token_lens);
/* recordings across devices, and on each device advanced together by fa_ahc_linkage_batch; HOST pointers */
fa_status fa_ahc_linkage_many(fa_pool *pool, int32_t count, const double *const *data, const size_t *n, size_t d,
                              double *const *dendrograms, int32_t mode, fa_ahc_stats *stats, int32_t *statuses);

#ifdef __cplusplus
}
#endif
#endif /* FLUIDAUDIO_HIP_H */
