// online_launch.h — what the online diarizer's two host units (speaker_db_host.hip: the speaker database's handle and entries;
// online_host.hip: the entries around the networks) and its kernel unit (online.hip) share: the database's device arrays, the operands
// of each kernel, the launch plans and the launchers, and at the end the handle itself with the two checks both host units make.  The
// arithmetic, the per-slot layout and the management edits: speaker_db_core.h.  Internal; not part of the C ABI.  Launch errors
// surface through hipGetLastError().
#pragma once
#include "fa_common.h"
#include "speaker_db_core.h"

namespace fa {
namespace online {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;   // one wavefront per stream (or per query); four of them share a workgroup

// The whole database on the device, per stream and per slot.
struct DbArrays {
    float *current;            // [streams][S][256]
    float *raws;               // [streams][S][R][256]
    spk::SlotMeta *meta;       // [streams][S]
    int32_t *next_id;          // [streams]
    int32_t streams, S, R;
};

struct AssignArgs {
    DbArrays db;
    spk::Params p;
    const float *embeddings;   // [streams][per][256]
    const float *durations;    // [streams][per]
    const int32_t *skip;       // [streams][per] or null
    int32_t per;
    int64_t tick;
    spk::Record *out;          // [streams][per]
};

struct DistanceArgs {
    DbArrays db;
    const float *queries;      // [streams][per][256]
    int32_t per;
    float *dist;               // [streams][per][S]
    int32_t *best_slot;        // [streams][per] or null
};

struct PairArgs {
    DbArrays db;
    float threshold;
    int32_t exclude_if_both_permanent;
    fa_speaker_pair *pairs;    // [streams][capacity]
    int32_t capacity;
    int32_t *counts;           // [streams]
};

struct Plan {
    unsigned grid, block;
};
// waves: the wavefronts the kernel needs, one per stream or per (stream, query)
inline Plan plan_of(const int64_t waves) { return Plan{grid_for(waves, kWavesPerBlock), static_cast<unsigned>(kWave * kWavesPerBlock)}; }

// ---- around the networks (DiarizerManager.processChunkWithSpeakerTracking :255-531, EmbeddingExtractor :60-199)
struct PlanArgs {
    const float *weights;          // [streams][chunks][frames][3]
    const int32_t *samples;        // [streams][chunks] or null (chunk_samples)
    int32_t streams, chunks, frames, chunk_samples;
    float min_active_frames;
    float *activities;             // [streams][chunks][3]
    int32_t *flags;                // [streams * chunks * 3 + 1] scratch: 1 where the speaker runs the model, then its exclusive prefix
    fa_online_run *runs;           // [run_capacity]
    int32_t run_capacity;
    int32_t *run_count;            // [1]
    float *mask_rows;              // [run_capacity][frames]
};
struct PackArgs {
    const float *audio;
    const int64_t *offsets;        // [rows]
    const int32_t *lengths;        // [rows]
    int32_t rows, chunk_samples, repeat;
    float *out;                    // [rows][chunk_samples]
};
struct FinishArgs {
    DbArrays db;
    spk::Params p;
    const float *weights, *activities, *embeddings;   // [streams][chunks][frames][3], [..][3], [..][3][256]
    const double *offsets;         // [streams][chunks]
    int32_t chunks, frames;
    float min_active_frames, min_speech_duration;
    double frame_step;
    int64_t tick;
    spk::Record *assignments;      // [streams][chunks][3]
    int32_t *counts;               // [streams * chunks + 1] scratch: the segments of every chunk, then their exclusive prefix; the last: the total
    fa_online_segment *segments;   // [capacity]
    int64_t capacity;
};
void launch_plan(hipStream_t stream, const PlanArgs &a);
void launch_pack(hipStream_t stream, const PackArgs &a);
void launch_finish(hipStream_t stream, const FinishArgs &a);

void launch_assign(hipStream_t stream, const AssignArgs &a);
void launch_distances(hipStream_t stream, const DistanceArgs &a);
void launch_pairs(hipStream_t stream, const PairArgs &a);

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace online
}  // namespace fa

struct fa_speaker_db {
    int device = 0;
    fa::spk::Params p{};
    int32_t streams = 0;
    fa::DevBuf current, raws, meta, next_id;
    fa::online::DbArrays arrays() const {
        return fa::online::DbArrays{current.as<float>(), raws.as<float>(), meta.as<fa::spk::SlotMeta>(), next_id.as<int32_t>(), streams, p.max_speakers, p.raw_capacity};
    }
};

namespace fa {
namespace online {

inline fa_status check_db(fa_ctx *ctx, const fa_speaker_db *db, const char *what) {
    if (!ctx || !db) return FA_INVALID_ARGUMENT;
    if (db->device != ctx->device) return fa::set_error(ctx, FA_INVALID_ARGUMENT, "%s: the database lives on another device than the context", what);
    return FA_SUCCESS;
}

}  // namespace online
}  // namespace fa
