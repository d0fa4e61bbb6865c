// rnnt_stream_launch.h — what the host side of the Nemotron streaming session (rnnt_stream_host.hip: the handle, the argument checks, the
// C ABI) and its kernel unit (rnnt_stream.hip) share: the state's device arrays, the operands of every step, the launch plan and the
// launchers.  The integers and the RMS order: rnnt_stream_core.h.  Internal; not part of the C ABI.  Launch errors surface through
// hipGetLastError().
#pragma once
#include "fa_common.h"
#include "rnnt_stream_core.h"

namespace fa {
namespace rns {

constexpr int kGateBlock = kGateWaves * kLanes;   // one workgroup per stream
constexpr int kWaveBlock = kLanes;                // track, mel_inputs, merge: one wavefront per stream (and mel row)
constexpr int kListBlock = 256;                   // advance, the mel cache's frame count: one thread per listed slot

// The whole state on the device, per stream.
struct StateArrays {
    int32_t *scalars;   // [B][kScalars]
    float *span;        // [B][span_capacity]
    float *ring;        // [B][pre_roll_capacity]: window slots, the oldest at kPreHead
    float *mel_cache;   // [B][mel_features][pre_encode_cache]
    // the library's scratch of one track / finalize
    uint64_t *silent;   // [B][words]: bit w of word w / 64: window w is silent
    uint64_t *wanted;   // [B][words]: the span closing at window w asks for a rescue (finalize: bit 0)
    int32_t *found;     // [B + 1]: requests per slot, scanned in place; [B] their sum
    int64_t *floats;    // [B + 1]: padded floats per slot, scanned in place
    int32_t words;      // words per stream of silent / wanted
    int32_t B;
};

struct GateArgs {
    StateArrays st; Config c;
    const float *chunks; int32_t chunk_samples; const int32_t *active;
    float *rms; int32_t *skip, *run_list, *run_count, *status;
};
struct MelArgs {
    StateArrays st; Config c;
    const float *mel; int32_t chunk_frames; int64_t stream_stride, row_stride, frame_stride;
    const int32_t *streams, *count; int32_t max_count;
    float *rows; int32_t *status;
};
struct AdvanceArgs { StateArrays st; const int32_t *streams, *count; int32_t max_count; const int32_t *d_frames; int32_t frames; };
struct TrackArgs {
    StateArrays st; Config c;
    const float *chunks; int32_t chunk_samples;     // finalize: null, 0
    const int32_t *active;                          // track
    const int32_t *streams, *count; int32_t slots;  // finalize: the list; track: null, null, B
    int32_t finalize;
    const int32_t *tok_frame, *tok_id, *tok_count; int32_t token_capacity;
    const uint8_t *class_of; int32_t vocab;
    int32_t rescue_chunk_samples;
    fa_rnnt_stream_request *requests; int32_t request_capacity;
    float *arena; int64_t arena_capacity;
    int32_t *request_count, *status;
};
struct MergeArgs {
    StateArrays st;
    const fa_rnnt_stream_request *requests; const int32_t *request_count; int32_t request_capacity;
    const int32_t *staged_ids, *staged_frames, *staged_id_count, *staged_frame_count; int32_t staged_capacity;
    int32_t *live_ids, *live_frames, *live_timed_ids, *live_id_count, *live_timed_count; int32_t live_capacity;
    const uint8_t *class_of; int32_t vocab;
    int32_t *request_status;
};

// windows of one chunk, and the words of their ballot
inline int32_t windows_of(const Config &c, const int32_t chunk_samples) { return chunk_samples / c.window_samples; }
constexpr int32_t kMaxWords = 16;   // 1 024 windows a chunk: 82 s of 80 ms windows

void launch_gate(hipStream_t stream, const GateArgs &a);        // rms + decision, the run list: 2 launches
void launch_mel(hipStream_t stream, const MelArgs &a);          // rows, the frame counts: 2 launches
void launch_advance(hipStream_t stream, const AdvanceArgs &a);  // 1 launch
void launch_track(hipStream_t stream, const TrackArgs &a);      // decide, place, copy: 3 launches
void launch_merge(hipStream_t stream, const MergeArgs &a);      // 1 launch

}  // namespace rns
}  // namespace fa
