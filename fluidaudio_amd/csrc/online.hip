// online.hip — the kernels of the online diarizer.  Second half of the file: chunk planning, waveform packing and timed segments around
// the networks (DiarizerManager.swift:255-531), lane = frame.  First half: the speaker database (SpeakerManager.assignSpeaker / findSpeaker / findMergeablePairs,
// Diarizer/Clustering/SpeakerManager.swift:135-212, 282-328, 411-492), batched over streams.  One wavefront per stream: lane l holds the
// dimensions 4l .. 4l+3 of every 256-vector (one 16-byte load per lane, 1 KiB coalesced per row), a dot product is the lane's partial and
// six butterfly steps — the definition of speaker_db_core.h, which also holds the algorithm itself; this unit supplies the lane vector.
// Items of a stream are taken in index order by the stream's wavefront; streams are independent.  No atomics.  Built with
// -ffp-contract=off: the definition needs every product and sum rounded on its own.
#include "online_launch.h"
#include "block_scan.h"

namespace fa {
namespace online {

namespace {

struct LaneVec {
    float x, y, z, w;
    static __device__ LaneVec load(const float *p) {
        const float4 v = reinterpret_cast<const float4 *>(p)[threadIdx.x & (kWave - 1)];
        return LaneVec{v.x, v.y, v.z, v.w};
    }
    __device__ void store(float *p) const { reinterpret_cast<float4 *>(p)[threadIdx.x & (kWave - 1)] = make_float4(x, y, z, w); }
    static __device__ LaneVec zero() { return LaneVec{0.0f, 0.0f, 0.0f, 0.0f}; }
    static __device__ float dot(const LaneVec &a, const LaneVec &b) {
        float p = spk::partial4(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off);
        return p;
    }
    __device__ LaneVec scaled(const float s) const { return LaneVec{x * s, y * s, z * s, w * s}; }
    __device__ LaneVec plus(const LaneVec &o) const { return LaneVec{x + o.x, y + o.y, z + o.z, w + o.w}; }
    __device__ LaneVec over(const float d) const { return LaneVec{x / d, y / d, z / d, w / d}; }
    static __device__ LaneVec blend(const float a, const LaneVec &p, const float b, const LaneVec &q) {
        return LaneVec{a * p.x + b * q.x, a * p.y + b * q.y, a * p.z + b * q.z, a * p.w + b * q.w};
    }
    __device__ bool finite() const { return __all(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(w)) != 0; }
};

__device__ spk::View view_of(const DbArrays &db, const int stream) {
    spk::View v;
    v.current = db.current + static_cast<int64_t>(stream) * db.S * spk::kDim;
    v.raws = db.raws + static_cast<int64_t>(stream) * db.S * db.R * spk::kDim;
    v.meta = db.meta + static_cast<int64_t>(stream) * db.S;
    v.next_id = db.next_id + stream;
    v.S = db.S; v.R = db.R;
    v.live = spk::live_mask(v.meta, v.S);
    return v;
}

__device__ int wave_index() { return blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); }

__global__ __launch_bounds__(kWave * kWavesPerBlock) void assign_kernel(const AssignArgs a) {
    const int stream = wave_index(), lane = threadIdx.x & (kWave - 1);
    if (stream >= a.db.streams) return;
    spk::View db = view_of(a.db, stream);
    for (int i = 0; i < a.per; ++i) {
        const int64_t item = static_cast<int64_t>(stream) * a.per + i;
        spk::Record rec{0, -1, spk::kSkipped, spk::inf32()};
        if (!(a.skip && a.skip[item] != 0))
            rec = spk::assign_one<LaneVec>(db, a.p, LaneVec::load(a.embeddings + item * spk::kDim), a.durations[item], a.tick);
        if (lane == 0) a.out[item] = rec;
    }
}

// findClosestSpeaker on queries as they are (findSpeaker does not normalise): every slot's distance, +inf on a dead one
__global__ __launch_bounds__(kWave * kWavesPerBlock) void distances_kernel(const DistanceArgs a) {
    const int64_t item = wave_index();
    const int lane = threadIdx.x & (kWave - 1);
    if (item >= static_cast<int64_t>(a.db.streams) * a.per) return;
    const spk::View db = view_of(a.db, static_cast<int>(item / a.per));
    const LaneVec q = LaneVec::load(a.queries + item * spk::kDim);
    const float ssq = spk::sumsq(q);
    float best = spk::inf32();
    int at = -1;
    for (int s = 0; s < db.S; ++s) {
        float d = spk::inf32();
        if (db.live >> s & 1) {
            const LaneVec c = LaneVec::load(db.cur(s));
            d = spk::cosine_from_sums(LaneVec::dot(q, c), ssq, spk::sumsq(c));
        }
        if (d < best) { best = d; at = s; }
        if (lane == 0) a.dist[item * db.S + s] = d;
    }
    if (lane == 0 && a.best_slot) a.best_slot[item] = at;
}

// findMergeablePairs (:282-328) with the slots in ascending order for the dictionary's keys; the stream's wavefront walks the pairs in
// order, so its records are compact and ordered as they are written
__global__ __launch_bounds__(kWave * kWavesPerBlock) void pairs_kernel(const PairArgs a) {
    const int stream = wave_index(), lane = threadIdx.x & (kWave - 1);
    if (stream >= a.db.streams) return;
    const spk::View db = view_of(a.db, stream);
    int n = 0;
    for (uint64_t li = db.live; li; li &= li - 1) {
        const int i = __builtin_ctzll(li);
        const LaneVec ci = LaneVec::load(db.cur(i));
        const float ssi = spk::sumsq(ci);
        const bool pi = (db.meta[i].flags & spk::kPermanent) != 0;
        for (uint64_t lj = li & (li - 1); lj; lj &= lj - 1) {
            const int j = __builtin_ctzll(lj);
            const bool pj = (db.meta[j].flags & spk::kPermanent) != 0;
            if (a.exclude_if_both_permanent && pi && pj) continue;
            const LaneVec cj = LaneVec::load(db.cur(j));
            const float d = spk::cosine_from_sums(LaneVec::dot(ci, cj), ssi, spk::sumsq(cj));
            if (!(d < a.threshold)) continue;
            if (lane == 0 && n < a.capacity) {
                const int src = pj ? i : j, dst = pj ? j : i;   // :318-323: speaker1 is the destination unless speaker2 is permanent
                a.pairs[static_cast<int64_t>(stream) * a.capacity + n] = fa_speaker_pair{db.meta[src].id, db.meta[dst].id, src, dst, d};
            }
            ++n;
        }
    }
    if (lane == 0) a.counts[stream] = n;
}


// ======== around the networks.  Lane = frame: a wavefront takes 64 frames of a chunk at a time.

// One wavefront per (stream, chunk): calculateSpeakerActivities (:400-412) and the clean masks' sums (:321-333, EmbeddingExtractor :71),
// both sequential fp32 sums over the frames — the 64 values of a block are added in frame order through cross-lane reads.
__global__ __launch_bounds__(kWave * kWavesPerBlock) void plan_sums_kernel(const PlanArgs a) {
    const int64_t sc = wave_index();
    const int lane = threadIdx.x & (kWave - 1);
    if (sc >= static_cast<int64_t>(a.streams) * a.chunks) return;
    const float *w = a.weights + sc * a.frames * 3;
    float act[3] = {0.0f, 0.0f, 0.0f}, clean[3] = {0.0f, 0.0f, 0.0f};
    for (int f0 = 0; f0 < a.frames; f0 += kWave) {
        const int f = f0 + lane;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (f < a.frames) { v[0] = w[f * 3]; v[1] = w[f * 3 + 1]; v[2] = w[f * 3 + 2]; }
        const float is_clean = ((0.0f + v[0]) + v[1]) + v[2] < 2.0f ? 1.0f : 0.0f;
        const int n = a.frames - f0 < kWave ? a.frames - f0 : kWave;
        for (int l = 0; l < n; ++l)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                act[s] = act[s] + __shfl(v[s], l);
                clean[s] = clean[s] + __shfl(v[s] * is_clean, l);
            }
    }
    if (lane < 3) {
        const float mine = lane == 0 ? act[0] : lane == 1 ? act[1] : act[2], mine_clean = lane == 0 ? clean[0] : lane == 1 ? clean[1] : clean[2];
        a.activities[sc * 3 + lane] = mine;
        a.flags[sc * 3 + lane] = !(mine_clean < a.min_active_frames) ? 1 : 0;   // EmbeddingExtractor :73: inactive when the sum is below the minimum
    }
}

// One workgroup: block_scan.h's workgroup_exclusive over the flags in triple order, the run list and its count.
__global__ __launch_bounds__(fa::scan::kThreads) void plan_scan_kernel(const PlanArgs a) {
    const int64_t n = static_cast<int64_t>(a.streams) * a.chunks * 3;
    const int count = fa::scan::workgroup_exclusive(n, [&](const int64_t i) { return a.flags[i]; }, [&](const int64_t i, const int keep, const int at) {
        a.flags[i] = keep ? at : -1;
        if (keep && at < a.run_capacity) a.runs[at] = fa_online_run{static_cast<int32_t>(i / 3 / a.chunks), static_cast<int32_t>(i / 3 % a.chunks), static_cast<int32_t>(i % 3)};
    });
    if (threadIdx.x == 0) *a.run_count = count;
}

// One workgroup per (stream, chunk, speaker) that runs: its model mask row with the repeat padding of fillMaskBufferOptimized (:154-199)
__global__ __launch_bounds__(256) void plan_rows_kernel(const PlanArgs a) {
    const int64_t t = blockIdx.x;
    const int at = a.flags[t];
    if (at < 0 || at >= a.run_capacity) return;
    const int64_t sc = t / 3;
    const int s = static_cast<int>(t % 3);
    const float *w = a.weights + sc * a.frames * 3;
    const int64_t samples = a.samples ? a.samples[sc] : a.chunk_samples;
    int64_t n = (static_cast<int64_t>(a.frames) * samples + a.chunk_samples / 2) / a.chunk_samples;   // numMasksInChunk (:63-66)
    if (n > a.frames) n = a.frames;
    float *row = a.mask_rows + static_cast<int64_t>(at) * a.frames;
    for (int i = threadIdx.x; i < a.frames; i += blockDim.x) {
        float v = 0.0f;
        if (n > 0) {
            const int f = static_cast<int>(i % n);
            v = w[f * 3 + s] * (((0.0f + w[f * 3]) + w[f * 3 + 1]) + w[f * 3 + 2] < 2.0f ? 1.0f : 0.0f);
        }
        row[i] = v;
    }
}

// Ragged audio -> [rows][chunk_samples]: the zero tail of DiarizerManager :266-303, or out[i] = in[i % n], which is what the doubling loop of
// fillWaveformBuffer (:118-151) leaves.  A thread writes four samples with one 16-byte store where the row allows it.
__global__ __launch_bounds__(256) void pack_kernel(const PackArgs a) {
    const int row = blockIdx.y;
    const float *in = a.audio + a.offsets[row];
    const int64_t n = a.lengths[row] < a.chunk_samples ? a.lengths[row] : a.chunk_samples;
    float *out = a.out + static_cast<int64_t>(row) * a.chunk_samples;
    const int64_t i0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) * 4;
    if (i0 >= a.chunk_samples) return;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k;
        v[k] = n <= 0 ? 0.0f : i < n ? in[i] : a.repeat ? in[i % n] : 0.0f;
    }
    if ((a.chunk_samples & 3) == 0) {
        reinterpret_cast<float4 *>(out + i0)[0] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < 4 && i0 + k < a.chunk_samples; ++k) out[i0 + k] = v[k];
    }
}

// The gate and the assignment (:351-378): one wavefront per stream, its chunks and their three local speakers in order.
__global__ __launch_bounds__(kWave * kWavesPerBlock) void finish_assign_kernel(const FinishArgs a) {
    const int stream = wave_index(), lane = threadIdx.x & (kWave - 1);
    if (stream >= a.db.streams) return;
    spk::View db = view_of(a.db, stream);
    for (int c = 0; c < a.chunks; ++c)
        for (int s = 0; s < 3; ++s) {
            const int64_t item = (static_cast<int64_t>(stream) * a.chunks + c) * 3 + s;
            const float activity = a.activities[item];
            spk::Record rec{0, -1, spk::kSkipped, spk::inf32()};
            if (activity > a.min_active_frames)
                rec = spk::assign_one<LaneVec>(db, a.p, LaneVec::load(a.embeddings + item * spk::kDim), activity * static_cast<float>(a.frame_step), a.tick);
            if (lane == 0) a.assignments[item] = rec;
        }
}

// createTimedSegments (:415-531) for one (stream, chunk) in its wavefront: per local speaker the predicate of 64 frames is one ballot, and the
// runs are read off the ballots (a run open at the last frame ends at `frames`).  emit(speaker, start, end) is called in speaker order, runs
// ascending, for the runs createSegmentIfValid keeps.
template <class Emit> __device__ void walk_segments(const FinishArgs &a, const int64_t sc, Emit &&emit) {
    const int lane = threadIdx.x & (kWave - 1);
    const float *w = a.weights + sc * a.frames * 3;
    const double offset = a.offsets[sc];
    for (int s = 0; s < 3; ++s) {
        if (a.activities[sc * 3 + s] < a.min_active_frames) continue;
        if (a.assignments[sc * 3 + s].id == 0) continue;             // speakerIds[speakerIndex].isEmpty: no run of it is kept
        int open = -1;                                                // the start frame of the run that is open
        for (int f0 = 0; f0 <= a.frames; f0 += kWave) {              // one block past the end closes the last run when frames is a multiple of 64
            const int f = f0 + lane;
            bool active = false;
            if (f < a.frames) {
                const float v0 = w[f * 3], v1 = w[f * 3 + 1], v2 = w[f * 3 + 2];
                const float mine = s == 0 ? v0 : s == 1 ? v1 : v2;
                const bool other = (s != 0 && v0 > 0.3f) || (s != 1 && v1 > 0.3f) || (s != 2 && v2 > 0.3f);
                active = mine > (other ? 0.15f : 0.3f);
            }
            const uint64_t m = __ballot(active);
            const uint64_t prev = (m << 1) | (open >= 0 ? 1ull : 0ull);
            uint64_t edges = m ^ prev;                                // a bit where the state changes at that frame
            while (edges) {
                const int b = __builtin_ctzll(edges);
                edges &= edges - 1;
                if (open < 0) { open = f0 + b; continue; }
                const int start = open, end = f0 + b;
                open = -1;
                const double t0 = offset + static_cast<double>(start) * a.frame_step, t1 = offset + static_cast<double>(end) * a.frame_step;
                if (static_cast<float>(t1 - t0) < a.min_speech_duration) continue;
                emit(s, start, end, t0, t1);
            }
        }
    }
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void finish_count_kernel(const FinishArgs a) {
    const int64_t sc = wave_index();
    if (sc >= static_cast<int64_t>(a.db.streams) * a.chunks) return;
    int n = 0;
    walk_segments(a, sc, [&](int, int, int, double, double) { ++n; });
    if ((threadIdx.x & (kWave - 1)) == 0) a.counts[sc] = n;
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void finish_write_kernel(const FinishArgs a) {
    const int64_t sc = wave_index();
    const int lane = threadIdx.x & (kWave - 1);
    if (sc >= static_cast<int64_t>(a.db.streams) * a.chunks) return;
    const int64_t first = a.counts[sc];
    int n = 0;
    float quality_scale[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {                                     // calculateEmbeddingQuality (:528-531)
        const float magnitude = sqrtf(spk::sumsq(LaneVec::load(a.embeddings + (sc * 3 + s) * spk::kDim))) / 10.0f;
        quality_scale[s] = magnitude < 1.0f ? magnitude : 1.0f;
    }
    walk_segments(a, sc, [&](const int s, const int start, const int end, const double t0, const double t1) {
        const int64_t at = first + n++;
        if (lane != 0 || at >= a.capacity) return;
        const float scale = s == 0 ? quality_scale[0] : s == 1 ? quality_scale[1] : quality_scale[2];
        fa_online_segment r;
        r.stream = static_cast<int32_t>(sc / a.chunks); r.chunk = static_cast<int32_t>(sc % a.chunks); r.local_speaker = s;
        r.id = a.assignments[sc * 3 + s].id; r.start_frame = start; r.end_frame = end;
        r.start = static_cast<float>(t0); r.end = static_cast<float>(t1);
        r.quality = scale * (a.activities[sc * 3 + s] / static_cast<float>(end - start));
        // segments.sort by start time: the records arrive in speaker order, each speaker's ascending; insert behind every record that does
        // not start later (ties: the lower local speaker, then the earlier frame, stay in front)
        int64_t j = at;
        while (j > first && a.segments[j - 1].start > r.start) { a.segments[j] = a.segments[j - 1]; --j; }
        a.segments[j] = r;
    });
}

}  // namespace

void launch_plan(hipStream_t stream, const PlanArgs &a) {
    const int64_t sc = static_cast<int64_t>(a.streams) * a.chunks;
    const Plan pl = plan_of(sc);
    hipLaunchKernelGGL(plan_sums_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, a);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(fa::scan::kThreads), 0, stream, a);
    hipLaunchKernelGGL(plan_rows_kernel, dim3(static_cast<unsigned>(sc * 3)), dim3(256), 0, stream, a);
}
void launch_pack(hipStream_t stream, const PackArgs &a) {
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for((a.chunk_samples + 3) / 4, 256), static_cast<unsigned>(a.rows)), dim3(256), 0, stream, a);
}
void launch_finish(hipStream_t stream, const FinishArgs &a) {
    const int64_t n = static_cast<int64_t>(a.db.streams) * a.chunks;
    const Plan per_stream = plan_of(a.db.streams), per_chunk = plan_of(n);
    hipLaunchKernelGGL(finish_assign_kernel, dim3(per_stream.grid), dim3(per_stream.block), 0, stream, a);
    hipLaunchKernelGGL(finish_count_kernel, dim3(per_chunk.grid), dim3(per_chunk.block), 0, stream, a);
    hipLaunchKernelGGL(fa::scan::scan_totals<>, dim3(1), dim3(fa::scan::kThreads), 0, stream, a.counts, n, a.counts + n);   // the chunks' counts -> offsets, counts[n] the total
    hipLaunchKernelGGL(finish_write_kernel, dim3(per_chunk.grid), dim3(per_chunk.block), 0, stream, a);
}

void launch_assign(hipStream_t stream, const AssignArgs &a) {
    const Plan pl = plan_of(a.db.streams);
    hipLaunchKernelGGL(assign_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, a);
}
void launch_distances(hipStream_t stream, const DistanceArgs &a) {
    const Plan pl = plan_of(static_cast<int64_t>(a.db.streams) * a.per);
    hipLaunchKernelGGL(distances_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, a);
}
void launch_pairs(hipStream_t stream, const PairArgs &a) {
    const Plan pl = plan_of(a.db.streams);
    hipLaunchKernelGGL(pairs_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, a);
}

}  // namespace online
}  // namespace fa
