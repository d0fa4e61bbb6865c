"""A line-by-line numpy-float32 restatement of the reference's online speaker database — SpeakerManager (Diarizer/Clustering/
SpeakerManager.swift:45-125, 135-212, 282-328, 334-367, 411-492, 552-628), Speaker / RawEmbedding (SpeakerTypes.swift:36-55, 68-162,
213-217), SpeakerUtilities.cosineDistance / validateEmbedding (SpeakerOperations.swift:62-126) and VDSPOperations.l2Normalize
(Offline/Utils/VDSPOperations.swift:12-23) — parametrised by the dot product, which the reference leaves to Accelerate.  `dot256` is the
library's definition (include/fluidaudio_hip.h); `dot64` is a float64 sequential sum, a second opinion.

Where the library departs from the reference (integer ids, a tick for Date(), slots searched in ascending order with ties to the lowest,
a bounded number of slots, INVALID for a non-finite embedding) the restatement follows the library when `max_speakers` is given, and is
the plain reference when it is None.  BRANCHES counts the paths taken, for the tests' coverage conditions."""
import collections

import numpy as np

F = np.float32
INF = F(np.inf)
DIM = 256
KINDS = ("SKIPPED", "UPDATED", "DURATION_ONLY", "LOW_ENERGY", "CREATED", "TOO_SHORT", "INVALID", "FULL")
BRANCH_NAMES = KINDS + ("ring_wrap", "cosine_non_unit", "cosine_infinite", "tie")
BRANCHES = collections.Counter()
_LANES = np.arange(64)


def dot256_lanes(a, b):
    """Every lane's result of the library's dot product: lane l holds dimensions 4l .. 4l+3."""
    p = (np.asarray(a, F) * np.asarray(b, F)).reshape(64, 4)
    s = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[_LANES ^ off]
    return s


def dot256(a, b):
    return dot256_lanes(a, b)[0]


def dot64(a, b):
    return F(np.cumsum(np.asarray(a, np.float64) * np.asarray(b, np.float64))[-1])


def swift_max(x, y):
    return y if y >= x else x


def swift_min(x, y):
    return y if y < x else x


class Arith:
    def __init__(self, dot=dot256):
        self.dot = dot

    def sumsq(self, a):                                   # vDSP_svesq
        return self.dot(a, a)

    def l2_normalize(self, a):                            # VDSPOperations.swift:12-23
        a = np.asarray(a, F)
        norm = swift_max(np.sqrt(self.sumsq(a)), F(1e-12))
        scale = F(1) / norm
        return a * scale

    def cosine_distance(self, a, b):                      # SpeakerOperations.swift:62-101
        a, b = np.asarray(a, F), np.asarray(b, F)
        if a.size != b.size or a.size == 0:
            return INF
        dot, ssa, ssb = self.dot(a, b), self.sumsq(a), self.sumsq(b)
        if not (ssa > 0 and ssb > 0):
            BRANCHES["cosine_infinite"] += 1
            return INF
        unit_a, unit_b = abs(ssa - F(1)) <= F(1e-3), abs(ssb - F(1)) <= F(1e-3)
        if unit_a and unit_b:
            similarity = dot
        else:
            BRANCHES["cosine_non_unit"] += 1
            ma, mb = np.sqrt(ssa), np.sqrt(ssb)
            if not (ma > 0 and mb > 0):
                return INF
            with np.errstate(all="ignore"):
                similarity = dot / (ma * mb)
        return F(1) - swift_min(swift_max(similarity, F(-1)), F(1))

    def validate_embedding(self, e, min_magnitude=F(0.1)):   # SpeakerOperations.swift:106-126
        e = np.asarray(e, F)
        if e.size == 0:
            return False
        with np.errstate(all="ignore"):
            magnitude = np.sqrt(self.sumsq(e))
        if not magnitude > F(min_magnitude):
            return False
        return bool(np.all(np.isfinite(e)))


class RawEmbedding:                                       # SpeakerTypes.swift:208-218
    def __init__(self, ar, embedding, timestamp=0, normalized=False):
        self.embedding = np.asarray(embedding, F).copy() if normalized else ar.l2_normalize(embedding)
        self.timestamp = timestamp


class Speaker:                                            # SpeakerTypes.swift:6-162
    def __init__(self, ar, id, current, duration=F(0), created=0, updated=0, permanent=False, raw_capacity=50):
        self.ar, self.id = ar, id
        self.current = ar.l2_normalize(current)
        self.duration = F(duration)
        self.created, self.updated = created, updated
        self.update_count = 1
        self.raws = []
        self.permanent = permanent
        self.raw_capacity = raw_capacity

    def update_main_embedding(self, duration, embedding, tick, alpha=F(0.9)):
        ar = self.ar
        if not ar.sumsq(embedding) > F(0.01):
            return
        normalized = ar.l2_normalize(embedding)
        self.add_raw_embedding(RawEmbedding(ar, normalized, tick), tick)
        if self.current.size == normalized.size:
            self.current = F(alpha) * self.current + (F(1) - F(alpha)) * normalized
            self.current = ar.l2_normalize(self.current)
        self.duration = self.duration + F(duration)
        self.updated = tick
        self.update_count += 1

    def add_raw_embedding(self, raw, tick):
        if not self.ar.sumsq(raw.embedding) > F(0.01):
            return
        if len(self.raws) >= self.raw_capacity:
            BRANCHES["ring_wrap"] += 1
            self.raws.pop(0)
        self.raws.append(raw)
        self.recalculate_main_embedding(tick)

    def recalculate_main_embedding(self, tick):
        if not self.raws or self.raws[0].embedding.size == 0:
            return
        size = self.raws[0].embedding.size
        average = np.zeros(size, F)
        valid = 0
        for raw in self.raws:
            if raw.embedding.size == size:
                average = average + raw.embedding
                valid += 1
        if valid > 0:
            average = average / F(valid)
            self.current = self.ar.l2_normalize(average)
            self.updated = tick


class SpeakerManager:
    """max_speakers None: the reference (an unbounded table, searched in slot = insertion order); else the library's bounded slots."""

    def __init__(self, ar=None, speaker_threshold=0.65, embedding_threshold=0.45, min_speech_duration=1.0, max_speakers=None, raw_capacity=50,
                 ema_alpha=0.9, validate_min_magnitude=-1.0):
        self.ar = ar or Arith()
        self.speaker_threshold, self.embedding_threshold = F(speaker_threshold), F(embedding_threshold)
        self.min_speech_duration, self.ema_alpha, self.validate_min_magnitude = F(min_speech_duration), F(ema_alpha), F(validate_min_magnitude)
        self.max_speakers, self.raw_capacity = max_speakers, raw_capacity
        self.slots = [None] * (max_speakers or 0)
        self.next_id = 1
        self.last = None   # (kind, slot, distance) of the last assign_speaker

    # ---- the table
    def speakers(self):
        return [(s, sp) for s, sp in enumerate(self.slots) if sp is not None]

    def slot_of(self, id):
        return next((s for s, sp in self.speakers() if sp.id == id), -1)

    def get_speaker(self, id):
        s = self.slot_of(id)
        return None if s < 0 else self.slots[s]

    def _free_slot(self):
        for s, sp in enumerate(self.slots):
            if sp is None:
                return s
        if self.max_speakers is None:
            self.slots.append(None)
            return len(self.slots) - 1
        return -1

    @property
    def speaker_count(self):
        return len(self.speakers())

    @property
    def speaker_ids(self):
        return [sp.id for _, sp in self.speakers()]

    # ---- assignSpeaker :135-177
    def assign_speaker(self, embedding, speech_duration, tick=0):
        embedding = np.asarray(embedding, F)
        speech_duration = F(speech_duration)
        if embedding.size != DIM:
            return None
        if self.max_speakers is not None and not np.all(np.isfinite(embedding)):     # the library: no NaN speaker
            return self._took("INVALID", -1, INF)
        if self.validate_min_magnitude >= 0 and not self.ar.validate_embedding(embedding, self.validate_min_magnitude):
            return self._took("INVALID", -1, INF)
        normalized = self.ar.l2_normalize(embedding)
        closest, distance = self.find_closest_speaker(normalized)
        if closest is not None and distance < self.speaker_threshold:
            kind = self.update_existing_speaker(closest, normalized, speech_duration, distance, tick)
            self._took(kind, closest, distance)
            return self.slots[closest]
        if speech_duration >= self.min_speech_duration:
            slot = self._free_slot()
            if slot < 0:
                return self._took("FULL", -1, distance)
            self.create_new_speaker(slot, normalized, speech_duration, tick)
            self._took("CREATED", slot, distance)
            return self.slots[slot]
        return self._took("TOO_SHORT", -1, distance)

    def _took(self, kind, slot, distance):
        BRANCHES[kind] += 1
        self.last = (kind, slot, F(distance))
        return None

    def find_closest_speaker(self, embedding):            # :417-430
        min_distance, closest = INF, None
        for slot, speaker in self.speakers():
            distance = self.ar.cosine_distance(embedding, speaker.current)
            if closest is not None and distance == min_distance:
                BRANCHES["tie"] += 1
            if distance < min_distance:
                min_distance, closest = distance, slot
        return closest, min_distance

    def update_existing_speaker(self, slot, embedding, duration, distance, tick):   # :432-460
        speaker = self.slots[slot]
        if distance < self.embedding_threshold:
            if self.ar.sumsq(embedding) > F(0.01):
                speaker.update_main_embedding(duration, embedding, tick, alpha=self.ema_alpha)
                return "UPDATED"
            return "LOW_ENERGY"
        speaker.duration = speaker.duration + duration
        speaker.updated = tick
        return "DURATION_ONLY"

    def create_new_speaker(self, slot, embedding, duration, tick):                  # :462-492
        normalized = self.ar.l2_normalize(embedding)
        id = self.next_id
        self.next_id += 1
        speaker = Speaker(self.ar, id, normalized, duration, tick, tick, False, self.raw_capacity)
        speaker.add_raw_embedding(RawEmbedding(self.ar, normalized, tick), tick)
        self.slots[slot] = speaker
        return id

    # ---- queries
    def distances(self, query):
        """cosineDistance of the query as it is to every slot, +inf on a free one; the strict minimum's slot (-1: none)."""
        d = np.full(len(self.slots), INF, F)
        for slot, speaker in self.speakers():
            d[slot] = self.ar.cosine_distance(query, speaker.current)
        best, at = INF, -1
        for s in range(len(d)):
            if d[s] < best:
                best, at = d[s], s
        return d, at

    def find_speaker(self, embedding, speaker_threshold=None):                      # :184-191
        closest, distance = self.find_closest_speaker(np.asarray(embedding, F))
        threshold = self.speaker_threshold if speaker_threshold is None else F(speaker_threshold)
        if closest is not None and distance <= threshold:
            return self.slots[closest].id, distance
        return None, INF

    def find_matching_speakers(self, embedding, speaker_threshold=None):            # :198-212
        threshold = self.speaker_threshold if speaker_threshold is None else F(speaker_threshold)
        matches = []
        for _, speaker in self.speakers():
            distance = self.ar.cosine_distance(embedding, speaker.current)
            if distance <= threshold:
                matches.append((speaker.id, distance))
        matches.sort(key=lambda m: m[1])                                             # stable: ties by slot
        return matches

    def find_mergeable_pairs(self, speaker_threshold=None, exclude_if_both_permanent=True):   # :282-328
        """(speakerToMerge, destination, distance)"""
        threshold = self.speaker_threshold if speaker_threshold is None else F(speaker_threshold)
        live = [sp for _, sp in self.speakers()]
        pairs = []
        for i in range(len(live)):
            for j in range(i + 1, len(live)):
                s1, s2 = live[i], live[j]
                if exclude_if_both_permanent and s1.permanent and s2.permanent:
                    continue
                distance = self.ar.cosine_distance(s1.current, s2.current)
                if not distance < threshold:
                    continue
                pairs.append((s2.id, s1.id, distance) if not s2.permanent else (s1.id, s2.id, distance))
        return pairs

    # ---- management
    def make_speaker_permanent(self, id):
        if self.get_speaker(id) is not None:
            self.get_speaker(id).permanent = True

    def revoke_permanence(self, id):
        if self.get_speaker(id) is not None:
            self.get_speaker(id).permanent = False

    def remove_speaker(self, id, keep_if_permanent=True):                            # :334-347
        s = self.slot_of(id)
        if s < 0 or (keep_if_permanent and self.slots[s].permanent):
            return
        self.slots[s] = None

    def remove_speakers_inactive(self, since, keep_if_permanent=True):               # :353-367
        for s, sp in self.speakers():
            if sp.updated < since and not (keep_if_permanent and sp.permanent):
                self.slots[s] = None

    def upsert_speaker(self, id, current, duration, raws=(), update_count=1, created=0, updated=0, permanent=False):   # :552-606
        """raws: RawEmbedding objects (normalised when they were made), oldest first.  True unless no slot is free."""
        speaker = self.get_speaker(id)
        if speaker is not None:
            speaker.current = np.asarray(current, F).copy()
            speaker.duration = F(duration)
            speaker.raws = list(raws)
            speaker.update_count = update_count
            speaker.updated = updated
            if permanent:
                speaker.permanent = True
            return True
        slot = self._free_slot()
        if slot < 0:
            return False
        speaker = Speaker(self.ar, id, current, duration, created, updated, permanent, self.raw_capacity)
        speaker.raws = list(raws)
        speaker.update_count = update_count
        self.slots[slot] = speaker
        self.next_id = max(self.next_id, id + 1)
        return True

    def initialize_known_speakers(self, speakers, mode="skip", preserve_if_permanent=True):   # :62-125, without .merge
        assert mode in ("skip", "overwrite", "reset")
        if mode == "reset":
            self.reset(keep_if_permanent=preserve_if_permanent)
        max_id = 0
        for speaker in speakers:
            if speaker.current.size != DIM:
                continue
            s = self.slot_of(speaker.id)
            if s >= 0:
                if mode == "skip" or (self.slots[s].permanent and preserve_if_permanent):
                    continue
                self.slots[s] = speaker
            else:
                self.slots[self._free_slot()] = speaker
            max_id = max(max_id, speaker.id)
        self.next_id = max_id + 1

    def reset(self, keep_if_permanent=False):                                        # :610-628
        if not keep_if_permanent:
            self.slots = [None] * len(self.slots)
            self.next_id = 1
        else:
            self.slots = [sp if sp is not None and sp.permanent else None for sp in self.slots]
            self.next_id = max([0] + [sp.id for _, sp in self.speakers()]) + 1

    # ---- the whole state, for comparison with fa_speaker_db_get
    def state(self):
        return {sp.id: dict(slot=s, current=sp.current.copy(), raws=[r.embedding.copy() for r in sp.raws], duration=F(sp.duration),
                            update_count=sp.update_count, created=sp.created, updated=sp.updated, permanent=sp.permanent)
                for s, sp in self.speakers()}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def bits1(x):
    return int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


# ---- around the networks: DiarizerManager.processChunkWithSpeakerTracking (Diarizer/Core/DiarizerManager.swift:255-531) and
# EmbeddingExtractor.getEmbeddings (Diarizer/Extraction/EmbeddingExtractor.swift:60-199); the two networks are the caller's.
CHUNK_BRANCHES = collections.Counter()
CHUNK_BRANCH_NAMES = ("gate_pass", "gate_activity", "gate_invalid", "seg_skip_activity", "seg_at_minimum", "seg_no_id", "seg_overlap_threshold",
                      "seg_plain_threshold", "seg_closed", "seg_open_at_end", "seg_too_short", "seg_exact_duration", "seg_cross_64", "seg_frame0",
                      "seg_equal_start", "row_repeat", "row_zero", "run", "no_run")


class ChunkConfig:
    def __init__(self, frames=589, chunk_samples=160000, min_active_frames=10.0, min_speech_duration=1.0, validate_min_magnitude=0.1, frame_step=0.016875):
        self.frames, self.chunk_samples = frames, chunk_samples
        self.min_active_frames, self.min_speech_duration, self.validate_min_magnitude = F(min_active_frames), F(min_speech_duration), F(validate_min_magnitude)
        self.frame_step = float(frame_step)


def seq_sum(x):
    total = F(0)
    for v in np.asarray(x, F):
        total = total + v
    return total


def speaker_activities(w):                                  # calculateSpeakerActivities :400-412
    return np.array([seq_sum(w[:, s]) for s in range(w.shape[1])], F)


def clean_masks(w):                                         # :321-333
    masks = np.zeros((w.shape[1], w.shape[0]), F)
    for f in range(w.shape[0]):
        speaker_sum = F(0)
        for v in w[f]:
            speaker_sum = speaker_sum + v
        is_clean = F(1) if speaker_sum < F(2) else F(0)
        for s in range(w.shape[1]):
            masks[s, f] = w[f, s] * is_clean
    return masks


def plan_chunk(w, samples, cfg):
    """activities, and per speaker the model's mask row or None (EmbeddingExtractor :63-85, 154-199)."""
    frames = w.shape[0]
    masks = clean_masks(w)
    num_masks = min((frames * samples + cfg.chunk_samples // 2) // cfg.chunk_samples, frames)
    rows = []
    for s in range(masks.shape[0]):
        if seq_sum(masks[s]) < cfg.min_active_frames:
            CHUNK_BRANCHES["no_run"] += 1
            rows.append(None)
            continue
        CHUNK_BRANCHES["run"] += 1
        row = np.zeros(frames, F)
        current = num_masks
        row[:current] = masks[s][:current]
        if current > 0:
            CHUNK_BRANCHES["row_repeat"] += current < frames
            while current < frames:
                copy = min(current, frames - current)
                row[current:current + copy] = row[:copy]
                current += copy
        else:
            CHUNK_BRANCHES["row_zero"] += 1
        rows.append(row)
    return speaker_activities(w), rows


def pack_waveform(audio, chunk_samples, repeat):
    """DiarizerManager :266-303 (zero tail) or EmbeddingExtractor.fillWaveformBuffer :118-151 (the doubling loop)."""
    out = np.zeros(chunk_samples, F)
    count = min(len(audio), chunk_samples)
    out[:count] = audio[:count]
    if repeat and count > 0:
        while count < chunk_samples:
            copy = min(count, chunk_samples - count)
            out[count:count + copy] = out[:copy]
            count += copy
    return out


def finish_chunk(m, w, embeddings, offset, cfg, tick=0):
    """The rest of processChunkWithSpeakerTracking for one chunk on the SpeakerManager m: (segments, assignments).  A segment is
    (local speaker, id, start frame, end frame, Float start, Float end, quality); an assignment (id, slot, kind, distance)."""
    ar = m.ar
    activities = speaker_activities(w)
    ids, assignments = [], []
    saved = m.validate_min_magnitude
    m.validate_min_magnitude = cfg.validate_min_magnitude
    for s, activity in enumerate(activities):                # :351-378
        if activity > cfg.min_active_frames:
            duration = F(activity) * F(cfg.frame_step)
            sp = m.assign_speaker(embeddings[s], duration, tick=tick)
            kind, slot, dist = m.last
            CHUNK_BRANCHES["gate_invalid" if kind == "INVALID" else "gate_pass"] += 1
            ids.append(sp.id if sp is not None else 0)
            assignments.append((ids[-1], slot, KINDS.index(kind), bits1(dist)))
        else:
            CHUNK_BRANCHES["gate_activity"] += 1
            ids.append(0)
            assignments.append((0, -1, 0, bits1(INF)))
    m.validate_min_magnitude = saved
    frames, speakers = w.shape
    segments = []

    def create_segment_if_valid(s, start, end):              # :491-526
        if ids[s] == 0:
            CHUNK_BRANCHES["seg_no_id"] += 1
            return
        t0, t1 = offset + float(start) * cfg.frame_step, offset + float(end) * cfg.frame_step
        duration = t1 - t0
        if F(duration) < cfg.min_speech_duration:
            CHUNK_BRANCHES["seg_too_short"] += 1
            return
        CHUNK_BRANCHES["seg_exact_duration"] += F(duration) == cfg.min_speech_duration
        CHUNK_BRANCHES["seg_cross_64"] += start // 64 != (end - 1) // 64
        CHUNK_BRANCHES["seg_frame0"] += start == 0
        quality = swift_min(F(1), np.sqrt(ar.sumsq(embeddings[s])) / F(10)) * (activities[s] / F(end - start))
        segments.append((s, ids[s], start, end, F(t0), F(t1), F(quality)))

    for s in range(speakers):                                 # :428-481
        if activities[s] < cfg.min_active_frames:
            CHUNK_BRANCHES["seg_skip_activity"] += 1
            continue
        CHUNK_BRANCHES["seg_at_minimum"] += activities[s] == cfg.min_active_frames
        active, start = False, 0
        for f in range(frames):
            threshold = F(0.3)
            for other in range(speakers):
                if other != s and w[f, other] > F(0.3):
                    threshold = F(0.15)
                    break
            CHUNK_BRANCHES["seg_overlap_threshold" if threshold == F(0.15) else "seg_plain_threshold"] += 1
            if w[f, s] > threshold and not active:
                active, start = True, f
            elif w[f, s] <= threshold and active:
                CHUNK_BRANCHES["seg_closed"] += 1
                create_segment_if_valid(s, start, f)
                active = False
        if active:
            CHUNK_BRANCHES["seg_open_at_end"] += 1
            create_segment_if_valid(s, start, frames)
    starts = [g[4] for g in segments]
    CHUNK_BRANCHES["seg_equal_start"] += len(set(starts)) < len(starts)
    segments.sort(key=lambda g: (g[4], g[0], g[2]))           # by start time; the library's order among equal starts
    return segments, assignments
