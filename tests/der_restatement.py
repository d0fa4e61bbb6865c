"""A loop-for-loop Python restatement of DiarizationDER.compute (Sources/FluidAudio/Diarizer/DiarizationDER.swift:52-231) and of
HungarianAssignment.solve (Diarizer/HungarianAssignment.swift:8-61), written from the Swift.  Python floats are the reference's Doubles
and Python ints its Ints, so every count is exact and every double has the reference's bits.  The per-label masks are kept as numpy
bool columns only so that the frame loops stay within seconds at 20 000 frames; the arithmetic that decides a frame range is scalar."""
import math
from dataclasses import dataclass, field

import numpy as np


@dataclass(frozen=True)
class Segment:   # DERSpeakerSegment (:26-35)
    speaker: str
    start: float
    end: float


@dataclass
class Result:   # DERResult (:37-46) and, beside it, the integers it was formed from
    der: float = 0.0
    confusion: float = 0.0
    false_alarm: float = 0.0
    miss: float = 0.0
    total_ref_speech: float = 0.0
    mapping: dict = field(default_factory=dict)
    frames: int = 0
    counts: tuple = (0, 0, 0, 0)                      # miss, false alarm, confusion, ref
    ref_labels: list = field(default_factory=list)
    hyp_labels: list = field(default_factory=list)
    index_mapping: list = field(default_factory=list)  # hyp index -> ref index or -1
    overlap: list = field(default_factory=list)        # [H][R]


def hungarian(cost, n):   # HungarianAssignment.solve (:8-61)
    if n == 0:
        return []
    INF = (2 ** 63 - 1) // 4
    u = [0] * (n + 1)
    v = [0] * (n + 1)
    p = [0] * (n + 1)
    way = [0] * (n + 1)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = [INF] * (n + 1)
        used = [False] * (n + 1)
        while True:
            used[j0] = True
            i0 = p[j0]
            delta = INF
            j1 = 0
            for j in range(1, n + 1):
                if used[j]:
                    continue
                cur = cost[(i0 - 1) * n + (j - 1)] - u[i0] - v[j]
                if cur < minv[j]:
                    minv[j] = cur
                    way[j] = j0
                if minv[j] < delta:
                    delta = minv[j]
                    j1 = j
            for j in range(0, n + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while True:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == 0:
                break
    assign = [-1] * n
    for j in range(1, n + 1):
        if p[j] != 0:
            assign[p[j] - 1] = j - 1
    return assign


def rasterise(segs, label_idx, num_labels, num_frames, frame_step):   # :209-230; mask[t][label]
    mask = np.zeros((num_frames, num_labels), bool)
    if num_labels == 0:
        return mask
    for seg in segs:
        if not seg.end > seg.start:
            continue
        li = label_idx[seg.speaker]
        t_start = max(0, int(math.ceil(seg.start / frame_step - 0.5)))
        t_end_ex = min(num_frames, int(math.ceil(seg.end / frame_step - 0.5)))
        if t_end_ex <= t_start:
            continue
        mask[t_start:t_end_ex, li] = True
    return mask


def collar_mask(ref, num_frames, frame_step, collar):   # :181-204
    mask = np.ones(num_frames, bool)
    if collar <= 0:
        return mask
    half = collar / 2.0
    boundaries = []
    for s in ref:
        if s.end > s.start:
            boundaries.append(s.start)
            boundaries.append(s.end)
    for b in boundaries:
        lo = max(0, int(math.floor((b - half) / frame_step)))
        hi = min(num_frames, int(math.ceil((b + half) / frame_step)))
        if hi <= lo:
            continue
        mask[lo:hi] = False
    return mask


def compute(ref, hyp, frame_step=0.01, collar=0.0) -> Result:   # :52-175
    assert frame_step > 0 and collar >= 0
    ref_labels, hyp_labels, ref_idx, hyp_idx = [], [], {}, {}
    max_end = 0.0
    for s in ref:
        if s.speaker not in ref_idx:
            ref_idx[s.speaker] = len(ref_labels)
            ref_labels.append(s.speaker)
        max_end = max(max_end, s.end)
    for s in hyp:
        if s.speaker not in hyp_idx:
            hyp_idx[s.speaker] = len(hyp_labels)
            hyp_labels.append(s.speaker)
        max_end = max(max_end, s.end)
    num_frames = int(math.ceil(max_end / frame_step)) + 1
    if num_frames <= 0 or (not ref_labels and not hyp_labels):
        return Result()
    ref_mask = rasterise(ref, ref_idx, len(ref_labels), num_frames, frame_step)
    hyp_mask = rasterise(hyp, hyp_idx, len(hyp_labels), num_frames, frame_step)

    H, R = len(hyp_labels), len(ref_labels)
    overlap = [0] * (H * R)
    if H > 0 and R > 0:
        for t in range(num_frames):
            hs = np.flatnonzero(hyp_mask[t])
            if hs.size == 0:
                continue
            rs = np.flatnonzero(ref_mask[t])
            for h in hs:
                for r in rs:
                    overlap[h * R + r] += 1

    n = max(H, R)
    mapping = [-1] * H
    if n > 0:
        max_o = max(overlap) if overlap else 0
        cost = [max_o] * (n * n)
        for h in range(H):
            for r in range(R):
                cost[h * n + r] = max_o - overlap[h * R + r]
        assign = hungarian(cost, n)
        for h in range(H):
            r = assign[h]
            if r < R and overlap[h * R + r] > 0:
                mapping[h] = r

    scorable = collar_mask(ref, num_frames, frame_step, collar)
    sum_miss = sum_fa = sum_conf = sum_ref = 0
    for t in range(num_frames):
        if not scorable[t]:
            continue
        n_ref = int(ref_mask[t].sum())
        n_sys = int(hyp_mask[t].sum())
        n_correct = 0
        for h in np.flatnonzero(hyp_mask[t]):
            rm = mapping[h]
            if rm >= 0 and ref_mask[t, rm]:
                n_correct += 1
        sum_miss += max(0, n_ref - n_sys)
        sum_fa += max(0, n_sys - n_ref)
        sum_conf += min(n_ref, n_sys) - n_correct
        sum_ref += n_ref
    miss_s = float(sum_miss) * frame_step
    fa_s = float(sum_fa) * frame_step
    conf_s = float(sum_conf) * frame_step
    ref_s = float(sum_ref) * frame_step
    der = (miss_s + fa_s + conf_s) / ref_s if ref_s > 0 else 0.0
    map_out = {hyp_labels[h]: ref_labels[mapping[h]] for h in range(H) if mapping[h] >= 0}
    return Result(der, conf_s, fa_s, miss_s, ref_s, map_out, num_frames, (sum_miss, sum_fa, sum_conf, sum_ref), ref_labels, hyp_labels, mapping,
                  [overlap[h * R:(h + 1) * R] for h in range(H)])


# The inputs of the hand-checked cases (tests/test_der_cpu.py works the answers out), shared with the device tests.
CASE1 = ([Segment("A", 0.0, 10.0), Segment("B", 10.0, 20.0)], [Segment("x", 0.0, 12.0), Segment("y", 12.0, 20.0)])
CASE2 = ([Segment("A", 0.0, 1.0), Segment("B", 0.5, 1.5)], [Segment("x", 0.0, 1.5), Segment("y", 0.0, 1.5), Segment("z", 2.0, 2.0)])
CASE4 = ([Segment("A", 0.145, 0.64), Segment("A", 0.3, 1.28)], [Segment("x", -0.2, 0.635)])
