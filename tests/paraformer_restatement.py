"""Literal numpy restatement of the Paraformer host loop of the reference, line by line and in its own order of operations:
ParaformerCif.integrateAndFireWithFireFrames (Sources/FluidAudio/ASR/Paraformer/ParaformerCif.swift:19-50), the decoder's input packing
(ParaformerManager.swift:416-448) and decodeWithTimestamps with its helpers (ParaformerManager.swift:134-358).  fp32 values are
numpy.float32 scalars and arrays (every product and every sum rounded on its own: no fused multiply-add), the time arithmetic is Python
float (fp64).  The reference has no unit test of these routines: this restatement is the oracle, pinned by the hand-derived cases of
tests/test_paraformer_cpu.py."""
import numpy as np

F = np.float32
CIF_THRESHOLD, CIF_TAIL_THRESHOLD = F(1.0), F(0.45)        # ParaformerConfig.swift:28-29
DECODER_ENC_FRAMES, DECODER_MAX_TOKENS = 512, 128          # :19-20
BLANK_ID, SOS_ID, EOS_ID = 0, 1, 2                         # :23-25
SAMPLE_RATE = 16000                                        # :31
WORD_BOUNDARY = "▁"                                   # ASRConstants.sentencePieceWordBoundary


def integrate_and_fire(enc_rows, alphas, threshold=CIF_THRESHOLD, tail=CIF_TAIL_THRESHOLD):
    """ParaformerCif.swift:19-50.  enc_rows [T, D] (fp32, or fp16: widened as rows(of:) does), alphas [T].  Returns (embeds [L, D], fire frames)."""
    enc_rows = np.asarray(enc_rows).astype(np.float32)
    T, dim = enc_rows.shape
    threshold, tail = F(threshold), F(tail)
    embeds, fires = [], []
    integrate = F(0)
    frame = np.zeros(dim, np.float32)
    zero = np.zeros(dim, np.float32)
    with np.errstate(all="ignore"):
        for t in range(T + 1):
            alpha = F(alphas[t]) if t < T else tail
            hidden = enc_rows[t] if t < T else zero
            integrate = F(integrate + alpha)
            if integrate < threshold:
                frame = frame + alpha * hidden
            else:
                used = F(alpha - F(integrate - threshold))
                frame = frame + used * hidden
                embeds.append(frame)
                fires.append(t)
                integrate = F(integrate - threshold)
                leftover = F(alpha - used)
                frame = hidden * leftover
    return (np.stack(embeds) if embeds else np.zeros((0, dim), np.float32)), fires


def decoder_inputs(enc_rows, alphas, enc_frames=DECODER_ENC_FRAMES, max_tokens=DECODER_MAX_TOKENS):
    """runDecoder's fixed shapes (:416-448): ac [max_tokens, D], tn, enc [enc_frames, D]; and the unclamped fire frames."""
    enc_rows = np.asarray(enc_rows).astype(np.float32)
    embeds, fires = integrate_and_fire(enc_rows, alphas)
    n = min(len(fires), max_tokens)
    ac = np.zeros((max_tokens, enc_rows.shape[1]), np.float32)
    ac[:n] = embeds[:n]
    enc = np.zeros((enc_frames, enc_rows.shape[1]), np.float32)
    v = min(enc_rows.shape[0], enc_frames)
    enc[:v] = enc_rows[:v]
    return ac, n, fires, enc


def cif_wo_hidden_fire_indices(alphas, threshold):
    """:262-273"""
    integrate, fires = F(0), []
    for t, a in enumerate(alphas):
        integrate = F(integrate + F(a))
        if integrate >= threshold:
            fires.append(t)
            integrate = F(integrate - F(1.0))
    return fires


def energy_envelope(audio, sample_rate=16000.0, hop_sec=0.01):
    """:277-293"""
    audio = np.asarray(audio, np.float32)
    hop = max(1, int(hop_sec * sample_rate))
    if not audio.size > hop:
        return np.zeros(0, np.float32)
    n = audio.size // hop
    x = audio[:n * hop].reshape(n, hop)
    with np.errstate(all="ignore"):
        sq = x * x                      # each product rounded to fp32
        s = np.zeros(n, np.float32)
        for j in range(hop):            # the sequential sum, all frames at once
            s = s + sq[:, j]
        return np.sqrt(s / F(hop)).astype(np.float32)


def percentile(values, q):
    """:296-301"""
    values = np.asarray(values, np.float32)
    if values.size == 0:
        return F(0)
    s = np.sort(values, kind="stable")
    pos = max(0, min(s.size - 1, int(F(F(s.size - 1) * F(q)))))
    return s[pos]


def smooth(x, window=3):
    """:304-316"""
    x = np.asarray(x, np.float32)
    if not (window > 1 and x.size > window):
        return x
    out = x.copy()
    half = window // 2
    with np.errstate(all="ignore"):
        for i in range(x.size):
            lo, hi = max(0, i - half), min(x.size - 1, i + half)
            s = F(0)
            for k in range(lo, hi + 1):
                s = F(s + x[k])
            out[i] = F(s / F(hi - lo + 1))
    return out


def energy_span(frm, to, centroid, env, hop_sec, threshold, min_run, trace=None):
    """:322-358.  trace (a list) collects (runs in the window, index of the chosen one)."""
    if not (len(env) > 0 and hop_sec > 0 and to > frm and min_run > 0):
        return None
    i0 = max(0, int(frm / hop_sec))
    i1 = min(len(env) - 1, max(i0, int(to / hop_sec)))
    if not i1 >= i0:
        return None
    runs = []
    j = i0
    while j <= i1:
        if env[j] > threshold:
            k = j
            while k <= i1 and env[k] > threshold:
                k += 1
            if k - j >= min_run:
                runs.append((j, k - 1))
            j = k
        else:
            j += 1
    if not runs:
        return None
    ci = int(centroid / hop_sec)
    best, best_d = runs[0], abs((runs[0][0] + runs[0][1]) - 2 * ci)
    for r in runs[1:]:
        d = abs((r[0] + r[1]) - 2 * ci)
        if d < best_d:
            best_d, best = d, r
    if trace is not None:
        trace.append((len(runs), runs.index(best)))
    return (float(best[0]) * hop_sec, float(best[1]) * hop_sec)


def keep_table(vocabulary, size):
    """The charList filter of :146-156 as a table: 0 for blank, <s>, </s>, ids without an entry and empty strings."""
    keep = np.zeros(size, np.uint8)
    for i, tok in vocabulary.items():
        if 0 <= i < size and i not in (BLANK_ID, SOS_ID, EOS_ID) and tok:
            keep[i] = 1
    return keep


def raw_spans(token_ids, keep, alphas, audio, trace=None):
    """decodeWithTimestamps up to its `raw` array (:141-226): [(position in token_ids, start, end)].  trace (a dict) collects what the
    tests ask about: which path was taken."""
    trace = {} if trace is None else trace
    upsample = 3
    time_rate = 10.0 * 6.0 / 1000.0 / float(upsample)
    cif_threshold = F(F(1.0) - F(1e-4))
    kept = [i for i, t in enumerate(token_ids) if 0 <= t < len(keep) and keep[t]]
    if not len(kept) >= 1:
        return []
    us = [F(a) for a in alphas for _ in range(upsample)] + [CIF_TAIL_THRESHOLD]
    fires = cif_wo_hidden_fire_indices(us, cif_threshold)
    trace["fallback"] = len(fires) != len(kept) + 1
    if len(fires) != len(kept) + 1:
        target = F(len(kept) + 1)
        total = F(0)
        for a in us:
            total = F(total + a)
        m = F(1e-6) if F(1e-6) >= total else total       # Swift's max(x, y): y >= x ? y : x
        scale = F(target / m)
        us = [F(a * scale) for a in us]
        fires = cif_wo_hidden_fire_indices(us, cif_threshold)
    trace["fires"] = list(fires)
    if not len(fires) >= 2:
        return []
    audio = np.asarray(audio, np.float32)
    audio_end = float(audio.size) / float(SAMPLE_RATE)
    centroids = [float(f) * time_rate for f in fires]
    env = smooth(energy_envelope(audio, float(SAMPLE_RATE), 0.01), 3)
    floor = F(0) if env.size == 0 else percentile(env, 0.1)
    v = F(floor * F(2.5))
    energy_threshold = F(1e-4) if F(1e-4) >= v else v
    trace["threshold"] = energy_threshold
    min_run = 3
    n = min(len(kept), len(centroids) - 1)
    spacings = [F(centroids[i] - centroids[i - 1]) for i in range(1, max(n, 1))]
    typical = float(F(0.3) if not spacings else percentile(spacings, 0.5))
    raw, cursor = [], 0.0
    trace["no_run"], trace["runs"] = [], []
    for i in range(n):
        if i < n - 1:
            dur = centroids[i + 1] - centroids[i]
        else:
            dur = min(audio_end - centroids[i], max(typical * 2, 0.4))
        search_end = min(audio_end, centroids[i] + dur * 1.5 + 0.15)
        span = energy_span(cursor, search_end, centroids[i], env, 0.01, energy_threshold, min_run, trace["runs"])
        if span is not None:
            s, e = span
        else:
            s, e = cursor, min(audio_end, cursor + max(dur, 0.1))
            trace["no_run"].append(i)
        cursor = e
        raw.append((kept[i], s, e))
    return raw


def segments_from_spans(pieces, spans):
    """The emission of :228-256 over `raw`: pieces[i] is the text of span i; spans [(start, end)].  Returns [(startTime, endTime, text)]."""
    out, i = [], 0
    while i < len(spans):
        text, start, end = pieces[i], spans[i][0], spans[i][1]
        while text.endswith("@@"):
            text = text[:-2]
            i += 1
            if i < len(spans):
                piece = pieces[i][1:] if pieces[i].startswith(WORD_BOUNDARY) else pieces[i]
                text += piece
                end = spans[i][1]
        if text.startswith(WORD_BOUNDARY):
            text = text[1:]
        if text:
            out.append((start if start >= 0 else 0.0, end, text))   # max(0, item.start)
        i += 1
    return out


def decode_tokens(token_ids, vocabulary):
    """decode (:450-463) behind the argmax."""
    pieces = [vocabulary[t] for t in token_ids if t not in (BLANK_ID, SOS_ID, EOS_ID) and t in vocabulary]
    return "".join(pieces).replace(WORD_BOUNDARY, " ").strip(" \t")
