"""A line-by-line numpy restatement of the PocketTTS host code the session replaces (not a test): PocketTtsVoiceCloner.swift:79-118,
131-143, 296-299, 321-376; PocketTtsSynthesizer+KVCache.swift:190-240, 254-357, 368-455, 471-506; PocketTtsStateEngine.swift:80-111,
227-290; PocketTtsSynthesizer.swift:527-568, 1208-1223."""
import numpy as np

DIM, LATENT, WINDOW, KV_SEQ, KV_ROW, FRAME, ENCODER_SAMPLES, MAX_VOICE_FRAMES, EOS_THRESHOLD, EXTRA = 1024, 32, 256, 512, 1024, 1920, 240000, 125, -4.0, 2


def clone_plan(samples: int, available: int = MAX_VOICE_FRAMES):
    """VoiceCloner :137-143, :148, :296-299 -> (status, usable)"""
    if samples / 24000.0 < 1.0:
        return 1, 0
    real = min(samples, ENCODER_SAMPLES)
    return 0, min(available, (real + FRAME - 1) // FRAME, MAX_VOICE_FRAMES)


def encoder_input(samples: np.ndarray) -> np.ndarray:
    """VoiceCloner :281-288"""
    buffer = np.zeros(ENCODER_SAMPLES, np.float32)
    n = min(samples.size, ENCODER_SAMPLES)
    buffer[:n] = samples[:n]
    return buffer


def extract(flat: np.ndarray, frames: int, frame_stride: int, dim_stride: int) -> np.ndarray:
    """VoiceCloner :343-348 / :369-374, the strided fallback (the general case): float32 [frames, 1024]"""
    result = np.zeros((frames, DIM), np.float32)
    for frame in range(frames):
        base = frame * frame_stride
        result[frame] = flat[base:base + (DIM - 1) * dim_stride + 1:dim_stride].astype(np.float32)
    return result


def reproject(cond: np.ndarray, pinv: np.ndarray, w: np.ndarray, dtype=np.float64) -> np.ndarray:
    """VoiceCloner :79-118: two row-major sgemms"""
    return (cond.astype(dtype) @ pinv.astype(dtype)) @ w.astype(dtype).T


def kv_from_snapshot(layers, offsets, src_seq: int, kv_format: int):
    """KVCache :368-455 (formats 0 combined, 1 split) and StateEngine :227-290 (format 2, fp16) -> per layer (K [512, 1024], V), positions.
    `layers`: per layer the flat [2, 1, src_seq, 16, 64] floats, or None for the empty state (emptyKVCacheState / resetToZero)."""
    dt = np.float16 if kv_format == 2 else np.float32
    out = []
    for cache in layers or []:
        k, v = np.zeros((KV_SEQ, KV_ROW), dt), np.zeros((KV_SEQ, KV_ROW), dt)
        per = src_seq * KV_ROW
        with np.errstate(all="ignore"):
            k[:src_seq] = cache[:per].reshape(src_seq, KV_ROW).astype(dt)        # astype(float16): round to nearest even
            v[:src_seq] = cache[per:2 * per].reshape(src_seq, KV_ROW).astype(dt)
        out.append((k, v))
    if layers is None:
        return None, np.zeros(1 if kv_format == 2 else len(offsets), np.float32)
    pos = np.array([float(offsets[0])] if kv_format == 2 else [float(o) for o in offsets], np.float32)
    return out, pos


def embed_tokens(ids, table: np.ndarray) -> np.ndarray:
    """Synthesizer :1208-1223"""
    vocab = table.shape[0]
    return np.stack([table[min(max(int(i), 0), vocab - 1)] for i in ids]) if len(ids) else np.zeros((0, DIM), np.float32)


def windows_of(flat: np.ndarray):
    """KVCache :206-239 over one block: [(first, n, conditioning [256, 1024], valid_len)]"""
    out, processed, count = [], 0, flat.shape[0]
    while processed < count:
        n = min(WINDOW, count - processed)
        cond = np.zeros((WINDOW, DIM), np.float32)
        cond[:n] = flat[processed:processed + n]
        out.append((processed, n, cond, np.float32(n)))
        processed += n
    return out


def prefill_blocks(voice, ids, table, bos_before_voice):
    """KVCache :471-506 for one stream -> (status, [(block, first, n, conditioning, valid_len)]).  `voice`: dict(snapshot: bool, rows: float32
    [promptLength, 1024] or None)."""
    out = []
    if not voice["snapshot"] and voice["rows"] is not None and voice["rows"].shape[0] > 0:   # prefillKVCacheVoice :267-301
        if bos_before_voice is None:
            return 5, []
        flat = np.concatenate([bos_before_voice[None, :], voice["rows"]])
        out += [(0,) + w for w in windows_of(flat)]
    out += [(1,) + w for w in windows_of(embed_tokens(ids, table))]                          # prefillKVCacheText :340-347
    return 0, out


def generation_loop(eos_logits, max_gen_len: int, frames_after_eos: int):
    """Synthesizer :527-568 for one stream: the steps whose frame is decoded, and the end reason (2: EOS, 3: maxGenLen) with the number of
    network calls made."""
    emitted, eos_step, total_after = [], None, frames_after_eos + EXTRA
    for step in range(max_gen_len):
        eos_logit = eos_logits[step]
        if eos_logit > EOS_THRESHOLD and eos_step is None:
            eos_step = step
        if eos_step is not None and step >= eos_step + total_after:
            return emitted, 2, step + 1
        emitted.append(step)
    return emitted, 3, max_gen_len
