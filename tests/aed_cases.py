"""The calls that the CPU and the GPU tests of the AED unit share: decode cases (a config, one prompt per utterance and the logits
row of every step) and merge cases.  A scripted utterance is written step by step against the restatement (tests/aed_restatement.py),
so a row can aim at the history the reference's loop has at that step; the rows are then plain data.  tests/test_aed_cpu.py proves
that the cases hold every kind of decision; tests/test_gpu_aed.py replays them on the device."""
import numpy as np

import aed_restatement as R

F32_MAX = float(np.finfo(np.float32).max)


# ---- directors: feed (the restatement's state before the step), vocab, eos, rng -> the row of that step
def emit(t, hi=10.0):
    def row(feed, V, eos, rng):
        r = np.full(V, -3.0, np.float32)
        r[eos] = -50.0
        r[t] = hi
        return r
    return row


def eos_row(feed, V, eos, rng):
    r = np.full(V, -1.0, np.float32)
    r[eos] = 4.0
    return r


def _fresh(feed, V, eos, k=0):
    """the k-th id that is neither in the history nor EOS"""
    return [i for i in range(V) if i not in feed.all_tokens and i != eos][k]


def pos_flip(feed, V, eos, rng):
    """the penalty takes a positive maximum from a history id"""
    r = np.full(V, -5.0, np.float32)
    r[feed.all_tokens[0]], r[_fresh(feed, V, eos)] = 2.0, 1.9
    return r


def neg_flip(feed, V, eos, rng):
    """the same among negative logits: -1.0 * p falls below -1.05"""
    r = np.full(V, -9.0, np.float32)
    r[feed.all_tokens[-1]], r[_fresh(feed, V, eos)] = -1.0, -1.05
    return r


def tie(history_index, fresh_rank):
    """a history id whose penalised value EQUALS the value of an id outside the history (float32 arithmetic, as the penalty's)"""
    def row(feed, V, eos, rng):
        r = np.full(V, -7.0, np.float32)
        a, c = feed.all_tokens[history_index], _fresh(feed, V, eos, fresh_rank)
        r[a] = np.float32(3.3)
        r[c] = np.float32(3.3) / np.float32(feed.cfg["repetition_penalty"])
        return r
    return row


def ban_flip(feed, V, eos, rng):
    """the maximum sits on the id the n-gram rule bans at this step (the script has built the repeat); the runner-up is fresh"""
    probe = np.zeros(V, np.float32)
    R.apply_no_repeat_ngram(probe, feed.all_tokens, feed.cfg["no_repeat_ngram"])
    banned = [i for i in range(V) if probe[i] != 0 and i != eos]
    r = np.full(V, -4.0, np.float32)
    r[eos] = -50.0
    r[banned[0]] = 9.0
    r[_fresh(feed, V, eos)] = 1.0
    return r


def hot(feed, V, eos, rng):
    """a random row whose few hot ids make repeats, penalties and bans likely"""
    r = rng.standard_normal(V).astype(np.float32)
    ids = np.array([(int(k) * 977 + 11) % V for k in rng.integers(0, 6, 3)])   # three of six fixed ids, anywhere in the row
    r[ids] += np.float32(6.0) + rng.standard_normal(3).astype(np.float32) * np.float32(0.3)
    r[eos] -= np.float32(3.0)
    return r


def build(name, cfg, utterances, seed=0, dtype=np.float32, filler=hot, eos_after=None):
    """utterances: [(prompt, [director, ...])]; behind its script an utterance goes on with `filler` until it ends.  eos_after: per
    utterance the step from which the filler puts the maximum on EOS (None: never)."""
    rng = np.random.default_rng(seed)
    V, eos = cfg["vocab"], cfg["eos_id"]
    feeds = [(R.SequenceFeed if cfg["mode"] == 1 else R.TokenFeed)(p, cfg) for p, _ in utterances]
    rows = []
    step = 0
    while any(f.reason == R.RUNNING for f in feeds):
        now = np.zeros((len(feeds), V), dtype)
        for b, f in enumerate(feeds):
            if f.reason != R.RUNNING:
                continue
            script = utterances[b][1]
            director = script[step] if step < len(script) else filler
            if step >= len(script) and eos_after is not None and eos_after[b] is not None and step >= eos_after[b]:
                director = eos_row
            now[b] = director(f, V, eos, rng).astype(dtype)
            f.step(now[b])
        rows.append(now)
        step += 1
    return dict(name=name, cfg=cfg, prompts=[list(p) for p, _ in utterances], rows=np.stack(rows) if rows else np.zeros((0, len(feeds), V), dtype))


def replay(case):
    """The restatement over a case: per step what every utterance looks like after it, and the decisions' kinds."""
    cfg = case["cfg"]
    feeds = [(R.SequenceFeed if cfg["mode"] == 1 else R.TokenFeed)(p, cfg) for p in case["prompts"]]
    kinds, discarded = [], []
    for now in case["rows"]:
        for b, f in enumerate(feeds):
            if f.reason != R.RUNNING:
                continue
            if cfg["mode"] == 0 and not f.decides():
                discarded.append((b, f.step_index, R.argmax_first(R.widen(now[b]))))
            f.step(now[b])
            if cfg["mode"] == 0 and f.kind is not None:
                kinds.append(dict(f.kind, utterance=b, n=cfg["no_repeat_ngram"], penalty=cfg["repetition_penalty"]))
                f.kind = None
        yield feeds, kinds, discarded


def token_cfg(V, max_seq, max_new, n, p, eos=3):
    return dict(R.COHERE, vocab=V, eos_id=eos, max_seq=max_seq, max_new=max_new, no_repeat_ngram=n, repetition_penalty=p)


def seq_cfg(V, max_seq, eos=3):
    return dict(R.CANARY, vocab=V, eos_id=eos, max_seq=max_seq)


def _all_inf(feed, V, eos, rng):
    return np.full(V, -np.inf, np.float32)


def _lowest(feed, V, eos, rng):
    """nothing above -greatestFiniteMagnitude but one id"""
    r = np.full(V, -F32_MAX, np.float32)
    r[5] = np.float32(-3.0e38)
    return r


def _tied(feed, V, eos, rng):
    r = np.full(V, 1.0, np.float32)
    r[[2, 6]] = 2.0
    return r


def scripted_cases():
    cases = []
    # n = 3 with the penalty; max_seq binds (min(30 + P, 16)); prompts of 3, 1 and 2 tokens in one batch
    a = token_cfg(12, 16, 30, 3, 1.1)
    cases.append(build("n3", a, [
        ([5, 6, 7], [eos_row, eos_row, pos_flip, neg_flip, tie(2, 0), tie(3, 2), emit(2), emit(4), emit(6), emit(2), emit(4), emit(1), ban_flip]),
        ([4], [eos_row]),                                         # P = 1 and EOS at the first output step
        ([2, 2], [eos_row, emit(0), emit(1), emit(4), emit(0), emit(1), emit(5), ban_flip]),
    ], seed=1, eos_after=[None, None, 9]))
    # n = 2; max_new binds: P = 2, max_new = 4 -> steps 0 ... 5, five outputs
    b = token_cfg(12, 16, 4, 2, 1.1)
    cases.append(build("n2", b, [([6, 7], [eos_row, emit(1), emit(0), emit(1), emit(2), ban_flip]), ([5], [emit(0), emit(1), pos_flip, neg_flip, emit(2)])], seed=2))
    # n = 4 without a penalty: the bit map is built for the ban alone; the history is shorter than n - 1 at the first decisions
    c = token_cfg(12, 14, 30, 4, 1.0)
    cases.append(build("n4", c, [([7], [emit(0), emit(1), emit(2), emit(4), emit(0), emit(1), emit(2), emit(5), ban_flip]), ([5, 5, 5, 5, 5], [])], seed=3))
    # n = 1 bans every history id; n = 0 leaves the penalty alone; both off: the plain argmax
    cases.append(build("n1", token_cfg(12, 12, 30, 1, 1.3), [([6], [emit(0), emit(1), ban_flip]), ([1, 2], [])], seed=4))
    cases.append(build("n0", token_cfg(12, 12, 30, 0, 1.2), [([6, 0], [eos_row, pos_flip, neg_flip, tie(0, 0)]), ([1], [])], seed=5, eos_after=[None, 6]))
    cases.append(build("plain", token_cfg(12, 12, 30, 0, 1.0), [([6, 0], [eos_row, emit(0), emit(0), emit(0)]), ([1], [_all_inf, emit(2)])], seed=6, eos_after=[7, 4]))
    # history ids outside the vocabulary (a prompt token beyond V, a negative one) are neither penalised nor banned
    cases.append(build("outside", token_cfg(5, 12, 30, 2, 1.1, eos=0), [([9, -1, 2], [eos_row, eos_row]), ([7, 1], [eos_row])], seed=7))
    # the sequence feed: EOS, the cap at pos == S, an all -inf row, nothing above -greatestFiniteMagnitude, a tie
    s = seq_cfg(12, 12)
    cases.append(build("seq", s, [([7, 7, 4], [_all_inf, _lowest, _tied, emit(1), eos_row]), ([1] * 11, [emit(2)]), ([1] * 12, []), ([5], [emit(i % 3) for i in range(11)])],
                       seed=8, filler=hot))
    return cases


def random_cases():
    """The shapes of the GPU test: V in {5, 130, 1025, 16384}, both dtypes, B in {1, 3, 67}, max_seq 12 ... 24, utterances that end at different steps."""
    cases = []
    grid = [(5, 67, 12, np.float32), (130, 3, 17, np.float16), (1025, 67, 14, np.float16), (16384, 3, 24, np.float32), (16384, 1, 13, np.float16), (130, 1, 12, np.float32),
            (1025, 3, 13, np.float32)]
    for k, (V, B, S, dt) in enumerate(grid):
        rng = np.random.default_rng(100 + k)
        eos = 3
        prompts = [rng.integers(0, V, int(rng.integers(1, 5))).tolist() for _ in range(B)]
        ends = [None if b % 3 == 0 else int(rng.integers(2, S)) for b in range(B)]
        cases.append(build(f"tok-{V}-{B}", token_cfg(V, S, S if k % 2 else 6, 3 if k % 3 else 2, 1.1, eos), [(p, []) for p in prompts], seed=200 + k, dtype=dt, eos_after=ends))
        cases.append(build(f"seq-{V}-{B}", seq_cfg(V, S, eos), [(p, []) for p in prompts], seed=300 + k, dtype=dt, eos_after=ends))
    return cases


# ---- merge cases: (name, [windows of one recording], window_tokens, min_match, expected or None)
MERGE_LITERAL = [   # CohereLongFormTests and CanaryChunkMergeTests, every mergeTokenStreams case
    ("cohere-prefix-empty", [[], [1, 2, 3]], 32, 4, [1, 2, 3]),
    ("cohere-suffix-empty", [[1, 2, 3], []], 32, 4, [1, 2, 3]),
    ("cohere-no-common-run", [[10, 11, 12, 13], [20, 21, 22, 23]], 32, 4, [10, 11, 12, 13, 20, 21, 22, 23]),
    ("cohere-short-match", [[1, 2, 3, 7, 8, 9], [7, 8, 9, 100, 200]], 32, 4, [1, 2, 3, 7, 8, 9, 7, 8, 9, 100, 200]),
    ("cohere-overlap-at-boundary", [[1, 2, 3, 4, 50, 51, 52, 53, 54], [50, 51, 52, 53, 54, 60, 61, 62]], 32, 4, [1, 2, 3, 4, 50, 51, 52, 53, 54, 60, 61, 62]),
    ("cohere-overlap-offset", [[1, 2, 3, 90, 91, 92, 93, 94, 95], [91, 92, 93, 94, 95, 200, 201]], 32, 4, [1, 2, 3, 90, 91, 92, 93, 94, 95, 200, 201]),
    ("cohere-longest-run", [[1, 2, 3, 4, 7, 8, 9, 10, 11], [1, 2, 3, 4, 7, 8, 9, 10, 11, 99]], 32, 4, [1, 2, 3, 4, 7, 8, 9, 10, 11, 99]),
    ("cohere-window-bounds", [list(range(200)) + [500, 501, 502, 503, 504], [500, 501, 502, 503, 504, 700, 701]], 32, 4,
     list(range(200)) + [500, 501, 502, 503, 504, 700, 701]),
    ("canary-empty-prefix", [[], [1, 2, 3]], 32, 4, [1, 2, 3]),
    ("canary-empty-suffix", [[1, 2, 3], []], 32, 4, [1, 2, 3]),
    ("canary-clean-seam", [[1, 2, 3, 7, 8, 9, 10], [7, 8, 9, 10, 11, 12]], 32, 4, [1, 2, 3, 7, 8, 9, 10, 11, 12]),
    ("canary-partial-overlap", [[1, 2, 20, 21, 22, 23, 24], [99, 20, 21, 22, 23, 24, 30, 31]], 32, 4, [1, 2, 20, 21, 22, 23, 24, 30, 31]),
    ("canary-no-match", [[1, 2, 3], [4, 5, 6]], 32, 4, [1, 2, 3, 4, 5, 6]),
    ("canary-short-match", [[1, 5, 6, 7], [5, 6, 7, 8, 9]], 32, 4, [1, 5, 6, 7, 5, 6, 7, 8, 9]),
    ("canary-match-at-threshold", [[1, 5, 6, 7, 8], [5, 6, 7, 8, 9]], 32, 4, [1, 5, 6, 7, 8, 9]),
]
MERGE_OWN = [
    # the longest run (4) appears twice in the suffix's head: the first one in row-major order wins, so the second copy stays
    ("run-twice", [[9, 1, 2, 3, 4], [1, 2, 3, 4, 8, 1, 2, 3, 4, 7]], 32, 4, None),
    # ... and twice in the prefix's tail: the lower row wins, the column is the same
    ("run-twice-rows", [[1, 2, 3, 4, 8, 1, 2, 3, 4], [1, 2, 3, 4, 6]], 32, 4, None),
    ("exactly-min-match", [[1, 5, 6, 7, 8], [5, 6, 7, 8, 9]], 32, 4, None),
    ("below-min-match", [[1, 5, 6, 7], [5, 6, 7, 8, 9]], 32, 4, None),
    ("prefix-longer-than-window", [list(range(100, 150)) + [1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6]], 7, 4, None),
    ("run-outside-window", [[1, 2, 3, 4, 5] + list(range(100, 110)), [1, 2, 3, 4, 5, 6]], 7, 4, None),
    ("empty-window-in-the-middle", [[1, 2, 3, 4, 5], [], [2, 3, 4, 5, 6], [], []], 32, 4, None),
    ("three-windows", [[1, 2, 3, 4, 5, 6], [3, 4, 5, 6, 7, 8], [5, 6, 7, 8, 9]], 32, 4, None),
    ("window-of-one", [[1, 2, 3], [3, 4]], 1, 1, None),
    ("window-of-64", [list(range(80)), list(range(20, 100))], 64, 4, None),
    ("min-match-zero", [[1, 2], [3, 4]], 32, 0, None),
    ("single-window", [[4, 5, 6]], 32, 4, None),
    ("no-window", [], 32, 4, None),
]


def random_merge_recordings(seed, n_recordings, window_tokens):
    """Recordings of overlapping windows cut from one random stream over a small alphabet (repeats are frequent), some windows noisy or empty."""
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n_recordings):
        stream = rng.integers(0, 6, 400).tolist()
        at, windows = 0, []
        for _ in range(int(rng.integers(0, 6))):
            length = int(rng.integers(0, 90))
            w = stream[at:at + length]
            if w and rng.random() < 0.3:
                w[int(rng.integers(0, len(w)))] = 99
            windows.append([] if rng.random() < 0.15 else w)
            at += max(0, length - int(rng.integers(0, window_tokens + 8)))
        recs.append(windows)
    return recs


WINDOW_PLANS = [   # (chunk, hop, samples, the windows) — the presets' numbers worked by hand from the loop
    (560_000, 480_000, 0, [(0, 0)]),
    (560_000, 480_000, 560_000, [(0, 560_000)]),
    (560_000, 480_000, 560_001, [(0, 560_000), (480_000, 80_001)]),
    (560_000, 480_000, 1_040_000, [(0, 560_000), (480_000, 560_000)]),
    (560_000, 480_000, 1_040_001, [(0, 560_000), (480_000, 560_000), (960_000, 80_001)]),
    (240_000, 192_000, 240_000, [(0, 240_000)]),
    (240_000, 192_000, 300_000, [(0, 240_000), (192_000, 108_000)]),
    (240_000, 192_000, 432_001, [(0, 240_000), (192_000, 240_000), (384_000, 48_001)]),
]
