"""The (hypothesis, reference) pairs the edit-distance tests share (tests/test_wer_emul.py on the CPU, tests/test_gpu_wer.py on the device):
lengths on every boundary of the kernel's schedule (csrc/wer_launch.h) and two families of symbols.  Test infrastructure.

Columns (reference length n): 64 C for C = 1, 2, 4, 8, 16 and one more or less — the class boundaries — then 1025 and 2049, the first
two- and three-panel lengths.  Rows (hypothesis length m): around 64, the block in which lane 0 is refilled, and past 128.  The table
work of the restatement over all of it stays below 3e6 cells."""
import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 257, 511, 513, 1023, 1024, 1025, 2049]
MS = [0, 1, 2, 63, 64, 65, 129, 200]
_SMALL, _LARGE = [0, 1, 2, 63, 64], [65, 129, 200]
# every n with one m up to 64 and one beyond; then the three-panel length with the rows that refill lane 0 once, not at all, three times
SHAPES = [(m, n) for i, n in enumerate(NS) for m in (_SMALL[i % 5], _LARGE[i % 3])] + [(1, 2049), (2, 2049)]
SHAPES_TIES_ONLY = [(64, 2049)]
SHAPES_EDITS_ONLY = [(200, 2049), (63, 2049)]


def tie_pair(rng, m, n, k):
    """An alphabet of 2 or 3 symbols — the extremes of int32 among them — where the traceback's ties are common."""
    alphabet = np.array([INT32_MIN, -1, INT32_MAX][:2 + k % 2], np.int64)
    return alphabet[rng.integers(0, alphabet.size, m)].astype(np.int32), alphabet[rng.integers(0, alphabet.size, n)].astype(np.int32)


def edited_pair(rng, m, n):
    """A reference over 1 000 symbols and a hypothesis of m symbols made from it by ~10 % substitutions, drops and insertions (past the
    reference's end: fresh symbols)."""
    alphabet = np.concatenate([[INT32_MIN, -1, INT32_MAX], rng.choice(np.arange(-500000, 500000), 997, replace=False)]).astype(np.int64)
    ref = alphabet[rng.integers(0, 1000, n)]
    hyp, j = [], 0
    while len(hyp) < m:
        u = rng.random()
        if j >= n or u < 0.033:
            hyp.append(alphabet[rng.integers(0, 1000)])           # an insertion
        elif u < 0.066:
            j += 1                                                # a drop
        elif u < 0.1:
            hyp.append(alphabet[rng.integers(0, 1000)])           # a substitution
            j += 1
        else:
            hyp.append(ref[j])
            j += 1
    return np.array(hyp, np.int64).astype(np.int32), ref.astype(np.int32)


def shape_pairs(seed=2024):
    """[(hyp, ref)] int32 arrays: both families on every shape."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k, (m, n) in enumerate(SHAPES + SHAPES_TIES_ONLY):
        pairs.append(tie_pair(rng, m, n, k))
    for m, n in SHAPES + SHAPES_EDITS_ONLY:
        pairs.append(edited_pair(rng, m, n))
    return pairs
