"""The decode calls tests/test_gpu_rnnt.py runs, built so that the decisions of interest occur, and the restatement's answers for them
(computed once per call and left alone).  tests/test_rnnt_cpu.py proves from the restatement alone that every call holds at least one
decision of each kind of KINDS.  No GPU, no product code.

A call is a batch of streams over one vocabulary.  Every stream is written by a small program that fills the row the walk will read
next so that the wanted decision happens there, follows the decision with the restatement's own pieces, and goes on; the cells off the
path keep a background the walk never reads.  All logits are multiples of 1/64 of magnitude below 64 (NaN and -inf apart): exact in
fp16, far from denormals, and every logit + boost is exact in fp32 — where a test wants a tie or an equality, it is one.

The vocabulary at vocab_with_blank >= 129 (ids spread over the row so that every piece of it matters):
  A = V1 - 3 "▁ab", A2 = 3 "▁AB" (a case twin: same folded piece, same boost), C = 64 "▁c", X = 100 "▁x" (continues nothing),
  L = 7 a piece of 32 scalars (fills the tail), Z = 66 "▁zzz" and Z2 = 67 "zzz" (the long form's pieces), 5 "<unk>" (special), 0 without a
  piece, eou = V1 - 2, blank = V1 - 1.  Terms: "ab c" (4.5), "c ab" (5.5: A is worth more behind C than at a fresh start) and, in the
  calls marked long, "z" * 69 (2.0): a form of 70 scalars, so tail_cap = 70 > 64.
At vocab_with_blank = 3 — the shape of the reference's pickBiased rows — there are three ids.  A continuation needs two tokens with a piece
and the loop needs blank, so a call with an end-of-utterance token cannot hold the matcher's kinds: the kinds are split over two calls,
V3 (A = 0, C = 1, blank = 2, no eou) with every kind but eou_mid_chunk, and V3_eou (A = 0, eou = 1, blank = 2) with that one."""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_restatement as R  # noqa: E402

MAX_SYMBOLS = 3
PAD = 5                       # row_stride - vocab_with_blank; the padding holds 50.0, which would win every argmax that read it
KINDS = ("plain_nonblank", "blank_overtaken", "nonblank_overtaken", "equal_no_flip", "tie_lowest_id", "continuation_flip", "continuation_dropped",
         "candidate_nan_or_inf", "all_nan_row", "symbol_cap", "eou_mid_chunk", "skip_past_end", "u_exhausted", "max_out_exhausted", "tail_trimmed")


def vocabulary(V1, variant, long):
    if variant == "V3":
        return SimpleNamespace(pieces={0: "▁ab", 1: "▁c"}, terms=[("ab c", None), ("c ab", 5.5)], A=0, C=1, blank=2, eou=-1, V1=3)
    if variant == "V3_eou":
        return SimpleNamespace(pieces={0: "▁ab"}, terms=[("ab c", None)], A=0, blank=2, eou=1, V1=3)
    pieces = {V1 - 3: "▁ab", 3: "▁AB", 64: "▁c", 100: "▁x", 7: "q" * 32, 66: "▁zzz", 67: "zzz", 5: "<unk>"}
    terms = [("ab c", None), ("c ab", 5.5)] + ([("z" * 69, 2.0)] if long else [])
    return SimpleNamespace(pieces=pieces, terms=terms, A=V1 - 3, A2=3, C=64, X=100, L=7, Z=66, Z2=67, R0=0, blank=V1 - 1, eou=V1 - 2, V1=V1)


class Stream:
    """One stream under construction: the walk's position, the restatement's match state, and the rows it will read."""

    def __init__(self, rng, v, U, T, frames, skip):
        self.v, self.U, self.T, self.frames, self.skip = v, U, T, frames, skip
        self.x = -(6.0 + rng.integers(0, 193, (U, T, v.V1 + PAD)) / 64.0)        # background in [-9, -6]: no boost lifts it to a plain logit of 2
        self.x[:, :, v.V1:] = 50.0
        self.bias = R.VocabularyBias(v.terms, v.pieces)
        self.max_t = max(0, min(frames, T))
        self.u, self.t, self.symbols, self.done = 0, min(skip, self.max_t), 0, False

    def row(self):
        assert not self.done and self.u < self.U and self.t < self.max_t, (self.u, self.t)
        return self.x[self.u, self.t]

    def decide(self):
        row = self.row()[:self.v.V1].astype(np.float32)
        plain = R.argmax_first(row)
        picked = R.pick_biased(plain, self.bias.candidates(), row)
        if picked == self.v.blank:
            self.t, self.symbols = self.t + 1, 0
        elif picked == self.v.eou:
            self.done = True
        else:
            self.bias.observe(picked)
            self.u, self.symbols = self.u + 1, self.symbols + 1
            if self.symbols == MAX_SYMBOLS:
                self.t, self.symbols = self.t + 1, 0
        return plain, picked

    def boost(self, cand):
        return float(self.bias.candidates()[cand])

    def plain(self, tok):                       # the plain argmax, taken
        self.row()[tok] = 2.0
        assert self.decide() == (tok, tok)

    def flip(self, plain, cand):                # the boosted candidate beats the plain argmax by 1/8
        row = self.row()
        row[plain], row[cand] = 2.0, 2.125 - self.boost(cand)
        assert self.decide() == (plain, cand)

    def equal(self, plain, cand):               # the boosted candidate EQUALS the plain logit: no flip
        row = self.row()
        row[plain], row[cand] = 2.0, 2.0 - self.boost(cand)
        assert self.decide() == (plain, plain)

    def tie(self, plain, low, high):            # two candidates with one score above the plain logit: the lowest id
        row = self.row()
        row[plain], row[low], row[high] = 2.0, 2.5 - self.boost(low), 2.5 - self.boost(high)
        assert low < high and self.decide() == (plain, low)

    def poisoned(self, plain, cand, value):     # a candidate whose logit is NaN or -inf
        row = self.row()
        row[plain], row[cand] = 2.0, value
        assert cand in self.bias.candidates() and self.decide() == (plain, plain)

    def all_nan(self):
        self.row()[:self.v.V1] = np.nan
        assert self.decide() == (0, 0)

    def blanks(self):                           # blank to the end of the chunk
        while not self.done and self.t < self.max_t and self.u < self.U:
            self.plain(self.v.blank)


def matcher_stream(rng, v, U, T, eou_at):
    """Every decision kind of the matcher, the symbol cap, and — where the vocabulary has one — an end of utterance mid-chunk."""
    s = Stream(rng, v, U, T, T, 0)
    if v.V1 == 3:
        s.plain(v.A)                            # t 0: plain non-blank; "▁ab" is live: C continues it
        s.tie(v.blank, v.A, v.C)                # blank overtaken, two equal candidates: A, the lower id; the old "▁ab" dies on it
        s.flip(v.blank, v.C)                    # only the continuation offers C; third symbol of the frame: the cap
        s.plain(v.C)                            # t 1: "▁c▁c" is no form: the live "▁c" is dropped
        s.flip(v.C, v.A)                        # a non-blank plain argmax overtaken (A behind "▁c": 5.5)
        s.plain(v.blank)
    else:
        s.plain(v.A)                            # t 0: plain non-blank; "▁ab" is live
        s.flip(v.blank, v.C)                    # blank overtaken by what only the continuation offers
        s.tie(v.X, v.A2, v.A)                   # a non-blank plain argmax overtaken; the case twins tie: the lower id; the cap
        s.plain(v.X)                            # t 1: "▁x" continues nothing: the live "▁ab" is dropped
        s.plain(v.A)
        s.plain(v.blank)
    s.equal(v.blank, v.C)                       # "▁ab" is live again
    s.poisoned(v.blank, v.C, np.nan)
    s.poisoned(v.blank, v.C, -np.inf)
    s.flip(v.blank, v.C)                        # frames after "▁ab" was emitted: a chunk split in between has to carry the tail
    s.all_nan()                                 # emits id 0
    s.plain(v.blank)
    if v.V1 > 3:
        for _ in range(3):
            s.plain(v.L)                        # 96 scalars: the tail is trimmed at any tail_cap up to 70
        while s.t < eou_at:
            s.plain(v.blank)
        s.plain(v.eou)
    else:
        s.blanks()
    return s


def eou_stream(rng, v, U, T):
    s = Stream(rng, v, U, T, T - 2, 1)
    s.plain(v.A)
    s.plain(v.blank)
    if v.V1 == 3:
        s.flip(v.blank, v.A)
    else:
        s.flip(v.blank, v.A2)
        s.plain(v.R0)
    s.plain(v.blank)
    s.plain(v.eou)
    return s


def exhausting_stream(rng, v, U, T):
    """MAX_SYMBOLS tokens per frame until a decision is needed at u = U; with max_out < U the outputs run out first."""
    s = Stream(rng, v, U, T, T, 0)
    while s.u < U:
        s.plain(v.A)
    assert s.t < s.max_t
    return s


def long_match_stream(rng, v, U, T):
    """Two pieces of 32 scalars, then a match that opens at ring slot 64 — a suffix start of the second pass — and grows through the trim."""
    s = Stream(rng, v, U, T, T - 1, 2)
    s.plain(v.L)
    s.plain(v.L)
    s.flip(v.blank, v.Z) if v.Z in s.bias.candidates() else s.plain(v.Z)
    while s.u < U - 2 and s.t < s.max_t - 1:
        s.flip(v.blank, v.Z2) if v.Z2 in s.bias.candidates() else s.plain(v.Z2)
        s.plain(v.blank) if s.symbols else None
    s.blanks()
    return s


def random_stream(rng, v, U, T):
    """Rows of random eighths with many equal values, blank on top of half of them: whatever decisions follow."""
    s = Stream(rng, v, U, T, T, 0)
    s.x[:, :, :v.V1] = rng.integers(-32, 33, (U, T, v.V1)) / 8.0
    top = rng.random((U, T)) < 0.5
    s.x[:, :, v.blank][top] = 4.5
    return s


class Call:
    def __init__(self, name, V1, f16, variant="general", long=False, B=6, U=16, T=12, seed=0):
        self.name, self.V1, self.f16, self.variant, self.long, self.B, self.U, self.T, self.seed = name, V1, f16, variant, long, B, U, T, seed
        self.max_out = U - 4
        self.kinds = {"V3": [k for k in KINDS if k != "eou_mid_chunk"], "V3_eou": ["plain_nonblank", "blank_overtaken", "eou_mid_chunk", "skip_past_end",
                                                                                   "u_exhausted", "max_out_exhausted", "symbol_cap"]}.get(variant, list(KINDS))


CALLS = [Call(f"{'f16' if f16 else 'f32'}_{tag}", V1, f16, variant, long, B, U, T, seed)
         for f16 in (False, True)
         for tag, V1, variant, long, B, U, T, seed in (("V3", 3, "V3", False, 6, 16, 12, 1), ("V3_eou", 3, "V3_eou", False, 6, 16, 12, 2),
                                                        ("V129", 129, "general", False, 6, 16, 12, 3), ("V1025_long", 1025, "general", True, 6, 16, 12, 4),
                                                        ("V8193_long", 8193, "general", True, 3, 12, 10, 5))]
BY_NAME = {c.name: c for c in CALLS}
_TABLES = {}


def table(call):
    """The call's inputs and the restatement's answers: logits [B][U][T][W] in the call's element type, frames, skip, the vocabulary,
    per stream `expected` (what the entry returns) and `trace` (one dict per decision, rnnt_restatement.greedy)."""
    if call.name in _TABLES:
        return _TABLES[call.name]
    rng = np.random.default_rng(call.seed)
    v = vocabulary(call.V1, call.variant, call.long)
    U, T = call.U, call.T
    if call.variant == "V3_eou":
        streams = [eou_stream(rng, v, U, T), Stream(rng, v, U, T, 5, 7), exhausting_stream(rng, v, U, T), eou_stream(rng, v, U, T), random_stream(rng, v, U, T),
                   random_stream(rng, v, U, T)]
    else:
        streams = [matcher_stream(rng, v, U, T, T - 3), Stream(rng, v, U, T, 5, 7), exhausting_stream(rng, v, U, T)]
        if call.B == 6:
            streams += [eou_stream(rng, v, U, T) if v.eou >= 0 else random_stream(rng, v, U, T),
                        long_match_stream(rng, v, U, T) if v.V1 > 3 else random_stream(rng, v, U, T), random_stream(rng, v, U, T)]
    assert len(streams) == call.B
    logits = np.stack([s.x for s in streams]).astype(np.float16 if call.f16 else np.float32)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(logits.astype(np.float64), np.stack([s.x for s in streams]), equal_nan=True)      # exact in the element type
    finite = logits[np.isfinite(logits)].astype(np.float64)
    assert np.all((finite == 0) | (np.abs(finite) >= 2.0 ** -14))                                                # no denormals, fp16's included
    t = SimpleNamespace(call=call, v=v, logits=logits, frames=[s.frames for s in streams], skip=[s.skip for s in streams], B=call.B,
                        W=call.V1 + PAD, expected=[], trace=[])
    for b in range(call.B):
        trace = []
        t.expected.append(run(t, b, trace=trace))
        t.trace.append(trace)
    _TABLES[call.name] = t
    return t


def new_bias(t, terms=None):
    return R.VocabularyBias(t.v.terms if terms is None else terms, t.v.pieces)


def run(t, b, bias="own", frames=None, skip=None, logits=None, max_out=None, trace=None):
    """The restatement on stream b of table t."""
    bias = new_bias(t) if isinstance(bias, str) else bias
    return R.greedy(t.logits[b] if logits is None else logits, t.call.V1, t.frames[b] if frames is None else frames, t.skip[b] if skip is None else skip,
                    bias=bias, blank_id=t.v.blank, eou_id=t.v.eou, max_symbols=MAX_SYMBOLS, max_out=t.call.max_out if max_out is None else max_out, trace=trace)


def kinds_of(t, b):
    """The kinds stream b of table t holds, from the restatement's trace and answer alone."""
    r, trace, v, call = t.expected[b], t.trace[b], t.v, t.call
    max_t = max(0, min(t.frames[b], call.T))
    found = set()
    per_frame = {}
    for e in trace:
        row, plain, picked, cands = e["row"], e["plain"], e["picked"], {i: c for i, c in e["candidates"].items() if i < call.V1}
        with np.errstate(invalid="ignore", over="ignore"):
            scores = {i: np.float32(row[i] + np.float32(c)) for i, c in cands.items()}
        if e["emitted"]:
            per_frame[e["t"]] = per_frame.get(e["t"], 0) + 1
        if picked == plain and e["emitted"]:
            found.add("plain_nonblank")
        if picked != plain:
            found.add("blank_overtaken" if plain == v.blank else "nonblank_overtaken")
            if sum(1 for i in scores if scores[i] == scores[picked]) >= 2 and picked == min(i for i in scores if scores[i] == scores[picked]):
                found.add("tie_lowest_id")
            if R.pick_biased(plain, {i: c for i, c in e["fresh"].items()}, row) == plain:
                found.add("continuation_flip")
        if picked == plain and any(i != plain and s == row[plain] for i, s in scores.items()):
            found.add("equal_no_flip")
        if any(np.isnan(row[i]) or row[i] == -np.inf for i in cands) and not np.all(np.isnan(row)):
            found.add("candidate_nan_or_inf")
        if np.all(np.isnan(row)):
            found.add("all_nan_row")
        if e["dropped"]:
            found.add("continuation_dropped")
        if e["trimmed"]:
            found.add("tail_trimmed")
    if any(n == MAX_SYMBOLS for n in per_frame.values()):
        found.add("symbol_cap")
    if r["eou"] and trace[-1]["t"] < max_t - 1:
        found.add("eou_mid_chunk")
    if t.skip[b] >= max_t and not trace:
        found.add("skip_past_end")
    if r["status"] == R.OUTPUT_TOO_SMALL and r["final_u"] == call.U:
        found.add("u_exhausted")
    if r["count"] > call.max_out:
        found.add("max_out_exhausted")
    return found
