"""The float64 yardstick for the joint decisions of fa_tdt_greedy_logits_dev (csrc/tdt.hip: tdt_logits_fits_kernel<false, 1>, <true, 1>,
<true, 2> with the row in registers, tdt_logits_kernel<false>, <true> streaming it), the bound an emitted token's confidence is held to, a
float32 emulation of the kernels' summation order, and the table of cases that tests/test_tdt_logits_cpu.py and
tests/test_gpu_tdt_logits.py walk.  Plain numpy, no GPU.

A decision on a row of W >= V1 + nd logits (TdtModelInference.swift:84-188, LogitsArgmax.swift:16-55): the token is the first index of the
maximum of the V1 token logits (strict '>', NaN never wins, nothing above -inf: 0), the duration bin the same over the nd logits behind
them, the probability 1 / sum exp(x - max) over the token logits.  The entry hands back walks, not decisions: `diagonal` lays rows out so
that the walk decides on every one of them and emits what it decided."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

LANES = 64
FITS_LOGITS = 17 * LANES          # rows of up to 1 088 token logits stay in registers (kFitsLogits, csrc/tdt_route.h)
STREAM_BATCH = 16                 # the streaming kernels take sixteen logits per lane at a time: 1 024 per wavefront
F16_MAX = 65504.0
F32_BIG = 1e30
SCALES = (1.0, 3.0, 50.0)
FORMS = ("registers", "pairs", "streaming")
INSTANCES = ("f32_registers", "f16_halves", "f16_pairs", "f32_streaming", "f16_streaming")
BASE = 0x7F0000000000             # a 16-byte aligned device pointer
U24 = 2.0 ** -24                  # the relative error of one float32 rounding


# ---- the reference

def reference(rows, V1: int, nd: int):
    """(token, bin, prob) of [..., W] fp32 / fp16 rows, W >= V1 + nd; fp16 is widened first, everything behind that is float64.  prob is
    NaN where it is not finite by definition — a NaN among the token logits, a +inf token logit, nothing above -inf —: the walk's clamp
    makes that 0.  Elements at V1 + nd and behind are not looked at."""
    x = np.asarray(rows).astype(np.float64)
    assert x.shape[-1] >= V1 + nd and V1 >= 1 and nd >= 1
    tk, du = x[..., :V1], x[..., V1:V1 + nd]
    tclean, dclean = np.where(np.isnan(tk), -np.inf, tk), np.where(np.isnan(du), -np.inf, du)
    token = np.argmax(tclean, axis=-1).astype(np.int32)          # numpy's argmax is the first maximum; a row of -inf gives 0
    dbin = np.argmax(dclean, axis=-1).astype(np.int32)
    mx = tclean.max(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        prob = 1.0 / np.exp(tclean - mx).sum(axis=-1)
    undefined = np.isnan(tk).any(-1) | np.isposinf(tk).any(-1) | np.isneginf(mx[..., 0])
    return token, dbin, np.where(undefined, np.nan, prob)


def clamp(prob):
    """TdtDurationMapping.clampProbability in float64: NaN and +-inf become 0, the rest is cut to [0, 1]."""
    p = np.asarray(prob, np.float64)
    return np.where(np.isfinite(p), np.clip(p, 0.0, 1.0), 0.0)


def spread(prob, V1: int):
    """An upper bound on sum_i p_i (max - x_i), p the soft-max of the row, from its largest probability `prob` alone.  That sum is
    H(p) + ln(prob) (max - x_i = -ln(p_i / prob)), and with the largest probability fixed the entropy is greatest when the other V1 - 1
    share the rest evenly: (1 - prob) ln(prob (V1 - 1) / (1 - prob)).  0 for a flat row and for a certain one, at most ln V1."""
    p = np.asarray(prob, np.float64)
    with np.errstate(all="ignore"):
        e = (1.0 - p) * np.log(p * (V1 - 1) / (1.0 - p))
    return np.where(np.isfinite(e) & (e > 0.0), e, 0.0)


def tolerance(prob, V1: int, form: str):
    """Elementwise bound on |device confidence - clamp(reference prob)|:

        2**-24 * prob * (ceil(V1 / 64) + c),   c = 14 + 2.25 spread(prob, V1)   (+ 3 (ceil(V1 / 1024) - 1) for form "streaming")

    The device computes S = sum exp(x_i - M) and returns 1 / S, so a relative error of S is the same relative error of prob.  Every term
    is positive, so a relative error of a term or of a partial sum is at most that relative error of S.  In units of 2**-24, one float32
    rounding:

    - ceil(V1 / 64): the roundings on one lane's partial sum.  A lane of the one-logit-per-request kernels and of the streaming kernels
      adds its elements l, l + 64, ... in turn: at most ceil(V1 / 64) additions.  A lane of the pair kernel adds both halves of its pairs
      l, l + 64, ... (masked halves add an exact 0): at most 2 ceil(V1 / 128) <= ceil(V1 / 64) + 1, and that
    - 1 is part of c for every form.
    - 6: the six DPP additions of tdt_wave_softmax (four row shifts, two row broadcasts).
    - 5: a term reaches the sum as __expf(x - m) * __expf(m - M), m the lane's maximum (tdt_wave_softmax rescales once per lane): two
      hardware exponentials of one ulp = 2 each, and the rounding of the product, 1.
    - 3 (ceil(V1 / 1024) - 1), streaming only: the running sum is rescaled once per batch of 1 024 logits when the batch raises the
      lane's maximum — another hardware exponential, 2, and another product, 1; the first batch meets an empty sum and rounds nothing.
    - 2: the final reciprocal, one ulp.
    - 2.25 spread(prob, V1): __expf(d) is exp2(fl(log2e * d)) with d = fl(x - m).  The rounding of d changes the term by d 2**-24
      relative, the rounding of the product by another d 2**-24, and float32's log2e is 0.22 2**-24 away from log2 e: 2.25 d 2**-24
      for an exponent of size d.  The exponents along a term's chain (x - m, then m' - m'' of every rescale, then m - M) are all of one
      sign and add up to M - x_i, and the term's share of the sum is p_i / 1: together 2.25 sum_i p_i (M - x_i) <= 2.25 spread.
      A term far below the maximum has a large relative error and no share; one that the hardware flushes to zero (below 2**-126) is an
      absolute error of 2**-126 against a sum of at least 1.
    - Widening fp16 is exact, the maxima are exact, and comparing float32 with float64 adds nothing the reciprocal's ulp has not counted.

    c comes from this count alone.  The bound is a worst case — every rounding at its limit and in one direction —; roundings of random
    sign add up like the root of their number, which is why the float32 emulation below (whose exp, numpy's, is also correctly rounded
    where the hardware's is allowed a whole ulp) uses about a sixth of it on its worst row (tests/test_tdt_logits_cpu.py prints the figure).

    Where the reference is NaN the expected confidence is exactly 0 and the bound is 0."""
    assert form in FORMS
    p = np.asarray(prob, np.float64)
    c = 14.0 + 2.25 * spread(p, V1) + (3.0 * (math.ceil(V1 / (LANES * STREAM_BATCH)) - 1) if form == "streaming" else 0.0)
    return np.where(np.isfinite(p), U24 * p * (math.ceil(V1 / LANES) + c), 0.0)


# ---- the kernels' arithmetic, in float32 and in their order

def _wave_sum(t: np.ndarray) -> np.ndarray:
    """t [R, 64] float32 -> [R]: row_shr 1, 2, 4, 8 inside each row of sixteen lanes (a lane without that neighbour adds 0), row_bcast15
    into rows 1 and 3, row_bcast31 into rows 2 and 3; lane 63 holds the sum."""
    v = t.astype(np.float32).copy()
    lane = np.arange(LANES)
    for k in (1, 2, 4, 8):
        shifted = np.where(lane % 16 >= k, v[:, np.maximum(lane - k, 0)], np.float32(0.0))
        v = (v + shifted).astype(np.float32)
    v = (v + np.where((lane // 16) % 2 == 1, v[:, (lane // 16) * 16 - 1], np.float32(0.0))).astype(np.float32)
    v = (v + np.where(lane // 16 >= 2, v[:, [31]], np.float32(0.0))).astype(np.float32)
    return v[:, 63]


def _wave_softmax(m: np.ndarray, s: np.ndarray) -> np.ndarray:
    """tdt_wave_softmax and the reciprocal: lane maxima m and lane sums s [R, 64] -> 1 / sum [R]."""
    M = m.max(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        t = np.where(np.isneginf(m), np.float32(0.0), s * np.exp((m - M).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return (np.float32(1.0) / _wave_sum(t)).astype(np.float32)


def device_order_emulation(rows, V1: int, form: str) -> np.ndarray:
    """The kernels' soft-max in float32 and in their summation order, for [..., W] rows whose token logits are finite -> prob [...] float32.
    numpy's float32 exp stands in for __expf.

    "registers": lane l holds x[min(l + 64 j, V1 - 1)], j = 0 .. 16 — beyond the row a clamped duplicate of the last token logit, which
    enters the lane's maximum and not its sum —, adds exp(x - lane maximum) for ascending j, then the wave step.  "pairs": lane l holds
    the pairs at 2 (l + 64 j), j = 0 .. 8, clamped to the row's last pair; a half behind the last token logit is -inf unless it is the
    first half of a clamped pair (a duplicate again).  "streaming": per lane batches of sixteen x[l + 64 j + 1024 b]; the batch maximum,
    one rescale of the running sum when it rises, sixteen additions; the same wave step."""
    assert form in FORMS
    x = np.asarray(rows)
    shape = x.shape[:-1]
    x = x.astype(np.float32).reshape(-1, x.shape[-1])[:, :V1]
    assert np.isfinite(x).all()
    lane = np.arange(LANES)[:, None]
    last = V1 - 1
    ninf = np.float32(-np.inf)
    with np.errstate(all="ignore"):
        if form == "streaming":
            R = x.shape[0]
            m, s = np.full((R, LANES), ninf, np.float32), np.zeros((R, LANES), np.float32)
            for k0 in range(0, V1, LANES * STREAM_BATCH):
                idx = k0 + lane + LANES * np.arange(STREAM_BATCH)[None, :]                     # [64, 16]
                inrow = idx < V1
                v = np.where(inrow, x[:, np.minimum(idx, last)], ninf)                           # [R, 64, 16]
                bm = v.max(axis=2)
                up = bm > m
                rescaled = np.where(np.isneginf(m), np.float32(0.0), s * np.exp((m - bm).astype(np.float32)).astype(np.float32)).astype(np.float32)
                s, m = np.where(up, rescaled, s), np.where(up, bm, m)
                for j in range(STREAM_BATCH):
                    e = np.exp((v[:, :, j] - m).astype(np.float32)).astype(np.float32)
                    s = (s + np.where(inrow[:, j], e, np.float32(0.0))).astype(np.float32)
            return _wave_softmax(m, s).reshape(shape)
        assert V1 <= FITS_LOGITS
        if form == "registers":
            idx = lane + LANES * np.arange(17)[None, :]                                         # [64, 17]
            v = x[:, np.minimum(idx, last)]
        else:
            j = np.arange(18)[None, :]
            idx = 2 * (lane + LANES * (j // 2)) + j % 2                                          # index_of(j)
            lim = last // 2 * 2
            k = 2 * (lane + LANES * (j // 2))
            src = np.where(k < lim, k, lim) + j % 2                                              # the element the clamped request brings
            v = np.where((j % 2 == 0) | (idx <= last), x[:, np.minimum(src, last)], ninf)
        insum = idx <= last
        m = v.max(axis=2)
        s = np.zeros(m.shape, np.float32)
        for j in range(idx.shape[1]):
            e = np.exp((v[:, :, j] - m).astype(np.float32)).astype(np.float32)
            s = (s + np.where(insum[:, j], e, np.float32(0.0))).astype(np.float32)
        return _wave_softmax(m, s).reshape(shape)


# ---- the rows of the table: a kind of token logits and a pattern of duration logits

def winner_positions(V1: int):
    """Index 0, the last, the last but one; the even and the odd half of a pair; either side of a lane-piece boundary and of the
    piece-16 / piece-17 boundary (the first streaming batch ends there too)."""
    return sorted({p for p in (0, V1 - 1, V1 - 2, 10, 11, 63, 64, 1023, 1024) if 0 <= p < V1})


def tie_pairs(V1: int):
    """Exact ties inside a pair, across lanes, across the pieces of one lane (64 apart: one logit per request; 128 apart: pairs), across
    streaming batches, across the 1 023 / 1 024 boundary, and between the first and the last logit (every clamped request repeats the
    last one)."""
    seen = []
    for a, b in ((10, 11), (11, 12), (3, 67), (3, 131), (5, 1029), (1023, 1024), (0, V1 - 1)):
        if 0 <= a < b < V1 and (a, b) not in seen:
            seen.append((a, b))
    return seen


def token_kinds(V1: int, rows: str):
    """[(kind, category)] for a row list: "full" has every kind that fits V1, "short" one or two of each category."""
    if rows == "short":
        out = [("x1", "scale"), ("x3", "scale"), ("flat", "scale"), (f"win@{V1 - 1}", "winner")]
        if V1 >= 2:
            out += [(f"tie@0,{V1 - 1}", "winner"), ("one_nan", "nonfinite"), ("two_pinf", "nonfinite")]
        return out + [("all_ninf", "nonfinite"), ("all_nan", "nonfinite")]
    out = [("x1", "scale"), ("x3", "scale"), ("x50", "scale"), ("flat", "scale")]
    out += [(f"win@{p}", "winner") for p in winner_positions(V1)]
    out += [(f"tie@{a},{b}", "winner") for a, b in tie_pairs(V1)]
    out += [("all_nan", "nonfinite"), ("all_ninf", "nonfinite"), ("one_pinf", "nonfinite")]
    if V1 >= 2:
        out += [("one_nan", "nonfinite"), ("two_pinf", "nonfinite"), ("pinf_nan", "nonfinite")]
    if V1 >= 4:
        out += [("ninf_range", "nonfinite"), ("extremes", "nonfinite"), ("extremes_tie", "nonfinite")]
    return out


def token_row(kind: str, V1: int, f16: bool, rng) -> np.ndarray:
    """V1 token logits of the kind, as float32 values the row's dtype holds exactly."""
    dt = np.float16 if f16 else np.float32
    scale = {"x3": 3.0, "x50": 50.0}.get(kind, 1.0)
    x = (rng.standard_normal(V1) * scale).astype(dt).astype(np.float32)
    big = np.float32(F16_MAX if f16 else F32_BIG)
    top = np.float32(np.ceil(x.max()) + 2.5)
    if kind.startswith("win@"):
        x[int(kind[4:])] = top
    elif kind.startswith("tie@"):
        a, b = (int(w) for w in kind[4:].split(","))
        x[a] = x[b] = top
    elif kind == "flat":
        x[:] = 0.75
    elif kind == "all_nan":
        x[:] = np.nan
    elif kind == "one_nan":
        x[V1 // 2] = np.nan
    elif kind == "all_ninf":
        x[:] = -np.inf
    elif kind == "ninf_range":
        x[V1 // 4:3 * V1 // 4] = -np.inf
    elif kind == "one_pinf":
        x[V1 // 3] = np.inf
    elif kind == "two_pinf":
        x[V1 // 3] = x[V1 - 1] = np.inf
    elif kind == "pinf_nan":
        x[0], x[V1 - 1] = np.nan, np.inf
    elif kind == "extremes":
        x[0] = x[V1 - 1] = -big
        x[V1 // 2] = big
    elif kind == "extremes_tie":
        x[0] = x[V1 - 1] = -big
        x[1] = x[V1 - 2] = big
    else:
        assert kind in ("x1", "x3", "x50"), kind
    return x.astype(dt).astype(np.float32)


def duration_patterns(nd: int, target: int):
    """The ways the nd duration logits select `target`: by a margin, as the first of equal maxima, beside NaN or -inf everywhere else,
    and — bin 0 only — with nothing above -inf and with nothing but NaN."""
    out = ["margin", "tie", "nan_others", "ninf_others"]
    if target == 0:
        out += ["all_ninf", "all_nan"]
    return out


def duration_row(pattern: str, nd: int, target: int, top: float, f16: bool, rng) -> np.ndarray:
    """nd duration logits.  `top` is the largest finite token logit: "dominate_all" puts every duration logit 20 above it or a little more (the target 21),
    "dominate_first" the first one only."""
    dt = np.float16 if f16 else np.float32
    d = rng.standard_normal(nd).astype(np.float32)
    if pattern == "margin":
        d[target] = np.ceil(d.max()) + 6.0
    elif pattern == "tie":
        d[:target] -= 8.0
        d[target:] = 4.0
    elif pattern in ("nan_others", "ninf_others"):
        d[:] = np.nan if pattern == "nan_others" else -np.inf
        d[target] = -3.0
    elif pattern == "all_ninf":
        d[:] = -np.inf
    elif pattern == "all_nan":
        d[:] = np.nan
    elif pattern == "dominate_all":
        d[:] = np.ceil(top) + 20.0                     # (whole numbers: fp16 holds them exactly)
        d[target] = np.ceil(top) + 21.0
    else:
        assert pattern == "dominate_first" and target == 0, (pattern, target)
        d[0] = np.ceil(top) + 20.0
    return d.astype(dt).astype(np.float32)


# ---- the case table: one Call is one call of the entry

@dataclasses.dataclass(frozen=True)
class Call:
    name: str
    category: str                  # boundary | nd | padding | offset
    f16: bool
    V1: int
    nd: int = 5
    target: int = 1                # the duration bin every row of the call selects; its duration is 1
    pad: int = 0                   # row_stride - (V1 + nd)
    off: int = 0                   # elements between a 16-byte boundary and the matrix
    rows: str = "short"

    @property
    def np_dtype(self):
        return np.float16 if self.f16 else np.float32

    @property
    def W(self) -> int:
        return self.V1 + self.nd + self.pad

    @property
    def duration_bins(self) -> tuple:
        """The reference's map (0, 1, 2, 3, 4) where it gives the target duration 1; else 1 for the target and 2, 3, ... for the others:
        a wrong bin shows as a wrong duration and a walk that leaves the diagonal."""
        if self.nd == 5 and self.target == 1:
            return (0, 1, 2, 3, 4)
        others = iter(range(2, 2 + self.nd))
        return tuple(1 if b == self.target else next(others) for b in range(self.nd))

    @property
    def base(self) -> "Call":
        """The contiguous, aligned call on the same rows."""
        return dataclasses.replace(self, name=f"base_{'f16' if self.f16 else 'f32'}_V{self.V1}_nd{self.nd}_bin{self.target}_{self.rows}",
                                   category="base", pad=0, off=0)

    def instance(self, tdt_route) -> str:
        route = tdt_route(self.f16, self.V1, self.W, BASE + self.off * (2 if self.f16 else 4))
        dt = "f16" if self.f16 else "f32"
        return f"{dt}_streaming" if route == 0 else ("f16_pairs" if route == 2 else ("f16_halves" if self.f16 else "f32_registers"))

    def form(self, tdt_route) -> str:
        return {"f32_registers": "registers", "f16_halves": "registers", "f16_pairs": "pairs"}.get(self.instance(tdt_route), "streaming")


BOUNDARY_V1 = (1, 2, 63, 64, 65, 128, 129, 1024, 1025, 1087, 1088, 1089, 2048, 2049, 8193)
ND_TARGETS = ((1, 0), (2, 0), (2, 1), (5, 0), (5, 4), (8, 0), (8, 7))
PADS = (0, 1, 2, 3, 7)
OFFSETS = (0, 1, 2, 3)             # elements: 0, 2, 4, 6 bytes for fp16 and 0, 4, 8, 12 bytes for fp32
LAYOUT_ROWS = ((False, 1025), (True, 1025), (False, 1089), (True, 1089))


def _calls():
    out = []
    for V1 in BOUNDARY_V1:         # every V1 on the fp32 instance and, where the row fits the registers, on both fp16 ones
        out.append(Call(f"boundary_f32_V{V1}", "boundary", False, V1, rows="full"))
        out.append(Call(f"boundary_f16_V{V1}", "boundary", True, V1, rows="full"))
        out.append(Call(f"boundary_f16_V{V1}_pad1", "boundary", True, V1, pad=1, rows="full"))
    for nd, target in ND_TARGETS:
        even = (129 + nd) % 2      # the pad that makes an fp16 row of 129 + nd logits even: pairs; the other one: halves
        for f16, V1, pad, tag in ((False, 129, 0, "f32"), (True, 129, even, "f16_pairs"), (True, 129, 1 - even, "f16_halves"),
                                  (False, 1100, 0, "f32_stream"), (True, 1100, 0, "f16_stream")):
            out.append(Call(f"nd{nd}_bin{target}_{tag}", "nd", f16, V1, nd=nd, target=target, pad=pad))
    for f16, V1 in LAYOUT_ROWS:
        dt = "f16" if f16 else "f32"
        out += [Call(f"pad{pad}_{dt}_V{V1}", "padding", f16, V1, pad=pad) for pad in PADS]
        out += [Call(f"off{off}_{dt}_V{V1}", "offset", f16, V1, off=off) for off in OFFSETS]
    return tuple(out)


CALLS = _calls()
BY_NAME = {c.name: c for c in CALLS}
assert len(BY_NAME) == len(CALLS)
CALL_CATEGORIES = ("boundary", "nd", "padding", "offset")
ROW_CATEGORIES = ("scale", "winner", "nonfinite", "dominate")


def of_category(category: str):
    return [c for c in CALLS if c.category == category]


def row_specs(call: Call):
    """[(token kind, row category, duration pattern)]: the call's token kinds, each with the next duration pattern in turn, then the rows
    whose duration logits dominate — on a random row, on a winner in the last slot and in the last but one, on a first / last tie —, then
    random rows until every pattern has been used and a last one for the cell the walk decides and does not emit."""
    patterns = duration_patterns(call.nd, call.target)
    specs = [(kind, cat, patterns[i % len(patterns)]) for i, (kind, cat) in enumerate(token_kinds(call.V1, call.rows))]
    V1 = call.V1
    dominated = ["x1", f"win@{V1 - 1}"] + ([f"win@{V1 - 2}", f"tie@0,{V1 - 1}"] if V1 >= 2 else [])
    for kind in dominated:
        specs.append((kind, "dominate", "dominate_all"))
        if call.target == 0:
            specs.append((kind, "dominate", "dominate_first"))
    while len(specs) < len(patterns):
        specs.append(("x1", "scale", patterns[len(specs) % len(patterns)]))
    return specs


def poison(n: int, dtype, start: int = 0) -> np.ndarray:
    """+inf, NaN and the dtype's largest finite value in turn."""
    big = F32_BIG if dtype == np.float32 else F16_MAX
    return np.array([np.inf, np.nan, big], dtype)[(start + np.arange(n)) % 3]


@dataclasses.dataclass
class Diagonal:
    call: Call
    logits: np.ndarray             # [B, T, T, W] of the call's dtype: case row k of chunk b at (b, k, k), other random rows elsewhere
    specs: list                    # [B][T] (token kind, row category, duration pattern)
    token: np.ndarray              # [B, T] reference decisions of the diagonal
    dbin: np.ndarray
    prob: np.ndarray               # float64; NaN where undefined

    @property
    def B(self) -> int:
        return self.logits.shape[0]

    @property
    def T(self) -> int:
        return self.logits.shape[1]


def diagonal(call: Call) -> Diagonal:
    """The call's rows as chunks the walk decides row by row.  With blank_id = -1 nothing is a blank, every row selects the bin whose
    duration is 1, is_last = 0 and U == T == enc_len: the walk visits (k, k), k = 0 .. T - 1, and emits token k at time k for k <= T - 2.
    The rows depend on (dtype, V1, nd, target, row list) only: a padded or offset call decides on the rows of its base call."""
    specs = row_specs(call)
    t_max = 17 if call.V1 > FITS_LOGITS else 33
    B = -(-len(specs) // (t_max - 1))                  # - 1: each chunk ends with a cell that is decided and not emitted
    per = -(-len(specs) // B)
    T = per + 1
    patterns = duration_patterns(call.nd, call.target)
    while len(specs) < B * per:
        specs.append(("x3", "scale", patterns[len(specs) % len(patterns)]))
    rng = np.random.default_rng([call.V1, int(call.f16), call.nd, call.target, len(specs)])
    V1, nd, W, dt = call.V1, call.nd, call.W, call.np_dtype
    lg = np.empty((B, T, T, W), dt)
    lg[..., :V1 + nd] = (rng.standard_normal((B, T, T, V1 + nd), dtype=np.float32) * 3.0).astype(dt)
    if call.pad:
        lg[..., V1 + nd:] = poison(B * T * T * call.pad, dt, call.pad).reshape(B, T, T, call.pad)
    grid = [[None] * T for _ in range(B)]
    for b in range(B):
        for k in range(T):
            spec = specs[b * per + k] if k < per else ("x1", "scale", "margin")
            x = token_row(spec[0], V1, call.f16, rng)
            finite = x[np.isfinite(x)]
            d = duration_row(spec[2], nd, call.target, float(finite.max()) if finite.size else 0.0, call.f16, rng)
            lg[b, k, k, :V1], lg[b, k, k, V1:V1 + nd] = x.astype(dt), d.astype(dt)
            grid[b][k] = spec
    idx = np.arange(T)
    token, dbin, prob = reference(lg[:, idx, idx], V1, nd)
    return Diagonal(call, lg, grid, token, dbin, prob)


def decision_tables(d: Diagonal):
    """tok / bin / prob [B, T, T] for the oracle: the reference on the diagonal; elsewhere the token and the bin of the random rows (finite:
    a float32 argmax is the reference's) and an undefined probability — a walk that left the diagonal would emit other tokens, with
    confidence 0."""
    V1, nd = d.call.V1, d.call.nd
    x = d.logits[..., :V1 + nd].astype(np.float32)
    tok, bn = np.argmax(x[..., :V1], -1).astype(np.int32), np.argmax(x[..., V1:], -1).astype(np.int32)
    prob = np.full(tok.shape, np.nan, np.float32)
    idx = np.arange(d.T)
    with np.errstate(invalid="ignore"):                 # all-NaN rows: argmax of NaN is not the reference's 0
        tok[:, idx, idx], bn[:, idx, idx], prob[:, idx, idx] = d.token, d.dbin, d.prob.astype(np.float32)
    return tok, bn, prob


def expected_walks(d: Diagonal, oracle_mod):
    """The oracle on decision_tables, one dict per chunk, after the check that makes every row of the table a compared decision: status 0,
    T - 1 tokens, which are the reference's diagonal with timestamps 0 .. T - 2 and duration 1, final_u = T - 1, final_time = T."""
    tok, bn, prob = decision_tables(d)
    T, call = d.T, d.call
    assert (d.dbin == call.target).all(), (call.name, np.argwhere(d.dbin != call.target)[:4].tolist())
    assert call.duration_bins[call.target] == 1 and sorted(call.duration_bins).count(1) == 1
    out = []
    for b in range(d.B):
        r = oracle_mod.tdt_greedy(tok[b], bn[b], prob[b], T, None, 0, False, 0, None, blank_id=-1, bins=call.duration_bins, max_out=T)
        assert (r["status"], r["count"], r["final_u"], r["final_time"]) == (0, T - 1, T - 1, T), (call.name, b, r)
        assert r["tokens"].tolist() == d.token[b, :T - 1].tolist() and r["timestamps"].tolist() == list(range(T - 1)), (call.name, b)
        assert r["durations"].tolist() == [1] * (T - 1), (call.name, b)
        np.testing.assert_array_equal(r["confidences"], clamp(d.prob[b, :T - 1]).astype(np.float32), err_msg=f"{call.name} chunk {b}")
        out.append(r)
    return out


def compare_walks(got, d: Diagonal, expected, form: str):
    """The entry's result for the call against `expected`: integers exactly, every confidence within `tolerance` of the clamped reference,
    exactly 0.0 where the reference is undefined.  Returns the largest |error| / tolerance."""
    T, V1 = d.T, d.call.V1
    worst = 0.0
    assert len(got) == d.B
    for b, (g, r) in enumerate(zip(got, expected)):
        where = f"{d.call.name} chunk {b}"
        assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (r["status"], r["count"], r["final_u"], r["final_time"]), where
        for key in ("tokens", "timestamps", "durations"):
            np.testing.assert_array_equal(g[key], r[key], err_msg=f"{where} {key} {d.specs[b]}")
        conf = np.asarray(g["confidences"])
        assert conf.dtype == np.float32 and conf.shape == (T - 1,)
        ref = d.prob[b, :T - 1]
        undefined = ~np.isfinite(ref)
        assert (conf[undefined] == 0.0).all(), (where, [d.specs[b][k] for k in np.flatnonzero(undefined & (conf != 0.0))])
        tol = tolerance(ref, V1, form)
        err = np.abs(conf.astype(np.float64) - clamp(ref))
        ratio = np.where(undefined, 0.0, err / np.where(undefined, 1.0, tol))
        k = int(ratio.argmax())
        assert ratio[k] <= 1.0, f"{where} row {k} {d.specs[b][k]}: confidence {conf[k]!r}, reference {ref[k]!r}, |error| / tolerance {ratio[k]:.3f}"
        worst = max(worst, float(ratio[k]))
    return worst
