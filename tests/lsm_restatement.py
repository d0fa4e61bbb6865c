"""The float64 yardstick for fa_ctc_log_softmax_batch_dev (csrc/ctc.hip: ctc_log_softmax_vec4_kernel, ctc_log_softmax_kernel<F16> in its
register and its streaming form), the bound the device is held to, a float32 emulation of the device's summation order that shows the bound
is neither loose nor out of reach, and the table of cases that tests/test_lsm_cpu.py and tests/test_gpu_ctc_log_softmax.py walk.
Plain numpy, no GPU.

The operation is makeLogProbs / logSoftmax of the reference (CtcKeywordSpotter+Inference.swift:350-431): x / temperature (skipped when the
temperature is 1), the row maximum, the sum of exp(x - max), (x - max) - log(sum), then blankBias subtracted from the blank column."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

LANES = 64
REG_LIMIT = 2048                  # 64 lanes x kLsmRegs values: the row stays in registers up to here, three streaming passes above
B, T = 3, 7                       # 21 rows: six workgroups of four wavefronts, the last one with three idle wavefronts
SCALES = (1.0, 3.0, 50.0)
SETTINGS = ((1.0, 0.0), (1.7, 2.5), (0.05, 0.5))       # (temperature, blank bias)
F16_MAX = 65504.0


def scaled(x, temperature) -> np.ndarray:
    """The reference's input to the softmax: float32(x) / float32(temperature), rounded to float32; no division at temperature 1."""
    x32 = np.asarray(x).astype(np.float32)
    t = np.float32(temperature)
    with np.errstate(all="ignore"):
        return x32 if t == np.float32(1.0) else (x32 / t).astype(np.float32)


def bias_applies(blank_bias, blank_id, V) -> bool:
    return np.float32(blank_bias) != np.float32(0.0) and 0 <= blank_id < V


def reference(x, temperature=1.0, blank_bias=0.0, blank_id=-1) -> np.ndarray:
    """The float64 answer for [..., V] fp32 / fp16 logits.  Everything behind the float32 quotient is float64.  Rows that are not finite by
    definition get their defined result: a NaN anywhere, a +inf, or nothing but -inf make the row all NaN (inf - inf or NaN in the sum);
    a -inf element of an otherwise finite row is -inf (its probability is 0)."""
    v = scaled(x, temperature).astype(np.float64)
    V = v.shape[-1]
    with np.errstate(all="ignore"):
        finite_max = np.max(np.where(np.isfinite(v), v, -np.inf), axis=-1, keepdims=True)
        d = v - finite_max
        lse = np.log(np.sum(np.exp(np.where(np.isfinite(d), d, -np.inf)), axis=-1, keepdims=True))
        out = d - lse
    if bias_applies(blank_bias, blank_id, V):
        out[..., blank_id] -= np.float64(np.float32(blank_bias))
    undefined = np.isnan(v).any(-1) | np.isposinf(v).any(-1) | np.isneginf(v).all(-1)
    out[undefined] = np.nan
    return out


def tolerance(ref, V) -> np.ndarray:
    """Elementwise bound on |device - reference|: 2**-24 * (ceil(V / 64) + 52 + 3 |ref|), in units of 2**-24 (half a float32 ulp at 1):

    - ceil(V / 64) + 6: the roundings on one lane's partial sum (it adds elements l, l + 64, ...) plus the six steps of the xor tree.  Every
      term is positive, so this relative error of the sum is an absolute error of log(sum).  The vec4 form has fewer roundings.
    - 4: one ulp of expf, again relative to a positive sum.
    - 10: the rounding of x - max carried through exp, weighted by the probabilities: at most ln V.
    - 32: two ulp of logf where log(sum) <= 16.
    - 3 |ref|: the roundings of x - max, of the final subtraction and of the blank bias, each half an ulp of a number no larger than |ref|.

    A non-finite reference element has no bound (the comparison there is on the pattern); it counts as 0 here."""
    a = np.abs(np.asarray(ref, np.float64))
    a = np.where(np.isfinite(a), a, 0.0)
    return 2.0 ** -24 * (math.ceil(V / LANES) + 52 + 3.0 * a)


def _lane_sums(e: np.ndarray) -> np.ndarray:
    """e [R, N] float32 -> [R, 64]: lane l adds e[l], e[l + 64], ... in that order, in float32."""
    R, N = e.shape
    steps = -(-N // LANES)
    padded = np.zeros((R, steps * LANES), np.float32)
    padded[:, :N] = e
    padded = padded.reshape(R, steps, LANES)
    s = np.zeros((R, LANES), np.float32)
    for j in range(steps):
        s = s + padded[:, j]
    return s


def device_order_emulation(x, temperature=1.0, blank_bias=0.0, blank_id=-1, vec4=False) -> np.ndarray:
    """The kernels' arithmetic in float32 and in their summation order, for finite [..., V] logits: lane sums (per float4 group
    (x + y) + (z + w) in the vec4 form), then the six-step xor tree.  numpy's float32 exp and log stand in for expf and logf."""
    v = scaled(x, temperature)
    shape, V = v.shape, v.shape[-1]
    v = v.reshape(-1, V)
    mx = v.max(axis=1, keepdims=True)
    d = (v - mx).astype(np.float32)
    e = np.exp(d).astype(np.float32)
    if vec4:
        assert V % 4 == 0
        g = e.reshape(-1, V // 4, 4)
        e = ((g[:, :, 0] + g[:, :, 1]) + (g[:, :, 2] + g[:, :, 3])).astype(np.float32)
    s = _lane_sums(e)
    lane = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lane ^ off]).astype(np.float32)
    lse = np.log(s[:, :1]).astype(np.float32)
    out = (d - lse).astype(np.float32)
    if bias_applies(blank_bias, blank_id, V):
        out[:, blank_id] = out[:, blank_id] - np.float32(blank_bias)
    return out.reshape(shape)


def compare(got, x, temperature, blank_bias, blank_id):
    """`got` ([..., V] float32) against reference(x, ...).  Returns (problems, worst): a list of strings, empty when `got` passes, and the
    largest |error| / tolerance over the finite elements.

    1. The NaN mask and the -inf positions equal the reference's; nothing is +inf.
    2. Finite elements are within `tolerance` of the reference.
    3. Without the reference: over the rows `got` itself shows as defined, the float64 logsumexp of `got` with the bias undone is 0 within
       sum_i p_i tolerance(got_i), p = softmax(got) — to first order an error e_i on element i moves the logsumexp by p_i e_i, and the exact
       answer's logsumexp is exactly 0."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    V = got.shape[-1]
    ref = reference(x, temperature, blank_bias, blank_id)
    assert ref.shape == got.shape, (ref.shape, got.shape)
    problems = []
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        problems.append(f"NaN mask differs at {np.argwhere(np.isnan(got) != np.isnan(ref))[:4].tolist()}")
    if not np.array_equal(np.isneginf(got), np.isneginf(ref)):
        problems.append(f"-inf positions differ at {np.argwhere(np.isneginf(got) != np.isneginf(ref))[:4].tolist()}")
    if np.isposinf(got).any():
        problems.append(f"+inf at {np.argwhere(np.isposinf(got))[:4].tolist()}")
    tol = tolerance(ref, V)
    both = np.isfinite(ref) & np.isfinite(got)
    ratio = np.zeros(ref.shape)
    ratio[both] = np.abs(got.astype(np.float64)[both] - ref[both]) / tol[both]
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        problems.append(f"|error| / tolerance = {worst:.3f} at {tuple(int(k) for k in i)}: got {got[i]!r}, reference {ref[i]!r}")
    g = got.astype(np.float64)
    if bias_applies(blank_bias, blank_id, V):
        g[..., blank_id] += np.float64(np.float32(blank_bias))
    rows = ~np.isnan(g).any(-1) & ~np.isposinf(g).any(-1)
    if rows.any():
        g = g[rows]
        m = g.max(-1, keepdims=True)
        with np.errstate(all="ignore"):
            p = np.exp(g - m)
            z = p.sum(-1)
            lse = m[..., 0] + np.log(z)
            bound = (p / z[..., None] * tolerance(g, V)).sum(-1)
        bad = ~(np.abs(lse) <= bound)
        if bad.any():
            k = int(np.argmax(np.where(bad, np.abs(lse) / bound, 0)))
            problems.append(f"logsumexp of the output is {lse[k]!r}, bound {bound[k]!r} (defined row {k})")
    return problems, worst


# ---- the inputs

NONFINITE_KINDS = ("ninf_head", "ninf_middle", "ninf_last", "ninf_but_one", "ninf_all", "nan_first", "nan_last", "pinf")


def plant_nonfinite(x: np.ndarray) -> dict:
    """One kind per row of matrix 0 (rows 0 .. 7 of the 21; the others stay finite).  Returns kind -> (row, column or None)."""
    V = x.shape[-1]
    rows = x.reshape(-1, V)
    assert np.shares_memory(rows, x)
    single = {"ninf_head": (0, -np.inf), "ninf_middle": (V // 2, -np.inf), "ninf_last": (V - 1, -np.inf), "nan_first": (0, np.nan),
              "nan_last": (V - 1, np.nan), "pinf": (V // 3, np.inf)}
    where = {}
    for r, kind in enumerate(NONFINITE_KINDS):
        if kind in single:
            col, value = single[kind]
            rows[r, col] = value
        elif kind == "ninf_but_one":
            col = (2 * V) // 3
            keep = rows[r, col]
            rows[r] = -np.inf
            rows[r, col] = keep
        else:
            col = None
            rows[r] = -np.inf
        where[kind] = (r, col)
    return where


def make_logits(case: "Case", scale: float, extremes: bool = False) -> np.ndarray:
    """[B, T, V] logits of the case's dtype: N(0, 1) * scale, the same numbers for every layout of one (dtype, V)."""
    rng = np.random.default_rng([case.V, int(case.f16), int(scale)])
    x = (rng.standard_normal((B, T, case.V)) * scale).astype(case.np_dtype)
    if extremes:                                   # the ends of the fp16 range, doubled by temperature 0.5
        x[:, :, 0] = F16_MAX
        x[:, 1::2, 0] = -F16_MAX
        if case.V > 2:
            x[:, 1::2, case.V // 2] = F16_MAX
            x[:, :, case.V - 1] = -F16_MAX
    if case.nonfinite:
        plant_nonfinite(x)
    return x


# ---- the case table

@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    category: str                  # boundary | dtype | blank | strided | alignment | nonfinite | guard
    f16: bool
    V: int
    runs: tuple = ((3.0, 1.7, 2.5, False),)       # (scale, temperature, blank bias, fp16 extremes planted)
    blank: int | None = None       # None: V - 1
    row_pad: int = 0               # row_stride - V
    # None: the matrices follow each other (matrix_stride = T * row_stride).  Else the input is a view [:, :T, :V] of matrices of T + 2 rows
    # of row_stride elements, which lie (T + 2) * row_stride rounded up to a multiple of 4, plus matrix_pad, apart.
    matrix_pad: int | None = None
    in_off: int = 0                # storage offset of the input view, in elements, from a 16-byte aligned address
    out_off: int = 0               # the same for the output
    nonfinite: bool = False

    @property
    def np_dtype(self):
        return np.float16 if self.f16 else np.float32

    @property
    def blank_id(self) -> int:
        return self.V - 1 if self.blank is None else self.blank

    @property
    def row_stride(self) -> int:
        return self.V + self.row_pad

    @property
    def rows_allocated(self) -> int:
        return T if self.matrix_pad is None else T + 2

    @property
    def matrix_stride(self) -> int:
        if self.matrix_pad is None:
            return T * self.row_stride
        return -(-(self.rows_allocated * self.row_stride) // 4) * 4 + self.matrix_pad

    def route(self, lsm_vec4) -> str:
        """vec4 | scalar, by the restated route condition, for 16-byte aligned allocations."""
        base = 0x7F0000000000
        esz = 2 if self.f16 else 4
        return "vec4" if lsm_vec4(self.f16, self.V, self.row_stride, self.matrix_stride, base + esz * self.in_off, base + 4 * self.out_off) else "scalar"

    def form(self, lsm_vec4) -> str:
        """The five forms of the computation: vec4, regs_f32, regs_f16, stream_f32, stream_f16."""
        if self.route(lsm_vec4) == "vec4":
            return "vec4"
        return ("regs" if self.V <= REG_LIMIT else "stream") + ("_f16" if self.f16 else "_f32")


ALL_RUNS = tuple((s, t, b, False) for s in SCALES for t, b in SETTINGS)
F16_RUNS = ALL_RUNS + ((1.0, 0.5, 1.0, True),)


def _cases():
    out = []
    # boundaries in V.  fp32, aligned: the vec4 lane boundary nvec = 63 / 64 / 65, the register limit, the step to streaming
    for V in (4, 252, 256, 260, 1024, 2044, 2048, 2052):
        out.append(Case(f"f32_aligned_V{V}", "boundary", False, V, ALL_RUNS))
    # fp32 rows the scalar kernel serves at any alignment (V = 64 only off a 16-byte boundary): its lane edges, the register limit, streaming
    for V, off in ((1, 0), (2, 1), (63, 0), (64, 1), (65, 2), (1025, 0), (2047, 3), (2049, 0), (5000, 1), (25055, 0)):
        out.append(Case(f"f32_scalar_V{V}_off{off}", "boundary", False, V, ALL_RUNS, in_off=off))
    for V in (1, 9, 257, 1025, 2048, 2049, 4100):
        out.append(Case(f"f16_V{V}", "dtype", True, V, F16_RUNS))
    out.append(Case("f32_vec4_V1024", "dtype", False, 1024))
    out.append(Case("f32_scalar_V1025", "dtype", False, 1025))
    # the blank: every float4 component, more than one register group; the same ids through the scalar kernels
    for blank in (0, 1, 2, 3, 257, 1022, 1023):
        out.append(Case(f"blank{blank}_vec4", "blank", False, 1024, blank=blank))
    for blank in (0, 1, 2, 3, 257, 1022, 1023):
        out.append(Case(f"blank{blank}_scalar", "blank", False, 1024, blank=blank, in_off=1))
    for blank in (0, 3, 257, 1023):
        out.append(Case(f"blank{blank}_f16", "blank", True, 1024, blank=blank))
    # strided input: padded rows and matrices, poison in every element the view does not own
    for f16 in (False, True):
        for row_pad in (4, 8, 1, 3):
            for matrix_pad in (0, 1):
                out.append(Case(f"strided_{'f16' if f16 else 'f32'}_rowpad{row_pad}_matpad{matrix_pad}", "strided", f16, 260,
                                row_pad=row_pad, matrix_pad=matrix_pad))
    # alignment of either side: element offsets 1, 2, 3 (fp16: 1 and 3 are odd, 2-byte aligned addresses), and 4 — another 16-byte boundary
    for f16 in (False, True):
        for in_off, out_off in ((0, 0), (4, 0), (0, 4), (4, 4), (8, 0)) + tuple((k, 0) for k in (1, 2, 3)) + tuple((0, k) for k in (1, 2, 3)) \
                + tuple((k, k) for k in (1, 2, 3)):
            out.append(Case(f"align_{'f16' if f16 else 'f32'}_in{in_off}_out{out_off}", "alignment", f16, 1024, in_off=in_off, out_off=out_off))
    # non-finite rows on every form
    for f16, V, off in ((False, 4, 0), (False, 1024, 0), (False, 1024, 1), (False, 1025, 0), (False, 5, 0), (False, 2052, 0), (False, 2049, 0),
                        (True, 1024, 0), (True, 1025, 1), (True, 5, 0), (True, 2049, 0)):
        out.append(Case(f"nonfinite_{'f16' if f16 else 'f32'}_V{V}_off{off}", "nonfinite", f16, V, in_off=off, nonfinite=True))
    # writes stay inside `out`: once on each route
    out.append(Case("guard_vec4", "guard", False, 1024))
    out.append(Case("guard_scalar", "guard", False, 1025))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def of_category(category: str):
    return [c for c in CASES if c.category == category]
