"""The float64 yardstick for fa_resample_poly_dev (csrc/resample.hip: poly_kernel, poly_lds_kernel, poly_decim_tile_kernel, poly_decim_kernel,
poly_interp_kernel, poly_rows_kernel and the wide row kernels), the bound every kernel is held to, the route of a call restated
(csrc/resample_route.h, and the plan facts resample_host.hip feeds it), and the table of cases that tests/test_resample_cpu.py and
tests/test_gpu_resample_reference.py walk.  Plain numpy, no GPU; shares no code with oracle/ or csrc/.

The operation: y[m] = sum over k of h[p - k up] x[k], p = (m + pre) down, over the k with 0 <= p - k up < len(h) and 0 <= k < n — a polyphase FIR
on the zero-stuffed signal with the output alignment of scipy.signal.resample_poly.  h is the library's own float32 filter (fa.poly_taps): its
design is pinned to scipy.signal.firwin by tests/test_oracle_resample.py, so what is left here is the kernels' arithmetic alone.

The bound is derived, not measured: a float32 dot product of N terms, in any order, with or without fused multiply-adds, errs by at most
gamma_N S, gamma_N = N u / (1 - N u), u = 2^-24, S = sum |h| |x| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; an fma
rounds once where a multiply and an add round twice, so it stays inside).  N 2^-149 covers products that underflow.  Zero taps the row kernels pad
their windows with add +-0 and no error.  No margin on top."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

U = 2.0 ** -24


# ---- the reference

def n_out_of(n, up, down):
    g = math.gcd(up, down)
    return -(-n * (up // g) // (down // g))


def _gather(x, h, up, down, pre):
    """Index matrices of the sum: for output m (row) and j (column), k = k_min[m] + j and the tap p - k up, with the mask of the terms that exist."""
    n, nh = len(x), len(h)
    m = np.arange(n_out_of(n, up, down), dtype=np.int64)
    p = (m + pre) * down
    k_lo = np.maximum(0, -((nh - 1 - p) // up))                       # ceil((p - (nh - 1)) / up)
    k_hi = np.minimum(p // up, n - 1)
    k = k_lo[:, None] + np.arange(-(-nh // up), dtype=np.int64)[None, :]
    mask = k <= k_hi[:, None]
    t = p[:, None] - k * up
    assert ((t >= 0) & (t < nh))[mask].all() and (k_hi - k_lo + 1 <= k.shape[1]).all()
    return np.where(mask, k, 0), np.where(mask, t, 0), mask


def reference(x, h, up, down, pre):
    """(ref, S, N): the float64 sum, the sum of |h| |x| and the number of terms, per output, for a float32 signal and float32 taps."""
    assert x.dtype == np.float32 and h.dtype == np.float32
    k, t, mask = _gather(x, h, up, down, pre)
    prod = np.where(mask, h.astype(np.float64)[t] * x.astype(np.float64)[k], 0.0)
    return prod.sum(axis=1), np.abs(prod).sum(axis=1), mask.sum(axis=1)


def tolerance(S, N):
    N = N.astype(np.float64)
    return N * U / (1.0 - N * U) * S + N * 2.0 ** -149


def compare(got, ref, S, N):
    """`got` (float32) against (ref, S, N) of `reference`: (problems, worst |error| / tolerance).  Finite where the reference is; within the
    bound everywhere.  An output with tolerance 0 (every term 0) must equal the reference."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    problems = []
    bad = np.isfinite(ref) & ~np.isfinite(got)
    if bad.any():
        problems.append(f"{int(bad.sum())} non-finite outputs, first at {np.flatnonzero(bad)[:4].tolist()}")
    tol = tolerance(S, N)
    err = np.abs(got.astype(np.float64) - ref)
    ok = np.isfinite(got)
    with np.errstate(all="ignore"):
        ratio = np.where(ok, np.where(err == 0, 0.0, err / tol), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not (err[ok] <= tol[ok]).all():
        i = int(np.argmax(np.where(ok, ratio, 0.0)))
        problems.append(f"|error| / tolerance = {worst:.3f} at output {i} of {got.size}: got {got[i]!r}, reference {ref[i]!r}, tolerance {tol[i]!r}; "
                        f"{int((ok & (err > tol)).sum())} outputs outside")
    return problems, worst


# ---- the signals

def signal_of(n, seed):
    """uniform(-1, 1) * 0.5 plus a sine: every sample matters, no window is quiet."""
    rng = np.random.default_rng(seed)
    return (0.5 * rng.uniform(-1, 1, n) + 0.4 * np.sin(2 * np.pi * 440 * np.arange(n) / 16000.0)).astype(np.float32)


def impulse_spacing(h_len, up):
    return -(-h_len // up) + 2


def impulses(n, spacing, seed):
    """Isolated samples of +-1 and +-0.5 at pseudo-random positions at least `spacing` apart, zeros elsewhere (the first one at 0 .. spacing - 1,
    so that the shortest signals carry one)."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.float32)
    at = int(rng.integers(0, min(spacing, n)))
    while at < n:
        x[at] = rng.choice(np.array([1.0, -1.0, 0.5, -0.5], np.float32))
        at += spacing + int(rng.integers(0, spacing))
    return x


def impulse_answer(x, h, up, down, pre):
    """What every kernel must return on an `impulses` signal: the one non-zero term h[p - k up] x[k], correctly rounded (the product of two float32 is
    exact in float64), or 0.  Also the number of non-zero terms per output, which must not exceed 1."""
    k, t, mask = _gather(x, h, up, down, pre)
    prod = np.where(mask, h.astype(np.float64)[t] * x.astype(np.float64)[k], 0.0)
    return prod.sum(axis=1).astype(np.float32), (prod != 0).sum(axis=1)


# ---- the route, restated (resample_geom.h, resample_route.h, and the plan of resample_host.hip)

KINDS = ("DECIM", "INTERP", "ROWS", "LDS", "SIMPLE")
LDS_LIMIT = 150 * 1024
DECIM_TILE_DOWNS, DECIM_REG_DOWNS = (2, 3, 4, 5, 6, 12), (2, 3, 4, 5, 6)
INTERP_INSTANCES = ((2, 1, 42), (2, 3, 64), (4, 3, 83), (4, 1, 82), (3, 1, 62), (3, 2, 63))
DECIM_TILE_R = {2: 6, 3: 4, 4: 3, 5: 4, 6: 2, 12: 1}
ROWS_NV = (4, 6, 8, 10, 12, 14, 16, 32)
# {rows per tile, wavefronts, reads per window, phases per window, units per wavefront} of the wide kernels, and per form
# (rows, waves, long windows?) -> (floats per LDS row at most, phase groups at most)
WIDE_INSTANCES = ((32, 8, 16, 2, 3), (32, 8, 10, 4, 5), (16, 8, 16, 2, 2), (16, 8, 10, 4, 3), (16, 8, 8, 4, 5), (16, 8, 16, 4, 1), (16, 8, 32, 1, 1),
                  (16, 10, 16, 2, 1), (16, 10, 10, 4, 2), (16, 10, 8, 4, 4), (32, 10, 16, 2, 1), (32, 10, 10, 4, 2), (32, 10, 8, 4, 4), (32, 10, 16, 4, 1),
                  (32, 10, 32, 1, 1))
ONE_GROUP, GROUP_BUDGET = 1 << 30, 64 * 288 * 4


def wide_form_limits(rows, waves, nv):
    long = nv == 32
    table = (((32, 8), None, 512, 512, 1), ((16, 8), None, 512, 576, 1), ((16, 10), None, 512, 576, 1), ((32, 10), True, 576, 576, 8), ((32, 10), False, 288, 288, 8))
    for rw, win, fs, fl, g in table:
        if rw == (rows, waves) and (win is None or win == long):
            return (fl if long else fs), g
    return 0, 0


def decim_split(down, frames, n_out, tiles):
    m_begin = 10
    m_last = (frames - 1) // down - 11 if frames >= 1 else -12
    m_avail = max(m_begin, min(m_last + 1, n_out))

    def whole(m0, step, most):
        n = min((m_avail - m0) // step, most)
        while n > 0 and ((m0 + n * step - 1) + 11) * down + 3 > frames - 1:
            n -= 1
        return m0 + n * step
    to = 256 * DECIM_TILE_R.get(down, 1)
    m_tiles = whole(m_begin, to, (1 << 30) // to) if tiles else m_begin
    return m_begin, m_tiles, whole(m_tiles, 8, 1 << 62)


def interp_geometry(up, down, nt, frames, n_out, pre, r=4):
    no, kb = r * up, (nt - 1) // up
    nin = ((no - 1) * down) // up + kb + 1
    nv = (nin + 3) // 4
    j = -(-kb // down)
    while j * up < pre:
        j += 1
    m_begin, q_begin = j * up - pre, j * down
    first = q_begin - kb
    groups = (frames - first - 4 * nv) // (r * down) + 1 if frames >= first + 4 * nv else 0
    groups = min(groups, (n_out - m_begin) // no) if m_begin < n_out else 0
    return m_begin, q_begin, groups


def rows_tiles(G, frames, n_out, rows):
    last_need = G["k_begin"] + (rows - 1) * G["down"] + G["smax"]
    tiles = (frames - last_need) // (rows * G["down"]) + 1 if frames >= last_need else 0
    per_tile = rows * G["up"]
    return min(tiles, -(-(n_out - G["m_begin"]) // per_tile)) if G["m_begin"] < n_out else 0


def lds_need(up, down, n_taps):
    return 4 * (((n_taps + 3) & ~3) + (2048 * down + up - 1) // up + (n_taps + up - 1) // up + 4)


def rows_plan(geom_of, up, down, no_wide=False, wide=None):
    """The row tables a plan gets (rows_build of resample_host.hip): None, or the geometry dict of `geom_of(budget, share_max)` (None: not served)
    with `form` ("16:8", "32:8", "32:10", "64"), tile_rows and the (budget, share_max) it was built with added.  `wide`: the value of FA_RESAMPLE_WIDE."""
    if not no_wide:
        cands = [(32, 10, ONE_GROUP), (16, 8, ONE_GROUP), (32, 10, GROUP_BUDGET), (32, 8, ONE_GROUP)]
        if wide is not None:
            r, w = (int(v) for v in wide.split(":"))
            cands = [(32, 10, ONE_GROUP), (32, 10, GROUP_BUDGET)] if (r, w) == (32, 10) else [(r, w, ONE_GROUP)]
        for rows, waves, budget in cands:
            G = geom_of(budget, 4)
            if G is None:
                continue
            if (rows, waves) == (32, 10) and budget > GROUP_BUDGET and G["nv"] != 32:
                continue
            pu = 4 * 64 // rows
            units = -(-G["ppg"] // pu)
            if waves == 10 and units % 10 != 0:
                continue
            ch = -(-units // waves)
            row_floats, max_groups = wide_form_limits(rows, waves, G["nv"])
            if G["sld"] <= row_floats and G["groups"] <= max_groups and (rows, waves, G["nv"], G["share"], ch) in WIDE_INSTANCES:
                return dict(G, form=f"{rows}:{waves}", tile_rows=rows, budget=budget, share_max=4)
    G, share_max = geom_of(0, 4), 4
    if G is None:
        return None
    if G["sld"] > 64 * 5 and G["share"] != 1:             # the long-row build of the 64-row kernel is instantiated for share = 1 only
        G, share_max = geom_of(0, 1), 1
        if G is None:
            return None
    return dict(G, form="64", tile_rows=64, budget=0, share_max=share_max) if G["nv"] in ROWS_NV else None


def plan_facts(up, down, n_taps, pre, rows):
    """What plan_get keeps for a reduced pair; `rows`: the result of rows_plan."""
    decim_pair = up == 1 and n_taps == 21 * down + 1 and pre == 11
    return dict(up=up, down=down, n_taps=n_taps, pre=pre, decim_tiles=decim_pair and down in DECIM_TILE_DOWNS, decim_regs=decim_pair and down in DECIM_REG_DOWNS,
                interp=(up, down, n_taps) in INTERP_INSTANCES, rows=rows, lds_bytes=lds_need(up, down, n_taps))


def pick_route(P, sw, x_addr, y_addr, frames, n_out):
    """(kind, lo, hi, split, count): the first family, in this order, that has an instance for the pair, is not switched off and finds whole work
    items inside the signal.  sw: the set of switch names that are on."""
    if "FA_RESAMPLE_SIMPLE" in sw:
        return ("SIMPLE", 0, 0, 0, 0)
    if P["decim_tiles"] and "FA_RESAMPLE_NO_DECIM" not in sw and x_addr % 16 == 0 and y_addr % 8 == 0:
        m_begin, m_tiles, m_regs = decim_split(P["down"], frames, n_out, "FA_RESAMPLE_NO_DECIM_TILES" not in sw)
        if not P["decim_regs"]:
            m_regs = m_tiles
        if m_regs > m_begin:
            return ("DECIM", m_begin, m_regs, m_tiles, 0)
    if P["interp"]:
        m_begin, q_begin, groups = interp_geometry(P["up"], P["down"], P["n_taps"], frames, n_out, P["pre"])
        if groups > 0:
            return ("INTERP", m_begin, m_begin + groups * 4 * P["up"], q_begin, groups)
    G = P["rows"]
    if G is not None and "FA_RESAMPLE_NO_ROWS" not in sw:
        tiles = rows_tiles(G, frames, n_out, G["tile_rows"])
        if tiles > 0 and (tiles + 8) * G["groups"] < 2 ** 31:
            return ("ROWS", G["m_begin"], min(n_out, G["m_begin"] + tiles * G["tile_rows"] * G["up"]), 0, tiles)
    if P["lds_bytes"] <= LDS_LIMIT:
        return ("LDS", 0, n_out, 0, 0)
    return ("SIMPLE", 0, 0, 0, 0)


# ---- the case table

@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str                    # decim_tiles | decim_regs | interp | wide16:8 | wide32:8 | wide32:10 | rows64 | lds | simple
    up: int
    down: int
    n: int
    kind: str                      # the route the case is meant to reach ...
    form: str | None = None        # ... and for ROWS the form: "16:8", "32:8", "32:10" (wide) or "64"
    count: int | None = None       # INTERP: threads, ROWS: tiles the route must report, where the case's name promises a number
    interior: bool = True          # the family serves a non-empty [lo, hi) (LDS: everything; SIMPLE: nothing, by definition)
    in_off: int = 0                # offset of the input, in floats, from a 16-byte aligned address
    out_off: int = 0               # the same for the output
    switches: tuple = ()           # ((name, value), ...)

    @property
    def on(self):
        return frozenset(name for name, _ in self.switches)

    @property
    def wide(self):
        return dict(self.switches).get("FA_RESAMPLE_WIDE")

    @property
    def plan_switches(self):
        """The switches a context reads when it BUILDS the tables of a pair: such a case needs a context of its own."""
        return tuple((k, v) for k, v in self.switches if k in ("FA_RESAMPLE_WIDE", "FA_RESAMPLE_NO_WIDE"))


# k_begin + smax of fa::rows_geometry per pair — tile 0 of a kernel with `rows` rows per tile stages x[k_begin, k_begin + (rows - 1) down + smax) —
# the same for every form of a pair; the shortest signal that gives poly_interp_kernel one thread (fa::interp_geometry).  The lengths below are
# built on them, and tests/test_resample_cpu.py::test_table_lengths_follow_the_geometry holds them against resample_geom.h.
ROWS_FIRST = {(160, 441): 502, (320, 441): 479, (640, 441): 470, (80, 441): 572, (80, 189): 249, (160, 147): 174, (16, 15): 42, (8, 7): 33, (147, 160): 191,
              (441, 160): 189}
INTERP_FIRST = {(2, 1): 24, (2, 3): 46, (4, 3): 33, (4, 1): 24, (3, 1): 24, (3, 2): 28}


def _cases():
    out = []

    def add(name, family, up, down, n, kind, **kw):
        out.append(Case(name, family, up, down, n, kind, **kw))
    # Decimation tiles.  A tile is TO = 256 R outputs from output 10 on; its last input is ((10 + TO t - 1) + 11) down, and the 16-byte piece that
    # holds it must end inside the signal: t whole tiles need n >= (TO t + 20) down + 4.  Lengths: one tile exactly; the tile's last input 1, 2 and 3
    # samples before the end (n = (TO + 20) down + 1 .. 3: no tile, the register kernel takes what the tile would have); two tiles plus a
    # ragged rest for the register kernel and the edge.
    for down in (2, 3, 4, 5, 6, 12):
        to = 256 * DECIM_TILE_R[down]
        one = (to + 20) * down + 4
        add(f"decim_tiles_1_{down}_one_tile", "decim_tiles", 1, down, one, "DECIM")
        add(f"decim_tiles_1_{down}_two_tiles_ragged", "decim_tiles", 1, down, (2 * to + 20) * down + 4 + 13 * down + 1, "DECIM")
        if down in (2, 3, 12):
            for short in (1, 2, 3):
                # (192 kHz has no register kernel: without a tile the call falls through to the LDS-staged kernel)
                add(f"decim_tiles_1_{down}_last_input_{short}_before_end", "decim_regs" if down != 12 else "lds", 1, down, one - 4 + short, "DECIM" if down != 12 else "LDS")
    # Decimation from registers alone: a thread is 8 outputs from output 10 on: n >= (8 g + 20) down + 4 for g threads.  About 40 down: two threads and
    # a ragged rest; one unit short of the first thread: all edges, and the call falls through to the LDS-staged kernel.
    for down in (2, 3, 4, 5, 6):
        add(f"decim_regs_1_{down}_two_threads", "decim_regs", 1, down, 40 * down + 7, "DECIM", switches=(("FA_RESAMPLE_NO_DECIM_TILES", "1"),))
        add(f"decim_regs_1_{down}_one_thread", "decim_regs", 1, down, 28 * down + 4, "DECIM", switches=(("FA_RESAMPLE_NO_DECIM_TILES", "1"),))
        add(f"decim_regs_1_{down}_one_short", "lds", 1, down, 28 * down + 3, "LDS", interior=True, switches=(("FA_RESAMPLE_NO_DECIM_TILES", "1"),))
    # Interpolation: a thread is 4 up outputs.  The shortest signal with one thread, one sample short of it (no thread: LDS-staged), around the first
    # few threads, and a few thousand samples (more than one workgroup of 256 threads at 2/1 .. 3/1)
    for up, down, short, long in ((2, 1, 57, 3001), (2, 3, 130, 4099), (4, 3, 64, 3002), (4, 1, 45, 1031), (3, 1, 50, 1537), (3, 2, 40, 2049)):
        first = INTERP_FIRST[(up, down)]
        add(f"interp_{up}_{down}_n{first}_first_thread", "interp", up, down, first, "INTERP", count=1)
        add(f"interp_{up}_{down}_n{first - 1}_one_short", "lds", up, down, first - 1, "LDS")
        add(f"interp_{up}_{down}_n{short}", "interp", up, down, short, "INTERP")
        add(f"interp_{up}_{down}_n{long}", "interp", up, down, long, "INTERP")
    # Wide rows.  A tile is `rows` x up outputs and stages x[k_begin + rows down t, + (rows - 1) down + smax): one tile, three tiles plus a ragged
    # rest, and one sample short of the first tile (ROWS_FIRST above).
    for up, down, wide, form in ((160, 441, "16:8", "16:8"), (160, 441, "32:8", "32:8"), (160, 441, "32:10", "32:10"), (320, 441, "16:8", "16:8"), (320, 441, "32:8", "32:8"),
                                 (320, 441, "32:10", "32:10"), (640, 441, None, "16:8"), (80, 441, None, "32:10"), (80, 189, None, "16:8")):
        sw = (("FA_RESAMPLE_WIDE", wide),) if wide else ()
        rows = int(form.split(":")[0])
        first = ROWS_FIRST[(up, down)] + (rows - 1) * down
        tag = f"wide_{up}_{down}_{form.replace(':', 'x')}"
        add(f"{tag}_one_tile", f"wide{form}", up, down, first, "ROWS", form=form, count=1, switches=sw)
        add(f"{tag}_three_tiles_ragged", f"wide{form}", up, down, first + 2 * rows * down + 5 * down + 3, "ROWS", form=form, count=3, switches=sw)
        add(f"{tag}_one_short", "lds", up, down, first - 1, "LDS", switches=sw)
    # The 64-row kernel: the pairs no wide kernel has an instance for, and 160/441 with FA_RESAMPLE_NO_WIDE.  One, two and three tiles (the last ragged).
    for up, down, sw in ((160, 147, ()), (16, 15, ()), (8, 7, ()), (147, 160, ()), (441, 160, ()), (160, 441, (("FA_RESAMPLE_NO_WIDE", "1"),))):
        first = ROWS_FIRST[(up, down)] + 63 * down
        for tiles in (1, 2, 3):
            add(f"rows64_{up}_{down}_{tiles}_tiles", "rows64", up, down, first + (tiles - 1) * 64 * down + (0 if tiles == 1 else 7 * down + 2), "ROWS", form="64", count=tiles, switches=sw)
    # LDS-staged: two full tiles of 2048 outputs plus a ragged third; the largest LDS request (1/18: 147 KB); the pairs of other families switched over
    add("lds_1_1", "lds", 1, 1, 2 * 2048 + 301, "LDS")
    add("lds_5_4", "lds", 5, 4, (2 * 2048 + 301) * 4 // 5, "LDS")
    add("lds_1_7", "lds", 1, 7, (2 * 2048 + 301) * 7, "LDS")
    add("lds_1_18_largest_request", "lds", 1, 18, (2 * 2048 + 301) * 18, "LDS")
    add("lds_1_3_no_decim", "lds", 1, 3, (2 * 2048 + 301) * 3, "LDS", switches=(("FA_RESAMPLE_NO_DECIM", "1"),))
    add("lds_160_441_no_rows", "lds", 160, 441, (2 * 2048 + 301) * 441 // 160, "LDS", switches=(("FA_RESAMPLE_NO_ROWS", "1"),))
    # SIMPLE: a filter plus span over 150 KB, and the switch
    add("simple_1_20_filter_too_long", "simple", 1, 20, 20 * 900 + 7, "SIMPLE", interior=False)
    add("simple_1_3_switch", "simple", 1, 3, 3300, "SIMPLE", interior=False, switches=(("FA_RESAMPLE_SIMPLE", "1"),))
    add("simple_160_441_switch", "simple", 160, 441, 9000, "SIMPLE", interior=False, switches=(("FA_RESAMPLE_SIMPLE", "1"),))
    # Tiny signals: shorter than the filter, both clamps act on every output; no family finds a work item, the LDS-staged kernel serves them
    for up, down in ((3, 2), (1, 3), (160, 441)):
        for n in (1, 2, 5, 21):
            add(f"tiny_{up}_{down}_n{n}", "lds", up, down, n, "LDS")
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Alignment rows: (input offset, output offset) in floats from a 16-byte boundary, applied to one case per family.  Decimation leaves its route
# when x is off 16 bytes or y off 8 (kind LDS then); the other families keep theirs.
ALIGN_OFFSETS = tuple((i, o) for i in range(4) for o in range(4) if (i, o) != (0, 0))
ALIGN_BASES = ("decim_tiles_1_3_two_tiles_ragged", "interp_2_3_n4099", "rows64_160_147_2_tiles", "wide_160_441_16x8_three_tiles_ragged")


def aligned_variant(case, in_off, out_off):
    kind = case.kind
    if case.kind == "DECIM" and (in_off % 4 != 0 or out_off % 2 != 0):
        kind = "LDS"
    return dataclasses.replace(case, name=f"{case.name}_in{in_off}_out{out_off}", in_off=in_off, out_off=out_off, kind=kind,
                               form=case.form if kind == case.kind else None, family=case.family if kind == case.kind else "lds")


ALIGN_CASES = tuple(aligned_variant(BY_NAME[b], i, o) for b in ALIGN_BASES for i, o in ALIGN_OFFSETS)
