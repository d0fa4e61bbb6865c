"""The yardstick of the resampler tests, checked without a GPU (tests/resample_restatement.py): the float64 restatement equals
scipy.signal.upfirdn; the float32 ascending-fma evaluation (poly_simple of tests/cpu/resample_geom_emul.cpp = poly_kernel) and the CPU
emulations of the row, interpolation and decimation-tile kernels stay inside the derived bound on every case of the table and return exactly the
taps on the impulse signal; every case's planned route is what csrc/resample_route.h decides on the plan facts the case implies; and the table
covers what it says it covers.

Worst |error| / tolerance of the float32 ascending-fma evaluation over the table, per family (signal_of; each is the value of one case, printed as
`resample-ratio-cpu <family> <ratio> <case>` with -s):

    decim_tiles   0.093   decim_tiles_1_2_one_tile
    decim_regs    0.087   decim_tiles_1_2_last_input_2_before_end
    interp        0.242   interp_4_1_n24_first_thread
    wide16:8      0.293   wide_640_441_16x8_three_tiles_ragged
    wide32:8      0.186   wide_320_441_32x8_one_tile
    wide32:10     0.186   wide_320_441_32x10_one_tile
    rows64        0.261   rows64_441_160_2_tiles
    lds           0.495   tiny_3_2_n1   (one term: a single rounded product against gamma_1 S, at most 0.5 by construction; 0.21 on the longer cases)
    simple        0.088   simple_160_441_switch
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_restatement as R  # noqa: E402
from test_resample_routes import BASE, build_routes, line_of, run as run_routes  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_CASES = R.CASES + R.ALIGN_CASES


def load_emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("resample_emul") / "libresample_geom_emul.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "cpu", "resample_geom_emul.cpp")], check=True)
    L = C.CDLL(so)
    f32p, i64 = np.ctypeslib.ndpointer(np.float32, flags="C"), C.c_int64
    L.poly_simple.argtypes = [f32p, i64, f32p, i64, C.c_int, C.c_int, i64, f32p, i64, i64]
    L.poly_simple.restype = None
    L.rows_emulate.argtypes = [f32p, i64, f32p, i64, C.c_int, C.c_int, i64, i64, f32p, C.POINTER(i64), C.POINTER(i64), np.ctypeslib.ndpointer(np.int32, flags="C"), C.c_int, i64, C.c_int]
    L.interp_emulate.argtypes = [f32p, i64, f32p, C.c_int, C.c_int, C.c_int, i64, i64, f32p, C.POINTER(i64), C.POINTER(i64)]
    L.decim_tiles_emulate.argtypes = [f32p, i64, f32p, C.c_int, i64, f32p, C.POINTER(i64), C.POINTER(i64)]
    L.rows_geom_of.argtypes = [f32p, i64, C.c_int, C.c_int, i64, C.c_int, i64, np.ctypeslib.ndpointer(np.int64, flags="C")]
    return L


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return load_emul(tmp_path_factory)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    return build_routes(tmp_path_factory)


class Inputs:
    """Signals, taps and references of the table's shapes, computed once and shared (read-only) by the tests of a module."""

    def __init__(self, fa):
        self.taps = functools.lru_cache(None)(lambda up, down: self._taps(fa, up, down))
        self.signal = functools.lru_cache(None)(self._signal)
        self.reference = functools.lru_cache(None)(self._reference)
        self.impulse = functools.lru_cache(None)(self._impulse)

    @staticmethod
    def _taps(fa, up, down):
        h, pre = fa.poly_taps(up, down)
        h.setflags(write=False)
        return h, pre

    def _signal(self, up, down, n):
        x = R.signal_of(n, n + 7 * up + down)
        x.setflags(write=False)
        return x

    def _reference(self, up, down, n):
        h, pre = self.taps(up, down)
        out = R.reference(self.signal(up, down, n), h, up, down, pre)
        for a in out:
            a.setflags(write=False)
        return out

    def _impulse(self, up, down, n):
        h, pre = self.taps(up, down)
        x = R.impulses(n, R.impulse_spacing(h.size, up), n + 3 * up + down)
        want, terms = R.impulse_answer(x, h, up, down, pre)
        assert terms.max(initial=0) <= 1 and np.count_nonzero(x) >= 1
        x.setflags(write=False)
        want.setflags(write=False)
        return x, want


@pytest.fixture(scope="module")
def inputs(fa):
    return Inputs(fa)


def geom_of_for(emul, h, pre, up, down):
    def geom_of(budget, share_max):
        out = np.zeros(8, np.int64)
        if emul.rows_geom_of(h, h.size, up, down, pre, share_max, budget, out) != 0:
            return None
        return dict(zip(("m_begin", "k_begin", "groups", "ppg", "sld", "smax", "share", "nv"), (int(v) for v in out)), up=up, down=down)
    return geom_of


def plan_of(emul, inputs, case):
    """The plan facts the case implies: the library's filter for the pair, the row tables rows_build would make under the case's switches."""
    h, pre = inputs.taps(case.up, case.down)
    rows = R.rows_plan(geom_of_for(emul, h, pre, case.up, case.down), case.up, case.down, no_wide="FA_RESAMPLE_NO_WIDE" in case.on, wide=case.wide)
    return R.plan_facts(case.up, case.down, h.size, pre, rows)


def poly_simple(emul, x, h, up, down, pre):
    y = np.zeros(R.n_out_of(x.size, up, down), np.float32)
    emul.poly_simple(x, x.size, h, h.size, up, down, pre, y, 0, y.size)
    return y


def emulate(emul, plan, case, x, h, pre):
    """(y, lo, hi) of the CPU emulation of the case's family on [lo, hi), or None where there is none (register decimation, LDS-staged, simple)."""
    n_out = R.n_out_of(x.size, case.up, case.down)
    y = np.full(n_out, np.nan, np.float32)
    lo, hi = C.c_int64(), C.c_int64()
    if case.kind == "ROWS":
        G = plan["rows"]
        info = np.zeros(6, np.int32)
        rc = emul.rows_emulate(x, x.size, h, h.size, case.up, case.down, pre, n_out, y, C.byref(lo), C.byref(hi), info, G["share_max"], G["budget"], G["tile_rows"])
    elif case.kind == "INTERP":
        rc = emul.interp_emulate(x, x.size, h, h.size, case.up, case.down, pre, n_out, y, C.byref(lo), C.byref(hi))
    elif case.kind == "DECIM" and "FA_RESAMPLE_NO_DECIM_TILES" not in case.on:
        rc = emul.decim_tiles_emulate(x, x.size, h, case.down, n_out, y, C.byref(lo), C.byref(hi))
    else:
        return None
    assert rc == 0, (case.name, rc)
    return y, lo.value, hi.value


def ids(cases):
    return [c.name for c in cases]


SHAPES = sorted({(c.up, c.down, c.n) for c in R.CASES})


def test_restatement_equals_upfirdn(inputs):
    """The gather of the restatement against scipy's polyphase evaluation of the same float32 taps and signal in float64: 1e-12 (3e-16 seen)."""
    from scipy import signal
    worst = 0.0
    for up, down, n in SHAPES:
        h, pre = inputs.taps(up, down)
        ref, S, N = inputs.reference(up, down, n)
        full = signal.upfirdn(h.astype(np.float64), inputs.signal(up, down, n).astype(np.float64), up, down)
        want = np.zeros(ref.size)
        part = full[pre:pre + ref.size]
        want[:part.size] = part
        worst = max(worst, float(np.abs(ref - want).max()))
        assert np.abs(ref - want).max() <= 1e-12, (up, down, n)
        assert (S >= np.abs(ref)).all() and N.max() <= -(-h.size // up) and N.min() >= 1
    print(f"restatement vs upfirdn: {worst:.3g}")


def test_poly_simple_stays_inside_the_bound_and_returns_the_taps(emul, inputs):
    """The float32 ascending-fma evaluation — what every kernel claims the bits of — on every case: inside the derived bound, so the bound is not out of
    reach; exactly the taps on the impulse signal."""
    worst = {}
    for case in R.CASES:
        h, pre = inputs.taps(case.up, case.down)
        got = poly_simple(emul, inputs.signal(case.up, case.down, case.n), h, case.up, case.down, pre)
        problems, ratio = R.compare(got, *inputs.reference(case.up, case.down, case.n))
        assert problems == [], (case.name, problems)
        if ratio > worst.get(case.family, (-1.0, ""))[0]:
            worst[case.family] = (ratio, case.name)
        x, want = inputs.impulse(case.up, case.down, case.n)
        assert np.array_equal(poly_simple(emul, x, h, case.up, case.down, pre), want), case.name
    for family, (ratio, name) in sorted(worst.items()):
        print(f"resample-ratio-cpu {family} {ratio:.3f} {name}")


def test_a_shifted_or_dropped_tap_is_far_outside_the_bound(emul, inputs):
    """What the bound is for: on signal_of a kernel that starts one input late, or drops a term, misses by orders of magnitude (the middle term of every window dropped: the median output; the signal shifted by one sample: the worst)."""
    for up, down, n in ((160, 441, 7117), (1, 3, 3136), (2, 1, 3001), (441, 160, 10269)):
        h, pre = inputs.taps(up, down)
        x = inputs.signal(up, down, n)
        ref, S, N = inputs.reference(up, down, n)
        shifted = poly_simple(emul, np.concatenate([x[1:], x[:1]]), h, up, down, pre)
        _, ratio = R.compare(shifted, ref, S, N)
        assert ratio > 100, (up, down, ratio)
        k, t, mask = R._gather(x, h, up, down, pre)
        mid = mask.sum(axis=1) // 2                                     # the term in the middle of each output's window
        rows = np.arange(ref.size)
        dropped = (ref - h.astype(np.float64)[t[rows, mid]] * x.astype(np.float64)[k[rows, mid]]).astype(np.float32)
        err = np.abs(dropped.astype(np.float64) - ref) / R.tolerance(S, N)
        assert np.median(err) > 100, (up, down, float(np.median(err)))


@pytest.mark.parametrize("case", [c for c in R.CASES if c.kind in ("ROWS", "INTERP", "DECIM")], ids=ids([c for c in R.CASES if c.kind in ("ROWS", "INTERP", "DECIM")]))
def test_emulated_kernels_stay_inside_the_bound_and_return_the_taps(emul, inputs, case):
    h, pre = inputs.taps(case.up, case.down)
    plan = plan_of(emul, inputs, case)
    ref, S, N = inputs.reference(case.up, case.down, case.n)
    em = emulate(emul, plan, case, inputs.signal(case.up, case.down, case.n), h, pre)
    if em is None:
        return
    y, lo, hi = em
    problems, _ = R.compare(y[lo:hi], ref[lo:hi], S[lo:hi], N[lo:hi])
    assert problems == [], problems
    x, want = inputs.impulse(case.up, case.down, case.n)
    y, lo2, hi2 = emulate(emul, plan, case, x, h, pre)
    assert (lo2, hi2) == (lo, hi) and np.array_equal(y[lo:hi], want[lo:hi])


def test_planned_routes_agree_with_the_route_header(emul, routes, inputs):
    """Every case (the alignment rows included) reaches the kind it plans when csrc/resample_route.h is given the plan facts the case implies, the
    row form it plans is the one rows_build picks, and the interior is the range the emulation of the family covers."""
    lines, plans = [], []
    for case in ALL_CASES:
        plan = plan_of(emul, inputs, case)
        plans.append(plan)
        lines.append(line_of(plan, case.on, BASE + 4 * case.in_off, BASE + (1 << 20) + 4 * case.out_off, case.n, R.n_out_of(case.n, case.up, case.down)))
    got = run_routes(routes, lines)
    for case, plan, (kind, lo, hi, split, count) in zip(ALL_CASES, plans, got):
        assert (kind, lo, hi, split, count) == R.pick_route(plan, case.on, BASE + 4 * case.in_off, BASE + (1 << 20) + 4 * case.out_off, case.n, R.n_out_of(case.n, case.up, case.down))
        assert kind == case.kind, (case.name, kind)
        assert case.count is None or count == case.count, (case.name, count)
        assert (plan["rows"]["form"] if kind == "ROWS" else None) == case.form, (case.name, plan["rows"])
        if case.interior and kind != "SIMPLE":
            assert hi > lo, case.name
        h, pre = inputs.taps(case.up, case.down)
        em = emulate(emul, plan, case, inputs.signal(case.up, case.down, case.n), h, pre)
        if em is not None:
            assert (em[1], em[2]) == ((lo, split) if kind == "DECIM" else (lo, hi)), case.name


def test_table_lengths_follow_the_geometry(emul, inputs):
    for (up, down), first in R.ROWS_FIRST.items():
        h, pre = inputs.taps(up, down)
        geom_of = geom_of_for(emul, h, pre, up, down)
        for budget, share_max in ((0, 4), (R.ONE_GROUP, 4), (R.GROUP_BUDGET, 4)):
            G = geom_of(budget, share_max)
            assert G["k_begin"] + G["smax"] == first, (up, down, budget, G)
    for (up, down), first in R.INTERP_FIRST.items():
        h, pre = inputs.taps(up, down)
        assert R.interp_geometry(up, down, h.size, first, R.n_out_of(first, up, down), pre)[2] == 1
        assert R.interp_geometry(up, down, h.size, first - 1, R.n_out_of(first - 1, up, down), pre)[2] == 0


def test_table_hygiene(emul, inputs):
    """Every family and every row form has a case with a non-empty interior and two non-empty edges; every case states its route; every kind,
    every switch and the sizes the issue names are there."""
    assert all(c.kind in R.KINDS and (c.form is not None) == (c.kind == "ROWS") for c in ALL_CASES)
    full = set()
    for case in R.CASES:
        plan = plan_of(emul, inputs, case)
        kind, lo, hi, split, count = R.pick_route(plan, case.on, BASE, BASE, case.n, R.n_out_of(case.n, case.up, case.down))
        n_out = R.n_out_of(case.n, case.up, case.down)
        if kind in ("DECIM", "INTERP", "ROWS") and 0 < lo < hi < n_out:
            full.add(case.family)
            if kind == "DECIM" and lo < split < hi:
                full.add("decim_tiles+regs")
            if kind == "ROWS" and count >= 3:
                full.add(case.family + " three tiles")
        if kind == "LDS" and n_out > 2 * 2048:
            full.add("lds")
        if kind == "SIMPLE":
            full.add("simple")
    assert full >= {"decim_tiles", "decim_regs", "decim_tiles+regs", "interp", "wide16:8", "wide32:8", "wide32:10", "rows64", "lds", "simple",
                    "wide16:8 three tiles", "wide32:8 three tiles", "wide32:10 three tiles", "rows64 three tiles"}, full
    names = {(c.up, c.down) for c in R.CASES}
    assert names >= {(1, d) for d in (2, 3, 4, 5, 6, 12, 7, 18, 20, 1)} | {(2, 1), (2, 3), (4, 3), (4, 1), (3, 1), (3, 2), (5, 4)}
    assert names >= {(160, 441), (320, 441), (640, 441), (80, 441), (80, 189), (160, 147), (16, 15), (8, 7), (147, 160), (441, 160)}
    assert {k for c in R.CASES for k, _ in c.switches} == {"FA_RESAMPLE_SIMPLE", "FA_RESAMPLE_NO_DECIM", "FA_RESAMPLE_NO_DECIM_TILES", "FA_RESAMPLE_NO_ROWS",
                                                           "FA_RESAMPLE_NO_WIDE", "FA_RESAMPLE_WIDE"}
    assert {(c.in_off, c.out_off) for c in R.ALIGN_CASES} == {(i, o) for i in range(4) for o in range(4)} - {(0, 0)}
    assert {c.kind for c in R.ALIGN_CASES} == {"DECIM", "LDS", "INTERP", "ROWS"} and {c.form for c in R.ALIGN_CASES} == {None, "64", "16:8"}
    assert max(c.n for c in ALL_CASES) <= 100000
