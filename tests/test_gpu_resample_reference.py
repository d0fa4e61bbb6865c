"""fa_resample_poly_dev against the float64 restatement of tests/resample_restatement.py on every route of csrc/resample_route.h: decimation
through LDS tiles and from registers, interpolation from registers, the three persistent wide row kernels (16:8, 32:8, 32:10) and the 64-row
kernel, the LDS-staged kernel up to its largest request, and the one-thread-per-output kernel.  A case (resample_restatement.CASES;
tests/test_resample_cpu.py keeps the table honest without a GPU) reaches its route through the rate pair, the length, the pointer offsets and
the FA_RESAMPLE_* switches; before it calls, every test asks fa_debug_resample_route which family will serve the call and asserts the planned
one, so "equals the reference" is said of a known kernel.

The input lies inside a device buffer with 64 floats of +inf / NaN / 1e30 on either side (a read outside [0, frames) that reaches the
arithmetic poisons an output), the output inside a buffer of sentinels with 64 floats on either side that must be unchanged afterwards.

Comparisons: resample_restatement.compare — finite, and |got - ref| <= gamma_N S + N 2^-149 per output, a bound derived from the float32
format alone; on the impulse signal equality with the correctly rounded tap; bit equality with the one-thread-per-output kernel.

Largest |error| / tolerance measured on an MI355X, per family, over the table with signal_of (every comparison prints
`resample-ratio <family> <ratio> <case>`; read them with -s), beside the CPU's float32 ascending-fma evaluation of the same case
(tests/test_resample_cpu.py):

    family         MI355X   CPU     case
    decim_tiles    0.093    0.093   decim_tiles_1_2_one_tile
    decim_regs     0.087    0.087   decim_tiles_1_2_last_input_2_before_end   (no whole tile: the register kernel takes the interior)
    interp         0.242    0.242   interp_4_1_n24_first_thread
    wide16:8       0.293    0.293   wide_640_441_16x8_three_tiles_ragged
    wide32:8       0.186    0.186   wide_320_441_32x8_one_tile
    wide32:10      0.186    0.186   wide_320_441_32x10_one_tile
    rows64         0.261    0.261   rows64_441_160_2_tiles
    lds            0.495    0.495   tiny_3_2_n1   (one term: a single rounded product against gamma_1 S — at most 0.5 by construction)
    simple         0.088    0.088   simple_160_441_switch

The two columns agree to every printed digit, as they must: each kernel claims the bits of poly_kernel, which the CPU column evaluates, and
test_every_route_has_the_bits_of_the_simple_kernel holds them to that claim route by route.
"""
import contextlib
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_restatement as R  # noqa: E402
from test_resample_cpu import Inputs  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
MARGIN = 64            # floats kept either side of the input and of the output: 256 bytes, so the offsets of a case are offsets from a 16-byte boundary
INVALID_ARGUMENT, OUTPUT_TOO_SMALL = 1, 3


@pytest.fixture(scope="module")
def inputs(fa):
    return Inputs(fa)


def device_input(x, in_off=0):
    """x inside one device buffer: MARGIN + in_off floats of +inf, NaN, 1e30 in turn before it, MARGIN behind it."""
    import torch
    host = np.resize(np.array([np.inf, np.nan, 1e30], np.float32), MARGIN + in_off + x.size + MARGIN)
    lo = MARGIN + in_off
    host[lo:lo + x.size] = x
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lo:lo + x.size]


def device_output(n_out, out_off=0):
    import torch
    buf = torch.full((MARGIN + out_off + n_out + MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lo = MARGIN + out_off
    return buf, buf[lo:lo + n_out], lo


def ptr(t):
    return C.c_void_p(t.data_ptr())


def route_of(fa, ctx, d_x, n, up, down, d_y):
    r = fa._lib.ResampleRoute()
    ctx.check(fa.lib().fa_debug_resample_route(ctx.handle, ptr(d_x), n, up, down, ptr(d_y), C.byref(r)), "fa_debug_resample_route")
    return r


@contextlib.contextmanager
def context_for(fa, gpu_ctx, switch, case):
    """The case's switches set, and the context its call runs on: a fresh one where a switch decides how a context BUILDS the tables of a pair."""
    for name, value in case.switches:
        switch(name, value)
    if not case.plan_switches:
        yield gpu_ctx
        return
    ctx = fa.Context(0)
    try:
        yield ctx
    finally:
        ctx.close()


def call(fa, ctx, x, up, down, in_off=0, out_off=0, expect=None):
    """One fa_resample_poly_dev call on x laid out at the given offsets.  expect: the Case whose route the call must take (asked of
    fa_debug_resample_route first).  Checks both margins of the output; returns (output, route)."""
    import torch
    n_out = R.n_out_of(x.size, up, down)
    _, d_x = device_input(x, in_off)
    buf, d_y, lo = device_output(n_out, out_off)
    assert d_x.data_ptr() % 16 == 4 * in_off and d_y.data_ptr() % 16 == 4 * out_off
    torch.cuda.synchronize()
    route = route_of(fa, ctx, d_x, x.size, up, down, d_y)
    if expect is not None:
        kind = R.KINDS[route.kind]
        r_up = up // R.math.gcd(up, down)                     # the plan is the reduced pair's
        assert kind == expect.kind, (expect.name, kind, route.lo, route.hi)
        if kind == "ROWS":
            form = f"{route.tile_rows}:{route.wide_waves}" if route.wide else "64"
            assert form == expect.form and route.tile_rows == int(form.split(":")[0]), (expect.name, form)
            assert route.count >= 1 and route.hi == min(n_out, route.lo + route.count * route.tile_rows * r_up) and route.nv > 0 and route.share in (1, 2, 4) and route.groups >= 1
        else:
            assert (route.wide, route.tile_rows, route.wide_waves, route.nv, route.share, route.groups) == (0,) * 6
        if kind == "INTERP":
            assert route.count >= 1 and route.hi == route.lo + route.count * 4 * r_up
        if kind == "DECIM":
            assert route.lo == 10 <= route.split <= route.hi and (route.split - 10) % 256 == 0 and (route.hi - route.split) % 8 == 0
        if kind == "LDS":
            assert (route.lo, route.hi) == (0, n_out)
        if kind == "SIMPLE":
            assert (route.lo, route.hi, route.split, route.count) == (0, 0, 0, 0)
        if expect.interior and kind != "SIMPLE":
            assert route.hi > route.lo, expect.name
        assert 0 <= route.lo <= route.hi <= n_out
        assert expect.count is None or route.count == expect.count, (expect.name, route.count)
    got = C.c_int64(-1)
    ctx.check(fa.lib().fa_resample_poly_dev(ctx.handle, ptr(d_x), x.size, up, down, ptr(d_y), n_out, C.byref(got)), "fa_resample_poly_dev")
    ctx.synchronize()
    assert got.value == n_out
    whole = buf.cpu().numpy()
    assert (whole[:lo] == SENTINEL).all(), "wrote before the output"
    assert (whole[lo + n_out:] == SENTINEL).all(), "wrote behind the output"
    return whole[lo:lo + n_out].copy(), route


def run(fa, gpu_ctx, switch, case, x):
    with context_for(fa, gpu_ctx, switch, case) as ctx:
        return call(fa, ctx, x, case.up, case.down, case.in_off, case.out_off, expect=case)


def check(case, got, ref, S, N):
    problems, worst = R.compare(got, ref, S, N)
    print(f"resample-ratio {case.family} {worst:.3f} {case.name}")
    assert problems == [], (case.name, problems)
    return worst


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ids(cases):
    return [c.name for c in cases]


NOT_SIMPLE = [c for c in R.CASES if c.kind != "SIMPLE"]


@pytest.mark.parametrize("case", R.CASES, ids=ids(R.CASES))
def test_every_route_against_the_reference(fa, gpu_ctx, switch, inputs, case):
    got, _ = run(fa, gpu_ctx, switch, case, inputs.signal(case.up, case.down, case.n))
    check(case, got, *inputs.reference(case.up, case.down, case.n))


@pytest.mark.parametrize("case", R.CASES, ids=ids(R.CASES))
def test_every_route_returns_the_taps_on_impulses(fa, gpu_ctx, switch, inputs, case):
    """Isolated samples of +-1 and +-0.5: every output has at most one non-zero term and must be that tap times the sample, correctly rounded — in the
    interior and on both edges.  Equality as numbers (the sign of a zero is not compared); no tolerance, no other kernel."""
    x, want = inputs.impulse(case.up, case.down, case.n)
    got, route = run(fa, gpu_ctx, switch, case, x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (case.name, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist(), (route.lo, route.hi))


@pytest.mark.parametrize("case", NOT_SIMPLE, ids=ids(NOT_SIMPLE))
def test_every_route_has_the_bits_of_the_simple_kernel(fa, gpu_ctx, switch, inputs, case):
    """The claim of resample.hip's header — every kernel adds the terms of an output in ascending input order with fused multiply-adds, and gives the
    bits of poly_kernel — once per route, with the route known."""
    x = inputs.signal(case.up, case.down, case.n)
    with context_for(fa, gpu_ctx, switch, case) as ctx:
        got, _ = call(fa, ctx, x, case.up, case.down, case.in_off, case.out_off, expect=case)
        switch("FA_RESAMPLE_SIMPLE", "1")
        ref, route = call(fa, ctx, x, case.up, case.down, case.in_off, case.out_off)
        assert R.KINDS[route.kind] == "SIMPLE"
    diff = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    assert diff.size == 0, (case.name, diff[:8].tolist(), got[diff[:8]].tolist(), ref[diff[:8]].tolist())


@pytest.mark.parametrize("case", R.ALIGN_CASES, ids=ids(R.ALIGN_CASES))
def test_alignment_rows(fa, gpu_ctx, switch, inputs, case):
    """Input 0 .. 3 floats and output 0 .. 3 floats off a 16-byte boundary: within the bound everywhere, the bits of the aligned call, nothing
    written outside.  Integer decimation leaves its kernels for the LDS-staged one when x is off 16 bytes or y off 8; interpolation (unaligned
    16-byte loads and stores), the 64-row kernel and the wide kernel (piecewise stores, unaligned global -> LDS requests) keep theirs."""
    x = inputs.signal(case.up, case.down, case.n)
    base = R.BY_NAME[case.name[:case.name.rindex("_in")]]
    with context_for(fa, gpu_ctx, switch, case) as ctx:
        got, _ = call(fa, ctx, x, case.up, case.down, case.in_off, case.out_off, expect=case)
        aligned, _ = call(fa, ctx, x, case.up, case.down, 0, 0, expect=base)
    check(case, got, *inputs.reference(case.up, case.down, case.n))
    assert same_bits(got, aligned), np.flatnonzero(got.view(np.uint32) != aligned.view(np.uint32))[:8].tolist()


@pytest.mark.parametrize("up,down,red_up,red_down,name", [(320, 882, 160, 441, "wide_160_441_16x8_three_tiles_ragged"), (2, 6, 1, 3, "decim_tiles_1_3_two_tiles_ragged")])
def test_unreduced_factors(fa, gpu_ctx, switch, inputs, up, down, red_up, red_down, name):
    case = R.BY_NAME[name]
    assert (case.up, case.down) == (red_up, red_down)
    x = inputs.signal(case.up, case.down, case.n)
    with context_for(fa, gpu_ctx, switch, case) as ctx:
        got, route = call(fa, ctx, x, up, down, expect=case)
        reduced, route2 = call(fa, ctx, x, red_up, red_down, expect=case)
    assert (route.kind, route.lo, route.hi, route.split, route.count) == (route2.kind, route2.lo, route2.hi, route2.split, route2.count)
    assert same_bits(got, reduced)
    check(case, got, *inputs.reference(case.up, case.down, case.n))


def test_plan_cache_under_alternating_pairs(fa, switch, inputs):
    """A context keeps the plan of its last pair only: A, B, A rebuilds A's plan, and the third call must equal the first bit for bit (and both the
    reference); the same with a pair in between that has no row tables at all."""
    a, b, c = R.BY_NAME["wide_320_441_16x8_three_tiles_ragged"], R.BY_NAME["rows64_160_147_2_tiles"], R.BY_NAME["decim_tiles_1_3_two_tiles_ragged"]
    ctx = fa.Context(0)
    try:
        outs = []
        for case in (a, b, a, c, a, b):
            got, _ = call(fa, ctx, inputs.signal(case.up, case.down, case.n), case.up, case.down, expect=case)
            check(case, got, *inputs.reference(case.up, case.down, case.n))
            outs.append(got)
        assert same_bits(outs[0], outs[2]) and same_bits(outs[0], outs[4]) and same_bits(outs[1], outs[5])
    finally:
        ctx.close()


def test_two_contexts_keep_their_own_row_form(fa, switch, inputs):
    """FA_RESAMPLE_WIDE is read when a context builds the tables of a pair: two contexts built under different values keep their forms after the
    switch is gone, side by side, and produce the same bits."""
    other_form = R.BY_NAME["wide_160_441_32x10_three_tiles_ragged"]
    one_form = dataclasses.replace(R.BY_NAME["wide_160_441_16x8_three_tiles_ragged"], n=other_form.n, count=None)     # the same signal: three 32-row tiles
    x = inputs.signal(one_form.up, one_form.down, one_form.n)
    ctxs = []
    try:
        for case in (one_form, other_form):
            switch("FA_RESAMPLE_WIDE", case.wide)
            ctxs.append(fa.Context(0))
            call(fa, ctxs[-1], x, case.up, case.down, expect=case)
        switch("FA_RESAMPLE_WIDE", None)
        outs = [call(fa, ctx, x, case.up, case.down, expect=case)[0] for _ in range(2) for ctx, case in zip(ctxs, (one_form, other_form))]
        assert all(same_bits(outs[0], o) for o in outs[1:])
        check(one_form, outs[0], *inputs.reference(one_form.up, one_form.down, one_form.n))
    finally:
        for ctx in ctxs:
            ctx.close()


def test_entry_contract(fa, gpu_ctx):
    import torch
    L = fa.lib()
    n, up, down = 300, 3, 2
    n_out = R.n_out_of(n, up, down)
    _, d_x = device_input(R.signal_of(n, 1))
    buf, d_y, lo = device_output(n_out)
    torch.cuda.synchronize()
    got = C.c_int64(-1)

    def untouched():
        gpu_ctx.synchronize()
        return bool((buf == SENTINEL).all().item())
    for frames, u, d in ((-1, up, down), (n, 0, down), (n, up, 0), (n, -3, down), (n, up, -2)):
        got.value = -1
        assert L.fa_resample_poly_dev(gpu_ctx.handle, ptr(d_x), frames, u, d, ptr(d_y), n_out, C.byref(got)) == INVALID_ARGUMENT and got.value == 0
    got.value = -1
    assert L.fa_resample_poly_dev(gpu_ctx.handle, ptr(d_x), n, up, down, ptr(d_y), n_out - 1, C.byref(got)) == OUTPUT_TOO_SMALL and got.value == 0
    assert untouched()
    got.value = -1
    assert L.fa_resample_poly_dev(gpu_ctx.handle, ptr(d_x), 0, up, down, ptr(d_y), n_out, C.byref(got)) == 0 and got.value == 0
    assert L.fa_resample_poly_dev(gpu_ctx.handle, None, 0, up, down, None, 0, C.byref(got)) == 0 and got.value == 0
    assert untouched()
    assert L.fa_resample_poly_dev(gpu_ctx.handle, None, n, up, down, ptr(d_y), n_out, C.byref(got)) == INVALID_ARGUMENT
    assert L.fa_resample_poly_dev(gpu_ctx.handle, ptr(d_x), n, up, down, None, n_out, C.byref(got)) == INVALID_ARGUMENT
    assert L.fa_resample_poly_dev(None, ptr(d_x), n, up, down, ptr(d_y), n_out, C.byref(got)) == INVALID_ARGUMENT
    assert L.fa_resample_poly_dev(gpu_ctx.handle, ptr(d_x), n, up, down, ptr(d_y), n_out, None) == INVALID_ARGUMENT
    assert untouched()
    # the diagnostic entry answers the same way and launches nothing
    r = fa._lib.ResampleRoute()
    assert L.fa_debug_resample_route(None, ptr(d_x), n, up, down, ptr(d_y), C.byref(r)) == INVALID_ARGUMENT
    assert L.fa_debug_resample_route(gpu_ctx.handle, ptr(d_x), n, up, down, ptr(d_y), None) == INVALID_ARGUMENT
    for frames, u, d in ((-1, up, down), (n, 0, down), (n, up, 0)):
        assert L.fa_debug_resample_route(gpu_ctx.handle, ptr(d_x), frames, u, d, ptr(d_y), C.byref(r)) == INVALID_ARGUMENT
    assert L.fa_debug_resample_route(gpu_ctx.handle, ptr(d_x), 0, up, down, ptr(d_y), C.byref(r)) == 0 and R.KINDS[r.kind] == "SIMPLE" and (r.lo, r.hi) == (0, 0)
    assert L.fa_debug_resample_route(gpu_ctx.handle, ptr(d_x), n, up, down, ptr(d_y), C.byref(r)) == 0 and R.KINDS[r.kind] == "INTERP"
    assert untouched()
    assert L.fa_resample_poly_dev(gpu_ctx.handle, ptr(d_x), n, up, down, ptr(d_y), n_out, C.byref(got)) == 0 and got.value == n_out
    gpu_ctx.synchronize()
    assert bool((buf[:lo] == SENTINEL).all().item()) and bool((buf[lo + n_out:] == SENTINEL).all().item()) and not bool((buf[lo:lo + n_out] == SENTINEL).any().item())


@pytest.mark.parametrize("name", ["decim_tiles_1_3_two_tiles_ragged", "interp_2_3_n4099", "wide_640_441_16x8_three_tiles_ragged"])
def test_host_entry_equals_the_device_entry(fa, gpu_ctx, switch, inputs, name):
    """fa.resample_poly (host pointers, buffers from the context's pool) on a decimation, an interpolation and a rows pair.  The pool's addresses cannot be
    seen from Python, so the route cannot be asked for them; instead the result must equal, bit for bit, the device entry's on 16-byte aligned
    buffers, whose route is asserted — and every route has the bits of every other (test_every_route_has_the_bits_of_the_simple_kernel)."""
    case = R.BY_NAME[name]
    assert not case.switches
    x = inputs.signal(case.up, case.down, case.n)
    dev, _ = call(fa, gpu_ctx, x, case.up, case.down, expect=case)
    host = fa.resample_poly(x, case.up, case.down, ctx=gpu_ctx)
    assert same_bits(host, dev)
    check(case, host, *inputs.reference(case.up, case.down, case.n))
