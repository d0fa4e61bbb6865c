"""Which kernel family serves a fa_resample_poly_dev call (csrc/resample_route.h: pick_route, the plain C++ part of resample_host.hip) walked on
the CPU by tests/cpu/resample_routes.cpp over synthetic plan facts, against the conditions restated in tests/resample_restatement.py.  The program
is stand-alone, reads its cases from stdin and is built with the address and undefined-behaviour sanitizers.  No GPU."""
import itertools
import os
import subprocess

import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_restatement as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = 0x7F0000000000          # a 16-byte aligned device pointer
SWITCHES = ("FA_RESAMPLE_SIMPLE", "FA_RESAMPLE_NO_DECIM", "FA_RESAMPLE_NO_DECIM_TILES", "FA_RESAMPLE_NO_ROWS")


def build_routes(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample_routes") / "resample_routes")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "resample_routes.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    return build_routes(tmp_path_factory)


def line_of(P, sw, x_addr, y_addr, frames, n_out):
    G = P["rows"] or dict(tile_rows=64, m_begin=0, k_begin=0, groups=0, ppg=0, sld=0, smax=0, share=0)
    return ("route", P["up"], P["down"], P["n_taps"], P["pre"], P["decim_tiles"], P["decim_regs"], P["interp"], P["rows"] is not None, G["tile_rows"],
            G["m_begin"], G["k_begin"], G["groups"], G["ppg"], G["sld"], G["smax"], G["share"], P["lds_bytes"],
            *(s in sw for s in SWITCHES), x_addr, y_addr, frames, n_out)


def run(routes, lines):
    r = subprocess.run([routes], input="".join(" ".join(str(int(w) if isinstance(w, bool) else w) for w in ln) + "\n" for ln in lines),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return [(R.KINDS[int(o[0])],) + tuple(int(v) for v in o[1:]) for o in out]


def facts(up, down, n_taps, pre, rows=None, **kw):
    P = R.plan_facts(up, down, n_taps, pre, rows)
    P.update(kw)
    return P


# synthetic plans: the filters of fa_resample_poly_taps (21 max(up, down) + 1 taps and a pad), row geometries of the shape fa::rows_geometry gives
ROWS_441 = dict(up=160, down=441, m_begin=12, k_begin=6, groups=1, ppg=160, sld=500, smax=496, share=2, nv=16, tile_rows=16)
ROWS_441_G2 = dict(ROWS_441, groups=2, ppg=80, sld=276, tile_rows=32)
ROWS_147 = dict(up=160, down=147, m_begin=12, k_begin=2, groups=2, ppg=80, sld=100, smax=172, share=4, nv=8, tile_rows=64)
PLANS = {
    "decim_1_3": facts(1, 3, 64, 11),
    "decim_1_6": facts(1, 6, 127, 11),
    "decim_1_12_192kHz_tiles_only": facts(1, 12, 253, 11),
    "decim_1_7_no_instance": facts(1, 7, 148, 11),
    "decim_1_3_other_filter": facts(1, 3, 65, 11),
    "interp_2_1": facts(2, 1, 42, 21),
    "interp_3_2": facts(3, 2, 63, 16),
    "interp_2_1_other_filter": facts(2, 1, 44, 21),
    "rows_160_441_16": facts(160, 441, 9262, 11, ROWS_441),
    "rows_160_441_32_two_groups": facts(160, 441, 9262, 11, ROWS_441_G2),
    "rows_160_147_64": facts(160, 147, 3218, 11, ROWS_147),
    "rows_and_interp_and_decim": facts(1, 3, 64, 11, dict(ROWS_147, up=1, down=3), interp=True),     # every family at once: the order decides
    "lds_at_the_limit": facts(1, 18, 379, 11, lds_bytes=R.LDS_LIMIT),
    "lds_over_the_limit": facts(1, 18, 379, 11, lds_bytes=R.LDS_LIMIT + 4),
    "lds_1_18": facts(1, 18, 379, 11),
    "simple_1_20": facts(1, 20, 421, 11),
    "rows_over_the_lds_limit": facts(160, 441, 9262, 11, ROWS_441, lds_bytes=R.LDS_LIMIT + 4),
}
FRAMES = (0, 1, 23, 24, 100, 115, 116, 500, 3135, 3136, 3137, 6200, 6221, 7116, 7117, 7118, 14172, 14173, 28396, 28397, 40000, 100003)
ADDRS = ((0, 0), (4, 0), (8, 0), (12, 0), (16, 0), (0, 4), (0, 8), (0, 12), (4, 4), (8, 8))


def test_route_equals_the_restated_conditions(routes):
    """Every plan x every switch combination x alignments of either pointer x lengths around each family's first work item."""
    cases = []
    for name, P in PLANS.items():
        g = R.math.gcd(P["up"], P["down"])
        assert g == 1
        for k in range(len(SWITCHES) + 1):
            for sw in itertools.combinations(SWITCHES, k):
                for xo, yo in ADDRS:
                    for frames in FRAMES:
                        cases.append((name, frozenset(sw), BASE + xo, BASE + 4096 + yo, frames, R.n_out_of(frames, P["up"], P["down"])))
    got = run(routes, [line_of(PLANS[c[0]], *c[1:]) for c in cases])
    want = [R.pick_route(PLANS[c[0]], *c[1:]) for c in cases]
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:5]
    assert {g[0] for g in got} == set(R.KINDS)


def one(routes, plan, frames, sw=(), xo=0, yo=0, n_out=None):
    P = PLANS[plan] if isinstance(plan, str) else plan
    n_out = R.n_out_of(frames, P["up"], P["down"]) if n_out is None else n_out
    got = run(routes, [line_of(P, frozenset(sw), BASE + xo, BASE + 4096 + yo, frames, n_out)])[0]
    assert got == R.pick_route(P, frozenset(sw), BASE + xo, BASE + 4096 + yo, frames, n_out)
    return got


def test_order_of_the_families(routes):
    every = "rows_and_interp_and_decim"
    assert one(routes, every, 40000)[0] == "DECIM"
    assert one(routes, every, 40000, ["FA_RESAMPLE_NO_DECIM"])[0] == "INTERP"
    no_interp = dict(PLANS[every], interp=False)
    assert one(routes, no_interp, 40000, ["FA_RESAMPLE_NO_DECIM"])[0] == "ROWS"
    assert one(routes, no_interp, 40000, ["FA_RESAMPLE_NO_DECIM", "FA_RESAMPLE_NO_ROWS"]) == ("LDS", 0, R.n_out_of(40000, 1, 3), 0, 0)
    assert one(routes, dict(no_interp, lds_bytes=R.LDS_LIMIT + 1), 40000, ["FA_RESAMPLE_NO_DECIM", "FA_RESAMPLE_NO_ROWS"]) == ("SIMPLE", 0, 0, 0, 0)
    assert one(routes, every, 40000, SWITCHES) == ("SIMPLE", 0, 0, 0, 0)            # FA_RESAMPLE_SIMPLE goes first


def test_alignment_gate_of_the_decimation_kernels(routes):
    """16-byte loads of the input, 8-byte stores of the output: x & 15 and y & 7 must be 0; no other family looks at an address."""
    for xo in range(0, 32, 4):
        for yo in range(0, 32, 4):
            kind = one(routes, "decim_1_3", 40000, xo=xo, yo=yo)[0]
            assert kind == ("DECIM" if xo % 16 == 0 and yo % 8 == 0 else "LDS"), (xo, yo)
            assert one(routes, "interp_2_1", 4000, xo=xo, yo=yo)[0] == "INTERP"
            assert one(routes, "rows_160_441_16", 40000, xo=xo, yo=yo)[0] == "ROWS"
            assert one(routes, "rows_160_147_64", 40000, xo=xo, yo=yo)[0] == "ROWS"


def test_decimation_split(routes):
    # 1/3: tiles of 1024 outputs from output 10 on, threads of 8; a whole unit needs its last input's 16-byte piece inside the signal
    assert one(routes, "decim_1_3", 3136) == ("DECIM", 10, 1034, 1034, 0)                       # (1024 + 20) 3 + 4: exactly one tile
    for short in (1, 2, 3):                                                                       # the tile's last input 1 .. 3 samples before the end: no tile
        kind, lo, hi, split, _ = one(routes, "decim_1_3", 3132 + short)
        assert (kind, lo, split) == ("DECIM", 10, 10) and hi == 10 + 8 * ((1034 - 10) // 8 - 1)
    assert one(routes, "decim_1_3", (2048 + 20) * 3 + 4 + 8 * 3 + 2) == ("DECIM", 10, 2058 + 8, 2058, 0)   # two tiles, one thread, a ragged rest
    assert one(routes, "decim_1_3", 40000, ["FA_RESAMPLE_NO_DECIM_TILES"])[3] == 10              # no tiles: the register kernel from output 10 on
    assert one(routes, "decim_1_3", 28 * 3 + 4, ["FA_RESAMPLE_NO_DECIM_TILES"]) == ("DECIM", 10, 18, 10, 0)
    assert one(routes, "decim_1_3", 28 * 3 + 3, ["FA_RESAMPLE_NO_DECIM_TILES"])[0] == "LDS"     # one sample short of the first thread: falls through
    assert one(routes, "decim_1_3", 40000, ["FA_RESAMPLE_NO_DECIM"])[0] == "LDS"
    assert one(routes, "decim_1_7_no_instance", 40000)[0] == "LDS" and one(routes, "decim_1_3_other_filter", 40000)[0] == "LDS"


def test_192_khz_has_tiles_but_no_register_kernel(routes):
    P = PLANS["decim_1_12_192kHz_tiles_only"]
    assert P["decim_tiles"] and not P["decim_regs"]
    one_tile = (256 + 20) * 12 + 4
    assert one(routes, P, one_tile) == ("DECIM", 10, 266, 266, 0)
    assert one(routes, P, one_tile + 500) == ("DECIM", 10, 266, 266, 0)                         # what the tiles leave goes to the edges: hi = split
    assert one(routes, P, one_tile - 1)[0] == "LDS"                                               # no tile: nothing for the family, it falls through
    assert one(routes, P, 400003, ["FA_RESAMPLE_NO_DECIM_TILES"])[0] == "LDS"


def test_interpolation_and_rows_without_a_work_item_fall_through(routes):
    assert one(routes, "interp_2_1", 24) == ("INTERP", 19, 27, 20, 1)
    assert one(routes, "interp_2_1", 23) == ("LDS", 0, 46, 0, 0)                                  # groups == 0
    assert one(routes, "interp_2_1_other_filter", 4000)[0] == "LDS"
    first = 6 + 15 * 441 + 496
    assert one(routes, "rows_160_441_16", first) == ("ROWS", 12, 12 + 16 * 160, 0, 1)
    assert one(routes, "rows_160_441_16", first - 1)[0] == "LDS"                                  # tiles == 0
    assert one(routes, "rows_160_441_16", first, ["FA_RESAMPLE_NO_ROWS"])[0] == "LDS"
    assert one(routes, "rows_160_441_16", 5)[0] == "LDS"                                          # m_begin >= n_out
    assert one(routes, "rows_over_the_lds_limit", first - 1)[0] == "SIMPLE"
    kind, lo, hi, _, tiles = one(routes, "rows_160_441_32_two_groups", 6 + 31 * 441 + 496 + 32 * 441 + 17)
    assert (kind, lo, tiles) == ("ROWS", 12, 2) and hi == 12 + 2 * 32 * 160
    kind, lo, hi, _, tiles = one(routes, "rows_160_147_64", 40000)
    assert kind == "ROWS" and tiles == 4 and hi == lo + tiles * 64 * 160 <= R.n_out_of(40000, 160, 147)
    assert one(routes, "rows_160_147_64", 40000, n_out=30000)[1:] == (12, 30000, 0, 3)            # (fewer outputs than the tiles hold: hi is clamped to n_out)


def test_tile_count_guard(routes):
    """(tiles + 8) groups must stay below 2^31: the kernels count workgroups in an int."""
    for groups, P in ((1, PLANS["rows_160_441_16"]), (2, PLANS["rows_160_441_32_two_groups"])):
        G = P["rows"]
        limit = 2 ** 31 // groups - 8                                                             # the first tile count that is refused (groups 1, 2 divide 2^31)
        for tiles, kind in ((limit - 1, "ROWS"), (limit, "LDS")):
            frames = G["k_begin"] + (G["tile_rows"] - 1) * 441 + G["smax"] + (tiles - 1) * G["tile_rows"] * 441
            got = one(routes, P, frames, n_out=R.n_out_of(frames, 160, 441))
            assert got[0] == kind and (kind != "ROWS" or got[4] == tiles), (groups, tiles, got)


def test_lds_limit_and_the_simple_kernel_behind_it(routes):
    assert one(routes, "lds_at_the_limit", 40000)[0] == "LDS" and one(routes, "lds_over_the_limit", 40000)[0] == "SIMPLE"
    assert PLANS["lds_1_18"]["lds_bytes"] == 150508 <= R.LDS_LIMIT < PLANS["simple_1_20"]["lds_bytes"] == 167236
    assert one(routes, "lds_1_18", 80000)[0] == "LDS" and one(routes, "simple_1_20", 80000) == ("SIMPLE", 0, 0, 0, 0)


def test_every_switch(routes):
    for plan, frames, sw, kind in (("decim_1_3", 40000, (), "DECIM"), ("decim_1_3", 40000, ("FA_RESAMPLE_NO_DECIM",), "LDS"),
                                   ("decim_1_3", 40000, ("FA_RESAMPLE_NO_DECIM_TILES",), "DECIM"), ("decim_1_3", 40000, ("FA_RESAMPLE_NO_ROWS",), "DECIM"),
                                   ("rows_160_441_16", 40000, ("FA_RESAMPLE_NO_DECIM", "FA_RESAMPLE_NO_DECIM_TILES"), "ROWS"),
                                   ("rows_160_441_16", 40000, ("FA_RESAMPLE_NO_ROWS",), "LDS"), ("interp_3_2", 4000, ("FA_RESAMPLE_NO_ROWS", "FA_RESAMPLE_NO_DECIM"), "INTERP"),
                                   ("decim_1_3", 40000, ("FA_RESAMPLE_SIMPLE",), "SIMPLE"), ("interp_3_2", 4000, ("FA_RESAMPLE_SIMPLE",), "SIMPLE"),
                                   ("rows_160_441_16", 40000, ("FA_RESAMPLE_SIMPLE",), "SIMPLE"), ("lds_1_18", 40000, ("FA_RESAMPLE_SIMPLE",), "SIMPLE")):
        assert one(routes, plan, frames, sw)[0] == kind, (plan, sw)


def test_route_entry_is_inert_without_the_debug_hooks():
    """fa_debug_resample_route in a process started without FLUIDAUDIO_HIP_DEBUG_HOOKS=1: RUNTIME_ERROR, like fa_debug_set_switch, before it looks at the
    context (which therefore need not be a real one here: no GPU)."""
    code = r'''
import ctypes as C, sys
sys.path.insert(0, %r)
import fluidaudio_amd as fa
lib = fa.lib()
assert lib.fa_debug_hooks_enabled() == 0
not_a_context = C.create_string_buffer(1 << 16)
r = fa._lib.ResampleRoute()
print(lib.fa_debug_resample_route(C.cast(not_a_context, C.c_void_p), None, 100, 1, 3, None, C.byref(r)), lib.fa_debug_set_switch(b"FA_RESAMPLE_SIMPLE", b"1"),
      lib.fa_debug_resample_route(None, None, 100, 1, 3, None, C.byref(r)), lib.fa_debug_resample_route(C.cast(not_a_context, C.c_void_p), None, 100, 1, 3, None, None))
''' % os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k != "FLUIDAUDIO_HIP_DEBUG_HOOKS"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.split() == ["5", "5", "1", "1"], (r.stdout, r.stderr[-500:])
