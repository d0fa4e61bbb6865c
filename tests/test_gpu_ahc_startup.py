"""The start-up of the linkage (csrc/ahc_startup.hip) against an exact reference, through fa_debug_ahc_startup — the hook runs the start-up kernels of a
problem exactly as a linkage call does and stops before the first round.  FA_AHC_MODE_AUTO treats every matrix entry as a filter that is trusted beyond
2 eps, so three things have to hold that no dendrogram test looks at: every entry of M is within the Gram share of eps, 8 (d + 2) u nmax, of the exact
squared distance (the bound is ahc_set_eps's own term, not a measured one); the row records (d1, nn, nnnode) and e2 are the minimum, the lowest-index
argmin and the second smallest entry of the row of M the device wrote; dmax, nmax and eps are what the comment in ahc_set_eps says.

Reference (tests/ahc_startup_restatement.py): squared distances and norms in numpy.longdouble, broadcast over k, for every shape — N = 1024, d = 256
included (1.5 s per family, computed once and shared by the cases of a shape); EXACT is held bit for bit against the sequential
float64 sum in ascending k.  Inputs per shape: (unit) the speaker mixture of the linkage tests, unit rows; (offset) the same + 8 in every coordinate,
not normalised again — norms of ~64 d dwarf the distances, the Gram form loses digits, the clamp at 0 and the bound are exercised.  Rows 127 | 128 (two
tiles) are exact duplicates, row 300 (a third tile) a third copy where N allows: a tie that the merge across tiles (min_merge), the halves inside a
tile and the mirrored partials each have to resolve by index.

The Gram form does not give 0.0 for a duplicated pair: the entry is 2 |x|^2 - 2 x.x with the norm summed in quarters and the product on the matrix
cores, a few ulp of |x|^2 apart, clamped at 0 from below.  What the three entries of the triple are is therefore asserted as: equal bit patterns, >= 0,
never -0.0, within the bound — and each row's d1 AND e2 carry exactly that value (0.0 in EXACT, and wherever the entry is 0.0).

Measured on an MI355X, max |M - D| / ((d + 2) u nmax) — the bound is 8, the derivation in ahc_set_eps promises 4:
(every ratio is below 4; the largest, 1.50, at d = 3 where d + 2 is smallest)
    shape (N x d), route                                   unit    offset
    512 x 16    ahc_gram_mfma2_t<true>, one chunk          0.478   0.545
    300 x 32    ahc_gram_mfma2_t<true>, dead slots         0.322   0.459
    513 x 48    ahc_gram_mfma2_t<true>, float root         0.264   0.393
    1024 x 256  ahc_gram_mfma2_t<true>, production d       0.093   0.136
    2 x 16      ahc_gram_mfma2_t<true>, two points         0.033   0.090
    400 x 20    ahc_gram_mfma, k tail                      0.466   0.501
    700 x 3     ahc_gram_mfma, d below one k-step          1.501   1.151
    513 x 48    startup_gram, ahc_gram_mfma2_t<false>      0.264   0.393
    400 x 20    startup_gram, ahc_gram_mfma                0.466   0.501
The duplicated pair's entry came out 0.0 in all but two cases (300 x 32 unit: 2.2e-16, 512 x 16 offset: 2.3e-13).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from ahc_startup_restatement import DEAD, U, exact_sqdist, row_minima, sequential_sqdist
from conftest import speaker_mixture

AUTO, EXACT = 0, 1
INVALID_ARGUMENT, OUTPUT_TOO_SMALL, RUNTIME_ERROR = 1, 3, 5
# id: N, d, mode, route — and what the shape reaches (Np is N rounded up to the round's block of 256 slots: two tiles of 128)
CASES = {
    "mfma2_one_chunk": (512, 16, AUTO, 0),         # ahc_gram_mfma2_t<true>, one k-chunk: no second LDS stage
    "mfma2_dead_slots": (300, 32, AUTO, 0),        # dead slots 300 .. 511: a tile row that is partly dead, tiles that are all dead
    "mfma2_float_root": (513, 48, AUTO, 0),        # Np 768: 21 workgroups through the float root; one live row in tile row 4, tile row 5 all dead; odd chunk count
    "mfma2_production_d": (1024, 256, AUTO, 0),    # the production dimension, full tiles: 8 x 8 of them, 36 workgroups
    "mfma2_two_points": (2, 16, AUTO, 0),          # the smallest problem: each row's only finite entry
    "mfma_k_tail": (400, 20, AUTO, 0),             # ahc_gram_mfma + ahc_row_minima: d % 16 != 0, the zero-filled k tail, k < d on a chunk partly there
    "mfma_d_below_k_step": (700, 3, AUTO, 0),      # d below one MFMA k-step; ahc_sqnorms with empty quarters
    "ro_mfma2_global_norms": (513, 48, AUTO, 1),   # startup_gram, ahc_gram_mfma2_t<false>: norms read from global memory instead of LDS
    "ro_mfma_k_tail": (400, 20, AUTO, 1),          # startup_gram, ahc_gram_mfma
    "exact_d32": (300, 32, EXACT, 0),              # ahc_pairwise + ahc_row_minima
    "exact_d20": (300, 20, EXACT, 0),
}
FAMILIES = ("unit", "offset")
TRIPLE = (127, 128, 300)


def points(n, d, family):
    x = speaker_mixture(n, d, 12, 0.05, seed=7 * n + d)
    if family == "offset":
        x = x + 8.0
    for r in TRIPLE[1:]:
        if r < n:
            x[r] = x[TRIPLE[0]]
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def reference(n, d, family):
    """(points, exact squared distances, exact squared norms) of a shape and family: computed once, read by every case of that shape."""
    x = points(n, d, family)
    D, norms = exact_sqdist(x)
    for a in (x, D, norms):
        a.setflags(write=False)
    return x, D, norms


def bits(a):
    """The bit patterns of an array of doubles; of one double: a Python int."""
    b = np.asarray(a, np.float64)
    return int(b.reshape(1).view(np.uint64)[0]) if b.ndim == 0 else np.ascontiguousarray(b).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_startup_matches_the_exact_reference(fa, gpu_ctx, case, family):
    n, d, mode, route = CASES[case]
    x, D, norms_exact = reference(n, d, family)
    out = fa.ahc.debug_startup(x, mode=mode, route=route, ctx=gpu_ctx)
    Np, M, node = out["slots"], out["M"], out["node"]
    assert Np == -(-n // 256) * 256 and M.shape == (Np, Np) and out["nan_flag"] == 0
    live = np.arange(Np) < n
    pair = live[:, None] & live[None, :] & ~np.eye(Np, dtype=bool)
    nmax_exact = float(norms_exact.max())
    bound = 8.0 * (d + 2.0) * U * nmax_exact                   # the Gram term of eps (ahc_set_eps)
    Ml = M[:n, :n]
    off = pair[:n, :n]

    # ---- masking, node ids, symmetry
    assert np.array_equal(np.isposinf(M), ~pair), "M is +inf exactly on the diagonal and at dead slots"
    assert np.array_equal(node[:n], np.arange(n)) and (node[n:] == DEAD).all()
    assert np.array_equal(bits(M), bits(M.T)), "the mirrored copy equals the direct one bit for bit"
    assert (Ml[off] >= 0).all() and not np.signbit(Ml[off]).any(), "entries are >= 0 and never -0.0"

    # ---- values
    if mode == EXACT:
        want = sequential_sqdist(x)
        assert np.array_equal(bits(Ml[off]), bits(want[off])), "EXACT: the sequential float64 sum in ascending k, bit for bit"
    else:
        err = np.abs(Ml.astype(np.longdouble) - D)[off]
        ratio = float(err.max() / ((d + 2.0) * U * nmax_exact))
        print(f"\nahc start-up {case} [{family}]: max|M - D| / ((d + 2) u nmax) = {ratio:.3f} (bound 8, derivation 4); duplicate entry {Ml[127, 128] if n > 128 else None}")
        assert float(err.max()) <= bound, f"max |M - D| = {float(err.max()):.3e} > 8 (d + 2) u nmax = {bound:.3e} (ratio {ratio:.3f})"

    # ---- norms (AUTO and route 1)
    if mode == AUTO:
        norms = out["norms"]
        nerr = np.abs(norms[:n].astype(np.longdouble) - norms_exact)
        assert (nerr <= (d + 2.0) * U * norms_exact).all(), f"norms: worst {float((nerr / norms_exact).max() / U):.2f} u, allowed (d + 2) u"
        assert (norms[n:] < 0).all(), "dead slots carry a negative norm"
    else:
        assert out["norms"] is None

    # ---- maxima and eps
    finite = M[np.isfinite(M)]
    assert bits(out["dmax"]) == bits(finite.max() if finite.size else 0.0), "dmax is the largest finite entry of the device's own M"
    if mode == AUTO:
        assert bits(out["nmax"]) == bits(out["norms"][:n].max()), "nmax is the largest of the device's own norms"
    if route == 0 and mode == AUTO:
        u = 1.1102230246251565e-16
        want = 16.0 * float(n) * u * out["dmax"] + 8.0 * (float(d) + 2.0) * u * out["nmax"]
        assert abs(bits(out["eps"]) - bits(want)) <= 1, (out["eps"], want)      # one ulp: the kernel's contraction is its own business
    elif route == 0:
        assert out["eps"] == 0.0 and not np.signbit(out["eps"])

    # ---- the duplicated rows: an entry across a tile edge, and a tie that tile boundaries separate
    members = [r for r in TRIPLE if r < n]
    if len(members) > 1:
        v = M[members[0], members[1]]
        for a in members:
            for b in members:
                if a != b:
                    assert bits(M[a, b]) == bits(v), "all entries of the duplicated rows are one value"
        assert v >= 0 and not np.signbit(v) and (v == 0.0 if mode == EXACT else v <= bound)

    # ---- row minima, against the device's own M (route 0 only: the reference-order start takes its own)
    if route == 1:
        assert out["d1"] is None and out["e2"] is None
        return
    d1, nn, nnnode, e2 = out["d1"], out["nn"], out["nnnode"], out["e2"]
    wd1, wnn, we2 = row_minima(M[:n])
    assert np.array_equal(bits(d1[:n]), bits(wd1)), "d1 is the row minimum"
    assert np.array_equal(nn[:n], wnn), f"nn is the lowest index that attains it (first rows that differ: {np.nonzero(nn[:n] != wnn)[0][:8]})"
    assert np.array_equal(nnnode[:n], node[nn[:n]])
    assert np.array_equal(bits(e2[:n]), bits(we2)), f"e2 is the smallest entry elsewhere in the row (first rows that differ: {np.nonzero(bits(e2[:n]) != bits(we2))[0][:8]})"
    assert np.isposinf(d1[n:]).all() and np.isposinf(e2[n:]).all() and (nn[n:] == -1).all() and (nnnode[n:] == -1).all(), "dead rows"
    if n == 2:
        assert np.isposinf(e2[:2]).all() and nn[:2].tolist() == [1, 0]
    if len(members) > 1 and (np.delete(M[members], members, axis=1) > v).all():     # nothing else as small as the duplicates' entry
        for a in members:
            others = [b for b in members if b != a]
            assert nn[a] == others[0] and bits(d1[a]) == bits(v), f"row {a} names the lowest-index other copy"
            if len(others) > 1:
                assert bits(e2[a]) == bits(v), f"row {a}: the minimum occurs twice, e2 is that value"
                assert mode != EXACT or e2[a] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,mode,route", [(300, 32, AUTO, 0), (400, 20, AUTO, 0), (300, 32, AUTO, 1), (400, 20, AUTO, 1), (300, 20, EXACT, 0)])
def test_a_nan_coordinate_raises_the_flag(fa, gpu_ctx, n, d, mode, route):
    x = points(n, d, "unit")
    x[129, d - 1] = np.nan
    assert fa.ahc.debug_startup(x, mode=mode, route=route, ctx=gpu_ctx)["nan_flag"] != 0


@pytest.mark.gpu
def test_the_hook_refuses_what_it_cannot_copy_out(fa, gpu_ctx):
    import ctypes as C
    f, info = fa.lib().fa_debug_ahc_startup, fa._lib.AhcStartupInfo()
    x = np.zeros((2049, 16))
    assert f(gpu_ctx.handle, x.ctypes.data, 2049, 16, AUTO, 0, C.byref(info), 4096, *[None] * 7) == INVALID_ARGUMENT and info.slots == 2304   # 32 MB cap
    x = points(300, 32, "unit")
    arrays = [np.full(511 * 511, -7.0), np.full(511, -7.0), np.full(511, -7, np.int32), np.full(511, -7.0), np.full(511, -7, np.int32),
              np.full(511, -7, np.int32), np.full(511, -7.0)]                                                  # m, norms, node, d1, nn, nnnode, e2
    assert f(gpu_ctx.handle, x.ctypes.data, 300, 32, AUTO, 0, C.byref(info), 511, *(a.ctypes.data for a in arrays)) == OUTPUT_TOO_SMALL and info.slots == 512
    assert all((a == -7).all() for a in arrays), "a refused call writes nothing"
    for bad in ((None, x.ctypes.data, 300, 32, AUTO, 0, C.byref(info)), (gpu_ctx.handle, None, 300, 32, AUTO, 0, C.byref(info)),
                (gpu_ctx.handle, x.ctypes.data, 300, 32, AUTO, 0, None), (gpu_ctx.handle, x.ctypes.data, 1, 32, AUTO, 0, C.byref(info)),
                (gpu_ctx.handle, x.ctypes.data, 300, 0, AUTO, 0, C.byref(info)), (gpu_ctx.handle, x.ctypes.data, 300, 32, 2, 0, C.byref(info)),
                (gpu_ctx.handle, x.ctypes.data, 300, 32, EXACT, 1, C.byref(info)), (gpu_ctx.handle, x.ctypes.data, 300, 32, AUTO, 2, C.byref(info))):
        assert f(*bad, 512, *[None] * 7) == INVALID_ARGUMENT, bad[2:6]


def test_the_hook_is_inert_without_the_debug_hooks(fa):
    """fa_debug_ahc_startup in a process started without FLUIDAUDIO_HIP_DEBUG_HOOKS=1: RUNTIME_ERROR, like its siblings, before it looks at the context
    (which therefore need not be a real one here: no GPU)."""
    code = r'''
import ctypes as C, sys
sys.path.insert(0, %r)
import numpy as np
import fluidaudio_amd as fa
lib = fa.lib()
assert lib.fa_debug_hooks_enabled() == 0
not_a_context, x, info = C.create_string_buffer(1 << 16), np.zeros((4, 16)), fa._lib.AhcStartupInfo()
print(lib.fa_debug_ahc_startup(C.cast(not_a_context, C.c_void_p), x.ctypes.data, 4, 16, 0, 0, C.byref(info), 0, *[None] * 7),
      lib.fa_debug_ahc_startup(None, x.ctypes.data, 4, 16, 0, 0, C.byref(info), 0, *[None] * 7))
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "FLUIDAUDIO_HIP_DEBUG_HOOKS"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.split() == [str(RUNTIME_ERROR), str(INVALID_ARGUMENT)], (r.stdout, r.stderr[-500:])
