"""fa_ctc_log_softmax_batch_dev against the float64 reference of tests/lsm_restatement.py on every route of csrc/ctc_route.h: the vec4 kernel,
the scalar kernels with the row in registers and streaming, fp32 and fp16.  The cases (lsm_restatement.CASES; tests/test_lsm_cpu.py keeps the
table on both routes) reach a route through shapes, strides and pointer offsets only: boundaries in V, every float4 component of the blank,
blank ids outside the row, padded rows and matrices with poison around them, misaligned pointers on either side, non-finite rows, sentinel
margins around the output; then the entry's argument contract and the checks of the Python seam.

Every comparison is lsm_restatement.compare: finite elements within `tolerance` of the reference, the NaN mask and the -inf positions
identical, and the logsumexp of the output 0 within the same tolerance.

Largest |error| / tolerance measured on an MI355X over the 314 comparisons of this file, per form (every test prints its own as a line
`lsm-ratio <form> <ratio> <case> ...`; read them with -s):

    vec4                        0.639   V = 252,  logits x 50, temperature 0.05, bias 0.5
    scalar, registers, fp32     0.628   V = 64,   logits x 50, temperature 0.05, bias 0.5
    scalar, registers, fp16     0.558   V = 257,  logits x 50, temperature 1.7,  bias 2.5
    scalar, streaming, fp32     0.622   V = 2049, logits x 50, temperature 0.05, bias 0.5
    scalar, streaming, fp16     0.543   V = 2049, logits x 50, temperature 1.7,  bias 2.5

All five are where the float32 emulation of tests/test_lsm_cpu.py puts them (0.64 / 0.64 / 0.56 / 0.62 / 0.54): the largest ratios belong
to references of a few thousand, where the 3 |ref| term is the bound and the roundings of x - max and of the last subtraction use it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsm_restatement as R  # noqa: E402
from test_decoder_routes import lsm_vec4  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
MARGIN = 64            # floats kept either side of the output
B, T = R.B, R.T


def _poison(n, dtype):
    big = 1e30 if dtype == np.float32 else 6e4           # (1e30 is +inf in fp16)
    return np.resize(np.array([np.inf, np.nan, big], dtype), n)


def device_input(case, x, slack=4):
    """x [B, T, V] laid out as the case says, inside one device buffer whose every other element is +inf, NaN or 1e30 in turn: the columns
    V .. row_stride, the rows T .., the gaps between matrices, the elements before the view and `slack` elements behind it."""
    import torch
    V, W, ms = case.V, case.row_stride, case.matrix_stride
    host = _poison(case.in_off + (B - 1) * ms + case.rows_allocated * W + slack, case.np_dtype)
    esz = host.itemsize
    np.lib.stride_tricks.as_strided(host[case.in_off:], (B, T, V), (ms * esz, W * esz, esz))[...] = x
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    d = buf.as_strided((B, T, V), (ms, W, 1), case.in_off)
    assert d.data_ptr() == buf.data_ptr() + case.in_off * esz
    return d


def device_output(case, tail=MARGIN):
    import torch
    n = B * T * case.V
    buf = torch.full((MARGIN + case.out_off + n + tail,), SENTINEL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lo = MARGIN + case.out_off
    return buf, buf[lo:lo + n].view(B, T, case.V), lo


def run(fa, gpu_ctx, case, x, temperature, bias, blank, tail=MARGIN, slack=4):
    """One call as the case lays it out.  Checks that the operands reach the route the case table plans and that nothing outside the
    [B, T, V] output changed; returns the output."""
    d = device_input(case, x, slack)
    buf, out, lo = device_output(case, tail)
    vec4 = lsm_vec4(case.f16, case.V, d.stride(1), d.stride(0), d.data_ptr(), out.data_ptr())
    assert ("vec4" if vec4 else "scalar") == case.route(lsm_vec4)
    got = fa.ctc_log_probs_dev(gpu_ctx, d, temperature, bias, blank, d_out=out)
    gpu_ctx.synchronize()
    assert got is out
    whole = buf.cpu().numpy()
    assert (whole[:lo] == SENTINEL).all(), "wrote before the output"
    assert (whole[lo + B * T * case.V:] == SENTINEL).all(), "wrote behind the output"
    return whole[lo:lo + B * T * case.V].reshape(B, T, case.V).copy()


def check(case, got, x, temperature, bias, blank):
    problems, worst = R.compare(got, x, temperature, bias, blank)
    print(f"lsm-ratio {case.form(lsm_vec4)} {worst:.3f} {case.name} T={temperature} bias={bias} blank={blank}")
    assert problems == [], (case.name, temperature, bias, blank, problems)
    return worst


def ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", R.of_category("boundary") + R.of_category("dtype"), ids=ids(R.of_category("boundary") + R.of_category("dtype")))
def test_boundaries_in_vocab(fa, gpu_ctx, case):
    """The vec4 lane boundary (nvec 63 / 64 / 65), the scalar lane edges, the register limit and the step to streaming, in both dtypes; logits
    scaled by 1, 3 and 50 under each (temperature, bias) pair, fp16 also with +-65504 at temperature 0.5."""
    for scale, temperature, bias, extremes in case.runs:
        x = R.make_logits(case, scale, extremes)
        check(case, run(fa, gpu_ctx, case, x, temperature, bias, case.blank_id), x, temperature, bias, case.blank_id)


@pytest.mark.parametrize("case", R.of_category("blank"), ids=ids(R.of_category("blank")))
def test_blank_component(fa, gpu_ctx, case):
    """The bias lands on the blank column and on no other: each component of a float4, first and later register groups, both routes."""
    (scale, temperature, bias, _), = case.runs
    x = R.make_logits(case, scale)
    got = run(fa, gpu_ctx, case, x, temperature, bias, case.blank_id)
    check(case, got, x, temperature, bias, case.blank_id)
    plain = run(fa, gpu_ctx, case, x, temperature, 0.0, -1)
    moved = np.argwhere((got != plain).any(axis=(0, 1)))[:, 0].tolist()
    assert moved == [case.blank_id]
    np.testing.assert_array_equal(got[:, :, case.blank_id], plain[:, :, case.blank_id] - np.float32(bias))


@pytest.mark.parametrize("name", ["f32_vec4_V1024", "f32_scalar_V1025", "f16_V1025", "f16_V2049", "f32_scalar_V2049_off0"])
def test_blank_outside_the_row_or_without_bias(fa, gpu_ctx, name):
    """blank_id = -1, V, V + 5 and a valid blank with bias 0 move no element away from the unbiased result, bit for bit."""
    case = R.BY_NAME[name]
    x = R.make_logits(case, 3.0)
    plain = run(fa, gpu_ctx, case, x, 1.7, 0.0, -1)
    check(case, plain, x, 1.7, 0.0, -1)
    for blank, bias in ((-1, 2.5), (case.V, 2.5), (case.V + 5, 2.5), (case.V - 2, 0.0), (0, 0.0), (-7, 2.5), (2 ** 31 - 1, 2.5), (-2 ** 31, 2.5)):
        got = run(fa, gpu_ctx, case, x, 1.7, bias, blank)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), (blank, bias)


@pytest.mark.parametrize("case", R.of_category("strided"), ids=ids(R.of_category("strided")))
def test_strided_input(fa, gpu_ctx, case):
    """The input is a view [:, :T, :V] of wider, longer matrices that lie a padded stride apart, with +inf, NaN and 1e30 in every element the
    view does not own: one stray read poisons a row's maximum or its sum.  The output is dense.  Row paddings of 4 and 8 keep a row on a
    16-byte boundary, 1 and 3 do not; the matrix stride is a multiple of 4 or one more."""
    (scale, temperature, bias, _), = case.runs
    x = R.make_logits(case, scale)
    got = run(fa, gpu_ctx, case, x, temperature, bias, case.blank_id)
    check(case, got, x, temperature, bias, case.blank_id)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_alignment_of_either_side(fa, gpu_ctx, f16):
    """Input, output and both at element offsets 1, 2, 3 from a 16-byte boundary (and at 4 and 8: the next boundaries): within tolerance
    everywhere, and bit for bit the same wherever the same kernel ran — neither kernel's arithmetic depends on where the rows lie."""
    cases = [c for c in R.of_category("alignment") if c.f16 == f16]
    x = R.make_logits(cases[0], 3.0)
    (_, temperature, bias, _), = cases[0].runs
    first = {}
    for case in cases:
        got = run(fa, gpu_ctx, case, x, temperature, bias, case.blank_id)
        check(case, got, x, temperature, bias, case.blank_id)
        route = case.route(lsm_vec4)
        if route not in first:
            first[route] = (case.name, got)
        else:
            assert np.array_equal(got.view(np.uint32), first[route][1].view(np.uint32)), (case.name, "differs from", first[route][0])
    assert set(first) == ({"scalar"} if f16 else {"vec4", "scalar"})


@pytest.mark.parametrize("case", R.of_category("guard"), ids=ids(R.of_category("guard")))
def test_writes_stay_inside_the_output(fa, gpu_ctx, case):
    """The output is a [B, T, V] view in the middle of a sentinel-filled buffer: 64 floats before it and, behind it, the rows the three idle
    wavefronts of the last workgroup would own, plus 64.  (The input has as many rows behind it.)  Both margins stay as they were."""
    (scale, temperature, bias, _), = case.runs
    x = R.make_logits(case, scale)
    got = run(fa, gpu_ctx, case, x, temperature, bias, case.blank_id, tail=4 * case.V + MARGIN, slack=4 * case.row_stride)
    check(case, got, x, temperature, bias, case.blank_id)


@pytest.mark.parametrize("case", R.of_category("nonfinite"), ids=ids(R.of_category("nonfinite")))
def test_nonfinite_rows(fa, gpu_ctx, case):
    """-inf in the head, the middle and the last column; a row that is -inf but for one element (0 there); a row of -inf, a NaN in the first
    and in the last column, a +inf (all NaN, as the reference and the oracle have it) — the other rows of the call stay finite."""
    (scale, temperature, bias, _), = case.runs
    x = R.make_logits(case, scale)
    where = R.plant_nonfinite(x.copy())
    got = run(fa, gpu_ctx, case, x, temperature, bias, case.blank_id)
    check(case, got, x, temperature, bias, case.blank_id)
    rows = got.reshape(-1, case.V)
    for kind in ("ninf_head", "ninf_middle", "ninf_last"):
        r, col = where[kind]
        assert np.isneginf(rows[r, col]) and np.isfinite(np.delete(rows[r], col)).all(), kind
    r, col = where["ninf_but_one"]
    assert col != case.blank_id and rows[r, col] == 0.0 and np.isneginf(np.delete(rows[r], col)).all()
    for kind in ("ninf_all", "nan_first", "nan_last", "pinf"):
        assert np.isnan(rows[where[kind][0]]).all(), kind
    assert np.isfinite(rows[len(R.NONFINITE_KINDS):]).all()


def test_entry_contract(fa, gpu_ctx):
    """fa_ctc_log_softmax_batch_dev itself: every malformed call is FA_INVALID_ARGUMENT and launches nothing; an empty batch is a success
    that launches nothing."""
    import ctypes as C

    import torch
    lib, L = fa._lib, fa.lib()
    V, W = 12, 16
    x = torch.zeros((B, T, W), dtype=torch.float32, device="cuda")
    out = torch.full((B, T, V), SENTINEL, dtype=torch.float32, device="cuda")
    good = dict(logits=x.data_ptr(), dtype=lib.DTYPE_F32, batch=B, frames=T, vocab=V, row_stride=W, matrix_stride=T * W, temperature=1.0,
                bias=0.5, blank=V - 1, out=out.data_ptr())

    def call(**change):
        a = dict(good, **change)
        st = L.fa_ctc_log_softmax_batch_dev(gpu_ctx.handle, C.c_void_p(a["logits"]), a["dtype"], a["batch"], a["frames"], a["vocab"], a["row_stride"],
                                            a["matrix_stride"], a["temperature"], a["bias"], a["blank"], C.c_void_p(a["out"]))
        gpu_ctx.synchronize()
        return st

    bad = {"dtype": dict(dtype=7), "dtype_negative": dict(dtype=-1), "vocab_0": dict(vocab=0), "vocab_negative": dict(vocab=-3),
           "row_stride_below_vocab": dict(row_stride=V - 1), "temperature_0": dict(temperature=0.0), "temperature_negative": dict(temperature=-1.0),
           "temperature_nan": dict(temperature=float("nan")), "matrix_stride_short": dict(matrix_stride=(T - 1) * W + V - 1),
           "matrix_stride_0": dict(matrix_stride=0), "null_output": dict(out=None), "null_logits": dict(logits=None),
           "batch_negative": dict(batch=-1), "frames_negative": dict(frames=-1)}
    for name, change in bad.items():
        assert call(**change) == lib.INVALID_ARGUMENT, name
        assert bool((out == SENTINEL).all()), name
    for name, change in {"batch_0": dict(batch=0), "frames_0": dict(frames=0), "batch_0_null_logits": dict(batch=0, logits=None)}.items():
        assert call(**change) == lib.SUCCESS, name
        assert bool((out == SENTINEL).all()), name
    # the smallest matrix stride the contract allows, and the call the malformed ones were derived from
    assert call(matrix_stride=(T - 1) * W + V, batch=1) == lib.SUCCESS
    assert bool((out[0] != SENTINEL).all()) and bool((out[1:] == SENTINEL).all())
    assert call() == lib.SUCCESS
    ref = R.reference(np.zeros((B, T, V), np.float32), 1.0, 0.5, V - 1)
    assert np.abs(out.cpu().numpy() - ref).max() <= R.tolerance(ref, V).min()


def test_python_seam_checks_the_output_tensor(fa, gpu_ctx):
    """ctc_log_probs_dev refuses, before any launch, a d_out that is not float32, not contiguous [B, T, V], or not on the logits' device —
    and logits of a dtype the entry has no code for."""
    import torch
    V = 12
    x = torch.zeros((B, T, V), dtype=torch.float32, device="cuda")
    outs = {"float64": torch.full((B, T, V), SENTINEL, dtype=torch.float64, device="cuda"),
            "float16": torch.full((B, T, V), SENTINEL, dtype=torch.float16, device="cuda"),
            "padded_rows": torch.full((B, T, V + 4), SENTINEL, dtype=torch.float32, device="cuda")[:, :, :V],
            "transposed": torch.full((T, B, V), SENTINEL, dtype=torch.float32, device="cuda").transpose(0, 1),
            "flat": torch.full((B * T * V,), SENTINEL, dtype=torch.float32, device="cuda"),
            "another_shape": torch.full((B, T, V + 1), SENTINEL, dtype=torch.float32, device="cuda"),
            "host": torch.full((B, T, V), SENTINEL, dtype=torch.float32)}
    for name, out in outs.items():
        with pytest.raises(AssertionError):
            fa.ctc_log_probs_dev(gpu_ctx, x, d_out=out)
        gpu_ctx.synchronize()
        assert bool((out == SENTINEL).all()), name
    for dtype in (torch.float64, torch.bfloat16, torch.int32):
        with pytest.raises(AssertionError):
            fa.ctc_log_probs_dev(gpu_ctx, x.to(dtype))
    good = torch.full((B, T, V), SENTINEL, dtype=torch.float32, device="cuda")
    assert fa.ctc_log_probs_dev(gpu_ctx, x, d_out=good) is good
    gpu_ctx.synchronize()
    np.testing.assert_allclose(good.cpu().numpy(), -np.log(V), rtol=0, atol=float(R.tolerance(np.log(V), V)))
