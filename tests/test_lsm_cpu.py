"""The yardstick of the log-softmax tests, checked without a GPU (tests/lsm_restatement.py): the float32 emulation of the device's summation
order stays inside the tolerance on the whole case table, so the bound is reachable; the fp32 CPU oracle agrees with the float64 reference
on which elements are NaN and -inf; and the case table still sends every category down both routes of csrc/ctc_route.h —
tests/test_gpu_ctc_log_softmax.py cannot see which kernel served a call."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsm_restatement as R  # noqa: E402
from test_decoder_routes import lsm_vec4  # noqa: E402


def test_reference_known_answers():
    x = np.log(np.array([[1.0, 2.0, 5.0]], np.float32))
    np.testing.assert_allclose(R.reference(x), np.log(np.array([[0.125, 0.25, 0.625]])), rtol=0, atol=1e-7)   # the float32 rounding of log(2), log(5)
    biased = R.reference(x, 1.0, 0.5, 2)
    np.testing.assert_array_equal(biased[0, :2], R.reference(x)[0, :2])
    assert biased[0, 2] == R.reference(x)[0, 2] - 0.5
    for blank, bias in ((-1, 0.5), (3, 0.5), (8, 0.5), (1, 0.0)):
        np.testing.assert_array_equal(R.reference(x, 1.0, bias, blank), R.reference(x))
    # the quotient is a float32 one: 1 / 3 in float32 is not the float64 third
    third = R.reference(np.array([[1.0, 0.0]], np.float32), 3.0)
    q = np.float64(np.float32(1.0) / np.float32(3.0))
    np.testing.assert_allclose(third[0], [-np.log1p(np.exp(-q)), -q - np.log1p(np.exp(-q))], rtol=0, atol=1e-15)
    inf, nan = np.inf, np.nan
    rows = np.array([[0.0, -inf, 0.0], [-inf, 7.0, -inf], [-inf, -inf, -inf], [nan, 1.0, 2.0], [1.0, inf, 2.0], [1.0, 2.0, nan]], np.float32)
    got = R.reference(rows)
    np.testing.assert_allclose(got[0], [-np.log(2.0), -inf, -np.log(2.0)], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got[1], [-inf, 0.0, -inf])
    assert np.isnan(got[2:]).all()
    assert R.tolerance(np.array([0.0, -10.0, -inf, nan]), 1025).tolist() == [2.0 ** -24 * 69, 2.0 ** -24 * 99, 2.0 ** -24 * 69, 2.0 ** -24 * 69]


def test_compare_notices_what_it_should():
    """The comparison itself: a clean answer passes; a shifted row, a moved -inf, a lost NaN and a biased wrong column do not."""
    c = R.BY_NAME["blank1_vec4"]
    x = R.make_logits(c, 3.0)
    good = R.device_order_emulation(x, 1.7, 2.5, 1, vec4=True)
    assert R.compare(good, x, 1.7, 2.5, 1)[0] == []
    shifted = good.copy()
    shifted[1, 2] += np.float32(1e-4)                      # every element of one row: the logsumexp check sees it as well
    assert len(R.compare(shifted, x, 1.7, 2.5, 1)[0]) == 2
    wrong_column = R.device_order_emulation(x, 1.7, 2.5, 2, vec4=True)
    assert R.compare(wrong_column, x, 1.7, 2.5, 1)[0]
    y = x.copy()
    y[0, 0, 5] = -np.inf
    y[0, 1, 6] = np.nan
    got = R.reference(y).astype(np.float32)
    assert R.compare(got, y, 1.0, 0.0, -1)[0] == []
    moved = got.copy()
    moved[0, 0, 5], moved[0, 0, 4] = moved[0, 0, 4], moved[0, 0, 5]
    assert any("-inf" in p for p in R.compare(moved, y, 1.0, 0.0, -1)[0])
    lost = got.copy()
    lost[0, 1] = R.reference(x)[0, 1]
    assert any("NaN" in p for p in R.compare(lost, y, 1.0, 0.0, -1)[0])


def _finite_problems():
    seen = {}
    for c in R.CASES:
        c = dataclasses.replace(c, nonfinite=False)
        for run in c.runs:
            seen.setdefault((c.f16, c.V, c.blank_id, run), c)
    return seen


def test_emulation_within_tolerance_on_the_case_table():
    worst = {False: 0.0, True: 0.0}
    n = 0
    for (f16, V, blank, (scale, temp, bias, extremes)), c in _finite_problems().items():
        x = R.make_logits(c, scale, extremes)
        forms = [False] + ([True] if not f16 and V % 4 == 0 and V <= R.REG_LIMIT else [])
        for vec4 in forms:
            got = R.device_order_emulation(x, temp, bias, blank, vec4=vec4)
            problems, w = R.compare(got, x, temp, bias, blank)
            assert problems == [], (c.name, scale, temp, bias, vec4, problems)
            worst[vec4] = max(worst[vec4], w)
            n += 1
    assert n > 200
    # not loose by an order of magnitude either: the emulation uses a good part of the bound
    assert 0.1 < worst[False] <= 1.0 and 0.1 < worst[True] <= 1.0, worst


def test_emulation_forms_differ_only_in_rounding():
    c = R.BY_NAME["f32_aligned_V2048"]
    x = R.make_logits(c, 3.0)
    a = R.device_order_emulation(x, 1.7, 2.5, 2047, vec4=False)
    b = R.device_order_emulation(x, 1.7, 2.5, 2047, vec4=True)
    assert not np.array_equal(a, b)
    np.testing.assert_allclose(a, b, rtol=0, atol=4e-6)


def test_oracle_agrees_on_the_nonfinite_pattern(oracle_mod):
    cases = R.of_category("nonfinite")
    assert cases
    for c in cases:
        for scale, temp, bias, extremes in c.runs:
            x = R.make_logits(c, scale, extremes)
            for b in range(R.B):
                ref = R.reference(x[b], temp, bias, c.blank_id)
                got = oracle_mod.ctc_log_probs(x[b].astype(np.float32), temp, bias, c.blank_id)
                np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=c.name)
                np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref), err_msg=c.name)
                assert not np.isposinf(got).any()
            ref0 = R.reference(x, temp, bias, c.blank_id).reshape(-1, c.V)
            where = R.plant_nonfinite(x.copy())
            for kind in ("ninf_head", "ninf_middle", "ninf_last"):
                r, col = where[kind]
                assert np.isneginf(ref0[r, col]) and np.isfinite(np.delete(ref0[r], col)).all()
            r, col = where["ninf_but_one"]
            assert ref0[r, col] == (-np.float64(np.float32(bias)) if col == c.blank_id else 0.0)
            for kind in ("ninf_all", "nan_first", "nan_last", "pinf"):
                assert np.isnan(ref0[where[kind][0]]).all()
            assert np.isfinite(ref0[len(R.NONFINITE_KINDS):]).all()


def test_case_table_reaches_both_routes_in_every_category():
    routes = {}
    forms = set()
    for c in R.CASES:
        routes.setdefault(c.category, set()).add((c.f16, c.route(lsm_vec4)))
        forms.add(c.form(lsm_vec4))
        assert R.B * R.T % 4 != 0 and R.B * R.T <= 100
        assert c.matrix_stride >= (R.T - 1) * c.row_stride + c.V
    assert forms == {"vec4", "regs_f32", "regs_f16", "stream_f32", "stream_f16"}
    for category in ("boundary", "dtype", "blank", "strided", "alignment", "nonfinite", "guard"):
        got = routes[category]
        assert (False, "vec4") in got and (False, "scalar") in got, category
        assert (True, "vec4") not in got
    for category in ("dtype", "blank", "strided", "alignment", "nonfinite"):
        assert (True, "scalar") in routes[category], category

    def where(category, route, f16=False):
        return [c for c in R.of_category(category) if c.route(lsm_vec4) == route and c.f16 == f16]
    # the boundaries the issue names, each on the route it is there for
    assert {c.V for c in where("boundary", "vec4")} == {4, 252, 256, 260, 1024, 2044, 2048}
    assert {c.V for c in where("boundary", "scalar")} == {2052, 1, 2, 63, 64, 65, 1025, 2047, 2049, 5000, 25055}
    assert {c.V for c in where("dtype", "scalar", True)} == {1, 9, 257, 1025, 2048, 2049, 4100}
    assert {c.form(lsm_vec4) for c in R.of_category("boundary")} == {"vec4", "regs_f32", "stream_f32"}
    # every float4 component of the blank, more than one register group, on both routes
    assert {c.blank for c in where("blank", "vec4")} == {c.blank for c in where("blank", "scalar")} == {0, 1, 2, 3, 257, 1022, 1023}
    assert {b & 3 for b in (0, 1, 2, 3)} == {0, 1, 2, 3} and 257 >> 2 >= 64
    # strides: the padded row keeps or breaks the route as planned, and so does the matrix stride
    assert {(c.row_pad, c.matrix_stride % 4 == 0) for c in where("strided", "vec4")} == {(4, True), (8, True)}
    assert {(c.row_pad, c.matrix_stride % 4 == 0) for c in where("strided", "scalar")} == {(4, False), (8, False), (1, True), (1, False), (3, True), (3, False)}
    assert {(c.row_pad, c.matrix_stride % 4 == 0) for c in where("strided", "scalar", True)} == {(p, m) for p in (4, 8, 1, 3) for m in (True, False)}
    # alignment: each side alone and both, at 1, 2, 3 elements; two placements on the vec4 route to compare bit for bit
    assert {(c.in_off, c.out_off) for c in where("alignment", "scalar")} == {(k, 0) for k in (1, 2, 3)} | {(0, k) for k in (1, 2, 3)} | {(k, k) for k in (1, 2, 3)}
    assert len(where("alignment", "vec4")) >= 2
    assert {c.in_off for c in where("alignment", "scalar", True)} >= {0, 1, 2, 3}
    # the non-finite rows on all five forms
    assert {c.form(lsm_vec4) for c in R.of_category("nonfinite")} == forms
    assert all(c.nonfinite == (c.category == "nonfinite") for c in R.CASES)
    assert [c.route(lsm_vec4) for c in R.of_category("guard")] == ["vec4", "scalar"]
