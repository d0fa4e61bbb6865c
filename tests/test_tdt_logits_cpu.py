"""The yardstick of the TDT joint-logits tests, checked without a GPU (tests/tdt_logits_restatement.py): the float32 emulation of both
soft-max forms stays inside the tolerance on every finite row of the case table, so the bound is reachable; the reference agrees with the
numpy expressions tests/test_gpu_tdt.py has used so far; the table still sends every category to each of the five kernel instances of
csrc/tdt.hip — tests/test_gpu_tdt_logits.py cannot see which one served a call —; and every row of every call is a decision the walk
takes and emits (the diagonal condition), so none is left out of the comparison on the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_logits_restatement as R  # noqa: E402
from test_decoder_routes import tdt_route  # noqa: E402

_DIAGONALS = {}


def diagonal(call):
    if call.name not in _DIAGONALS:
        _DIAGONALS[call.name] = R.diagonal(call)
    return _DIAGONALS[call.name]


def test_reference_known_answers():
    inf, nan = np.inf, np.nan
    rows = np.array([[0.0, np.log(3.0), 0.0, 9.0, 1.0, 2.0, 2.0],          # token 1 of 3, probability 3 / 5; bins 1 and 2 tie: the first
                     [2.0, 2.0, 1.0, 9.0, nan, 5.0, -inf],                # tie: the first; a NaN bin never wins
                     [nan, 1.0, 0.0, 9.0, -inf, -inf, -inf],              # NaN never wins, the probability is undefined; no bin above -inf: 0
                     [nan, nan, nan, 9.0, nan, nan, nan],
                     [-inf, -inf, -inf, 9.0, 1.0, 0.0, 0.0],
                     [0.0, inf, inf, 9.0, 0.0, 0.0, 1.0],
                     [-inf, 4.0, -inf, 9.0, 0.0, 1.0, 0.0]], np.float32)
    rows[:, 3] = [9.0, nan, inf, 9.0, 9.0, 9.0, 9.0]                       # the first duration logit: never part of the token decision
    token, dbin, prob = R.reference(np.concatenate([rows, np.full((7, 2), inf, np.float32)], axis=1), 3, 4)
    assert token.tolist() == [1, 0, 1, 0, 0, 1, 1]
    assert dbin.tolist() == [0, 2, 0, 0, 0, 0, 0]
    np.testing.assert_allclose(prob[[0, 1, 6]], [0.6, 1.0 / (2.0 + np.exp(-1.0)), 1.0], rtol=1e-7)    # float32's log(3)
    assert np.isnan(prob[2:6]).all()
    assert R.clamp([nan, inf, -0.5, 0.25, 1.5]).tolist() == [0.0, 0.0, 0.0, 0.25, 1.0]
    half = R.reference(np.array([1.0, 1.0, 0.0], np.float16), 2, 1)
    assert (int(half[0]), int(half[1]), float(half[2])) == (0, 0, 0.5)


def test_tolerance_is_the_derived_count():
    """c by the count in tolerance's docstring, and the hard condition: at V1 = 1 025 no wider than the flat rtol = 3e-5 of test_gpu_tdt.py."""
    u = 2.0 ** -24
    assert R.tolerance(1.0, 1, "registers") == u * (1 + 14)                     # a certain row has no spread
    assert R.tolerance(1.0 / 1025, 1025, "pairs") == u / 1025 * (17 + 14)       # nor has a flat one
    assert R.tolerance(1.0 / 8193, 8193, "streaming") == u / 8193 * (129 + 14 + 3 * 8)
    assert R.tolerance(1.0 / 1089, 1089, "streaming") == u / 1089 * (18 + 14 + 3)
    assert R.tolerance(np.nan, 64, "registers") == 0.0
    p = np.linspace(1.0 / 1025, 1.0, 20001)
    assert (R.spread(p, 1025) <= np.log(1025)).all() and (R.spread(p, 1025) >= 0).all()
    for form in R.FORMS:
        assert (R.tolerance(p, 1025, form) <= 3e-5 * p).all()
        assert (R.tolerance(p, 1025, form) <= u * p * (17 + 14 + 3 + 2.25 * np.log(1025)) * (1 + 1e-12)).all()
    # the spread is what it bounds: sum p_i (max - x_i) of real rows
    rng = np.random.default_rng(0)
    for V1 in (2, 65, 1025):
        x = rng.standard_normal((50, V1)) * rng.choice(R.SCALES, (50, 1))
        d = x.max(-1, keepdims=True) - x
        w = np.exp(-d)
        prob = 1.0 / w.sum(-1)
        assert ((w * d).sum(-1) * prob <= R.spread(prob, V1) + 1e-12).all()


def test_reference_agrees_with_the_expressions_of_test_gpu_tdt():
    """argmax with NaN -> -inf and 1 / exp(x - mx).sum, as the three logits tests of tests/test_gpu_tdt.py build their tables: the same
    tokens and bins everywhere, the same clamped probability wherever theirs is defined — it is inf - inf = NaN for a row of -inf, as the
    reference has it, and 1 / inf = 0 beside a +inf, the value the clamp gives the reference's NaN."""
    n = 0
    for call in R.CALLS:
        if call.category != "boundary" or call.pad:
            continue
        d = diagonal(call)
        V1, nd = call.V1, call.nd
        idx = np.arange(d.T)
        x = d.logits[:, idx, idx].astype(np.float32)
        xt = np.where(np.isnan(x[..., :V1]), -np.inf, x[..., :V1])
        xd = np.where(np.isnan(x[..., V1:V1 + nd]), -np.inf, x[..., V1:V1 + nd])
        mx = np.max(xt, axis=-1, keepdims=True)
        with np.errstate(all="ignore"):
            pr = (1.0 / np.exp(x[..., :V1].astype(np.float64) - mx).sum(-1)).astype(np.float32)
        np.testing.assert_array_equal(np.argmax(xt, -1), d.token, err_msg=call.name)
        np.testing.assert_array_equal(np.argmax(xd, -1), d.dbin, err_msg=call.name)
        np.testing.assert_array_equal(R.clamp(pr).astype(np.float32), R.clamp(d.prob).astype(np.float32), err_msg=call.name)
        n += x.shape[0] * x.shape[1]
    assert n > 500


def test_emulation_within_tolerance_on_the_case_table():
    """Both soft-max forms (and the pair form) in float32 and in the device's order, over every finite row of every call: inside the bound,
    and using a good part of it.  The bound is a worst case over ~40 roundings of one sign; the emulation's add up like their root and its
    exp is correctly rounded, so its worst row uses about a sixth (0.155 to 0.175)."""
    worst = {form: (0.0, "") for form in R.FORMS}
    rows = 0
    for call in R.CALLS:
        if call.category in ("padding", "offset") and (call.pad or call.off):
            continue                                       # the rows of their base call
        d = diagonal(call)
        idx = np.arange(d.T)
        x = d.logits[:, idx, idx].reshape(-1, call.W)
        finite = np.isfinite(x[:, :call.V1].astype(np.float32)).all(-1)
        assert np.isfinite(d.prob.reshape(-1)[finite]).all()                 # (a row with a -inf range is defined and not finite)
        x, ref = x[finite], d.prob.reshape(-1)[finite]
        rows += len(x)
        for form in R.FORMS if call.V1 <= R.FITS_LOGITS else ("streaming",):
            got = R.device_order_emulation(x, call.V1, form)
            assert got.dtype == np.float32
            ratio = np.abs(got.astype(np.float64) - ref) / R.tolerance(ref, call.V1, form)
            k = int(ratio.argmax())
            assert ratio[k] <= 1.0, (call.name, form, k, got[k], ref[k], ratio[k])
            if ratio[k] > worst[form][0]:
                worst[form] = (float(ratio[k]), call.name)
    for form in R.FORMS:
        print(f"tdt-emulation {form} worst |error| / tolerance {worst[form][0]:.3f} ({worst[form][1]}) over {rows} rows")
    assert rows > 1400
    assert all(0.1 < worst[form][0] <= 1.0 for form in R.FORMS), worst


def test_emulation_forms_differ_only_in_rounding():
    x = diagonal(R.BY_NAME["boundary_f32_V1025"]).logits[0, :, 0]              # random rows
    regs, pairs, stream = (R.device_order_emulation(x, 1025, form) for form in R.FORMS)
    assert not np.array_equal(regs, pairs)                 # (registers and streaming add a row of 1 025 in nearly the same order)
    ref = R.reference(x, 1025, 5)[2]
    for got, form in ((regs, "registers"), (pairs, "pairs"), (stream, "streaming")):
        assert (np.abs(got - ref) <= R.tolerance(ref, 1025, form)).all()


def test_table_reaches_every_instance_in_every_category():
    by_call = {cat: set() for cat in R.CALL_CATEGORIES}
    by_row = {cat: set() for cat in R.ROW_CATEGORIES}
    patterns = {}
    sizes = set()
    for call in R.CALLS:
        inst = call.instance(tdt_route)
        assert inst in R.INSTANCES
        assert (call.form(tdt_route) == "streaming") == (call.V1 > R.FITS_LOGITS)
        by_call[call.category].add(inst)
        d = diagonal(call)
        sizes.add((d.B, d.T))
        assert d.B <= 8 and d.T <= (17 if call.V1 > R.FITS_LOGITS else 33) and d.logits.size < 16 * 2 ** 20
        assert d.logits.shape == (d.B, d.T, d.T, call.V1 + call.nd + call.pad)
        for chunk in d.specs:
            for kind, cat, pattern in chunk[:-1]:
                by_row[cat].add(inst)
                patterns.setdefault((call.nd, call.target, inst), set()).add(pattern)
    for cat, got in {**by_call, **by_row}.items():
        assert got == set(R.INSTANCES), (cat, got)
    print("tdt-table every category on", sorted(R.INSTANCES))
    assert {1, 3} <= {b for b, _ in sizes}                                   # one chunk, an odd number of chunks
    # every V1 boundary on the fp32 instance and on every fp16 instance that can serve it
    for V1 in R.BOUNDARY_V1:
        got = {c.instance(tdt_route) for c in R.of_category("boundary") if c.V1 == V1}
        assert got == ({"f32_registers", "f16_halves", "f16_pairs"} if V1 <= R.FITS_LOGITS else {"f32_streaming", "f16_streaming"}), V1
    assert {1088, 1089} <= set(R.BOUNDARY_V1)
    # every (nd, target) on all five, with every way of selecting the target
    for nd, target in R.ND_TARGETS:
        for inst in R.INSTANCES:
            assert patterns[(nd, target, inst)] >= set(R.duration_patterns(nd, target)) | {"dominate_all"}, (nd, target, inst)
            assert ("dominate_first" in patterns[(nd, target, inst)]) == (target == 0)
    assert {nd for nd, _ in R.ND_TARGETS} == {1, 2, 5, 8} and all((nd, nd - 1) in R.ND_TARGETS and (nd, 0) in R.ND_TARGETS for nd in (1, 2, 5, 8))
    # padding and offsets: fp16 flips between halves and pairs with the parity of the stride and with a base that is 2 mod 4
    pads = {(c.pad, c.instance(tdt_route)) for c in R.of_category("padding") if c.f16 and c.V1 == 1025}
    assert pads == {(0, "f16_pairs"), (1, "f16_halves"), (2, "f16_pairs"), (3, "f16_halves"), (7, "f16_halves")}
    offs = {(c.off, c.instance(tdt_route)) for c in R.of_category("offset") if c.f16 and c.V1 == 1025}
    assert offs == {(0, "f16_pairs"), (1, "f16_halves"), (2, "f16_pairs"), (3, "f16_halves")}
    assert {c.pad for c in R.of_category("padding")} == set(R.PADS) and {c.off for c in R.of_category("offset")} == set(R.OFFSETS)


def test_dominating_duration_logits_would_change_a_leaky_decision():
    """What the rows of category "dominate" are for: on each of them a duration logit exceeds every token logit by 20, so a kernel that let
    one into the token's arg-max or soft-max would answer another token or another probability — and on the pair route with odd V1 the first
    duration logit shares a dword with the last token logit.  The reference is that of the same row with small duration logits."""
    seen = set()
    for call in R.CALLS:
        d = diagonal(call)
        V1, nd = call.V1, call.nd
        for b, chunk in enumerate(d.specs):
            for k, (kind, cat, pattern) in enumerate(chunk):
                if cat != "dominate":
                    continue
                row = d.logits[b, k, k].astype(np.float32)
                assert row[V1] >= row[:V1].max() + 20.0
                assert pattern == "dominate_first" or (row[V1:V1 + nd] >= row[:V1].max() + 20.0).all()
                leaky = R.reference(np.append(row[:V1 + 1], np.float32(0.0))[None], V1 + 1, 1)
                assert int(leaky[0][0]) == V1 and leaky[2][0] > 1.0 - 1e-6        # with it, the answer is the duration logit's index, certain
                quiet = row.copy()
                quiet[V1:V1 + nd] = 0.0
                t, _, p = R.reference(quiet[None], V1, nd)
                assert int(t[0]) == d.token[b, k] and p[0] == d.prob[b, k]
                seen.add((call.instance(tdt_route), V1 % 2, pattern))
    assert {("f16_pairs", 1, "dominate_all"), ("f16_pairs", 1, "dominate_first"), ("f16_pairs", 0, "dominate_all")} <= seen
    assert {inst for inst, _, _ in seen} == set(R.INSTANCES)


def test_padding_is_poison_and_ignored():
    for call in R.of_category("padding") + [c for c in R.of_category("boundary") if c.pad]:
        d = diagonal(call)
        used = call.V1 + call.nd
        if call.pad:
            tail = d.logits[..., used:].astype(np.float32)
            assert not np.isfinite(tail).all() and (np.isnan(tail) | (tail >= 6e4)).all()
            if call.pad * d.logits[..., 0].size >= 3:
                assert np.isnan(tail).any() and np.isposinf(tail).any() and np.isfinite(tail).any()
        base = diagonal(call.base)
        assert np.array_equal(d.logits[..., :used].view(np.uint16 if call.f16 else np.uint32),
                              base.logits.view(np.uint16 if call.f16 else np.uint32))
        assert np.array_equal(d.token, base.token) and np.array_equal(d.prob, base.prob, equal_nan=True)


def test_every_row_is_a_compared_decision(oracle_mod):
    """The diagonal condition for every chunk of every call (expected_walks asserts it on the oracle's output: status 0, T - 1 tokens with
    timestamps 0 .. T - 2, which are the reference's diagonal), and no row of a call's list is missing from its chunks."""
    rows = 0
    for call in R.CALLS:
        d = diagonal(call)
        expected = R.expected_walks(d, oracle_mod)
        assert len(expected) == d.B and all(r["count"] == d.T - 1 for r in expected)
        placed = [spec for chunk in d.specs for spec in chunk[:-1]]
        wanted = R.row_specs(call)
        assert placed[:len(wanted)] == wanted and len(placed) == d.B * (d.T - 1)
        kinds = {kind for kind, _, _ in placed}
        assert kinds >= {kind for kind, _ in R.token_kinds(call.V1, call.rows)}
        rows += len(placed)
        # the comparison passes on the oracle's own answer and notices a confidence that is off, a lost zero and a wrong token
        assert R.compare_walks(expected, d, expected, call.form(tdt_route)) < 0.1    # (the rounding of the reference to float32)
    print(f"tdt-diagonal {rows} rows in {len(R.CALLS)} calls, none skipped")
    assert rows > 2000


def test_compare_notices_what_it_should(oracle_mod):
    call = R.BY_NAME["boundary_f16_V65"]
    d = diagonal(call)
    expected = R.expected_walks(d, oracle_mod)
    form = call.form(tdt_route)

    def changed(b, key, k, value):
        got = [dict(r, **{name: np.array(r[name]) for name in ("tokens", "timestamps", "durations", "confidences")}) for r in expected]
        got[b][key][k] = value
        return got

    finite = int(np.flatnonzero(np.isfinite(d.prob[0, :-1]))[0])
    undefined = int(np.flatnonzero(~np.isfinite(d.prob[0, :-1]))[0])
    inside = expected[0]["confidences"][finite] * np.float32(1 + 2.0 ** -23)
    assert R.compare_walks(changed(0, "confidences", finite, inside), d, expected, form) > 0.0
    for got in (changed(0, "confidences", finite, expected[0]["confidences"][finite] * np.float32(1 + 1e-5)),
                changed(0, "confidences", undefined, np.float32(1e-30)), changed(0, "tokens", 2, int(expected[0]["tokens"][2]) + 1),
                changed(d.B - 1, "durations", 0, 2)):
        with pytest.raises(AssertionError):
            R.compare_walks(got, d, expected, form)
