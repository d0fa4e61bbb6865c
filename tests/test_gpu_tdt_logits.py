"""fa_tdt_greedy_logits_dev against the float64 reference of tests/tdt_logits_restatement.py on every kernel instance of csrc/tdt.hip:
tdt_logits_fits_kernel<false, 1> (fp32, row in registers), <true, 1> (fp16, one half per request), <true, 2> (fp16 pairs), and
tdt_logits_kernel<false> / <true> (streaming).  A call reaches an instance through its dtype, V1, row stride and base pointer only
(tests/test_tdt_logits_cpu.py keeps the table on all five).  The table's rows — boundaries in V1, winner positions and exact ties, duration
logits that dominate the row, 1 / 2 / 5 / 8 duration bins, non-finite and extreme rows, padded rows full of poison, base pointers off a
16-byte boundary — lie on the diagonal of their chunk, where the walk decides on each and emits what it decided: integers must equal the
oracle's exactly, a confidence is within `tolerance` of the clamped reference and exactly 0 where the reference is undefined.  Then the
full walk (blanks, audio_frames, flush, offsets, emit_after, max_out = 1) over padded and offset matrices, the entry's argument contract
and the checks of the Python seam.

Largest |error| / tolerance measured on an MI355X over the 2 262 rows of the 116 calls of the table, per kernel instance (every call
prints `tdt-ratio <instance> <ratio> <call>`, the last test the five maxima; read them with -s):

    tdt_logits_fits_kernel<false, 1>   fp32, registers    0.175   V1 = 65
    tdt_logits_fits_kernel<true, 1>    fp16, halves       0.134   V1 = 65, row stride 71
    tdt_logits_fits_kernel<true, 2>    fp16, pairs        0.196   V1 = 65, row stride 70
    tdt_logits_kernel<false>           fp32, streaming    0.055   V1 = 1 100
    tdt_logits_kernel<true>            fp16, streaming    0.070   V1 = 1 100

The float32 emulation of tests/test_tdt_logits_cpu.py puts its worst rows at 0.175 (registers, streaming) and 0.155 (pairs): the device
is where its arithmetic says it should be.  The bound is a worst case over some forty roundings of one sign, so a sixth of it is what
roundings of random sign leave; no row came near it, and no pattern check failed: the tests found no bug in the kernels.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_logits_restatement as R  # noqa: E402
from test_decoder_routes import tdt_route  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 8             # poisoned elements either side of a matrix: 16 bytes of fp16, 32 of fp32
SENTINEL = 77
_CACHE = {}
WORST = {}


def diagonal(call, oracle_mod):
    """(Diagonal, expected walks) of a call; the reference side is computed once per call and left alone."""
    if call.name not in _CACHE:
        d = R.diagonal(call)
        d.logits.setflags(write=False)
        _CACHE[call.name] = (d, R.expected_walks(d, oracle_mod))
    return _CACHE[call.name]


def device_matrix(lg: np.ndarray, off: int):
    """lg [B, U, T, W] as a contiguous view `off` elements behind a 16-byte boundary of a larger allocation that is +inf, NaN and the
    dtype's largest finite value everywhere else.  Returns (allocation, view)."""
    import torch
    lead = MARGIN + off
    host = R.poison(lead + lg.size + MARGIN, lg.dtype.type)
    host[lead:lead + lg.size] = lg.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:lead + lg.size].view(*lg.shape)
    assert view.is_contiguous() and (view.data_ptr() - off * lg.itemsize) % 16 == 0 and (off == 0 or view.data_ptr() % 16 != 0)
    return buf, view


def instance_of(f16, V1, view):
    route = tdt_route(f16, V1, view.shape[-1], view.data_ptr())
    return ("f16_streaming" if f16 else "f32_streaming") if route == 0 else ("f16_pairs" if route == 2 else ("f16_halves" if f16 else "f32_registers"))


def run(fa, gpu_ctx, oracle_mod, call):
    """One call of the table: the walk over its diagonal chunks, compared with the reference.  Returns the entry's result."""
    d, expected = diagonal(call, oracle_mod)
    buf, view = device_matrix(d.logits, call.off)
    assert instance_of(call.f16, call.V1, view) == call.instance(tdt_route)
    cfg = fa.TdtConfig(blank_id=-1, duration_bins=call.duration_bins)
    got = fa.tdt_decode_logits(view, call.V1, [d.T] * d.B, config=cfg, max_out=d.T, ctx=gpu_ctx)
    worst = R.compare_walks(got, d, expected, call.form(tdt_route))
    inst = call.instance(tdt_route)
    print(f"tdt-ratio {inst} {worst:.3f} {call.name} B={d.B} T={d.T}")
    if worst > WORST.get(inst, (-1.0, ""))[0]:
        WORST[inst] = (worst, call.name)
    return got


def ids(calls):
    return [c.name for c in calls]


TABLE = R.of_category("boundary") + R.of_category("nd")
LAYOUT = R.of_category("padding") + R.of_category("offset")


@pytest.mark.parametrize("call", TABLE, ids=ids(TABLE))
def test_table_by_the_diagonal_walk(fa, gpu_ctx, oracle_mod, call):
    """Every V1 boundary on every instance that can serve it, with every winner position, tie, non-finite kind and dominating duration
    pattern that fits the row; 1, 2, 5 and 8 duration bins with the first and the last bin selected in every way a bin can be."""
    run(fa, gpu_ctx, oracle_mod, call)


@pytest.mark.parametrize("call", LAYOUT, ids=ids(LAYOUT))
def test_padded_rows_and_offset_bases(fa, gpu_ctx, oracle_mod, call):
    """The matrix carved out of a larger allocation: +inf, NaN and the largest finite value before it, behind it and in the pad elements of
    every row; the base 0 .. 3 elements off a 16-byte boundary.  Within the bound of the reference, all integers those of the contiguous
    aligned call on the same rows, and the confidences bit for bit wherever the same kernel instance served both."""
    got = run(fa, gpu_ctx, oracle_mod, call)
    base = run(fa, gpu_ctx, oracle_mod, call.base)
    d, _ = diagonal(call, oracle_mod)
    same = call.instance(tdt_route) == call.base.instance(tdt_route)
    assert same == (not call.f16 or call.V1 > R.FITS_LOGITS or ((call.pad % 2 == 0) and (call.off % 2 == 0)))
    for b, (g, r) in enumerate(zip(got, base)):
        assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (r["status"], r["count"], r["final_u"], r["final_time"]), b
        for key in ("tokens", "timestamps", "durations"):
            np.testing.assert_array_equal(g[key], r[key], err_msg=f"{call.name} chunk {b}")
        if same:
            assert np.array_equal(g["confidences"].view(np.uint32), r["confidences"].view(np.uint32)), (call.name, b)
        else:                                                  # halves against pairs: both within the bound of one reference
            ref = d.prob[b, :d.T - 1]
            both = R.tolerance(ref, call.V1, call.form(tdt_route)) + R.tolerance(ref, call.V1, call.base.form(tdt_route))
            assert (np.abs(g["confidences"].astype(np.float64) - r["confidences"]) <= both).all(), (call.name, b)


# ---- the full walk over strided matrices

SCN_B, SCN_U, SCN_T, SCN_ND = 8, 12, 17, 5


def scenario(V1, dtype):
    """The scenario of test_logits_walk_every_row_form_and_every_option (tests/test_gpu_tdt.py) at B = 8, U = 12, T = 17: ~50 % blanks,
    audio_frames, a chunk of one frame, a start frame beyond the chunk, last-chunk flush, offsets, emit_after; a tie, NaN and -inf rows."""
    rng = np.random.default_rng(V1 + 7)
    B, U, T, nd = SCN_B, SCN_U, SCN_T, SCN_ND
    blank = V1 - 1
    lg = rng.standard_normal((B, U, T, V1 + nd)).astype(np.float32)
    lg[..., blank] += 0.75 + 0.25 * np.log2(V1)           # about half of the decisions are blanks at every row length
    lg[2, 0, 0, 0] = lg[2, 0, 0, 4] = 30.0                 # exact tie -> lowest index
    lg[3, 0, 1, :V1] = np.nan                              # all NaN -> token 0, probability 0
    lg[4, 0, :4, 2] = np.nan                               # one NaN among finite logits
    lg[5, 0, :4, :V1] = -np.inf                            # nothing above -inf -> token 0
    lg[6, 0, :3, V1 - 2] = 40.0                            # the maximum in the row's last-but-one slot
    lg[7, 0, :3, V1:] = -np.inf                            # duration logits all -inf -> bin 0
    lg[7, 1, :, V1 + 1] = np.nan                           # a NaN duration logit never wins
    lg = lg.astype(dtype)
    enc = rng.integers(T // 2, T + 1, B).astype(np.int32)
    enc[0] = 1
    af = np.minimum(enc, rng.integers(T // 2, T + 4, B)).astype(np.int32)
    t0 = rng.integers(0, 4, B).astype(np.int32)
    t0[1] = T + 2
    last = (np.arange(B) % 2).astype(np.int32)
    goff = rng.integers(0, 300, B).astype(np.int32)
    ea = [None if b % 3 else int(goff[b] + 3) for b in range(B)]
    return lg, enc, af, t0, last, goff, ea


def padded(lg, pad):
    if not pad:
        return lg
    out = np.empty(lg.shape[:-1] + (lg.shape[-1] + pad,), lg.dtype)
    out[..., :lg.shape[-1]] = lg
    out[..., lg.shape[-1]:] = R.poison(out[..., lg.shape[-1]:].size, lg.dtype.type, pad).reshape(lg.shape[:-1] + (pad,))
    return out


# one V1 per kernel instance: fp16 rows of 130 + 5 logits are halves when contiguous and pairs with one pad element on an aligned base;
# rows of 131 + 5 are pairs when contiguous and stay pairs with two pad elements
@pytest.mark.parametrize("V1,dtype", [(130, "float32"), (130, "float16"), (131, "float16"), (1100, "float32"), (1100, "float16")])
def test_full_walk_over_padded_and_offset_matrices(fa, gpu_ctx, oracle_mod, V1, dtype):
    """The only place where the blank-advance and the flush phases see a strided matrix.  The contiguous aligned call against the oracle on
    numpy's tables (confidences within the bound), then row pads 1 and 2 on an aligned base and on one that is an element off: everything
    equals the contiguous aligned call — the confidences bit for bit where the same instance served both, within the bound otherwise."""
    f16 = dtype == "float16"
    lg, enc, af, t0, last, goff, ea = scenario(V1, dtype)
    nd, blank = SCN_ND, V1 - 1
    tok, bn, pr = R.reference(lg, V1, nd)
    cfg = fa.TdtConfig(blank_id=blank)
    seen = set()
    for max_out in (64, 1):
        calls = {}
        for pad, off in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
            buf, view = device_matrix(padded(lg, pad), off)
            seen.add(instance_of(f16, V1, view))
            calls[(pad, off)] = (instance_of(f16, V1, view), fa.tdt_decode_logits(view, V1, enc, af, t0, last, goff, ea, config=cfg, max_out=max_out, ctx=gpu_ctx))
        inst0, got0 = calls[(0, 0)]
        form0 = "streaming" if V1 > R.FITS_LOGITS else ("pairs" if inst0 == "f16_pairs" else "registers")
        refs = [oracle_mod.tdt_greedy(tok[b], bn[b], pr[b].astype(np.float32), enc[b], af[b], t0[b], bool(last[b]), goff[b], ea[b], max_out=max_out,
                                      blank_id=blank) for b in range(SCN_B)]
        tols = []
        for b, (g, r) in enumerate(zip(got0, refs)):
            assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (r["status"], r["count"], r["final_u"], r["final_time"]), (b, max_out)
            for key in ("tokens", "timestamps", "durations"):
                np.testing.assert_array_equal(g[key], r[key], err_msg=str(b))
            tol = R.tolerance(r["confidences"].astype(np.float64), V1, form0) + 2.0 ** -25 * r["confidences"]   # (the oracle's probability is float32)
            tols.append(tol)
            assert (np.abs(g["confidences"].astype(np.float64) - r["confidences"]) <= tol).all(), (b, max_out)
        assert 0 in {r["status"] for r in refs} and refs[0]["final_time"] is None and refs[1]["final_time"] is None
        if max_out == 64:
            assert sum(r["count"] for r in refs) > SCN_B and any(r["count"] and last[b] for b, r in enumerate(refs))
            assert any(r["joint_calls"] > r["count"] + 4 for r in refs)                  # blanks are walked over
        else:
            assert any(r["status"] != 0 for r in refs)                                   # room for fewer tokens than the walk emits
        for key, (inst, got) in calls.items():
            for b, (g, r) in enumerate(zip(got, got0)):
                assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (r["status"], r["count"], r["final_u"], r["final_time"]), (key, b, max_out)
                for name in ("tokens", "timestamps", "durations"):
                    np.testing.assert_array_equal(g[name], r[name], err_msg=f"{key} {b}")
                if inst == inst0:
                    assert np.array_equal(g["confidences"].view(np.uint32), r["confidences"].view(np.uint32)), (key, b, max_out)
                else:
                    assert (np.abs(g["confidences"].astype(np.float64) - r["confidences"]) <= 2.0 * tols[b]).all(), (key, b, max_out)
    assert seen == {"float32": {130: {"f32_registers"}, 1100: {"f32_streaming"}},
                    "float16": {130: {"f16_halves", "f16_pairs"}, 131: {"f16_halves", "f16_pairs"}, 1100: {"f16_streaming"}}}[dtype][V1]


# ---- the entry and the Python seam

def test_entry_contract(fa, gpu_ctx, oracle_mod):
    """fa_tdt_greedy_logits_dev itself: every malformed call is FA_INVALID_ARGUMENT and leaves the sentinel-filled outputs alone, an empty
    batch is a success that writes nothing, and without room for tokens (max_out = 0, null token buffers) the counts keep counting and the
    status is the oracle's."""
    import torch
    lib, L = fa._lib, fa.lib()
    call = R.Call("contract", "contract", False, 12, pad=3)
    d, expected = diagonal(call, oracle_mod)
    B, T, V1, nd, W = d.B, d.T, call.V1, call.nd, call.W
    x = torch.from_numpy(d.logits.copy()).cuda()
    enc = torch.full((B,), T, dtype=torch.int32, device="cuda")
    cfg = fa.TdtConfig(blank_id=-1, duration_bins=call.duration_bins)

    def outputs():
        o = {k: torch.full((B, T), SENTINEL, dtype=torch.int32, device="cuda") for k in ("tok", "time", "dur")}
        o["conf"] = torch.full((B, T), float(SENTINEL), dtype=torch.float32, device="cuda")
        o.update({k: torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda") for k in ("count", "final_time", "final_u", "status")})
        return o

    def untouched(o):
        return all(bool((t == SENTINEL).all()) for t in o.values())

    good = dict(logits=x.data_ptr(), dtype=lib.DTYPE_F32, batch=B, U=T, T=T, V1=V1, row_stride=W, enc=enc.data_ptr(), max_out=T, bins=nd, null_tokens=False)

    def entry(o, **change):
        a = dict(good, **change)
        c = cfg.c()
        c.n_duration_bins = a["bins"]
        p = lambda name: None if a["null_tokens"] and name in ("tok", "time", "dur", "conf") else C.c_void_p(o[name].data_ptr())  # noqa: E731
        st = L.fa_tdt_greedy_logits_dev(gpu_ctx.handle, C.byref(c), None if a["logits"] is None else C.c_void_p(a["logits"]), a["dtype"], a["batch"],
                                        a["U"], a["T"], a["V1"], a["row_stride"], C.c_void_p(a["enc"]), None, None, None, None, None, a["max_out"],
                                        p("tok"), p("time"), p("dur"), p("conf"), p("count"), p("final_time"), p("final_u"), p("status"))
        gpu_ctx.synchronize()
        return st

    bad = {"row_stride_one_short": dict(row_stride=V1 + nd - 1), "no_bins": dict(bins=0), "nine_bins": dict(bins=9), "dtype": dict(dtype=7),
           "null_logits": dict(logits=None), "U_0": dict(U=0), "batch_negative": dict(batch=-1), "null_token_buffers": dict(null_tokens=True)}
    for name, change in bad.items():
        o = outputs()
        assert entry(o, **change) == lib.INVALID_ARGUMENT, name
        assert untouched(o), name
    o = outputs()
    assert entry(o, batch=0) == lib.SUCCESS and untouched(o)
    assert entry(o, batch=0, logits=None) == lib.SUCCESS and untouched(o)
    # the smallest row stride the contract allows is the row itself; here the stride is three more, and the call the others derive from works
    o = outputs()
    assert entry(o) == lib.SUCCESS
    for b in range(B):
        assert (int(o["status"][b]), int(o["count"][b]), int(o["final_u"][b]), int(o["final_time"][b])) == (0, T - 1, T - 1, T)
        np.testing.assert_array_equal(o["tok"][b, :T - 1].cpu().numpy(), expected[b]["tokens"])
        assert int(o["tok"][b, T - 1]) == SENTINEL and float(o["conf"][b, T - 1]) == SENTINEL
    # no room at all
    o = outputs()
    assert entry(o, max_out=0, null_tokens=True) == lib.SUCCESS
    for b in range(B):
        tok, bn, prob = (t[b] for t in R.decision_tables(d))
        r = oracle_mod.tdt_greedy(tok, bn, prob, T, None, 0, False, 0, None, blank_id=-1, bins=call.duration_bins, max_out=0)
        assert r["count"] == T - 1 and r["status"] != 0
        assert (int(o["status"][b]), int(o["count"][b]), int(o["final_u"][b]), int(o["final_time"][b])) == (r["status"], r["count"], r["final_u"], r["final_time"])
    assert all(bool((o[k] == SENTINEL).all()) for k in ("tok", "time", "dur", "conf"))


def test_python_seam_checks_the_logits_tensor(fa, gpu_ctx):
    """decode_logits refuses, before any launch, logits that are not float16 / float32, not on the device, not [B, U, T, W], not
    contiguous, or whose rows cannot hold the token and the duration logits."""
    import torch
    B, T, V1 = 2, 4, 6
    x = torch.zeros((B, T, T, V1 + 5), dtype=torch.float32, device="cuda")
    enc = [T] * B
    wrong = {"float64": x.double(), "bfloat16": x.bfloat16(), "int32": x.int(), "host": x.cpu(), "three_dimensions": x[0], "five_dimensions": x[None],
             "not_contiguous": torch.zeros((B, T, T, V1 + 6), dtype=torch.float32, device="cuda")[..., :V1 + 5],
             "transposed": x.transpose(1, 2)[:, :, :T - 1], "numpy": x.cpu().numpy()}
    for name, t in wrong.items():
        with pytest.raises(AssertionError, match="decode_logits"):
            fa.tdt_decode_logits(t, V1, enc, ctx=gpu_ctx)
    with pytest.raises(AssertionError, match="cannot hold"):
        fa.tdt_decode_logits(x, V1 + 1, enc, ctx=gpu_ctx)
    with pytest.raises(AssertionError, match="cannot hold"):
        fa.tdt_decode_logits(x, V1, enc, config=fa.TdtConfig(duration_bins=(0, 1, 2, 3, 4, 5)), ctx=gpu_ctx)
    for t in (x, x.half()):                                   # what is accepted: flat rows decode to token 0, nothing is a blank
        got = fa.tdt_decode_logits(t, V1, enc, config=fa.TdtConfig(blank_id=-1, duration_bins=(1, 1, 1, 1, 1)), max_out=T, ctx=gpu_ctx)
        for g in got:
            assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (0, T - 1, T - 1, T) and g["tokens"].tolist() == [0] * (T - 1)
            tol = float(R.tolerance(1.0 / V1, V1, "registers"))
            assert (np.abs(g["confidences"].astype(np.float64) - 1.0 / V1) <= tol).all()


def test_worst_ratios(fa):
    """Runs last: the largest |error| / tolerance per kernel instance over the calls of this session (the figures of the module docstring)."""
    for inst in R.INSTANCES:
        if inst in WORST:
            print(f"tdt-worst {inst} {WORST[inst][0]:.3f} {WORST[inst][1]}")
    assert all(w <= 1.0 for w, _ in WORST.values())
