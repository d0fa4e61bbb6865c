"""fa_tdt_greedy_logits_lang_dev against the language-mode walk of tests/tdt_lang_restatement.py, one call per kernel instance of
csrc/tdt.hip (fp32 registers, fp16 halves, fp16 pairs, both streaming instances) at V1 = 129, 1 088, 1 089 and 8 193 with K = 64, one call
with K = 3, all three scripts, the blocklist on and — on the rows of two of the calls — off.  Every call holds a row of each kind of
G.KINDS (tests/test_tdt_lang_cpu.py proves that, and that each gets the outcome its name says, from the restatement alone; the three
blocklist kinds do not exist in a call without the blocklist).  Tokens, timestamps, durations, routes, swap counts, status, final_u and
final_time must be equal; the confidence of a token the filters left alone lies within tdt_logits_restatement.tolerance, that of a
replaced token within G.swap_tolerance, and it is exactly 0 where the reference says 0.  With a table in which every token is LATIN_OK
and script Latin the entry equals fa_tdt_greedy_logits_dev bit for bit.

Every call prints `tdt-lang-ratio <call> <largest |error| / swap_tolerance> <largest |error| / tolerance>`; read them with -s.
Measured on an MI355X: replaced tokens 0.104 (fp32 registers, V1 = 129), 0.078 (fp16 pairs), 0.072 (fp16 halves, V1 = 1 088), 0.076 (fp32
streaming, V1 = 1 089), 0.022 / 0.030 (fp16 / fp32 streaming, V1 = 8 193), 0.062 (K = 3); tokens the filters left alone 0.058 – 0.177.  The
float32 emulation of tests/test_tdt_lang_cpu.py puts its worst replaced token at 0.114 of the bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_lang_restatement as G  # noqa: E402
import tdt_logits_restatement as R  # noqa: E402
from test_decoder_routes import tdt_route  # noqa: E402
from test_gpu_tdt_logits import device_matrix, instance_of  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 77
_TABLES = {}


def table_of(call):
    """The call's table; the reference side is computed once and left alone."""
    if call.name not in _TABLES:
        _TABLES[call.name] = G.lang_table(call)
    return _TABLES[call.name]


def config_of(fa, call):
    return fa.TdtConfig(blank_id=call.V1 - 1)


@pytest.mark.parametrize("call", G.LANG_CALLS, ids=[c.name for c in G.LANG_CALLS])
def test_language_mode_walk(fa, gpu_ctx, call):
    t = table_of(call)
    buf, view = device_matrix(t.logits, 0)
    assert instance_of(call.f16, call.V1, view) == call.instance(tdt_route)
    classes = fa.tdt_token_classes(t.vocabulary, sorted(t.blocklist))
    np.testing.assert_array_equal(classes, t.classes)
    got = fa.tdt_decode_logits_lang(view, call.V1, classes, fa.Script(call.script), [G.CHUNK_T] * t.B, is_last=t.is_last, use_blocklist=call.blocklist,
                                    top_k=call.K, config=config_of(fa, call), max_out=G.CHUNK_U, ctx=gpu_ctx)
    form = call.form(tdt_route)
    worst_swap = worst_plain = 0.0
    assert len(got) == t.B
    for b, (g, r) in enumerate(zip(got, t.expected)):
        where = f"{call.name} chunk {b}"
        assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (r["status"], r["count"], r["final_u"], r["final_time"]), where
        assert tuple(g["swap_counts"]) == tuple(r["swap_counts"]), (where, g["swap_counts"], r["swap_counts"])
        for key in ("tokens", "timestamps", "durations", "routes"):
            np.testing.assert_array_equal(g[key], r[key], err_msg=f"{where} {key}")
        emitted = {e[5]: (e, d) for e, d in zip(r["trace"], r["decisions"]) if e[5] >= 0}
        conf = g["confidences"]
        assert conf.dtype == np.float32 and conf.shape == r["confidences"].shape
        for i in range(r["count"]):
            (phase, u, frame, tok, route, _), (raw, prob, lst, xb) = emitted[i]
            kind = t.cells[b].get((u, frame))
            ref = float(R.clamp(prob))
            if route:
                tol = G.swap_tolerance(lst, xb, call.V1)
            else:
                tol = float(R.tolerance(prob, call.V1, form))
            err = abs(float(conf[i]) - ref)
            print(f"tdt-lang-conf {where} token {i} {kind} route {route}: device {conf[i]!r} reference {ref!r} tolerance {tol!r}")
            if tol == 0.0:
                assert conf[i] == 0.0 and ref == 0.0, (where, i, kind, conf[i])
            else:
                assert err <= tol, f"{where} token {i} {kind} route {route}: confidence {conf[i]!r}, reference {ref!r}, |error| / tolerance {err / tol:.3f}"
                if route:
                    worst_swap = max(worst_swap, err / tol)
                else:
                    worst_plain = max(worst_plain, err / tol)
    print(f"tdt-lang-ratio {call.name} {worst_swap:.3f} {worst_plain:.3f}")


@pytest.mark.parametrize("name", ["f32_registers_V129_latin", "f16_pairs_V129_cyrillic", "f16_halves_V1088_greek", "f32_streaming_V1089_cyrillic",
                                  "f16_streaming_V8193_latin"])
def test_nothing_to_filter_is_the_plain_entry(fa, gpu_ctx, name):
    """Every token LATIN_OK and in the vocabulary, script Latin, the blocklist on with nothing on it: no decision differs from
    fa_tdt_greedy_logits_dev, and no confidence by a bit; routes and swap counts are 0."""
    call = G.LANG_BY_NAME[name]
    t = table_of(call)
    buf, view = device_matrix(t.logits, 0)
    classes = np.full(call.V1, G.LATIN_OK | G.IN_VOCAB, np.uint8)
    args = ([G.CHUNK_T] * t.B,)
    kw = dict(is_last=t.is_last, config=config_of(fa, call), max_out=G.CHUNK_U, ctx=gpu_ctx)
    plain = fa.tdt_decode_logits(view, call.V1, *args, **kw)
    lang = fa.tdt_decode_logits_lang(view, call.V1, classes, fa.Language.FRENCH, *args, use_blocklist=True, **kw)
    for b, (g, r) in enumerate(zip(lang, plain)):
        assert (g["status"], g["count"], g["final_u"], g["final_time"]) == (r["status"], r["count"], r["final_u"], r["final_time"]), (name, b)
        for key in ("tokens", "timestamps", "durations"):
            np.testing.assert_array_equal(g[key], r[key], err_msg=f"{name} {b} {key}")
        assert np.array_equal(g["confidences"].view(np.uint32), r["confidences"].view(np.uint32)), (name, b)
        assert not g["routes"].any() and g["swap_counts"] == (0, 0) and r["count"] > 0


def test_entry_contract(fa, gpu_ctx):
    """NULL classes, top_k = 0 and 65, a script outside 0 .. 2 and NULL swap counts are FA_INVALID_ARGUMENT before any launch: the
    sentinel-filled outputs are untouched.  The same call with good arguments succeeds."""
    import torch
    lib, L = fa._lib, fa.lib()
    call = G.LANG_BY_NAME["f32_registers_V129_latin"]
    t = table_of(call)
    B, U, T, W = t.logits.shape
    x = torch.from_numpy(t.logits.copy()).cuda()
    enc = torch.full((B,), T, dtype=torch.int32, device="cuda")
    cls = torch.from_numpy(t.classes).cuda()
    cfg = config_of(fa, call).c()

    def outputs():
        o = {k: torch.full((B, U), SENTINEL, dtype=torch.int32, device="cuda") for k in ("tok", "time", "dur", "route")}
        o["conf"] = torch.full((B, U), float(SENTINEL), dtype=torch.float32, device="cuda")
        o.update({k: torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda") for k in ("count", "final_time", "final_u", "status")})
        o["swaps"] = torch.full((B, 2), SENTINEL, dtype=torch.int32, device="cuda")
        return o

    good = dict(classes=cls.data_ptr(), script=0, top_k=64, swaps=True)

    def entry(o, **change):
        a = dict(good, **change)
        p = lambda name: C.c_void_p(o[name].data_ptr())  # noqa: E731
        st = L.fa_tdt_greedy_logits_lang_dev(gpu_ctx.handle, C.byref(cfg), C.c_void_p(x.data_ptr()), lib.DTYPE_F32, B, U, T, call.V1, W, C.c_void_p(enc.data_ptr()),
                                             None, None, None, None, None, U, p("tok"), p("time"), p("dur"), p("conf"), p("count"), p("final_time"),
                                             p("final_u"), p("status"), None if a["classes"] is None else C.c_void_p(a["classes"]), a["script"], 1,
                                             a["top_k"], p("route"), p("swaps") if a["swaps"] else None)
        gpu_ctx.synchronize()
        return st

    for name, change in {"null_classes": dict(classes=None), "top_k_0": dict(top_k=0), "top_k_65": dict(top_k=65), "script_3": dict(script=3),
                         "script_negative": dict(script=-1), "null_swap_counts": dict(swaps=False)}.items():
        o = outputs()
        assert entry(o, **change) == lib.INVALID_ARGUMENT, name
        assert all(bool((v == SENTINEL).all()) for v in o.values()), name
    o = outputs()
    assert entry(o) == lib.SUCCESS
    r = G.walk_logits(t.logits[0], call.V1, G.ND, T, t.mode(), blank_id=call.V1 - 1, max_out=U)   # (is_last = 0 for both chunks here)
    assert int(o["count"][0]) == r["count"] and o["tok"][0, :r["count"]].cpu().numpy().tolist() == r["tokens"].tolist()
    assert tuple(o["swaps"][0].cpu().numpy().tolist()) == r["swap_counts"]
