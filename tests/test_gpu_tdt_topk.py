"""fa_tdt_topk_rows_dev (csrc/tdt_lang.h: tdt_topk_kernel<false>, <true>) against the ordered list of tests/tdt_lang_restatement.py: ids
and the bit patterns of the reported logits must be equal, slot by slot.  V1 on both sides of a wavefront, of the 17 x 64 logits the
register routes hold and of a streaming batch; K = 1, 2, 63, 64; fp32, and fp16 at scale 3, where natural ties are dense.  Rows: random,
flat (the list is ids 0 .. K - 1), a tie straddling the K-th place, -0.0 and +0.0 mixed (equal keys: a selection on raw bit patterns
would put +0.0 first), NaN / -inf / +inf, fewer than K entries above -inf.  Every matrix once contiguous and aligned, once with three
poisoned pad elements per row behind a base one element (fp16: two bytes) off a 16-byte boundary."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_lang_restatement as G  # noqa: E402
import tdt_logits_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

V1S = (1, 2, 63, 64, 65, 129, 1088, 1089, 2049, 8193)
KS = (1, 2, 63, 64)
MARGIN = 8


def rows_of(V1: int, K: int, f16: bool, rng):
    """[(kind, row float32 [V1])]: values the dtype holds exactly."""
    dt = np.float16 if f16 else np.float32
    scale = 3.0 if f16 else 1.0
    rnd = lambda: (rng.standard_normal(V1) * scale).astype(dt).astype(np.float32)  # noqa: E731
    out = [("random", rnd()), ("random", rnd()), ("flat", np.full(V1, 0.75, np.float32))]
    x = rnd()                                                        # K - 1 distinct tokens on top, then four tied for the K-th place
    order = rng.permutation(V1)
    top = np.float32(np.ceil(np.abs(x).max()) + 2.0)
    for r, i in enumerate(order[:K - 1]):
        x[i] = top + np.float32(K - r)
    x[order[K - 1:K + 3]] = top
    out.append(("tie_at_K", x))
    x = rnd()                                                        # zeros of both signs among negative values: the zeros lead, by id
    x = -np.abs(x) - np.float32(1.0)
    z = rng.permutation(V1)[:max(1, min(V1, K + 5))]
    x[z] = np.where(rng.random(z.size) < 0.5, np.float32(-0.0), np.float32(0.0))
    out.append(("signed_zeros", x))
    x = rnd()
    idx = rng.permutation(V1)
    x[idx[:V1 // 5]] = np.nan
    x[idx[V1 // 5:2 * V1 // 5]] = -np.inf
    x[idx[2 * V1 // 5:2 * V1 // 5 + 2]] = np.inf
    out.append(("nonfinite", x))
    out.append(("all_nan", np.full(V1, np.nan, np.float32)))
    x = np.full(V1, -np.inf, np.float32)                             # fewer than K entries above -inf: the list goes on by ascending id
    keep = rng.permutation(V1)[:min(V1, max(K // 2, 1)) if V1 > 1 else 0]
    x[keep] = rnd()[keep]
    x[rng.permutation(V1)[:V1 // 7]] = np.nan
    out.append(("few_above_ninf", x))
    return out


def device_rows(x: np.ndarray, pad: int, off: int):
    """x [R, V1] as a contiguous [R, V1 + pad] view `off` elements behind a 16-byte boundary of a poisoned allocation."""
    import torch
    lead = MARGIN + off
    W = x.shape[1] + pad
    host = R.poison(lead + x.shape[0] * W + MARGIN, x.dtype.type)
    body = host[lead:lead + x.shape[0] * W].reshape(x.shape[0], W)
    body[:, :x.shape[1]] = x
    buf = torch.from_numpy(host).cuda()
    view = buf[lead:lead + x.shape[0] * W].view(x.shape[0], W)
    assert view.is_contiguous() and (view.data_ptr() - off * x.itemsize) % 16 == 0
    return buf, view


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("V1", V1S)
def test_list_equals_the_restatement(fa, gpu_ctx, V1, f16):
    rng = np.random.default_rng([V1, int(f16)])
    dt = np.float16 if f16 else np.float32
    for K in KS:
        kinds, rows = zip(*rows_of(V1, K, f16, rng))
        x = np.stack(rows).astype(dt)
        ids, lg, cnt = G.topk_rows(x, V1, K)
        if V1 >= K:
            assert ids[kinds.index("flat")].tolist() == list(range(K))
        for pad, off in ((0, 0), (3, 1)):
            buf, view = device_rows(x, pad, off)
            g_ids, g_lg, g_cnt = fa.tdt_topk_rows(view, V1, K, ctx=gpu_ctx)
            assert g_ids.dtype == np.int32 and g_lg.dtype == np.float32 and g_ids.shape == (len(rows), K)
            for r, kind in enumerate(kinds):
                where = f"V1={V1} K={K} {kind} pad={pad} off={off}"
                np.testing.assert_array_equal(g_ids[r], ids[r], err_msg=where)
                np.testing.assert_array_equal(g_lg[r].view(np.uint32), lg[r].view(np.uint32), err_msg=where)
            np.testing.assert_array_equal(g_cnt, cnt)
            assert (g_ids[:, min(K, V1):] == -1).all() and np.isneginf(g_lg[:, min(K, V1):]).all()


def test_entry_contract(fa, gpu_ctx):
    """K outside 1 .. 64, a row stride below V1, an unknown dtype and null buffers are FA_INVALID_ARGUMENT and write nothing; no rows is a
    success; counts may be null."""
    import ctypes as C

    import torch
    lib, L = fa._lib, fa.lib()
    x = torch.zeros((3, 10), dtype=torch.float32, device="cuda")
    ids = torch.full((3, 4), 77, dtype=torch.int32, device="cuda")
    lg = torch.full((3, 4), 77.0, dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    good = dict(rows=x, dtype=lib.DTYPE_F32, R=3, V1=10, stride=10, K=4, ids=ids, lg=lg)

    def entry(**change):
        a = dict(good, **change)
        st = L.fa_tdt_topk_rows_dev(gpu_ctx.handle, p(a["rows"]), a["dtype"], a["R"], a["V1"], a["stride"], a["K"], p(a["ids"]), p(a["lg"]), None)
        gpu_ctx.synchronize()
        return st

    for name, change in {"K_0": dict(K=0), "K_65": dict(K=65), "stride": dict(stride=9), "dtype": dict(dtype=7), "V1_0": dict(V1=0), "rows": dict(rows=None),
                         "ids": dict(ids=None), "logits": dict(lg=None), "R_negative": dict(R=-1)}.items():
        assert entry(**change) == lib.INVALID_ARGUMENT, name
        assert bool((ids == 77).all()) and bool((lg == 77.0).all()), name
    assert entry(R=0) == lib.SUCCESS and bool((ids == 77).all())
    assert entry() == lib.SUCCESS
    assert ids.cpu().numpy().tolist() == [[0, 1, 2, 3]] * 3 and bool((lg == 0.0).all())
