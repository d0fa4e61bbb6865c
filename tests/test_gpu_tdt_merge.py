"""fa_tdt_merge_windows(_dev) on the device against the Python restatement of ChunkProcessor's seam merge
(tests/tdt_merge_restatement.py) on the batches of tests/tdt_merge_cases.py: tokens, timestamps, durations, confidences (by their
bytes), counts, statuses and routes.  No tolerances.  What each batch reaches is asserted on the restatement alone in
tests/test_tdt_merge_cpu.py."""
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_merge_cases as K  # noqa: E402
import tdt_merge_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def on_device(batch, fa, ctx, host=False):
    """The batch through the library: (per recording four arrays, statuses, routes, raw result)."""
    import torch
    p = K.pack(batch)
    kw = dict(splice_safe=p.safe, case_canon=p.canon, vocab=batch.vocab, overlap_seconds=batch.overlap, capacities=p.caps, ctx=ctx)
    if host:
        m = fa.merge_windows(p.tok, p.time, p.dur, p.conf, p.counts, p.window_range, **kw)
        flat = (m.tokens, m.timestamps, m.durations, m.confidences)
    else:
        d = [torch.from_numpy(a).cuda() for a in (p.tok, p.time, p.dur, p.conf, p.counts)]
        m = fa.merge_windows_dev(*d, p.window_range, **kw)
        flat = tuple(t.cpu().numpy() for t in (m.tokens, m.timestamps, m.durations, m.confidences))
    streams = [tuple(a[m.out_range[r]:m.out_range[r] + m.counts[r]] for a in flat) for r in range(len(batch.recs))]
    return streams, m.statuses, m.routes, (flat, m)


def check(batch, fa, ctx, host=False):
    got, statuses, routes, raw = on_device(batch, fa, ctx, host)
    want, w_statuses, w_routes = K.flatten(K.expected(batch))
    assert statuses.tolist() == w_statuses.tolist(), batch.name
    assert routes.tolist() == w_routes.tolist(), batch.name
    for r, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (batch.name, r)
    return raw


def test_the_17_pinned_cases(fa, gpu_ctx):
    n = 0
    for batch, want in K.pinned_batches():
        (flat, m) = check(batch, fa, gpu_ctx)
        for r, ids in enumerate(want):
            assert flat[0][m.out_range[r]:m.out_range[r] + m.counts[r]].tolist() == ids
        n += len(want)
    assert n == 17


def test_rounding_boundaries(fa, gpu_ctx):
    check(K.boundary_batch(), fa, gpu_ctx)


def test_overlap_sides_and_the_workspace_route(fa, gpu_ctx, switch):
    """Sides of 1 ... 130 tokens with the kernel's LDS limit, then everything small again with a limit of 4 tokens a side."""
    small = [K.side_batch(), K.edge_batch(), K.fold_batch()] + K.splice_batches() + [b for b, _ in K.pinned_batches()]
    check(K.side_batch(), fa, gpu_ctx)
    switch("FA_TDT_MERGE_LDS_SIDE", K.SMALL_LDS_SIDE)
    for b in small:
        check(b, fa, gpu_ctx)
    switch("FA_TDT_MERGE_LDS_SIDE", None)
    check(K.side_batch(), fa, gpu_ctx)


def test_strategy_edges_and_splice_routes(fa, gpu_ctx):
    check(K.edge_batch(), fa, gpu_ctx)
    for b in K.splice_batches():
        check(b, fa, gpu_ctx)


def test_folds_empty_windows_and_counts_beyond_max_out(fa, gpu_ctx):
    check(K.fold_batch(), fa, gpu_ctx)
    none = K.Batch("none", [], None, None, 0, R.OVERLAP)
    _, statuses, routes, _ = on_device(none, fa, gpu_ctx)
    assert statuses.size == 0 and routes.size == 0


def test_a_slice_one_token_short_fails_alone(fa, gpu_ctx):
    b = K.tight_batch()
    _, m = check(b, fa, gpu_ctx)
    assert m.statuses.tolist() == [0, 3, 0] and m.counts[1] == 0 and m.counts[0] == m.counts[2] > 0


def test_host_entry_and_dev_entry_give_the_same_bytes(fa, gpu_ctx):
    for b in (K.fold_batch(), K.fuzz_batches()[0], K.tight_batch()):
        flat_h, mh = check(b, fa, gpu_ctx, host=True)
        flat_d, md = check(b, fa, gpu_ctx, host=False)
        assert mh.counts.tolist() == md.counts.tolist() and mh.routes.tobytes() == md.routes.tobytes()
        for r in range(len(b.recs)):
            if mh.statuses[r] == 0:
                lo, hi = mh.out_range[r], mh.out_range[r] + mh.counts[r]
                assert all(x[lo:hi].tobytes() == y[lo:hi].tobytes() for x, y in zip(flat_h, flat_d))


def test_greedy_walk_outputs_chain_into_the_merge(fa, gpu_ctx):
    """fa_tdt_greedy_tables_dev over windows of 60 frames every 35 (global_offset set), its device outputs straight into
    merge_windows_dev; compared with the restatement of the same outputs copied back."""
    import torch
    L = fa._lib
    rng = np.random.default_rng(3)
    recs, per, T, U, stride, blank, max_out = 6, 4, 60, 64, 35, 8192, 48
    B = recs * per
    tok, goff = np.zeros((B, U, T), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        r, k = divmod(b, per)
        goff[b] = 1000 * r + stride * k
        g = goff[b] + np.arange(T)
        frame_tok = np.where((g * 2654435761 >> 7) % 3 == 0, (g * 7 + r) % 40, blank)       # what the recording says at a global frame
        flip = rng.random(T) < 0.08                                                         # what this window hears differently
        frame_tok = np.where(flip, rng.integers(0, 40, T), frame_tok)
        tok[b] = frame_tok[None, :]
    bins = np.ones((B, U, T), np.int32)
    prob = rng.random((B, U, T)).astype(np.float32)
    enc = np.full(B, T, np.int32)
    d = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    d_tok, d_bin, d_prob, d_enc, d_goff = d(tok), d(bins), d(prob), d(enc), d(goff)
    o_tok, o_time, o_dur = (torch.zeros((B, max_out), dtype=torch.int32, device="cuda") for _ in range(3))
    o_conf = torch.zeros((B, max_out), dtype=torch.float32, device="cuda")
    o_cnt, o_ft, o_fu, o_st = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(4))
    cfg = fa.TdtConfig().c()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    with gpu_ctx.torch_ordered():
        gpu_ctx.check(L.lib().fa_tdt_greedy_tables_dev(gpu_ctx.handle, C.byref(cfg), p(d_tok), p(d_bin), p(d_prob), B, U, T, p(d_enc), None, None, None, p(d_goff), None,
                                                       max_out, p(o_tok), p(o_time), p(o_dur), p(o_conf), p(o_cnt), p(o_ft), p(o_fu), p(o_st)), "fa_tdt_greedy_tables_dev")
    window_range = np.arange(0, B + 1, per, dtype=np.int64)
    safe, canon = R.fuzz_tables(40)
    s, c = R.tables(safe, canon, 40)
    m = fa.merge_windows_dev(o_tok, o_time, o_dur, o_conf, o_cnt, window_range, splice_safe=s, case_canon=c, ctx=gpu_ctx)
    h_tok, h_time, h_dur, h_conf, h_cnt = (t.cpu().numpy() for t in (o_tok, o_time, o_dur, o_conf, o_cnt))
    assert h_cnt.min() >= 5 and h_cnt.max() <= max_out and h_time.max() > 5000
    flat = [t.cpu().numpy() for t in (m.tokens, m.timestamps, m.durations, m.confidences)]
    seen = Counter()
    for r in range(recs):
        wins = [[(int(h_tok[b, i]), int(h_time[b, i]), int(h_dur[b, i]), float(h_conf[b, i])) for i in range(h_cnt[b])] for b in range(r * per, (r + 1) * per)]
        toks, status, routes = R.fold(wins, safe, canon)
        assert m.statuses[r] == status == 0 and m.routes[r * per:(r + 1) * per].tolist() == routes
        seen.update(x & 15 for x in routes[1:])
        lo, hi = m.out_range[r], m.out_range[r] + m.counts[r]
        for a, b in zip(flat, R.as_arrays(toks)):
            assert a[lo:hi].tobytes() == b.tobytes(), r
    assert seen[R.CONTIGUOUS] + seen[R.LCS] >= recs


def test_fuzz_batch(fa, gpu_ctx):
    batches = K.fuzz_batches()
    routes = Counter(x for b in batches for _, _, rt in K.expected(b) for x in rt if x >= 0)
    for base in (R.CONCAT, R.CONTIGUOUS, R.LCS, R.MIDPOINT):
        assert sum(v for k, v in routes.items() if k & 15 == base) >= 20
    for tail in (R.TAIL_ADOPT_RIGHT, R.TAIL_KEEP_LEFT):
        assert sum(v for k, v in routes.items() if k >> 4 == tail) >= 20
    assert 250 <= sum(len(b.recs) for b in batches) <= 350
    for b in batches:
        check(b, fa, gpu_ctx)


def test_device_time_is_reported(fa, gpu_ctx):
    lib = fa.lib()
    lib.fa_ctx_set_timing(gpu_ctx.handle, 1)
    try:
        check(K.edge_batch(), fa, gpu_ctx)
        assert 0.0 < lib.fa_ctx_last_device_ms(gpu_ctx.handle) < 1000.0
    finally:
        lib.fa_ctx_set_timing(gpu_ctx.handle, 0)
