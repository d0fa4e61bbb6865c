"""Every `*_dev` entry behind a busy torch stream (tests/stream_order_cases.py holds the calls).  The entries enqueue on the context's own
stream, which nothing orders against torch's current stream but Context.torch_ordered in the wrappers; every other GPU test hands the
wrappers inputs that are complete.  Here each call runs in three arms:

  settled  fresh inputs, complete before the call: the expectation (its correctness is what the unit's own tests pin), and its wall time;
  stale    the stale inputs, complete before the call: it must differ from the settled arm, or the case could not fail;
  raced    the value tensors hold the stale version; torch's stream gets a delay of at least 4 x the settled call's wall time, then the
           producers (device copies of the fresh version), then an event.  The event must still be pending when the wrapper is called —
           else the test FAILS with "delay too short" —, the wrapper is called without any synchronisation, and every output tensor is
           cloned on torch's stream at once.  Only then is anything copied to the host.  The result must be the settled arm's bit for bit:
           the entry-side wait makes the kernels read the fresh version, the exit-side wait makes the clones read what the kernels wrote.
           Whether the race was still on is recorded where the order is made: Context.torch_ordered is watched during the call, and the
           event must be pending when the call reaches it (the first time, or every time of a session).  The few wrappers that upload a
           host argument on torch's stream first — the host then waits for the producers — are marked in the table with the line that
           does it; for them the test asserts that the race HAD ended, so the mark cannot go stale.  Cases whose wrapper returns device
           tensors without waiting also assert that the event is pending when it returns: their clones test the exit-side wait.

The two controls switch the bridge off with the wrapper's own order=False: there the raced arm must give the STALE arm's result bit for
bit, which shows on the machine that this harness sees a missing order.  Both versions of every late tensor are valid inputs, so a missing
order is a wrong answer and never a fault.  The delay is elementwise passes over a scratch tensor no case touches; how long a pass takes
is measured once per module.  The scratch is 256 MB so that a delay of some hundred milliseconds is a few thousand launches, which the
host enqueues far faster than the device runs them."""
import math
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_order_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

SCRATCH_FLOATS = 64 << 20
MARGIN = 4                 # the delay is at least this many settled calls long
PAD = 1.5                  # passes asked for beyond that: the clock the calibration saw may not be the clock of the delay
MIN_PASSES = 16


@pytest.fixture(scope="module")
def delay(gpu_ctx):
    """(passes(k): enqueue k passes on torch's current stream; seconds per pass, measured with two events after a warm-up)"""
    import torch
    scratch = torch.zeros(SCRATCH_FLOATS, dtype=torch.float32, device=f"cuda:{gpu_ctx.device}")

    def passes(k):
        for _ in range(k):
            scratch.add_(1.0).sub_(1.0)

    passes(64)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    passes(64)
    b.record()
    torch.cuda.synchronize()
    per_pass = a.elapsed_time(b) / 64 / 1000.0
    print(f"\nstream order: one pass over {SCRATCH_FLOATS * 4 >> 20} MB takes {per_pass * 1e6:.0f} us")
    return passes, per_pass


def upload(arrays, dev):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrays.items()}


def to_host(outputs):
    import torch
    return [None if x is None else x.cpu().numpy() if isinstance(x, torch.Tensor) else np.array(x) for x in outputs]


def same(x, y):
    """Bit for bit: integers as they are, floats through their bits, records through their bytes."""
    if x is None or y is None:
        return x is y
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.dtype.kind == "f":
        return np.array_equal(x.view(f"u{x.dtype.itemsize}"), y.view(f"u{y.dtype.itemsize}"))
    if x.dtype.kind in "iub":
        return np.array_equal(x, y)
    return x.tobytes() == y.tobytes()


def all_same(got, want):
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


def differing(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if not same(g, w)]


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_entry_is_ordered_against_a_busy_torch_stream(fa, gpu_ctx, delay, case):
    import torch
    passes, per_pass = delay
    dev = f"cuda:{gpu_ctx.device}"
    inp = case.build(fa, np.random.default_rng(0))
    assert inp.fresh.keys() == inp.stale.keys() and all(inp.fresh[k].shape == inp.stale[k].shape and inp.fresh[k].dtype == inp.stale[k].dtype and
                                                        np.isfinite(inp.stale[k]).all() and np.isfinite(inp.fresh[k]).all() for k in inp.fresh), "fresh and stale: same names, shapes, dtypes; finite"
    fresh, stale = upload(inp.fresh, dev), upload(inp.stale, dev)
    keep = []

    def run(values):
        """the call on settled addressing tensors of its own (an entry may write into what it is handed)"""
        args = dict(inp.host, **upload(inp.addr, dev), **values)
        assert "keep" not in args, "the name is the harness's"
        args["keep"] = keep
        if case.setup is not None:
            case.setup(fa, gpu_ctx, args)
        torch.cuda.synchronize()
        gpu_ctx.synchronize()
        return lambda: case.call(fa, gpu_ctx, args)

    def settle():
        torch.cuda.synchronize()
        gpu_ctx.synchronize()
        while keep:
            getattr(keep.pop(), "close", lambda: None)()

    def settled(values):
        call = run({k: v.clone() for k, v in values.items()})
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        gpu_ctx.synchronize()
        seconds = time.perf_counter() - t0
        host = to_host(out)
        settle()
        return host, seconds

    # (a) settled, after one warm-up call; (b) stale
    settled(fresh)
    want, seconds = settled(fresh)
    other, _ = settled(stale)
    assert not all_same(other, want), "the stale inputs give the settled result: this case cannot fail"

    # (c) raced
    bufs = {k: v.clone() for k, v in stale.items()}
    call = run(bufs)
    n = max(MIN_PASSES, math.ceil(PAD * MARGIN * seconds / per_pass))
    t_before, t_after, produced = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    t_before.record()
    passes(n)
    t_after.record()
    for k, buf in bufs.items():
        buf.copy_(fresh[k])
    produced.record()
    assert not produced.query(), f"delay too short: {n} passes were over before the call"
    bridge, ordered = [], gpu_ctx.torch_ordered

    def watched(enabled=True):
        """Context.torch_ordered, noting whether the producer is still pending when the call reaches it: whether the race is still on"""
        if enabled:
            bridge.append(not produced.query())
        return ordered(enabled)

    gpu_ctx.torch_ordered = watched
    try:
        out = call()
    finally:
        del gpu_ctx.torch_ordered
    returned_early = not produced.query()          # False: the host waited inside the call (the entry's own copies to the host, or an upload of the wrapper's)
    snaps = [x.clone() if isinstance(x, torch.Tensor) else x for x in out]
    torch.cuda.synchronize()
    measured = t_before.elapsed_time(t_after) / 1000.0
    got = to_host(snaps)
    settle()
    print(f"\nstream order {case.name}: settled {seconds * 1e3:.3f} ms, delay {measured * 1e3:.3f} ms ({n} passes, {measured / seconds:.1f} x), "
          f"producer pending at the call: yes, at the bridge: {sum(bridge)} of {len(bridge)}, after the call: {'yes' if returned_early else 'no'}")
    assert measured >= MARGIN * seconds, f"the delay ran {measured * 1e3:.3f} ms, below {MARGIN} x the settled call's {seconds * 1e3:.3f} ms"
    # was the race still on where the order is made?  A wrapper that uploads a host argument on torch's stream first has ended it by then
    if case.control:
        assert bridge == [], "order=False must not reach the bridge"
    elif case.live == "none":
        assert case.drains, "a case whose wrapper ends the race says where"
        assert bridge and not bridge[0], f"marked as drained ({case.drains}) but the producer was pending at the bridge: the mark is out of date"
    else:
        assert bridge and bridge[0], "the producer had finished before the call reached torch_ordered: nothing was raced (a host wait in the wrapper or the case)"
        assert case.live != "all" or all(bridge), f"the race ended inside the session: pending at the bridge {bridge}"
    assert returned_early or not case.exit_raced, "the host waited inside the call: the clones no longer test the exit-side wait"
    if case.control:
        assert all_same(got, other), f"order=False must read the stale inputs: outputs {differing(got, other)} differ from the stale arm"
    else:
        assert all_same(got, want), f"outputs {differing(got, want)} differ from the settled arm" + (": they are the stale arm's" if all_same(got, other) else "")


def test_cluster_stage_refuses_tensors_it_cannot_read(fa, gpu_ctx):
    """The device-pointer form reads float32 embeddings and float64 rho behind the pointers: anything else is refused before the library
    is called — an int32 tensor of the right shape used to be read as floats."""
    import torch
    emb, rho, chunks, phi = K._session(20, 3, 0)
    d_emb, d_rho = torch.from_numpy(emb).cuda(), torch.from_numpy(rho).cuda()
    wide = torch.from_numpy(np.concatenate([emb, emb], axis=1)).cuda()
    bad = [(d_emb.to(torch.int32), d_rho), (d_emb.to(torch.float16), d_rho), (d_emb, d_rho.to(torch.float32)), (d_emb, d_rho.to(torch.int64)),
           (wide[:, :256], d_rho), (d_emb, torch.cat([d_rho, d_rho], dim=1)[:, :128])]
    for e, r in bad:
        with pytest.raises(TypeError):
            fa.cluster_embeddings(e, r, chunks, phi, ctx=gpu_ctx)
        with pytest.raises(TypeError):
            fa.cluster_embeddings(e, r, chunks, phi, ctx=gpu_ctx, intermediates=True)
        with pytest.raises(TypeError):
            fa.cluster_embeddings_batch([(d_emb, d_rho, chunks), (e, r, chunks)], phi, ctx=gpu_ctx)
    with pytest.raises(TypeError):
        fa.cluster_embeddings(torch.from_numpy(emb), d_rho, chunks, phi, ctx=gpu_ctx)          # a CPU tensor is no device pointer
    one = fa.cluster_embeddings(d_emb, d_rho, chunks, phi, ctx=gpu_ctx)                         # and the right tensors are taken
    assert one.assignments == fa.cluster_embeddings(emb, rho, chunks, phi, ctx=gpu_ctx).assignments
