"""Times fa_sortformer_stream_update_dev on one MI355X at the default geometry (DESIGN.md quotes the figures): B in {1, 64, 1024}, one
update in each of three regimes — append only (an empty FIFO takes 6 rows), pop (a FIFO of 36 rows pops 31 into an empty cache), pop +
compress (the same pop into a full cache of 188 rows).  An update advances its state, so every timed launch is preceded by two device
copies that put the two length arrays back (the regime depends on nothing else); the copies are also timed alone and the figures are
launch + copies minus copies.  `inner` launches on resident operands between two device events on the context's stream, ten windows, the
median and the spread.  Beside each: the bytes the update moves and the fraction of the HBM data-sheet rate.  --dry stops before the
device work (no GPU needed)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC = 8.0e12          # bytes / s, MI355X data sheet


class DeviceView:
    """A device address as torch sees an array (the state's length arrays, fixed for its lifetime)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def regime_bytes(cfg, g, regime):
    """What one stream's update reads and writes, rows of d_model floats and pred rows of `speakers` floats."""
    row, pred = cfg.d_model * 4, cfg.speakers * 4
    core, pop, fifo = cfg.chunk_len, 31, 36
    if regime == "append":
        return 2 * core * row + 4 * core * pred + (core + cfg.chunk_right_context) * pred
    moved = 2 * pop * row + 2 * (fifo + core - pop) * row + (fifo - (fifo + core - pop)) * row   # popped rows, the shift, the zeroed tail
    preds = (fifo + 2 * core + cfg.chunk_right_context) * pred + 2 * (fifo + core) * pred
    if regime == "pop":
        return moved + preds
    cap = g.spkcache_len
    return moved + preds + 4 * cap * row + (2 * cap + pop) * pred + cap * 4                      # the gather through scratch: two reads, two writes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    args = ap.parse_args()
    import fluidaudio_amd as fa
    cfg = fa.SortformerStreamConfig()
    g = cfg.geometry()
    print(f"config: cache {g.spkcache_len}, fifo {cfg.fifo_len}, chunk {cfg.chunk_len}+{cfg.chunk_left_context}+{cfg.chunk_right_context}, period {g.spkcache_update_period}, "
          f"d_model {cfg.d_model}, score rows {g.score_rows}, control kernel LDS {g.lds_bytes} bytes", flush=True)
    if args.dry:
        return
    import torch
    ctx = fa.default_context(0)
    own = torch.cuda.ExternalStream(ctx.stream, device=ctx.device)
    rows = []
    for B in args.batches:
        gen = torch.Generator(device="cuda").manual_seed(B)
        st = fa.SortformerStreamState(B, cfg, ctx)
        ptrs = st.input_pointers()
        spk_len, fifo_len = (torch.as_tensor(DeviceView(ptrs[i], B), device="cuda") for i in (1, 3))
        M, stride = g.out_rows, g.spkcache_len + cfg.fifo_len + g.out_rows
        embs = torch.randn((B, M, cfg.d_model), generator=gen, device="cuda")
        preds = torch.rand((B, stride, cfg.speakers), generator=gen, device="cuda")
        vec = lambda v: torch.full((B,), v, dtype=torch.int32, device="cuda")  # noqa: E731
        emb_len, pred_rows, left, right = vec(M), vec(stride), vec(cfg.chunk_left_context), vec(cfg.chunk_right_context)
        out = st.update_dev(embs, emb_len, preds, pred_rows, left, right)          # from empty: an append
        while True:                                                                # until every cache is full and has compressed once
            out = st.update_dev(embs, emb_len, preds, pred_rows, left, right, out=out)
            ctx.synchronize()
            snap = st.get(0)
            if snap.spkcache_length == g.spkcache_len and snap.spkcache_preds_present:
                break
        assert int(out.status.max()) == 0
        full, zero, fifo36 = vec(g.spkcache_len), vec(0), vec(36)
        regimes = {"append": (zero, zero), "pop": (zero, fifo36), "compress": (full, fifo36)}
        # "pop" runs on a cache whose preds are present: its popped preds are appended, nothing else differs
        torch.cuda.synchronize()

        def window(kind):
            spk0, fifo0 = regimes["append" if kind == "copy" else kind]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(own):
                e0.record(own)
                for _ in range(args.inner):
                    spk_len.copy_(spk0)
                    fifo_len.copy_(fifo0)
                    if kind != "copy":
                        st.update_dev(embs, emb_len, preds, pred_rows, left, right, out=out)
                e1.record(own)
            ctx.synchronize()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.inner    # microseconds per (copies + update)

        kinds = ("copy", "append", "pop", "compress")
        for k in kinds:
            window(k), window(k)
        times = {k: [] for k in kinds}
        for _ in range(args.repeats):
            for k in kinds:
                times[k].append(window(k))
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k in kinds[1:]:
            us = max(med[k] - med["copy"], 1e-3)
            nbytes = B * regime_bytes(cfg, g, k)
            row = dict(B=B, regime=k, us=us, copies_us=med["copy"], spread_us=[float(np.min(times[k])), float(np.max(times[k]))], bytes=nbytes,
                       hbm_fraction_spec=nbytes / (us * 1e-6) / HBM_SPEC)
            print(json.dumps(row), flush=True)
            rows.append(row)
        st.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
