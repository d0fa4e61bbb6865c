#!/usr/bin/env python3
"""fa_tdt_greedy_tables_dev (tdt_kernel) timed with HIP events at the bench leg's shape (U = 64, T = 188; tables built as bench.tdt_leg builds
them: argmax / softmax of seeded logits with ~75 % blanks, a slice of 256 chunks at a time), B = 1 024 and 4 096, for the library named by
FLUIDAUDIO_HIP_LIBRARY.  One JSON line: per size the median and the minimum of 7 windows of 40 launches, and a checksum of the outputs."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluidaudio_amd as fa  # noqa: E402
from fluidaudio_amd import _lib as L  # noqa: E402
from fluidaudio_amd.tdt import TdtConfig  # noqa: E402

ctx = fa.Context(0)
BMAX, U, T, V1, nd, SL = 4096, 64, 188, 1025, 5, 256
g = torch.Generator(device="cuda").manual_seed(17)
tok = torch.empty((BMAX, U, T), dtype=torch.int32, device="cuda")
bn = torch.empty_like(tok)
pr = torch.empty((BMAX, U, T), dtype=torch.float32, device="cuda")
for b0 in range(0, BMAX, SL):
    part = torch.randn((SL, U, T, V1 + nd), generator=g, device="cuda", dtype=torch.float32)
    part[..., V1 - 1] += 4.0
    tok[b0:b0 + SL] = torch.argmax(part[..., :V1], dim=-1).to(torch.int32)
    bn[b0:b0 + SL] = torch.argmax(part[..., V1:], dim=-1).to(torch.int32)
    pr[b0:b0 + SL] = torch.softmax(part[..., :V1], dim=-1).amax(dim=-1)
    del part
torch.cuda.synchronize()
cfg = TdtConfig(blank_id=V1 - 1).c()
stream = torch.cuda.ExternalStream(ctx.stream)
pp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
out = {"lib": os.environ.get("FLUIDAUDIO_HIP_LIBRARY", "default")}
for B in (1024, 4096):
    v_enc = torch.full((B,), T, dtype=torch.int32, device="cuda")
    o = [torch.zeros((B, U), dtype=torch.int32, device="cuda") for _ in range(3)]
    o_conf = torch.zeros((B, U), dtype=torch.float32, device="cuda")
    o1 = [torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(4)]

    def run():
        ctx.check(fa.lib().fa_tdt_greedy_tables_dev(ctx.handle, C.byref(cfg), pp(tok), pp(bn), pp(pr), B, U, T, pp(v_enc), None, None, None, None, None, U,
                                                    pp(o[0]), pp(o[1]), pp(o[2]), pp(o_conf), pp(o1[0]), pp(o1[1]), pp(o1[2]), pp(o1[3])), "fa_tdt_greedy_tables_dev")
    torch.cuda.synchronize()
    for _ in range(5):
        run()
    ctx.synchronize()
    ms = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(40):
            run()
        e1.record(stream)
        ctx.synchronize()
        ms.append(e0.elapsed_time(e1) / 40)
    cnt = o1[0].cpu().numpy().astype(np.int64)
    mask = np.arange(U)[None, :] < cnt[:, None]
    chk = int(sum(int((t.cpu().numpy().astype(np.int64) * mask * (1 + np.arange(U))[None, :]).sum()) for t in o)) + int(cnt.sum()) * 1000003
    conf = float((o_conf.cpu().numpy().astype(np.float64) * mask).sum())
    out[f"B{B}"] = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_all": [round(m, 5) for m in ms], "tokens": int(cnt.sum()),
                    "status_nonzero": int((o1[3].cpu().numpy() != 0).sum()), "final_time_sum": int(o1[1].cpu().numpy().astype(np.int64).sum()),
                    "checksum": chk, "conf_sum": conf}
print(json.dumps(out), flush=True)
