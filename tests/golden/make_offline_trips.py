#!/usr/bin/env python3
"""Writes tests/golden/offline_trips_1h.npz: what the CPU restatement of OfflineDiarizerManager.cluster (oracle/) gives on the 1 h session of e2e_inputs.py
for the inputs of tests/test_gpu_offline_trips.py whose restatement is too slow for a test — no finite row (the linkage degrades to 5 400 singletons and
VBx runs on 5 400 speakers: two minutes on a host core), the forced speaker count and no PLDA features (6 - 10 s each).  Per input: assignments, centroids,
distinct AHC labels, VBx iterations, was_adjusted; and the digest of the session they belong to.

    python tests/golden/make_offline_trips.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

KINDS = ("none_finite", "forced", "no_rho")


def restatement(oracle, emb, rho, chunks, phi, kw, kind):
    """{assignments, centroids, initial (AHC labels), was_adjusted, elbos} as tests/test_gpu_pipeline.py computes them."""
    if kind == "no_rho":                                                    # AHC labels -> per-cluster means -> constrained assignment
        e64 = emb.astype(np.float64)
        init = oracle.ahc_cluster(e64, 0.6)
        cen = np.stack([np.cumsum(e64[init == k], axis=0)[-1] / (init == k).sum() for k in sorted(set(init.tolist()))])
        return {"assignments": oracle.constrained_assign(oracle.centroid_scores(e64, cen), chunks), "centroids": cen, "initial": init, "was_adjusted": False, "elbos": []}
    return oracle.cluster_embeddings(emb, rho, chunks, phi, **kw)


def main():
    import oracle
    from e2e_inputs import e2e_session, input_digest
    from test_gpu_offline_trips import _variant
    oracle.build()
    out = {"input_digest": np.array(input_digest(e2e_session(1.0)))}
    for kind in KINDS:
        emb, rho, chunks, phi, kw = _variant("1h", kind)
        ref = restatement(oracle, emb, rho, chunks, phi, kw, kind)
        out[kind + "_assignments"] = np.asarray(ref["assignments"], np.int32)
        out[kind + "_centroids"] = np.asarray(ref["centroids"], np.float64)
        out[kind + "_counts"] = np.array([max(1, len(set(np.asarray(ref["initial"]).tolist()))), len(ref["elbos"]), int(bool(ref["was_adjusted"]))], np.int64)
        print(kind, out[kind + "_centroids"].shape, out[kind + "_counts"].tolist(), flush=True)
    np.savez_compressed(os.path.join(HERE, "offline_trips_1h.npz"), **out)


if __name__ == "__main__":
    main()
