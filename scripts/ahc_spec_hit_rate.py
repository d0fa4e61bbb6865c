"""How often the merge after a merge can be foreseen (CPU only; DESIGN.md 3.3, the speculative round).

A numpy restatement of the filter linkage on the bench's session generator.  Before each merge it predicts the next one the way the speculative round
does: the block-partial minima (256-slot blocks) of the row the previous merge produced, re-ranked by their Lance-Williams value for the cluster about to
be formed; the counts compare that guess ("hit_blk"), the top two per block, and unranked minima of the row with the merge that actually follows.

    python scripts/ahc_spec_hit_rate.py <hours> [sigma]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
from e2e_inputs import e2e_session
s = e2e_session(hours=float(sys.argv[1]), sigma=float(sys.argv[2]) if len(sys.argv) > 2 else 0.03)
X = np.asarray(s["emb"], np.float64)
X /= np.linalg.norm(X, axis=1, keepdims=True)
N = len(X); BLK = 256; nblk = (N + BLK - 1) // BLK
sq = (X * X).sum(1)
D = sq[:, None] + sq[None, :] - 2 * X @ X.T
np.maximum(D, 0, out=D); np.fill_diagonal(D, np.inf)
size = np.ones(N); alive = np.ones(N, bool)
d1 = D.min(1); nn = D.argmin(1)
prev = None; pred = None
st = dict(merges=0, snow=0, hit_blk=0, hit_top2blk=0, hit_glob8=0, hit_glob32=0, norank1=0, norank2=0)
for k in range(N - 1):
    a = int(np.argmin(d1)); b = int(nn[a]); dab = D[a, b]
    if a > b: a, b = b, a
    if pred is not None:
        kept, zs = pred
        st["merges"] += 1
        pair = {a, b}
        if kept in pair: st["snow"] += 1
        for key, z in zs.items():
            if key == "norank2":
                if z is not None and any(pair == {kept, int(q)} for q in z): st[key] += 1
            elif z is not None and pair == {kept, z}: st[key] += 1
    # candidates from the row of the previous result R (the row whose block minima the records carry)
    cands = {}
    if prev is not None and alive[prev]:
        r = D[prev].copy(); r[[a, b]] = np.inf
        pad = np.full(nblk * BLK, np.inf); pad[:N] = r
        blocks = pad.reshape(nblk, BLK)
        bi = blocks.argmin(1) + np.arange(nblk) * BLK
        bi = bi[np.isfinite(pad[bi])]
        two = np.argsort(blocks, 1)[:, :2] + np.arange(nblk)[:, None] * BLK
        two = two.ravel(); two = two[np.isfinite(pad[two])]
        order = np.argsort(r); g8 = order[:8]; g32 = order[:32]
        cands = dict(hit_blk=bi, hit_top2blk=two, hit_glob8=g8, hit_glob32=g32)
    na, nb = size[a], size[b]; t = na + nb
    new = (na * D[a] + nb * D[b]) / t - na * nb * dab / (t * t)
    new[a] = np.inf; new[b] = np.inf; new[~alive] = np.inf
    zz = {key: (int(c[np.argmin(new[c])]) if len(c) else None) for key, c in cands.items()}
    if cands:
        zz["norank1"] = int(order[0]); zz["norank2"] = order[:2]
    pred = (a, zz)
    D[a] = new; D[:, a] = new; D[b] = np.inf; D[:, b] = np.inf
    alive[b] = False; d1[b] = np.inf; size[a] = t
    stale = np.where(alive & ((nn == a) | (nn == b)))[0]
    upd = alive & (new < d1)
    d1[upd] = new[upd]; nn[upd] = a
    for i in stale:
        d1[i] = D[i].min(); nn[i] = D[i].argmin()
    d1[a] = D[a].min(); nn[a] = D[a].argmin()
    if not np.isfinite(d1[a]): d1[a] = np.inf
    prev = a
print("N", N, {k: (v, round(v / max(1, st['merges']), 4)) for k, v in st.items()})
