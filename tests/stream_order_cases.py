"""The calls tests/test_gpu_stream_order.py races against a busy torch stream: one case per public wrapper call (or per short session)
that reaches a `fa_*_dev` entry, and the two `device_pointers` forms of the clustering stage.  Plain data and small builders: importable
without a GPU, torch and the other case modules are imported inside the functions.

A case has
  name     what pytest shows,
  entries  the library functions the call reaches (tests/test_stream_order_inventory.py holds them against the wrappers' source),
  build    build(fa, rng) -> Inputs,
  setup    optional setup(fa, ctx, a): run with the addressing tensors, before the delay starts (plans and session objects: creating one
           synchronises, which would end the race before the entries under test are called),
  live     whether the race is still on when the call reaches the bridge — the test records it at every Context.torch_ordered —: at the
           "first" one, at "all", or at "none" because the wrapper itself uploads a host argument from pageable memory on torch's stream
           first (`drains` names the line).  A case marked "none" reaches its entries, but only a host wait orders them: it cannot fail.
  exit_raced  the producer must still be pending when the wrapper returns, so that the clones test the exit-side wait,
  call     call(fa, ctx, a) -> the outputs as a flat list of tensors and arrays.  `a` holds Inputs.host as it is, Inputs.addr as settled
           device tensors, the value tensors as device tensors, and a["keep"]: a list for what must outlive the call (plans, session
           objects: the test closes them after it has synchronised).

VALUE tensors hold numbers the kernels compute with (audio, logits, probabilities, weights, embeddings, token values); ADDRESSING
tensors hold what a kernel forms an address or a trip count from (offsets, ranges, counts, lengths, stream ids, window records).  Only
value tensors are produced late, and each has two versions: `fresh` and `stale` — same shape and dtype, both valid finite inputs of the
entry, with different results.  So whatever a mis-ordered kernel reads is in bounds and well formed: a missing order is a wrong answer,
never a fault.  The problems are the smallest valid ones of each entry; the numerics are pinned elsewhere."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

F, I = np.float32, np.int32


@dataclass
class Inputs:
    fresh: dict                                  # value tensors, as host arrays
    stale: dict                                  # the same names, shapes and dtypes
    addr: dict = field(default_factory=dict)     # addressing tensors the call takes on the device: uploaded and settled before the delay
    host: dict = field(default_factory=dict)     # everything that stays on the host


@dataclass
class Case:
    name: str
    entries: tuple
    build: object
    call: object
    control: bool = False                        # positive control: the wrapper's own order=False, the raced arm must give the stale result
    setup: object = None                         # setup(fa, ctx, a): what the call needs made BEFORE the delay starts because making it synchronises (a plan, a session)
    live: str = "first"                          # the producer is still pending when the call reaches Context.torch_ordered: "first" time, "all" times, or "none"
    drains: str = ""                             # for live == "none": the wrapper's own line that waits for torch's stream before the bridge
    exit_raced: bool = False                     # the wrapper returns device tensors without waiting: the producer must still be pending when it returns


# Entries of the wrapper modules no case reaches yet: {entry: reason}.  At most 8, none of pipeline.py, mel.py, ctc.py or tdt.py.
NOT_YET: dict = {
    "fa_aed_begin_dev": "takes no device tensor of the caller's: AedDecodeState uploads the host prompts itself (aed.py: A.to_device(packed, ...)), which waits for "
                        "torch's stream, so there is nothing to produce late; the sessions of aed-decode and aed-gather-hidden begin before the delay",
}


def _noise(rng, n, scale=0.1):
    return (rng.standard_normal(n) * scale).astype(F)


def _two(make):
    """fresh and stale from one generator and two seeds"""
    return make(np.random.default_rng(101)), make(np.random.default_rng(202))


# ---- pipeline.py --------------------------------------------------------------------------------------------------------------------
def _session(n_chunks, speakers, seed, d=256, dr=128):
    """test_gpu_pipeline.synth_session: three local speaker slots per chunk, unit speaker centres + noise, rho from VBx's model"""
    rng = np.random.default_rng(seed)
    n = 3 * n_chunks
    centers = rng.standard_normal((speakers, d))
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    spk = np.stack([rng.permutation(speakers)[:3] for _ in range(n_chunks)]).reshape(-1)
    emb = (centers[spk] + 0.03 * rng.standard_normal((n, d))).astype(F)
    phi = np.linspace(2.0, 1.0, dr)
    rho = rng.standard_normal((speakers, dr))[spk] * np.sqrt(phi) + rng.standard_normal((n, dr))
    return emb, np.ascontiguousarray(rho, np.float64), np.repeat(np.arange(n_chunks), 3).astype(I), phi


def _build_cluster(fa, rng):
    emb, rho, chunks, phi = _session(100, 4, 0)            # 300 rows
    emb2, rho2, _, _ = _session(100, 3, 1)                 # another recording of the same size with another speaker count
    return Inputs(dict(emb=emb, rho=rho), dict(emb=emb2, rho=rho2), host=dict(chunks=chunks, phi=phi))


def _cluster_outputs(res):
    return [np.asarray(res.assignments, I), np.ascontiguousarray(res.centroids)]


def _call_cluster(fa, ctx, a):
    return _cluster_outputs(fa.cluster_embeddings(a["emb"], a["rho"], a["chunks"], a["phi"], ctx=ctx))


def _call_cluster_ex(fa, ctx, a):
    res = fa.cluster_embeddings(a["emb"], a["rho"], a["chunks"], a["phi"], ctx=ctx, intermediates=True)
    return _cluster_outputs(res) + [np.asarray(res.initial_clusters, I), np.asarray(res.info["vbx_hard"], I), np.asarray(res.info["elbos"], np.float64)]


def _build_cluster_batch(fa, rng):
    e0, r0, c0, phi = _session(100, 4, 0)
    e1, r1, c1, _ = _session(60, 3, 2)
    s0, t0, _, _ = _session(100, 3, 1)
    s1, t1, _, _ = _session(60, 4, 3)
    return Inputs(dict(emb0=e0, rho0=r0, emb1=e1, rho1=r1), dict(emb0=s0, rho0=t0, emb1=s1, rho1=t1), host=dict(chunks0=c0, chunks1=c1, phi=phi))


def _call_cluster_batch(fa, ctx, a):
    st, out = fa.cluster_embeddings_batch([(a["emb0"], a["rho0"], a["chunks0"]), (a["emb1"], a["rho1"], a["chunks1"])], a["phi"], ctx=ctx)
    assert st == [0, 0], st
    return [x for res in out for x in _cluster_outputs(res)]


# ---- mel.py -------------------------------------------------------------------------------------------------------------------------
MEL_SAMPLES, MEL_BATCH = 4000, 2


def _build_mel(fa, rng):
    fresh, stale = _two(lambda r: _noise(r, MEL_BATCH * MEL_SAMPLES))
    return Inputs(dict(pcm=fresh), dict(pcm=stale), host=dict(offsets=np.arange(MEL_BATCH + 1, dtype=np.int64) * MEL_SAMPLES))


def _setup_mel(fa, ctx, a):
    import torch
    a["plan"] = fa.AudioMelSpectrogram(ctx=ctx).plan(a["offsets"])
    a["keep"].append(a["plan"])
    # the output is zeroed and settled here: a fill enqueued behind the delay would wipe what an unordered kernel wrote
    a["out"] = torch.zeros(a["plan"].out_shape(), dtype=torch.float32, device=a["pcm"].device)


def _call_mel(order):
    def call(fa, ctx, a):
        a["plan"].execute(a["pcm"], a["out"], order=order)
        return [a["out"]]
    return call


def _build_mel_features(fa, rng):
    fresh, stale = _two(lambda r: _noise(r, (2, 3200)))
    return Inputs(dict(windows=fresh), dict(windows=stale))


def _call_mel_features(fa, ctx, a):
    mel, valid = fa.UnifiedMelExtractor(3200, ctx=ctx).features_batch(a["windows"], [3200, 1600])
    return [mel, valid]


# ---- ctc.py -------------------------------------------------------------------------------------------------------------------------
def _build_ctc(fa, rng):
    fresh, stale = _two(lambda r: (2.0 * r.standard_normal((2, 20, 33))).astype(F))
    return Inputs(dict(logits=fresh), dict(logits=stale))


def _call_ctc_greedy(fa, ctx, a):
    import torch
    B, T, _ = a["logits"].shape
    tok, fids = (torch.zeros((B, T), dtype=torch.int32, device=a["logits"].device) for _ in range(2))
    lens = torch.zeros(B, dtype=torch.int32, device=a["logits"].device)
    fa.ctc_greedy_ids_dev(ctx, a["logits"], 32, tok, lens, fids)
    return [tok, lens, fids]


def _call_ctc_log_probs(order):
    def call(fa, ctx, a):
        return [fa.ctc_log_probs_dev(ctx, a["logits"], temperature=1.5, blank_bias=0.5, blank_id=32, order=order)]
    return call


# ---- tdt.py -------------------------------------------------------------------------------------------------------------------------
TDT_B, TDT_U, TDT_T, TDT_V1, TDT_ND = 2, 12, 20, 34, 5


def _walk_outputs(got):
    out = []
    for g in got:
        out += [np.array([g["status"], g["count"], g["final_u"], -1 if g["final_time"] is None else g["final_time"]], np.int64),
                g["tokens"], g["timestamps"], g["durations"], g["confidences"]] + ([g["routes"], np.array(g["swap_counts"], I)] if "routes" in g else [])
    return out


def _tdt_vectors():
    """the walk's per-chunk vectors, settled on the device: handed in as host lists the wrapper would upload them on torch's stream and wait"""
    return dict(enc=np.array([TDT_T, TDT_T - 3], I), t0=np.array([0, 2], I), last=np.array([1, 0], I))


def _build_tdt_tables(fa, rng):
    def make(r):
        tok = r.integers(0, 50, (TDT_B, TDT_U, TDT_T)).astype(I)
        tok[r.random(tok.shape) < 0.7] = 8192
        return dict(tok=tok, bin=r.integers(0, 5, tok.shape).astype(I), prob=r.uniform(0.0, 1.0, tok.shape).astype(F))
    fresh, stale = _two(make)
    return Inputs(fresh, stale, addr=_tdt_vectors())


def _call_tdt_tables(fa, ctx, a):
    return _walk_outputs(fa.tdt_decode_tables(a["tok"], a["bin"], a["prob"], a["enc"], None, a["t0"], a["last"], None, None, max_out=64, ctx=ctx))


def _build_tdt_logits(fa, rng):
    def make(r):
        lg = r.standard_normal((TDT_B, TDT_U, TDT_T, TDT_V1 + TDT_ND)).astype(F)
        lg[..., TDT_V1 - 1] += 3.2
        return dict(logits=lg)
    fresh, stale = _two(make)
    texts = [("a%d" % i if i % 2 == 0 else "б%d" % i) for i in range(TDT_V1 - 1)] + [None]        # Latin and Cyrillic pieces, the blank has none
    return Inputs(fresh, stale, addr=dict(_tdt_vectors(), classes=fa.tdt_token_classes(texts)))


def _call_tdt_logits(fa, ctx, a):
    cfg = fa.TdtConfig(blank_id=TDT_V1 - 1)
    return _walk_outputs(fa.tdt_decode_logits(a["logits"], TDT_V1, a["enc"], None, a["t0"], a["last"], None, None, config=cfg, max_out=64, ctx=ctx))


def _call_tdt_lang(fa, ctx, a):
    cfg = fa.TdtConfig(blank_id=TDT_V1 - 1)
    return _walk_outputs(fa.tdt_decode_logits_lang(a["logits"], TDT_V1, a["classes"], fa.Script.LATIN, a["enc"], None, a["t0"], a["last"], None, None, top_k=8,
                                                   config=cfg, max_out=64, ctx=ctx))


def _build_topk(fa, rng):
    fresh, stale = _two(lambda r: r.standard_normal((7, 40)).astype(F))
    return Inputs(dict(rows=fresh), dict(rows=stale))


def _call_topk(fa, ctx, a):
    return list(fa.tdt_topk_rows(a["rows"], 37, 5, ctx=ctx))


# ---- tdt_plan.py --------------------------------------------------------------------------------------------------------------------
TDT_PLAN_LENGTHS = (20000, 30001)


def _plan_audio(r, quiet_tail):
    parts = []
    for n in TDT_PLAN_LENGTHS:
        x = _noise(r, n, 0.05)
        if quiet_tail:
            x[n - 9000:] = 0        # another speech end, another threshold
        parts.append(x)
    return np.concatenate(parts)


def _build_tdt_plan(fa, rng):
    fresh, stale = _plan_audio(np.random.default_rng(1), False), _plan_audio(np.random.default_rng(2), True)
    offsets = np.concatenate([[0], np.cumsum(TDT_PLAN_LENGTHS)]).astype(np.int64)
    spans = np.array([(0, 0, 0, 16000), (1, 0, 1000, 30001)], fa.TDT_SPAN_DTYPE)
    return Inputs(dict(audio=fresh), dict(audio=stale), host=dict(offsets=offsets, spans=spans, fresh_audio=fresh))


def _setup_tdt_pack(fa, ctx, a):
    a["windows"] = fa.tdt_plan_windows(a["fresh_audio"], a["offsets"], ctx=ctx).windows          # the same lengths: the windows address both versions alike


def _call_tdt_plan(fa, ctx, a):
    p = fa.tdt_plan_windows_dev(a["audio"], a["offsets"], ctx=ctx)
    return [p.windows, p.window_range, p.speech_end, p.statuses, p.audio_frames, p.t0, p.is_last, p.global_offset, p.emit_after]


def _call_tdt_pack(fa, ctx, a):
    return list(fa.tdt_pack_windows_dev(a["audio"], a["offsets"], a["windows"], ctx=ctx))


def _call_tdt_gate(fa, ctx, a):
    return list(fa.tdt_speech_gate_dev(a["audio"], a["offsets"], a["spans"], ctx=ctx))


# ---- tdt_merge.py -------------------------------------------------------------------------------------------------------------------
def _build_tdt_merge(fa, rng):
    import tdt_merge_cases as K
    batch = K.edge_batch()
    p = K.pack(batch)
    held = p.tok >= 0                                                   # the cells behind a window's tokens keep their filler
    stale_tok = np.where(held, p.tok % 8 + 1, p.tok).astype(I)          # other ids of the same vocabulary
    stale_conf = np.where(held, p.conf * F(0.5), p.conf).astype(F)
    return Inputs(dict(tok=p.tok, conf=p.conf), dict(tok=stale_tok, conf=stale_conf), addr=dict(time=p.time, dur=p.dur, counts=p.counts),
                  host=dict(window_range=p.window_range, caps=p.caps, safe=p.safe, canon=p.canon, vocab=batch.vocab, overlap=batch.overlap))


def _call_tdt_merge(fa, ctx, a):
    m = fa.merge_windows_dev(a["tok"], a["time"], a["dur"], a["conf"], a["counts"], a["window_range"], splice_safe=a["safe"], case_canon=a["canon"], vocab=a["vocab"],
                             overlap_seconds=a["overlap"], capacities=a["caps"], ctx=ctx)
    return [m.tokens, m.timestamps, m.durations, m.confidences, m.out_range, m.counts, m.statuses, m.routes]


# ---- rnnt.py ------------------------------------------------------------------------------------------------------------------------
def _build_rnnt(fa, rng):
    def make(r):
        lg = r.standard_normal((2, 10, 16, 21)).astype(F)
        lg[..., 20] += 2.0
        return dict(logits=lg)
    fresh, stale = _two(make)
    return Inputs(fresh, stale, addr=dict(frames=np.array([16, 11], I)))


def _call_rnnt(fa, ctx, a):
    got = fa.rnnt_decode_logits(a["logits"], 21, a["frames"], config=fa.RnntConfig(blank_id=20), max_out=64, ctx=ctx)
    return [x for g in got for x in (np.array([g["status"], g["count"], g["final_u"], int(g["eou"])], I), g["tokens"], g["frames"], g["flips"])]


# ---- rnnt_stream.py: one session over the smallest scripted scenario ------------------------------------------------------------------
def _build_rnnt_stream(fa, rng):
    import rnnt_stream_cases as K
    sc = K.SCENARIOS["w320"]
    exp = K.expected(sc)
    steps = len(sc.steps)
    fresh = {f"chunk{t}": sc.chunk(t) for t in range(steps)}
    fresh.update({f"mel{t}": sc.mel(t) for t in range(steps)})
    other = K.Scenario(sc.name, sc.cfg, sc.steps, streams=sc.streams, seed=sc.seed + 50)          # the same loud / silent windows, other samples
    stale = {f"chunk{t}": other.chunk(t)[::-1].copy() for t in range(steps)}                      # and the streams swapped
    stale.update({f"mel{t}": other.mel(t) for t in range(steps)})
    rc = sc.request_capacity

    def staged(requests):                                                # what the rescue decode would hand back for the fresh session's requests
        ids, frames, nid, nfr = np.zeros((rc, sc.staged_capacity), I), np.zeros((rc, sc.staged_capacity), I), np.zeros(rc, I), np.zeros(rc, I)
        for r, q in enumerate(requests[:rc]):
            x, y = K.stub_decoder(q)
            ids[r, :len(x)], frames[r, :len(y)], nid[r], nfr[r] = x, y, len(x), len(y)
        return ids, frames, nid, nfr

    addr = dict(cls=K.class_table(), finalize=np.array(list(sc.finalize), I), n_finalize=np.array([len(sc.finalize)], I))
    for t in range(steps):
        addr[f"sid{t}"], addr[f"sfr{t}"], addr[f"nid{t}"], addr[f"nfr{t}"] = staged(exp.requests[t])
    addr["sidF"], addr["sfrF"], addr["nidF"], addr["nfrF"] = staged(exp.final_requests)
    return Inputs(fresh, stale, addr=addr, host=dict(steps=steps))


def _setup_rnnt_stream(fa, ctx, a):
    import rnnt_stream_cases as K
    sc = K.SCENARIOS["w320"]
    a["state"] = fa.RnntStreamState(sc.streams, fa.RnntStreamConfig(**vars(sc.cfg)), ctx)
    a["keep"].append(a["state"])


def _call_rnnt_stream(fa, ctx, a):
    """gate -> mel_inputs -> advance -> track -> merge_rescued per step, then finalize -> merge_rescued; nothing is waited for in between.  Every
    output buffer is handed in zeroed, so that rows an entry does not write compare equal."""
    import torch
    import rnnt_stream_cases as K
    sc = K.SCENARIOS["w320"]
    B, dev, st = sc.streams, a["cls"].device, a["state"]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    live = [z((B, sc.token_capacity), torch.int32) for _ in range(3)] + [z((B,), torch.int32) for _ in range(2)]       # ids, frames, timed ids, id count, timed count
    out = []

    def tracked(slots):
        return fa.RnntStreamTracked(z((sc.request_capacity, fa.rnnt_stream.RNNT_STREAM_REQUEST_DTYPE.itemsize), torch.uint8), z((sc.arena_capacity,), torch.float32),
                                    z((1,), torch.int32), z((slots,), torch.int32))

    for t in range(a["steps"]):
        chunk, mel = a[f"chunk{t}"], a[f"mel{t}"]
        gate = st.gate_dev(chunk, None, out=(z((B,), torch.float32), z((B,), torch.int32), z((B,), torch.int32), z((1,), torch.int32), z((B,), torch.int32)))
        rows = st.mel_inputs_dev(mel, gate[2], gate[3], out=(z((B, sc.cfg.mel_features, sc.cfg.total_mel_frames), torch.float32), z((B,), torch.int32)))
        st.advance_dev(gate[2], gate[3], frames=sc.enc_frames)
        tr = st.track_dev(chunk, live[1], live[2], live[4], a["cls"], sc.rescue_chunk_samples, sc.request_capacity, sc.arena_capacity, out=tracked(B))
        status = st.merge_rescued_dev(tr, a[f"sid{t}"], a[f"sfr{t}"], a[f"nid{t}"], a[f"nfr{t}"], *live, a["cls"], out=z((sc.request_capacity,), torch.int32))
        out += list(gate) + list(rows) + [tr.requests, tr.arena, tr.request_count, tr.status, status]
    tr = st.finalize_dev(a["finalize"], a["n_finalize"], live[1], live[2], live[4], a["cls"], sc.rescue_chunk_samples, sc.request_capacity, sc.arena_capacity,
                         out=tracked(len(sc.finalize)))
    status = st.merge_rescued_dev(tr, a["sidF"], a["sfrF"], a["nidF"], a["nfrF"], *live, a["cls"], out=z((sc.request_capacity,), torch.int32))
    return out + [tr.requests, tr.arena, tr.request_count, tr.status, status] + live


# ---- aed.py -------------------------------------------------------------------------------------------------------------------------
AED_KEYS = ("mode", "vocab", "eos_id", "max_seq", "max_new", "no_repeat_ngram", "repetition_penalty")


def _aed_case():
    import aed_cases as K
    cfg = K.token_cfg(12, 16, 4, 2, 1.1)
    return K.build("n2", cfg, [([6, 7], [K.eos_row, K.emit(1), K.emit(0), K.emit(1), K.emit(2), K.ban_flip]), ([5], [K.emit(0), K.emit(1), K.pos_flip, K.neg_flip, K.emit(2)])],
                   seed=2)


def _build_aed_decode(fa, rng):
    case = _aed_case()
    rows = np.ascontiguousarray(case["rows"], F)                        # [steps, B, V]
    # the rows with their vocabulary mirrored: finite logits of the same shape that decide otherwise
    return Inputs(dict(rows=rows), dict(rows=np.ascontiguousarray(rows[..., ::-1])), host=dict(prompts=case["prompts"], cfg={k: case["cfg"][k] for k in AED_KEYS}))


def _setup_aed_decode(fa, ctx, a):
    a["state"] = fa.AedDecodeState(a["prompts"], fa.AedConfig(**a["cfg"]), self_mask="float32", ctx=ctx)       # begin: it uploads the prompts and waits


def _call_aed_decode(fa, ctx, a):
    st = a["state"]
    for s in range(a["rows"].shape[0]):
        st.step(a["rows"][s])
    return list(st.finish_dev()) + [st.input_id, st.position_id, st.self_mask]


def _build_aed_hidden(fa, rng):
    import aed_cases as K
    fresh, stale = _two(lambda r: r.standard_normal((4, 12, 24)).astype(F))
    return Inputs(dict(dec=fresh), dict(dec=stale), host=dict(prompts=[[7, 7, 4], [1], [2] * 12, [5] * 11], cfg={k: K.seq_cfg(12, 12)[k] for k in AED_KEYS}))


def _setup_aed_hidden(fa, ctx, a):
    a["state"] = fa.AedDecodeState(a["prompts"], fa.AedConfig(**a["cfg"]), ctx=ctx)     # the sequence feed: positions 3, 1, 12 (capped) and 11


def _call_aed_hidden(fa, ctx, a):
    return [a["state"].gather_hidden(a["dec"])]


def _build_aed_mask(fa, rng):
    # the mask's only input: every int32 is a valid count (it is clamped), so both versions are in bounds
    return Inputs(dict(valid=np.array([0, 1, 17, 64, 65, 9999, -5], I)), dict(valid=np.array([3, 0, 65, 1, 64, -5, 30], I)))


def _call_aed_mask(fa, ctx, a):
    return [fa.aed_cross_attention_mask(a["valid"], 65, "float32", ctx=ctx)]


def _build_aed_context(fa, rng):
    fresh, stale = _two(lambda r: r.standard_normal((3, 20, 13)).astype(F))
    return Inputs(dict(enc=fresh), dict(enc=stale), addr=dict(lengths=np.array([0, 7, 18], I)))


def _call_aed_context(fa, ctx, a):
    return list(fa.aed_encoder_context(a["enc"], a["lengths"], ctx=ctx))


def _build_aed_merge(fa, rng):
    def make(r):
        base = r.integers(4, 30, 40)
        w0, w1, w2 = base[:20], np.concatenate([base[12:20], r.integers(4, 30, 10)]), r.integers(4, 30, 9)
        return np.concatenate([w0, w1, w2, base[:7], base[2:12]]).astype(I)
    fresh, stale = _two(make)
    return Inputs(dict(tokens=fresh), dict(tokens=stale), host=dict(offsets=np.array([0, 20, 38, 47, 54, 64], np.int64), recordings=np.array([0, 3, 5], np.int64)))


def _call_aed_merge(fa, ctx, a):
    m = fa.aed_merge_token_windows_dev(a["tokens"], a["offsets"], a["recordings"], window_tokens=8, min_match=3, ctx=ctx)
    return [m.tokens, m.out_range, m.counts, m.best_len, m.best_s_end]


# ---- kws.py, vocab_rescore.py: log-probabilities on the device -------------------------------------------------------------------------
KWS_TERMS = [[3], [5, 9], [1, 2, 3, 4], [7, -1, 8], [2, 2], list(range(10, 16))]


def _log_probs(r, B, T, V, blank):
    x = (2.0 * r.standard_normal((B, T, V))).astype(np.float64)
    x[:, :, blank] += 2.0
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(F)


def _build_kws(fa, rng):
    fresh, stale = _two(lambda r: _log_probs(r, 2, 30, 37, 36))
    return Inputs(dict(lp=fresh), dict(lp=stale))


def _call_kws_spot(fa, ctx, a):
    # a threshold nothing falls below: both versions have detections to differ in
    return list(fa.spot_keywords_batch(a["lp"], KWS_TERMS, min_score=-1000.0, blank_id=36, valid_frames=[30, 21], ctx=ctx))


def _call_kws_windows(fa, ctx, a):
    return [fa.score_windows(a["lp"], KWS_TERMS, [(0, 1, 2, 20), (1, 2, 0, 21), (1, 3, 15, 40), (0, 5, 20, 30)], blank_id=36, valid_frames=[30, 21], ctx=ctx)]


def _build_vocab_rescore(fa, rng):
    import vocab_rescore_cases as K
    p = K.verdict_problem()
    lp = p["lp"]
    stale = (F(-0.5) * np.random.default_rng(6).integers(0, 8, lp.shape).astype(F)).astype(F)       # the problem's own grid, other draws
    cands = np.zeros(len(p["cands"]), fa.vocab_rescore.VR_CANDIDATE_DTYPE)
    for i, c in enumerate(p["cands"]):
        cands[i] = tuple(c)
    return Inputs(dict(lp=lp), dict(lp=stale), host=dict(p=p, cands=cands))


def _call_vocab_rescore(fa, ctx, a):
    V, p = fa.vocab_rescore, a["p"]
    cfg = V.default_config()
    cfg.frame_duration, cfg.margin_seconds, cfg.cbw, cfg.blank_id = p["frame_duration"], p["margin"], float(p["cbw"]), p["blank"]
    flat = lambda rows: [x for r in rows for x in r]   # noqa: E731
    verdicts, applied = V.decide(a["lp"], a["cands"], [len(s) for s in p["starts"]], flat(p["starts"]), flat(p["ends"]), p["term_tokens"], p["alt_tokens"], p["phrase_tokens"],
                                 config=cfg, occupied=flat(p["occupied"]), valid_frames=p["valid"], ctx=ctx)
    return [verdicts] + [np.asarray(x, I) for x in applied]


# ---- wer.py -------------------------------------------------------------------------------------------------------------------------
def _build_wer(fa, rng):
    fresh, stale = _two(lambda r: dict(hyp=r.integers(0, 6, 40).astype(I), ref=r.integers(0, 6, 45).astype(I)))
    return Inputs(fresh, stale, host=dict(hyp_range=np.array([0, 0, 7, 25, 40], np.int64), ref_range=np.array([0, 5, 11, 30, 45], np.int64)))


def _call_wer(fa, ctx, a):
    return [fa.edit_distance_batch_dev(a["hyp"], a["hyp_range"], a["ref"], a["ref_range"], ctx=ctx)]


# ---- paraformer.py ------------------------------------------------------------------------------------------------------------------
def _paraformer_cfg(fa):
    cfg = fa.paraformer.default_config()
    cfg.max_tokens, cfg.enc_frames = 24, 70
    return cfg


def _build_cif(fa, rng):
    fresh, stale = _two(lambda r: dict(enc=r.standard_normal((2, 66, 16)).astype(F), alphas=r.uniform(0.0, 0.45, (2, 66)).astype(F)))
    return Inputs(fresh, stale, host=dict(valid=[66, 23]))


def _call_cif(fa, ctx, a):
    c = fa.cif_batch_dev(a["enc"], a["alphas"], a["valid"], config=_paraformer_cfg(fa), pack_enc=True, ctx=ctx)
    return [c.ac, c.token_counts, c.fire_counts, c.fire_frames, c.enc_packed]


STAMP_IDS = ([1, 3, 4, 0, 5, 6, 7, 8, 9, 10, 40, 11, 3, 4, 0, 5, 6, 2], [1, 3, 4, 0, 5, 6, 8, 2, 40, 4, 4, 4, 4, 4])      # test_gpu_paraformer's IDS_12 and IDS_9


def _gated_tone(r, shift):
    """test_gpu_paraformer.gated_tone: 4 s of a 220 Hz tone gated at 5 Hz, solid for 0.9 s, over faint noise"""
    t = np.arange(4 * 16000) / 16000.0 + shift
    gate = ((np.floor(t * 10) % 2) == 0) | ((t >= 2.0) & (t < 2.9))
    return (0.3 * np.sin(2 * np.pi * 220 * t) * gate + 0.001 * r.standard_normal(t.size)).astype(F)


def _build_stamps(fa, rng):
    def make(r, shift, order):
        ids = np.full((2, 24), 3, I)
        for k, u in enumerate(order):
            ids[k, :len(STAMP_IDS[u])] = STAMP_IDS[u]
        return dict(alphas=r.uniform(0.0, 0.45, (2, 66)).astype(F), ids=ids, audio=np.concatenate([_gated_tone(r, shift), _gated_tone(r, shift)]))
    fresh, stale = make(np.random.default_rng(189), 0.0, (0, 1)), make(np.random.default_rng(190), 0.33, (1, 0))
    keep = np.zeros(12, np.uint8)
    keep[[3, 4, 5, 6, 7, 9, 10, 11]] = 1
    return Inputs(fresh, stale, host=dict(valid=[66, 60], counts=np.array([14, 14], I), keep_table=keep, audio_offsets=np.array([0, 64000, 128000], np.int64)))


def _call_stamps(fa, ctx, a):
    return list(fa.timestamps_batch_dev(a["alphas"], a["valid"], a["ids"], a["counts"], a["keep_table"], a["audio"], a["audio_offsets"], config=_paraformer_cfg(fa), ctx=ctx))


# ---- vad.py -------------------------------------------------------------------------------------------------------------------------
VAD_LENGTHS = (9000, 20001)


def _build_vad_probs(fa, rng):
    def make(r):
        return np.repeat(r.random(12) < 0.5, 10).astype(F) * F(0.9) + r.uniform(0.0, 0.05, 120).astype(F)     # runs of ten chunks either side of the threshold
    fresh, stale = _two(make)
    return Inputs(dict(probs=fresh), dict(probs=stale), host=dict(frame_range=np.array([0, 50, 120], np.int64), total=np.array([50 * 4096, 70 * 4096 - 100], np.int64)))


def _call_vad_segments(fa, ctx, a):
    return list(fa.segment_speech_batch_dev(a["probs"], a["frame_range"], a["total"], ctx=ctx))


def _build_vad_audio(fa, rng):
    fresh, stale = _two(lambda r: _noise(r, sum(VAD_LENGTHS)))
    offsets = np.concatenate([[0], np.cumsum(VAD_LENGTHS)]).astype(np.int64)
    segs = np.zeros(3, fa.VAD_SEGMENT_DTYPE)
    for i, (rec, t0, t1) in enumerate(((0, 0.1, 0.4), (1, 0.0, 0.25), (1, 0.9, 1.3))):     # 16 kHz: every span ends inside its recording or is clamped to it
        segs[i]["recording"], segs[i]["start_time"], segs[i]["end_time"] = rec, t0, t1
        segs[i]["start_sample"], segs[i]["end_sample"] = int(t0 * 16000), int(t1 * 16000)
    return Inputs(dict(audio=fresh), dict(audio=stale), host=dict(offsets=offsets, segs=segs))


def _call_vad_pack(fa, ctx, a):
    return list(fa.pack_chunks_dev(a["audio"], a["offsets"], ctx=ctx))


def _call_vad_gather(fa, ctx, a):
    return list(fa.gather_segments_dev(a["audio"], a["offsets"], a["segs"], ctx=ctx))


def _build_vad_stream(fa, rng):
    def make(r):
        return np.ascontiguousarray((np.repeat(r.random((3, 4)) < 0.5, 6, axis=1).astype(F) * F(0.9) + r.uniform(0.0, 0.05, (3, 24)).astype(F)))
    fresh, stale = _two(make)
    return Inputs(dict(probs=fresh), dict(probs=stale))


def _call_vad_stream(fa, ctx, a):
    states = fa.initial_stream_states(3)                                # a fresh session: the entry updates the records in place
    events = fa.stream_advance_dev(a["probs"], states, ctx=ctx)
    return [events, states]


# ---- fsmn_vad.py --------------------------------------------------------------------------------------------------------------------
FSMN_LENGTHS = (8000, 12345)


def _build_fsmn(fa, rng):
    chunks, chunk_range, frame_range = fa.fsmn_vad_plan_chunks(np.array(FSMN_LENGTHS, np.int64))
    frames = int(chunks["frames"].max())

    def make(r):
        import fsmn_vad_cases as K
        return dict(audio=_noise(r, sum(FSMN_LENGTHS)), feats=r.standard_normal((chunks.size, frames + 3, 400)).astype(F),
                    scores=r.uniform(0.0, 1.0, (chunks.size, frames + 3, 3)).astype(F), probs=np.concatenate([K.blocks(r, 200), K.noise(r, 130)]))
    fresh, stale = _two(make)
    return Inputs(fresh, stale, host=dict(offsets=np.concatenate([[0], np.cumsum(FSMN_LENGTHS)]).astype(np.int64), chunks=chunks, frame_range=frame_range, bucket=frames + 3,
                                          probs_range=np.array([0, 200, 330], np.int64)))


def _call_fsmn_waveforms(fa, ctx, a):
    return [fa.fsmn_vad_pack_waveforms_dev(a["audio"], a["offsets"], a["chunks"], ctx=ctx)]


def _call_fsmn_feats(fa, ctx, a):
    return [fa.fsmn_vad_pack_feats_dev(a["feats"], a["chunks"], a["bucket"], ctx=ctx)]


def _call_fsmn_silence(fa, ctx, a):
    return [fa.fsmn_vad_gather_silence_dev(a["scores"], a["chunks"], a["frame_range"], ctx=ctx)]


def _call_fsmn_segments(fa, ctx, a):
    return list(fa.fsmn_vad_segments_dev(a["probs"], a["probs_range"], ctx=ctx))


# ---- sortformer.py, timeline.py -----------------------------------------------------------------------------------------------------
SORTFORMER_LENGTHS = (207, 41, 20)


def _sortformer_cfg(fa):
    return fa.OfflineSortformerConfig(window_output_frames=10, subsampling_factor=2, num_speakers=4, mel_features=8, overlap_output_frames=5)


def _build_sortformer_pack(fa, rng):
    fresh, stale = _two(lambda r: r.standard_normal((3, 8, 210)).astype(F))
    return Inputs(dict(mel=fresh), dict(mel=stale))


def _call_sortformer_pack(fa, ctx, a):
    return list(fa.pack_windows(a["mel"], SORTFORMER_LENGTHS, "mel_major", _sortformer_cfg(fa), ctx))


def _build_sortformer_stitch(fa, rng):
    w = int(fa.offline_windows(SORTFORMER_LENGTHS, _sortformer_cfg(fa))["window_range"][-1])
    fresh, stale = _two(lambda r: r.random((w, 10, 4)).astype(F))
    return Inputs(dict(preds=fresh), dict(preds=stale))


def _call_sortformer_stitch(fa, ctx, a):
    return list(fa.stitch(a["preds"], SORTFORMER_LENGTHS, _sortformer_cfg(fa), ctx))


def _build_timeline(fa, rng):
    def make(r):
        return np.ascontiguousarray(np.repeat(r.random((30, 4)) < 0.4, 5, axis=0).astype(F) * F(0.8) + r.uniform(0.0, 0.1, (150, 4)).astype(F))
    fresh, stale = _two(make)
    return Inputs(dict(fin=fresh[:110], tent=fresh[110:]), dict(fin=stale[:110], tent=stale[110:]), host=dict(fin_frames=[70, 40], tent_frames=[15, 25]))


def _call_timeline(fa, ctx, a):
    return list(fa.timeline_segments(a["fin"], a["fin_frames"], a["tent"], a["tent_frames"], fa.DiarizerTimelineConfig.sortformer_default(), False, ctx))


# ---- sortformer_stream.py -----------------------------------------------------------------------------------------------------------
SF_STREAM_KEYS = ("speakers", "d_model", "chunk_len", "chunk_left_context", "chunk_right_context", "fifo_len", "spkcache_len", "spkcache_update_period", "sil_frames_per_spk",
                  "max_index", "max_chunk_frames", "subsampling", "n_mels", "silence_threshold", "pred_score_threshold", "scores_boost_latest", "strong_boost_rate",
                  "weak_boost_rate", "min_pos_scores_rate")
SF_STEPS = 12      # the small geometry pops its FIFO and compresses its speaker cache within these


def _build_sf_update(fa, rng):
    import sortformer_stream_cases as K
    cfg, steps = K.operands(K.Case("small", 1, "uniform"))
    _, others = K.operands(K.Case("small", 9, "uniform"))               # the operands depend on the lengths alone: another seed has the same counts
    steps, others = steps[:SF_STEPS], others[:SF_STEPS]
    fresh, stale, addr = {}, {}, {}
    for t, (s, o) in enumerate(zip(steps, others)):
        assert all(np.array_equal(getattr(s, k), getattr(o, k)) for k in ("emb_len", "pred_rows", "left", "right", "active"))
        fresh[f"chunk{t}"], stale[f"chunk{t}"] = s.chunk, o.chunk
        fresh[f"preds{t}"], stale[f"preds{t}"] = np.nan_to_num(s.preds, nan=0.5), np.nan_to_num(o.preds, nan=0.5)          # an injected NaN stays out: finite inputs only
        for k in ("emb_len", "pred_rows", "left", "right", "active"):
            addr[f"{k}{t}"] = getattr(s, k)
    return Inputs(fresh, stale, addr=addr, host=dict(cfg={f: getattr(cfg, f) for f in SF_STREAM_KEYS}, streams=5))


def _setup_sf_update(fa, ctx, a):
    a["state"] = fa.SortformerStreamState(a["streams"], fa.SortformerStreamConfig(**a["cfg"]), ctx)
    a["keep"].append(a["state"])


def _call_sf_update(fa, ctx, a):
    st, out = a["state"], []
    for t in range(SF_STEPS):
        u = st.update_dev(a[f"chunk{t}"], a[f"emb_len{t}"], a[f"preds{t}"], a[f"pred_rows{t}"], a[f"left{t}"], a[f"right{t}"], a[f"active{t}"], log_scores=True)
        out += [u.confirmed, u.tentative, u.counts, u.status, u.log_scores]
    return out


def _sf_pack_cfg(fa):
    return fa.SortformerStreamConfig(speakers=4, d_model=24, chunk_len=3, chunk_left_context=1, chunk_right_context=2, fifo_len=5, spkcache_len=32, spkcache_update_period=4,
                                     subsampling=2, n_mels=6)


def _build_sf_pack(fa, rng):
    fresh, stale = _two(lambda r: r.standard_normal(3 * 40 * 6).astype(F))
    chunks = fa.sortformer_stream_chunk_plan([40, 25, 3], [0, 4, 0], _sf_pack_cfg(fa))
    return Inputs(dict(mel=fresh), dict(mel=stale), host=dict(offsets=np.array([0, 40, 80], np.int64), chunks=chunks))


def _call_sf_pack(fa, ctx, a):
    return [fa.sortformer_stream_pack_chunks(a["mel"], a["offsets"], a["chunks"], _sf_pack_cfg(fa), ctx)]


# ---- online.py ----------------------------------------------------------------------------------------------------------------------
ONLINE_FRAMES = 65
ONLINE_CFG = dict(frames=ONLINE_FRAMES, chunk_samples=160000, min_active_frames=10.0, min_speech_duration=float(F(16.0 * 0.016875)))


def _online_weights(r, B=2, chunks=2):
    w = np.zeros((B, chunks, ONLINE_FRAMES, 3), F)
    for b in range(B):
        for c in range(chunks):
            for s in range(3):
                f = int(r.integers(0, 12))
                while f < ONLINE_FRAMES:
                    n = int((15, 16, 17, 40)[r.integers(4)])
                    w[b, c, f:f + n, s] = 1.0
                    f += n + int((3, 16, 30)[r.integers(3)])
    return w


def _unit(r):
    v = r.standard_normal(256).astype(F)
    return v / F(np.sqrt(np.sum(v.astype(np.float64) ** 2)))


def _build_online_plan(fa, rng):
    fresh, stale = _two(_online_weights)
    return Inputs(dict(weights=fresh), dict(weights=stale))


def _call_online_plan(fa, ctx, a):
    act, runs, rows = fa.online_chunk_plan(a["weights"], None, config=fa.OnlineChunkConfig(**ONLINE_CFG), ctx=ctx)
    return [act, runs, rows]


def _build_online_pack(fa, rng):
    lengths = np.array([0, 1, 5, 333, 999, 1000, 1003], I)
    offsets = np.concatenate([[3], 3 + np.cumsum(lengths[:-1] + 1)]).astype(np.int64)
    n = int(offsets[-1] + lengths[-1] + 5)
    fresh, stale = _two(lambda r: _noise(r, n))
    return Inputs(dict(audio=fresh), dict(audio=stale), host=dict(offsets=offsets, lengths=lengths))


def _call_online_pack(fa, ctx, a):
    return [fa.online_pack_waveforms(a["audio"], a["offsets"], a["lengths"], 1000, fa.ONLINE_PACK_REPEAT, ctx=ctx)]


def _build_online_finish(fa, rng):
    def make(r):
        voices = [_unit(r) for _ in range(4)]
        w = _online_weights(r)
        emb = np.stack([F(3.0) * (voices[r.integers(4)] + F(0.2) * _unit(r)) for _ in range(2 * 2 * 3)]).reshape(2, 2, 3, 256).astype(F)
        act = np.ascontiguousarray(w.sum(axis=2), F)                    # the gate's input; any finite activity is valid
        return dict(weights=w, activities=act, embeddings=emb)
    fresh, stale = _two(make)
    return Inputs(fresh, stale, host=dict(offsets=np.array([[0.0, 10.0], [0.0, 10.37]])))


def _setup_online_finish(fa, ctx, a):
    a["db"] = fa.SpeakerDatabase(2, fa.SpeakerDbConfig(max_speakers=4, raw_capacity=3, min_speech_duration=0.1), ctx=ctx)
    a["keep"].append(a["db"])


def _call_online_finish(fa, ctx, a):
    return list(fa.online_chunk_finish(a["db"], a["weights"], a["activities"], a["embeddings"], a["offsets"], config=fa.OnlineChunkConfig(**ONLINE_CFG), tick=7))


def _build_speaker_db(fa, rng):
    def make(r):
        voices = [_unit(r) for _ in range(3)]
        emb = np.stack([F(2.0) * (voices[r.integers(3)] + F(0.15) * _unit(r)) for _ in range(2 * 5)]).reshape(2, 5, 256).astype(F)
        return dict(embeddings=emb, durations=r.uniform(0.5, 3.0, (2, 5)).astype(F))
    fresh, stale = _two(make)
    return Inputs(fresh, stale)


def _setup_speaker_db(fa, ctx, a):
    a["db"] = fa.SpeakerDatabase(2, fa.SpeakerDbConfig(max_speakers=4, raw_capacity=3), ctx=ctx)
    a["keep"].append(a["db"])
    if "seed_embeddings" in a:                                          # the distances case: speakers from settled embeddings
        a["db"].assign_dev(a["seed_embeddings"], a["seed_durations"], None, tick=3)


def _call_speaker_db(fa, ctx, a):
    """assign, then the pairs of what it left in the tables: both reach the bridge while the embeddings are still pending"""
    records = a["db"].assign_dev(a["embeddings"], a["durations"], None, tick=3)
    pairs = a["db"].mergeable_pairs(speaker_threshold=1.5)
    return [records] + pairs


def _build_speaker_distances(fa, rng):
    seed = _build_speaker_db(fa, rng).fresh
    fresh, stale = _two(lambda r: np.stack([_unit(r) for _ in range(4)]).reshape(2, 2, 256))
    return Inputs(dict(queries=fresh), dict(queries=stale), addr=dict(seed_embeddings=seed["embeddings"], seed_durations=seed["durations"]))


def _call_speaker_distances(fa, ctx, a):
    return list(a["db"].distances(a["queries"]))


# ---- embedding.py, reconstruct.py ---------------------------------------------------------------------------------------------------
EMB_CHUNKS, EMB_FRAMES, EMB_TOTAL = 4, 589, 16000 * 33 + 77


def _hard_weights(r, chunks=EMB_CHUNKS, frames=EMB_FRAMES):
    """0 / 1 weights with at most one speaker per frame (nothing for the overlap exclusion to drop), in blocks of 60 ... 150 frames"""
    w = np.zeros((chunks, frames, 3), F)
    for c in range(chunks):
        f = 0
        while f < frames:
            n, s = int(r.integers(60, 150)), int(r.integers(-1, 3))
            if s >= 0:
                w[c, f:f + n, s] = 1.0
            f += n
    return w


def _build_embedding_plan(fa, rng):
    fresh, stale = _two(_hard_weights)
    return Inputs(dict(weights=fresh), dict(weights=stale), host=dict(offsets=np.arange(EMB_CHUNKS) * 10.0))


def _call_embedding_plan(fa, ctx, a):
    p = fa.plan_embeddings(fa.SegmentationOutput(a["weights"], a["offsets"], 10.0 / EMB_FRAMES), EMB_TOTAL, fa.EmbeddingConfig(batch_size=3), mask_rows=True, ctx=ctx)
    return [p.records, p.run_of_job, p.window_of_run, p.window_start, p.window_chunk, p.run_weights, p.mask_rows]


def _build_embedding_audio(fa, rng):
    fresh, stale = _two(lambda r: _noise(r, EMB_TOTAL))
    return Inputs(dict(audio=fresh), dict(audio=stale), host=dict(spans=[(1.0, 3.5), (30.0, 45.0), (0.00003125, 0.5), (-1.0, 0.25)]))


def _setup_embedding_windows(fa, ctx, a):
    a["plan"] = fa.plan_embeddings(fa.SegmentationOutput(_hard_weights(np.random.default_rng(7)), np.arange(EMB_CHUNKS) * 10.0, 10.0 / EMB_FRAMES), EMB_TOTAL,
                                   fa.EmbeddingConfig(batch_size=3), ctx=ctx)


def _call_embedding_windows(fa, ctx, a):
    return [a["plan"].windows(b, a["audio"]) for b in range(a["plan"].batches)]


def _call_span_inputs(fa, ctx, a):
    return list(fa.span_inputs(a["audio"], a["spans"], fa.EmbeddingConfig(batch_size=3), ctx=ctx))


def _build_resample(fa, rng):
    fresh, stale = _two(lambda r: r.standard_normal((13, 589)).astype(F))
    return Inputs(dict(rows=fresh), dict(rows=stale))


def _call_resample(fa, ctx, a):
    return [fa.weight_resample(a["rows"], 300, ctx=ctx)]


def _build_powerset(fa, rng):
    fresh, stale = _two(lambda r: (1.5 * r.standard_normal((2, 333, 7))).astype(F))
    return Inputs(dict(logits=fresh), dict(logits=stale))


def _call_powerset(fa, ctx, a):
    seg = fa.powerset_decode(a["logits"], log_probs=True, ctx=ctx)
    return [seg.speaker_weights, seg.log_probs]


def _build_reconstruct(fa, rng):
    fresh, stale = _two(lambda r: _hard_weights(r, 6, 100))
    hard = np.random.default_rng(3).integers(0, 3, (6, 3)).astype(I)
    return Inputs(dict(weights=fresh), dict(weights=stale), host=dict(hard=hard, offsets=np.arange(6) * 2.0))


def _call_reconstruct(fa, ctx, a):
    rec = fa.OfflineReconstruction(fa.ReconstructionConfig(min_segment_duration=0.0), ctx=ctx)
    segs = rec.build_segments(fa.SegmentationOutput(a["weights"], a["offsets"]), a["hard"], np.zeros((3, 2)))
    return [np.array([(s.start_time_seconds, s.end_time_seconds, s.quality_score) for s in segs], np.float64).reshape(-1, 3), np.array([s.speaker_id for s in segs], dtype="S32")]


# ---- the table ----------------------------------------------------------------------------------------------------------------------
CASES = [
    Case("pipeline-cluster", ("fa_offline_cluster",), _build_cluster, _call_cluster),
    Case("pipeline-cluster-intermediates", ("fa_offline_cluster_ex",), _build_cluster, _call_cluster_ex),
    Case("pipeline-cluster-batch", ("fa_offline_cluster_batch_dev",), _build_cluster_batch, _call_cluster_batch),
    Case("mel-execute", ("fa_mel_execute_dev",), _build_mel, _call_mel(True), setup=_setup_mel, exit_raced=True),
    Case("mel-features-batch", ("fa_mel_execute_dev", "fa_mel_normalize_per_feature_dev"), _build_mel_features, _call_mel_features, live="none",
         drains="mel.py features_batch: torch.from_numpy(valid).to(device) uploads the valid counts on torch's stream"),
    Case("ctc-greedy", ("fa_ctc_greedy_batch_dev",), _build_ctc, _call_ctc_greedy, exit_raced=True),
    Case("ctc-log-probs", ("fa_ctc_log_softmax_batch_dev",), _build_ctc, _call_ctc_log_probs(True), exit_raced=True),
    Case("tdt-tables", ("fa_tdt_greedy_tables_dev",), _build_tdt_tables, _call_tdt_tables),
    Case("tdt-logits", ("fa_tdt_greedy_logits_dev",), _build_tdt_logits, _call_tdt_logits),
    Case("tdt-logits-lang", ("fa_tdt_greedy_logits_lang_dev",), _build_tdt_logits, _call_tdt_lang),
    Case("tdt-topk", ("fa_tdt_topk_rows_dev",), _build_topk, _call_topk),
    Case("tdt-plan-windows", ("fa_tdt_plan_windows_dev",), _build_tdt_plan, _call_tdt_plan),
    Case("tdt-pack-windows", ("fa_tdt_pack_windows_dev",), _build_tdt_plan, _call_tdt_pack, setup=_setup_tdt_pack, exit_raced=True),
    Case("tdt-speech-gate", ("fa_tdt_speech_gate_dev",), _build_tdt_plan, _call_tdt_gate),
    Case("tdt-merge", ("fa_tdt_merge_windows_dev",), _build_tdt_merge, _call_tdt_merge),
    Case("rnnt-greedy", ("fa_rnnt_greedy_logits_dev",), _build_rnnt, _call_rnnt),
    Case("rnnt-stream-session", ("fa_rnnt_stream_gate_dev", "fa_rnnt_stream_mel_inputs_dev", "fa_rnnt_stream_advance_dev", "fa_rnnt_stream_track_dev",
                                 "fa_rnnt_stream_finalize_dev", "fa_rnnt_stream_merge_rescued_dev"), _build_rnnt_stream, _call_rnnt_stream, setup=_setup_rnnt_stream, live="all", exit_raced=True),
    Case("aed-decode", ("fa_aed_step_dev", "fa_aed_finish_dev"), _build_aed_decode, _call_aed_decode, setup=_setup_aed_decode, live="all", exit_raced=True),
    Case("aed-gather-hidden", ("fa_aed_gather_hidden_dev",), _build_aed_hidden, _call_aed_hidden, setup=_setup_aed_hidden, exit_raced=True),
    Case("aed-cross-mask", ("fa_aed_cross_mask_dev",), _build_aed_mask, _call_aed_mask, exit_raced=True),
    Case("aed-encoder-context", ("fa_aed_encoder_context_dev",), _build_aed_context, _call_aed_context, exit_raced=True),
    Case("aed-merge-windows", ("fa_aed_merge_windows_dev",), _build_aed_merge, _call_aed_merge),
    Case("kws-spot", ("fa_ctc_kws_spot_batch_dev",), _build_kws, _call_kws_spot),
    Case("kws-score-windows", ("fa_ctc_kws_score_windows_dev",), _build_kws, _call_kws_windows),
    Case("vocab-rescore-decide", ("fa_vocab_rescore_decide_dev",), _build_vocab_rescore, _call_vocab_rescore),
    Case("wer-edit-distance", ("fa_edit_distance_batch_dev",), _build_wer, _call_wer),
    Case("paraformer-cif", ("fa_paraformer_cif_dev",), _build_cif, _call_cif),
    Case("paraformer-timestamps", ("fa_paraformer_timestamps_dev",), _build_stamps, _call_stamps),
    Case("vad-segments", ("fa_vad_segments_dev",), _build_vad_probs, _call_vad_segments),
    Case("vad-pack-chunks", ("fa_vad_pack_chunks_dev",), _build_vad_audio, _call_vad_pack, exit_raced=True),
    Case("vad-gather-segments", ("fa_vad_gather_segments_dev",), _build_vad_audio, _call_vad_gather),
    Case("vad-stream-advance", ("fa_vad_stream_advance_dev",), _build_vad_stream, _call_vad_stream),
    Case("fsmn-pack-waveforms", ("fa_fsmn_vad_pack_waveforms_dev",), _build_fsmn, _call_fsmn_waveforms, exit_raced=True),
    Case("fsmn-pack-feats", ("fa_fsmn_vad_pack_feats_dev",), _build_fsmn, _call_fsmn_feats, exit_raced=True),
    Case("fsmn-gather-silence", ("fa_fsmn_vad_gather_silence_dev",), _build_fsmn, _call_fsmn_silence, exit_raced=True),
    Case("fsmn-segments", ("fa_fsmn_vad_segments_dev",), _build_fsmn, _call_fsmn_segments),
    Case("sortformer-pack-windows", ("fa_sortformer_pack_windows_dev",), _build_sortformer_pack, _call_sortformer_pack),
    Case("sortformer-stitch", ("fa_sortformer_stitch_dev",), _build_sortformer_stitch, _call_sortformer_stitch),
    Case("timeline-segments", ("fa_timeline_segments_dev",), _build_timeline, _call_timeline),
    Case("sortformer-stream-pack-chunks", ("fa_sortformer_stream_pack_chunks_dev",), _build_sf_pack, _call_sf_pack, exit_raced=True),
    Case("sortformer-stream-update", ("fa_sortformer_stream_update_dev",), _build_sf_update, _call_sf_update, setup=_setup_sf_update, live="all", exit_raced=True),
    Case("online-chunk-plan", ("fa_online_chunk_plan",), _build_online_plan, _call_online_plan),
    Case("online-pack-waveforms", ("fa_online_pack_waveforms_dev",), _build_online_pack, _call_online_pack, live="none",
         drains="online.py pack_waveforms: A.to_device(offsets / lengths) uploads the host ranges on torch's stream"),
    Case("online-chunk-finish", ("fa_online_chunk_finish_dev", "fa_speaker_db_assign_dev"), _build_online_finish, _call_online_finish, setup=_setup_online_finish),
    Case("online-speaker-db", ("fa_speaker_db_assign_dev", "fa_speaker_db_mergeable_pairs_dev"), _build_speaker_db, _call_speaker_db, setup=_setup_speaker_db, live="all"),
    Case("online-speaker-distances", ("fa_speaker_db_distances_dev",), _build_speaker_distances, _call_speaker_distances, setup=_setup_speaker_db),
    Case("embedding-plan", ("fa_embedding_plan_dev",), _build_embedding_plan, _call_embedding_plan),
    Case("embedding-windows", ("fa_embedding_windows_dev",), _build_embedding_audio, _call_embedding_windows, setup=_setup_embedding_windows),
    Case("embedding-span-inputs", ("fa_embedding_span_inputs_dev",), _build_embedding_audio, _call_span_inputs),
    Case("embedding-weight-resample", ("fa_weight_resample_dev",), _build_resample, _call_resample, exit_raced=True),
    Case("reconstruct-powerset-decode", ("fa_powerset_decode_dev",), _build_powerset, _call_powerset, exit_raced=True),
    Case("reconstruct-build-segments", ("fa_offline_reconstruct_dev",), _build_reconstruct, _call_reconstruct),
    Case("control-ctc-log-probs-unordered", ("fa_ctc_log_softmax_batch_dev",), _build_ctc, _call_ctc_log_probs(False), control=True, exit_raced=True),
    Case("control-mel-execute-unordered", ("fa_mel_execute_dev",), _build_mel, _call_mel(False), control=True, setup=_setup_mel, exit_raced=True),
]
