"""The arithmetic of ``OfflineDiarizerManager.cluster`` (reference:
Sources/FluidAudio/Diarizer/Offline/Core/OfflineDiarizerManager.swift:270-375) on precomputed embeddings — the "embeddings in
-> final per-embedding cluster ids out" path of BASELINE config 5.  ``cluster_embeddings`` is ONE call into the library
(``fa_offline_cluster``, csrc/offline_host.hip: inputs go up once, the intermediates stay in HBM); ``cluster_embeddings_stagewise``
is the same composition made of the single-stage entries (every intermediate crosses PCIe), kept because it exposes the
intermediate results (AHC labels, VBx posteriors) the tests compare with the CPU restatement:

    select finite embeddings (:591-611) -> AHC (AHCClustering.cluster, threshold 0.6) -> VBx refine (Fa 0.07, Fb 0.8,
    <= 20 iterations) -> gamma-weighted centroids of the active speakers (:613-691) -> cosine scores (:789-798) ->
    constrained per-chunk assignment (ConstrainedClusterAssignment, default) or plain argmax (:800-822).

Speaker-count constraints (numSpeakers / minSpeakers / maxSpeakers, :308-326) route through
``VBxClustering.refine_with_constraints`` and the batched K-Means fallback; as in the reference (:355-358) the constrained
assignment is skipped when the count was forced.  Segmentation, embedding extraction and PLDA are CoreML models in the
reference (out of scope)."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from .ahc import AHCClustering
from .kmeans import SpeakerCountConstraints
from .post import ConstrainedClusterAssignment, assign_embeddings, centroid_scores, compute_centroids
from .vbx import VBxClustering, VBxOutput


@dataclass
class OfflineClusteringConfig:  # OfflineDiarizerTypes.swift:155-163,189-192
    clustering_threshold: float = 0.6
    warm_start_fa: float = 0.07
    warm_start_fb: float = 0.8
    max_vbx_iterations: int = 20
    convergence_tolerance: float = 1e-4
    constrained_assignment: bool = True
    num_speakers: int | None = None      # OfflineDiarizerTypes.swift clustering.numSpeakers / minSpeakers / maxSpeakers
    min_speakers: int | None = None
    max_speakers: int | None = None

    def validate(self) -> None:
        """The clustering / VBx guards of OfflineDiarizerConfig.validate (OfflineDiarizerTypes.swift:357-408; the reference throws
        OfflineDiarizationError.invalidConfiguration with these messages before any audio is touched)."""
        t = self.clustering_threshold
        if not (t > 0 and t <= 2.0):                         # distances between unit rows live in [0, 2] (:358-364); NaN fails too
            raise ValueError(f"invalidConfiguration: clustering.threshold must be within (0, 2], got {t}")
        if not (self.warm_start_fa > 0 and self.warm_start_fb > 0):
            raise ValueError(f"invalidConfiguration: clustering warm-start Fa/Fb must be positive (Fa={self.warm_start_fa}, Fb={self.warm_start_fb})")
        if not self.max_vbx_iterations > 0:
            raise ValueError(f"invalidConfiguration: maxVBxIterations must be > 0, got {self.max_vbx_iterations}")
        if not self.convergence_tolerance > 0:
            raise ValueError("invalidConfiguration: convergenceTolerance must be positive")


@dataclass
class ClusteringResult:
    assignments: list
    centroids: np.ndarray
    initial_clusters: list
    vbx: VBxOutput
    training_indices: list = field(default_factory=list)
    timings: dict = field(default_factory=dict)
    info: dict = field(default_factory=dict)


def select_training_embeddings(embedding256) -> list:
    """selectTrainingEmbeddings (:591-611): indices of the rows without NaN/Inf; all rows if none qualifies."""
    e = np.asarray(embedding256)
    ok = np.isfinite(e).all(axis=1) if e.ndim == 2 and e.size else np.zeros(len(e), bool)
    sel = np.nonzero(ok)[0].tolist()
    return sel if sel else list(range(len(e)))


def _resident(t, dtype_name: str, ctx: L.Context, what: str):
    """A matrix the device-pointer forms read behind its pointer: a contiguous two-dimensional torch CUDA tensor of exactly that dtype
    (the library reads the bytes as they are: an int32 tensor would be taken for floats) on the context's device.  Refused before any
    library call: TypeError for what is no such tensor, ValueError for one on another device, as _args.device_tensor does."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError(f"{what}: a torch CUDA tensor is required")
    if t.dtype != getattr(torch, dtype_name) or t.dim() != 2 or not t.is_contiguous():
        raise TypeError(f"{what}: a contiguous two-dimensional {dtype_name} tensor is required, not {t.dtype} {tuple(t.shape)} with strides {tuple(t.stride())}")
    if t.device.index != ctx.device:
        raise ValueError(f"{what} on {t.device}, context on cuda:{ctx.device}")
    return t


def _rho_dim(rho, ctx: L.Context, what: str) -> int:
    """The PLDA dimension of device-resident rho: 0 — no VBx, nothing is read behind the pointer — for None and for a tensor that is empty or
    not two-dimensional, as ever; a matrix that is read has to be what _resident asks for."""
    if rho is None:
        return 0
    if not hasattr(rho, "data_ptr"):
        raise TypeError(f"{what}: a torch CUDA tensor beside device-resident embeddings, or None")
    if rho.dim() != 2 or rho.numel() == 0:
        return 0
    return int(_resident(rho, "float64", ctx, what).shape[1])


def cluster_embeddings(embedding256, rho128, chunk_indices, phi, config: OfflineClusteringConfig | None = None,
                       ctx: L.Context | None = None, intermediates: bool = False) -> ClusteringResult:
    """One device-resident call (fa_offline_cluster).  ``initial_clusters`` / ``vbx`` of the result are not populated (they never
    leave the device) unless ``intermediates`` asks for copies (fa_offline_cluster_ex: AHC labels in ``initial_clusters``, VBx hard
    labels and ELBOs in ``info["vbx_hard"]`` / ``info["elbos"]``); ``timings`` carries the library's per-stage wall-clock and
    ``info`` its counters.  Embeddings / rho given as torch CUDA tensors (float32 / float64, contiguous, on ctx's device) are read where
    they are (device_pointers = 1), on ctx's stream, ordered against torch's current stream (Context.torch_ordered): whatever produces
    them there is complete when the stage reads them."""
    import ctypes as C
    cfg = config or OfflineClusteringConfig()
    cfg.validate()
    ctx = ctx or L.default_context()
    on_device = hasattr(embedding256, "data_ptr")          # torch CUDA tensors: device_pointers = 1, nothing is uploaded
    if on_device:
        emb = _resident(embedding256, "float32", ctx, "cluster_embeddings: embeddings")
        rho = rho128
        if emb.shape[0] == 0:
            raise ValueError("noSpeechDetected")
        n, d = int(emb.shape[0]), int(emb.shape[1])
        rd = _rho_dim(rho, ctx, "cluster_embeddings: rho")
        if rd and int(rho.shape[0]) != n:
            raise ValueError(f"cluster_embeddings: rho has {int(rho.shape[0])} rows, the embeddings {n}")
        emb_ptr, rho_ptr = emb.data_ptr(), (rho.data_ptr() if rd else None)
    else:
        emb = np.ascontiguousarray(embedding256, np.float32)
        if emb.ndim != 2 or emb.shape[0] == 0:
            raise ValueError("noSpeechDetected")                                 # :281-283
        n, d = emb.shape
        rho = np.ascontiguousarray(rho128, np.float64)
        rd = rho.shape[1] if rho.ndim == 2 and rho.size else 0
        emb_ptr, rho_ptr = emb.ctypes.data, (rho.ctypes.data if rd else None)
    ph = np.ascontiguousarray(phi, np.float64)
    if rd and ph.size != rd:
        ph = np.ones(rd)                                                      # dimension mismatch -> identity (VBxClustering.swift:72-76)
    chunks = np.ascontiguousarray(chunk_indices, np.int32)
    c = L.OfflineClusterConfig()
    L.lib().fa_offline_cluster_default_config(C.byref(c))
    c.clustering_threshold, c.warm_start_fa, c.warm_start_fb = cfg.clustering_threshold, cfg.warm_start_fa, cfg.warm_start_fb
    c.max_vbx_iterations, c.convergence_tolerance = cfg.max_vbx_iterations, cfg.convergence_tolerance
    c.constrained_assignment = int(cfg.constrained_assignment)
    c.num_speakers = -1 if cfg.num_speakers is None else cfg.num_speakers
    c.min_speakers = -1 if cfg.min_speakers is None else cfg.min_speakers
    c.max_speakers = -1 if cfg.max_speakers is None else cfg.max_speakers
    labels = np.zeros(n, np.int32)
    cap = 256
    cen = np.zeros((cap, d), np.float64)
    k, info = C.c_int32(), L.OfflineClusterInfo()
    if intermediates:
        ahc_lab, hard, elbos = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(max(cfg.max_vbx_iterations, 1))
        with ctx.torch_ordered(on_device):
            st = L.lib().fa_offline_cluster_ex(ctx.handle, emb_ptr, n, d, rho_ptr, rd, chunks.ctypes.data,
                                               ph.ctypes.data if rd else None, C.byref(c), int(on_device), labels.ctypes.data, cen.ctypes.data, cap, C.byref(k),
                                               C.byref(info), ahc_lab.ctypes.data, hard.ctypes.data, elbos.ctypes.data)
        ctx.check(st, "fa_offline_cluster_ex")
    else:
        with ctx.torch_ordered(on_device):
            st = L.lib().fa_offline_cluster(ctx.handle, emb_ptr, n, d, rho_ptr, rd, chunks.ctypes.data,
                                            ph.ctypes.data if rd else None, C.byref(c), int(on_device), labels.ctypes.data, cen.ctypes.data, cap, C.byref(k),
                                            C.byref(info))
        ctx.check(st, "fa_offline_cluster")
    t = {"inputs_s": info.inputs_s, "ahc_s": info.ahc_s, "vbx_s": info.vbx_s, "assign_s": info.assign_s, "total_s": info.total_s}
    res = ClusteringResult(labels if intermediates else np.asarray(labels).tolist(), cen[:k.value].copy(), [], None, [], t)
    res.info = {f: getattr(info, f) for f, _ in info._fields_ if f != "ahc"}
    res.info["ahc"] = info.ahc.as_dict()
    if intermediates:
        nt = int(info.training_rows)
        res.initial_clusters = ahc_lab[:nt]
        res.info["vbx_hard"] = hard[:nt]
        res.info["elbos"] = elbos[:int(info.vbx_iterations)].copy()
    return res


class _DevArray:
    """A torch CUDA tensor behind the few ndarray attributes cluster_embeddings_batch reads (shape / ndim / size / ctypes.data = the device address)."""

    class _Ptr:
        def __init__(self, p):
            self.data = p

    def __init__(self, t):
        self.t = t
        self.shape = tuple(t.shape) if t is not None else (0,)
        self.ndim = len(self.shape)
        self.size = int(t.numel()) if t is not None else 0
        self.ctypes = _DevArray._Ptr(int(t.data_ptr()) if t is not None and t.numel() else 0)


def _c_config(cfg: OfflineClusteringConfig):
    import ctypes as C
    c = L.OfflineClusterConfig()
    L.lib().fa_offline_cluster_default_config(C.byref(c))
    c.clustering_threshold, c.warm_start_fa, c.warm_start_fb = cfg.clustering_threshold, cfg.warm_start_fa, cfg.warm_start_fb
    c.max_vbx_iterations, c.convergence_tolerance = cfg.max_vbx_iterations, cfg.convergence_tolerance
    c.constrained_assignment = int(cfg.constrained_assignment)
    c.num_speakers = -1 if cfg.num_speakers is None else cfg.num_speakers
    c.min_speakers = -1 if cfg.min_speakers is None else cfg.min_speakers
    c.max_speakers = -1 if cfg.max_speakers is None else cfg.max_speakers
    return c


def cluster_embeddings_batch(recordings, phi, config: OfflineClusteringConfig | None = None, ctx: L.Context | None = None):
    """Several recordings through the clustering stage in one call (fa_offline_cluster_batch: their merge chains advance together).
    recordings: iterable of (embedding256 [n, d] float32, rho128 [n, rho_dim] float64, chunk_indices [n]) with common d / rho_dim.
    Embeddings / rho given as torch CUDA tensors (all recordings, or none; float32 / float64, contiguous, on ctx's device) go through
    fa_offline_cluster_batch_dev: nothing is uploaded, and the call is ordered against torch's current stream (Context.torch_ordered).
    Returns (statuses, [ClusteringResult | None]) — per recording identical to cluster_embeddings()."""
    import ctypes as C
    cfg = config or OfflineClusteringConfig()
    cfg.validate()
    ctx = ctx or L.default_context()
    recordings = list(recordings)
    on_device = bool(recordings) and all(hasattr(e, "data_ptr") for e, _, _ in recordings)
    if on_device:
        for i, (e, r, _) in enumerate(recordings):
            _resident(e, "float32", ctx, f"cluster_embeddings_batch: embeddings of recording {i}")
            _rho_dim(r, ctx, f"cluster_embeddings_batch: rho of recording {i}")
        recs = [(_DevArray(e), _DevArray(r), np.ascontiguousarray(c, np.int32)) for e, r, c in recordings]
    else:
        recs = [(np.ascontiguousarray(e, np.float32), np.ascontiguousarray(r, np.float64), np.ascontiguousarray(c, np.int32)) for e, r, c in recordings]
    k = len(recs)
    if k == 0:
        return [], []
    d = recs[0][0].shape[1]
    rd = recs[0][1].shape[1] if recs[0][1].ndim == 2 and recs[0][1].size else 0
    ph = np.ascontiguousarray(phi, np.float64)
    if rd and ph.size != rd:
        ph = np.ones(rd)
    cap = 256
    labels = [np.zeros(max(e.shape[0], 1), np.int32) for e, _, _ in recs]
    cens = [np.zeros((cap, d), np.float64) for _ in recs]
    dummy = np.zeros(4, np.float32)
    P = C.c_void_p * k
    ep = P(*[e.ctypes.data if e.size else dummy.ctypes.data for e, _, _ in recs])
    rp = P(*[r.ctypes.data if r.size else dummy.ctypes.data for _, r, _ in recs])
    cp = P(*[c.ctypes.data if c.size else dummy.ctypes.data for _, _, c in recs])
    lp = P(*[x.ctypes.data for x in labels])
    zp = P(*[x.ctypes.data for x in cens])
    ns = (C.c_int64 * k)(*[e.shape[0] for e, _, _ in recs])
    kc = (C.c_int32 * k)()
    infos = (L.OfflineClusterInfo * k)()
    st = (C.c_int32 * k)()
    c = _c_config(cfg)
    entry = L.lib().fa_offline_cluster_batch_dev if on_device else L.lib().fa_offline_cluster_batch
    with ctx.torch_ordered(on_device):
        entry(ctx.handle, k, ep, ns, d, rp if rd else None, rd, cp, ph.ctypes.data if rd else None, C.byref(c), lp, zp, cap, kc, infos, st)
    out = []
    for i in range(k):
        if st[i] != L.SUCCESS:
            out.append(None)
            continue
        info = infos[i]
        t = {"inputs_s": info.inputs_s, "ahc_s": info.ahc_s, "vbx_s": info.vbx_s, "assign_s": info.assign_s, "total_s": info.total_s}
        res = ClusteringResult(labels[i][:recs[i][0].shape[0]].tolist(), cens[i][:kc[i]].copy(), [], None, [], t)
        res.info = {f: getattr(info, f) for f, _ in info._fields_ if f != "ahc"}
        res.info["ahc"] = info.ahc.as_dict()
        out.append(res)
    return [int(v) for v in st], out


def cluster_embeddings_stagewise(embedding256, rho128, chunk_indices, phi, config: OfflineClusteringConfig | None = None,
                                 ctx: L.Context | None = None) -> ClusteringResult:
    import time
    cfg = config or OfflineClusteringConfig()
    cfg.validate()
    ctx = ctx or L.default_context()
    t = {}
    emb = np.asarray(embedding256, np.float32).astype(np.float64)          # Float -> Double widening (:286)
    rho = np.ascontiguousarray(rho128, np.float64)
    if emb.shape[0] == 0:
        raise ValueError("noSpeechDetected")                                 # :281-283
    train = select_training_embeddings(embedding256)
    temb, trho = emb[train], rho[train]
    t0 = time.perf_counter()
    if len(train) >= 2:
        initial = AHCClustering(ctx=ctx).cluster(temb, cfg.clustering_threshold)   # :301-306
    else:
        initial = [0] * len(train)
    t["ahc_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    if trho.size and initial:
        has = cfg.num_speakers is not None or cfg.min_speakers is not None or cfg.max_speakers is not None   # :309-312
        cons = SpeakerCountConstraints.resolve(len(train), cfg.num_speakers, cfg.min_speakers, cfg.max_speakers) if has else None
        vbx = VBxClustering(phi, cfg.max_vbx_iterations, cfg.convergence_tolerance, cfg.warm_start_fa, cfg.warm_start_fb,
                            ctx=ctx).refine_with_constraints(trho, temb, initial, cons)    # :328-333
    else:
        vbx = VBxOutput(np.zeros((0, 0)), np.zeros(0), [list(initial)], [], (max(initial) + 1) if initial else 0, [])
    t["vbx_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    centroids = np.zeros((0, emb.shape[1]))
    if vbx.was_adjusted and len(vbx.centroids):                              # K-Means centroids as they are (:622-629)
        centroids = np.asarray(vbx.centroids, np.float64)
    elif vbx.gamma.size and vbx.pi.size:
        centroids, _ = compute_centroids(temb, vbx.gamma, vbx.pi, ctx=ctx)  # :613-684
    if centroids.shape[0] == 0:                                              # computeCentroidsFromClusters (:686-) fallback
        labs = np.asarray(initial)
        # sequential sums in row order (cblas_daxpy per row, :700-728), then one division: numpy's mean() sums pairwise
        centroids = np.stack([np.cumsum(temb[labs == k], axis=0)[-1] / float((labs == k).sum()) for k in sorted(set(initial))]) if len(initial) else centroids
    use_constrained = cfg.constrained_assignment and not vbx.was_adjusted and centroids.shape[0] > 1  # :355-358
    if use_constrained:
        scores = centroid_scores(emb, centroids, ctx=ctx)
        assignments = ConstrainedClusterAssignment.assign(scores, chunk_indices, ctx=ctx)
    else:
        assignments = assign_embeddings(emb, centroids, ctx=ctx)
    t["assign_s"] = time.perf_counter() - t0
    return ClusteringResult(assignments, centroids, list(initial), vbx, train, t)


@dataclass
class DiarizationSegments:
    segments: list
    speaker_database: dict
    clustering: ClusteringResult
    hard_clusters: np.ndarray
    info: dict = field(default_factory=dict)


def diarize_segments(embedding256, rho128, chunk_indices, speaker_indices, phi, segmentation, config: OfflineClusteringConfig | None = None,
                     reconstruction=None, span_embedder=None, ctx: L.Context | None = None) -> DiarizationSegments:
    """The rest of OfflineDiarizerManager.cluster (:377-467) behind ``cluster_embeddings``: chunk assignments (buildChunkAssignments,
    :885-911) -> OfflineReconstruction.buildSegments -> buildSpeakerDatabase, i.e. DiarizationResult.segments / .speakerDatabase.
    ``segmentation`` is a ``reconstruct.SegmentationOutput`` (speaker weights [chunks, frames, speakers], numpy or a torch CUDA tensor:
    ``powerset_decode`` of the segmentation logits); ``speaker_indices`` is each embedding's local speaker slot in its chunk;
    ``reconstruction`` a ``reconstruct.ReconstructionConfig``."""
    from .reconstruct import OfflineReconstruction, chunk_assignments
    ctx = ctx or L.default_context()
    res = cluster_embeddings(embedding256, rho128, chunk_indices, phi, config, ctx=ctx)
    nc, _, ns = segmentation.shape
    k = int(res.centroids.shape[0])
    hard = chunk_assignments(chunk_indices, speaker_indices, res.assignments, k, nc, ns)
    rec = OfflineReconstruction(reconstruction, ctx=ctx)
    segs = rec.build_segments(segmentation, hard, res.centroids, span_embedder)
    return DiarizationSegments(segs, rec.build_speaker_database(segs, res.centroids), res, hard, dict(rec.last_info))


@dataclass
class ExtractedEmbeddings:
    """extractEmbeddings' [TimedEmbedding] as arrays, in the reference's order: what diarize_segments takes (embedding256 [n, 256] fp32,
    rho128 [n, 128] fp64, chunk_indices, speaker_indices) plus the metadata records (embedding.RECORD_DTYPE) and the plan behind them."""
    embedding256: np.ndarray
    rho128: np.ndarray
    chunk_indices: np.ndarray
    speaker_indices: np.ndarray
    records: np.ndarray
    plan: object


def extract_embeddings(segmentation, audio, embedder, plda, config=None, ctx: L.Context | None = None) -> ExtractedEmbeddings:
    """OfflineEmbeddingExtractor.extractEmbeddings (OfflineEmbeddingExtractor.swift:177-711) with the networks supplied by the caller:
    ``embedder(windows [Bw, S], weights [Br, W], window_of_run [Br]) -> [Br, 256]`` is called once per fbank batch with that batch's
    audio windows, the resampled masks of its model runs and, per run, the index of its window in ``windows`` (all torch CUDA tensors);
    ``plda(emb [n, 256]) -> rho [n, 128]`` (fp64).  ``segmentation``: a ``reconstruct.SegmentationOutput`` (speaker weights on the host
    are moved to ctx's device first); ``audio``: the recording, fp32.  ``config``: an ``embedding.EmbeddingConfig``.  Jobs skipped by maskSimilarity carry their cached
    run's embedding."""
    import torch
    from .embedding import EmbeddingConfig, plan_embeddings
    ctx = ctx or L.default_context()
    cfg = config or EmbeddingConfig()
    dev = torch.device("cuda", ctx.device)
    a = audio if hasattr(audio, "data_ptr") else torch.from_numpy(np.ascontiguousarray(audio, np.float32))
    a = a.to(dev, torch.float32).contiguous()
    w = segmentation.speaker_weights
    if not (hasattr(w, "is_cuda") and w.is_cuda):                       # the device entry: run_weights stay on the device for the embedder
        w = torch.as_tensor(np.ascontiguousarray(w, np.float32) if not hasattr(w, "data_ptr") else w).to(dev, torch.float32)
        segmentation = dataclasses.replace(segmentation, speaker_weights=w)
    plan = plan_embeddings(segmentation, a.numel(), cfg, ctx=ctx)
    runs = int(plan.info["runs"])
    run_emb = []
    for b in range(plan.batches):
        r = plan.batch_runs(b)
        if len(r) == 0:
            continue
        wins = plan.windows(b, a)
        wor = torch.as_tensor(plan.window_of_run[r.start:r.stop] - plan.batch_windows(b).start, dtype=torch.int64, device=dev)
        e = embedder(wins, plan.run_weights[r.start:r.stop], wor)
        run_emb.append(torch.as_tensor(e).detach().float().cpu().numpy())
    emb_runs = np.concatenate(run_emb, axis=0) if run_emb else np.zeros((runs, 256), np.float32)
    emb = np.ascontiguousarray(emb_runs[plan.run_of_job], np.float32) if plan.run_of_job.size else np.zeros((0, emb_runs.shape[1]), np.float32)
    rho = np.asarray(torch.as_tensor(plda(emb)).detach().double().cpu().numpy(), np.float64) if emb.shape[0] else np.zeros((0, 128))
    return ExtractedEmbeddings(emb, rho, plan.chunk_indices, plan.speaker_indices, plan.records, plan)


def span_embedder(audio, embedder, config=None, ctx: L.Context | None = None):
    """A ``span_embedder(start_s, end_s) -> embedding or None`` for ``OfflineReconstruction.build_segments`` (the zero-vote re-embed pass):
    embedSpan (OfflineEmbeddingExtractor.swift:243-297) through ``embedding.span_inputs`` and the same ``embedder`` as extract_embeddings
    (one window, one run); None for a span without samples."""
    import torch
    from .embedding import EmbeddingConfig, span_inputs
    ctx = ctx or L.default_context()
    cfg = config or EmbeddingConfig()
    a = audio if hasattr(audio, "data_ptr") else torch.from_numpy(np.ascontiguousarray(audio, np.float32))
    a = a.to(torch.device("cuda", ctx.device), torch.float32).contiguous()

    def embed(start_s, end_s):
        win, wts, ok = span_inputs(a, [(start_s, end_s)], cfg, ctx=ctx)
        if not bool(ok[0]):
            return None
        e = embedder(win, wts, torch.zeros(1, dtype=torch.int64, device=a.device))
        return torch.as_tensor(e).detach().float().cpu().numpy()[0]
    return embed
