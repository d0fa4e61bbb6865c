"""fluidaudio::OfflineEmbeddingPlanner (include/fluidaudio.hpp) from a C++ host built with g++ -Werror (tests/cabi/embedding_host.cpp): the
flattening of [[[Float]]] weights and the plan on the device against the Python path (fluidaudio_amd.plan_embeddings) and the numpy
restatement (tests/embedding_restatement.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import embedding_restatement as E  # noqa: E402


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "embedding_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "embedding_host.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def test_host_compiles(host):
    assert os.path.exists(host)


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [None, 0.9])
def test_plan_on_the_device(fa, gpu_ctx, host, tmp_path, skip):
    rng = np.random.default_rng(12)
    C, F, S, W = 45, 120, 3, 150
    w = np.zeros((C, F, S), np.float32)
    for c in range(C):                                                             # one block of speech per speaker, some overlapping
        for s in range(S):
            a = int(rng.integers(0, F - 30))
            w[c, a:a + int(rng.integers(20, 80)), s] = 1
    w[::4, :, 1] = rng.random((len(range(0, C, 4)), F)).astype(np.float32)      # some soft rows
    offs = np.arange(C - 5) * 1.5
    total = 16000 * 62
    p = tmp_path / "in.txt"
    p.write_text(f"{C} {F} {S} {W} 7 {int(skip is not None)} {skip or 0.0!r} 1 {total} {offs.size}\n"
                 + " ".join(f"{float(v):.9g}" for v in w.reshape(-1)) + "\n" + " ".join(repr(float(o)) for o in offs) + "\n")
    r = subprocess.run([host, str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    cfg = fa.EmbeddingConfig(weight_frames=W, batch_size=7, skip_threshold=skip)
    py = fa.plan_embeddings(fa.SegmentationOutput(w, offs), total, cfg, mask_rows=True, ctx=gpu_ctx)
    want = E.plan(w, offs, total, E.Config(weight_frames=W, batch_size=7, skip_threshold=skip))
    recs = [ln for ln in lines if ln[0] == "REC"]
    assert len(recs) == len(py.records) == len(want["records"]) > 0
    for ln, rec, run in zip(recs, py.records, py.run_of_job):
        assert [int(x) for x in ln[1:5]] == [int(rec[k]) for k in ("chunk_index", "speaker_index", "start_frame", "end_frame")]
        assert int(ln[5], 16) == int(rec["start_time"].view(np.uint64)) and int(ln[6], 16) == int(rec["end_time"].view(np.uint64))
        assert int(ln[7]) == run
    assert py.run_of_job.tolist() == want["run_of_job"].tolist()
    assert [(int(a), int(b)) for _, a, b in (ln for ln in lines if ln[0] == "WIN")] == list(zip(py.window_chunk.tolist(), py.window_start.tolist()))
    runs = [ln for ln in lines if ln[0] == "RUN"]
    assert [int(ln[1]) for ln in runs] == py.window_of_run.tolist()
    assert np.array_equal(np.array([[int(x, 16) for x in ln[2:]] for ln in runs], np.uint32), want["run_rows"].view(np.uint32))
    masks = np.array([[int(x, 16) for x in ln[1:]] for ln in lines if ln[0] == "MASK"], np.uint32)
    assert np.array_equal(masks, want["mask_rows"].view(np.uint32))
    info = [ln for ln in lines if ln[0] == "INFO"][0]
    assert [int(x) for x in info[1:]] == [want["evaluated"], want["empty"], want["fallback"], want["skipped"]]
