"""`python bench.py --gpus N` starts its own N ranks (the driver's N = 1 command form with another N): the launcher, the
rendezvous on 127.0.0.1 and the rank count the process group really saw — without a GPU (control flow only, gloo) and, on the GPU box, the
whole bench line of two ranks sharing the one device (FA_BENCH_BACKEND=gloo: a rehearsal of every N > 1 leg incl. the sharded-VBx all-gather).
A plain run times the headline alone; `--full` adds every other leg."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strict(text):
    def refuse(name):
        raise ValueError(f"{name} is not JSON")
    return json.loads(text, parse_constant=refuse)


def _run(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (_strict(lines[-1]) if lines else None)


def _legs(r):
    out = {}
    for l in r.stdout.splitlines():
        if l.startswith('{"leg"'):
            rec = _strict(l)
            out[rec["leg"]] = rec["result"]
    return out


def test_bare_command_with_gpus_2_starts_two_ranks():
    r, line = _run(["--gpus", "2", "--launch-check"], timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert line == {"launch_check": True, "n_gpus": 2, "world_size_env": 2, "backend": "gloo"}


def test_single_rank_needs_no_launcher():
    r, line = _run(["--launch-check"], timeout=120)
    assert r.returncode == 0 and line["n_gpus"] == 1


def test_rank_count_that_differs_from_gpus_is_refused():
    r, line = _run(["--gpus", "2", "--launch-check"], {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"}, timeout=120)
    assert r.returncode == 2 and line is None and "WORLD_SIZE 3" in r.stderr


@pytest.mark.gpu
def test_two_ranks_on_the_one_gpu_print_a_whole_line():
    """Two ranks, gloo, both on cuda:0, a 1 h recording each, --full: n_gpus is what the process group saw, every N > 1 leg ran."""
    r, line = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--hours", "1", "--mel-steps", "5", "--mel-warmup", "2", "--clock-warm-s", "0",
                    "--chunks", "64", "--ctc-matrices", "64", "--full"], {"FA_BENCH_BACKEND": "gloo"}, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    last = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert len(last) < 4096                                             # the driver parses this line: small, strict JSON (round 5's 25 KB line was not parsed)
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["steps"] == 2
    assert line["roofline"]["frac"] > 0 and line["cpu_baseline"] is None and len(line["config"]) <= 13
    assert line["config"]["e2e_all_ranks_ok"] is True and line["config"]["vbx_sharded_all_ranks_same_elbos"] is True
    assert line["config"]["ctc_matrices_per_s_strong_scaled"] > 0 and line["config"]["e2e_slowest_rank_audio_hours_per_s"] > 0
    assert abs(line["value"] - 2 * 1.0 * 2 / (line["ms_per_step"] * 2 / 1e3)) < 1e-4 * line["value"]
    legs = _legs(r)                                                     # every N > 1 leg ran and was printed as its own line
    assert legs["e2e_8h"]["all_ranks_ok"] is True
    assert legs["vbx_sharded"]["all_ranks_same_elbos"] is True and legs["vbx_sharded"]["elbos_equal_single_device"] is True
    assert legs["ctc"]["ids_exact"] is True and legs["ctc"]["matrices_per_rank"] == 32
    full = json.load(open(os.path.join(ROOT, "bench_legs.json")))
    assert full["vbx_sharded"] == legs["vbx_sharded"] and full["n_gpus"] == 2


def test_steps_below_one_are_refused():
    r, line = _run(["--steps", "0"], timeout=120)
    assert r.returncode == 2 and line is None and "--steps" in r.stderr


@pytest.mark.parametrize("extra", ["--cpu-full", "--in-flight", "--vbx-sharded"])
def test_options_that_add_to_the_full_legs_need_full(extra):
    r, line = _run(["--steps", "1", extra], timeout=120)
    assert r.returncode == 2 and line is None and extra in r.stderr and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone(tmp_path):
    """The driver's own command form, shortened: no leg but the headline's, no summary line, the result line last (strict JSON < 4 KB,
    the contract's keys, cpu_baseline null); --dump-outputs writes what the last timed step returned."""
    dump = tmp_path / "dump"
    r, line = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--hours", "1", "--dump-outputs", str(dump)], timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and lines[0].startswith('{"leg": "e2e_8h"') and len(lines[1]) < 4096
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "audio_hours/s" and line["higher_is_better"] is True
    assert line["metric"].startswith("audio hours/sec featurized+clustered per node") and line["dtype"] == "f64"
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1
    assert line["cpu_baseline"] is None and line["config"]["ahc_50k_seconds"] is None and line["config"]["mel_realtime_factor"] is None
    assert abs(line["value"] - 1.0 * 2 / (line["ms_per_step"] * 2 / 1e3)) < 1e-4 * line["value"]
    h = _legs(r)["e2e_8h"]
    assert h["labels_match_speakers"] is True and h["identical_every_step"] is True and h["all_ranks_ok"] is True
    assert h["digest_checks"] is None and h["mel_s"] is None                        # runs of their own: --full only
    import numpy as np
    out = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert set(out) == {"mel", "mel_chunk_index", "mel_lengths", "assignments", "centroids"}
    assert out["mel"].shape[:2] == (32, 128) and (out["mel_lengths"] == 1501).all() and out["mel_lengths"].shape == (240,)
    assert out["assignments"].shape == (5400,) and out["centroids"].shape == (h["clusters_found"], 256)


@pytest.mark.gpu
def test_plain_two_rank_run_times_the_headline_alone():
    """Two ranks, gloo, both on cuda:0, without --full: the headline on every rank, no other leg, the line of rank 0 last."""
    r, line = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--hours", "1"], {"FA_BENCH_BACKEND": "gloo"}, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert set(_legs(r)) == {"e2e_8h"} and '{"summary"' not in r.stdout
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["cpu_baseline"] is None
    assert line["config"]["e2e_all_ranks_ok"] is True and line["config"]["e2e_slowest_rank_audio_hours_per_s"] > 0
    assert line["config"]["vbx_sharded_all_ranks_same_elbos"] is None and line["config"]["ctc_matrices_per_s_strong_scaled"] is None
    assert abs(line["value"] - 2 * 1.0 * 2 / (line["ms_per_step"] * 2 / 1e3)) < 1e-4 * line["value"]


@pytest.mark.gpu
def test_single_gpu_run_prints_a_line_the_driver_can_parse(tmp_path):
    """A --full run, shortened: last line strict JSON < 4 KB with roofline + cpu_baseline, legs on their own lines;
    --dump-outputs writes what the last timed step returned."""
    dump = tmp_path / "dump"
    r, line = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--hours", "1", "--mel-steps", "5", "--mel-warmup", "2", "--clock-warm-s", "0",
                    "--chunks", "64", "--ctc-matrices", "64", "--skip-ahc", "--skip-e2e", "--skip-beam", "--skip-resample", "--dump-outputs", str(dump),
                    "--full"], timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    last = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert len(last) < 4096
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "audio_hours/s"
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1
    assert line["cpu_baseline"]["kind"] in ("port", "reference") and line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] == 1
    assert abs(line["value"] - 1.0 * 2 / (line["ms_per_step"] * 2 / 1e3)) < 1e-4 * line["value"]
    legs = _legs(r)
    assert {"e2e_8h", "cpu_baseline", "mel", "ctc"} <= set(legs)
    summary = [l for l in r.stdout.splitlines() if l.startswith('{"summary"')]
    assert len(summary) == 1 and _strict(summary[0])["summary"]["errors"] == []
    import numpy as np
    out = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert set(out) == {"mel", "mel_chunk_index", "mel_lengths", "assignments", "centroids"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values()) and sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["mel"].shape[:2] == (32, 128) and out["mel_chunk_index"].shape == (32,) and np.isfinite(out["mel"]).all()
    assert (out["mel_lengths"] == 1501).all() and out["mel_lengths"].shape == (240,)              # 1 h = 240 chunks of 15 s
    assert out["assignments"].shape == (5400,) and out["centroids"].shape == (legs["e2e_8h"]["clusters_found"], 256)
    assert set(out["assignments"].tolist()) <= set(range(legs["e2e_8h"]["clusters_found"]))


@pytest.mark.gpu
def test_nccl_with_more_ranks_than_gpus_fails_loudly():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer GPUs than ranks")
    r, line = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], timeout=300)
    assert r.returncode != 0 and line is None and "needs 2 visible GPUs" in r.stderr
