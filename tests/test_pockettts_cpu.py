"""The PocketTTS session without a GPU: the EOS machine, the window plan and the clip plan of fluidaudio_amd/csrc/pockettts_core.h against
the reference's loops (tests/cpu/pockettts_core_main.cpp, compiled with g++), the clip plan through the library against the restatement,
and the status contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pockettts_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))


def test_machine_and_plans_equal_the_naive_loops(tmp_path):
    exe = str(tmp_path / "pockettts_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "cpu", "pockettts_core_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 16655", r.stdout[-400:]   # 3 x 2047 patterns, 4 x 601 blocks, the statuses, 8109 clips


@pytest.mark.parametrize("available", [0, 12, 125, 200])
def test_clone_plan_equals_the_restatement(fa, available):
    samples = [0, 23999, 24000, 24001, 25 * 1920, 25 * 1920 + 1, 239999, 240000, 240001, 10 ** 7]
    usable, status = fa.pockettts_clone_plan(samples, available)
    assert [(int(s), int(u)) for s, u in zip(status, usable)] == [R.clone_plan(n, available) for n in samples]


def test_status_contract_needs_no_gpu(fa):
    lib, cfg = fa.lib(), fa.pockettts_config(kv_format="fp16", streams=3)
    assert (cfg.layers, cfg.kv_format, cfg.streams, cfg.voice_seq) == (6, 2, 3, 512)
    n, out = np.array([5], np.int64), np.zeros(1, np.int32)
    assert lib.fa_pockettts_clone_plan(0, n.ctypes.data, None, out.ctypes.data, out.ctypes.data) == 1
    assert lib.fa_pockettts_clone_plan(1, (-n).ctypes.data, None, out.ctypes.data, out.ctypes.data) == 1
    assert lib.fa_pockettts_session_create(None, C.byref(cfg), None) == 1 and lib.fa_pockettts_plan(None, 1, None, None, None, None, None, None) == 1
