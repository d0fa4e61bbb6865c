"""The fbank front end without a GPU: the kernel's store plan against the naive LFR gather (tests/cpu/fbank_core_main.cpp compiles
fluidaudio_amd/csrc/fbank_core.h with g++), the row count against the schedule the FSMN-VAD unit assumes, and the status contract."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def test_store_plan_equals_the_gather_and_covers_every_element_once(tmp_path):
    exe = str(tmp_path / "fbank_core")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "cpu", "fbank_core_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 328", r.stdout[-400:]   # 4 shapes x 2 tails x 41 lengths


def test_valid_rows_of_5_1_are_the_fsmn_vad_frame_count(fa):
    cfg = fa.fbank_config(lfr_m=5, lfr_n=1, tail_mode="valid")
    for samples in range(2001):
        assert fa.fbank_num_rows(cfg, fa.fbank_num_frames(cfg, samples)) == fa.fsmn_vad_frame_count(samples), samples


def test_status_contract_needs_no_gpu(fa):
    lib, cfg = fa.lib(), fa.fbank_config()
    assert (cfg.n_mels, cfg.window_type, cfg.lfr_m, cfg.lfr_n, cfg.tail_mode) == (80, 0, 7, 6, 0)
    assert [fa.fbank_num_frames(cfg, n) for n in (0, 399, 400, 559, 560)] == [0, 0, 1, 1, 2]
    assert [fa.fbank_num_rows(cfg, t) for t in (0, 1, 6, 7, 13)] == [0, 1, 1, 2, 3]
    offs, out, plan = np.zeros(2, np.int64), np.zeros(4, np.float32), C.c_void_p()
    assert lib.fa_fbank_num_frames(None, 400) == 0 and lib.fa_fbank_num_rows(None, 4) == 0
    assert lib.fa_fbank_plan_create(None, C.byref(cfg), offs.ctypes.data, 1, None, None, 0, C.byref(plan)) == fa.INVALID_ARGUMENT
    assert lib.fa_fbank_execute_dev(None, None, out.ctypes.data, None) == fa.INVALID_ARGUMENT
    assert lib.fa_fbank_batch(None, C.byref(cfg), None, offs.ctypes.data, 1, None, None, 0, out.ctypes.data, None) == fa.INVALID_ARGUMENT
    assert lib.fa_fbank_window(C.byref(cfg), None) == fa.INVALID_ARGUMENT and lib.fa_fbank_filterbank(None, out.ctypes.data) == fa.INVALID_ARGUMENT
    assert lib.fa_fbank_plan_row_stride(None) == 0 and lib.fa_fbank_plan_utt_stride(None) == 0
    # the tables: Hamming ends at 0.08, triangles of neighbouring mels sum to one between the first and the last centre, Nyquist is 0
    w, fb = fa.fbank_window(cfg), fa.fbank_filterbank(cfg)
    assert abs(w[0] - 0.08) < 1e-6 and abs(w[-1] - 0.08) < 1e-6 and w.argmax() in (199, 200)
    assert fb.shape == (80, 257) and np.all(fb[:, 256] == 0) and np.all(fb >= 0)
    centres = fb.argmax(axis=1)
    np.testing.assert_allclose(fb[:, centres[0] + 1:centres[-1]].sum(axis=0), 1.0, atol=1e-6)
