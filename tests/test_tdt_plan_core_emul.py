"""The integer arithmetic host and device share for the TDT window planner (fluidaudio_amd/csrc/tdt_plan_core.h, the same text the GPU
compiles, and the geometry of tdt_plan_launch.h), built with g++ (tests/cpu/tdt_plan_core.cpp) and walked the way the kernel walks it,
against tests/tdt_plan_restatement.py: the layouts, the fill of the last window, the bound, and every window of every recording of
tests/tdt_plan_cases.py from the restatement's starts.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tdt_plan_cases as K  # noqa: E402
import tdt_plan_restatement as R  # noqa: E402

FIELDS = ("recording", "use_warmup_prefix", "is_last", "emit_after_frame", "global_frame_offset", "context_frames", "actual_audio_frames", "reserved", "chunk_start",
          "warmup_samples", "context_samples", "context_start", "length")


class Config(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("frame_samples", C.c_int32), ("mel_hop", C.c_int32), ("max_model_samples", C.c_int32), ("overlap_seconds", C.c_double),
                ("mel_chunk_context", C.c_int32), ("silence_aligned", C.c_int32), ("warmup_prefix_frames", C.c_int32), ("end_aligned", C.c_int32)]


WINDOW = np.dtype([(f, np.int32) for f in FIELDS[:8]] + [(f, np.int64) for f in FIELDS[8:]])


def abi(cfg: R.Config) -> Config:
    return Config(cfg.sample_rate, cfg.frame_samples, cfg.mel_hop, cfg.max_model_samples, cfg.overlap_seconds, int(cfg.mel_chunk_context), int(cfg.silence_aligned),
                  cfg.warmup_prefix_frames, int(cfg.end_aligned))


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(HERE, "cpu", "libtdt_plan_core.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "cpu", "tdt_plan_core.cpp")], check=True)
    lib = C.CDLL(so)
    lib.tp_emul_layout.argtypes = [C.POINTER(Config), C.c_void_p]
    lib.tp_emul_last_chunk_warmup.argtypes = [C.c_int64] * 6
    lib.tp_emul_last_chunk_warmup.restype = C.c_int64
    lib.tp_emul_bound.argtypes = [C.POINTER(Config), C.c_int64]
    lib.tp_emul_bound.restype = C.c_int64
    lib.tp_emul_walk.argtypes = [C.POINTER(Config), C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    lib.tp_emul_walk.restype = C.c_int64
    return lib


def layout_of(emul, cfg):
    out = np.zeros(10, np.int64)
    return emul.tp_emul_layout(C.byref(abi(cfg)), out.ctypes.data), out.tolist()


def test_layouts_and_refusals(emul):
    geometries = [R.Config(**m) for m in R.MODES.values()] + [R.Config(overlap_seconds=0.0), R.Config(overlap_seconds=9.99), R.Config(overlap_seconds=1000.0),
                                                              R.Config(max_model_samples=20000, mel_chunk_context=False), R.Config(frame_samples=1024, mel_hop=128),
                                                              R.Config(sample_rate=8000, frame_samples=640, mel_hop=80, max_model_samples=120000)]
    for cfg in geometries:
        st, got = layout_of(emul, cfg)
        assert st == 0 and tuple(got[:4]) == R.chunk_layout(cfg)
    assert layout_of(emul, R.Config())[1] == [238080, 206080, 1280, 0, 50, 6, 8000, 3200, 320, 0]
    assert layout_of(emul, R.Config(**R.MODES["path_b"]))[1] == [239360, 207360, 0, 7 * 1280, 50, 6, 8000, 3200, 320, 1]
    for bad in (R.Config(sample_rate=0), R.Config(frame_samples=0), R.Config(mel_hop=0), R.Config(max_model_samples=0), R.Config(warmup_prefix_frames=-1),
                R.Config(overlap_seconds=float("nan")), R.Config(overlap_seconds=float("inf")), R.Config(overlap_seconds=-1.0), R.Config(overlap_seconds=1e9),
                R.Config(max_model_samples=6 * 1280 + 160),          # a chunk of six frames does not exceed the minimal overlap
                R.Config(frame_samples=1000),                       # a silence radius of 64 frames
                R.Config(max_model_samples=1280 * 8, mel_chunk_context=False, warmup_prefix_frames=7)):   # the prefix is as long as the chunk
        assert layout_of(emul, bad)[0] == 1, bad


def test_the_fill_of_the_last_window(emul):
    rng = np.random.default_rng(3)
    chunk = 238080
    for _ in range(4000):
        start = int(rng.integers(0, 3 * chunk))
        total = start + int(rng.integers(-2000, chunk + 5000))
        speech_end = total - int(rng.integers(0, 2)) * int(rng.integers(0, 60)) * 1280 - int(rng.integers(0, 3))
        default = int(rng.integers(0, 3)) * 7 * 640
        assert emul.tp_emul_last_chunk_warmup(start, default, chunk, total, speech_end, 1280) == R.last_chunk_warmup_samples(start, default, chunk, total, speech_end)


@pytest.mark.parametrize("mode", list(R.MODES))
def test_every_window_from_the_restated_starts(emul, mode):
    cfg = R.Config(**R.MODES[mode])
    c = abi(cfg)
    for b, x in enumerate(K.recordings()):
        planner = R.Planner(x, cfg)
        windows, speech_end = planner.plan()
        bound = R.window_count_bound(cfg, x.size)
        assert emul.tp_emul_bound(C.byref(c), x.size) == bound >= len(windows)
        starts = np.array([(s << 1) | int(w) for s, w in planner.chunk_start_decisions()] if x.size else [], np.int64)
        out = np.zeros(bound + 1, WINDOW)
        n = emul.tp_emul_walk(C.byref(c), b, x.size, speech_end, starts.ctypes.data, starts.size, out.ctypes.data, bound)
        assert n == len(windows)
        assert [tuple(int(v) for v in r) for r in out[:n]] == [(b, w["use_warmup_prefix"], w["is_last"], w["emit_after_frame"], w["global_frame_offset"], w["context_frames"],
                                                                w["actual_audio_frames"], 0, w["chunk_start"], w["warmup_samples"], w["context_samples"], w["context_start"],
                                                                w["length"]) for w in windows]
