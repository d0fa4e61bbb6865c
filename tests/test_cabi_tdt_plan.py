"""The TDT window-planner entries and their Swift-shaped mirror in include/fluidaudio.hpp from a C++ host built with g++ -Werror
(tests/cabi/tdt_plan.cpp): the struct layouts as the compiler and as ctypes / numpy see them, the defaults, the layouts and the bound,
and every refusal answered without a device.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def f64hex(x):
    return f"{struct.unpack('<Q', struct.pack('<d', x))[0]:016x}"


@pytest.fixture(scope="module")
def out(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "tdt_plan_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cabi", "tdt_plan.cpp"), "-o", exe, lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return [l.split() for l in r.stdout.splitlines()]


def rows(out, tag):
    return [l[1:] for l in out if l[0] == tag]


def test_struct_layouts(fa, out):
    L = fa._lib
    layouts = {l[0]: [int(x) for x in l[1:]] for l in rows(out, "LAYOUT")}
    for name, record, dtype, want in (("config", L.TdtWindowConfig, None, [40, 0, 4, 8, 12, 16, 24, 28, 32, 36]),
                                      ("window", L.TdtWindowRecord, fa.TDT_WINDOW_DTYPE, [72, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64]),
                                      ("span", L.TdtSpanRecord, fa.TDT_SPAN_DTYPE, [24, 0, 8, 16])):
        fields = [f for f, _ in record._fields_ if not (name == "span" and f == "reserved")]
        assert layouts[name] == want == [C.sizeof(record)] + [getattr(record, f).offset for f in fields]
        if dtype is not None:
            assert dtype.itemsize == C.sizeof(record) and all(dtype.fields[f][1] == getattr(record, f).offset for f, _ in record._fields_)


def test_defaults_layouts_and_the_bound(fa, out):
    default = ["16000", "1280", "160", "240000", f64hex(2.0), "1", "0", "0", "1"]              # ASRConstants.swift:6-31, ChunkProcessor.swift:28
    assert rows(out, "CFG") == [default, default, ["16000", "1280", "160", "240000", f64hex(2.0), "0", "1", "7", "1"]]
    cfg = fa.tdt_window_config()
    assert [str(cfg.sample_rate), str(cfg.frame_samples), str(cfg.mel_hop), str(cfg.max_model_samples), f64hex(cfg.overlap_seconds), str(cfg.mel_chunk_context),
            str(cfg.silence_aligned), str(cfg.warmup_prefix_frames), str(cfg.end_aligned)] == default
    assert rows(out, "CHUNKS") == [["238080", "206080", "1280", "0"], ["239360", "207360", "0", "8960"]]
    assert fa.tdt_window_layout() == (238080, 206080, 1280, 0) and fa.tdt_window_layout(fa.tdt_window_config(False, True)) == (239360, 207360, 0, 0)
    # regular starts: one window per started stride; aligned starts: as many again, less one, for the steps beyond the list
    assert rows(out, "BOUND") == [["0", "0", "1", "1", "2", "1", "3", "-1"]]


def test_every_refusal_is_answered_without_a_device(out):
    INVALID, OVERFLOW, TOO_SMALL = "1", "2", "3"
    assert rows(out, "ST") == [["config"] + [INVALID] * 12,
                               ["plan"] + [INVALID] * 8 + [OVERFLOW],
                               ["pack"] + [INVALID] * 10 + [TOO_SMALL],
                               ["gate"] + [INVALID] * 10]
    assert rows(out, "RANGE") == [["-7", "-7", "-7"]] and rows(out, "THR") == [["-7"]]        # a refusal writes nothing
    assert rows(out, "THROW") == [["1"]]
