"""fa_tdt_merge_windows(_dev) and ChunkProcessor of include/fluidaudio.hpp from a C++ host built with g++ -Werror
(tests/cabi/tdt_merge.cpp): the build and the argument contract on the CPU tier — every error is decided before any device work and
nothing is written —, two of the reference's literal cases on the GPU tier."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def host(fa, tmp_path_factory):
    fa.lib()
    lib = fa._lib.LIB_PATH
    exe = str(tmp_path_factory.mktemp("cabi") / "tdt_merge_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cabi", "tdt_merge.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def test_argument_errors_without_a_device(host):
    r = subprocess.run([host, "args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [l.split() for l in r.stdout.splitlines()]
    assert [l[1:] for l in out if l[0] == "CFG"] == [["1", "1"]]
    # INVALID_ARGUMENT for every bad argument — and for the good ones, which reach the missing context; INDEX_OVERFLOW for a slice
    # of 2^31 tokens and for 2^31 - 1 recordings; nothing thrown across the ABI, nothing written
    assert [l[1:] for l in out if l[0] == "ST"] == [["1"] * 3, ["1"] * 13, ["1"] * 3, ["2"] * 2]
    assert [l[1:] for l in out if l[0] == "OUT"] == [["1"]]
    assert [l[1:] for l in out if l[0] == "THROWN"] == [["1"]]


def test_python_wrapper_contract_needs_no_device(fa):
    import numpy as np
    z = np.zeros((2, 3), np.int32)
    zf = np.zeros((2, 3), np.float32)
    for bad in ([0, 3], [2, 0], [-1, 2]):
        with pytest.raises(fa.FluidAudioHipError) as e:
            fa.merge_windows(z, z, z, zf, [1, 1], bad)
        assert e.value.status == fa.INVALID_ARGUMENT
    with pytest.raises(fa.FluidAudioHipError):
        fa.merge_windows(z, z, z[:1], zf, [1, 1], [0, 2])
    with pytest.raises(fa.FluidAudioHipError):
        fa.merge_windows(z, z, z, zf, [1, 1], [0, 2], splice_safe=np.zeros(3, np.uint8), case_canon=np.zeros(4, np.int32))
    # zero recordings: answered without a context
    m = fa.merge_windows(z, z, z, zf, [1, 1], [0])
    assert m.counts.size == 0 and m.tokens.size == 0 and m.routes.tolist() == [fa.MERGE_NO_SEAM] * 2
    assert fa.merge_capacity([3, 2, 0, 4, 1], [0, 2, 2, 5]).tolist() == [3 + 4, 0, 0 + 8 + 2]
    assert fa.splice_safe_table(None, 4) is None and fa.splice_safe_table({1, 9}, 4).tolist() == [0, 1, 0, 0]
    assert fa.case_canon_table({2: 1, 1: 1}, 4).tolist() == [-1, 1, 1, -1]
    assert [fa.merge_route_name(c) for c in (-1, 1, 2 | 16, 3 | 32, 4)] == ["none", "concat", "contiguous+adopt-right", "lcs+keep-left", "midpoint"]


@pytest.mark.gpu
def test_two_pinned_cases_on_the_device(host):
    r = subprocess.run([host, "merge"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines()}
    assert out["ADOPT"] == ["0", "10@120", "27@130", "25@131", "28@132", "30@134", "|", "-1", str(3 | 16)]   # the LCS route, right's word adopted
    assert out["MIDPOINT"] == ["0", "10@120", "20@133", "50@136", "30@138", "|", "-1", "4"]
    assert out["NONE"] == ["0", "|"]
    assert out["ONE"] == ["0", "10@120", "20@133", "21@135", "|", "-1"]
