"""Every `fa_*_dev` entry a wrapper module names, and the two `device_pointers` forms of the clustering stage, has a case in
tests/stream_order_cases.py that races it against a busy torch stream (tests/test_gpu_stream_order.py) — or stands in NOT_YET with its
reason.  A wrapper added without an ordering case fails here, without a GPU."""
import glob
import os
import re

import stream_order_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_POINTER_ENTRIES = {"fa_offline_cluster", "fa_offline_cluster_ex"}
BENCH_DRIVEN = ("pipeline.py", "mel.py", "ctc.py", "tdt.py")        # what bench.py drives: nothing of theirs may wait
NOT_YET_LIMIT = 8


def named_entries():
    """{entry: [modules that name it]} from the wrappers' source"""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "fluidaudio_amd", "*.py"))):
        module = os.path.basename(path)
        if module == "_lib.py":
            continue
        with open(path, encoding="utf-8") as f:
            for name in set(re.findall(r"fa_[a-z0-9_]*_dev\b", f.read())):
                found.setdefault(name, []).append(module)
    for name in DEVICE_POINTER_ENTRIES:
        found.setdefault(name, []).append("pipeline.py")
    return found


def declared_entries():
    with open(os.path.join(ROOT, "include", "fluidaudio_hip.h"), encoding="utf-8") as f:
        return set(re.findall(r"\bfa_[a-z0-9_]+\b", f.read()))


def test_every_named_entry_has_a_case_or_a_reason():
    named = named_entries()
    assert len(named) >= 59, sorted(named)
    covered = {e for c in K.CASES for e in c.entries}
    missing = sorted(set(named) - covered - set(K.NOT_YET))
    assert not missing, f"no ordering case and no NOT_YET reason for {missing}"


def test_not_yet_is_short_and_spares_the_benchmarked_paths():
    named = named_entries()
    assert len(K.NOT_YET) <= NOT_YET_LIMIT, sorted(K.NOT_YET)
    assert all(isinstance(r, str) and r.strip() for r in K.NOT_YET.values()), "every entry left out says why"
    assert set(K.NOT_YET) <= set(named), sorted(set(K.NOT_YET) - set(named))
    spared = sorted(e for e in K.NOT_YET if any(m in BENCH_DRIVEN for m in named[e]))
    assert not spared, f"{spared} belong to {BENCH_DRIVEN}"
    assert not set(K.NOT_YET) & {e for c in K.CASES for e in c.entries}, "an entry with a case needs no reason"


def test_no_case_names_an_entry_that_does_not_exist():
    declared, named = declared_entries(), named_entries()
    for c in K.CASES:
        assert c.entries, c.name
        unknown = [e for e in c.entries if e not in declared or (e not in named and e != "fa_online_chunk_plan")]
        assert not unknown, f"{c.name}: {unknown}"
    names = [c.name for c in K.CASES]
    assert len(set(names)) == len(names)


def test_the_controls_are_the_two_wrappers_with_a_switch():
    assert sorted(c.entries for c in K.CASES if c.control) == [("fa_ctc_log_softmax_batch_dev",), ("fa_mel_execute_dev",)]
