"""The AED unit without a GPU: the restatement (tests/aed_restatement.py) against the reference's own known answers (every
mergeTokenStreams case of CohereLongFormTests and CanaryChunkMergeTests, the mask cases of CoherePipelineMaskTests, the presets'
numbers), the proof that the shared cases (tests/aed_cases.py) hold every kind of decision, and csrc/aed_core.h / csrc/aed_launch.h
walked by a stand-alone program (tests/cpu/aed_core_main.cpp) built with the address and undefined-behaviour sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aed_cases as K  # noqa: E402
import aed_restatement as R  # noqa: E402

OK, INVALID, OVERFLOW, TOO_SMALL = 0, 1, 2, 3


# ---- the restatement against the reference's literal tests
@pytest.mark.parametrize("case", K.MERGE_LITERAL, ids=lambda c: c[0])
def test_merge_restatement_reproduces_the_reference_tests(case):
    _, windows, wt, mm, want = case
    assert R.merge_token_streams(windows[0], windows[1], wt, mm) == want


def test_mask_restatement_reproduces_the_reference_tests():
    L = R.COHERE["max_seq"]
    assert L == 108
    for f16, zero, dt in ((False, 0.0, np.float32), (True, 0, np.uint16)):
        assert R.dynamic_self_mask(4, f16).tolist() == [zero] * 5 and R.dynamic_self_mask(7, f16).dtype == dt and R.dynamic_self_mask(0, f16).shape == (1,)
    m = R.self_mask_row(10, L, False)                                            # testStaticMaskCausalSplitFloat32
    assert m.shape == (L,) and m.dtype == np.float32 and (m[:11] == 0).all() and (m[11:] == np.float32(-1.0e4)).all()
    h = R.self_mask_row(5, L, True)                                              # testStaticMaskCausalSplitFloat16
    assert (h[:6] == 0).all() and h[6] != 0 and h[6] & 0x8000 and (h[6:] == h[6]).all()
    assert h[6] == np.float32(-1.0e4).astype(np.float16).view(np.uint16) == 0xF0E2
    assert (R.self_mask_row(L - 1, L, False) == 0).all()                         # testStaticMaskAtFinalStepHasNoBlockedPositions
    z = R.self_mask_row(0, L, False)                                             # testStaticMaskAtStepZeroBlocksAllExceptFirst
    assert z[0] == 0 and (z[1:] == np.float32(-1.0e4)).all()
    assert R.cross_mask(6, 4, False).tolist() == [0, 0, 0, 0, -1.0e4, -1.0e4] and R.cross_mask(3, 9, True).tolist() == [0, 0, 0]
    assert R.cross_mask(3, -2, True).tolist() == [0xF0E2] * 3


def test_presets_and_window_plans():
    assert (R.COHERE["chunk_samples"], R.COHERE["hop_samples"]) == (35 * 16000, 30 * 16000)      # maxAudioSeconds 35, chunkHopSeconds 30
    assert (R.CANARY["chunk_samples"], R.CANARY["chunk_samples"] - R.CANARY["hop_samples"]) == (240_000, 48_000)   # chunkOverlapSamples
    for chunk, hop, samples, want in K.WINDOW_PLANS:
        assert R.plan_windows(samples, chunk, hop) == want
    assert [R.encoder_valid_frames(f, 438) for f in (0, 1, 8, 3499, 3500, 9000)] == [1, 1, 2, 438, 438, 438]
    assert R.encoder_valid_frames(3500, 400) == 400 and R.encoder_valid_frames(1000, 438) == 126                 # ceil(125.14)
    assert R.context_mask(0, 4).tolist() == [1, 0, 0, 0] and R.context_mask(9, 4).tolist() == [1, 1, 1, 1] and R.context_mask(2, 4).tolist() == [1, 1, 0, 0]


# ---- the shared cases hold every kind of decision
@pytest.fixture(scope="module")
def replayed():
    out = []
    for case in K.scripted_cases() + K.random_cases():
        feeds, kinds, discarded = [], [], []
        for feeds, kinds, discarded in K.replay(case):
            pass
        if not len(case["rows"]):
            feeds = [(R.SequenceFeed if case["cfg"]["mode"] == 1 else R.TokenFeed)(p, case["cfg"]) for p in case["prompts"]]
        out.append((case, feeds, kinds, discarded))
    return out


def test_decode_cases_hold_every_decision_kind(replayed):
    kinds = [k for _, _, ks, _ in replayed for k in ks]
    flips = [k for k in kinds if k["plain"] != k["after_penalty"]]
    assert any(k["raw"][k["plain"]] > 0 for k in flips) and any(k["raw"][k["plain"]] < 0 for k in flips)          # the penalty changes the winner, both signs
    assert any(k["after_penalty"] != k["final"] and k["after_penalty"] in k["banned"] for k in kinds)             # a ban changes the winner
    assert any(k["banned"] & k["penalised"] for k in kinds)                                                        # a banned id that is also penalised
    assert {k["n"] for k in kinds} >= {0, 1, 2, 3, 4}
    for n in (1, 2, 3, 4):
        assert any(k["n"] == n and k["banned"] for k in kinds), n
    assert any(k["n"] >= 2 and 0 < k["history"] + 1 < k["n"] for k in kinds) and any(k["n"] == 4 and k["history"] == 1 for k in kinds)   # a history shorter than n - 1

    def tied(k):   # the maximum is held by a penalised id AND by an untouched one
        top = k["values"][k["final"]]
        holders = {int(i) for i in np.flatnonzero(k["values"] == top)}
        return len(holders) > 1 and holders & k["penalised"] and holders - k["penalised"] and k["final"] == min(holders), (k["final"] in k["penalised"])
    ties = [tied(k) for k in kinds]
    assert any(t and pen for t, pen in ties) and any(t and not pen for t, pen in ties)                             # the tie goes to the lower index, either way round
    cases = {c["name"]: (c, feeds, ks, disc) for c, feeds, ks, disc in replayed}
    assert any(tok == c["cfg"]["eos_id"] for c, _, _, disc in replayed for _, _, tok in disc)                      # a discarded decision that would have been EOS
    c, feeds, _, _ = cases["n3"]
    assert [len(p) for p in c["prompts"]] == [3, 1, 2]                                                             # P = 1; different prompt lengths in one batch
    assert feeds[1].reason == R.EOS and feeds[1].output_tokens == [] and feeds[1].step_index == 0                  # EOS at the first output step
    assert feeds[0].reason == R.CAP and feeds[0].step_index == 16 == c["cfg"]["max_seq"] < c["cfg"]["max_new"] + 3  # max_seq binds
    c, feeds, _, _ = cases["n2"]
    assert all(f.reason == R.CAP and len(f.output_tokens) == c["cfg"]["max_new"] + 1 for f in feeds)              # max_new binds: max_new + 1 outputs
    assert all(f.step_index == c["cfg"]["max_new"] + len(p) < c["cfg"]["max_seq"] for f, p in zip(feeds, c["prompts"]))
    c, feeds, ks, _ = cases["outside"]
    assert all(not (k["banned"] | k["penalised"]) - set(range(c["cfg"]["vocab"])) for k in ks) and 9 in feeds[0].all_tokens and -1 in feeds[0].all_tokens
    c, feeds, _, _ = cases["seq"]
    assert feeds[0].generated[:3] == [0, 5, 2] and [f.reason for f in feeds] == [R.EOS, R.CAP, R.CAP, R.CAP] and feeds[2].generated == [] and feeds[3].pos == 12
    for c, feeds, _, _ in replayed:                                                                                # utterances end at different steps
        if len(feeds) > 2 and c["name"].startswith(("tok-", "seq-")):
            assert len({(f.reason, len(f.output_tokens)) for f in feeds}) > 1, c["name"]
    big = [k for k in kinds if k["raw"].size >= 1025]
    assert any(k["plain"] != k["after_penalty"] for k in big) and any(k["banned"] for k in big)                    # the large rows meet penalties and bans too


def test_merge_cases_hold_every_seam_kind():
    own = {name: (windows, wt, mm) for name, windows, wt, mm, _ in K.MERGE_OWN}
    windows, wt, mm = own["run-twice"]
    merged, bl, be = R.merge_token_streams(windows[0], windows[1], wt, mm, detail=True)
    assert (bl, be) == (4, 4) and windows[1][5:9] == windows[1][0:4] and merged == windows[0] + windows[1][4:]   # the first of two equal runs wins
    windows, wt, mm = own["run-twice-rows"]
    assert R.merge_token_streams(windows[0], windows[1], wt, mm, detail=True)[1:] == (4, 4)
    assert R.merge_token_streams(*own["exactly-min-match"][0], 32, 4, detail=True)[1] == 4 and R.merge_token_streams(*own["below-min-match"][0], 32, 4, detail=True)[1] == 3
    windows, wt, mm = own["prefix-longer-than-window"]
    assert len(windows[0]) > wt and R.merge_token_streams(windows[0], windows[1], wt, mm) == windows[0] + [6]
    windows, wt, mm = own["run-outside-window"]
    assert R.merge_token_streams(windows[0], windows[1], wt, mm) == windows[0] + windows[1]                       # the run lies before the last 7 tokens
    windows, wt, mm = own["empty-window-in-the-middle"]
    assert [] in windows[1:-1] and R.merge_recording(windows, wt, mm)[0] == [1, 2, 3, 4, 5, 6]
    assert R.merge_recording(own["three-windows"][0])[0] == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert R.merge_recording(own["window-of-one"][0], 1, 1) == ([1, 2, 3, 4], [(0, 0), (1, 1)])
    assert R.merge_recording(own["window-of-64"][0], 64, 4)[0] == list(range(100))


# ---- the shared headers on the CPU, under the sanitizers
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("aed_core") / "aed_core")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "aed_core_main.cpp"), "-o", exe], check=True)

    def ask(*lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [l.split()[1:] for l in r.stdout.strip().splitlines()]
    return ask


def test_core_window_plan(core):
    rng = np.random.default_rng(5)
    asks = [(c, h, s) for c, h, s, _ in K.WINDOW_PLANS]
    for _ in range(300):
        chunk = int(rng.integers(1, 60))
        hop = int(rng.integers(1, chunk + 1))
        asks.append((chunk, hop, int(rng.integers(0, 400))))
    asks += [(7, 7, 21), (7, 7, 22), (7, 1, 30), (1, 1, 5), (240_000, 192_000, 16_000 * 3600)]
    got = core(*[f"windows {c} {h} {s}" for c, h, s in asks])
    for (c, h, s), line in zip(asks, got):
        want = R.plan_windows(s, c, h)
        vals = [int(x) for x in line]
        assert vals[0] == vals[1] == len(want) and list(zip(vals[2::2], vals[3::2])) == want, (c, h, s)


def test_core_valid_frames_layout_and_plans(core):
    asks = [(f, s, m, e) for f in (0, 1, 7, 8, 9, 3499, 3500, 3501, 10**6) for s, m, e in ((438, 3500, 438), (100, 3500, 438), (1, 7, 3), (50, 1501, 188))]
    got = core(*[f"valid {f} {s} {m} {e}" for f, s, m, e in asks])
    assert [int(g[0]) for g in got] == [R.encoder_valid_frames(*a) for a in asks]
    # the state: 8 header words, the history, the prompt, the output tokens; max_out = min(max_new + 1, max_seq) / max_seq
    assert core("layout 0 16384 108 108", "layout 0 16 24 4", "layout 1 16384 128 0", "layout 0 5 12 11") == [
        ["108", "332", "8", "116", "224", "8"], ["5", "61", "8", "32", "56", "8"], ["128", "392", "8", "136", "264", "8"], ["12", "44", "8", "20", "32", "8"]]
    # the last step min(max_new + P, max_seq) - 1 and the first deciding step P - 1
    assert core("last 108 10 108 8", "last 4 2 16 1", "last 0 1 16 0", "last 2147483647 5 24 4", "last 4 3 16 1") == [["107", "0"], ["5", "1"], ["0", "1"], ["23", "1"], ["6", "0"]]
    # one workgroup per utterance; LDS = the history and the banned tokens (max_seq rounded up to 4, each) + one bit per id, none where no id of the row can change
    assert core("stepplan 0 16384 108 3 1.1 67", "stepplan 0 16384 108 0 1.0 1", "stepplan 1 16384 128 3 1.1 5", "stepplan 0 130 12 0 1.5 2", "stepplan 0 33 12 1 1.0 2") == [
        ["67", "256", str(8 * 108 + 2048), "1", "4", "512", "67", "256"], ["1", "256", "0", "0", "4", "512", "1", "256"], ["5", "256", "0", "0", "4", "512", "5", "256"],
        ["2", "256", str(96 + 20), "1", "1", "5", "2", "256"], ["2", "256", str(96 + 8), "1", "1", "2", "2", "256"]]
    assert core("defaults") == [["0", "16384", "3", "108", "108", "3", "1.1", "32", "4", "560000", "480000", "108"],
                                ["1", "16384", "3", "128", "128", "0", "1", "32", "4", "240000", "192000", "128"]]


def test_core_refusals(core):
    labels = ["config", "begin", "step", "finish", "strided", "windows", "overflow", "merge"]                     # the order the program prints them in
    got = dict(zip(labels, ([int(x) for x in line] for line in core("refusals"))))
    assert got["config"] == [INVALID, OK, OK] + [INVALID] * 7 + [OK]
    assert got["begin"] == [OK] + [INVALID] * 12 + [OK, INVALID]                                                   # P < 1, P beyond the stride, P beyond max_seq among them
    assert got["step"] == [OK] + [INVALID] * 7 + [OK, INVALID]
    assert got["finish"] == [OK, TOO_SMALL] + [INVALID] * 4
    assert got["strided"] == [OK] + [INVALID] * 5
    assert got["windows"] == [OK] + [INVALID] * 10 + [OK]
    assert got["overflow"] == [OVERFLOW]
    assert got["merge"] == [OK, OK, OK, INVALID, INVALID, INVALID, OK, INVALID, INVALID, INVALID, INVALID, TOO_SMALL, INVALID, INVALID]
