"""Which kernel serves a CTC / TDT decoder call, and the contract of the CTC rows entries (csrc/ctc_route.h, csrc/tdt_route.h: the plain
C++ part of ctc_launch.h / tdt_launch.h) walked on the CPU by tests/cpu/decoder_routes.cpp against the conditions restated here.  The
program is stand-alone, reads its cases from stdin and is built with the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = 0x7F0000000000          # a 16-byte aligned device pointer


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decoder_routes") / "decoder_routes")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpu", "decoder_routes.cpp"), "-o", exe], check=True)
    return exe


def run(routes, lines):
    r = subprocess.run([routes], input="".join(" ".join(str(int(w) if isinstance(w, bool) else w) for w in ln) + "\n" for ln in lines),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


# ---- the conditions, restated

def tdt_route(f16, v1, row_stride, ptr):
    """0: the streaming kernel; 1: the row stays in registers (at most 17 x 64 logits), one logit per request; 2: the same for fp16 rows that
    all start on a 4-byte boundary, read as pairs."""
    if v1 > 64 * 17:
        return 0
    return 2 if f16 and (2 * row_stride) % 4 == 0 and ptr % 4 == 0 else 1


def greedy_mode(f16, vocab, row_stride, matrix_stride, ptr):
    """0: 16-byte aligned rows of whole vectors; 1: element-aligned matrices whose rows hold two vectors or more; 2: scalar loads."""
    vw, esz = (8, 2) if f16 else (4, 4)
    if vocab % vw == 0 and row_stride % vw == 0 and matrix_stride % vw == 0 and ptr % 16 == 0:
        return 0
    return 1 if ptr % esz == 0 and vocab >= 2 * vw else 2


def lsm_vec4(f16, vocab, row_stride, matrix_stride, ptr, out):
    return (not f16) and vocab % 4 == 0 and vocab <= 2048 and row_stride % 4 == 0 and matrix_stride % 4 == 0 and ptr % 16 == 0 and out % 16 == 0


def rows_contract(batch, total_rows, utt, off, has_tok):
    if batch < 0 or total_rows < 0:
        return "ctc rows: bad shape"
    if batch == 0:
        return "ok"
    if utt is None and batch != 1:
        return "ctc rows: a batch needs utt_rows"
    if total_rows > 0 and (off is None or not has_tok):
        return "ctc rows: null buffer"
    if total_rows > 0:
        if off[0] < 0:
            return "ctc rows: negative offset"
        if any(off[r + 1] < off[r] for r in range(total_rows)):
            return "ctc rows: row_offsets decrease"
    if utt is not None:
        if utt[0] < 0 or utt[batch] > total_rows:
            return "ctc rows: utt_rows out of range"
        if any(utt[u + 1] < utt[u] for u in range(batch)):
            return "ctc rows: utt_rows decrease"
    return "ok"


# ---- the cases

def test_tdt_logits_route(routes):
    cases = [(f16, v1, v1 + 5 + pad, BASE + off)
             for f16 in (False, True) for v1 in (1, 8, 9, 1025, 1087, 1088, 1089, 8193)
             for pad in (0, 1)                                  # fp16: an even and an odd row stride for every vocabulary
             for off in (0, 2, 4)]                              # off 4-byte alignment (fp16 only can be: an fp32 pointer is 4-byte aligned)
    got = run(routes, [("tdt",) + c for c in cases])
    assert all(g.split()[1:] == ["limit", "1088"] for g in got)            # the limit the kernel's requests are sized by (kFitsPieces)
    assert [int(g.split()[0]) for g in got] == [tdt_route(*c) for c in cases]
    route = {c: int(g.split()[0]) for c, g in zip(cases, got)}
    assert route[(True, 1087, 1092, BASE)] == 2 and route[(True, 1088, 1093, BASE)] == 1 and route[(True, 1088, 1094, BASE)] == 2
    assert route[(True, 1088, 1094, BASE + 2)] == 1                          # a pointer off 4-byte alignment: no pairs
    assert route[(True, 1089, 1094, BASE)] == 0 and route[(False, 1089, 1094, BASE)] == 0 and route[(False, 1088, 1093, BASE)] == 1
    assert route[(True, 8, 13, BASE)] == 1 and route[(True, 9, 14, BASE)] == 2 and route[(False, 8, 13, BASE)] == 1


def test_ctc_greedy_mode(routes):
    cases = []
    for f16 in (False, True):
        for vocab in (1, 3, 4, 7, 8, 15, 16, 1024, 1025, 1028):           # multiples of the vector width and not; below two vectors (fp32 8, fp16 16)
            for row_pad in (0, 1, 2, 4, 8):                                 # strides that keep and that break the 16-byte alignment of a row
                for mat_pad in (0, 4, 6):
                    for off in (0, 1, 2, 4, 8, 16):                         # a pointer off 16-byte and off element alignment
                        cases.append((f16, vocab, vocab + row_pad, 10 * (vocab + row_pad) + mat_pad, BASE + off))
    got = [int(g) for g in run(routes, [("greedy",) + c for c in cases])]
    assert got == [greedy_mode(*c) for c in cases]
    mode = dict(zip(cases, got))
    assert mode[(False, 1024, 1024, 10240, BASE)] == 0 and mode[(False, 1025, 1025, 10250, BASE)] == 1
    assert mode[(True, 8, 8, 80, BASE)] == 0 and mode[(True, 4, 4, 40, BASE)] == 2          # fp16: 8 is one vector; 4 is below one
    assert mode[(True, 1028, 1028, 10280, BASE)] == 1                                         # a multiple of 4, not of 8
    assert mode[(False, 1024, 1025, 10250, BASE)] == 1 and mode[(False, 1024, 1024, 10244, BASE)] == 0 and mode[(False, 1024, 1024, 10246, BASE)] == 1
    assert mode[(False, 1024, 1024, 10240, BASE + 8)] == 1 and mode[(False, 1024, 1024, 10240, BASE + 2)] == 2
    assert mode[(True, 1024, 1024, 10240, BASE + 2)] == 1 and mode[(True, 1024, 1024, 10240, BASE + 1)] == 2
    assert mode[(False, 7, 7, 70, BASE)] == 2 and mode[(False, 8, 9, 90, BASE)] == 1 and mode[(True, 15, 15, 150, BASE)] == 2
    assert set(got) == {0, 1, 2}


def test_log_softmax_vec4(routes):
    cases = [(f16, vocab, vocab + row_pad, 7 * (vocab + row_pad) + mat_pad, BASE + off, BASE + 4096 + out_off)
             for f16 in (False, True) for vocab in (4, 1022, 1024, 1025, 2048, 2050, 2052) for row_pad in (0, 2, 4) for mat_pad in (0, 2, 4)
             for off in (0, 4, 16) for out_off in (0, 4, 8, 16)]
    got = [bool(int(g)) for g in run(routes, [("lsm",) + c for c in cases])]
    assert got == [lsm_vec4(*c) for c in cases]
    vec4 = dict(zip(cases, got))
    assert vec4[(False, 2048, 2048, 7 * 2048, BASE, BASE + 4096)] and not vec4[(False, 2052, 2052, 7 * 2052, BASE, BASE + 4096)]
    assert not vec4[(False, 1022, 1022, 7 * 1022, BASE, BASE + 4096)] and not vec4[(False, 1025, 1025, 7 * 1025, BASE, BASE + 4096)]
    assert not vec4[(False, 1024, 1024, 7 * 1024, BASE, BASE + 4096 + 8)] and not vec4[(True, 1024, 1024, 7 * 1024, BASE, BASE + 4096)]
    assert any(got)


ROWS = {                                  # batch, total_rows, utt_rows, row_offsets, token_ids given
    "plain": (2, 4, [0, 1, 4], [0, 3, 3, 9, 12], True),
    "one_utterance_without_utt_rows": (1, 3, None, [0, 2, 4, 6], True),
    "no_rows": (1, 0, None, None, False),
    "empty_batch_needs_nothing": (0, 5, None, None, False),
    "negative_batch": (-1, 4, None, [0, 1, 2, 3, 4], True),
    "negative_rows": (1, -1, None, None, True),
    "batch_without_utt_rows": (2, 4, None, [0, 3, 3, 9, 12], True),
    "no_offsets": (1, 2, None, None, True),
    "no_token_ids": (1, 2, None, [0, 1, 2], False),
    "negative_first_offset": (1, 2, None, [-1, 1, 2], True),
    "decreasing_pair": (1, 3, None, [0, 5, 4, 6], True),
    "decreasing_last_pair": (1, 3, None, [0, 5, 6, 5], True),
    "utt_rows_beyond_total": (2, 4, [0, 2, 5], [0, 3, 3, 9, 12], True),
    "utt_rows_negative": (2, 4, [-1, 2, 4], [0, 3, 3, 9, 12], True),
    "utt_rows_decrease": (3, 4, [0, 3, 2, 4], [0, 3, 3, 9, 12], True),
    "utt_rows_over_no_rows": (2, 0, [0, 0, 0], None, False),
}


def test_rows_contract(routes):
    names = sorted(ROWS)
    lines = []
    for n in names:
        batch, total, utt, off, has_tok = ROWS[n]
        lines.append(("rows", batch, total, utt is not None, off is not None, has_tok, len(off or []), *(off or []), len(utt or []), *(utt or [])))
    got = dict(zip(names, run(routes, lines)))
    assert got == {n: rows_contract(ROWS[n][0], ROWS[n][1], ROWS[n][2], ROWS[n][3], ROWS[n][4]) for n in names}
    assert got["plain"] == got["one_utterance_without_utt_rows"] == got["no_rows"] == got["empty_batch_needs_nothing"] == got["utt_rows_over_no_rows"] == "ok"
    assert got["negative_first_offset"] == "ctc rows: negative offset" and got["decreasing_pair"] == got["decreasing_last_pair"] == "ctc rows: row_offsets decrease"
    assert got["utt_rows_beyond_total"] == got["utt_rows_negative"] == "ctc rows: utt_rows out of range" and got["utt_rows_decrease"] == "ctc rows: utt_rows decrease"
    assert got["batch_without_utt_rows"] == "ctc rows: a batch needs utt_rows" and got["no_offsets"] == got["no_token_ids"] == "ctc rows: null buffer"
    assert got["negative_batch"] == got["negative_rows"] == "ctc rows: bad shape"
