"""logits -> fa_ctc_log_softmax_batch_dev -> fa_ctc_kws_spot_batch_dev without leaving the device (fp32 and fp16 logits): the detections
equal the restatement (tests/kws_restatement.py) run on the log-probabilities downloaded afterwards, score bits and frames.  The constrained
windows read the same device tensor."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kws_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_log_softmax_then_spotting(fa, gpu_ctx, dtype):
    import torch
    B, T, V, blank = 2, 30, 37, 36
    rng = np.random.default_rng(17)
    logits = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    logits[:, :, blank] += 2.0
    terms = [[3], [5, 9], [1, 2, 3, 4], [7, R.WILDCARD, 8], [2, 2], [], list(range(10, 16))]
    d_logits = torch.from_numpy(logits).to(getattr(torch, dtype)).cuda()
    with gpu_ctx.torch_ordered():
        d_lp = fa.ctc_log_probs_dev(gpu_ctx, d_logits, temperature=1.5, blank_bias=0.5, blank_id=blank, order=False)
        dets, counts = fa.spot_keywords_batch(d_lp, terms, min_score=-4.0, blank_id=blank, valid_frames=[T, 21], ctx=gpu_ctx, order=False)
        wins = [(0, 1, 2, 20), (1, 2, 0, 21), (1, 3, 15, 40), (0, 6, 25, 30)]
        con = fa.score_windows(d_lp, terms, wins, blank_id=blank, valid_frames=[T, 21], ctx=gpu_ctx, order=False)
    lp = d_lp.cpu().numpy()
    want = []
    for u, t in enumerate((T, 21)):
        want += [(u, k, R.bits(s), a, b) for k, s, a, b in R.spot_keywords(list(lp[u, :t]), terms, min_score=-4.0, blank_id=blank)]
    assert [(int(d["utterance"]), int(d["keyword"]), R.bits(d["score"]), int(d["start_frame"]), int(d["end_frame"])) for d in dets] == want
    assert len(want) >= 4 and counts.tolist() == [sum(1 for w in want if w[0] == u) for u in range(B)]
    for g, (u, k, a, b) in zip(con, wins):
        s, st, en = R.word_spot_constrained(list(lp[u, :(T, 21)[u]]), terms[k], a, b, blank)
        assert (R.bits(g["score"]), int(g["start_frame"]), int(g["end_frame"])) == (R.bits(s), st, en)
