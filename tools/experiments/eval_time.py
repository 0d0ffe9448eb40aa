"""Caption-set evaluation timing on one GPU at validation size: 5 000 images x 20 captions x 5 references of 8-16 words (vocabulary
10 000; a caption is one of its image's references with 30 % of the words replaced, so n-grams of every order match somewhere).  Host
clock around synchronised calls, median of --reps after warm-up: the evaluator's build (once), a whole evaluate(), and its parts -- the
hypothesis count table, the three vc_ngram_overlap launches (against the references, the earlier captions, the other captions), the
vc_lcs_overlap launch of ROUGE-L (against the references: the pairs of the first overlap launch), evaluate() with that launch left out
(alternating with the whole one, call by call), the CIDEr-D path (idf vectors of the captions + vc_consensus_score) with its scoring launch alone, which visits the same (caption,
reference) pairs as the first overlap launch.  host_ms = evaluate - the device parts (word rows, uploads, the copy-back, the float64
reductions, the distinct / novel look-ups).  Next to them the plain-Python reference (tests/eval_ref.py, tests/rouge_ref.py) on --ref-images images, scaled to
all of them; the evaluator's numbers on that slice are compared with the reference's.  One JSON line.
    python tools/experiments/eval_time.py [--images 5000] [--reps 7] [--ref-images 200]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_captioning_amd import abi  # noqa: E402
from vae_captioning_amd import evaluate as ev  # noqa: E402
from vae_captioning_amd.consensus import upload, word_rows  # noqa: E402

BOS, EOS = 1, 2


def data(rng, B, K, R, V):
    lens = rng.integers(8, 17, size=B * R)
    refs, cands = [], []
    for b in range(B):
        rs = [rng.integers(3, V, size=int(n)) for n in lens[b * R:(b + 1) * R]]
        refs.append([[BOS] + r.tolist() + [EOS] for r in rs])
        cs = []
        for _ in range(K):
            c = rs[int(rng.integers(R))]
            cs.append(np.where(rng.random(c.size) < 0.3, rng.integers(3, V, size=c.size), c).tolist() + [EOS])
        cands.append(cs)
    return cands, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-images", type=int, default=200)
    a = ap.parse_args()
    lib = abi.load()
    B, K, R, V = a.images, 20, 5, 10000
    cands, refs = data(np.random.default_rng(0), B, K, R, V)
    train = [r for rs in refs[:B // 2] for r in rs]

    def clock(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts)) * 1e3, out

    build_ms, e = clock(lambda: ev.CaptionEvaluator(lib, refs, BOS, EOS, vocab_size=V, train_captions=train), 1)
    for _ in range(2):
        e.evaluate(cands)
    eval_ms, res = clock(lambda: e.evaluate(cands), a.reps)
    # the same call without the ROUGE-L launch (what evaluate() did before it had one), alternating with the whole call
    real_lcs, with_ts, without_ts = ev._launch_lcs, [], []
    for _ in range(a.reps):
        with_ts.append(clock(lambda: e.evaluate(cands), 1)[0])
        ev._launch_lcs = lambda *args: None
        try:
            without_ts.append(clock(lambda: e.evaluate(cands), 1)[0])
        finally:
            ev._launch_lcs = real_lcs
    # the parts, on the arrays evaluate() builds
    flat = [c for cs in cands for c in cs]
    rows_ms, (W, L) = clock(lambda: word_rows(flat, BOS, EOS), 3)
    C = len(flat)
    table_ms, hyp = clock(lambda: ev.count_vectors(lib, e.dev, W, L, BOS, EOS), a.reps)
    img = np.repeat(np.arange(B), K)
    ci = np.arange(0, C + 1, K)
    rows, none = np.arange(C), np.full(C, -1)
    forms = dict(references=(e.ref_off[img], e.ref_off[img + 1], none, e.ref_counts), earlier=(ci[img], rows, none, hyp),
                 others=(ci[img], ci[img + 1], rows, hyp))
    out = torch.empty(ev.OUT_COLS * C, dtype=torch.int32, device=e.dev)
    part = {}
    for name, (lo, hi, skip, table) in forms.items():
        rng_dev = upload(e.dev, np.stack([lo, hi, skip]).astype(np.int32))
        part[name], _ = clock(lambda: ev._launch(lib, hyp, table, rng_dev, out), a.reps)
    rng_dev = upload(e.dev, np.stack(forms["references"][:3]).astype(np.int32))
    lcs_out = torch.empty(ev.LCS_COLS * C, dtype=torch.int32, device=e.dev)
    lcs_ms, _ = clock(lambda: ev._launch_lcs(lib, hyp, e.ref_counts, rng_dev, lcs_out), a.reps)
    cider_ms, _ = clock(lambda: e._cider(W, L, ci, K), a.reps)
    cv, rv, P = e._idf_vectors(W, L, head=ci), e.ref_idf, abi.ptr
    sc = torch.empty(C, dtype=torch.float64, device=e.dev)

    def score():
        lib.vc_consensus_score(torch.cuda.current_stream().cuda_stream, B, 1, P(rv.head[B + 1:]), P(rv.head[:B + 1]), P(rv.off), P(rv.nnz),
                               P(rv.keys), P(rv.w), P(rv.norm), P(rv.words), P(cv.head), K, P(cv.off), P(cv.nnz), P(cv.keys), P(cv.w),
                               P(cv.norm), P(cv.words), ev.MAX_REFS, P(sc))
    score_ms, _ = clock(score, a.reps)
    device_ms = table_ms + sum(part.values()) + lcs_ms + cider_ms
    # the plain-Python reference on a slice, and the evaluator on the same slice
    from tests import eval_ref as ref
    from tests import rouge_ref
    n = min(a.ref_images, B)
    t = time.perf_counter()
    want = ref.evaluate(cands[:n], refs[:n], BOS, EOS, train_captions=train)
    want.update(zip(("rouge_l", "oracle_rouge_l", "mean_rouge_l"), rouge_ref.evaluate_rouge(cands[:n], refs[:n], BOS, EOS)[:3]))
    ref_s = time.perf_counter() - t
    got = ev.CaptionEvaluator(lib, refs[:n], BOS, EOS, vocab_size=V, train_captions=train).evaluate(cands[:n])
    exact = all(abs(got[k] - want[k]) <= 1e-12 * abs(want[k]) for k in ev.METRICS if "cider" not in k)
    close = all(abs(got[k] - want[k]) <= 1e-5 * abs(want[k]) + 1e-6 for k in ev.METRICS if "cider" in k)
    print(json.dumps({"images": B, "captions": C, "references": e.n_refs, "distinct_ngrams": e.n_df, "build_ms": round(build_ms, 1),
                      "evaluate_ms": round(eval_ms, 1), "evaluate_alternating_ms": round(float(np.median(with_ts)), 1),
                      "evaluate_without_lcs_alternating_ms": round(float(np.median(without_ts)), 1), "word_rows_ms": round(rows_ms, 1), "hypothesis_table_ms": round(table_ms, 3),
                      "overlap_references_ms": round(part["references"], 3), "overlap_earlier_ms": round(part["earlier"], 3),
                      "overlap_others_ms": round(part["others"], 3), "lcs_references_ms": round(lcs_ms, 3), "cider_path_ms": round(cider_ms, 3),
                      "consensus_score_same_pairs_ms": round(score_ms, 3), "host_ms": round(eval_ms - device_ms, 1),
                      "ref_images": n, "ref_s": round(ref_s, 2), "ref_s_scaled": round(ref_s * B / n, 1),
                      "slice_counts_match_reference": bool(exact), "slice_cider_matches_reference": bool(close),
                      "metrics": {k: res[k] for k in ev.METRICS}}))


if __name__ == "__main__":
    main()
