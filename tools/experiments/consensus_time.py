"""Consensus re-ranking timing on one GPU at the full MSCOCO index size: 119 287 images x 4096 random-ReLU fc2 features, 5 captions of
8-16 words per image (vocabulary 10 000); 128 query images with 20 candidates each, k = 90, m = 125.  Host clock around synchronised
calls, median of --reps after warm-up: the index build (once), neighbours, the candidate n-gram vectors, the scoring launch, a whole
rerank.  Next to them the float64 numpy reference (tests/consensus_ref.py) on --ref-images images, scaled to 128.  One JSON line.
    python tools/experiments/consensus_time.py [--reps 10] [--ref-images 2] [--once]
--once: one warm rerank then one timed rerank only (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
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
from vae_captioning_amd import consensus as cs  # noqa: E402
from vae_captioning_amd.abi import ptr as P  # noqa: E402

BOS, EOS = 1, 2


def captions(rng, n, vocab):
    lens = rng.integers(8, 17, size=n)
    ids = rng.integers(3, vocab, size=int(lens.sum())).tolist()
    out, o = [], 0
    for L in lens.tolist():
        out.append([BOS] + ids[o:o + L] + [EOS])
        o += L
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=119287)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-images", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    lib = abi.load()
    rng = np.random.default_rng(0)
    D, F, V, B, K, k, m = a.images, 4096, 10000, 128, 20, 90, 125
    X = np.empty((D, F), np.float32)
    for r0 in range(0, D, 8192):
        X[r0:r0 + 8192] = np.maximum(rng.standard_normal((min(8192, D - r0), F), dtype=np.float32), 0)
    flat = captions(rng, D * 5, V)
    caps = [flat[5 * i:5 * i + 5] for i in range(D)]
    Q = np.maximum(rng.standard_normal((B, F), dtype=np.float32), 0)
    cands = [[c[1:] for c in captions(rng, K, V)] for _ in range(B)]          # "w.. <EOS>", as diverse() returns them
    diverse = [[(c, -1.0 - 0.01 * j, 1) for j, c in enumerate(cb)] for cb in cands]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx = cs.ConsensusIndex(lib, X, caps, BOS, EOS, k=k, m=m, vocab_size=V)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    Qd = torch.from_numpy(Q).cuda()

    def clock(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts)) * 1e3, out

    if a.once:
        idx.rerank(Qd, diverse)
        torch.cuda.synchronize()
        ms, _ = clock(lambda: idx.rerank(Qd, diverse), 1)
        print(json.dumps({"rerank_ms": round(ms, 3)}))
        return
    for _ in range(3):
        idx.rerank(Qd, diverse)
    nb_ms, (ids, _) = clock(lambda: idx._neighbours_dev(Qd), a.reps)
    flatc = [c for cb in cands for c in cb]
    W, L = cs.word_rows(flatc, BOS, EOS)
    vec_ms, cv = clock(lambda: idx._vectors(W, L), a.reps)
    cand_img = torch.from_numpy(np.arange(0, B * K + 1, K, dtype=np.int32)).cuda()
    out = torch.empty(B * K, dtype=torch.float64, device="cuda")
    rv = idx.caps

    def score():
        lib.vc_consensus_score(torch.cuda.current_stream().cuda_stream, B, k, P(ids), P(idx.img_cap), P(rv.off), P(rv.nnz), P(rv.keys),
                               P(rv.w), P(rv.norm), P(rv.words), P(cand_img), K, P(cv.off), P(cv.nnz), P(cv.keys), P(cv.w), P(cv.norm),
                               P(cv.words), m, P(out))
    sc_ms, _ = clock(score, a.reps)
    rr_ms, res = clock(lambda: idx.rerank(Qd, diverse), a.reps)
    # the float64 numpy reference on a few images, scaled to B
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import consensus_ref as ref
    n = a.ref_images
    t = time.perf_counter()
    C = ref.cosines(Q[:n], X)
    nbr = [ref.topk_order(C[b], k) for b in range(n)]
    ref_nb_s = (time.perf_counter() - t) * B / n
    t = time.perf_counter()
    ridf, unseen = ref.df_idf(caps, BOS, EOS)
    ref_df_s = time.perf_counter() - t
    t = time.perf_counter()
    for b in range(n):
        pool = [ref.vector(c, BOS, EOS, ridf, unseen) for i in nbr[b] for c in caps[i]]
        ref.consensus([ref.vector(c, BOS, EOS, ridf, unseen) for c in cands[b]], pool, m)
    ref_sc_s = (time.perf_counter() - t) * B / n
    print(json.dumps({"index_images": D, "index_captions": idx.n_captions, "distinct_ngrams": idx.n_df, "queries": B, "candidates": K,
                      "k": k, "m": m, "index_build_s": round(build_s, 2), "neighbours_ms": round(nb_ms, 3),
                      "candidate_vectors_ms": round(vec_ms, 3), "score_ms": round(sc_ms, 3), "rerank_ms": round(rr_ms, 3),
                      "ref_neighbours_s_scaled": round(ref_nb_s, 2), "ref_df_s": round(ref_df_s, 2), "ref_score_s_scaled": round(ref_sc_s, 2),
                      "ref_images": n, "winner_moved": float(np.mean([r[0][1] != -1.0 for r in res]))}))


if __name__ == "__main__":
    main()
