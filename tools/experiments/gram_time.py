"""In-set CIDEr-D timing on one GPU: 128 images x K captions (K = 20 and 100) of 8-16 words over a vocabulary of 10 000, a caption = its
image's base caption with 30 % of the words replaced and a random cut; idf from 5 000 corpus images x 5 captions.  Host clock around
synchronised calls, the median of 7 after 2 warm-ups:
  gram_ms             vc_cider_gram alone, both outputs, on a table that is already on the device
  consensus_ms        one vc_consensus_score call computing the unweighted means on the same table (k = 1, nbr[b] = b, img_cap =
                      cand_img, m = 2048): what the library could do before vc_cider_gram -- the same pair work plus a sort
  rerank_ms           a whole CiderGram.rerank (token lists -> word rows -> vectors -> matrices and means -> copy-back -> order)
  evaluate_ms         CaptionEvaluator.evaluate(self_cider=True) against 5 references per image; evaluate_plain_ms without the flag;
                      eigvalsh_ms the host eigenvalue part of it alone (mbr.self_cider of every image's matrix)
  ref_s_scaled        the float64 reference (tests/gram_ref.py) on --ref-images images, scaled to 128
One JSON line per K, appended to --out (default profiles/gram_time.txt).
    python tools/experiments/gram_time.py [--out FILE] [--ref-images 2]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_captioning_amd import abi, mbr  # noqa: E402
from vae_captioning_amd import consensus as cs  # noqa: E402
from vae_captioning_amd.abi import ptr as P  # noqa: E402
from vae_captioning_amd.evaluate import CaptionEvaluator  # noqa: E402

BOS, EOS = 1, 2
WARM, REPS = 2, 7


def caption(rng, vocab):
    return rng.integers(3, vocab, size=rng.integers(8, 17))


def variants(rng, base, n, vocab):
    out = []
    for _ in range(n):
        c = np.where(rng.random(base.size) < 0.3, rng.integers(3, vocab, size=base.size), base)[:rng.integers(8, base.size + 1)]
        out.append(c.tolist() + [EOS])                       # "w.. <EOS>", as diverse() returns them
    return out


def clock(fn):
    ts, out = [], None
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram_time.txt"))
    ap.add_argument("--ref-images", type=int, default=2)
    a = ap.parse_args()
    lib = abi.load()
    rng = np.random.default_rng(0)
    V, B = 10000, 128
    corpus = [[[BOS] + caption(rng, V).tolist() + [EOS] for _ in range(5)] for _ in range(5000)]
    cg = mbr.CiderGram(lib, corpus, BOS, EOS, vocab_size=V)
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    for K in (20, 100):
        bases = [np.concatenate([caption(rng, V), caption(rng, V)])[:16] for _ in range(B)]
        cands = [variants(rng, b, K, V) for b in bases]
        refs = [[[BOS] + c for c in variants(rng, b, 5, V)] for b in bases]
        diverse = [[(c, -1.0 - 0.01 * j, 1) for j, c in enumerate(cb)] for cb in cands]
        W, L = cs.word_rows([c for cb in cands for c in cb], BOS, EOS)
        cand_img = np.arange(0, B * K + 1, K)
        v = cs.ngram_vectors(lib, cg.dev, W, L, BOS, EOS, cg.df_keys, cg.idf, cg.n_df, cg.idf_unseen, head=cand_img)
        ld = (K + 3) // 4 * 4
        G = torch.empty((B * K, ld), dtype=torch.float32, device="cuda")
        m = torch.empty(B * K, dtype=torch.float64, device="cuda")
        sc = torch.empty(B * K, dtype=torch.float64, device="cuda")
        nbr = torch.arange(B, dtype=torch.int32, device="cuda")
        gram_ms, _ = clock(lambda: lib.vc_cider_gram(st, B, P(v.head), K, P(v.off), P(v.nnz), P(v.keys), P(v.w), P(v.norm), P(v.words), None,
                                                     P(G), ld, P(m)))
        cons_ms, _ = clock(lambda: lib.vc_consensus_score(st, B, 1, P(nbr), P(v.head), P(v.off), P(v.nnz), P(v.keys), P(v.w), P(v.norm),
                                                          P(v.words), P(v.head), K, P(v.off), P(v.nnz), P(v.keys), P(v.w), P(v.norm),
                                                          P(v.words), 2048, P(sc)))
        same = float(np.abs(m.cpu().numpy() / sc.cpu().numpy() - 1).max())
        rerank_ms, res = clock(lambda: cg.rerank(diverse))
        e = CaptionEvaluator(lib, refs, BOS, EOS, vocab_size=V)
        eval_ms, out = clock(lambda: e.evaluate(cands, self_cider=True))
        plain_ms, _ = clock(lambda: e.evaluate(cands))
        Gs, _ = cg.gram(cands)
        eig_ms, _ = clock(lambda: [mbr.self_cider(g) for g in Gs])
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import consensus_ref as cref
        n = a.ref_images
        idf, unseen = cref.df_idf(corpus, BOS, EOS) if not lines else lines[0]["_idf"]
        t = time.perf_counter()
        for b in range(n):
            vec = [cref.vector(c, BOS, EOS, idf, unseen) for c in cands[b]]
            [[cref.cider_d(h, r) for r in vec] for h in vec]
        ref_s = (time.perf_counter() - t) * B / n
        lines.append({"images": B, "captions_per_image": K, "gram_ms": round(gram_ms, 4), "consensus_ms": round(cons_ms, 4),
                      "gram_over_consensus": round(gram_ms / cons_ms, 3), "means_max_rel_diff": same, "rerank_ms": round(rerank_ms, 3),
                      "evaluate_ms": round(eval_ms, 3), "evaluate_plain_ms": round(plain_ms, 3), "eigvalsh_ms": round(eig_ms, 3),
                      "ref_images": n, "ref_s_scaled": round(ref_s, 2), "winner_moved": float(np.mean([r[0][1] != -1.0 for r in res])),
                      "self_cider": out["self_cider"], "mbr_cider_d": out["mbr_cider_d"], "cider_d": out["cider_d"],
                      "oracle_cider_d": out["oracle_cider_d"], "_idf": (idf, unseen)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for rec in lines:
            rec.pop("_idf")
            print(json.dumps(rec))
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
