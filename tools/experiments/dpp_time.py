"""DPP selection timing on one GPU: B images x K captions (128 x 20, 128 x 256 and 4096 x 20) of 8-16 words over a vocabulary of
10 000, a caption = its image's base caption with 30 % of the words replaced and a random cut; idf from 5 000 corpus images x 5
captions; qualities from descending scores with weight 1.  Host clock around synchronised calls, the median of 7 after 2 warm-ups:
  gram_ms             the vc_cider_gram call the selection follows (matrix only), on a table that is already on the device
  dpp_n5_ms .. dpp_n32_ms   vc_dpp_select_f64 alone on the block that call wrote, n = 5, 8, 9 and 32 (8 and 9 do nearly the same work
                      in the kernel's two instantiations, 16 KiB and 64 KiB of LDS: what the smaller one buys shows at 4096 images)
  select_n5_ms        a whole CiderGram.select(n = 5): token lists -> word rows -> vectors -> matrices -> selection -> the three small
                      arrays back -> entries
  host_n5_ms          what the device selection replaces: CiderGram.gram (every matrix copied to the host) and the numpy float64
                      reference of the definition (tests/dpp_ref.py) per image, n = 5
chosen_n*: the mean number of captions the greedy steps chose per image (the rest of n is the fill).
One JSON line per shape, appended to --out (default profiles/dpp_time.txt).
    python tools/experiments/dpp_time.py [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpp_time.txt"))
    a = ap.parse_args()
    lib = abi.load()
    rng = np.random.default_rng(0)
    V = 10000
    corpus = [[[BOS] + caption(rng, V).tolist() + [EOS] for _ in range(5)] for _ in range(5000)]
    cg = mbr.CiderGram(lib, corpus, BOS, EOS, vocab_size=V)
    st = torch.cuda.current_stream().cuda_stream
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dpp_ref
    lines = []
    for B, K in ((128, 20), (128, 256), (4096, 20)):
        bases = [np.concatenate([caption(rng, V), caption(rng, V)])[:16] for _ in range(B)]
        cands = [variants(rng, b, K, V) for b in bases]
        diverse = [[(c, -1.0 - 0.01 * j, 1) for j, c in enumerate(cb)] for cb in cands]
        W, L = cs.word_rows([c for cb in cands for c in cb], BOS, EOS)
        cand_img = np.arange(0, B * K + 1, K)
        v = cs.ngram_vectors(lib, cg.dev, W, L, BOS, EOS, cg.df_keys, cg.idf, cg.n_df, cg.idf_unseen, head=cand_img)
        ld = (K + 3) // 4 * 4
        G = torch.empty((B * K, ld), dtype=torch.float32, device="cuda")
        qh = np.concatenate([mbr.dpp_quality(mbr.list_keys(e), 1.0) for e in diverse])
        q = torch.from_numpy(qh).cuda()
        gram_ms, _ = clock(lambda: lib.vc_cider_gram(st, B, P(v.head), K, P(v.off), P(v.nnz), P(v.keys), P(v.w), P(v.norm), P(v.words), None,
                                                     P(G), ld, None))
        rec = {"images": B, "captions_per_image": K, "gram_ms": round(gram_ms, 4)}
        for n in (5, 8, 9, 32):
            sel = torch.empty(B * n, dtype=torch.int32, device="cuda")
            gain = torch.empty(B * n, dtype=torch.float64, device="cuda")
            nd = torch.empty(B, dtype=torch.int32, device="cuda")
            ms, _ = clock(lambda: lib.vc_dpp_select_f64(st, B, P(v.head), K, P(G), ld, P(q), n, P(sel), P(gain), P(nd)))
            rec["dpp_n%d_ms" % n] = round(ms, 4)
            rec["dpp_n%d_over_gram" % n] = round(ms / gram_ms, 3)
            rec["chosen_n%d" % n] = float(nd.cpu().numpy().mean())
        select_ms, picked = clock(lambda: cg.select(diverse, 5))

        def on_the_host():
            Gs, _ = cg.gram(cands)
            return [dpp_ref.select(g, qh[b * K:(b + 1) * K], 5) for b, g in enumerate(Gs)]
        host_ms, want = clock(on_the_host)
        same = float(np.mean([[e[0] for e in out] == [cands[b][j] for j in w[0] if j >= 0] for b, (out, w) in enumerate(zip(picked[0], want))]))
        rec.update(select_n5_ms=round(select_ms, 3), host_n5_ms=round(host_ms, 3), same_selection_as_the_host=same)
        lines.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for rec in lines:
            print(json.dumps(rec))
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
