"""-m gpu: consensus re-ranking of diverse captions (vae_captioning_amd/consensus.py, csrc/consensus.hip).  The wide top-k against
vc_topk_rows_f32 bit for bit, the neighbours against a float64 cosine top-k, the n-gram vectors and consensus scores against the float64
reference of tests/consensus_ref.py, the re-ranking's behaviour on a planted index, and the Decoder / inference() / main.py paths."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd.abi import ptr as P
from vae_captioning_amd.consensus import ConsensusIndex, unpack_key

from . import consensus_ref as ref

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = np.array([-0.5, -0.0, 0.0, 0.25, 1.0, 3.0], np.float32)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _wide(lib, x, k, exclude=None):
    rows, cols = x.shape
    xd = torch.from_numpy(x).cuda()
    v, i = torch.empty((rows, k), device="cuda"), torch.empty((rows, k), dtype=torch.int32, device="cuda")
    nb = lib.vc_topk_rows_wide_workspace_bytes(rows, cols, k)
    ws = torch.empty(max(1, nb // 4 + 1), device="cuda")
    ex = torch.from_numpy(np.asarray(exclude, np.int32)).cuda() if exclude is not None else None
    lib.vc_topk_rows_wide_f32(_st(), P(xd), rows, cols, cols, k, P(ex), P(v), P(i), P(ws), nb)
    return v.cpu().numpy(), i.cpu().numpy()


def _narrow(lib, x, k):
    rows, cols = x.shape
    xd = torch.from_numpy(x).cuda()
    v, i = torch.empty((rows, k), device="cuda"), torch.empty((rows, k), dtype=torch.int32, device="cuda")
    lib.vc_topk_rows_f32(_st(), P(xd), rows, cols, cols, k, P(v), P(i))
    return v.cpu().numpy(), i.cpu().numpy()


WIDE = [(c, k, r) for c in (1, 255, 10000, 119287) for k in (1, 8, 9, 90, 256) if k <= c
        for r in ((1, 7) if c == 119287 else (1, 7, 128))]


@pytest.mark.parametrize("cols,k,rows", WIDE, ids=lambda v: str(v))
def test_wide_topk_is_bit_identical_to_topk_rows(lib, cols, k, rows):
    rng = np.random.default_rng(cols * 7 + k * 3 + rows)
    x = LEVELS[rng.integers(0, LEVELS.size, size=(rows, cols))]
    if cols > 300:
        x[0, rng.integers(0, cols, size=5)] = 7.0           # a few distinct maxima far apart
    gv, gi = _wide(lib, x, k)
    nv, ni = _narrow(lib, x, k)
    assert np.array_equal(gi, ni)
    assert np.array_equal(gv.view(np.uint32), nv.view(np.uint32))


@pytest.mark.parametrize("cols,k", [(255, 9), (10000, 90), (119287, 256)])
def test_wide_topk_with_exclusions_drops_the_column(lib, cols, k):
    rng = np.random.default_rng(cols + k)
    rows = 5
    x = LEVELS[rng.integers(0, LEVELS.size, size=(rows, cols))]
    ex = np.array([-1, 0, cols - 1, int(rng.integers(cols)), -1])
    ex[3] = int(ref.topk_order(x[3], 1)[0])                   # the row's best column
    gv, gi = _wide(lib, x, k, ex)
    for r in range(rows):
        want = ref.topk_order(x[r], k, ex[r])
        assert gi[r].tolist() == want.tolist(), r
        assert np.array_equal(gv[r], x[r, want])


def _index(lib, feats, caps=None, k=5, m=125, **kw):
    caps = caps if caps is not None else [[[BOS, 3 + i % 50, EOS]] for i in range(len(feats))]
    return ConsensusIndex(lib, feats, caps, BOS, EOS, k=k, m=m, **kw)


def test_neighbours_match_float64_cosines(lib):
    rng = np.random.default_rng(11)
    D, F, B, k = 50000, 4096, 256, 90
    X = np.maximum(rng.standard_normal((D, F), dtype=np.float32), 0)
    X[[3, 777, 49999]] = 0.0
    Q = np.maximum(rng.standard_normal((B, F), dtype=np.float32), 0)
    Q[:8] = X[rng.integers(0, D, size=8)] * 2.0               # queries that are index rows (cosine 1)
    Q[9] = 0.0
    idx = _index(lib, X, k=k)
    ids, cos = idx.neighbours(Q)
    C = ref.cosines(Q, X)
    assert ids.shape == (B, k) and ids.dtype == np.int32 and cos.dtype == np.float32
    for b in range(B):
        want = ref.topk_order(C[b], k)
        np.testing.assert_allclose(cos[b], C[b, ids[b]], rtol=0, atol=1e-5)
        assert np.all(np.abs(C[b, ids[b]] - C[b, want]) < 2e-5), b    # equal lists up to swaps of near-equal cosines
        assert len(set(ids[b].tolist())) == k
    assert ids[9].tolist() == list(range(k)) and np.all(cos[9] == 0)  # a zero query: every cosine 0, index order
    ex = np.full(B, -1)
    ex[:8] = ids[:8, 0]                                         # the query's own index row
    ids_ex, _ = idx.neighbours(Q, exclude=ex)
    assert np.array_equal(ids_ex[8:], ids[8:])
    assert all(ids_ex[b].tolist() == ids[b, 1:].tolist() + [ids_ex[b, -1]] and ids[b, 0] not in ids_ex[b] for b in range(8))


def test_neighbours_in_query_passes_equal_one_pass_at_full_size(lib):
    rng = np.random.default_rng(12)
    D, F, B = 119287, 4096, 256
    X = np.maximum(rng.standard_normal((D, F), dtype=np.float32), 0)
    Q = np.maximum(rng.standard_normal((B, F), dtype=np.float32), 0)
    idx = _index(lib, X, k=90)
    one = idx.neighbours(Q)
    idx.block_bytes = 128 * 4 * ((D + 3) // 4 * 4)          # 128 queries per pass: two passes
    two = idx.neighbours(Q)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1].view(np.uint32), two[1].view(np.uint32))


def _random_caps(rng, n_img, per, vocab, lo=1, hi=16):
    return [[[BOS] + rng.integers(3, vocab, size=rng.integers(lo, hi + 1)).tolist() + [EOS] for _ in range(per)] for _ in range(n_img)]


def test_ngram_vectors_match_the_reference(lib):
    rng = np.random.default_rng(5)
    caps = _random_caps(rng, 60, 3, 9, 0, 20)
    caps[0][0] = [BOS] + [4] * 64 + [EOS]                     # 64 words, one repeated word
    caps[1][1] = [0, BOS, 5, 0, 6, EOS, 0]                    # PAD / BOS / EOS anywhere
    idx = _index(lib, np.maximum(rng.standard_normal((60, 16), dtype=np.float32), 0), caps)
    ridf, unseen = ref.df_idf(caps, BOS, EOS)
    v = idx.caps
    off, nnz = v.off.cpu().numpy(), v.nnz.cpu().numpy()
    keys, w = v.keys.cpu().numpy().view(np.uint64), v.w.cpu().numpy()
    norm, nw = v.norm.cpu().numpy(), v.words.cpu().numpy()
    for i, c in enumerate(x for cs in caps for x in cs):
        L, vec, norms = ref.vector(c, BOS, EOS, ridf, unseen)
        want = sorted((g, wt) for n in range(1, 5) for g, wt in vec[n].items())
        got_k = keys[off[i]:off[i] + nnz[i]].tolist()
        assert got_k == [g for g, _ in want] and nw[i] == L
        assert np.array_equal(w[off[i]:off[i] + nnz[i]], np.array([wt for _, wt in want], np.float32))
        np.testing.assert_allclose(norm[i], norms, rtol=1e-6, atol=0)
    assert unpack_key(keys[off[0] + 1]) == [4, 4]


SCORE_CASES = [  # (K candidates per image, neighbours k, captions per index image, m)
    (1, 1, 1, 1), (20, 90, 5, 125), (20, 90, 5, 1), (256, 3, 2, 125), (20, 256, 8, 125), (20, 256, 8, 5000), (7, 30, 4, 200)]


@pytest.mark.parametrize("K,k,per,m", SCORE_CASES, ids=lambda v: str(v))
def test_consensus_scores_match_the_reference(lib, K, k, per, m):
    rng = np.random.default_rng(K * 1000 + k + per + m)
    D, F, B, vocab = max(300, k + 10), 32, 2, 30
    X = np.maximum(rng.standard_normal((D, F), dtype=np.float32), 0)
    caps = _random_caps(rng, D, per, vocab, 1, 16)
    idx = _index(lib, X, caps, k=k, m=m)
    Q = np.maximum(rng.standard_normal((B, F), dtype=np.float32), 0)
    cands = []
    for b in range(B):
        cb = [[int(t) for t in rng.integers(3, vocab, size=rng.integers(0, 18))] + [EOS] for _ in range(K)]
        cb[0] = list(caps[int(rng.integers(D))][0])            # an index caption among the candidates
        cands.append(cb)
    got = idx.score(Q, cands)
    ids, _ = idx.neighbours(Q)
    ridf, unseen = ref.df_idf(caps, BOS, EOS)
    for b in range(B):
        pool = [ref.vector(c, BOS, EOS, ridf, unseen) for i in ids[b] for c in caps[i]]
        assert len(pool) == k * per
        want = ref.consensus([ref.vector(c, BOS, EOS, ridf, unseen) for c in cands[b]], pool, m)
        assert got[b].dtype == np.float64 and got[b].shape == (K,)
        np.testing.assert_allclose(got[b], want, rtol=1e-5, atol=1e-6)
        if K > 1:
            top = np.sort(want)[::-1]
            if top[0] - top[1] > 1e-5 * abs(top[0]):
                assert np.argmax(got[b]) == np.argmax(want)


# ------------------------------------------------------------------ behaviour on a planted index
def test_rerank_puts_the_planted_last_candidate_first_and_zero_scores_keep_the_likelihood_order(lib):
    from .test_gpu_generate import setup
    p, eng, gen, _, feats, _, _, _ = setup(lib, 21)
    p.temperature = 1.5
    B, K = feats.shape[0], 12
    res = gen.diverse(feats, None, None, BOS, EOS, draws=K, method="sample", max_len=10)
    cand = [b for b in range(B) if len(res[b]) >= 2 and len(ref.words(res[b][-1][0], BOS, EOS)) >= 1]
    assert len(cand) >= 2, [len(r) for r in res]
    rng = np.random.default_rng(0)
    copies, others = 3, 40
    X = np.concatenate([np.repeat(feats[cand], copies, axis=0), np.maximum(rng.standard_normal((others, feats.shape[1])), 0)]).astype(np.float32)
    far = [[[BOS] + (100 + rng.integers(0, 50, size=6)).tolist() + [EOS]] for _ in range(others)]   # no word of the model's 40
    planted = [[list(res[b][-1][0])] for b in cand for _ in range(copies)]
    idx = ConsensusIndex(eng, X, planted + far, BOS, EOS, k=copies, m=125)
    sub = [res[b] for b in cand]
    out = idx.rerank(feats[cand], sub)
    for entries, o in zip(sub, out):
        assert o[0][0] == entries[-1][0] and o[0][3] > max(e[3] for e in o[1:])
        assert sorted(e[0] for e in o) == sorted(e[0] for e in entries) and len(o) == len(entries)
    blank = [[[BOS] + (200 + rng.integers(0, 50, size=5)).tolist() + [EOS]] for _ in planted]
    idx0 = ConsensusIndex(eng, X, blank + far, BOS, EOS, k=copies, m=125)
    out0 = idx0.rerank(feats[cand], sub)
    for entries, o in zip(sub, out0):
        assert all(e[3] == 0.0 for e in o)
        assert [e[:3] for e in o] == [tuple(e) for e in entries]


# ------------------------------------------------------------------ facade, driver, command line
class _Dict(object):
    word2idx = {"<BOS>": BOS, "<EOS>": EOS, "<PAD>": 0}
    idx2word = {i: "w%d" % i for i in range(40)}
    idx2word.update({BOS: "<BOS>", EOS: "<EOS>", 0: "<PAD>"})
    vocab_size = 40


def _facade_params():
    from vae_captioning_amd.utils.parameters import Parameters
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden = 32, 64, 64
    p.latent_size, p.gen_z_samples, p.cnn_feature_size = 10, 4, 48
    p.mode, p.num_captions, p.vocab_size, p.gen_max_len = "inference", 1, 40, 10
    p.sample_gen, p.diverse_draws, p.diverse_method, p.temperature = "diverse", 6, "sample", 1.5
    return p


def _facade_index(lib, feats):
    rng = np.random.default_rng(9)
    X = np.concatenate([feats, np.maximum(rng.standard_normal((30, feats.shape[1])), 0)]).astype(np.float32)
    return ConsensusIndex(lib, X, _random_caps(rng, X.shape[0], 3, 40, 2, 9), BOS, EOS, k=4, m=6)


def test_decoder_diverse_inference_records_with_and_without_consensus(lib):
    from vae_captioning_amd.vae_model.decoder import Decoder
    p = _facade_params()
    dec = Decoder(None, None, None, p, _Dict)
    feats = np.maximum(np.random.default_rng(0).standard_normal((3, 48)), 0).astype(np.float32)
    plain = dec.diverse_inference(None, ["a", "b", "c"], feats, None)
    assert all(set(r) == {"image_id", "caption", "captions", "scores", "counts"} for r in plain)
    p.diverse_rerank = "consensus"
    with pytest.raises(RuntimeError, match="consensus_index"):
        dec.diverse_inference(None, ["a", "b", "c"], feats, None)
    dec.consensus_index = _facade_index(lib, feats)
    recs = dec.diverse_inference(None, ["a", "b", "c"], feats, None)
    for r, q in zip(recs, plain):
        assert set(r) == {"image_id", "caption", "captions", "scores", "counts", "consensus"}
        assert r["caption"] == r["captions"][0] and len(r["consensus"]) == len(r["captions"])
        assert r["consensus"] == sorted(r["consensus"], reverse=True)
        assert sorted(r["captions"]) == sorted(q["captions"])       # the same distinct captions (same draws), re-ordered
    two = dec.diverse_inference(None, ["a", "b", "c"], feats, None, n_best=2)
    assert [r["captions"] for r in two] == [r["captions"][:2] for r in recs]


def test_inference_driver_writes_the_consensus_winner(lib, tmp_path, monkeypatch):
    from vae_captioning_amd.ops.inference import inference
    from vae_captioning_amd.vae_model.decoder import Decoder
    p = _facade_params()
    p.gen_name, p.diverse_rerank = "cs", "consensus"
    feats = np.maximum(np.random.default_rng(1).standard_normal((4, 48)), 0).astype(np.float32)

    class Val(object):
        def next_val_batch(self, get_image_ids=True, use_obj_vectors=False):
            yield feats[:2], None, None, [11, 12], np.zeros((2, 91), np.float32)
            yield feats[2:], None, None, [13, 14], np.zeros((2, 91), np.float32)

    monkeypatch.chdir(tmp_path)
    dec = Decoder(None, None, None, p, _Dict)
    dec.consensus_index = _facade_index(lib, feats)
    inference(p, dec, Val(), None)
    coco = json.load(open(tmp_path / "val_cs.json"))
    full = json.load(open(tmp_path / "val_cs_diverse.json"))
    assert [r["image_id"] for r in coco] == [11, 12, 13, 14] and all(set(r) == {"image_id", "caption"} for r in coco)
    assert [r["caption"] for r in coco] == [r["captions"][0] for r in full]
    assert all(r["consensus"] == sorted(r["consensus"], reverse=True) and len(r["consensus"]) == len(r["captions"]) for r in full)


def test_main_synthetic_inference_with_consensus_reranking(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    common = ["--synthetic", "--vocab", "200", "--embed_dim", "32", "--enc_hid", "64", "--dec_hid", "64", "--latent", "10",
              "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "cs"]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + common + ["--epochs", "1", "--max_steps", "1"],
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + common +
                       ["--mode", "inference", "--sample_gen", "diverse", "--diverse_draws", "4", "--gen_name", "cs",
                        "--diverse_rerank", "consensus", "--consensus_k", "20", "--consensus_m", "30"],
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = json.load(open(tmp_path / "val_cs.json"))
    assert len(recs) == 8 and all(sum(x["counts"]) == 4 and len(x["consensus"]) == len(x["captions"]) for x in recs)
    assert all(x["consensus"] == sorted(x["consensus"], reverse=True) for x in recs)
