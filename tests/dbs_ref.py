"""Group ("diverse") beam search in numpy / Python: the checker of vc_beam_update_groups and CaptionGenerator.diverse_beam_search
(test infrastructure, never the product path).  Diverse Beam Search (Vijayakumar et al. 2016) with the Hamming dissimilarity on the
TopN / Beam classes and the decoder step of oracle.decode:

    chosen = []                                  # last words of the NEW live beams of this round's groups 0..g-1
    for g in 0..G-1:
        for beam in partial[g].extract():        # heap ARRAY order
            cand = the kc most probable words of the beam's row, descending, stable
            lp   = beam.logprob + float64(float32 log p);  c = chosen.count(word);  key = lp if c == 0 else lp - lam * c
            the first w of cand under (key descending, raw rank ascending), in that order:
                skip if p < 1e-12;  <EOS> -> complete[g] (score lp / len**len_norm_f);  else -> partial[g] (logprob lp, score key)
        chosen += last words of partial[g]'s heap array
"""
import numpy as np

from oracle import decode as od
from oracle.decode import Beam, TopN
from vae_captioning_amd import spec
from vae_captioning_amd.utils.parameters import Parameters

CASES = [dict(no_encoder=True), dict(prior="Normal"), dict(prior="AG", use_c_v=True), dict(prior="GMM")]
CASE_IDS = ["-".join("%s=%s" % i for i in k.items()) for k in CASES]


def model_inputs(seed, V=40, B=6, **kw):
    """The small model and images of the generation parity tests (tests/test_gpu_generate.py: setup), without an engine:
    (params, float32 weights, features, cluster vectors, eps, float64 cluster means or None)."""
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden = 32, 64, 64
    p.latent_size, p.gen_z_samples, p.cnn_feature_size = 10, 4, 48
    p.mode, p.num_captions = "inference", 1
    for k, v in kw.items():
        setattr(p, k, v)
    rng = np.random.default_rng(seed)
    P0 = spec.init_caption_params(p, V, seed=seed)
    for k in P0:  # larger weights -> peaked distributions, <EOS> reachable
        P0[k] = (P0[k] * 3).astype(np.float32) if not k.endswith("bias") else rng.normal(0, 0.5, P0[k].shape).astype(np.float32)
    feats = np.maximum(rng.standard_normal((B, p.cnn_feature_size)), 0).astype(np.float32)
    cv = np.zeros((B, 90), np.float32)
    for b in range(B - 1):  # last image: empty cluster vector (AG fallback branch, Q16)
        cv[b, rng.choice(90, size=2, replace=False)] = 0.5
    eps = rng.standard_normal((p.gen_z_samples, B, p.latent_size)).astype(np.float32)
    cm = od.init_clusters(90, p.latent_size).astype(np.float64) if p.prior == "AG" else None
    return p, P0, feats, cv, eps, cm


def reference(p, P0, feats, cv, eps, cm, bos, eos, dtype=np.float64, **kw):
    """diverse_beam_search below for every image of model_inputs, computed in `dtype`: per image the list of G (sentences, scores)."""
    Pd = {k: v.astype(dtype) for k, v in P0.items()}
    cmd = cm.astype(dtype) if cm is not None else None
    return [diverse_beam_search(Pd, p, feats[b].astype(dtype), cv[b].astype(dtype), eps[:, b:b + 1].astype(dtype), bos, eos, c_means=cmd, **kw)
            for b in range(feats.shape[0])]


def group_round(partial, complete, rows, w, lam, eos, len_norm_f):
    """One round of one image.  partial / complete: lists of G TopN; rows(g, i, beam) -> (words, probs) of the i-th live beam of group g
    (descending, stable), or (words, probs, state) where the new beams carry `state`.  New beams' .state is that state if given, else
    the index i of the beam they continue."""
    chosen = []
    for g in range(len(partial)):
        plist = partial[g].extract()
        partial[g].reset()
        for i, beam in enumerate(plist):
            got = rows(g, i, beam)
            words, probs, state = got if len(got) == 3 else (got[0], got[1], i)
            lps, keys = [], []
            for word, p in zip(words, probs):
                lp = beam.logprob + float(np.log(np.float32(p)))   # decoder.py:282: float32 log, float64 sum
                c = chosen.count(int(word))
                lps.append(lp)
                keys.append(lp if c == 0 else lp - lam * c)
            order = sorted(range(len(words)), key=lambda r: (-keys[r], r))[:w]
            for r in order:
                word, p = int(words[r]), probs[r]
                if p < 1e-12:
                    continue
                sent = beam.sentence + [word]
                if word == eos:
                    score = lps[r] / len(sent) ** len_norm_f if len_norm_f > 0 else lps[r]
                    complete[g].push(Beam(sent, state, lps[r], score))
                else:
                    partial[g].push(Beam(sent, state, lps[r], keys[r]))
        chosen += [b.sentence[-1] for b in partial[g]._data]


def start(G, w, bos, state=0):
    partial, complete = [TopN(w) for _ in range(G)], [TopN(w) for _ in range(G)]
    for g in range(G):
        partial[g].push(Beam([bos], state, 0.0, 0.0))
    return partial, complete


def table_rounds(tables, B, G, w, lam, bos, eos, len_norm_f):
    """The kernel test's reference: tables = [(top_p, top_i), ...] per round, each [B*G*w, kc] (row (b*G + g)*w + i is the i-th live beam
    of group g of image b).  Yields after every round (partial, complete): per image the lists of G TopN."""
    heaps = [start(G, w, bos) for _ in range(B)]
    for tv, ti in tables:
        with np.errstate(divide="ignore"):
            for b in range(B):
                rows = lambda g, i, beam, b=b: (ti[(b * G + g) * w + i], tv[(b * G + g) * w + i])
                group_round(heaps[b][0], heaps[b][1], rows, w, lam, eos, len_norm_f)
        yield [h[0] for h in heaps], [h[1] for h in heaps]


def diverse_beam_search(P, cfg, feature, c_v_row, eps, bos, eos, c_means=None, groups=5, group_size=2, diversity=0.5, max_len=30,
                        len_norm_f=0.7, kc=None):
    """One image, end to end, in the precision of P / feature / eps.  kc: candidates per row (None: min(G*w, V); "all": the whole
    vocabulary).  Returns per group (sentences, scores), descending."""
    G, w = int(groups), int(group_size)
    state = od.initial_state(P, cfg, feature, c_v_row, eps, c_means, std=getattr(cfg, "std", 0.1))
    _, state = od.step(P, bos, state)   # decoder.py:230-236: <BOS> consumed twice, probabilities discarded
    partial, complete = start(G, w, bos, state)

    def rows(g, i, beam):
        probs, st = od.step(P, beam.sentence[-1], beam.state)
        probs = probs.ravel()
        n = probs.size if kc == "all" else min(kc or G * w, probs.size)
        words = np.argsort(-probs, kind="stable")[:n]
        return words, probs[words], st

    for _ in range(max_len - 1):
        with np.errstate(divide="ignore"):
            group_round(partial, complete, rows, w, diversity, eos, len_norm_f)
        if all(p.size() == 0 for p in partial):
            break
    out = []
    for g in range(G):
        beams = (complete[g] if complete[g].size() else partial[g]).extract(sort=True)
        out.append(([b.sentence for b in beams], [b.score for b in beams]))
    return out
