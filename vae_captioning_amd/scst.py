"""Self-critical sequence training (Rennie et al. 2017): the decoder is fine-tuned on the CIDEr-D of its OWN samples.

One `Trainer.scst_step(batch)`:

1. sample K = num_captions captions per image (CaptionGenerator's diverse pass, method "sample", temperature 1, no truncation), each
   under its own prior draw z;
2. (baseline "greedy") decode the same rows greedily under the same z;
3. reward every caption with its CIDEr-D against the image's own human captions of the batch (`CiderReward`, the kernels
   `CaptionEvaluator._cider` uses), turn rewards into advantages (`advantages`, host float64);
4. one policy-gradient step of the decoder on the sampled captions under the given z (`CaptionEngine.policy_forward`, csrc/loss.hip's
   vc_softmax_xent_policy_f32): the gradient of 1/N sum_n -A[n] log p(caption n | z_n, image) (- beta * token entropies).

The reward is any object with `rewards(candidates_per_image, references_per_image)`: `CiderReward` alone by default; with
--scst_rouge W > 0 the `SumReward` CIDEr-D + W * ROUGE-L (`RougeReward`: csrc/lcs.hip's vc_lcs_overlap, evaluate.rouge_l).

DESIGN.md, "Self-critical training", has the estimator, the trained variables and how z travels from the sampler to the step.
"""
import types

import numpy as np
import torch

from .abi import ptr as P
from .consensus import MAX_POOL, host_index, library_and_device, ngram_vectors, upload, word_rows
from .engine import _stream
from .generate import DIVERSE_MAX_DRAWS

BASELINES = ("average", "greedy")


def check_baseline(baseline, num_captions):
    if baseline not in BASELINES:
        raise ValueError("scst baseline must be one of %s (got %r)" % (", ".join(BASELINES), baseline))
    if baseline == "average" and int(num_captions) < 2:
        raise ValueError("the average baseline compares an image's samples with each other: it needs num_captions >= 2 (got %d)" % num_captions)


def advantages(rewards, baseline="average", greedy_rewards=None):
    """rewards [B, K] -> advantages [B, K], float64 on the host.
    "average": A[b,k] = r[b,k] - mean over j != k of r[b,j] (the other samples of the image are the baseline; K >= 2);
    "greedy":  A[b,k] = r[b,k] - greedy_rewards[b,k] (the reward of the greedy decode of the same row under the same z)."""
    r = np.asarray(rewards, np.float64)
    if r.ndim != 2:
        raise ValueError("rewards must be [images, samples per image]")
    check_baseline(baseline, r.shape[1])
    if baseline == "average":
        K = r.shape[1]
        # the mean over j != k of the DIFFERENCES r[b,k] - r[b,j]: equal rewards give exactly 0, whatever K
        return (r[:, :, None] - r[:, None, :]).sum(axis=2) / (K - 1)
    if greedy_rewards is None:
        raise ValueError("the greedy baseline needs the greedy captions' rewards")
    g = np.asarray(greedy_rewards, np.float64)
    if g.shape != r.shape:
        raise ValueError("greedy rewards %s for rewards %s" % (g.shape, r.shape))
    return r - g


def policy_batch(samples, bos, eos):
    """Sampled captions -> the caption arrays of a policy step.  samples: N token lists (without <BOS>, with their <EOS> when they
    ended, at least one token each), in caption-row order.  Returns cap_dec [N, T] ("<BOS> w.."), cap_enc [N, T] (the labels: the
    sampled tokens) and lengths [N]; T = the longest sample of the batch (what form_captions_batch does with human captions).
    Id 0 is a class of the logits layer, so a model may sample it: such a token stays in the caption (the decoder is fed it and runs
    on), but as a label it is <PAD> -- its row is masked like every PAD label of the cross-entropy objective and trains nothing."""
    N = len(samples)
    lens = np.fromiter((len(s) for s in samples), np.int32, N)
    if N == 0 or lens.min() < 1:
        raise ValueError("every sampled caption holds at least one token (its <EOS>)")
    T = int(lens.max())
    cap_dec, cap_enc = np.zeros((N, T), np.int32), np.zeros((N, T), np.int32)
    for n, s in enumerate(samples):
        cap_enc[n, :len(s)] = s
        cap_dec[n, 0] = bos
        cap_dec[n, 1:len(s)] = s[:-1]
    return dict(cap_dec=cap_dec, cap_enc=cap_enc, lengths=lens)


def batch_references(cap_enc, lengths, nc):
    """The human captions of an XE batch as references: per image the token lists of its nc rows b*nc .. b*nc + nc - 1 of cap_enc
    ("w.. <EOS>"; the all-PAD rows of an image with fewer captions are left out)."""
    cap_enc, lengths = np.asarray(cap_enc), np.asarray(lengths)
    B = cap_enc.shape[0] // nc
    out = []
    for b in range(B):
        refs = [[int(t) for t in cap_enc[b * nc + k, :int(lengths[b * nc + k])]] for k in range(nc)]
        out.append([r for r in refs if r] or [[]])   # (an image without any caption keeps one empty reference: reward 0)
    return out


def corpus_df(corpus_captions_per_image, bos, eos, vocab_size=None):
    """Host half of CiderReward: (sorted n-gram keys uint64, their idf float32, the idf of an unseen n-gram) with document
    frequencies counted over the corpus IMAGES (consensus.host_index: idf = log D - log max(1, df), unseen n-grams log D)."""
    h = host_index(corpus_captions_per_image, bos, eos, vocab_size)
    return h.df_keys, h.idf, float(h.idf_unseen)


class CiderReward(object):
    """Per-caption CIDEr-D against given references, with document frequencies from a CORPUS (per image a list of token lists: the
    training captions): df / idf are computed once (consensus.host_index) and held on the device.
    lib_or_engine: the C-ABI library (abi.load()) or a CaptionEngine (its library and device)."""

    def __init__(self, lib_or_engine, corpus_captions_per_image, bos, eos, vocab_size=None):
        self.lib, self.dev = library_and_device(lib_or_engine)
        self.bos, self.eos = int(bos), int(eos)
        df_keys, idf, self.idf_unseen = corpus_df(corpus_captions_per_image, bos, eos, vocab_size)
        self.D = len(corpus_captions_per_image)
        self.n_df = int(df_keys.size)
        self.df_keys = upload(self.dev, df_keys.view(np.int64) if self.n_df else np.zeros(1, np.int64))
        self.idf = upload(self.dev, idf if self.n_df else np.zeros(1, np.float32))
        self.host_seconds = 0.0   # time spent in the host half of rewards() (token lists -> word rows), accumulated

    def _vectors(self, W, L, head):
        return ngram_vectors(self.lib, self.dev, W, L, self.bos, self.eos, self.df_keys, self.idf, self.n_df, self.idf_unseen, head)

    def rewards(self, candidates_per_image, references_per_image):
        """candidates_per_image / references_per_image: per image a list of token lists (<BOS> / <EOS> / PAD are dropped).  Returns
        float64 [sum of candidates]: each candidate's CIDEr-D, the mean over its image's references (vc_consensus_score with k = 1 and
        the references as the pool, as CaptionEvaluator._cider).  A candidate without words has reward 0."""
        import time
        t0 = time.perf_counter()
        rows = reward_rows(candidates_per_image, references_per_image, self.bos, self.eos)
        if rows is None:
            return np.zeros(0, np.float64)
        self.host_seconds += time.perf_counter() - t0
        return self.rewards_rows(rows)

    def rewards_rows(self, rows):
        """the device half of rewards() on the word rows reward_rows made (with this reward's bos / eos)"""
        B, Lc = rows.B, rows.Lc
        rv = self._vectors(rows.Wr, rows.Lr, np.concatenate([rows.ref_off, np.arange(B)]))   # head: img_cap [B + 1], nbr [B, 1]
        cv = self._vectors(rows.Wc, Lc, rows.cand_off)
        out = torch.empty(max(1, cv.n), dtype=torch.float64, device=self.dev)
        self.lib.vc_consensus_score(_stream(), B, 1, P(rv.head[B + 1:]), P(rv.head[:B + 1]), P(rv.off), P(rv.nnz), P(rv.keys), P(rv.w),
                                    P(rv.norm), P(rv.words), P(cv.head), rows.max_cands, P(cv.off), P(cv.nnz), P(cv.keys), P(cv.w),
                                    P(cv.norm), P(cv.words), MAX_POOL, P(out))
        r = out.cpu().numpy()[:cv.n].copy()
        r[Lc == 0] = 0.0
        return r


def reward_rows(candidates_per_image, references_per_image, bos, eos):
    """Host half of a reward: the checks and limits every reward shares, and the token lists as word rows (consensus.word_rows).
    -> a namespace (B, ref_off / cand_off [B + 1], Wr, Lr, Wc, Lc, max_cands), or None when there is no candidate at all."""
    B = len(candidates_per_image)
    if len(references_per_image) != B:
        raise ValueError("%d images of candidates for %d images of references" % (B, len(references_per_image)))
    per_c = np.fromiter((len(c) for c in candidates_per_image), np.int64, B)
    per_r = np.fromiter((len(r) for r in references_per_image), np.int64, B)
    if B == 0 or per_c.sum() == 0:
        return None
    if per_r.min() < 1:
        raise ValueError("image %d has no reference caption" % int(np.argmin(per_r)))
    if per_r.max() > MAX_POOL or per_c.max() > DIVERSE_MAX_DRAWS:
        raise ValueError("at most %d references and %d candidates per image" % (MAX_POOL, DIVERSE_MAX_DRAWS))
    ref_off, cand_off = np.zeros(B + 1, np.int64), np.zeros(B + 1, np.int64)
    ref_off[1:], cand_off[1:] = np.cumsum(per_r), np.cumsum(per_c)
    Wr, Lr = word_rows([r for rs in references_per_image for r in rs], bos, eos, owner=lambda i: "reference row %d" % i)
    Wc, Lc = word_rows([c for cs in candidates_per_image for c in cs], bos, eos, owner=lambda i: "candidate row %d" % i)
    return types.SimpleNamespace(B=B, ref_off=ref_off, cand_off=cand_off, Wr=Wr, Lr=Lr, Wc=Wc, Lc=Lc, max_cands=int(per_c.max()),
                                 image_of=np.repeat(np.arange(B), per_c))


class RougeReward(object):
    """Per-caption ROUGE-L (coco-caption's definition, beta = 1.2: evaluate.rouge_l) against given references -- the duck type of
    CiderReward, with its limits and its error messages for bad input.  It needs no corpus: the LCS counts come from vc_lcs_overlap on
    the word rows of the step's candidates and references, the score from float64 arithmetic on those integers on the host.
    lib_or_engine: the C-ABI library (abi.load()) or a CaptionEngine (its library and device)."""

    def __init__(self, lib_or_engine, bos, eos, beta=1.2):
        self.lib, self.dev = library_and_device(lib_or_engine)
        self.bos, self.eos, self.beta = int(bos), int(eos), float(beta)
        self.host_seconds = 0.0   # as CiderReward: the host half of rewards() (token lists -> word rows), accumulated

    def rewards(self, candidates_per_image, references_per_image):
        """As CiderReward.rewards: float64 [sum of candidates], each candidate's ROUGE-L against its image's references (precision and
        recall take their maxima over the references separately).  A candidate without words has reward 0."""
        import time
        t0 = time.perf_counter()
        rows = reward_rows(candidates_per_image, references_per_image, self.bos, self.eos)
        if rows is None:
            return np.zeros(0, np.float64)
        self.host_seconds += time.perf_counter() - t0
        return self.rewards_rows(rows)

    def rewards_rows(self, rows):
        """the device half of rewards() on the word rows reward_rows made (with this reward's bos / eos)"""
        from . import evaluate as ev
        C, img = int(rows.Lc.size), rows.image_of
        rng = np.stack([rows.ref_off[img], rows.ref_off[img + 1], np.full(C, -1)]).astype(np.int32)
        hyp = ev.word_table(self.dev, rows.Wc, rows.Lc, head=rng)     # one upload per table; the ranges ride with the candidates
        ref = ev.word_table(self.dev, rows.Wr, rows.Lr)
        out = torch.empty(ev.LCS_COLS * C, dtype=torch.int32, device=self.dev)
        ev._launch_lcs(self.lib, hyp, ref, hyp.head, out)
        o = ev._split_lcs(out.cpu().numpy(), C)
        return ev.rouge_l(o["lcs_max"], o["rec_lcs"], o["rec_len"], rows.Lc, self.beta)


class SumReward(object):
    """The weighted sum of rewards: parts = [(reward, weight), ...], each reward an object with rewards(candidates_per_image,
    references_per_image) and host_seconds (CiderReward, RougeReward).  When every part can work on prepared word rows (it has
    rewards_rows) and the parts agree on <BOS> / <EOS>, the token lists are turned into word rows ONCE per call and shared; otherwise
    each part does its own conversion.  host_seconds: the sum over the parts, plus the shared conversion's own time."""

    def __init__(self, parts):
        self.parts = [(r, float(w)) for r, w in parts]
        if not self.parts:
            raise ValueError("a sum of rewards needs at least one part")
        marks = set((getattr(r, "bos", None), getattr(r, "eos", None)) for r, _ in self.parts)
        self.shared = all(hasattr(r, "rewards_rows") for r, _ in self.parts) and len(marks) == 1 and None not in next(iter(marks))
        self._own_seconds = 0.0

    @property
    def host_seconds(self):
        return self._own_seconds + sum(r.host_seconds for r, _ in self.parts)

    @host_seconds.setter
    def host_seconds(self, value):
        self._own_seconds = float(value)
        for r, _ in self.parts:
            r.host_seconds = 0.0

    def rewards(self, candidates_per_image, references_per_image):
        if self.shared:
            import time
            t0 = time.perf_counter()
            first = self.parts[0][0]
            rows = reward_rows(candidates_per_image, references_per_image, first.bos, first.eos)
            if rows is None:
                return np.zeros(0, np.float64)
            self._own_seconds += time.perf_counter() - t0
            each = [r.rewards_rows(rows) for r, _ in self.parts]
        else:
            each = [r.rewards(candidates_per_image, references_per_image) for r, _ in self.parts]
        total = np.zeros(np.asarray(each[0]).shape, np.float64)
        for (_, w), x in zip(self.parts, each):
            total = total + w * np.asarray(x, np.float64)
        return total
