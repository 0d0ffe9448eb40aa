"""`Decoder` with the constructor, attributes and methods of vae_model/decoder.py:10-320:
px_z_fi (training graph), online_inference (greedy / sampling) and beam_search, executed on the GPU
by engine.CaptionEngine and generate.CaptionGenerator (all images and beams batched per step)."""
import numpy as np

from .. import session, spec
from ..decode_host import merge_groups, rerank_by_marginal
from ..generate import CaptionGenerator


DECODE_METHODS = {"greedy": "online_inference", "sample": "online_inference", "beam_search": "beam_search", "diverse": "diverse_inference",
                  "diverse_beam": "diverse_beam_search", "stochastic_beam": "stochastic_beam_search", "marginal_greedy": "marginal_inference",
                  "marginal_beam": "marginal_inference", "constrained_beam": "constrained_beam_search",
                  "contrastive": "contrastive_search"}   # decode mode -> the method that runs it
DIVERSE_FILE_MODES = ("diverse", "diverse_beam", "stochastic_beam")   # their full per-image lists are also written to val_{gen_name}_diverse.json


class Decoder(object):
    def __init__(self, images_fv, captions, lengths, params, data_dict):
        """images_fv: layers.dense(..., name='imf_emb'); captions: cap_dec [N, T] int (`<BOS>...`, 0-padded); lengths [N]
        (vae_model/decoder.py:13-20).  Arrays given here are what the step runs on (session.bind)."""
        from .encoder import check_images_fv
        check_images_fv(images_fv)
        session.stage(params, owner='decoder', cap_dec=captions, lengths=lengths)
        self.images_fv = images_fv
        self.captions = captions
        self.lengths = lengths
        self.params = params
        self.data_dict = data_dict  # needs .word2idx / .idx2word / .vocab_size
        self.c_i = None
        self.c_i_ph = None
        self.cap_clusters = None
        self.consensus_index = None  # consensus.ConsensusIndex: --diverse_rerank consensus re-ranks diverse captions against it
        self.mbr = None              # mbr.CiderGram: --diverse_rerank mbr re-ranks diverse captions by their expected CIDEr-D against the set;
                                     # --diverse_select dpp selects from them by the same in-set CIDEr-D matrix
        self.last_token_ids = None   # per image of the last generation call its ranked token-id lists (what --eval_captions evaluates);
                                     # every generation method clears it first, so a call that fails leaves None, never older ids
        self.last_ranked_records = None   # --diverse_select dpp: the records of the last call's whole ranked lists, as a run without the
                                     # flag returns them (what ./val_{gen_name}.json is written from, so that the flag never changes that file)
        self.bound_stats = None      # bound_captions: skipped images and the running sums behind the active-units count
        self.constraints = None      # constraints.Constraints: what --sample_gen constrained_beam makes the captions mention
        self.controls = None         # controls.DecodeControls: what the captions may NOT say (--no_repeat_ngram, --min_len, --repetition_penalty,
                                     # --banned_words); every generation method but marginal_inference passes it to its decoder
        self.train_captions = None   # flat token-id lists of the training captions: `novel` of caption_evaluator (None: not reported)

    def px_z_fi(self, observed, gen_mode=False):
        """Training graph: returns (model, x_logits, shpe, (initial_state, final_state, sample)) like
        decoder.py:143.  `observed` = {'z': qz} or {} (--no_encoder); the z actually used is the
        encoder's sample held by the shared engine (zs.BayesianNet(observed) semantics)."""
        if gen_mode:
            raise ValueError("generation runs through online_inference / beam_search")
        tr = session.get(self.params)
        eng = tr.cap
        if session.staged(self.params) and not eng.enc:   # --no_encoder: no q_net ran, this is the first stage of the step
            if self.c_i_ph is not None:
                session.stage(self.params, owner='decoder', c_v=self.c_i_ph)
            feats = session.bind(self.params)
            if tr.vgg is not None and tr.vgg.wd:
                tr.vgg.reg_sumsq(eng.red.data_ptr() + 12)
            eng.fw_prepare(feats)
        logits = eng.fw_decode_train()   # (with --sched_sampling: both decoder passes; the logits are those of the mixed inputs)
        nid = eng.n_init_d
        hs, cs = eng.buf["hs_d"], eng.buf["cs_d"]
        shpe = (tuple(eng.buf["z"].shape) if eng.enc else (), (eng.T * eng.N, self.params.decoder_hidden),
                (eng.N, eng.T, self.params.decoder_hidden))
        return None, logits, shpe, ((cs[nid], hs[nid]), (cs[-1], hs[-1]), None)

    # ------------------------------------------------------------------ generation
    def _gen(self):
        tr = session.get(self.params)
        g = getattr(tr, "_generator", None)
        if g is None:
            g = tr._generator = CaptionGenerator(tr.cap)
        return g

    def _features(self, in_pictures):
        tr = session.get(self.params)
        a = np.asarray(in_pictures, np.float32)
        if a.ndim == 4:  # raw images: run the fine-tuned feature extractor (ops/inference.py:9-12)
            import torch
            return tr.vgg.forward(torch.from_numpy(a).cuda())
        return a.reshape(a.shape[0], -1)

    def _call(self, c_v, stop_word="<EOS>"):
        """(bos, eos, use_cv) of a generation call: the two token ids and the cluster vectors the model takes (None when it takes none)"""
        w2i = self.data_dict.word2idx
        return w2i["<BOS>"], w2i[stop_word], (c_v if (spec.uses_ci(self.params) and c_v is not None and len(c_v)) else None)

    def _text(self, tokens, skip):
        """token ids as a caption's text, without the ids in `skip` (<BOS>, <EOS>)"""
        return " ".join(self.data_dict.idx2word[t] for t in tokens if t not in skip)

    def _ranked_record(self, pid, entries, skip, counts, extra=(), rerank="likelihood", picked=None):
        """diverse_inference's record of an image's ranked entries (tokens, score, .., [the re-ranking's own value]), `extra` items after it.
        picked = (the ranked list's first tokens or None, n_dpp) under --diverse_select dpp: `entries` are then the selected ones in
        selection order, each ending in its gain; "caption" stays the ranked list's first and the record gains "dpp_gain" (aligned
        with "captions") and "dpp_chosen"."""
        texts = [self._text(e[0], skip) for e in entries]
        rec = {"image_id": pid, "caption": texts[0] if texts else "", "captions": texts, "scores": [float(e[1]) for e in entries], "counts": counts}
        rec.update(extra)
        if rerank in ("consensus", "marginal", "mbr"):
            rec[rerank] = [float(e[3]) for e in entries]
        if picked is not None:
            first, chosen = picked
            rec["caption"] = self._text(first, skip) if first is not None else ""
            rec["dpp_gain"] = [float(e[-1]) for e in entries]
            rec["dpp_chosen"] = int(chosen)
        return rec

    def _rerank(self):
        """params.diverse_rerank: "likelihood", "consensus" (RuntimeError without an attached consensus index), "marginal" or "mbr"
        (RuntimeError without an attached mbr.CiderGram)"""
        mode = getattr(self.params, "diverse_rerank", "likelihood")
        if mode == "consensus" and self.consensus_index is None:
            raise RuntimeError("diverse_rerank = 'consensus' needs a consensus index: attach one with decoder.consensus_index = "
                               "vae_captioning_amd.consensus.ConsensusIndex(engine, train_features, train_captions, bos, eos)")
        if mode == "mbr" and self.mbr is None:
            raise RuntimeError("diverse_rerank = 'mbr' needs the idf of the training captions: attach one with decoder.mbr = "
                               "vae_captioning_amd.mbr.CiderGram(engine, train_captions_per_image, bos, eos)")
        return mode

    def _select(self):
        """params.diverse_select: None ("none"), or (select_n, dpp_quality) for "dpp" (RuntimeError without an attached mbr.CiderGram)"""
        if getattr(self.params, "diverse_select", "none") != "dpp":
            return None
        if self.mbr is None:
            raise RuntimeError("diverse_select = 'dpp' needs the idf of the training captions: attach one with decoder.mbr = "
                               "vae_captioning_amd.mbr.CiderGram(engine, train_captions_per_image, bos, eos)")
        return int(getattr(self.params, "select_n", 5)), float(getattr(self.params, "dpp_quality", 1.0))

    def _dpp(self, ranked, select):
        """--diverse_select dpp on every image's ranked entries -> (the selected entries in selection order, each ending in its gain;
        per image `picked` for _ranked_record: the ranked list's first tokens and how many entries the greedy steps chose)"""
        chosen, n_dpp = self.mbr.select(ranked, select[0], quality=select[1])
        return chosen, [(entries[0][0] if entries else None, k) for entries, k in zip(ranked, n_dpp)]

    def decode(self, mode, picture_ids, in_pictures, c_v=None, sess=None, placeholder=None, **overrides):
        """The cap_list of a batch in decode mode `mode` (params.sample_gen, gen_caption's gen_method) from the mode's method (DECODE_METHODS),
        which gets `overrides` (draws=, beam_size=, ...) in place of its params defaults; beam_search's width defaults to params.beam_size.
        "greedy", "sample" and, as in the reference, any other name: online_inference, which decodes as params.sample_gen says (so does
        marginal_inference unless method= is given).  sess / placeholder: the reference's arguments, passed through."""
        name = DECODE_METHODS.get(mode, "online_inference")
        if name == "online_inference":
            return self.online_inference(sess, picture_ids, in_pictures, placeholder, c_v=c_v)[0]
        if mode == "beam_search" and "beam_size" not in overrides:
            overrides["beam_size"] = self.params.beam_size
        return getattr(self, name)(sess, picture_ids, in_pictures, placeholder, c_v, **overrides)

    def _cuts(self):
        """params.typical_p / min_p / eta as sample()'s and diverse()'s keywords (a params object pickled by an older run has none: off)"""
        return dict(typical_p=getattr(self.params, "typical_p", 1.0), min_p=getattr(self.params, "min_p", 0.0), eta=getattr(self.params, "eta", 0.0))

    def online_inference(self, sess, picture_ids, in_pictures, image_f_inputs, stop_word="<EOS>", c_v=None):
        """decoder.py:145-201.  Returns (cap_list, cap_raw)."""
        self.last_token_ids = None
        bos, eos, use_cv = self._call(c_v, stop_word)
        if self.params.sample_gen == "sample":  # tf.multinomial(logits / temperature): same distribution, own Philox stream
            raw = self._gen().sample(self._features(in_pictures), use_cv, None, bos, eos, self.params.gen_max_len,
                                     top_k=getattr(self.params, "top_k", 0), top_p=getattr(self.params, "top_p", 1.0), controls=self.controls, **self._cuts())
        else:
            raw = self._gen().greedy(self._features(in_pictures), use_cv, None, bos, eos, self.params.gen_max_len, controls=self.controls)
        cap_list = [{"image_id": pid, "caption": self._text(toks, (bos, eos))} for pid, toks in zip(picture_ids, raw)]
        self.last_token_ids = [[list(toks)] for toks in raw]
        return cap_list, raw

    def beam_search(self, sess, picture_ids, in_pictures, image_f_inputs, c_v=None, beam_size=2, ret_beams=False,
                    len_norm_f=0.7):
        """decoder.py:203-320.  Returns cap_list."""
        self.last_token_ids = None
        bos, eos, use_cv = self._call(c_v)
        res = self._gen().beam_search(self._features(in_pictures), use_cv, None, bos, eos, beam_size,
                                      self.params.gen_max_len, len_norm_f, controls=self.controls)
        cap_list = []
        for pid, beams in zip(picture_ids, res):
            texts = [self._text(s, (bos, eos)) for s, _ in beams]
            cap_list.append({"image_id": pid, "caption": texts if ret_beams else texts[0]})
        self.last_token_ids = [[list(s) for s, _ in (beams if ret_beams else beams[:1])] for beams in res]
        return cap_list

    def diverse_inference(self, sess, picture_ids, in_pictures, image_f_inputs, c_v=None, draws=None, method=None, n_best=None,
                          len_norm_f=0.7):
        """Diverse captioning (the purpose of z in the AG-CVAE paper): `draws` latent draws per image (params.diverse_draws), each decoded
        with `method` (params.diverse_method: greedy or sample; sample honours params.top_k / params.top_p or params.typical_p / min_p / eta), identical captions merged and
        ranked (generate.py: diverse).  Returns
        cap_list: per image {"image_id", "caption": the best text, "captions": [texts], "scores": [...], "counts": [...]}.
        params.diverse_rerank == "consensus": every distinct caption is re-ranked by its consensus against the attached
        `consensus_index` (consensus.py) before n_best cuts the list; the records gain "consensus" (aligned with "captions") and
        "caption" is the consensus winner.  params.diverse_rerank == "marginal": the distinct captions are ordered by their likelihood
        over ALL draws of the image (generate.py: diverse(rerank="marginal")); "scores" are those scores and the records gain "marginal"
        (aligned with "captions").  params.diverse_rerank == "mbr": every distinct caption is re-ranked by its expected CIDEr-D against
        the image's own captions, each weighted by its count (the attached `mbr`: mbr.CiderGram), before n_best cuts the list; the
        records gain "mbr" (aligned with "captions") and "caption" is the minimum-Bayes-risk choice.
        params.diverse_select == "dpp": after the re-ranking and in place of the n_best cut, params.select_n captions are chosen from the
        whole ranked list jointly for quality and difference (the attached `mbr`: CiderGram.select, quality weight params.dpp_quality);
        "captions" and the fields aligned with it hold them in selection order, the records gain "dpp_gain" (aligned) and "dpp_chosen",
        and "caption" stays the ranked list's first."""
        self.last_token_ids = None
        bos, eos, use_cv = self._call(c_v)
        draws = int(draws if draws is not None else self.params.diverse_draws)
        method = method if method is not None else self.params.diverse_method
        rerank = self._rerank()
        select = self._select()
        self.last_ranked_records = None
        if select is not None:
            n_best = None
        consensus, marginal, mbr = rerank == "consensus", rerank == "marginal", rerank == "mbr"
        feats = self._features(in_pictures)
        res = self._gen().diverse(feats, use_cv, None, bos, eos, draws=draws, method=method, n_best=None if consensus or mbr else n_best,
                                  max_len=self.params.gen_max_len, len_norm_f=len_norm_f, rerank="marginal" if marginal else "likelihood",
                                  top_k=getattr(self.params, "top_k", 0), top_p=getattr(self.params, "top_p", 1.0), controls=self.controls, **self._cuts())
        if consensus:
            res = self.consensus_index.rerank(feats, res, n_best=n_best)
        if mbr:
            res = self.mbr.rerank(res, n_best=n_best)     # weights: the counts

        def records(lists, picked):
            return [self._ranked_record(pid, entries, (bos, eos), [int(e[2]) for e in entries], rerank=rerank, picked=pk)
                    for pid, entries, pk in zip(picture_ids, lists, picked)]
        picked = [None] * len(res)
        if select is not None:
            self.last_ranked_records = records(res, picked)
            res, picked = self._dpp(res, select)
        cap_list = records(res, picked)
        self.last_token_ids = [[list(e[0]) for e in entries] for entries in res]
        return cap_list

    def diverse_beam_search(self, sess, picture_ids, in_pictures, image_f_inputs, c_v=None, beam_size=None, groups=None, diversity=None,
                            len_norm_f=0.7):
        """Group beam search (Diverse Beam Search; generate.py: diverse_beam_search): `groups` (params.beam_groups) beam searches of
        beam_size / groups beams per image (params.beam_size in all), a word costing a candidate `diversity` (params.beam_diversity)
        per live beam of the round's earlier groups that has just taken it.  Equal captions of different groups are merged under
        their best score and ranked.  Returns cap_list in diverse_inference's record shape: per image {"image_id", "caption": the
        best text, "captions": [texts], "scores": [...], "counts": [groups that produced the caption], "groups": [[group ids]]}.
        params.diverse_select == "dpp" selects from the merged list as diverse_inference does."""
        self.last_token_ids = None
        bos, eos, use_cv = self._call(c_v)
        select = self._select()
        self.last_ranked_records = None
        total = int(beam_size if beam_size is not None else self.params.beam_size)
        G = int(groups if groups is not None else self.params.beam_groups)
        lam = float(diversity if diversity is not None else self.params.beam_diversity)
        if G < 1 or total < G or total % G or total > 16:
            raise ValueError("diverse_beam_search: beam_size must be a multiple of groups and at most 16 (got %d and %d)" % (total, G))
        res = self._gen().diverse_beam_search(self._features(in_pictures), use_cv, None, bos, eos, groups=G, group_size=total // G,
                                              diversity=lam, max_len=self.params.gen_max_len, len_norm_f=len_norm_f,
                                              controls=self.controls)
        merged = [merge_groups(per_group) for per_group in res]

        def records(lists, picked):
            return [self._ranked_record(pid, entries, (bos, eos), [len(e[2]) for e in entries], {"groups": [[int(g) for g in e[2]] for e in entries]}, picked=pk)
                    for pid, entries, pk in zip(picture_ids, lists, picked)]
        picked = [None] * len(merged)
        if select is not None:
            self.last_ranked_records = records(merged, picked)
            merged, picked = self._dpp(merged, select)
        cap_list = records(merged, picked)
        self.last_token_ids = [[list(e[0]) for e in entries] for entries in merged]
        return cap_list

    def stochastic_beam_search(self, sess, picture_ids, in_pictures, image_f_inputs, c_v=None, beam_size=None, len_norm_f=0.7):
        """Stochastic beam search (Kool et al. 2019; generate.py: stochastic_beam_search): beam_size (params.beam_size, 1..32) distinct
        captions per image, sampled without replacement from the model, each with its exact log-probability and importance weight.
        Returns cap_list in diverse_inference's record shape, ranked as vc_diverse_rank ranks (<EOS>-ended first, then logprob /
        (1 + len)^len_norm_f descending): per image {"image_id", "caption", "captions", "scores", "counts" (all 1: the captions are
        distinct), "logprob", "perturbed", "weight", "norm_weight" (aligned with "captions"), "kappa"}.  params.diverse_rerank ==
        "consensus" re-ranks by the attached consensus index and adds "consensus"; "marginal" adds "marginal" (one latent draw per
        image: the caption's logprob, so the order is the likelihood order); "mbr" re-ranks by the expected CIDEr-D against the image's
        captions, each weighted by its norm_weight (the weights that estimate an expectation under the model), and adds "mbr".
        params.diverse_select == "dpp" selects from the ranked list as diverse_inference does; the aligned per-caption fields follow
        the selection."""
        self.last_token_ids = None
        bos, eos, use_cv = self._call(c_v)
        n = int(beam_size if beam_size is not None else self.params.beam_size)
        rerank = self._rerank()
        select = self._select()
        self.last_ranked_records = None
        consensus, marginal = rerank == "consensus", rerank == "marginal"
        feats = self._features(in_pictures)
        res = self._gen().stochastic_beam_search(feats, use_cv, None, bos, eos, beam_size=n, max_len=self.params.gen_max_len,
                                                 len_norm_f=len_norm_f, controls=self.controls)
        ranked = []
        for r in res:
            caps = sorted(r["captions"], key=lambda c: (not c[3], -(c[1] / (1 + len(c[0])) ** len_norm_f)))
            ranked.append([(list(c[0]), c[1] / (1 + len(c[0])) ** len_norm_f, 1) for c in caps])
        if consensus:
            ranked = self.consensus_index.rerank(feats, ranked)
        by_words = [{tuple(c[0]): c for c in r["captions"]} for r in res]
        if rerank == "mbr":
            ranked = self.mbr.rerank(ranked, weights=[[float(by[tuple(e[0])][5]) for e in entries] for entries, by in zip(ranked, by_words)])
        if marginal:
            ranked = [rerank_by_marginal(entries, [by[tuple(e[0])][1] for e in entries], eos, len_norm_f) for entries, by in zip(ranked, by_words)]

        def records(lists, picked):
            out = []
            for pid, entries, r, by, pk in zip(picture_ids, lists, res, by_words, picked):
                own = [by[tuple(e[0])] for e in entries]
                extra = {"logprob": [float(c[1]) for c in own], "perturbed": [float(c[2]) for c in own], "weight": [float(c[4]) for c in own],
                         "norm_weight": [float(c[5]) for c in own], "kappa": float(r["kappa"])}
                out.append(self._ranked_record(pid, entries, (bos, eos), [1] * len(entries), extra, rerank, picked=pk))
            return out
        picked = [None] * len(ranked)
        if select is not None:
            self.last_ranked_records = records(ranked, picked)
            ranked, picked = self._dpp(ranked, select)
        cap_list = records(ranked, picked)
        self.last_token_ids = [[list(e[0]) for e in entries] for entries in ranked]
        return cap_list

    def constrained_beam_search(self, sess, picture_ids, in_pictures, image_f_inputs, c_v=None, constraints=None, beam_size=None,
                                len_norm_f=0.7):
        """Constrained beam search (Anderson et al. 2017; generate.py: constrained_beam_search): captions that must mention given words.
        `constraints`: per image a list of at most 3 sets of at most 4 token ids (default: self.constraints.for_images(picture_ids)); a
        set is satisfied once any of its words is in the caption.  beam_size: beams per state (default: self.constraints.width, else the
        largest that fits, 16 >> the largest number of sets).  Returns cap_list: per image {"image_id", "caption", "constraints": the ids
        used, "satisfied": one bool per constraint, "score"} -- the best caption of the state with the most constraints met."""
        self.last_token_ids = None
        bos, eos, use_cv = self._call(c_v)
        if constraints is None:
            if self.constraints is None:
                raise RuntimeError("constrained_beam_search needs constraints: pass them or attach decoder.constraints = "
                                   "vae_captioning_amd.constraints.load_constraints(...)")
            constraints = self.constraints.for_images(picture_ids)
        if beam_size is None:
            beam_size = self.constraints.width if self.constraints is not None else 16 >> max([len(c) for c in constraints] + [0])
        res = self._gen().constrained_beam_search(self._features(in_pictures), constraints, use_cv, None, bos, eos, beam_size=int(beam_size),
                                                  max_len=self.params.gen_max_len, len_norm_f=len_norm_f, controls=self.controls)
        cap_list, token_ids = [], []
        for pid, sets, (beams, state) in zip(picture_ids, constraints, res):
            toks, score = (list(beams[0][0]), float(beams[0][1])) if beams else ([], float("-inf"))
            token_ids.append([toks])
            cap_list.append({"image_id": pid, "caption": self._text(toks, (bos, eos)),
                             "constraints": [[int(v) for v in st] for st in sets],
                             "satisfied": [bool((state >> j) & 1) for j in range(len(sets))], "score": score})
        self.last_token_ids = token_ids
        return cap_list

    def contrastive_search(self, sess, picture_ids, in_pictures, image_f_inputs, c_v=None, k=None, alpha=None):
        """Contrastive search (Su et al. 2022; generate.py: contrastive_search): every round the `k` (params.contrastive_k, 1..16) most
        likely next words are looked one decoder step ahead, and the word taken is likely and leads to a decoder state unlike those of
        the caption so far, weighted by `alpha` (params.contrastive_alpha, in [0, 1]; 0 = greedy).  Deterministic.  Returns cap_list:
        per image {"image_id", "caption", "logprob": the log-probability of the caption's words}."""
        self.last_token_ids = None
        bos, eos, use_cv = self._call(c_v)
        k = int(k if k is not None else getattr(self.params, "contrastive_k", 5))
        alpha = float(alpha if alpha is not None else getattr(self.params, "contrastive_alpha", 0.6))
        res = self._gen().contrastive_search(self._features(in_pictures), use_cv, None, bos, eos, k=k, alpha=alpha,
                                             max_len=self.params.gen_max_len, controls=self.controls)
        cap_list = [{"image_id": pid, "caption": self._text(toks, (bos, eos)), "logprob": float(lp)} for pid, (toks, lp) in zip(picture_ids, res)]
        self.last_token_ids = [[list(toks)] for toks, _ in res]
        return cap_list

    def marginal_inference(self, sess, picture_ids, in_pictures, image_f_inputs, c_v=None, method=None, draws=None, beam_size=None,
                           len_norm_f=0.7):
        """Decoding under the mixture of `draws` (params.marginal_draws) latent draws per image (generate.py: marginal_greedy /
        marginal_beam_search): `method` (params.sample_gen) "marginal_greedy" takes the mixture's best word every round,
        "marginal_beam" runs a beam search of beam_size (params.beam_size) hypotheses over it.  Returns cap_list: per image
        {"image_id", "caption", "marginal": log 1/K sum_k p(caption | z_k, image) as the decoder accumulated it, "draws": K}."""
        self.last_token_ids = None
        if self.controls is not None and not self.controls.is_noop():
            raise ValueError("marginal_inference takes no decoding controls: renormalising every draw's distribution would break the "
                             "mode's identity with score()'s marginal")
        bos, eos, use_cv = self._call(c_v)
        method = method if method is not None else self.params.sample_gen
        K = int(draws if draws is not None else self.params.marginal_draws)
        feats = self._features(in_pictures)
        if method == "marginal_greedy":
            res = self._gen().marginal_greedy(feats, use_cv, None, bos, eos, draws=K, max_len=self.params.gen_max_len)
            toks, marg = [r["tokens"] for r in res], [r["marginal"] for r in res]
        elif method == "marginal_beam":
            n = int(beam_size if beam_size is not None else self.params.beam_size)
            res = self._gen().marginal_beam_search(feats, use_cv, None, bos, eos, draws=K, beam_size=n, max_len=self.params.gen_max_len,
                                                   len_norm_f=len_norm_f)
            toks, marg = [], []
            for beams in res:   # a finished caption's score is logprob / len**len_norm_f (decoder.py:285-286), a cut one's its logprob
                s, sc = beams[0]
                toks.append(list(s))
                marg.append(sc * len(s) ** len_norm_f if (s and s[-1] == eos and len_norm_f > 0) else sc)
        else:
            raise ValueError("marginal_inference: method must be 'marginal_greedy' or 'marginal_beam' (got %r)" % (method,))
        cap_list = [{"image_id": pid, "caption": self._text(s, (bos, eos)), "marginal": float(m), "draws": K}
                    for pid, s, m in zip(picture_ids, toks, marg)]
        self.last_token_ids = [[list(s)] for s in toks]
        return cap_list

    def score_captions(self, picture_ids, in_pictures, captions, c_v=None, draws=None):
        """Held-out likelihood of given captions (generate.py: score): captions[b] = token-id lists of image b (with or without <BOS>; the
        <EOS> counts when present), scored under `draws` (params.score_draws) prior draws.  Returns per image {"image_id", "captions":
        [{"tokens": n, "marginal": log 1/K sum_k p(caption | z_k, image), "logprob": mean over the draws of log p(caption | z_k, image)}]}."""
        bos, eos, use_cv = self._call(c_v)
        draws = int(draws if draws is not None else self.params.score_draws)
        res = self._gen().score(self._features(in_pictures), captions, use_cv, None, bos, eos, draws=draws)
        return [{"image_id": pid, "captions": [{"tokens": int(r["tokens"]), "marginal": float(r["marginal"]), "logprob": float(np.mean(r["logprob"]))}
                                               for r in rs]} for pid, rs in zip(picture_ids, res)]

    def bound_captions(self, picture_ids, in_pictures, captions, c_v=None, draws=None):
        """Variational bounds on the likelihood of given captions with the model's posterior as proposal (generate.py: bound): captions as
        score_captions takes them, `draws` (params.bound_draws) posterior draws per caption.  Returns per image {"image_id", "captions":
        [{"tokens", "elbo", "iwae", "rec", "kl", "ess"}]}.  GMM prior: every caption's mixture component is drawn here from its image's
        normalised cluster vector (encoder.py:72-75 draws it per training row), by a generator seeded from params.seed that lives as long
        as this decoder.  AG / GMM: an image with an empty cluster vector has no posterior; it is left out and counted in
        self.bound_stats["skipped_images"].  bound_stats also keeps running float64 sums of the posterior means and their squares per
        latent dimension over every caption scored ("mu_sum", "mu_sq", "captions"): what ops.inference.active_units reads.  With
        params.bound_mi = N > 0 it also keeps the posteriors (mean, std) of the first N captions scored ("mi_mean", "mi_std": lists of
        float32 [L] rows; under the GMM prior the head of the component drawn here), which ops.inference.store_bounds hands to
        latent_mi.mutual_information."""
        bos, eos, use_cv = self._call(c_v)
        p = self.params
        use_cv = np.asarray(use_cv, np.float32) if use_cv is not None else None
        draws = int(draws if draws is not None else p.bound_draws)
        feats = self._features(in_pictures)
        st = self.bound_stats
        if st is None:
            L = p.latent_size
            st = self.bound_stats = {"skipped_images": 0, "captions": 0, "mu_sum": np.zeros(L, np.float64), "mu_sq": np.zeros(L, np.float64),
                                     "rng": np.random.default_rng(p.seed)}
            if int(getattr(p, "bound_mi", 0) or 0) > 0:
                st.update(mi_mean=[], mi_std=[])
        keep = list(range(len(picture_ids)))
        if p.prior in ("AG", "GMM") and use_cv is not None:
            keep = [b for b in keep if use_cv[b].any()]
            st["skipped_images"] += len(picture_ids) - len(keep)
        if not keep:
            return []
        caps = [captions[b] for b in keep]
        gmm_idx = None
        if p.prior == "GMM":
            gmm_idx = []
            for b, cl in zip(keep, caps):
                w = np.maximum(use_cv[b].astype(np.float64), 0.0)
                gmm_idx += st["rng"].choice(w.size, size=len(cl), p=w / w.sum()).tolist()
            gmm_idx = np.asarray(gmm_idx, np.int32)
        res = self._gen().bound(feats[keep], caps, use_cv[keep] if use_cv is not None else None, None, gmm_idx, bos, eos, draws=draws,
                                return_latents="stats")
        out = []
        for b, rs in zip(keep, res):
            for r in rs:
                mu = r["mean"].astype(np.float64)
                st["mu_sum"] += mu
                st["mu_sq"] += mu * mu
                st["captions"] += 1
                if "mi_mean" in st and len(st["mi_mean"]) < int(p.bound_mi):
                    st["mi_mean"].append(r["mean"])
                    st["mi_std"].append(r["std"])
            out.append({"image_id": picture_ids[b], "captions": [{k: (int(r[k]) if k == "tokens" else float(r[k]))
                                                                   for k in ("tokens", "elbo", "iwae", "rec", "kl", "ess")} for r in rs]})
        return out

    def caption_evaluator(self, references):
        """evaluate.CaptionEvaluator of the images whose human captions are `references` (per image a list of token-id lists), on this
        decoder's engine and dictionary; `novel` is reported against self.train_captions when those are set."""
        from ..evaluate import CaptionEvaluator
        d = self.data_dict
        return CaptionEvaluator(session.get(self.params).cap, references, d.word2idx["<BOS>"], d.word2idx["<EOS>"],
                                vocab_size=d.vocab_size, train_captions=self.train_captions)
