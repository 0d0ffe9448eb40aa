"""Caption the validation and test image sets and store them as COCO-style result files.

Counterpart of the reference's `inference(params, decoder, val_gen, test_gen, image_f_inputs, saver, sess)`
(ops/inference.py:4-56): same argument list, same output files -- `./val_{gen_name}.json` and `./test_{gen_name}.json`,
each a list of `{"image_id": ..., "caption": ...}` -- produced by the batched on-device decoders of
`vae_model/decoder.py`.  Validation images use `params.sample_gen` (beam search or greedy / sampling); the test set is
always decoded with `online_inference`, as in the reference.  `sample_gen == "diverse"` (additive): the validation images go through
`diverse_inference`; `./val_{gen_name}.json` keeps the COCO shape with each image's top caption and
`./val_{gen_name}_diverse.json` holds the full per-image lists (captions, scores, counts).  With `params.diverse_rerank ==
"consensus"` (a `consensus.ConsensusIndex` attached to the decoder) the top caption is the consensus winner and the lists also hold
the consensus scores; with `"marginal"` they hold each caption's likelihood over all of the image's draws; with `"mbr"` (an
`mbr.CiderGram` attached to the decoder) the top caption has the highest expected CIDEr-D against the image's own captions and the
lists hold those values under `"mbr"`.
`sample_gen == "diverse_beam"` (additive): group beam search (`decoder.diverse_beam_search`), written the same way: the merged ranked
captions of an image's groups in `./val_{gen_name}_diverse.json`, its best one in `./val_{gen_name}.json`.
`sample_gen == "stochastic_beam"` (additive): stochastic beam search (`decoder.stochastic_beam_search`), written the same way: the
`params.beam_size` distinct captions sampled without replacement for an image, ranked, in `./val_{gen_name}_diverse.json` (each with
its `logprob`, `perturbed` score, `weight` and `norm_weight`, the image with its `kappa`), the first in `./val_{gen_name}.json`.
`sample_gen == "marginal_greedy"` / `"marginal_beam"` (additive): greedy decoding / beam search under the mixture of
`params.marginal_draws` latent draws (`decoder.marginal_inference`); the records of `./val_{gen_name}.json` gain `"marginal"` (the
caption's log-likelihood over the draws) and `"draws"`.
`sample_gen == "constrained_beam"` (additive): constrained beam search (`decoder.constrained_beam_search` with the
`constraints.Constraints` attached to the decoder); the records of `./val_{gen_name}.json` gain `"constraints"` (the token ids used),
`"satisfied"` (one bool per constraint) and `"score"`.
`sample_gen == "contrastive"` (additive): contrastive search (`decoder.contrastive_search`, `params.contrastive_k` /
`params.contrastive_alpha`); the records of `./val_{gen_name}.json` gain `"logprob"` (the log-probability of the caption's words).
`params.score_draws = K >= 1` (additive): the validation images' HUMAN captions are also scored under K prior draws
(`decoder.score_captions`) -> `./val_{gen_name}_scores.json`, and the corpus perplexity exp(-sum marginal / sum tokens) is printed.
`params.bound_draws = K >= 1` (additive): the same human captions are bounded with K draws from the model's own posterior
(`decoder.bound_captions`, generate.py: bound) -> `./val_{gen_name}_bound.json`: a header record {"draws", "skipped_images",
"active_units", "latent_size"}, then per image {"image_id", "captions": [{"tokens", "elbo", "iwae", "rec", "kl", "ess"}]}; five printed
lines: the perplexity bounds exp(-sum iwae / sum tokens) and exp(-sum elbo / sum tokens), the mean KL per caption, the mean effective
sample size over K and the active latent units (Burda et al. 2016: dimensions whose posterior mean varies by more than 0.01 over the
captions).  `params.bound_mi = N >= 1` (additive, with `bound_draws`): the posteriors of the first N bounded captions
(`decoder.bound_stats`) give the mutual information I(x; z) under the aggregated posterior (latent_mi.py: mutual_information, seeded by
`params.seed`) once after the loop; the header gains {"mi", "mi_block", "mi_captions", "mi_ceiling"} and a sixth line is printed.
`params.eval_captions` (additive): what was decoded for the validation images (`decoder.last_token_ids`: the whole ranked list of an
image in the diverse modes, a list of one otherwise) is evaluated against ALL human captions of each image (taken from the generator's
caption table by image id, `validation_references`: the batches carry one random caption per image) (`decoder.caption_evaluator`,
evaluate.py: BLEU, CIDEr-D, oracle and diversity metrics) once after the loop -> `./val_{gen_name}_metrics.json`, one printed line
per metric.  The caption files are written exactly as without the flag.  `params.eval_self_cider` (additive, with `eval_captions`): the
evaluator also makes its in-set CIDEr-D pass (mbr.py, vc_cider_gram) and the file and the printed lines gain `self_cider` and
`mbr_cider_d`.
`params.no_repeat_ngram` / `min_len` / `repetition_penalty` / `banned_words` (additive): the decoding controls
(`controls.DecodeControls`, attached to the decoder as `decoder.controls`) go to whichever mode decodes, the test set's
`online_inference` included; the caption records gain nothing, `./val_{gen_name}_metrics.json` lists the four flags.
`params.diverse_select == "dpp"` (additive; the three list modes): `params.select_n` captions per image are chosen from the ranked
list by the DPP selection (`mbr.CiderGram.select`, attached as `decoder.mbr`); the records of `./val_{gen_name}_diverse.json` hold them
in selection order with `"dpp_gain"` and `"dpp_chosen"`, `./val_{gen_name}.json` keeps the ranked list's first caption, `--eval_captions`
evaluates the selected lists, and `./val_{gen_name}_metrics.json` gains `diverse_select`, `select_n` and `dpp_quality`."""
import json
import math
import os

import numpy as np


def _cluster_rows(c_v, wanted):
    """Batch generator rows are 91-vectors; the model takes columns 1..90 (ops/inference.py:17-19, main.py:236)."""
    if not wanted:
        return c_v
    a = np.asarray(c_v)
    return a[:, 1:] if a.ndim == 2 and a.shape[1] > 0 else a


def _decode(decoder, params, sess, placeholder, ids, images, c_v, allow_beam):
    """Decoder.decode in the mode of params.sample_gen; allow_beam=False (the test set): online_inference, whatever the mode.  (Called
    unbound: `decoder` may be any object with the reference's methods, so the beam width is given here.)"""
    from ..vae_model.decoder import Decoder
    mode = params.sample_gen if allow_beam else "greedy"
    return Decoder.decode(decoder, mode, ids, images, c_v, sess, placeholder, **({"beam_size": params.beam_size} if mode == "beam_search" else {}))


def human_captions(captions, lengths):
    """One validation item's captions as score() takes them: caption c of image b is lab[b, c, :lens[b, c]] (the `w.. <EOS>` label row;
    lab[b, :lens[b]] where the generator yields one caption per image); rows of length 0 (images with fewer captions) are skipped."""
    lab = np.asarray(captions[1])
    lens = np.asarray(lengths)
    if lab.ndim == 2:
        lab, lens = lab[:, None, :], lens.reshape(-1, 1)
    return [[lab[b, c, :int(lens[b, c])].tolist() for c in range(lab.shape[1]) if int(lens[b, c]) > 0] for b in range(lab.shape[0])]


def perplexity(score_records):
    """exp(-sum marginal / sum tokens) over every scored caption (nan when nothing was scored)"""
    caps = [c for r in score_records for c in r["captions"]]
    n = sum(c["tokens"] for c in caps)
    return math.exp(-sum(c["marginal"] for c in caps) / n) if n else float("nan")


def store_scores(params, score_records):
    _store("./val_{}_scores.json".format(params.gen_name), score_records)
    print("Held-out perplexity of the human captions under %d prior draws: %.17g" % (params.score_draws, perplexity(score_records)))


ACTIVE_UNIT_VARIANCE = 0.01   # Burda et al. 2016, section 5.2: a latent dimension is active when Var_x(E_q[z | x]) exceeds this


def active_units(mu_sum, mu_sq, n, threshold=ACTIVE_UNIT_VARIANCE):
    """How many latent dimensions are active: the (population) variance of the posterior mean over the n scored captions, from the running
    float64 sums of mu and mu^2 per dimension, exceeds `threshold`.  0 when nothing was scored."""
    if n <= 0:
        return 0
    m = np.asarray(mu_sum, np.float64) / n
    return int(np.count_nonzero(np.asarray(mu_sq, np.float64) / n - m * m > threshold))


def bound_summary(bound_records, draws):
    """(perplexity bound from iwae, the same from elbo, mean kl per caption, mean ess / draws) over every bounded caption; nan when nothing
    was bounded.  exp(-sum iwae / sum tokens) is an UPPER bound on the model's perplexity in expectation: iwae <= log p(caption | image)."""
    caps = [c for r in bound_records for c in r["captions"]]
    n = sum(c["tokens"] for c in caps)
    if not n:
        return (float("nan"),) * 4
    return (math.exp(-sum(c["iwae"] for c in caps) / n), math.exp(-sum(c["elbo"] for c in caps) / n),
            sum(c["kl"] for c in caps) / len(caps), sum(c["ess"] for c in caps) / (len(caps) * draws))


def mutual_information_of(params, stats):
    """--bound_mi: the MI estimate of the posteriors bound_captions kept in stats ("mi_mean", "mi_std"), params.gen_z_samples draws
    each, seeded by params.seed -> latent_mi.mutual_information's dict; None when the flag is off or no posterior was kept"""
    if not int(getattr(params, "bound_mi", 0) or 0) or not stats.get("mi_mean"):
        return None
    from .. import latent_mi
    return latent_mi.mutual_information(np.stack(stats["mi_mean"]), np.stack(stats["mi_std"]), int(params.gen_z_samples),
                                        seed=int(getattr(params, "seed", 0)))


def store_bounds(params, bound_records, stats):
    """./val_{gen_name}_bound.json and the five printed lines (six with --bound_mi); stats = decoder.bound_stats (None: nothing was
    bounded)"""
    K, L = int(params.bound_draws), int(params.latent_size)
    stats = stats or {"skipped_images": 0, "captions": 0, "mu_sum": np.zeros(L), "mu_sq": np.zeros(L)}
    active = active_units(stats["mu_sum"], stats["mu_sq"], stats["captions"])
    header = {"draws": K, "skipped_images": int(stats["skipped_images"]), "active_units": active, "latent_size": L}
    mi = mutual_information_of(params, stats)
    if mi is not None:
        header.update(mi=float(mi["mi"]), mi_block=float(mi["mi_block"]), mi_captions=int(mi["captions"]), mi_ceiling=float(mi["mi_ceiling"]))
    _store("./val_{}_bound.json".format(params.gen_name), [header] + list(bound_records))
    ppl_iwae, ppl_elbo, kl, ess = bound_summary(bound_records, K)
    print("Perplexity bound of the human captions from the importance-weighted bound, %d posterior draws: %.17g" % (K, ppl_iwae))
    print("Perplexity bound of the human captions from the ELBO, %d posterior draws: %.17g" % (K, ppl_elbo))
    print("Mean KL(q || p) per caption: %.6f nats" % kl)
    print("Mean effective sample size / draws: %.6f" % ess)
    print("Active latent units: %d of %d (%d images without a cluster vector skipped)" % (active, L, header["skipped_images"]))
    if mi is not None:
        print("Mutual information of caption and latent code: mi %.6f nats, mi_block %.6f nats per block (mi_ceiling %.6f = log of "
              "mi_captions %d)" % (header["mi"], header["mi_block"], header["mi_ceiling"], header["mi_captions"]))
    return header


EVAL_FLAGS = ("beam_size", "temperature", "diverse_draws", "diverse_method", "diverse_rerank", "consensus_k", "consensus_m", "beam_groups",
              "beam_diversity", "top_k", "top_p", "typical_p", "min_p", "eta", "marginal_draws", "constraints", "cbs_width",
              "no_repeat_ngram", "min_len", "repetition_penalty", "banned_words", "contrastive_k", "contrastive_alpha")


SELECT_FLAGS = ("diverse_select", "select_n", "dpp_quality")   # recorded only when a selection ran: without one the file is unchanged


def store_metrics(params, metrics, images, captions):
    """./val_{gen_name}_metrics.json: the evaluator's dict without its per-image arrays, the number of images and of captions evaluated,
    sample_gen and the decoding flags in force; one printed line per metric.  With params.eval_self_cider also the two SET_METRICS
    (self_cider, mbr_cider_d) and the flag itself; without it the file and the lines are those of a run that never knew the flag."""
    from ..evaluate import METRICS, SET_METRICS
    names = METRICS + (SET_METRICS if getattr(params, "eval_self_cider", False) else ())
    out = {k: metrics[k] for k in names}
    out.update(images=int(images), captions=int(captions), sample_gen=params.sample_gen)
    out.update({k: getattr(params, k) for k in EVAL_FLAGS if hasattr(params, k)})
    if len(names) > len(METRICS):
        out["eval_self_cider"] = True
    if getattr(params, "use_ema", False):   # --use_ema: the captions come from the averaged weights
        out["use_ema"] = True
    if getattr(params, "diverse_select", "none") != "none":   # --diverse_select dpp: the lists evaluated are the selected ones
        out.update({k: getattr(params, k) for k in SELECT_FLAGS})
    path ="./val_{}_metrics.json".format(params.gen_name)
    if os.path.exists(path):
        os.remove(path)
    with open(path, "w") as fh:
        json.dump(out, fh)
    for k in names:
        print("%s: %s" % (k, "n/a (no training captions at hand)" if out[k] is None else "%.6f" % out[k]))
    print("wrote the metrics of %d captions of %d images to %s" % (captions, images, path))
    return out


def validation_references(val_gen):
    """--eval_captions: {image id: every human caption of the image} of a Batch_Generator (consensus.references_from_generator).  Its
    validation batches carry ONE randomly drawn caption per image, which is no reference set: BLEU's clipping and closest length and
    CIDEr-D's idf need all of an image's captions, and the numbers must not depend on the generator's random state.  None for a
    generator that holds no captions by file name (then the batches' own captions are all there is)."""
    if not (hasattr(val_gen, "_iterable") and hasattr(val_gen, "_imid") and getattr(val_gen, "captions", None) is not None):
        return None
    from ..consensus import references_from_generator
    return references_from_generator(val_gen)


def decoded_ids(decoder, n):
    """what the generation call just made left in decoder.last_token_ids: per image its ranked token-id lists"""
    ids = getattr(decoder, "last_token_ids", None)
    if ids is None or len(ids) != n:
        raise RuntimeError("--eval_captions: the decoder left no token ids of the %d images it has just decoded in last_token_ids" % n)
    return ids


def evaluate_decoded(params, decoder, references, decoded):
    """--eval_captions: evaluate once what was decoded (per image its ranked token-id lists) against the images' human captions and
    store the metrics.  Images without a human caption cannot be scored and are left out."""
    keep = [i for i, r in enumerate(references) if r]
    if len(keep) < len(references):
        print("%d images without a human caption are not evaluated" % (len(references) - len(keep)))
    references, decoded = [references[i] for i in keep], [decoded[i] for i in keep]
    evaluator = decoder.caption_evaluator(references)
    metrics = evaluator.evaluate(decoded, self_cider=True) if getattr(params, "eval_self_cider", False) else evaluator.evaluate(decoded)
    return store_metrics(params, metrics, len(decoded), sum(map(len, decoded)))


def _store(path, records):
    if os.path.exists(path):
        os.remove(path)
    with open(path, "w") as fh:
        json.dump(records, fh)
    print("wrote %d captions to %s" % (len(records), path))


def _restore(saver, sess, prefix):
    """`saver` may be a tf.train.Saver look-alike (restore(sess, path)) or a Trainer (restore(path))."""
    if saver is None:
        return
    print("Restoring from checkpoint", prefix)
    try:
        saver.restore(sess, prefix)
    except TypeError:
        saver.restore(prefix)


def inference(params, decoder, val_gen, test_gen, image_f_inputs=None, saver=None, sess=None):
    _restore(saver, sess, "./checkpoints/{}.ckpt".format(params.checkpoint))
    if not params.fine_tune:
        print("Captioning from precomputed fc2 features; pass --fine_tune to run the fine-tuned VGG16 on the images.")
    if getattr(decoder, "controls", None) is None:   # (main.py attaches them; a caller with its own decoder gets them from the flags)
        from ..controls import from_params
        decoder.controls = from_params(params, getattr(decoder, "data_dict", None))
    val_cv = params.use_c_v or params.prior in ("GMM", "AG")
    records, scores = [], []
    n_score = int(getattr(params, "score_draws", 0) or 0)
    n_bound, bounds = int(getattr(params, "bound_draws", 0) or 0), []
    evaluate = bool(getattr(params, "eval_captions", False))
    references, decoded = [], []
    all_refs = validation_references(val_gen) if evaluate else None
    for images, caps, lens, ids, c_v in val_gen.next_val_batch(get_image_ids=True, use_obj_vectors=params.use_c_v):
        if evaluate:
            decoder.last_token_ids = None
        records += _decode(decoder, params, sess, image_f_inputs, ids, images, _cluster_rows(c_v, val_cv), allow_beam=True)
        if evaluate:
            references += [all_refs[i] for i in ids] if all_refs is not None else human_captions(caps, lens)
            decoded += decoded_ids(decoder, len(ids))
        if n_score:
            scores += decoder.score_captions(ids, images, human_captions(caps, lens), _cluster_rows(c_v, val_cv), draws=n_score)
        if n_bound:
            bounds += decoder.bound_captions(ids, images, human_captions(caps, lens), _cluster_rows(c_v, val_cv), draws=n_bound)
    if n_score:
        store_scores(params, scores)
    if n_bound:
        store_bounds(params, bounds, getattr(decoder, "bound_stats", None))
    from ..vae_model.decoder import DIVERSE_FILE_MODES
    if params.sample_gen in DIVERSE_FILE_MODES:
        _store("./val_{}_diverse.json".format(params.gen_name), records)
        records = [{"image_id": r["image_id"], "caption": r["caption"]} for r in records]
    _store("./val_{}.json".format(params.gen_name), records)
    if evaluate:
        evaluate_decoded(params, decoder, references, decoded)
    if test_gen is None:
        return
    records = []
    for images, ids, c_v in test_gen.next_test_batch(params.use_c_v):
        records += _decode(decoder, params, sess, image_f_inputs, ids, images, _cluster_rows(c_v, params.use_c_v), allow_beam=False)
    _store("./test_{}.json".format(params.gen_name), records)
