"""Run configuration object with the attribute names, default values and command-line flags of the reference's
``Parameters`` (utils/parameters.py:2-66 attributes, :75-132 flags), so that ``main.py`` invocations written for the
reference keep working.  The flag table below is the single place that maps a flag to its attribute.

Differences: ``--gpu`` selects devices through HIP_VISIBLE_DEVICES (a comma list is allowed
for data-parallel runs) and is optional; a handful of additive flags (``--synthetic``, ``--ckpt_format`` ...) exist only here.
"""
import argparse
import os

_COCO = "/home/luoyy16/datasets-large/mscoco/coco/"

# attribute -> default.  Grouped as in the reference: model sizes, decoding, regularisation / optimiser, bookkeeping,
# fine-tuning, data preparation.
_DEFAULTS = dict(
    latent_size=150, num_clusters=90, num_epochs=20, learning_rate=0.0005, num_captions=5, batch_size=32, cnn_feature_size=4096,
    temperature=1.0, sample_gen="beam_search", beam_size=10, gen_max_len=30, gen_z_samples=100,
    encoder_rnn_layers=1, encoder_hidden=512, decoder_rnn_layers=1, decoder_hidden=512, embed_size=256, std=0.1,
    dec_keep_rate=1.0, dec_lstm_drop=1.0, ann_param=0, optimizer="Adam", lstm_clip_by_norm=5.0, restore=False,
    LOG_DIR="./model_logs/", save_params=0, no_encoder=False, vocab_size=None, coco_dir=_COCO, logging=False,
    hdf5_file=_COCO + "train_val.hdf5", use_hdf5=True, fine_tune=False, fine_tune_top=True, fine_tune_fe=True,
    cnn_lr=0.00001, cnn_optimizer="Adam", cnn_dropout=0.5, weight_decay=0.00004,
    gen_name="00", checkpoint="last_run", num_epochs_per_decay=5, use_c_v=False, gen_val_captions=4000, keep_words=3,
    cap_max_length=100, prior="Normal", max_checkpoints_to_keep=5, mode="training", num_ex_per_epoch=150000,
    image_net_weights_path="./utils/vgg16_weights.npz",
    # additive (not in the reference)
    synthetic=False, seed=1234, max_steps=0, captions_json=None, features_pickle=None, cluster_pickle=None, ckpt_format="tf",
    diverse_draws=20, diverse_method="greedy", diverse_rerank="likelihood", consensus_k=90, consensus_m=125,
    score_draws=0, beam_groups=5, beam_diversity=0.5, top_k=0, top_p=1.0, typical_p=1.0, min_p=0.0, eta=0.0, eval_captions=False, eval_self_cider=False,
    bound_draws=0, bound_mi=0, marginal_draws=20, constraints=None, cbs_width=0,
    no_repeat_ngram=0, min_len=0, repetition_penalty=1.0, banned_words=None, contrastive_k=5, contrastive_alpha=0.6,
    diverse_select="none", select_n=5, dpp_quality=1.0,
    # training objective options (every one off by default: the reference's objective)
    kl_free_bits=0.0, kl_weight=1.0, kl_cycle_steps=0, kl_cycle_ramp=0.5, kl_cycles=0, label_smoothing=0.0, word_drop=0.0,
    # self-critical training (off by default)
    scst=False, scst_baseline="average", scst_entropy=0.0, scst_rouge=0.0,
    # scheduled sampling in the cross-entropy phase (off by default)
    sched_sampling=0.0, sched_schedule="linear", sched_ramp_steps=10000, sched_pick="sample", sched_temperature=1.0,
    # unlikelihood training (off by default)
    unlikelihood=0.0, ul_window=128,
    # bag-of-words auxiliary loss (off by default)
    bow_loss=0.0,
    # weight averaging (off by default)
    ema_decay=0.0, use_ema=False,
)

# (flag, attribute, converter or "flag" for store_true, choices).  The reference's flags first, in its order.
_FLAGS = [
    ("--lr", "learning_rate", float, None), ("--embed_dim", "embed_size", int, None), ("--enc_hid", "encoder_hidden", int, None),
    ("--dec_hid", "decoder_hidden", int, None), ("--latent", "latent_size", int, None), ("--restore", "restore", "flag", None),
    ("--gpu", None, str, None), ("--coco_dir", "coco_dir", str, None), ("--epochs", "num_epochs", int, None),
    ("--bs", "batch_size", int, None), ("--no_encoder", "no_encoder", "flag", None), ("--temperature", "temperature", float, None),
    ("--gen_name", "gen_name", str, None), ("--dec_drop", "dec_keep_rate", float, None), ("--gen_z_samples", "gen_z_samples", int, None),
    ("--ann_param", "ann_param", float, None), ("--dec_lstm_drop", "dec_lstm_drop", float, None), ("--sample_gen", "sample_gen", str, None),
    ("--checkpoint", "checkpoint", str, None), ("--optimizer", "optimizer", str, ["SGD", "Adam", "Momentum"]),
    ("--c_v", "use_c_v", "flag", None), ("--std", "std", float, None), ("--save_params", "save_params", "flag", None),
    ("--prior", "prior", str, ["GMM", "AG", "Normal"]), ("--fine_tune", "fine_tune", "flag", None),
    ("--mode", "mode", str, ["training", "inference"]),
    # additive
    ("--synthetic", "synthetic", "flag", None), ("--vocab", None, int, None), ("--seed", "seed", int, None),
    ("--max_steps", "max_steps", int, None), ("--captions_json", "captions_json", str, None),
    ("--features_pickle", "features_pickle", str, None), ("--cluster_pickle", "cluster_pickle", str, None),
    ("--ckpt_format", "ckpt_format", str, ["tf", "npz"]),
    ("--diverse_draws", "diverse_draws", int, None), ("--diverse_method", "diverse_method", str, ["greedy", "sample"]),
    ("--diverse_rerank", "diverse_rerank", str, ["likelihood", "consensus", "marginal", "mbr"]), ("--consensus_k", "consensus_k", int, None),
    ("--consensus_m", "consensus_m", int, None), ("--score_draws", "score_draws", int, None),
    ("--beam_size", "beam_size", int, None), ("--beam_groups", "beam_groups", int, None), ("--beam_diversity", "beam_diversity", float, None),
    ("--top_k", "top_k", int, None), ("--top_p", "top_p", float, None), ("--typical_p", "typical_p", float, None),
    ("--min_p", "min_p", float, None), ("--eta_cutoff", "eta", float, None), ("--eval_captions", "eval_captions", "flag", None),
    ("--eval_self_cider", "eval_self_cider", "flag", None),
    ("--bound_draws", "bound_draws", int, None), ("--bound_mi", "bound_mi", int, None), ("--marginal_draws", "marginal_draws", int, None),
    ("--constraints", "constraints", str, None), ("--cbs_width", "cbs_width", int, None),
    ("--no_repeat_ngram", "no_repeat_ngram", int, None), ("--min_len", "min_len", int, None),
    ("--repetition_penalty", "repetition_penalty", float, None), ("--banned_words", "banned_words", str, None),
    ("--contrastive_k", "contrastive_k", int, None), ("--contrastive_alpha", "contrastive_alpha", float, None),
    ("--diverse_select", "diverse_select", str, ["none", "dpp"]), ("--select_n", "select_n", int, None),
    ("--dpp_quality", "dpp_quality", float, None),
    ("--kl_free_bits", "kl_free_bits", float, None), ("--kl_weight", "kl_weight", float, None),
    ("--kl_cycle_steps", "kl_cycle_steps", int, None), ("--kl_cycle_ramp", "kl_cycle_ramp", float, None),
    ("--kl_cycles", "kl_cycles", int, None), ("--label_smoothing", "label_smoothing", float, None),
    ("--word_drop", "word_drop", float, None),
    ("--scst", "scst", "flag", None), ("--scst_baseline", "scst_baseline", str, ["average", "greedy"]),
    ("--scst_entropy", "scst_entropy", float, None), ("--scst_rouge", "scst_rouge", float, None),
    ("--sched_sampling", "sched_sampling", float, None), ("--sched_schedule", "sched_schedule", str, ["constant", "linear", "sigmoid"]),
    ("--sched_ramp_steps", "sched_ramp_steps", int, None), ("--sched_pick", "sched_pick", str, ["sample", "argmax"]),
    ("--sched_temperature", "sched_temperature", float, None),
    ("--unlikelihood", "unlikelihood", float, None), ("--ul_window", "ul_window", int, None),
    ("--bow_loss", "bow_loss", float, None),
    ("--ema_decay", "ema_decay", float, None), ("--use_ema", "use_ema", "flag", None),
]
_KL_FLAGS = ("kl_free_bits", "kl_weight", "kl_cycle_steps", "kl_cycle_ramp", "kl_cycles")
_SCHED_FLAGS = ("sched_schedule", "sched_ramp_steps", "sched_pick", "sched_temperature")
_HELP = {"--synthetic": "train on seeded synthetic batches (no MSCOCO needed)", "--vocab": "vocabulary size for --synthetic (default 10000)",
         "--max_steps": "steps per epoch (0 = the reference's num_ex_per_epoch rule, main.py:217-221)",
         "--captions_json": "COCO captions json (with --features_pickle: in-memory real-data path)",
         "--features_pickle": "pickle {file_name: fc2 feature [1, 4096]} (the reference's ./pickles/<split>.pickle format)",
         "--cluster_pickle": "pickle {file_name: 91-vector} (the reference's ./obj_vectors/c_v.pickle)",
         "--ckpt_format": "tf = TensorFlow V2 checkpoint files (what tf.train.Saver writes), npz = numpy archive",
         "--diverse_draws": "--sample_gen diverse: latent draws per image (1..256; default 20)",
         "--diverse_method": "--sample_gen diverse: decoding of each draw (greedy or sample; default greedy)",
         "--diverse_rerank": "--sample_gen diverse: order of each image's captions (likelihood, consensus with the captions of its "
                             "nearest training images, marginal: the likelihood over all of the image's draws, or mbr: the expected CIDEr-D "
                             "against the image's own captions, weighted by their counts -- minimum-Bayes-risk selection, which needs "
                             "only the training captions for its idf; default likelihood)",
         "--consensus_k": "--diverse_rerank consensus: nearest training images per image (1..256; default 90)",
         "--consensus_m": "--diverse_rerank consensus: best-matching pool captions averaged per candidate (>= 1; default 125)",
         "--score_draws": "--mode inference: also score the validation images' human captions under this many prior draws and write "
                          "./val_{gen_name}_scores.json (0..256; default 0 = off)",
         "--beam_size": "beams per image (default 10); --sample_gen diverse_beam: the total over the groups, a multiple of --beam_groups, <= 16; "
                        "--sample_gen stochastic_beam: distinct captions sampled per image, 1..32",
         "--beam_groups": "--sample_gen diverse_beam: groups per image, each a beam search of beam_size / beam_groups beams (default 5)",
         "--beam_diversity": "--sample_gen diverse_beam: what a word costs a candidate per live beam of the round's earlier groups that "
                             "has just taken it (>= 0; default 0.5)",
         "--top_k": "--sample_gen sample / --diverse_method sample: draw each word from the k most likely only (>= 0; default 0 = all)",
         "--top_p": "--sample_gen sample / --diverse_method sample: draw each word from the smallest set of most likely words that holds "
                    "this share of the probability (nucleus sampling; in (0, 1]; default 1.0 = all)",
         "--typical_p": "--sample_gen sample / --diverse_method sample: locally typical sampling -- draw each word from the words whose "
                        "surprisal is closest to the entropy of the prediction, the smallest such set that holds this share of the "
                        "probability (in (0, 1]; default 1.0 = all; not with --top_k / --top_p / --scst)",
         "--min_p": "--sample_gen sample / --diverse_method sample: draw each word from the words at least this fraction as likely as "
                    "the most likely one (in [0, 1]; default 0 = all; 1 = the most likely word; not with --top_k / --top_p / --scst)",
         "--eta_cutoff": "--sample_gen sample / --diverse_method sample: eta sampling -- draw each word from the words with probability "
                         ">= min(eta, sqrt(eta) * exp(-entropy)), a floor that drops when the prediction is uncertain (in [0, 1); "
                         "default 0 = all; try 3e-4 .. 4e-3; not with --top_k / --top_p / --scst)",
         "--eval_captions": "--mode inference: also evaluate the validation captions against the images' human captions on the GPU (BLEU, "
                            "CIDEr-D, oracle CIDEr-D, ROUGE-L, distinct / novel / Div-1 / Div-2 / mBLEU-4) and write ./val_{gen_name}_metrics.json",
         "--eval_self_cider": "--eval_captions: also report self_cider (Self-CIDEr diversity of each image's caption set, from the "
                              "eigenvalues of its in-set CIDEr-D matrix) and mbr_cider_d (the CIDEr-D of the caption that "
                              "minimum-Bayes-risk selection would take)",
         "--bound_draws": "--mode inference: also bound the likelihood of the validation images' human captions with this many posterior "
                          "draws per caption (ELBO, importance-weighted bound, KL, effective sample size, active latent units) and "
                          "write ./val_{gen_name}_bound.json (0..256; default 0 = off; not with --no_encoder)",
         "--bound_mi": "--bound_draws: also estimate the mutual information I(x; z) between a caption and its latent code under the "
                       "aggregated posterior, from the posteriors of the first this many bounded captions (every draw scored under "
                       "every posterior: the work grows with its square), and add mi, mi_block, mi_captions and mi_ceiling to the "
                       "header of ./val_{gen_name}_bound.json (0..65536; default 0 = off; gen_z_samples <= 128)",
         "--marginal_draws": "--sample_gen marginal_greedy / marginal_beam: latent draws per image whose mixture is searched (1..256; "
                             "default 20)",
         "--constraints": "--sample_gen constrained_beam: JSON file {image_id: [[word, ...], ...]} of the words the captions must mention "
                          "(at most 3 sets of at most 4 words per image; a set is met by any of its words; \"*\" = every other image; words "
                          "are vocabulary strings or integer token ids)",
         "--cbs_width": "--sample_gen constrained_beam: beams per state of satisfied constraints (default 0 = the largest that fits, "
                        "16 >> the number of constraints)",
         "--no_repeat_ngram": "decoding controls: no n-gram of this length appears twice in a caption (0..8; default 0 = off)",
         "--min_len": "decoding controls: no <EOS> before this many words (>= 0, below gen_max_len; default 0 = off)",
         "--repetition_penalty": "decoding controls: the logit of every word already in the caption is divided (positive) or multiplied "
                                 "(negative) by this (1..10; default 1.0 = off)",
         "--banned_words": "decoding controls: JSON file with a list of words (vocabulary strings or integer token ids, at most 256) that "
                           "no caption may hold; not with --sample_gen marginal_greedy / marginal_beam, like the three flags above",
         "--contrastive_k": "--sample_gen contrastive: next words looked one decoder step ahead per round (1..16; default 5; 1 = greedy)",
         "--contrastive_alpha": "--sample_gen contrastive: weight of the degeneration penalty, the largest cosine similarity between a "
                                "candidate's decoder state and the states of the caption so far, against the word's probability "
                                "(in [0, 1]; default 0.6; 0 = greedy)",
         "--diverse_select": "--sample_gen diverse / diverse_beam / stochastic_beam: which of an image's ranked captions are kept -- none: "
                             "the list as ranked; dpp: --select_n of them chosen jointly for quality and for difference from each "
                             "other (greedy MAP of a determinantal point process over the image's in-set CIDEr-D matrix, after "
                             "--diverse_rerank; needs only the training captions for its idf; default none)",
         "--select_n": "--diverse_select dpp: captions kept per image (1..32; default 5)",
         "--dpp_quality": "--diverse_select dpp: weight W of a caption's rank in its quality exp(W * rank score scaled to [0, 1] over "
                          "the image): the best-ranked caption weighs e^W times the worst (in [0, 8]; 0 = diversity alone; default "
                          "1.0, a choice that no captioning run has tuned)",
         "--kl_free_bits": "training objective: KL floor in nats per latent dimension and caption row (free bits: a dimension whose KL "
                           "is at or below it is held at the floor and gets no KL gradient; >= 0; default 0 = off)",
         "--kl_weight": "training objective: weight beta of the KL term in the lower bound and its gradient (> 0; default 1.0)",
         "--kl_cycle_steps": "training objective: period P of cyclical KL annealing in steps, annealing = min(1, (step mod P) / "
                             "(ramp * P)); also under --restore / --fine_tune; not with --ann_param > 1 (>= 0; default 0 = off)",
         "--kl_cycle_ramp": "--kl_cycle_steps: share of each period over which the coefficient rises from 0 to 1 (in (0, 1]; default 0.5)",
         "--kl_cycles": "--kl_cycle_steps: number of periods, after which the coefficient stays 1 (>= 0; default 0 = forever)",
         "--label_smoothing": "training objective: the reconstruction target is (1 - eps) * onehot + eps / vocabulary (in [0, 1); "
                              "default 0 = off; validation losses stay unsmoothed)",
         "--word_drop": "training: each decoder input word behind <BOS> is replaced by <UNK> with this probability (in [0, 1); "
                        "default 0 = off; seeded by --seed; never in validation or inference)",
         "--scst": "self-critical training: every training step samples num_captions captions per image, rewards them with CIDEr-D "
                   "against the image's human captions and takes a policy-gradient step of the decoder (the encoder is left alone); "
                   "meant for --restore from a cross-entropy-trained checkpoint; single GPU, precomputed features",
         "--scst_baseline": "--scst: what a sample's reward is compared with -- average: the mean reward of the image's other samples "
                            "(needs num_captions >= 2); greedy: the reward of the greedy caption under the same latent draw (default average)",
         "--scst_entropy": "--scst: weight of the token-entropy bonus in the policy loss (finite, >= 0; default 0 = off)",
         "--scst_rouge": "--scst: weight W of a ROUGE-L term in the reward, which is then CIDEr-D + W * ROUGE-L (finite, >= 0; "
                         "default 0 = off: CIDEr-D alone)",
         "--sched_sampling": "scheduled sampling, two-pass form: each decoder input word behind <BOS> is replaced with (at most) this "
                             "probability by a word the model itself predicts for that position in a first, teacher-forced pass; the "
                             "decoder is then re-run on the mixed inputs and trained against the unchanged labels (in [0, 1]; default "
                             "0 = off; never in validation or inference; not with --scst)",
         "--sched_schedule": "--sched_sampling: how the probability moves with the global step s -- constant: R; linear: R * min(1, s / K); "
                             "sigmoid: R * (1 - K / (K + exp(s / K))), K = --sched_ramp_steps (default linear)",
         "--sched_ramp_steps": "--sched_sampling: K of the linear and the sigmoid schedule (>= 1; default 10000; constant ignores it)",
         "--sched_pick": "--sched_sampling: the model's word is a draw from its prediction (sample) or its most likely word (argmax; "
                         "default sample)",
         "--sched_temperature": "--sched_sampling --sched_pick sample: temperature of the draw (> 0; default 1.0)",
         "--unlikelihood": "training objective: weight alpha of the token-level unlikelihood term, which at every caption position adds "
                           "-alpha * sum_c log(1 - p(c)) over the words c the target caption has already said (finite, >= 0; default "
                           "0 = off; validation losses and the reported rec_loss stay the cross-entropy; not with --scst)",
         "--ul_window": "--unlikelihood: how many earlier positions of the caption supply those words (1..128; default 128; a longer "
                        "caption is no error, the window bounds the look-back)",
         "--bow_loss": "training objective: weight A of the bag-of-words auxiliary loss -- a head that sees the latent code alone (the "
                       "decoder's z step) and must predict which words the caption contains, so that z has a reason of its own to carry "
                       "the caption (finite, >= 0; default 0 = off; adds the variables bow/kernel and bow/bias; validation losses and the "
                       "reported rec_loss stay as they are; not with --no_encoder, --scst or --mode inference)",
         "--ema_decay": "weight averaging: keep an exponential moving average of every trained variable with this decay, updated "
                        "inside the optimiser pass (with the num_updates warm-up min(decay, (1 + t) / (10 + t)) unless the averages "
                        "came from a checkpoint), validate with it as well and write it into the checkpoints as "
                        "<name>/ExponentialMovingAverage (in [0, 1); default 0 = off; not with --scst or --mode inference)",
         "--use_ema": "--mode inference: restore the averaged weights that a run with --ema_decay wrote in place of the last iterate",
         "--sample_gen": "decoding of the validation images: beam_search (default), greedy, sample, diverse, diverse_beam, or the search "
                         "under the mixture of --marginal_draws latent draws: marginal_greedy, marginal_beam (--beam_size beams, 1..16), or "
                         "constrained_beam: beam search whose captions mention the words of --constraints, or stochastic_beam: --beam_size "
                         "distinct captions sampled without replacement, each with its probability and importance weight, or "
                         "contrastive: contrastive search over the --contrastive_k most likely words (deterministic; --contrastive_alpha "
                         "weighs the similarity of a word's decoder state to the caption's earlier ones against its probability)"}


class Parameters(object):
    """Attributes = the keys of _DEFAULTS (class-level, so `Parameters().x` and pickled instances behave like the reference's)."""

    def build_parser(self):
        ap = argparse.ArgumentParser(description="CVAE / AG-CVAE captioning trainer (MI355X)")
        for flag, attr, conv, choices in _FLAGS:
            kw = dict(help=_HELP.get(flag))
            if conv == "flag":
                ap.add_argument(flag, action="store_true", **kw)
            else:
                ap.add_argument(flag, default=None, choices=choices, **kw)
        return ap

    def parse_args(self, argv=None):
        ap = self.build_parser()
        args = vars(ap.parse_args(argv))
        for flag, attr, conv, _ in _FLAGS:
            val = args[flag.lstrip("-")]
            if attr is None:
                continue
            if conv == "flag":
                if val:  # store_true flags only ever switch something on
                    setattr(self, attr, True if attr != "save_params" else 1)
                elif attr in ("restore", "no_encoder", "use_c_v", "fine_tune", "synthetic"):
                    setattr(self, attr, False)
            elif val is not None:
                setattr(self, attr, conv(val))
            else:
                setattr(self, attr, getattr(self, attr))  # materialise the default on the instance (it is pickled by --save_params)
        if not 1 <= self.consensus_k <= 256:
            ap.error("--consensus_k must be 1..256 (got %d)" % self.consensus_k)
        if self.consensus_m < 1:
            ap.error("--consensus_m must be >= 1 (got %d)" % self.consensus_m)
        if not 0 <= self.score_draws <= 256:
            ap.error("--score_draws must be 0..256 (got %d)" % self.score_draws)
        if not 0 <= self.bound_draws <= 256:
            ap.error("--bound_draws must be 0..256 (got %d)" % self.bound_draws)
        if self.bound_draws and self.mode != "inference":
            ap.error("--bound_draws needs --mode inference (got --mode %s)" % self.mode)
        if self.bound_draws and self.no_encoder:
            ap.error("--bound_draws needs the encoder's posterior: not with --no_encoder")
        if not 0 <= self.bound_mi <= 65536:
            ap.error("--bound_mi must be 0..65536 (0 = off; got %d)" % self.bound_mi)
        if self.bound_mi and not self.bound_draws:
            ap.error("--bound_mi reads the posteriors that --bound_draws > 0 computes (--mode inference, not with --no_encoder)")
        if self.bound_mi and not 1 <= self.gen_z_samples <= 128:
            ap.error("--bound_mi scores at most 128 draws per caption (got --gen_z_samples %d)" % self.gen_z_samples)
        if self.sample_gen == "diverse_beam":
            if self.beam_groups < 1:
                ap.error("--beam_groups must be >= 1 (got %d)" % self.beam_groups)
            if not 1 <= self.beam_size <= 16:
                ap.error("--beam_size must be 1..16 with --sample_gen diverse_beam (got %d)" % self.beam_size)
            if self.beam_size % self.beam_groups:
                ap.error("--beam_size must be divisible by --beam_groups (got %d and %d)" % (self.beam_size, self.beam_groups))
            if not (0.0 <= self.beam_diversity < float("inf")):
                ap.error("--beam_diversity must be finite and >= 0 (got %r)" % self.beam_diversity)
        if not 1 <= self.marginal_draws <= 256:
            ap.error("--marginal_draws must be 1..256 (got %d)" % self.marginal_draws)
        if self.sample_gen == "marginal_beam" and not 1 <= self.beam_size <= 16:
            ap.error("--beam_size must be 1..16 with --sample_gen marginal_beam (got %d)" % self.beam_size)
        if self.sample_gen == "stochastic_beam":
            if not 1 <= self.beam_size <= 32:
                ap.error("--beam_size must be 1..32 with --sample_gen stochastic_beam (got %d)" % self.beam_size)
            if self.temperature != 1.0:
                ap.error("--temperature must be 1 with --sample_gen stochastic_beam: its weights need the captions' probabilities under "
                         "the distribution that was sampled (got %r)" % self.temperature)
        if self.sample_gen == "constrained_beam":
            if not self.constraints:
                ap.error("--sample_gen constrained_beam needs --constraints FILE")
            if not 0 <= self.cbs_width <= 16:
                ap.error("--cbs_width must be 0..16 (0 = the largest that fits; got %d)" % self.cbs_width)
        elif self.constraints is not None or args["cbs_width"] is not None:
            ap.error("--constraints / --cbs_width belong to --sample_gen constrained_beam (got --sample_gen %s)" % self.sample_gen)
        if self.sample_gen == "contrastive":
            if not 1 <= self.contrastive_k <= 16:
                ap.error("--contrastive_k must be 1..16 (got %d)" % self.contrastive_k)
            if not (0.0 <= self.contrastive_alpha <= 1.0):
                ap.error("--contrastive_alpha must be in [0, 1] (got %r)" % self.contrastive_alpha)
            if self.temperature != 1.0:
                ap.error("--temperature must be 1 with --sample_gen contrastive: its scores weigh the model's own probabilities "
                         "against a similarity (got %r)" % self.temperature)
        elif args["contrastive_k"] is not None or args["contrastive_alpha"] is not None:
            ap.error("--contrastive_k / --contrastive_alpha belong to --sample_gen contrastive (got --sample_gen %s)" % self.sample_gen)
        if self.diverse_select == "dpp":
            if self.sample_gen not in ("diverse", "diverse_beam", "stochastic_beam"):
                ap.error("--diverse_select dpp selects from a list of captions per image: --sample_gen diverse, diverse_beam or "
                         "stochastic_beam (got --sample_gen %s)" % self.sample_gen)
            if not 1 <= self.select_n <= 32:
                ap.error("--select_n must be 1..32 (got %d)" % self.select_n)
            if not (0.0 <= self.dpp_quality <= 8.0):
                ap.error("--dpp_quality must be in [0, 8] (0 = diversity alone; got %r)" % self.dpp_quality)
        elif args["select_n"] is not None or args["dpp_quality"] is not None:
            ap.error("--select_n / --dpp_quality belong to --diverse_select dpp")
        if not 0 <= self.no_repeat_ngram <= 8:
            ap.error("--no_repeat_ngram must be 0..8 (0 = off; got %d)" % self.no_repeat_ngram)
        if not 0 <= self.min_len < self.gen_max_len:
            ap.error("--min_len must be >= 0 and below gen_max_len = %d (0 = off; got %d)" % (self.gen_max_len, self.min_len))
        if not (1.0 <= self.repetition_penalty <= 10.0):
            ap.error("--repetition_penalty must be in [1, 10] (1 = off; got %r)" % self.repetition_penalty)
        if self.sample_gen in ("marginal_greedy", "marginal_beam") and any(args[k] is not None for k in ("no_repeat_ngram", "min_len", "repetition_penalty", "banned_words")):
            ap.error("--no_repeat_ngram / --min_len / --repetition_penalty / --banned_words do not go with --sample_gen %s (the mixture "
                     "it searches is score()'s marginal, which they would change)" % self.sample_gen)
        if self.top_k < 0:
            ap.error("--top_k must be >= 0 (got %d)" % self.top_k)
        if not (0.0 < self.top_p <= 1.0):
            ap.error("--top_p must be in (0, 1] (got %r)" % self.top_p)
        if not (0.0 < self.typical_p <= 1.0):
            ap.error("--typical_p must be in (0, 1] (got %r)" % self.typical_p)
        if not (0.0 <= self.min_p <= 1.0):
            ap.error("--min_p must be in [0, 1] (got %r)" % self.min_p)
        if not (0.0 <= self.eta < 1.0):
            ap.error("--eta_cutoff must be in [0, 1) (got %r)" % self.eta)
        if self.typical_p != 1.0 or self.min_p != 0.0 or self.eta != 0.0:
            if self.top_k != 0 or self.top_p != 1.0:
                ap.error("--typical_p / --min_p / --eta_cutoff do not go with --top_k / --top_p: give one family of cuts (their order "
                         "of renormalisation is not defined)")
            if self.sample_gen == "diverse" and self.diverse_method != "sample":
                ap.error("--typical_p / --min_p / --eta_cutoff cut the draw of --diverse_method sample; --diverse_method %s has none"
                         % self.diverse_method)
            if self.scst:
                ap.error("--typical_p / --min_p / --eta_cutoff do not go with --scst: its samples come from the untruncated distribution")
        if not (0.0 <= self.kl_free_bits < float("inf")):
            ap.error("--kl_free_bits must be finite and >= 0 (0 = off; got %r)" % self.kl_free_bits)
        if not (0.0 < self.kl_weight < float("inf")):
            ap.error("--kl_weight must be finite and > 0 (got %r)" % self.kl_weight)
        if not (0.0 <= self.label_smoothing < 1.0):
            ap.error("--label_smoothing must be in [0, 1) (0 = off; got %r)" % self.label_smoothing)
        if self.kl_cycle_steps < 0:
            ap.error("--kl_cycle_steps must be >= 0 (0 = off; got %d)" % self.kl_cycle_steps)
        if not (0.0 < self.kl_cycle_ramp <= 1.0):
            ap.error("--kl_cycle_ramp must be in (0, 1] (got %r)" % self.kl_cycle_ramp)
        if self.kl_cycles < 0:
            ap.error("--kl_cycles must be >= 0 (0 = forever; got %d)" % self.kl_cycles)
        if not (0.0 <= self.word_drop < 1.0):
            ap.error("--word_drop must be in [0, 1) (0 = off; got %r)" % self.word_drop)
        if self.kl_cycle_steps > 0 and self.ann_param > 1:
            ap.error("--kl_cycle_steps and --ann_param > 1 are two schedules for the one annealing coefficient: give one of them")
        if self.no_encoder and any(args[k] is not None for k in _KL_FLAGS):
            ap.error("--kl_free_bits / --kl_weight / --kl_cycle_steps / --kl_cycle_ramp / --kl_cycles shape the KL term, and "
                     "--no_encoder has none")
        if not (0.0 <= self.scst_entropy < float("inf")):
            ap.error("--scst_entropy must be finite and >= 0 (0 = off; got %r)" % self.scst_entropy)
        if not (0.0 <= self.scst_rouge < float("inf")):
            ap.error("--scst_rouge must be finite and >= 0 (0 = off; got %r)" % self.scst_rouge)
        if not self.scst and (args["scst_baseline"] is not None or args["scst_entropy"] is not None):
            ap.error("--scst_baseline / --scst_entropy belong to --scst")
        if not self.scst and args["scst_rouge"] is not None:
            ap.error("--scst_rouge belongs to --scst")
        if self.scst:
            if self.fine_tune:
                ap.error("--scst does not go with --fine_tune: there is no VGG16 backward from the policy loss")
            if self.mode != "training":
                ap.error("--scst is a way of training: not with --mode %s" % self.mode)
            if self.temperature != 1.0:
                ap.error("--temperature must be 1 with --scst: the policy gradient needs the captions' probabilities under the "
                         "distribution that was sampled (got %r)" % self.temperature)
            if self.top_k != 0 or self.top_p != 1.0:
                ap.error("--top_k / --top_p do not go with --scst: its samples come from the untruncated distribution")
            shaped = [k for k in _KL_FLAGS + ("label_smoothing", "word_drop") if args[k] is not None]
            if shaped:
                ap.error("--%s shape(s) the cross-entropy / KL objective, which --scst does not optimise" % " / --".join(shaped))
            if self.scst_baseline == "average" and self.num_captions < 2:
                ap.error("--scst_baseline average compares an image's samples with each other: it needs num_captions >= 2 (got %d); "
                         "give --scst_baseline greedy" % self.num_captions)
        if not (0.0 <= self.sched_sampling <= 1.0):
            ap.error("--sched_sampling must be in [0, 1] (0 = off; got %r)" % self.sched_sampling)
        if self.sched_ramp_steps < 1:
            ap.error("--sched_ramp_steps must be >= 1 (got %d)" % self.sched_ramp_steps)
        if not (0.0 < self.sched_temperature < float("inf")):
            ap.error("--sched_temperature must be finite and > 0 (got %r)" % self.sched_temperature)
        if not self.sched_sampling > 0 and any(args[k] is not None for k in _SCHED_FLAGS):
            ap.error("--sched_schedule / --sched_ramp_steps / --sched_pick / --sched_temperature belong to --sched_sampling > 0")
        if self.sched_sampling > 0:
            if self.scst:
                ap.error("--sched_sampling mixes the inputs of the cross-entropy step, which --scst does not take")
            if self.mode != "training":
                ap.error("--sched_sampling is a way of training: not with --mode %s" % self.mode)
        if not (0.0 <= self.unlikelihood < float("inf")):
            ap.error("--unlikelihood must be finite and >= 0 (0 = off; got %r)" % self.unlikelihood)
        if not 1 <= self.ul_window <= 128:
            ap.error("--ul_window must be 1..128 (got %d)" % self.ul_window)
        if not self.unlikelihood > 0 and args["ul_window"] is not None:
            ap.error("--ul_window belongs to --unlikelihood > 0")
        if self.unlikelihood > 0 and self.scst:
            ap.error("--unlikelihood shapes the cross-entropy objective, which --scst does not optimise")
        if not (0.0 <= self.bow_loss < float("inf")):
            ap.error("--bow_loss must be finite and >= 0 (0 = off; got %r)" % self.bow_loss)
        if self.bow_loss > 0:
            if self.no_encoder:
                ap.error("--bow_loss trains the latent code through a head on it, and --no_encoder has none")
            if self.scst:
                ap.error("--bow_loss shapes the cross-entropy objective, which --scst does not optimise")
            if self.mode != "training":
                ap.error("--bow_loss is a way of training: not with --mode %s" % self.mode)
        if not (0.0 <= self.ema_decay < 1.0):
            ap.error("--ema_decay must be in [0, 1) (0 = off; got %r)" % self.ema_decay)
        if self.ema_decay > 0:
            if self.mode != "training":
                ap.error("--ema_decay averages the weights of a training run: not with --mode %s (give --use_ema to decode with the "
                         "averages of a checkpoint)" % self.mode)
            if self.scst:
                ap.error("--ema_decay does not go with --scst: the policy step updates ranges of the store only, and averaging under "
                         "it is not built")
        if self.use_ema and self.mode != "inference":
            ap.error("--use_ema needs --mode inference (got --mode %s)" % self.mode)
        if self.eval_captions and self.mode != "inference":
            ap.error("--eval_captions needs --mode inference (got --mode %s)" % self.mode)
        if self.eval_self_cider and not self.eval_captions:
            ap.error("--eval_self_cider belongs to --eval_captions")
        if self.synthetic:
            self.vocab_size = int(args["vocab"]) if args["vocab"] is not None else 10000
        self.hdf5_file = self.coco_dir + os.path.basename(self.hdf5_file)  # the image array lives next to the data set
        if args["gpu"] is not None:
            os.environ["HIP_VISIBLE_DEVICES"] = str(args["gpu"])
        return self


for _name, _value in _DEFAULTS.items():
    setattr(Parameters, _name, _value)
