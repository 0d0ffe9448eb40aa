#!/usr/bin/env python
"""Caption one image: the command line and the `Generator` class of the reference's gen_caption.py
(:19-150) on the MI355X-native path.

    python gen_caption.py --img_path cat.jpg --checkpoint ./checkpoints/last_run.ckpt \\
        --params_path ./pickles/params_Normal_False_last_run_False.pickle --vocab_path ./pickles/capt_vocab.pickle \\
        [--gen_method greedy|beam_search|sample|diverse|marginal_greedy|marginal_beam|constrained_beam|stochastic_beam|contrastive] [--must_include "dog,puppy;frisbee"] [--beam_size 2] [--diverse_draws 20] [--marginal_draws 20] [--vgg_weights ./utils/vgg16_weights.npz]
        [--top_k 0] [--top_p 1.0]     (sampled decoding: draw from the k best words / the nucleus holding a share p; default: the params')
        [--typical_p 1.0] [--min_p 0] [--eta_cutoff 0]   (sampled decoding: locally typical / min-p / eta sampling; not with --top_k / --top_p)
        [--contrastive_k 5] [--contrastive_alpha 0.6]    (--gen_method contrastive: words looked ahead per round, weight of the similarity penalty)
        [--diverse_select dpp] [--select_n 5] [--dpp_quality 1.0]   (--gen_method diverse / stochastic_beam: keep select_n captions chosen jointly for quality and difference)

Flow (gen_caption.py:73-130): load the pickled Parameters and the vocabulary, decode + resize the image,
VGG16 fc2 features [1, 4096], imf_emb -> decoder (prior z) -> greedy / beam search, print the caption.
Differences, all forced by what exists in this image:
  * the reference takes its features from Keras' ImageNet VGG16 (downloaded weights).  Here the features come
    from this build's VGG16 (`vc_conv3x3_*`) with the weights of `--vgg_weights` (the `vgg16_weights.npz` the
    training path uses, utils/image_embeddings.py:240-246) or, without that flag, the `cnn/*` variables of the
    checkpoint (present when the model was fine-tuned or `cnn` variables were saved, main.py:186-189).
  * `Dictionary(data_dict)` is called with keep_words from the params pickle (the reference call omits the
    argument and cannot run as written).
  * `--checkpoint` is a TF V2 checkpoint prefix (or an .npz archive written with --ckpt_format npz)."""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


class _ParamsUnpickler(pickle.Unpickler):
    """The reference pickles the Parameters INSTANCE (main.py:306-313), i.e. a reference to the class
    `utils.parameters.Parameters`; map it onto this build's class."""

    def find_class(self, module, name):
        if name == "Parameters" and module.endswith("parameters"):
            from vae_captioning_amd.utils.parameters import Parameters
            return Parameters
        return super().find_class(module, name)


class Generator(object):
    """Generate caption, given the image (gen_caption.py:19)."""

    def __init__(self, checkpoint_path, params_path, vocab_path, gen_method="greedy", vgg_weights=None, use_ema=False):
        from vae_captioning_amd.utils.captions import Dictionary
        self.checkpoint_path = checkpoint_path
        self.use_ema = bool(use_ema)   # (additive) caption with the averaged weights a run with --ema_decay wrote
        self.params = self._load_params(params_path)
        self.gen_method = gen_method
        self.vgg_weights = vgg_weights
        if not vocab_path or not os.path.exists(vocab_path):
            raise ValueError("No caption vocabulary path specified, usually it can be found in the ./pickles folder "
                             "after model training")
        with open(vocab_path, "rb") as rf:
            data_dict = pickle.load(rf)
        self.data_dict = Dictionary(data_dict, getattr(self.params, "keep_words", 3))
        self.params.vocab_size = self.data_dict.vocab_size
        self._trainer = None
        self._vgg = None

    def _c_v_generator(self, image):
        # the reference leaves this unimplemented ("TODO: finish cluster vector implementation") and returns None
        return None

    def _load_params(self, params_path):
        """Load serialized Parameters class (gen_caption.py:50-55); a plain dict of attributes (what this
        build's main.py --save_params writes) is accepted too."""
        from vae_captioning_amd.utils.parameters import Parameters
        with open(params_path, "rb") as rf:
            obj = _ParamsUnpickler(rf).load()
        if isinstance(obj, dict):
            params = Parameters()
            for k, v in obj.items():
                setattr(params, k, v)
            return params
        return obj

    # ------------------------------------------------------------------ model pieces
    def _checkpoint_tensors(self):
        if self.checkpoint_path.endswith(".npz"):
            with np.load(self.checkpoint_path) as z:
                return {k: z[k] for k in z.files}
        from vae_captioning_amd import tf_bundle
        return tf_bundle.read_bundle(self.checkpoint_path)

    def _build(self):
        """imf_emb + Decoder (+ cv_emb) on restored variables (gen_caption.py:84-115)."""
        if self._trainer is not None:
            return
        from vae_captioning_amd import spec
        from vae_captioning_amd.trainer import Trainer, VggEngine
        from vae_captioning_amd.utils.parameters import Parameters
        p = self.params
        p.sample_gen = self.gen_method                     # gen_caption.py:83
        p.mode, p.fine_tune = "inference", False            # features are fed, as images_ps [None, 4096]
        p.ema_decay = 0.0                                   # (a training run's pickle may carry it: nothing is averaged here)
        tensors = self._checkpoint_tensors()
        if self.use_ema:   # every <name>/ExponentialMovingAverage as <name> (Trainer.restore(use_ema=True))
            from vae_captioning_amd.engine import EMA_SUFFIX, split_averages
            avg = split_averages(tensors)
            if not avg:
                raise KeyError("--use_ema: checkpoint %s holds no averaged weights (<name>%s): it was written without --ema_decay"
                               % (self.checkpoint_path, EMA_SUFFIX))
            tensors = dict({k: v for k, v in tensors.items() if not k.endswith(EMA_SUFFIX)}, **avg)
        tr = Trainer(p, p.vocab_size)
        tr.load_state_dict(tensors)
        p._vc_trainer = tr
        pv = Parameters()
        pv.mode, pv.fine_tune = "inference", False          # dropout_keep 1.0
        vgg = VggEngine(pv, lib=tr.lib)
        if self.vgg_weights:
            vgg.load_weights(self.vgg_weights)
        elif all(n in tensors for n, _ in spec.vgg_variables()):
            vgg.load_params(tensors)
        else:
            raise ValueError("no VGG16 weights: give --vgg_weights vgg16_weights.npz (the checkpoint holds no cnn/* variables)")
        self._trainer, self._vgg = tr, vgg

    def _get_features(self, img_path):
        """Loads image, extracts fc2 features -> ([1, 4096] float32, PIL image)  (gen_caption.py:57-71)."""
        import torch
        from vae_captioning_amd.utils.image_utils import keras_load_img
        self._build()
        x, img = keras_load_img(img_path, target_size=(224, 224))
        fc2 = self._vgg.forward(torch.from_numpy(x).cuda())
        return fc2.cpu().numpy(), img

    def generate_caption(self, img_path, beam_size=2, diverse_draws=None, top_k=None, top_p=None, marginal_draws=None, must_include=None,
                         controls=None, typical_p=None, min_p=None, eta=None, contrastive_k=None, contrastive_alpha=None, diverse_select=None,
                         select_n=None, dpp_quality=None):
        """-> [{'image_id': file name, 'caption': text}]  (gen_caption.py:73-130).  gen_method "diverse" (additive): the record also holds
        "captions" / "scores" / "counts", every distinct caption of `diverse_draws` latent draws, best first.  top_k / top_p (additive):
        the truncation of sampled decoding ("sample", "diverse" with params.diverse_method "sample"), like the temperature taken from
        the params unless given; typical_p / min_p / eta (additive): the entropy- and peak-following cuts of sampled decoding, taken in
        the same way (not together with top_k / top_p).  gen_method "marginal_greedy" / "marginal_beam" (additive): the search under the mixture of
        `marginal_draws` latent draws (beam_size hypotheses for marginal_beam); the record also holds "marginal" and "draws".
        gen_method "constrained_beam" (additive): beam search whose caption mentions the words of `must_include` ("dog,puppy;frisbee":
        ';' separates sets, ',' the words of a set, any of which satisfies it); the record also holds "constraints", "satisfied", "score".
        controls (additive): a vae_captioning_amd.controls.DecodeControls -- no repeated n-gram, minimum length, repetition penalty,
        banned words -- for every gen_method but the marginal ones.  gen_method "stochastic_beam" (additive): beam_size distinct captions
        sampled without replacement (stochastic beam search); the record holds diverse's lists plus "logprob", "perturbed", "weight",
        "norm_weight" and "kappa".  gen_method "contrastive" (additive): contrastive search over the contrastive_k most likely words with
        the similarity penalty weighted by contrastive_alpha (each the params' unless given); the record also holds "logprob".
        diverse_select "dpp" (additive; gen_method "diverse" / "stochastic_beam"): select_n of the image's captions chosen jointly for
        quality and for difference from each other (DPP selection, quality weight dpp_quality; each the params' unless given); the
        record's lists hold them in selection order and gain "dpp_gain" and "dpp_chosen".  No training captions are at hand here, so
        the in-set CIDEr-D behind the selection weighs every n-gram alike (idf 1) where main.py uses the training captions' idf."""
        for name, val, conv in (("diverse_select", diverse_select, str), ("select_n", select_n, int), ("dpp_quality", dpp_quality, float)):
            if val is not None:
                setattr(self.params, name, conv(val))
        if top_k is not None:
            self.params.top_k = int(top_k)
        if top_p is not None:
            self.params.top_p = float(top_p)
        for name, val in (("typical_p", typical_p), ("min_p", min_p), ("eta", eta)):
            if val is not None:
                setattr(self.params, name, float(val))
        from vae_captioning_amd.vae_model.decoder import Decoder
        if not img_path or not os.path.exists(img_path):
            raise ValueError("Image not found")
        self._build()
        decoder = Decoder(None, None, None, self.params, self.data_dict)
        decoder.controls = controls
        if getattr(self.params, "diverse_select", "none") == "dpp":
            if self.gen_method not in ("diverse", "stochastic_beam"):
                raise ValueError("diverse_select dpp selects from a list of captions: gen_method diverse or stochastic_beam")
            import torch
            from vae_captioning_amd.mbr import CiderGram
            w2i, dev = self.data_dict.word2idx, self._trainer.cap.dev
            empty = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float32, device=dev), 0, 1.0)
            decoder.mbr = CiderGram(self._trainer.cap, None, w2i["<BOS>"], w2i["<EOS>"], df_table=empty)   # no df table: every n-gram's idf is 1
        im_id = [img_path.split("/")[-1]]
        feature_vector, image = self._get_features(img_path)
        c_v = self._c_v_generator(image) if self.params.use_c_v else None
        mode, own = self.gen_method, {}   # own: what this call gives the mode in place of its params defaults
        if mode not in ("greedy", "beam_search", "sample", "diverse", "marginal_greedy", "marginal_beam", "constrained_beam", "stochastic_beam", "contrastive"):
            raise ValueError("gen_method must be greedy, beam_search, sample, diverse, marginal_greedy, marginal_beam, constrained_beam, stochastic_beam "
                             "or contrastive")
        if mode in ("beam_search", "marginal_greedy", "marginal_beam", "stochastic_beam"):
            own["beam_size"] = int(beam_size)
        if mode == "diverse":
            own["draws"] = diverse_draws
        if mode in ("marginal_greedy", "marginal_beam"):
            own.update(method=mode, draws=marginal_draws)
        if mode == "contrastive":
            own.update(k=contrastive_k, alpha=contrastive_alpha)
        if mode == "constrained_beam":
            from vae_captioning_amd.constraints import parse_must_include
            w2i = self.data_dict.word2idx
            decoder.constraints = parse_must_include(must_include or "", w2i, self.data_dict.vocab_size, w2i["<BOS>"], w2i["<EOS>"])
            print(decoder.constraints.summary())
        return decoder.decode(mode, im_id, feature_vector, c_v, **own)


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Specify generation parameters")
    parser.add_argument("--img_path", help="Path to the image")
    parser.add_argument("--checkpoint", help="Model checkpoint path")
    parser.add_argument("--vocab_path", default="./pickles/capt_vocab.pickle", help="Indices to words dictionary")
    parser.add_argument("--gpu", default="", help="Specify GPU number if use GPU")
    parser.add_argument("--c_v_generator", default=None, help="If use cluster vectors, specify tensorflow api model (unused, as in the reference)")
    parser.add_argument("--gen_method", default="greedy", help="greedy, beam_search, sample, diverse, marginal_greedy, marginal_beam, constrained_beam, stochastic_beam or contrastive")
    parser.add_argument("--params_path", default=None, help="specify params pickle file")
    parser.add_argument("--beam_size", default=2, help="If using beam_search, specify beam_size; --gen_method stochastic_beam: distinct captions to sample (1..32)")
    parser.add_argument("--vgg_weights", default=None, help="vgg16_weights.npz for the feature extractor (additive flag)")
    parser.add_argument("--diverse_draws", type=int, default=None, help="--gen_method diverse: latent draws (default: the params' diverse_draws)")
    parser.add_argument("--top_k", type=int, default=None, help="sampled decoding: draw from the k most likely words (0 = all; default: the params')")
    parser.add_argument("--top_p", type=float, default=None, help="sampled decoding: draw from the nucleus holding this share of the probability "
                                                                  "((0, 1], 1 = all; default: the params')")
    parser.add_argument("--typical_p", type=float, default=None, help="sampled decoding: locally typical sampling, the words closest in surprisal "
                                                                      "to the prediction's entropy that hold this share ((0, 1], 1 = all; "
                                                                      "default: the params'; not with --top_k / --top_p)")
    parser.add_argument("--min_p", type=float, default=None, help="sampled decoding: the words at least this fraction as likely as the most "
                                                                  "likely one ([0, 1], 0 = all; default: the params')")
    parser.add_argument("--eta_cutoff", type=float, default=None, help="sampled decoding: eta sampling, the words with probability >= min(eta, "
                                                                       "sqrt(eta) * exp(-entropy)) ([0, 1), 0 = all; default: the params')")
    parser.add_argument("--marginal_draws", type=int, default=None, help="--gen_method marginal_greedy / marginal_beam: latent draws whose "
                                                                         "mixture is searched (1..256; default: the params' marginal_draws)")
    parser.add_argument("--must_include", default=None, help="--gen_method constrained_beam: words the caption must mention, e.g. "
                                                             "\"dog,puppy;frisbee\" (';' separates sets, ',' the words of a set; any word of a "
                                                             "set satisfies it; at most 3 sets of 4 words)")
    parser.add_argument("--no_repeat_ngram", type=int, default=0, help="no n-gram of this length twice in the caption (0..8; 0 = off)")
    parser.add_argument("--min_len", type=int, default=0, help="no <EOS> before this many words (0 = off)")
    parser.add_argument("--repetition_penalty", type=float, default=1.0, help="the logit of every word already in the caption is divided "
                                                                              "(positive) or multiplied (negative) by this (1..10; 1 = off)")
    parser.add_argument("--must_exclude", default=None, help="words the caption must not hold, e.g. \"a,the\" (vocabulary words or token ids)")
    parser.add_argument("--contrastive_k", type=int, default=None, help="--gen_method contrastive: next words looked one decoder step ahead per "
                                                                        "round (1..16; default: the params', 5)")
    parser.add_argument("--contrastive_alpha", type=float, default=None, help="--gen_method contrastive: weight of the similarity penalty against "
                                                                              "the word's probability ([0, 1], 0 = greedy; default: the params', 0.6)")
    parser.add_argument("--diverse_select", default=None, choices=["none", "dpp"], help="--gen_method diverse / stochastic_beam: dpp keeps "
                        "--select_n captions chosen jointly for quality and for difference from each other (default: the params')")
    parser.add_argument("--select_n", type=int, default=None, help="--diverse_select dpp: captions kept (1..32; default: the params', 5)")
    parser.add_argument("--dpp_quality", type=float, default=None, help="--diverse_select dpp: the best-ranked caption weighs e^W times the "
                                                                        "worst ([0, 8], 0 = diversity alone; default: the params', 1.0)")
    parser.add_argument("--use_ema", action="store_true", help="caption with the averaged weights (<name>/ExponentialMovingAverage) that a "
                                                               "run with --ema_decay wrote into the checkpoint")
    args = parser.parse_args()
    if not 0 <= args.no_repeat_ngram <= 8:
        parser.error("--no_repeat_ngram must be 0..8 (got %d)" % args.no_repeat_ngram)
    if args.min_len < 0:
        parser.error("--min_len must be >= 0 (got %d)" % args.min_len)
    if not (1.0 <= args.repetition_penalty <= 10.0):
        parser.error("--repetition_penalty must be in [1, 10] (got %r)" % args.repetition_penalty)
    controlled = args.no_repeat_ngram or args.min_len or args.repetition_penalty != 1.0 or args.must_exclude is not None
    if controlled and args.gen_method in ("marginal_greedy", "marginal_beam"):
        parser.error("--no_repeat_ngram / --min_len / --repetition_penalty / --must_exclude do not go with --gen_method %s" % args.gen_method)
    if (args.gen_method == "constrained_beam") != (args.must_include is not None):
        parser.error("--gen_method constrained_beam and --must_include go together")
    if args.marginal_draws is not None and not 1 <= args.marginal_draws <= 256:
        parser.error("--marginal_draws must be 1..256 (got %d)" % args.marginal_draws)
    if args.top_k is not None and args.top_k < 0:
        parser.error("--top_k must be >= 0 (got %d)" % args.top_k)
    if args.top_p is not None and not (0.0 < args.top_p <= 1.0):
        parser.error("--top_p must be in (0, 1] (got %r)" % args.top_p)
    if args.typical_p is not None and not (0.0 < args.typical_p <= 1.0):
        parser.error("--typical_p must be in (0, 1] (got %r)" % args.typical_p)
    if args.min_p is not None and not (0.0 <= args.min_p <= 1.0):
        parser.error("--min_p must be in [0, 1] (got %r)" % args.min_p)
    if args.eta_cutoff is not None and not (0.0 <= args.eta_cutoff < 1.0):
        parser.error("--eta_cutoff must be in [0, 1) (got %r)" % args.eta_cutoff)
    if args.gen_method == "stochastic_beam" and not 1 <= int(args.beam_size) <= 32:
        parser.error("--beam_size must be 1..32 with --gen_method stochastic_beam (got %s)" % args.beam_size)
    if args.gen_method != "contrastive" and (args.contrastive_k is not None or args.contrastive_alpha is not None):
        parser.error("--contrastive_k / --contrastive_alpha belong to --gen_method contrastive (got --gen_method %s)" % args.gen_method)
    if args.contrastive_k is not None and not 1 <= args.contrastive_k <= 16:
        parser.error("--contrastive_k must be 1..16 (got %d)" % args.contrastive_k)
    if args.contrastive_alpha is not None and not (0.0 <= args.contrastive_alpha <= 1.0):
        parser.error("--contrastive_alpha must be in [0, 1] (got %r)" % args.contrastive_alpha)
    if args.diverse_select == "dpp" and args.gen_method not in ("diverse", "stochastic_beam"):
        parser.error("--diverse_select dpp belongs to --gen_method diverse / stochastic_beam (got --gen_method %s)" % args.gen_method)
    if args.diverse_select != "dpp" and (args.select_n is not None or args.dpp_quality is not None):
        parser.error("--select_n / --dpp_quality belong to --diverse_select dpp")
    if args.select_n is not None and not 1 <= args.select_n <= 32:
        parser.error("--select_n must be 1..32 (got %d)" % args.select_n)
    if args.dpp_quality is not None and not (0.0 <= args.dpp_quality <= 8.0):
        parser.error("--dpp_quality must be in [0, 8] (got %r)" % args.dpp_quality)
    if args.gpu != "":
        os.environ["HIP_VISIBLE_DEVICES"] = args.gpu
    generator = Generator(checkpoint_path=args.checkpoint, params_path=args.params_path, vocab_path=args.vocab_path,
                          gen_method=args.gen_method, vgg_weights=args.vgg_weights, use_ema=args.use_ema)
    controls = None
    if controlled:
        from vae_captioning_amd.controls import DecodeControls, parse_banned
        words = [int(w) if w.lstrip("-").isdigit() else w for w in (x.strip() for x in (args.must_exclude or "").split(",")) if w]
        controls = DecodeControls(args.no_repeat_ngram, args.min_len, args.repetition_penalty, parse_banned(words, generator.data_dict))
    caption = generator.generate_caption(args.img_path, args.beam_size, args.diverse_draws, args.top_k, args.top_p, args.marginal_draws, args.must_include,
                                         controls, args.typical_p, args.min_p, args.eta_cutoff, args.contrastive_k, args.contrastive_alpha,
                                         args.diverse_select, args.select_n, args.dpp_quality)
    if args.gen_method == "diverse":
        for text, score, count in zip(caption[0]["captions"], caption[0]["scores"], caption[0]["counts"]):
            print("%.4f x%d %s" % (score, count, text))
    elif args.gen_method == "stochastic_beam":   # distinct captions sampled without replacement: probability, normalised weight, text
        for text, lp, w in zip(caption[0]["captions"], caption[0]["logprob"], caption[0]["norm_weight"]):
            print("logp %.4f w %.4f %s" % (lp, w, text))
    else:
        print(caption[0]["caption"])
