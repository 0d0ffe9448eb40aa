#!/usr/bin/env python
"""Training / inference driver with the command line of the reference's main.py
(utils/parameters.py:75-132) on the MI355X-native hot path.

    python main.py --gpu 0 --synthetic [--prior AG --c_v] [--fine_tune] [--mode inference]
    python -m torch.distributed.run --nproc-per-node 8 main.py --synthetic --fine_tune   # data parallel

The flow follows main.py:43-297 step for step, with the graph-building classes replaced by the
eager facades of vae_captioning_amd (same names, same call order):
    vgg16 -> imf_emb/cv_emb -> Encoder.q_net -> KL -> Decoder.px_z_fi -> masked CE ->
    non_cnn_optimizer / cnn_optimizer -> print every 500 steps -> validate -> checkpoint per epoch.
The MSCOCO data layer (utils/data.py, batch_gen.py) is out of scope; `--synthetic` feeds seeded
batches with the same tensor contract (vae_captioning_amd/synth.py).
"""
import json
import os

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for multi-process GPU work (RCCL peer mappings)
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from vae_captioning_amd import objective, session, spec, synth  # noqa: E402
from vae_captioning_amd.ops import optimizers  # noqa: E402
from vae_captioning_amd.utils.parameters import Parameters  # noqa: E402
from vae_captioning_amd.vae_model.decoder import DIVERSE_FILE_MODES, Decoder  # noqa: E402
from vae_captioning_amd.vae_model.encoder import Encoder  # noqa: E402


class SyntheticDictionary(object):
    """Stand-in for utils/captions.py's Dictionary: ids 0 = <PAD>, 1 = <BOS>, 2 = <EOS>."""

    def __init__(self, vocab_size):
        self.vocab_size = vocab_size
        self.idx2word = {0: "<PAD>", synth.BOS: "<BOS>", synth.EOS: "<EOS>"}
        for i in range(3, vocab_size):
            self.idx2word[i] = "w%d" % i
        self.word2idx = {w: i for i, w in self.idx2word.items()}


class SyntheticBatches(object):
    """next_batch() yields (images_or_features, (inputs, labels), lengths, c_v) already flattened to
    N = B * num_captions rows -- the state after preprocess_captions (main.py:226-228)."""

    def __init__(self, params, steps, seed, T=20):
        self.p, self.steps, self.T = params, steps, T
        self.rng = np.random.default_rng(seed)

    def next_batch(self):
        p = self.p
        for _ in range(self.steps):
            b = synth.make_batch(self.rng, p.batch_size, p.num_captions, self.T, p.vocab_size, use_ci=spec.uses_ci(p),
                                 images=p.fine_tune, variable_len=True)
            yield b


def coco_batches(gen, params, epoch_rule=False, world=1):
    """Batch_Generator.next_batch items -> Trainer.set_batch dicts (main.py:222-238).  epoch_rule: keep
    re-shuffling and passing over the data until steps * batch_size > num_ex_per_epoch (main.py:217-221,256-259;
    --max_steps overrides); batch_size is the GLOBAL batch (world * per-rank batch) in data-parallel runs."""
    from vae_captioning_amd.utils.batch_gen import feed_dict
    steps = 0
    while True:
        for images, captions, lengths, c_v in gen.next_batch(use_obj_vectors=params.use_c_v, num_captions=params.num_captions):
            yield feed_dict(images, captions, lengths, c_v, params.num_captions, params.fine_tune)
            steps += 1
            if epoch_rule and (steps >= params.max_steps if params.max_steps else steps * params.batch_size * world > params.num_ex_per_epoch):
                return
        if not epoch_rule:
            return


def training_index_data(params, coco_train):
    """(fc2 features, captions per image) of the training images at hand, or None.  MSCOCO: the training generator's images (train +
    repartitioned val, never the held-out ones); --synthetic: 512 seeded images with 5 captions each."""
    from vae_captioning_amd.consensus import index_data_from_generator
    if coco_train is not None:
        return index_data_from_generator(coco_train)
    if params.synthetic:
        b = synth.make_batch(np.random.default_rng(params.seed + 11), 512, 5, 12, params.vocab_size, feature_size=params.cnn_feature_size)
        return b["features"], [[[int(t) for t in r] for r in b["cap_enc"][i * 5:(i + 1) * 5]] for i in range(512)]   # "w.. <EOS>", 11 words
    return None


def consensus_index(params, tr, cap_dict, coco_train):
    """--diverse_rerank consensus: the index of training images (fc2 features + captions, training_index_data) that diverse captions are
    re-ranked against."""
    from vae_captioning_amd.consensus import ConsensusIndex
    if params.fine_tune:
        raise SystemExit("--diverse_rerank consensus needs precomputed fc2 features for its index of training images; "
                         "an index from a fine-tuned VGG16 is not supported (drop --fine_tune)")
    data = training_index_data(params, coco_train)
    if data is None:
        raise SystemExit("--diverse_rerank consensus needs the MSCOCO training images (--coco_dir) or --synthetic")
    feats, caps = data
    bos, eos = cap_dict.word2idx["<BOS>"], cap_dict.word2idx["<EOS>"]
    print("consensus index: %d images, k = %d, m = %d" % (len(caps), params.consensus_k, params.consensus_m))
    return ConsensusIndex(tr.cap, feats, caps, bos, eos, k=params.consensus_k, m=params.consensus_m, vocab_size=cap_dict.vocab_size)


def mbr_gram(params, tr, cap_dict, coco_train, real=None, flag="--diverse_rerank mbr", what="mbr re-ranking"):
    """--diverse_rerank mbr / --diverse_select dpp: the idf table of the training captions (per image; no features are read, so
    --fine_tune works) that the in-set CIDEr-D of an image's captions is weighted with."""
    from vae_captioning_amd.mbr import CiderGram
    if real is not None:
        corpus = [real.caps[n] for n in real.names if real.caps[n]]
    elif coco_train is not None:
        from vae_captioning_amd.consensus import captions_from_generator
        corpus = [c for c in captions_from_generator(coco_train) if c]
    elif params.synthetic:
        corpus = training_index_data(params, None)[1]
    else:
        raise SystemExit("%s needs the MSCOCO training captions (--coco_dir) or --synthetic for its idf" % flag)
    print("%s: idf over the captions of %d training images" % (what, len(corpus)))
    return CiderGram(tr.cap, corpus, cap_dict.word2idx["<BOS>"], cap_dict.word2idx["<EOS>"], cap_dict.vocab_size)


def training_captions(params, coco_train):
    """--eval_captions: the flat training captions `novel` is measured against -- the captions of the training generator's images (a
    walk of its caption table: no features are read, so --fine_tune works too) or of --synthetic's seeded index; None when neither is
    at hand (`novel` is then null)."""
    if coco_train is not None:
        from vae_captioning_amd.consensus import captions_from_generator
        return [c for caps in captions_from_generator(coco_train) for c in caps]
    data = training_index_data(params, coco_train)
    return None if data is None else [c for caps in data[1] for c in caps]


def main(params):
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    backend = os.environ.get("VC_DIST_BACKEND", "nccl")  # gloo: several ranks on ONE GPU (tests only)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local if backend == "nccl" else local % torch.cuda.device_count())
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend, rank=rank, world_size=world)
    real = coco_train = coco_val = coco_test = None
    if params.captions_json and params.features_pickle:
        # precomputed-feature path of the reference's data layer (utils/data.py + utils/batch_gen.py)
        from vae_captioning_amd.utils.batch_gen import BatchGenerator
        from vae_captioning_amd.utils.captions import Captions, Dictionary
        caps = Captions(params.captions_json)
        cap_dict = Dictionary(caps.captions, params.keep_words)
        os.makedirs("./pickles", exist_ok=True)  # utils/captions.py:122-125: the vocabulary source gen_caption.py reloads
        with open("./pickles/capt_vocab.pickle", "wb") as wf:
            pickle.dump(file=wf, obj=caps.captions)
        with open(params.features_pickle, "rb") as rf:
            feats = pickle.load(rf)
        cvs = None
        if params.cluster_pickle:
            with open(params.cluster_pickle, "rb") as rf:
                cvs = pickle.load(rf)
        real = BatchGenerator(caps.index_captions(cap_dict.word2idx), feats, params.batch_size, cvs, seed=params.seed,
                              shard=(rank, world) if world > 1 else None)
    elif params.synthetic:
        cap_dict = SyntheticDictionary(params.vocab_size)
    else:
        # the reference's own path (main.py:23-41): MSCOCO directory -> Data -> train / val / test generators
        if not os.path.exists(params.coco_dir + "annotations/captions_train2014.json"):
            raise SystemExit("no MSCOCO under --coco_dir %r: give --synthetic, or --captions_json + --features_pickle" % params.coco_dir)
        from vae_captioning_amd.utils.data import Data
        repartiton = params.gen_val_captions >= 0  # main.py:20-26: train on train + val minus the last gen_val_captions images
        coco = Data(params, extract_features=not params.fine_tune, weights_path=params.image_net_weights_path,
                    repartiton=repartiton and not params.fine_tune, gen_val_cap=params.gen_val_captions)
        cap_dict = coco.dictionary
        coco_train = coco.load_train_data_generator(params.batch_size, params.fine_tune, shard=(rank, world) if world > 1 else None)
        coco_val = coco.get_valid_data(params.batch_size, val_tr_unused=coco_train.unused_cap_in, pretrained=not params.fine_tune)
        coco_test = coco.get_test_data(params.batch_size, pretrained=not params.fine_tune) if os.path.exists(coco.test_cap_json) else None
        os.makedirs("./pickles", exist_ok=True)
        with open("./pickles/capt_vocab.pickle", "wb") as wf:  # utils/captions.py:122-125
            pickle.dump(file=wf, obj=coco.captions_tr.captions)
    params.vocab_size = cap_dict.vocab_size  # main.py:92
    from vae_captioning_amd.trainer import Trainer
    tr = Trainer(params, params.vocab_size, world=world, rank=rank, seed=params.seed)
    params._vc_trainer = tr  # the facades below share it (session.get)
    tr.load_state_dict({**spec.init_caption_params(params, params.vocab_size, seed=params.seed),
                        **(spec.init_vgg_params(seed=params.seed) if params.fine_tune else {})})
    if params.mode == "training" and not params.restore:
        # main.py:205-208: the ImageNet weights are loaded whether or not the CNN is fine-tuned (the VGG16 variables always
        # exist in the reference graph and are saved with every checkpoint, quirk Q22)
        if os.path.exists(params.image_net_weights_path):
            print("Loading imagenet weights for futher usage")
            if params.fine_tune:
                tr.vgg.load_weights(params.image_net_weights_path)
            else:
                from vae_captioning_amd.trainer import imagenet_weights
                tr.cnn_host = imagenet_weights(params.image_net_weights_path)
        elif params.fine_tune:
            print("No %s: VGG16 starts from random weights" % params.image_net_weights_path)
        else:
            print("No %s: checkpoints of this run will not contain the cnn/* variables" % params.image_net_weights_path)
    # saver.save(sess, "./checkpoints/{}.ckpt") (main.py:286-288): TF V2 checkpoint files by default,
    # --ckpt_format npz for a name-keyed numpy archive
    ckpt = "./checkpoints/%s.ckpt" % params.checkpoint + (".npz" if params.ckpt_format == "npz" else "")
    if params.restore or params.mode == "inference":
        have = ckpt if params.ckpt_format == "npz" else ckpt + ".index"
        if not os.path.exists(have):  # saver.restore raises NotFoundError (main.py:209-212, ops/inference.py:6-7)
            raise FileNotFoundError("checkpoint %s not found (--restore / --mode inference need ./checkpoints/%s.ckpt*)" % (have, params.checkpoint))
        print("Restoring from checkpoint")
        tr.restore(ckpt, use_ema=bool(params.use_ema))   # --use_ema: the averaged weights in place of the last iterate
    steps_per_epoch = params.max_steps or (params.num_ex_per_epoch // (params.batch_size * world) + 1)  # main.py:217-221, global batch
    say = print if rank == 0 else (lambda *a, **k: None)

    if params.mode == "training":
        cap = tr.cap
        encoder = None if params.no_encoder else Encoder(None, None, None, params)
        decoder = Decoder(None, None, None, params, cap_dict)
        optimize, global_step, global_norm = optimizers.non_cnn_optimizer(None, params)
        optimize_cnn = (lambda: 0.0)
        if params.fine_tune:
            optimize_cnn, _ = optimizers.cnn_optimizer(None, params)
        if params.ema_decay > 0:   # --ema_decay: averaged inside the optimiser pass, validated and saved beside the last iterate
            say("Weight averaging: decay {} ({}), averages of {} variables".format(
                params.ema_decay, "with warm-up" if cap.ema_warmup else "constant", sum(len(e.store.names()) for e in tr._ema_engines())))
        gs = 0  # host mirror of global_step (it restarts at 0 on --restore, Q11): no device sync on non-print steps
        # --word_drop: decoder input words replaced by <UNK> on the host, before the upload (the embedding-gradient index is built from
        # the replaced ids; nothing on the device changes); training batches only
        drop_rng = np.random.default_rng([params.seed, 7919, rank]) if params.word_drop > 0 else None
        unk = objective.unk_id(cap_dict.word2idx, params.vocab_size)

        if params.scst:   # self-critical training: every step below is a Trainer.scst_step (DESIGN.md "Self-critical training")
            if world > 1:
                raise SystemExit("--scst is single-GPU: not in a data-parallel run (WORLD_SIZE = %d)" % world)
            if not params.restore:
                say("Warning: --scst without --restore starts self-critical training from random weights; it is meant to "
                    "fine-tune a cross-entropy-trained checkpoint")
            from vae_captioning_amd.scst import CiderReward
            if real is not None:
                corpus = [real.caps[n] for n in real.names if real.caps[n]]
            elif coco_train is not None:
                from vae_captioning_amd.consensus import captions_from_generator
                corpus = [c for c in captions_from_generator(coco_train) if c]
            else:
                corpus = training_index_data(params, None)[1]
            bos, eos = cap_dict.word2idx["<BOS>"], cap_dict.word2idx["<EOS>"]
            rouge_w = float(getattr(params, "scst_rouge", 0.0))
            say("SCST: document frequencies from %d training images, baseline %s, entropy weight %g" % (len(corpus), params.scst_baseline, params.scst_entropy)
                + (", ROUGE-L weight %g" % rouge_w if rouge_w > 0 else ""))
            reward = CiderReward(cap, corpus, bos, eos, cap_dict.vocab_size)
            if rouge_w > 0:   # the reward is CIDEr-D + W * ROUGE-L; with 0 it is the CiderReward alone and vc_lcs_overlap is never launched
                from vae_captioning_amd.scst import RougeReward, SumReward
                reward = SumReward([(reward, 1.0), (RougeReward(cap, bos, eos), rouge_w)])
            tr.enable_scst(reward, bos, eos, baseline=params.scst_baseline, beta=params.scst_entropy)

        def say_scst(e, it):
            s = tr.scst_stats
            say("Epoch: {} Iteration: {} SCST: reward: {} baseline: {} sample_len: {} entropy: {}".format(e, it, s["reward"], s["baseline"], s["sample_len"], s["entropy"]))

        def say_objective():   # --kl_free_bits: what the floor does, beside the losses
            if cap.free_bits > 0:
                o = tr.objective_stats()
                say("Free bits: kl_raw: {} floored_share: {}".format(o["kl_raw"], o["floored_share"]))

        def say_ul():   # --unlikelihood: the penalty before its weight, and the probability the model puts on words the caption has already said
            if cap.unlikelihood > 0:
                o = tr.objective_stats()
                say("Unlikelihood: ul: {} candidates: {} repeat_mass: {}".format(o["ul"], o["ul_candidates"], o["repeat_mass"]))

        def say_bow():   # --bow_loss: the z-only head's loss per bag word, the distinct words per caption and the probability it puts on them
            if cap.bow_loss > 0:
                o = tr.objective_stats()
                say("BoW: bow: {} words: {} mass: {}".format(o["bow"], o["bow_words"], o["bow_mass"]))

        def say_sched():   # --sched_sampling: the rate of the last step and the share of its eligible words that were replaced (this rank's rows)
            o = tr.sched_stats()
            if o is not None:
                say("Sched sampling: rate: {} replaced_share: {}".format(o["rate"], o["replaced"] / max(o["eligible"], 1)))
        for e in range(params.num_epochs):
            if real is not None:
                it = real.next_batch(use_obj_vectors=spec.uses_ci(params), num_captions=params.num_captions)
            elif coco_train is not None:
                it = coco_batches(coco_train, params, epoch_rule=True, world=world)
            else:
                it = SyntheticBatches(params, steps_per_epoch, params.seed + 17 * e + rank).next_batch()
            for batch in it:
                if batch["cap_dec"].shape[0] != params.batch_size * params.num_captions:
                    continue  # ragged last batch: shapes are static on device
                if drop_rng is not None:
                    batch = dict(batch, cap_dec=objective.word_dropout(batch["cap_dec"], batch["lengths"], params.word_drop, unk, drop_rng))
                if params.scst:
                    tr.scst_step(batch)
                    gs += 1
                    if (gs - 1) % 500 == 0:
                        say_scst(e, gs - 1)
                    continue
                tr.set_batch(batch)
                # ---- one sess.run([kld, rec_loss, lower_bound, optimize, optimize_cnn, annealing]) ----
                feats = None
                if tr.vgg is not None:
                    feats = tr.vgg.forward(tr.images, cap.step)
                    if tr.vgg.wd:
                        tr.vgg.reg_sumsq(cap.red.data_ptr() + 12)
                images_fv = cap.fw_prepare(feats)                       # main.py:84-108
                if encoder is not None:
                    encoder.images_fv = decoder.images_fv = images_fv
                    qz, tm_list, tv_list = encoder.q_net()              # main.py:117
                dec_model, x_logits, shpe, _ = decoder.px_z_fi({} if params.no_encoder else {"z": qz})  # main.py:146-150
                cap.fw_loss(train=True)                                 # main.py:152-177
                optimize()                                              # main.py:179
                optimize_cnn()                                          # main.py:183
                gs += 1
                if (gs - 1) % 500 == 0:
                    kl, rl, lb, ann = tr.losses()
                    say("Epoch: {} Iteration: {} VLB: {} Rec Loss: {}".format(e, gs - 1, lb, rl))
                    if not params.no_encoder:
                        say("Annealing coefficient:{} KLD: {}".format(ann, kl))
                        say_objective()
                    say_ul()
                    say_bow()
                    say_sched()
            if params.scst:
                if tr.scst_stats is not None:
                    say_scst(e, int(global_step.item()))
            else:
                kl, rl, lb, ann = tr.losses()
                say("Epoch: {} Iteration: {} VLB: {} Rec Loss: {}".format(e, int(global_step.item()), lb, rl))
                if not params.no_encoder:
                    say_objective()
                say_ul()
                say_bow()
                say_sched()
            # validate(): rec_loss of the training graph on held-out batches (main.py:262-284)
            val = []
            held_out = coco_batches(coco_val, params) if coco_val is not None else SyntheticBatches(params, 4, params.seed + 99991 + rank).next_batch()
            for batch in held_out:
                if batch["cap_dec"].shape[0] != params.batch_size * params.num_captions:
                    continue
                tr.set_batch(batch)
                val.append(tr.eval_rec_loss())
            say("Validation reconstruction loss: {}".format(np.mean(val)))
            if params.ema_decay > 0:   # the same loop over the same held-out batches on the averaged weights
                val = []
                held_out = coco_batches(coco_val, params) if coco_val is not None else SyntheticBatches(params, 4, params.seed + 99991 + rank).next_batch()
                with tr.ema_weights():
                    for batch in held_out:
                        if batch["cap_dec"].shape[0] != params.batch_size * params.num_captions:
                            continue
                        tr.set_batch(batch)
                        val.append(tr.eval_rec_loss())
                say("Validation reconstruction loss (averaged weights, decay {}): {}".format(params.ema_decay, np.mean(val)))
            say("-----------------------------------------------")
            if rank == 0:
                os.makedirs("./checkpoints", exist_ok=True)
                tr.save(ckpt)
                say("Model saved in file: %s" % ckpt)
    if params.mode == "inference":
        # ops/inference.py:4-39: captions for the validation images -> ./val_{gen_name}.json
        decoder = Decoder(None, None, None, params, cap_dict)
        if params.sample_gen in ("diverse", "stochastic_beam") and params.diverse_rerank == "consensus":
            decoder.consensus_index = consensus_index(params, tr, cap_dict, coco_train)
        if params.sample_gen in ("diverse", "stochastic_beam") and params.diverse_rerank == "mbr":
            decoder.mbr = mbr_gram(params, tr, cap_dict, coco_train, real)
        if getattr(params, "diverse_select", "none") == "dpp" and decoder.mbr is None:   # (the parser admits it in the three list modes only)
            decoder.mbr = mbr_gram(params, tr, cap_dict, coco_train, real, "--diverse_select dpp", "dpp selection")
        if params.sample_gen == "constrained_beam":   # the words the captions must mention, looked up in the vocabulary once
            from vae_captioning_amd.constraints import load_constraints
            decoder.constraints = load_constraints(params.constraints, cap_dict.word2idx, cap_dict.vocab_size, cap_dict.word2idx["<BOS>"],
                                                   cap_dict.word2idx["<EOS>"], params.cbs_width)
            say(decoder.constraints.summary())
        from vae_captioning_amd.controls import from_params   # --no_repeat_ngram / --min_len / --repetition_penalty / --banned_words
        decoder.controls = from_params(params, cap_dict)
        if decoder.controls is not None:
            say(decoder.controls.summary())
        if params.eval_captions and rank == 0:
            decoder.train_captions = training_captions(params, coco_train)
        if coco_val is not None:  # ops/inference.py:4-56 on the validation / test image sets
            from vae_captioning_amd.ops.inference import inference
            if rank == 0:
                inference(params, decoder, coco_val, coco_test)
            if world > 1:
                dist.destroy_process_group()
            return
        rng = np.random.default_rng(params.seed + 5)
        captions_gen, scores, bounds, references, decoded = [], [], [], [], []
        selecting, ranked_gen = getattr(params, "diverse_select", "none") == "dpp", []
        for it in range(2):
            b = synth.make_batch(rng, params.batch_size, 1, 20, params.vocab_size, use_ci=spec.uses_ci(params), images=params.fine_tune)
            ids = ["synthetic_%06d" % (it * params.batch_size + i) for i in range(params.batch_size)]
            pics = b["images"] if params.fine_tune else b["features"]
            c_v = b.get("c_v")
            sent = decoder.decode(params.sample_gen, ids, pics, c_v)
            if params.sample_gen == "diverse":   # every distinct caption of every image, best first
                for r in sent:
                    say("%s: %s" % (r["image_id"], " | ".join("%s (x%d)" % (t, n) for t, n in zip(r["captions"], r["counts"]))))
            elif params.sample_gen == "diverse_beam":   # group beam search: the groups' captions merged, best first
                for r in sent:
                    say("%s: %s" % (r["image_id"], " | ".join("%s (groups %s)" % (t, ",".join(map(str, g))) for t, g in zip(r["captions"], r["groups"]))))
            elif params.sample_gen == "stochastic_beam":   # --beam_size distinct captions sampled without replacement, with their weights
                for r in sent:
                    say("%s: %s" % (r["image_id"], " | ".join("%s (logp %.3f, w %.3g)" % (t, lp, w) for t, lp, w in zip(r["captions"], r["logprob"], r["norm_weight"]))))
            captions_gen += sent
            # --diverse_select dpp: ./val_{gen_name}.json keeps the records of the whole ranked lists, the file of a run without the flag
            ranked_gen += decoder.last_ranked_records if selecting else sent
            if params.eval_captions:   # the batch's own captions (one per image, by construction) are its "human" references
                from vae_captioning_amd.ops.inference import decoded_ids, human_captions
                references += human_captions((b["cap_dec"], b["cap_enc"]), b["lengths"])
                decoded += decoded_ids(decoder, len(ids))
            if params.score_draws:   # held-out likelihood of the batch's own ("human") captions under the prior
                from vae_captioning_amd.ops.inference import human_captions
                scores += decoder.score_captions(ids, pics, human_captions((b["cap_dec"], b["cap_enc"]), b["lengths"]), c_v)
            if params.bound_draws:   # the same captions bounded with draws from the model's own posterior
                from vae_captioning_amd.ops.inference import human_captions
                bounds += decoder.bound_captions(ids, pics, human_captions((b["cap_dec"], b["cap_enc"]), b["lengths"]), c_v)
        say("Generated {} captions".format(len(captions_gen)))
        if rank == 0:
            with open("./val_{}.json".format(params.gen_name), "w") as wj:
                json.dump(ranked_gen, wj)
            if params.sample_gen in DIVERSE_FILE_MODES:   # the full per-image lists under the name ops/inference.py gives them
                with open("./val_{}_diverse.json".format(params.gen_name), "w") as wj:
                    json.dump(captions_gen, wj)
            if params.score_draws:
                from vae_captioning_amd.ops.inference import store_scores
                store_scores(params, scores)
            if params.bound_draws:
                from vae_captioning_amd.ops.inference import store_bounds
                store_bounds(params, bounds, decoder.bound_stats)
            if params.eval_captions:
                from vae_captioning_amd.ops.inference import evaluate_decoded
                evaluate_decoded(params, decoder, references, decoded)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    params = Parameters()
    params.parse_args()
    if params.save_params:
        os.makedirs("./pickles", exist_ok=True)
        fn = "./pickles/params_{}_{}_{}_{}.pickle".format(params.prior, params.no_encoder, params.checkpoint, params.use_c_v)
        print("Saving params to: ", fn)
        with open(fn, "wb") as wf:
            pickle.dump(file=wf, obj={k: v for k, v in vars(params).items() if not k.startswith("_")})
    main(params)
