"""CPU: the host end of caption-set evaluation (vae_captioning_amd/evaluate.py, csrc/evaluate.hip) -- the new C-ABI entry and its
argument checks (which run before any device work), the --eval_captions flag, the plain-Python reference tests/eval_ref.py and the
product's float64 BLEU formula on cases worked by hand, and the metrics file of the inference driver with a fake evaluator."""
import contextlib
import ctypes
import io
import json
import math
import os

import numpy as np
import pytest

from vae_captioning_amd import abi
from vae_captioning_amd.utils.parameters import Parameters

from . import eval_ref as ref
from . import inference_fakes as fakes

NEW = ["vc_ngram_overlap"]
X = 4096   # a non-null pointer value: the checks must refuse the call before anything dereferences it
POINTERS = ("c_off", "c_nnz", "c_keys", "c_w", "c_len", "r_off", "r_nnz", "r_keys", "r_w", "r_len", "lo", "hi", "skip", "total", "match",
            "distinct", "unseen", "ref_len")
ORDER = ("stream", "C", "c_off", "c_nnz", "c_keys", "c_w", "c_len", "n_ref", "r_off", "r_nnz", "r_keys", "r_w", "r_len", "lo", "hi", "skip",
         "total", "match", "distinct", "unseen", "ref_len")
BOS, EOS = 1, 2
THE, CAT, IS, ON, MAT, THERE, A = 3, 4, 5, 6, 7, 8, 9


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return abi.load()


def test_new_entry_is_declared_exported_and_additive(built):
    protos = abi.parse_header()
    cdll = ctypes.CDLL(abi.LIB_PATH)
    for n in NEW:
        assert n in protos and hasattr(cdll, n), n
        getattr(built, n)   # binds: every argument type is one the ctypes layer knows
    assert [a for _, a in protos["vc_ngram_overlap"][1]] == list(ORDER)
    assert built.vc_abi_version() == 4


@pytest.mark.parametrize("kw", [{p: None} for p in POINTERS] + [dict(C=-1), dict(n_ref=-1), dict(n_ref=1 << 31), dict(C=1 << 34)],
                         ids=["null-" + p for p in POINTERS] + ["C-negative", "n_ref-negative", "n_ref-2^31", "C-2^34"])
def test_overlap_rejects_bad_arguments_without_a_device(built, kw):
    a = dict({p: X for p in POINTERS}, stream=None, C=8, n_ref=40)
    a.update(kw)
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_ngram_overlap(*[a[k] for k in ORDER])


def test_host_range_check_names_the_row():
    from vae_captioning_amd.evaluate import check_ranges
    lo, hi, skip = check_ranges([0, 2], [2, 5], [-1, 3], 2, 5)
    assert lo.dtype == hi.dtype == skip.dtype == np.int32 and hi.tolist() == [2, 5]
    for bad in (([0, 3], [2, 2], [-1, -1]), ([0, 2], [2, 6], [-1, -1]), ([-1, 2], [2, 5], [-1, -1])):
        with pytest.raises(ValueError, match="row [01]: range"):
            check_ranges(*bad, 2, 5)
    with pytest.raises(ValueError, match="one entry per hypothesis"):
        check_ranges([0], [2, 5], [-1, -1], 2, 5)
    with pytest.raises(ValueError, match="skip"):
        check_ranges([0, 2], [2, 5], [-2, -1], 2, 5)


# ------------------------------------------------------------------ flags
def test_eval_captions_flag_defaults_off_and_needs_inference():
    assert Parameters().eval_captions is False and Parameters().parse_args([]).eval_captions is False
    p = Parameters().parse_args(["--mode", "inference", "--eval_captions"])
    assert p.eval_captions is True and p.mode == "inference"
    for bad in (["--eval_captions"], ["--eval_captions", "--mode", "training"]):
        with pytest.raises(SystemExit):
            Parameters().parse_args(bad)


# ------------------------------------------------------------------ BLEU, by hand
REF1 = [THE, CAT, IS, ON, THE, MAT]             # "the cat is on the mat"
REF2 = [THERE, IS, A, CAT, ON, THE, MAT]        # "there is a cat on the mat"


def _bleus():
    from vae_captioning_amd.evaluate import corpus_bleu
    return (ref.corpus_bleu, corpus_bleu)


def test_clipping_on_the_classic_example():
    o = ref.overlap([THE] * 7, [REF1, REF2])
    # "the" occurs twice in REF1 and once in REF2: the seven are clipped to 2; "the the" is in neither; lengths 6 and 7 against 7:
    # |6 - 7| = 1 > |7 - 7| = 0, so the closest reference has 7 words
    assert o["total"] == [7, 6, 5, 4] and o["match"] == [2, 0, 0, 0]
    assert o["distinct"] == [1, 1, 1, 1] and o["unseen"] == [0, 1, 1, 1] and o["ref_len"] == 7
    for bleu in _bleus():
        b = bleu(o["match"], o["total"], 7, 7)
        assert abs(b[0] - 2.0 / 7.0) < 1e-15 and b[1:] == [0.0, 0.0, 0.0]


def test_a_hypothesis_equal_to_a_reference_scores_one():
    o = ref.overlap(list(REF1), [REF2, REF1])
    assert o["match"] == o["total"] == [6, 5, 4, 3] and o["unseen"] == [0, 0, 0, 0] and o["ref_len"] == 6
    assert o["distinct"] == [5, 5, 4, 3]      # "the" twice
    for bleu in _bleus():
        assert bleu(o["match"], o["total"], 6, o["ref_len"]) == [1.0, 1.0, 1.0, 1.0]


def test_brevity_penalty():
    hyp = REF1[:4]                                # "the cat is on": every n-gram matches, C = 4 < R = 6
    o = ref.overlap(hyp, [REF1])
    assert o["match"] == o["total"] == [4, 3, 2, 1] and o["ref_len"] == 6
    for bleu in _bleus():
        for b in bleu(o["match"], o["total"], 4, 6):
            assert abs(b - math.exp(1.0 - 6.0 / 4.0)) <= 1e-15
        assert bleu(o["match"], o["total"], 6, 6) == [1.0] * 4 and bleu(o["match"], o["total"], 9, 6) == [1.0] * 4   # C >= R: no penalty
        assert bleu([0] * 4, [0] * 4, 0, 6) == [0.0] * 4                                                           # C = 0


def test_a_length_tie_goes_to_the_shorter_reference():
    hyp = [THE, CAT, IS, ON, MAT]                 # L = 5 against references of 3 and 7 words, in both orders
    short, long_ = [A, CAT, IS], [THERE, IS, A, CAT, ON, THE, MAT]
    assert ref.overlap(hyp, [short, long_])["ref_len"] == 3 and ref.overlap(hyp, [long_, short])["ref_len"] == 3
    assert ref.overlap(hyp, [])["ref_len"] == 0 and ref.overlap(hyp, [])["match"] == [0, 0, 0, 0]
    assert ref.overlap(hyp, [])["unseen"] == ref.overlap(hyp, [])["distinct"] == [5, 4, 3, 2]
    assert ref.overlap([], [short]) == dict(total=[0] * 4, match=[0] * 4, distinct=[0] * 4, unseen=[0] * 4, ref_len=3)


def test_the_product_formula_equals_the_reference_formula_on_random_sums():
    from vae_captioning_amd.evaluate import corpus_bleu
    rng = np.random.default_rng(3)
    for _ in range(200):
        total = np.sort(rng.integers(0, 5000, size=4))[::-1]
        match = [int(rng.integers(0, t + 1)) for t in total]
        C, R = int(rng.integers(0, 6000)), int(rng.integers(0, 6000))
        np.testing.assert_allclose(corpus_bleu(match, total, C, R), ref.corpus_bleu(match, total.tolist(), C, R), rtol=1e-14, atol=0)


# ------------------------------------------------------------------ the set metrics, by hand
def test_set_metrics_on_four_captions_worked_by_hand():
    a, b, c, d, e, f = 3, 4, 5, 6, 7, 8
    caps = [[BOS, a, b, c, d, EOS], [a, b, c, d, EOS], [BOS, a, b, c, d, e, EOS], [f]]      # "a b c d" twice, "a b c d e", "f"
    refs = [[[BOS, a, b, EOS]]]
    got = ref.evaluate([caps], refs, BOS, EOS, train_captions=[[BOS, a, b, c, d, EOS], [BOS, f, EOS], [BOS, e, EOS]], cider=False)
    assert got["distinct"] == 3 / 4                      # three distinct word sequences of four listed
    assert got["div_1"] == 6 / 14                        # a b c d e f over 4 + 4 + 5 + 1 words
    assert got["div_2"] == 4 / 14                        # ab bc cd de
    assert got["novel"] == 1 / 4                         # only "a b c d e" is not a training caption
    # mBLEU: each caption against the other three.
    #   "a b c d" (twice): its twin is among the others -> match = total = (4, 3, 2, 1), closest length 4
    #   "a b c d e": e, de, cde, bcde are new -> match (4, 3, 2, 1) of total (5, 4, 3, 2); lengths 4, 4, 1 against 5 -> 4
    #   "f": match 0 of total (1, 0, 0, 0); lengths 4, 4, 5 against 1 -> 4
    # sums: match (12, 9, 6, 3), total (14, 10, 7, 4), C = 14, R = 16
    want = math.exp(1 - 16 / 14) * math.exp((math.log(12 / 14) + math.log(9 / 10) + math.log(6 / 7) + math.log(3 / 4)) / 4)
    assert abs(got["mbleu_4"] - want) <= 1e-15
    assert ref.corpus_bleu([12, 9, 6, 3], [14, 10, 7, 4], 14, 16)[3] == got["mbleu_4"]
    # the top caption "a b c d" against "a b": unigrams 2 of 4, bigrams 1 of 3, no trigram; C = 4 >= R = 2
    assert abs(got["bleu_1"] - 0.5) <= 1e-15 and abs(got["bleu_2"] - math.sqrt(0.5 / 3)) <= 1e-15 and got["bleu_3"] == got["bleu_4"] == 0.0
    # lists of one and empty lists: distinct 1.0 over the images that list a caption, no mBLEU hypotheses
    one = ref.evaluate([[caps[0]], []], refs * 2, BOS, EOS, cider=False)
    assert one["distinct"] == 1.0 and one["mbleu_4"] == 0.0 and one["novel"] is None and one["div_1"] == 1.0 and one["div_2"] == 3 / 4


# ------------------------------------------------------------------ the driver's metrics file
class _Evaluator(object):
    def __init__(self, references, log):
        self.references, self.log = references, log

    def evaluate(self, candidates):
        from vae_captioning_amd.evaluate import METRICS
        self.log.append((self.references, candidates))
        out = {k: 0.125 * (i + 1) for i, k in enumerate(METRICS)}
        out["novel"] = None
        out["per_image"] = dict(captions=np.ones(len(candidates)))
        return out


class _Decoder(fakes.Decoder):
    def __init__(self, trace, log):
        fakes.Decoder.__init__(self, trace)
        self.log, self.last_token_ids = log, None

    def online_inference(self, sess, image_ids, f_images, placeholder, c_v=None):
        self.last_token_ids = [[[BOS, 3 + int(i), EOS]] for i in image_ids]
        return [{"image_id": int(i), "caption": "greedy %d" % i} for i in image_ids], None

    def caption_evaluator(self, references):
        return _Evaluator(references, self.log)


class _Gen(fakes.Gen):
    """a generator that holds no caption table: its batches' own captions (one per image, 2-D, as Batch_Generator yields them) are used"""

    def next_val_batch(self, get_image_ids=False, use_obj_vectors=False):
        for images, _, _, ids, c_v in fakes.Gen.next_val_batch(self, get_image_ids, use_obj_vectors):
            lab = np.array([[20 + i, 21 + i, EOS] if i != 5 else [15, EOS, 0] for i in ids], np.int32)
            yield images, (None, lab), np.array([3 if i != 5 else 2 for i in ids], np.int32), ids, c_v


def _run(tmp, flag):
    from vae_captioning_amd.ops.inference import inference
    params = fakes.Params(use_c_v=False, prior="Normal", sample_gen="greedy")
    if flag is not None:
        params.eval_captions = flag
    trace, log, cwd = [], [], os.getcwd()
    os.makedirs(tmp)
    os.chdir(tmp)
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            inference(params, _Decoder(trace, log), _Gen(trace, [[3, 5, 8], [13]]), _Gen(trace, [[21]]), "PH", fakes.Saver(trace), "SESS")
        return {f: open(f, "rb").read() for f in sorted(os.listdir("."))}, log, buf.getvalue()
    finally:
        os.chdir(cwd)


def test_the_metrics_file_of_the_inference_driver(tmp_path):
    from vae_captioning_amd.evaluate import METRICS
    plain, log0, out0 = _run(str(tmp_path / "plain"), None)       # params without the attribute at all: the reference's own Parameters
    off, log1, out1 = _run(str(tmp_path / "off"), False)
    on, log2, out2 = _run(str(tmp_path / "on"), True)
    assert sorted(plain) == sorted(off) == ["test_fx.json", "val_fx.json"] and plain == off and log0 == log1 == [] and out0 == out1
    assert sorted(on) == ["test_fx.json", "val_fx.json", "val_fx_metrics.json"]
    assert on["val_fx.json"] == off["val_fx.json"] and on["test_fx.json"] == off["test_fx.json"]      # the records' JSON is unchanged
    assert json.loads(on["val_fx.json"]) == [{"image_id": i, "caption": "greedy %d" % i} for i in (3, 5, 8, 13)]
    m = json.loads(on["val_fx_metrics.json"])
    assert set(METRICS) <= set(m) and "per_image" not in m and m["novel"] is None and m["bleu_4"] == 0.5
    assert m["images"] == 4 and m["captions"] == 4 and m["sample_gen"] == "greedy" and m["beam_size"] == 3
    (refs, cands), = log2                                         # evaluated once, after the loop, on everything decoded
    assert cands == [[[BOS, 3 + i, EOS]] for i in (3, 5, 8, 13)]
    assert refs == [[[23, 24, EOS]], [[15, EOS]], [[28, 29, EOS]], [[33, 34, EOS]]]
    for k in METRICS:
        assert ("\n%s: " % k) in "\n" + out2
    assert out2.startswith(out1[:out1.index("wrote 4 captions to ./val_fx.json")])



def test_a_decoder_that_leaves_no_ids_is_an_error_not_the_previous_batch(tmp_path, monkeypatch):
    from vae_captioning_amd.ops.inference import inference

    class Forgetful(_Decoder):
        def online_inference(self, sess, image_ids, f_images, placeholder, c_v=None):
            if len(image_ids) == 1:       # the second batch: the records come back, the ids do not
                return fakes.Decoder.online_inference(self, sess, image_ids, f_images, placeholder, c_v)
            return _Decoder.online_inference(self, sess, image_ids, f_images, placeholder, c_v)

    params = fakes.Params(use_c_v=False, prior="Normal", sample_gen="greedy")
    params.eval_captions = True
    monkeypatch.chdir(tmp_path)
    with pytest.raises(RuntimeError, match="last_token_ids"):
        inference(params, Forgetful([], []), _Gen([], [[3, 5, 8], [13]]), None, "PH", None, "SESS")


# ------------------------------------------------------------------ the references of a real Batch_Generator
def test_inference_hands_the_evaluator_every_human_caption_of_each_validation_image(tmp_path, monkeypatch):
    """Batch_Generator.next_val_batch carries ONE randomly drawn caption per image (a 2-D label array); --eval_captions must score
    against all five captions of the fixture's images, whatever the generator's random state, aligned with the image ids."""
    from vae_captioning_amd.ops.inference import inference
    from vae_captioning_amd.utils.batch_gen import Batch_Generator
    from vae_captioning_amd.utils.captions import Captions, Dictionary
    from . import coco_fixture
    root = coco_fixture.build(tmp_path / "coco")
    monkeypatch.chdir(tmp_path)
    d = Dictionary(Captions(root + "annotations/captions_train2014.json").captions, 1)
    got = []
    for seed in (42, 7):
        val = Captions(root + "annotations/captions_val2014.json")
        val.index_captions(d.word2idx)
        feats = {fn: np.zeros((1, 8), np.float32) for fn in val.captions}
        gen = Batch_Generator(root + "images/val2014/", root + "annotations/captions_val2014.json", val, 3, feature_dict=feats,
                              get_image_ids=True, seed=seed)
        one = [lab for _, (_, lab), _, _, _ in gen.next_val_batch(get_image_ids=True)]
        assert all(lab.ndim == 2 for lab in one)                       # what the batches carry: one caption per image
        params = fakes.Params(use_c_v=False, prior="Normal", sample_gen="greedy")
        params.eval_captions = True
        log = []
        with contextlib.redirect_stdout(io.StringIO()):
            inference(params, _Decoder([], log), gen, None, "PH", None, "SESS")
        (refs, cands), = log
        by_id = {val.filename_to_imid[fn]: caps for fn, caps in val.captions_indexed.items()}
        ids = [c[0][1] - 3 for c in cands]                             # _Decoder encodes the image id in what it "decodes"
        assert sorted(ids) == sorted(by_id) and len(refs) == 4
        for i, r in zip(ids, refs):
            assert len(r) == 5 and r == by_id[i], i
        got.append({i: r for i, r in zip(ids, refs)})
        assert json.load(open("val_fx_metrics.json"))["images"] == 4
    assert got[0] == got[1]                                            # no dependence on the generator's random state


def test_training_captions_come_from_the_caption_table_without_features():
    from vae_captioning_amd import consensus as cs
    from .test_consensus_host import _FakeGen
    g = _FakeGen()
    g.feature_dict = g.val_feature_dict = None          # --fine_tune: no precomputed features, the captions are still there
    assert cs.captions_from_generator(g) == [[[BOS, 5, EOS]], [[BOS, 6, EOS], [BOS, 7, EOS]], [[BOS, 8, EOS]], [[BOS, 9, EOS]]]
