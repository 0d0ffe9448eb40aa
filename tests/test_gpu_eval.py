"""-m gpu: evaluation of caption sets (vae_captioning_amd/evaluate.py, csrc/evaluate.hip).  vc_ngram_overlap against the plain-Python
reference of tests/eval_ref.py with exact equality of its five integer outputs, in the three range forms the evaluator uses; its
independence of the launch; CIDEr-D through the evaluator against tests/consensus_ref.py; CaptionEvaluator.evaluate end to end;
exact identities of the set metrics on captions of the small model; and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd.abi import ptr as P
from vae_captioning_amd.consensus import word_rows
from vae_captioning_amd.evaluate import METRICS, CaptionEvaluator, _split, count_vectors, ngram_overlap

from . import eval_ref as ref

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("total", "match", "distinct", "unseen", "ref_len")
DEV = "cuda"


def _caps(rng, n, vocab, lo=0, hi=20):
    return [[BOS] + rng.integers(3, vocab, size=rng.integers(lo, hi + 1)).tolist() + [EOS] for _ in range(n)]


def _table(lib, caps):
    W, L = word_rows(caps, BOS, EOS)
    return count_vectors(lib, torch.device(DEV, torch.cuda.current_device()), W, L, BOS, EOS)


def _planted(rng, n_img, K, n_refs, vocab):
    """candidates and references of n_img images with the rows that can go wrong planted (image p holds plant p in its first slot)"""
    cands = [_caps(rng, K, vocab) for _ in range(n_img)]
    refs = [_caps(rng, n_refs, vocab) for _ in range(n_img)]
    cands[0][0] = [BOS] + [4] * 64 + [EOS]                      # 64 words, one repeated word: counts 64 / 63 / 62 / 61
    refs[0][0] = [4] * 64
    cands[1][0] = [BOS, EOS]                                    # an empty hypothesis
    cands[2][0] = [0, BOS, 5, 0, 6, EOS, 0, 5, 6, 7, BOS]       # PAD, <BOS> and <EOS> inside a caption: the words are 5 6 5 6 7
    refs[2][-1] = [5, 6, 0, 0, 5, EOS, 6, 7]
    cands[3][0] = list(refs[3][-1])                             # identical to a reference
    cands[4][0] = [BOS, 3, 4, 5, 6, 7, EOS]                     # the length tie: 5 words against 3 and 7 words (and nothing closer)
    refs[4][0] = [BOS, 3, 4, 5, 6, 7, 8, 3, EOS]
    if n_refs >= 2:
        refs[4][1:] = [[BOS, 3, 4, 5, EOS]] + [[BOS] + [8] * 12 + [EOS]] * (n_refs - 2)
    if K >= 3:                                                  # the same tie among an image's own earlier captions
        cands[5][:3] = [BOS, 3, 4, 5, 6, 7, 8, 3, EOS], [BOS, 3, 4, 5, EOS], [BOS, 3, 4, 5, 6, 7, EOS]
    return cands, refs


def _from_max(hyp, m_of, ref_lens):
    """the five outputs from the hypothesis's words, m_of(n, gram) = the largest count over the range, and the range's lengths"""
    out = dict(total=[], match=[], distinct=[], unseen=[], ref_len=0)
    for n in range(1, 5):
        c = ref.grams(hyp, n)
        out["total"].append(sum(c.values()))
        out["match"].append(sum(min(v, m_of(n, g)) for g, v in c.items()))
        out["distinct"].append(len(c))
        out["unseen"].append(sum(1 for g in c if m_of(n, g) == 0))
    if ref_lens:
        out["ref_len"] = min((abs(l - len(hyp)), l) for l in ref_lens)[1]
    return out


def _earlier(cw):
    """per caption of one image its outputs against the image's earlier captions: a running maximum per n-gram"""
    run, lens, out = {}, [], []
    for c in cw:
        out.append(_from_max(c, lambda n, g: run.get((n, g), 0), lens))
        for n in range(1, 5):
            for g, v in ref.grams(c, n).items():
                run[(n, g)] = max(run.get((n, g), 0), v)
        lens.append(len(c))
    return out


def _others(cw):
    """per caption of one image its outputs against the image's other captions: per n-gram the two largest counts and the owner of the
    largest, so that leaving a caption out costs one look-up"""
    top = {}
    for i, c in enumerate(cw):
        for n in range(1, 5):
            for g, v in ref.grams(c, n).items():
                a, ia, b = top.get((n, g), (0, -1, 0))
                top[(n, g)] = (v, i, a) if v > a else (a, ia, max(b, v))
    out = []
    for i, c in enumerate(cw):
        def m_of(n, g, i=i):
            a, ia, b = top.get((n, g), (0, -1, 0))
            return b if ia == i else a
        out.append(_from_max(c, m_of, [len(x) for j, x in enumerate(cw) if j != i]))
    return out


def _expected(cands, refs, rng):
    """per range form the expected outputs of every caption row.  `references` is eval_ref.overlap itself; the two forms among an image's
    own captions cost K^2 pairs per image, so they come from the incremental look-ups above, which are themselves checked against
    eval_ref.overlap -- on every row of lists of up to 20 captions; of longer lists on every row of the first image (the one with
    the 64-word plant) and on the first two, the last and 8 drawn rows of each other image."""
    want = dict(references=[], earlier=[], others=[])
    for cs, rs in zip(cands, refs):
        cw, rw = [ref.words(c, BOS, EOS) for c in cs], [ref.words(r, BOS, EOS) for r in rs]
        want["references"] += [ref.overlap(c, rw) for c in cw]
        early, other = _earlier(cw), _others(cw)
        every = len(cw) <= 20 or not want["earlier"]
        for i in (range(len(cw)) if every else sorted(set([0, 1, len(cw) - 1] + rng.integers(0, len(cw), size=8).tolist()))):
            assert early[i] == ref.overlap(cw[i], cw[:i]) and other[i] == ref.overlap(cw[i], cw[:i] + cw[i + 1:]), i
        want["earlier"] += early
        want["others"] += other
    return want


def _ranges(cands, refs):
    per, nr = np.array([len(c) for c in cands]), np.array([len(r) for r in refs])
    co, ro = np.concatenate([[0], np.cumsum(per)]), np.concatenate([[0], np.cumsum(nr)])
    img = np.repeat(np.arange(len(cands)), per)
    rows, none = np.arange(co[-1]), np.full(co[-1], -1)
    return dict(references=(ro[img], ro[img + 1], none), earlier=(co[img], rows, none), others=(co[img], co[img + 1], rows))


def _launch_all(lib, cands, refs):
    hyp = _table(lib, [c for cs in cands for c in cs])
    rt = _table(lib, [r for rs in refs for r in rs])
    rg = _ranges(cands, refs)
    return {form: ngram_overlap(lib, hyp, rt if form == "references" else hyp, *rg[form]) for form in rg}


def _assert_equal(got, want, what):
    for k in KEYS:
        w = np.array([o[k] for o in want], np.int32)
        assert got[k].dtype == np.int32 and got[k].shape == w.shape, (what, k)
        bad = np.flatnonzero((got[k] != w).reshape(len(want), -1).any(axis=1))
        assert bad.size == 0, (what, k, "row %d: got %s want %s" % (bad[0], got[k][bad[0]], w[bad[0]]))


@pytest.mark.parametrize("vocab", [9, 30])
@pytest.mark.parametrize("n_refs", [1, 5])
@pytest.mark.parametrize("K", [1, 2, 20, 256])
def test_overlap_equals_the_reference_exactly_in_the_three_range_forms(lib, K, n_refs, vocab):
    """7 images, K captions each (256: 64 workgroups' worth of hypotheses per image, references ranges of up to 255 rows), lengths
    0..20; vocabulary 9 repeats n-grams within a caption, so the clipping decides most counts.  The first caption of every image has
    an empty range of earlier captions (lo == hi); with K = 1 the range of other captions is one row, which skip names."""
    rng = np.random.default_rng(1000 * K + 10 * n_refs + vocab)
    cands, refs = _planted(rng, 7, K, n_refs, vocab)
    got = _launch_all(lib, cands, refs)
    want = _expected(cands, refs, rng)
    for form in ("references", "earlier", "others"):
        _assert_equal(got[form], want[form], form)
    r = got["references"]
    assert r["total"][0].tolist() == [64, 63, 62, 61] and r["match"][0].tolist() == [64, 63, 62, 61] and r["distinct"][0].tolist() == [1] * 4
    assert r["total"][K].tolist() == [0] * 4 and r["distinct"][K].tolist() == [0] * 4            # the empty hypothesis
    assert r["total"][2 * K].tolist() == [5, 4, 3, 2]                                          # 5 6 5 6 7
    assert r["match"][3 * K].tolist() == r["total"][3 * K].tolist()                             # equal to a reference
    assert r["ref_len"][4 * K] == (3 if n_refs >= 2 else 7)                                     # the tie goes to the shorter
    e, o = got["earlier"], got["others"]
    first = np.arange(7) * K
    assert not e["match"][first].any() and not e["ref_len"][first].any() and np.array_equal(e["unseen"][first], e["distinct"][first])
    if K == 1:
        assert not o["match"].any() and not o["ref_len"].any() and np.array_equal(o["unseen"], o["distinct"])
    if K >= 3:
        assert e["ref_len"][5 * K + 2] == 3 and e["ref_len"][5 * K + 1] == 7 and o["ref_len"][0] > 0


def test_ranges_at_the_edges_and_the_device_clamp(lib):
    """explicit lo / hi / skip: an empty range, a one-row range that skip empties, a skip outside the range (drops nothing), a skip inside;
    and, past the host check, what the library documents for a bad range: clamped into the table, lo > hi empty"""
    rng = np.random.default_rng(8)
    hyps, refs = _caps(rng, 9, 9, 1, 12), _caps(rng, 11, 9, 1, 12)
    hw, rw = [ref.words(c, BOS, EOS) for c in hyps], [ref.words(c, BOS, EOS) for c in refs]
    lo = np.array([0, 4, 4, 2, 2, 0, 10, 11, 3])
    hi = np.array([0, 5, 5, 9, 9, 11, 11, 11, 4])
    skip = np.array([-1, 4, 7, 1, 5, 10, -1, -1, 3])
    hyp, rt = _table(lib, hyps), _table(lib, refs)
    got = ngram_overlap(lib, hyp, rt, lo, hi, skip)
    want = [ref.overlap(hw[c], [rw[r] for r in range(lo[c], hi[c]) if r != skip[c]]) for c in range(9)]
    _assert_equal(got, want, "edges")
    for c in (0, 1, 7, 8):
        assert not got["match"][c].any() and got["ref_len"][c] == 0 and np.array_equal(got["unseen"][c], got["distinct"][c])
    with pytest.raises(ValueError, match="row 1: range"):
        ngram_overlap(lib, hyp, rt, [0, 5] + [0] * 7, [0, 4] + [0] * 7, None)
    with pytest.raises(ValueError, match="row 0: range"):
        ngram_overlap(lib, hyp, rt, [0] * 9, [12] * 9, None)
    # the library's own clamp (the host check bypassed)
    blo = np.array([-5, 7, 3, 11, 40, 0, 2, 2, 2], np.int32)
    bhi = np.array([50, 3, 3, 99, 50, -3, 11, 2, 1], np.int32)
    clo = np.clip(blo, 0, 11)
    chi = np.clip(np.maximum(bhi, clo), 0, 11)
    rg = torch.from_numpy(np.stack([blo, bhi, np.full(9, -1, np.int32)])).to(DEV)
    out = torch.empty(17 * 9, dtype=torch.int32, device=DEV)
    o = [P(out) + 16 * 9 * i for i in range(5)]
    lib.vc_ngram_overlap(torch.cuda.current_stream().cuda_stream, 9, P(hyp.off), P(hyp.nnz), P(hyp.keys), P(hyp.w), P(hyp.words), 11,
                         P(rt.off), P(rt.nnz), P(rt.keys), P(rt.w), P(rt.words), P(rg), P(rg) + 36, P(rg) + 72, *o)
    _assert_equal(_split(out.cpu().numpy(), 9), [ref.overlap(hw[c], rw[clo[c]:chi[c]]) for c in range(9)], "clamp")


def test_rows_do_not_depend_on_the_launch(lib):
    """integer sums and maxima: the rows of three images launched alone equal the same rows of the full launch bit for bit, and a
    second call returns the first call's arrays"""
    rng = np.random.default_rng(21)
    cands, refs = _planted(rng, 7, 20, 5, 9)
    full, again = _launch_all(lib, cands, refs), _launch_all(lib, cands, refs)
    sub = [2, 4, 5]
    part = _launch_all(lib, [cands[i] for i in sub], [refs[i] for i in sub])
    rows = np.concatenate([np.arange(20 * i, 20 * i + 20) for i in sub])
    for form in full:
        for k in KEYS:
            assert np.array_equal(full[form][k], again[form][k]), (form, k)
            assert np.array_equal(full[form][k][rows], part[form][k]), (form, k)
    assert full["others"]["match"].any() and full["earlier"]["unseen"].any()


def _related(rng, n_img, K, n_refs, vocab, lo=8, hi=16):
    """references, and candidates that are references with a fifth of their words replaced and a random cut: n-grams of every order
    match somewhere, and differ somewhere"""
    refs = [_caps(rng, n_refs, vocab, lo, hi) for _ in range(n_img)]
    cands = []
    for rs in refs:
        cs = []
        for _ in range(K):
            c = np.array(rs[rng.integers(len(rs))][1:-1])
            c = np.where(rng.random(c.size) < 0.2, rng.integers(3, vocab, size=c.size), c)[:rng.integers(4, c.size + 1)]
            cs.append([BOS] + c.tolist() + [EOS])
        cands.append(cs)
    return cands, refs


def test_cider_d_through_the_evaluator_matches_the_float64_reference(lib):
    """each caption's CIDEr-D = the mean over its image's references of consensus_ref.cider_d (idf over the evaluated references), with
    test_gpu_consensus.py's bound for the same kernel and arithmetic; the oracle picks the reference's caption wherever the reference's
    best two differ by more than 1e-5 relative"""
    rng = np.random.default_rng(33)
    cands, refs = _related(rng, 7, 20, 5, 30)
    cands[3] = cands[3][:1]
    cands[5][7] = list(refs[5][2])                            # a candidate that IS a reference
    res = CaptionEvaluator(lib, refs, BOS, EOS, vocab_size=30).evaluate(cands)
    want = ref.cider_scores(cands, refs, BOS, EOS)
    got = res["per_image"]["caption_cider_d"]
    checked = 0
    for b in range(7):
        np.testing.assert_allclose(got[b], want[b], rtol=1e-5, atol=1e-6)
        s = np.sort(want[b])[::-1]
        if s.size < 2 or s[0] - s[1] > 1e-5 * abs(s[0]):
            assert int(np.argmax(got[b])) == int(np.argmax(want[b])), b
            checked += 1
    assert checked >= 4 and got[5][7] > np.median(got[5])
    np.testing.assert_allclose(res["cider_d"], np.mean([w[0] for w in want]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res["oracle_cider_d"], np.mean([w.max() for w in want]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res["mean_cider_d"], np.mean(np.concatenate(want)), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res["per_image"]["oracle_cider_d"], [w.max() for w in want], rtol=1e-5, atol=1e-6)
    assert res["cider_d"] <= res["oracle_cider_d"] and res["mean_cider_d"] <= res["oracle_cider_d"]


def test_evaluate_end_to_end_against_the_reference(lib):
    """12 images x 20 captions x 5 references, vocabulary 30; image 4 lists nothing and image 9 one caption.  Both sides apply the same
    float64 formula to identical integers: 1e-12 relative."""
    rng = np.random.default_rng(44)
    cands, refs = _related(rng, 12, 20, 5, 30)
    cands[4], cands[9] = [], cands[9][:1]
    cands[2][5], cands[2][11] = list(cands[2][0]), [BOS] + cands[2][0][1:-1] + [0, 0]      # equal word sequences, other tokens
    train = [c for cs in cands[:6] for c in cs[::3]] + [r for rs in refs for r in rs]
    res = CaptionEvaluator(lib, refs, BOS, EOS, vocab_size=30, train_captions=train).evaluate(cands)
    want = ref.evaluate(cands, refs, BOS, EOS, train_captions=train, cider=False)
    assert set(res) == set(METRICS) | {"per_image"}
    for k in ("bleu_1", "bleu_2", "bleu_3", "bleu_4", "mbleu_4", "div_1", "div_2", "distinct", "novel"):
        assert isinstance(res[k], float) and want[k] > 0.0, k
        np.testing.assert_allclose(res[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    assert res["bleu_1"] >= res["bleu_2"] >= res["bleu_3"] >= res["bleu_4"] > 0 and 0 < res["novel"] < 1
    per = res["per_image"]
    assert per["captions"].tolist() == [20] * 4 + [0] + [20] * 4 + [1] + [20] * 2
    assert np.isnan(per["distinct"][4]) and np.isnan(per["cider_d"][4]) and np.isnan(per["div_1"][4]) and per["distinct"][9] == 1.0
    assert per["distinct"][2] <= 18 / 20
    # the skips the definitions ask for: nothing of image 4 anywhere; image 9 in the top-caption and Div-n numbers, not in mBLEU
    keep = [b for b in range(12) if b != 4]
    sub = CaptionEvaluator(lib, [refs[b] for b in keep], BOS, EOS, vocab_size=30, train_captions=train).evaluate([cands[b] for b in keep])
    for k in ("bleu_1", "bleu_4", "mbleu_4", "div_1", "div_2", "distinct", "novel"):
        assert sub[k] == res[k], k                     # (CIDEr-D differs: its idf counts the images evaluated)
    no9 = [b for b in keep if b != 9]
    sub = CaptionEvaluator(lib, [refs[b] for b in no9], BOS, EOS, vocab_size=30).evaluate([cands[b] for b in no9])
    assert sub["mbleu_4"] == res["mbleu_4"] and sub["bleu_1"] != res["bleu_1"] and sub["novel"] is None
    # lists of one: the documented values of the set metrics
    one = CaptionEvaluator(lib, refs, BOS, EOS).evaluate([cs[:1] for cs in cands])
    assert one["distinct"] == 1.0 and one["mbleu_4"] == 0.0 and one["bleu_4"] == res["bleu_4"]
    assert one["oracle_cider_d"] == one["cider_d"] == one["mean_cider_d"]
    with pytest.raises(ValueError, match="caption 1 of image 2 has 65 words"):
        CaptionEvaluator(lib, refs, BOS, EOS).evaluate([[[3]], [], [[3], [4] * 65]] + [[]] * 9)
    with pytest.raises(ValueError, match="at most 256 captions per image"):
        CaptionEvaluator(lib, refs, BOS, EOS).evaluate([[[3]] * 257] + [[]] * 11)
    with pytest.raises(ValueError, match="image 1 has no reference"):
        CaptionEvaluator(lib, [refs[0], []], BOS, EOS)


def test_set_metrics_of_group_beam_search_on_the_small_model(lib):
    """Captions of test_gpu_generate.py's small model by group beam search (3 groups of 2 beams).  With diversity 0 every group is the
    same beam search, so the merged list of an image has at most 2 captions.  The ordering "a positive penalty gives no lower Div-1
    and no higher mBLEU-4" is NOT asserted, because it does not hold here.  Measured on this model and seed (MI355X): diversity 0 gives
    lists of 2, 2, 1, 1, 2, 2 captions with Div-1 0.8333, Div-2 0.1111, mBLEU-4 0.0; diversity 0.8 gives lists of 4, 4, 2, 3, 4, 3
    captions with Div-1 0.8167, Div-2 0.1389, mBLEU-4 0.0.  Div-1 FALLS with the penalty: Div-n divides by the words of the whole list
    and the penalty makes the list longer.  mBLEU-4 is 0.0 on both sides (no caption shares a 4-gram with another of its image), so
    its ordering holds only trivially and says nothing.  What holds by construction is asserted instead.  Listing every caption of every image twice
    (i) leaves every image's set of n-grams, hence the Div-n numerators, unchanged while the words double: Div-n halves exactly (a
    division by two and a sum of halves are exact in binary floating point); (ii) leaves the distinct sequences unchanged while the
    listed captions double: `distinct` halves exactly; (iii) gives every caption a twin among the image's other captions: every
    clipped count equals its total and the closest length is the caption's own, so mBLEU-4 is exactly 1.0; (iv) keeps the first
    caption: BLEU and CIDEr-D of the top caption, and the oracle, are unchanged."""
    from vae_captioning_amd.generate import merge_groups
    from .test_gpu_generate import setup
    p, eng, gen, _, feats, cv, eps, _ = setup(lib, 7, prior="Normal")
    rng = np.random.default_rng(7)
    lists = {}
    for lam in (0.0, 0.8):
        res = gen.diverse_beam_search(feats, None, eps, BOS, EOS, groups=3, group_size=2, diversity=lam, max_len=12)
        lists[lam] = [[e[0] for e in merge_groups(per_group)] for per_group in res]
    assert all(1 <= len(cs) <= 2 for cs in lists[0.0]) and all(1 <= len(cs) <= 6 for cs in lists[0.8])
    refs = [[cs[0]] + _caps(rng, 2, 40, 3, 10) for cs in lists[0.0]]
    ev = CaptionEvaluator(eng, refs, BOS, EOS, vocab_size=40)
    for lam, cands in lists.items():
        a = ev.evaluate(cands)
        b = ev.evaluate([[c for c in cs for _ in range(2)] for cs in cands])
        want = ref.evaluate(cands, refs, BOS, EOS, cider=False)
        for k in ("bleu_1", "bleu_4", "mbleu_4", "div_1", "div_2", "distinct"):
            np.testing.assert_allclose(a[k], want[k], rtol=1e-12, atol=0, err_msg=k)
        assert 0 < a["distinct"] <= 1 and 0 < a["div_1"] <= 1 and 0 <= a["mbleu_4"] <= 1
        assert b["div_1"] == a["div_1"] / 2 and b["div_2"] == a["div_2"] / 2 and b["distinct"] == a["distinct"] / 2
        assert any(len(ref.words(c, BOS, EOS)) >= 4 for cs in cands for c in cs) and b["mbleu_4"] == 1.0
        for k in ("bleu_1", "bleu_2", "bleu_3", "bleu_4", "cider_d", "oracle_cider_d"):
            assert b[k] == a[k], k
    assert ev.evaluate(lists[0.0])["bleu_1"] > 0          # the top caption of diversity 0 is the image's first reference


def test_main_synthetic_inference_with_eval_captions(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    common = ["--synthetic", "--vocab", "200", "--embed_dim", "32", "--enc_hid", "64", "--dec_hid", "64", "--latent", "10",
              "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz"]
    infer = common + ["--mode", "inference", "--sample_gen", "diverse", "--diverse_draws", "4"]
    runs = [common + ["--epochs", "1", "--max_steps", "1"], infer, infer + ["--eval_captions"]]
    files = []
    for args in runs:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=tmp_path, env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        files.append({f: open(tmp_path / f, "rb").read() for f in ("val_00.json", "val_00_diverse.json") if os.path.exists(tmp_path / f)})
        for f in files[-1]:
            os.remove(tmp_path / f)
        if args is infer:
            assert not os.path.exists(tmp_path / "val_00_metrics.json") and "bleu_1" not in r.stdout
    assert files[0] == {} and len(files[1]) == 2 and files[1] == files[2]          # byte-identical caption files with and without the flag
    m = json.load(open(tmp_path / "val_00_metrics.json"))
    assert set(METRICS) <= set(m) and "per_image" not in m
    assert m["images"] == 8 and 8 <= m["captions"] <= 32 and m["sample_gen"] == "diverse" and m["diverse_draws"] == 4
    for n in range(1, 5):
        assert 0.0 <= m["bleu_%d" % n] <= 1.0
    assert 0.0 <= m["cider_d"] <= m["oracle_cider_d"] and 0.0 < m["distinct"] <= 1.0 and 0.0 <= m["mbleu_4"] <= 1.0
    assert 0.0 <= m["novel"] <= 1.0 and 0.0 < m["div_1"] <= 1.0
    for k in METRICS:
        assert ("\n%s: " % k) in r.stdout, k
