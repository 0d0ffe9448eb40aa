"""-m gpu: DPP selection (csrc/dpp.hip, vae_captioning_amd/mbr.py: CiderGram.select).  vc_dpp_select_f64 against the float64 reference
of tests/dpp_ref.py by REPLAY -- every pick of the kernel must be one the definition's own rounding cannot tell from the best -- at the
wave boundaries and the 256-caption limit, for n = 1, 8, 32 and quality weights 0, 1, 8; its independence of the launch, the place and
max_cands; its argument checks; CiderGram.select behind CaptionGenerator.diverse, behind an mbr re-ranking and in the decoder's
stochastic beam search; the command line."""
import json

import numpy as np
import pytest
import torch

from vae_captioning_amd import mbr
from vae_captioning_amd.abi import VaecapError

from . import consensus_ref as cref
from . import dpp_ref as ref
from . import gram_ref
from .gpu_util import P, dev, host, stream
from .test_gpu_consensus import _Dict, _facade_params
from .test_gpu_rouge import SMALL, _main

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
PER = (0, 1, 2, 5, 63, 64, 65, 256)    # captions per image: nothing, one, the wave boundaries and the limit
LD = 264                               # > 256: every row has padding columns, poisoned with NaN
GUARD = 7                              # canary elements behind sel, gain and n_dpp
NS, WS = (1, 8, 32), (0.0, 1.0, 8.0)
PICK_RTOL = 1e-9                       # a pick's reference d >= (1 - 1e-9) x the live maximum; gain within 1e-9 q_j^2
BAND = (1e-12, 1e-6)                   # no candidate's d / q^2 may lie in here at any step (a condition on the INPUTS: live-or-not is then
                                       # the same question for the kernel and for the reference)


def _variants(rng, base, n, vocab=40, swap=0.4):
    """n perturbed copies of a base caption: 40 % of the words replaced, cut to 6 .. len(base) words"""
    out = []
    for _ in range(n):
        c = np.where(rng.random(base.size) < swap, rng.integers(3, vocab, size=base.size), base)[:rng.integers(6, base.size + 1)]
        out.append([BOS] + c.tolist() + [EOS])
    return out


@pytest.fixture(scope="module")
def case():
    """the eight images (two exact duplicates planted in each with room for them), their float64 reference matrices rounded to f32, the
    ranking keys of every caption, and the [C, LD] table block with NaN in every padding column"""
    rng = np.random.default_rng(11)
    corpus = [_variants(rng, rng.integers(3, 40, size=12), 3) for _ in range(30)]
    idf, unseen = cref.df_idf(corpus, BOS, EOS)
    imgs = [_variants(rng, rng.integers(3, 40, size=12), n) for n in PER]
    for b, n in enumerate(PER):
        if n >= 5:
            imgs[b][n - 2], imgs[b][n // 2] = list(imgs[b][0]), list(imgs[b][1])     # caption 0 again near the end, caption 1 in the middle
    Gs = [gram_ref.gram(cs, idf, unseen).astype(np.float32) for cs in imgs]
    keys = [rng.standard_normal(n) for n in PER]
    cand_img = np.concatenate([[0], np.cumsum(PER)]).astype(np.int32)
    table = np.full((int(cand_img[-1]), LD), np.nan, np.float32)
    for b, G in enumerate(Gs):
        table[cand_img[b]:cand_img[b + 1], :PER[b]] = G
    return imgs, Gs, keys, cand_img, table


def _launch(lib, cand_img, table, q, n, b0=0, B=None, max_cands=256, ld=LD):
    """vc_dpp_select_f64 on images b0 .. b0 + B - 1 of the table -> (sel [B, n], gain [B, n], n_dpp [B]) and the three guard bands"""
    B = len(cand_img) - 1 - b0 if B is None else B
    sel = torch.full((B * n + GUARD,), -77, dtype=torch.int32, device="cuda")
    gain = torch.full((B * n + GUARD,), -77.0, dtype=torch.float64, device="cuda")
    nd = torch.full((B + GUARD,), -77, dtype=torch.int32, device="cuda")
    lib.vc_dpp_select_f64(stream(), B, P(dev(cand_img)) + 4 * b0, max_cands, P(dev(table)), ld, P(dev(q, np.float64)), n, P(sel), P(gain), P(nd))
    s, g, d = host(sel), host(gain), host(nd)
    return (s[:B * n].reshape(B, n), g[:B * n].reshape(B, n), d[:B]), (s[B * n:], g[B * n:], d[B:])


def _check_by_replay(G, q, n, sel, gain, n_dpp, what):
    """the kernel's answer for one image against the definition, following the kernel's own picks"""
    m = len(q)
    assert 0 <= n_dpp <= min(n, m), what
    picks = sel[:n_dpp]
    assert len(set(picks.tolist())) == n_dpp and ((picks >= 0) & (picks < m)).all(), (what, picks)
    steps, tail = ref.replay(G, q, n, picks)
    for k, (st, j) in enumerate(zip(steps, picks)):
        assert st["live"][j], "%s: pick %d of step %d is not live in the reference" % (what, j, k)
        top = st["d"][st["live"]].max()
        assert st["d"][j] >= (1.0 - PICK_RTOL) * top, "%s: step %d took %d with d %.17g, the live maximum is %.17g" % (what, k, j, st["d"][j], top)
        assert abs(gain[k] - st["d"][j]) <= PICK_RTOL * q[j] ** 2, "%s: gain %d is %.17g, reference %.17g" % (what, k, gain[k], st["d"][j])
    assert not tail["more"], "%s: the kernel stopped after %d picks with a live caption left" % (what, n_dpp)
    assert np.array_equal(sel, tail["sel"]), (what, sel, tail["sel"])                       # the picks, the fill order, the -1 tail
    assert (gain[n_dpp:] == 0.0).all() and np.array_equal(np.signbit(gain[n_dpp:]), np.zeros(n - n_dpp, bool)), what
    return tail


def _ratios_of_the_reference(G, q, n):
    """every untaken candidate's d / q^2 at every step of the reference's own run, and after its last"""
    sel, _, n_dpp = ref.select(G, q, n)
    steps, tail = ref.replay(G, q, n, sel[:n_dpp])
    out = [st["d"][~st["taken"]] / q[~st["taken"]] ** 2 for st in steps] + [tail["ratios"]]
    return np.concatenate(out) if out else np.zeros(0)


# ------------------------------------------------------------------ the kernel against the reference
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("n", NS)
def test_the_kernel_against_the_reference(lib, case, n, W):
    imgs, Gs, keys, cand_img, table = case
    qs = [mbr.dpp_quality(k, W) for k in keys]
    (sel, gain, nd), guards = _launch(lib, cand_img, table, np.concatenate(qs), n)
    for g in guards:
        assert (g == -77).all()
    seen = picks = 0
    for b, m in enumerate(PER):
        r = _ratios_of_the_reference(Gs[b], qs[b], n)
        seen += r.size
        assert not ((r > BAND[0]) & (r < BAND[1])).any(), "image %d: the inputs put a candidate on the live threshold: %r" % (b, r[(r > BAND[0]) & (r < BAND[1])])
        _check_by_replay(Gs[b], qs[b], n, sel[b], gain[b], int(nd[b]), "image %d (%d captions), n %d, W %g" % (b, m, n, W))
        want_sel, want_gain, want_nd = ref.select(Gs[b], qs[b], n)
        assert int(nd[b]) == want_nd, (b, int(nd[b]), want_nd)
        picks += want_nd
        if m:
            assert sel[b, 0] == int(np.argmax(qs[b])) and gain[b, 0] == qs[b].max() ** 2     # the first pick: the best quality, exactly
        if m >= 5 and n == 32:                                                              # the planted copies: filled, never chosen by gain
            chosen = set(sel[b, :nd[b]].tolist())
            assert not ({0, m - 2} <= chosen) and not ({1, m // 2} <= chosen), (b, sorted(chosen))
    assert sel[0].tolist() == [-1] * n and (gain[0] == 0).all() and nd[0] == 0               # no caption: -1 / 0 / 0
    assert sel[1].tolist() == [0] + [-1] * (n - 1) and nd[1] == 1
    print("n %d W %g: %d reference ratios outside the band, %d picks" % (n, W, seen, picks))


# ------------------------------------------------------------------ independence
def test_an_image_does_not_depend_on_the_launch_its_place_or_max_cands(lib, case):
    imgs, Gs, keys, cand_img, table = case
    n = 8
    q = np.concatenate([mbr.dpp_quality(k, 1.0) for k in keys])
    (sel, gain, nd), _ = _launch(lib, cand_img, table, q, n)
    (sel2, gain2, nd2), _ = _launch(lib, cand_img, table, q, n)                          # two calls: equal bits
    assert np.array_equal(sel, sel2) and np.array_equal(gain.view(np.int64), gain2.view(np.int64)) and np.array_equal(nd, nd2)
    for b in (3, 4, 6, 7):                                                               # alone, with the smallest max_cands that holds it
        (s1, g1, d1), guards = _launch(lib, cand_img, table, q, n, b0=b, B=1, max_cands=max(1, PER[b]))
        assert np.array_equal(s1[0], sel[b]) and np.array_equal(g1[0].view(np.int64), gain[b].view(np.int64)) and d1[0] == nd[b], b
        for g in guards:
            assert (g == -77).all()
    (s3, g3, d3), guards = _launch(lib, cand_img, table, q, n, b0=4, B=3, max_cands=65)   # images 4..6 at places 0..2 of a smaller launch
    assert np.array_equal(s3, sel[4:7]) and np.array_equal(g3.view(np.int64), gain[4:7].view(np.int64)) and np.array_equal(d3, nd[4:7])
    for g in guards:
        assert (g == -77).all()
    # n decides the LDS the kernel asks for (two instantiations), not the arithmetic: the first 8 picks of n = 32 are those of n = 8
    (s32, g32, d32), _ = _launch(lib, cand_img, table, q, 32)
    for b, m in enumerate(PER):
        k = min(int(nd[b]), 8)
        assert np.array_equal(s32[b, :k], sel[b, :k]) and np.array_equal(g32[b, :k].view(np.int64), gain[b, :k].view(np.int64)), b


# ------------------------------------------------------------------ argument errors
def test_bad_arguments_return_before_any_launch(lib, case):
    imgs, Gs, keys, cand_img, table = case
    B, n = len(PER), 4
    sel = torch.full((B * n,), -77, dtype=torch.int32, device="cuda")
    gain = torch.full((B * n,), -77.0, dtype=torch.float64, device="cuda")
    nd = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    head, g, q = dev(cand_img), dev(table), dev(np.ones(int(cand_img[-1])), np.float64)

    def call(B=B, head=P(head), max_cands=256, gram=P(g), ld=LD, q_=P(q), n=n, sel_=P(sel), gain_=P(gain), nd_=P(nd)):
        lib.vc_dpp_select_f64(stream(), B, head, max_cands, gram, ld, q_, n, sel_, gain_, nd_)
    for bad in (dict(B=-1), dict(max_cands=0), dict(max_cands=257), dict(n=0), dict(n=33), dict(ld=255), dict(max_cands=64, ld=63),
                dict(head=None), dict(gram=None), dict(q_=None), dict(sel_=None), dict(gain_=None), dict(nd_=None)):
        with pytest.raises(VaecapError, match="invalid argument"):
            call(**bad)
    call(B=0)
    call(B=0, head=None, gram=None, q_=None, sel_=None, gain_=None, nd_=None)             # B == 0: no pointer is looked at
    assert (host(sel) == -77).all() and (host(gain) == -77).all() and (host(nd) == -77).all()   # no launch so far
    call()
    assert (host(nd)[1:] >= 1).all() and host(nd)[0] == 0


# ------------------------------------------------------------------ through the layers
def _decoder(lib):
    from vae_captioning_amd.vae_model.decoder import Decoder
    p = _facade_params()
    dec = Decoder(None, None, None, p, _Dict)
    rng = np.random.default_rng(12)
    corpus = [_variants(rng, rng.integers(3, 40, size=9), 3) for _ in range(30)]
    dec.mbr = mbr.CiderGram(lib, corpus, BOS, EOS, vocab_size=40)
    return dec, p


def _check_selection(cg, ranked, chosen, n_dpp, n, W):
    """CiderGram.select's answer against dpp_ref on CiderGram.gram's own matrices"""
    Gs, _ = cg.gram([[e[0] for e in entries] for entries in ranked])
    for b, (entries, out, k) in enumerate(zip(ranked, chosen, n_dpp)):
        m = len(entries)
        q = mbr.dpp_quality(mbr.list_keys(entries), W)
        assert len(out) == min(n, m) and all(len(o) == len(entries[0]) + 1 for o in out)
        where = {tuple(e[0]): i for i, e in enumerate(entries)}
        sel = np.array([where[tuple(o[0])] for o in out] + [-1] * (n - len(out)), np.int32)
        assert len(set(sel[:len(out)].tolist())) == len(out)                             # distinct members of the list
        assert all(tuple(o[:-1]) == tuple(entries[j]) for o, j in zip(out, sel))         # the entries themselves, each extended by its gain
        gain = np.array([o[-1] for o in out] + [0.0] * (n - len(out)), np.float64)
        _check_by_replay(Gs[b], q, n, sel, gain, k, "image %d" % b)
        assert k == ref.select(Gs[b], q, n)[2]
        if m:
            assert sel[0] == 0                                                           # the list's first stays first


def test_select_behind_diverse_and_behind_an_mbr_reranking(lib, monkeypatch):
    dec, p = _decoder(lib)
    feats = np.maximum(np.random.default_rng(0).standard_normal((4, 48)), 0).astype(np.float32)
    res = dec._gen().diverse(feats, None, None, BOS, EOS, draws=20, method="sample", max_len=p.gen_max_len)
    assert max(len(r) for r in res) > 5                                                  # (there is something to select from)
    chosen, n_dpp = dec.mbr.select(res, 5)
    _check_selection(dec.mbr, res, chosen, n_dpp, 5, 1.0)
    again, n_again = dec.mbr.select(res, 5)
    assert again == chosen and n_again == n_dpp
    for W in (0.0, 8.0):
        c2, k2 = dec.mbr.select(res, 5, quality=W)
        _check_selection(dec.mbr, res, c2, k2, 5, W)
    reranked = dec.mbr.rerank(res)
    c3, k3 = dec.mbr.select(reranked, 5)
    _check_selection(dec.mbr, reranked, c3, k3, 5, 1.0)
    assert all(len(o) == 5 for out in c3 for o in out)                                   # (tokens, score, count, mbr, gain)
    # one image per chunk: the same answer
    monkeypatch.setattr(mbr, "GRAM_BLOCK_BYTES", 1)
    c4, k4 = dec.mbr.select(res, 5)
    monkeypatch.undo()
    assert c4 == chosen and k4 == n_dpp
    # explicit keys and explicit qualities; their argument errors
    keys = [[-float(i) for i in range(len(r))] for r in res]
    c5, k5 = dec.mbr.select(res, 3, quality=2.0, keys=keys)
    c6, k6 = dec.mbr.select(res, 3, weights=[mbr.dpp_quality(k, 2.0).tolist() for k in keys])
    assert c5 == c6 and k5 == k6
    with pytest.raises(ValueError, match="not both"):
        dec.mbr.select(res, 3, keys=keys, weights=keys)
    with pytest.raises(ValueError, match="one number per caption"):
        dec.mbr.select(res, 3, keys=keys[:-1])
    with pytest.raises(ValueError, match="finite and > 0"):
        dec.mbr.select(res, 3, weights=keys)
    assert dec.mbr.select([], 5) == ([], []) and dec.mbr.select([[], []], 5) == ([[], []], [0, 0])


def test_decoder_records_with_the_selection(lib, monkeypatch):
    dec, p = _decoder(lib)
    feats = np.maximum(np.random.default_rng(3).standard_normal((3, 48)), 0).astype(np.float32)
    p.diverse_draws, p.diverse_select, p.select_n = 20, "dpp", 5
    seen = {}
    real = dec.mbr.select

    def spy(ranked, n, **kw):
        seen["ranked"] = ranked
        return real(ranked, n, **kw)
    monkeypatch.setattr(dec.mbr, "select", spy)
    for rerank in ("likelihood", "mbr"):
        p.diverse_rerank = rerank
        recs = dec.diverse_inference(None, ["a", "b", "c"], feats, None, n_best=2)       # the selection stands in place of the n_best cut
        for r, toks, ranked in zip(recs, dec.last_token_ids, seen["ranked"]):
            assert set(r) == {"image_id", "caption", "captions", "scores", "counts", "dpp_gain", "dpp_chosen"} | ({"mbr"} if rerank == "mbr" else set())
            k = len(r["captions"])
            assert k == min(5, len(ranked)) == len(r["dpp_gain"]) == len(r["scores"]) == len(r["counts"]) == len(toks)
            assert r["captions"] == [dec._text(t, (BOS, EOS)) for t in toks] and r["caption"] == dec._text(ranked[0][0], (BOS, EOS)) == r["captions"][0]
            assert 1 <= r["dpp_chosen"] <= k and all(g > 0 for g in r["dpp_gain"][:r["dpp_chosen"]]) and all(g == 0 for g in r["dpp_gain"][r["dpp_chosen"]:])
            by = {tuple(e[0]): e for e in ranked}
            assert r["scores"] == [float(by[tuple(t)][1]) for t in toks] and r["counts"] == [int(by[tuple(t)][2]) for t in toks]
            if rerank == "mbr":
                assert r["mbr"] == [float(by[tuple(t)][3]) for t in toks]
        # the records of the whole ranked lists stay at hand: what a run without the flag returns (and writes to val_*.json)
        for full, ranked, r in zip(dec.last_ranked_records, seen["ranked"], recs):
            assert full["captions"] == [dec._text(e[0], (BOS, EOS)) for e in ranked] and full["caption"] == r["caption"]
            assert not {"dpp_gain", "dpp_chosen"} & set(full) and set(full) | {"dpp_gain", "dpp_chosen"} == set(r)
    # stochastic beam search: the aligned per-caption fields follow the selection
    p.diverse_rerank, p.temperature = "likelihood", 1.0
    gen = dec._gen()
    raw = {}
    real_sbs = gen.stochastic_beam_search

    def spy_sbs(*a, **kw):
        raw["res"] = real_sbs(*a, **kw)
        return raw["res"]
    monkeypatch.setattr(gen, "stochastic_beam_search", spy_sbs)
    recs = dec.stochastic_beam_search(None, ["a", "b", "c"], feats, None, beam_size=12)
    for r, toks, res in zip(recs, dec.last_token_ids, raw["res"]):
        own = {tuple(c[0]): c for c in res["captions"]}
        assert len(own) == 12 and len(toks) == 5 == len(r["captions"]) == len(r["dpp_gain"]) and len(set(map(tuple, toks))) == 5
        for name, col in (("logprob", 1), ("perturbed", 2), ("weight", 4), ("norm_weight", 5)):
            assert r[name] == [float(own[tuple(t)][col]) for t in toks], name
        assert r["counts"] == [1] * 5 and r["kappa"] == float(res["kappa"]) and 1 <= r["dpp_chosen"] <= 5
    # group beam search takes the selection too
    p.sample_gen, p.beam_size, p.beam_groups, p.select_n = "diverse_beam", 12, 4, 3
    recs = dec.diverse_beam_search(None, ["a", "b", "c"], feats, None)
    for r, toks in zip(recs, dec.last_token_ids):
        assert len(r["captions"]) == len(r["groups"]) == len(r["dpp_gain"]) == len(toks) <= 3 and "dpp_chosen" in r
    # without an attached CiderGram: an error, and no stale ids
    dec.mbr = None
    with pytest.raises(RuntimeError, match=r"mbr\.CiderGram"):
        dec.diverse_beam_search(None, ["a", "b", "c"], feats, None)
    assert dec.last_token_ids is None
    p.diverse_select = "none"                                                            # off: the records of a run that never knew the flag
    recs = dec.diverse_beam_search(None, ["a", "b", "c"], feats, None)
    assert all(set(r) == {"image_id", "caption", "captions", "scores", "counts", "groups"} for r in recs)
    assert dec.last_ranked_records is None


def test_gen_caption_generator_with_the_selection(lib, tmp_path, monkeypatch):
    """gen_caption.Generator.generate_caption(diverse_select="dpp"): the model and the features are handed in (the VGG16 path is
    tests/test_gpu_cli.py's), the vocabulary and the params pickle are read as the command line reads them; no training captions are at
    hand there, so the selection's in-set matrix weighs every n-gram alike"""
    import pickle
    import gen_caption
    from vae_captioning_amd import session
    rng = np.random.default_rng(21)
    words = ["w%02d" % i for i in range(25)]
    caps = {"img%d.jpg" % i: [["<BOS>"] + [words[j] for j in rng.integers(0, 25, size=6)] + ["<EOS>"] for _ in range(5)] for i in range(12)}
    with open(tmp_path / "params.pickle", "wb") as f:
        pickle.dump(dict(embed_size=32, decoder_hidden=64, encoder_hidden=64, latent_size=10, gen_z_samples=4, gen_max_len=9, keep_words=3,
                         use_c_v=False, prior="Normal", cnn_feature_size=48, diverse_method="sample", temperature=1.5, mode="inference"), f)
    with open(tmp_path / "capt_vocab.pickle", "wb") as f:
        pickle.dump(caps, f)
    (tmp_path / "pic.png").write_bytes(b"not decoded here")
    g = gen_caption.Generator(None, str(tmp_path / "params.pickle"), str(tmp_path / "capt_vocab.pickle"), gen_method="diverse")
    g.params.sample_gen = "diverse"
    g._trainer = session.get(g.params)                                                   # a seeded random model stands in for the checkpoint
    feats = np.maximum(rng.standard_normal((1, 48)), 0).astype(np.float32)
    monkeypatch.setattr(g, "_get_features", lambda path: (feats, None))
    (full,) = g.generate_caption(str(tmp_path / "pic.png"), diverse_draws=20)
    (rec,) = g.generate_caption(str(tmp_path / "pic.png"), diverse_draws=20, diverse_select="dpp", select_n=3, dpp_quality=2.0)
    assert len(full["captions"]) > 3 and "dpp_gain" not in full
    assert len(rec["captions"]) == 3 == len(rec["dpp_gain"]) == len(rec["scores"]) and 1 <= rec["dpp_chosen"] <= 3
    assert len(set(rec["captions"])) == 3 and rec["dpp_gain"][0] == np.exp(2.0) ** 2 and rec["caption"] == rec["captions"][0]
    g.gen_method = "greedy"
    with pytest.raises(ValueError, match="diverse or stochastic_beam"):
        g.generate_caption(str(tmp_path / "pic.png"))                                    # (the params still say dpp)


# ------------------------------------------------------------------ the command line
def test_main_inference_with_the_selection(tmp_path):
    _main(SMALL + ["--epochs", "1", "--max_steps", "1"], tmp_path)
    infer = SMALL + ["--mode", "inference", "--sample_gen", "diverse", "--diverse_draws", "20", "--diverse_method", "sample", "--temperature", "1.5",
                     "--eval_captions"]
    plain_out = _main(infer + ["--gen_name", "plain"], tmp_path)
    out = _main(infer + ["--gen_name", "dpp", "--diverse_select", "dpp", "--select_n", "5"], tmp_path)
    assert "dpp selection: idf over the captions of 512 training images" in out and "dpp selection" not in plain_out
    assert open(tmp_path / "val_dpp.json", "rb").read() == open(tmp_path / "val_plain.json", "rb").read()
    full, recs = json.load(open(tmp_path / "val_plain_diverse.json")), json.load(open(tmp_path / "val_dpp_diverse.json"))
    assert len(recs) == len(full) == 8 and max(len(r["captions"]) for r in full) > 5
    for r, f in zip(recs, full):
        k = r["dpp_chosen"]
        assert len(r["captions"]) == min(5, len(f["captions"])) == len(r["dpp_gain"]) and 1 <= k <= len(r["captions"])
        assert set(r["captions"]) <= set(f["captions"]) and len(set(r["captions"])) == len(r["captions"]) and r["caption"] == f["caption"]
        assert all(a >= b for a, b in zip(r["dpp_gain"][:k], r["dpp_gain"][1:k])) and all(g > 0 for g in r["dpp_gain"][:k])
        assert all(g == 0 for g in r["dpp_gain"][k:])
        assert "dpp_gain" not in f and "dpp_chosen" not in f
    m, m0 = json.load(open(tmp_path / "val_dpp_metrics.json")), json.load(open(tmp_path / "val_plain_metrics.json"))
    assert (m["diverse_select"], m["select_n"], m["dpp_quality"]) == ("dpp", 5, 1.0) and not {"diverse_select", "select_n", "dpp_quality"} & set(m0)
    assert m["captions"] == sum(len(r["captions"]) for r in recs) < m0["captions"] and m["images"] == m0["images"] == 8
    assert m["cider_d"] == m0["cider_d"] and m["bleu_4"] == m0["bleu_4"] and m["rouge_l"] == m0["rouge_l"]                # the top caption and its metrics do not move
