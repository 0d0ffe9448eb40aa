"""-m gpu: marginal decoding -- the mixture kernels (csrc/mixture.hip) against the float64 reference of tests/mixture_ref.py at the
smallest shapes that cross their boundaries (1024-column chunks, the 12288-column LDS row, unaligned pitches, one to 256 draws),
hand-made groups, independence of a group from the launch around it; CaptionGenerator.marginal_greedy / marginal_beam_search against
the reference decoders, the single-draw decoders, score(), pass cuts and graph replay; a memorised model; the command line."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import spec, synth
from vae_captioning_amd.generate import CaptionGenerator
from vae_captioning_amd.trainer import Trainer
from vae_captioning_amd.utils.parameters import Parameters

from . import mixture_ref as mr
from .test_gpu_generate import count_replays, replayed_kinds, setup

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL_LP = 1e-5                      # the project's bound on the f32 log-softmax term (tests/test_gpu_score.py)
SUMS = dict(rtol=1e-4, atol=1e-6)   # the project's bound on float64 sums of such terms
MIN_GAP = 2e-5                      # adjacent words of the reference closer than this (log units) could legitimately swap in f32
PRIORS = [dict(prior="Normal"), dict(prior="AG", use_c_v=True), dict(prior="GMM")]
IDS = lambda k: "-".join("%s=%s" % i for i in k.items())


# ------------------------------------------------------------------ the kernels
def _inputs(V, ld, K, G=None, seed=None):
    """the recipe of the kernel tests: logits N(0, 2.5^2) with 77.0 in the padding columns, logw = -12 * U[0, 1)"""
    G = G or (6 if K * V > 300000 else 24)
    rng = np.random.default_rng(V * 1000 + K if seed is None else seed)
    x = np.full((G * K, ld), 77.0, np.float32)
    x[:, :V] = rng.standard_normal((G * K, V)) * 2.5
    return x, -12.0 * rng.random(G * K)


@functools.lru_cache(maxsize=None)
def _case(V, ld, K, G=None):
    """inputs and their float64 reference (16 words), once per shape"""
    x, logw = _inputs(V, ld, K, G)
    tp, ti, stat, q = mr.mixture_topk(x, V, K, logw, min(17, V))
    for a in (x, logw, tp, ti, stat):
        a.setflags(write=False)
    return x, logw, tp, ti, stat


def _topk(lib, x, V, K, logw, kc, keep=None):
    from .gpu_util import P, dev, empty_bytes, host, stream
    G = x.shape[0] // K
    dx, dl = dev(np.array(x)), dev(np.array(logw, np.float64))   # (copies: the shared reference arrays are read-only)
    tp, ti = torch.full((G, kc), -5.0, device="cuda"), torch.full((G, kc), -7, dtype=torch.int32, device="cuda")
    stat = torch.full((G * K, 2), 9.0, device="cuda")
    need = lib.vc_mixture_topk_workspace_bytes(G, V, kc)
    assert need == G * ((V + 1023) // 1024) * kc * 8
    ws = empty_bytes(need)
    lib.vc_mixture_topk_f32(stream(), P(dx), G, K, V, x.shape[1], P(dl), kc, P(tp), P(ti), P(stat), P(ws), need)
    if keep is not None:
        keep.update(x=dx, logw=dl, stat=stat)
    return host(tp), host(ti), host(stat)


def _advance(lib, keep, V, K, parent, tok, eos=EOS, done=None, seq=None, length=None):
    """vc_mixture_advance_f32 on the logits / stat / logw that _topk left in `keep`"""
    from .gpu_util import P, dev, host, stream
    Gn = len(tok)
    i32 = np.int32
    out = torch.full((Gn * K,), 3.0, dtype=torch.float64, device="cuda")
    prow, trow = torch.full((Gn * K,), -1, dtype=torch.int32, device="cuda"), torch.full((Gn * K,), -1, dtype=torch.int32, device="cuda")
    dp = dev(np.asarray(parent, i32)) if parent is not None else None
    g = [dev(np.asarray(a, i32)) for a in (done, seq, length)] if done is not None else [None] * 3
    lib.vc_mixture_advance_f32(stream(), P(keep["x"]), V, keep["x"].shape[1], P(keep["stat"]), Gn, K, P(dp), P(dev(np.asarray(tok, i32))),
                               P(keep["logw"]), P(out), P(prow), P(trow), int(eos), P(g[0]), P(g[1]), 0 if done is None else np.shape(seq)[1], P(g[2]))
    return (host(out), host(prow), host(trow)) + (tuple(host(t) for t in g) if done is not None else ())


SHAPES = [(40, 40), (1003, 1008), (10000, 10000), (13000, 13000)]


@pytest.mark.parametrize("kc", [1, 5, 16])
@pytest.mark.parametrize("K", [1, 3, 20, 64])
@pytest.mark.parametrize("V,ld", SHAPES + [(1003, 1003)], ids=lambda v: str(v))
def test_topk_and_advance_match_float64(lib, V, ld, K, kc):
    """top_i exact (every adjacent pair among the reference's first kc + 1 words of EVERY group is >= 2e-5 apart in log units: asserted,
    no group exempt), log top_p, stat and the advanced logw within 1e-5.  13000 columns: the row is not staged in LDS; 1003 of 1008: a
    ragged last chunk and the guarded tail of the vector path; pitch 1003: the scalar path."""
    x, logw, rp, ri, rstat = _case(V, ld, K)
    G = x.shape[0] // K
    gaps = np.log(rp[:, :kc]) - np.log(rp[:, 1:kc + 1])
    print("V %d ld %d K %d kc %d G %d: smallest adjacent gap %.3e, smallest top-1 gap %.3e" % (V, ld, K, kc, G, gaps.min(), gaps[:, 0].min()))
    assert gaps.min() >= MIN_GAP
    keep = {}
    tp, ti, stat = _topk(lib, x, V, K, logw, kc, keep)
    print("  max |log top_p - log q| = %.3e, max |stat - fp64| = %.3e" % (np.abs(np.log(tp) - np.log(rp[:, :kc])).max(), np.abs(stat - rstat).max()))
    np.testing.assert_array_equal(ti, ri[:, :kc])
    np.testing.assert_allclose(np.log(tp), np.log(rp[:, :kc]), rtol=0, atol=ATOL_LP)
    np.testing.assert_allclose(stat, rstat, rtol=0, atol=ATOL_LP)
    rng = np.random.default_rng(kc)
    parent, tok = rng.integers(0, G, size=G), np.where(rng.random(G) < 0.5, ti[:, 0], rng.integers(0, V, size=G))   # the beam form
    out, prow, trow = _advance(lib, keep, V, K, parent, tok)
    want, wrow, wtok = mr.advance(x, V, K, parent, tok, logw)
    print("  max |logw_out - fp64| = %.3e" % np.abs(out - want).max())
    np.testing.assert_allclose(out, want, rtol=0, atol=ATOL_LP)
    np.testing.assert_array_equal(prow, wrow)
    np.testing.assert_array_equal(trow, wtok)


@pytest.mark.parametrize("kc", [1, 5, 16])
def test_topk_with_256_draws(lib, kc):
    x, logw, rp, ri, rstat = _case(40, 40, 256, 3)
    assert (np.log(rp[:, :kc]) - np.log(rp[:, 1:kc + 1])).min() >= MIN_GAP
    tp, ti, stat = _topk(lib, x, 40, 256, logw, kc)
    np.testing.assert_array_equal(ti, ri[:, :kc])
    np.testing.assert_allclose(np.log(tp), np.log(rp[:, :kc]), rtol=0, atol=ATOL_LP)
    np.testing.assert_allclose(stat, rstat, rtol=0, atol=ATOL_LP)


def test_topk_merges_more_than_1024_listed_words_from_memory(lib):
    """70 000 columns x kc = 16: 69 chunk lists of 16 words, more than the merge kernel stages in LDS"""
    V, K, kc = 70000, 2, 16
    x, logw, rp, ri, rstat = _case(V, V, K, 2)
    assert ((V + 1023) // 1024) * kc > 1024 and (np.log(rp[:, :kc]) - np.log(rp[:, 1:kc + 1])).min() >= MIN_GAP
    tp, ti, stat = _topk(lib, x, V, K, logw, kc)
    np.testing.assert_array_equal(ti, ri[:, :kc])
    np.testing.assert_allclose(np.log(tp), np.log(rp[:, :kc]), rtol=0, atol=ATOL_LP)
    np.testing.assert_allclose(stat, rstat, rtol=0, atol=ATOL_LP)


def test_equal_columns_a_constant_row_and_a_dominant_draw(lib):
    rng = np.random.default_rng(77)
    V, ld, K = 2100, 2100, 3
    x = np.full((3 * K, ld), 0.0, np.float32)
    x[:, :V] = rng.standard_normal((3 * K, V)) * 2.5
    x[0:K, 1500] = x[0:K, 7] = 11.0            # group 0: two columns equal in all K rows, in different chunks: the lower index first
    x[K + 1, :] = -3.25                         # group 1: a constant row (uniform under that draw)
    logw = np.zeros(3 * K)
    logw[2 * K:] = [-2000.0, -1.0, -2001.0]     # group 2: a spread of 2000: only draw 1 counts
    tp, ti, stat = _topk(lib, x, V, K, logw, 4)
    rp, ri, rstat, _ = mr.mixture_topk(x, V, K, logw, 4)
    assert ti[0, :2].tolist() == [7, 1500] and tp[0, 0] == tp[0, 1]
    np.testing.assert_array_equal(ti, ri)
    np.testing.assert_allclose(np.log(tp), np.log(rp), rtol=0, atol=ATOL_LP)
    assert stat[K + 1, 0] == -3.25 and abs(stat[K + 1, 1] - np.log(V)) <= 1e-6   # (S = V exactly: a sum of ones)
    row = x[2 * K + 1, :V].astype(np.float64)
    assert ti[2].tolist() == np.argsort(-row, kind="stable")[:4].tolist()
    np.testing.assert_allclose(np.log(tp[2]), (row - row.max() - np.log(np.exp(row - row.max()).sum()))[ti[2]], rtol=0, atol=ATOL_LP)


def test_greedy_form_of_advance(lib):
    """a live group appends and advances; an <EOS> ends its group; a done group changes nothing (logw copied through); a full seq row
    takes nothing more"""
    V, K, Lmax = 50, 3, 3
    x, logw = _inputs(V, V, K, G=4, seed=5)
    keep = {}
    _topk(lib, x, V, K, logw, 1, keep)
    done, seq, ln = [0, 0, 1, 0], [[5, 0, 0], [6, 7, 0], [8, EOS, 0], [9, 9, 9]], [1, 2, 2, 3]
    tok = [11, EOS, 13, 14]
    out, prow, trow, d2, s2, l2 = _advance(lib, keep, V, K, None, tok, EOS, done, seq, ln)
    want, _, wtok, wd, ws_, wl = mr.advance(x, V, K, None, tok, logw, EOS, done, seq, ln)
    assert d2.tolist() == wd.tolist() == [0, 1, 1, 0] and l2.tolist() == wl.tolist() == [2, 3, 2, 3]
    assert s2.tolist() == ws_.tolist() == [[5, 11, 0], [6, 7, EOS], [8, EOS, 0], [9, 9, 9]]
    np.testing.assert_allclose(out, want, rtol=0, atol=ATOL_LP)
    np.testing.assert_array_equal(out[2 * K:], logw[2 * K:])     # bit for bit
    assert prow.tolist() == list(range(4 * K))
    np.testing.assert_array_equal(trow, wtok)


@pytest.mark.parametrize("V,ld,K,kc", [(10000, 10000, 20, 5), (1003, 1008, 3, 16), (1003, 1003, 3, 1), (13000, 13000, 2, 16)], ids=str)
def test_a_group_does_not_depend_on_the_launch_around_it(lib, V, ld, K, kc):
    """one group alone (G = 1) and as group 5 of 7: top_p, top_i, stat and the advanced logw bit-identical; so are two calls"""
    x, logw = _inputs(V, ld, K, G=7, seed=V + K)
    sl = slice(5 * K, 6 * K)
    k7, k1 = {}, {}
    a7 = _topk(lib, x, V, K, logw, kc, k7)
    a1 = _topk(lib, np.ascontiguousarray(x[sl]), V, K, logw[sl], kc, k1)
    again = _topk(lib, x, V, K, logw, kc)
    for got7, got1, rep in zip(a7, a1, again):
        np.testing.assert_array_equal(got7.reshape(7, -1)[5], got1.reshape(-1))
        np.testing.assert_array_equal(got7, rep)
    tok = a7[1][:, 0]
    o7, o1 = _advance(lib, k7, V, K, None, tok), _advance(lib, k1, V, K, None, tok[5:6])
    np.testing.assert_array_equal(o7[0][sl], o1[0])
    np.testing.assert_array_equal(o7[0], _advance(lib, k7, V, K, None, tok)[0])


def test_rows_of_dead_beams_cannot_steer_an_index(lib):
    """a group whose rows and weights hold NaN and infinities gets indices in [0, V); its neighbours' results do not move by a bit"""
    V, ld, K, kc = 2500, 2500, 4, 5
    x, logw = _inputs(V, ld, K, G=4, seed=3)
    clean = _topk(lib, x, V, K, logw, kc)
    x, logw = x.copy(), logw.copy()
    x[K:2 * K, 0::3], x[K:2 * K, 1::3], x[K + 1, :] = np.nan, np.inf, -np.inf
    logw[K:2 * K] = [np.nan, np.inf, -np.inf, 1e300]
    tp, ti, stat = _topk(lib, x, V, K, logw, kc)
    assert ((ti >= 0) & (ti < V)).all()
    for got, want in zip((tp, ti, stat), clean):
        np.testing.assert_array_equal(np.delete(got.reshape(4, -1), 1, 0), np.delete(want.reshape(4, -1), 1, 0))


# ------------------------------------------------------------------ the decoders
def _draws(p, K, B, seed=4):
    return np.random.default_rng(seed).standard_normal((K, p.gen_z_samples, B, p.latent_size)).astype(np.float32)


def _ref_args(P64, p, feats, cv, eps, b):
    return P64, p, feats[b].astype(np.float64), cv[b].astype(np.float64), eps[:, :, b:b + 1].astype(np.float64)


GREEDY_SEED, BEAM_SEED = 31, 31   # (chosen on the CPU: the reference's gaps below hold for the three priors)


@pytest.mark.parametrize("kw", PRIORS, ids=IDS)
def test_marginal_greedy_matches_the_reference(lib, kw):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, GREEDY_SEED, **kw)
    B, K, T = feats.shape[0], 5, 12
    eps = _draws(p, K, B)
    got = gen.marginal_greedy(feats, cv if spec.uses_ci(p) else None, eps, BOS, EOS, draws=K, max_len=T)
    for b in range(B):
        toks, logw, marg, gap = mr.marginal_greedy(*_ref_args(P64, p, feats, cv, eps, b), BOS, EOS, c_means=cm, max_len=T)
        print("image %d: %d tokens, marginal %.6f (fp64 %.6f), smallest top-1 gap %.3e" % (b, len(toks), got[b]["marginal"], marg, gap))
        assert gap >= 1e-4
        assert got[b]["tokens"] == toks
        np.testing.assert_allclose(got[b]["logprob"], logw, **SUMS)
        np.testing.assert_allclose(got[b]["marginal"], marg, **SUMS)


@pytest.mark.parametrize("kw", PRIORS, ids=IDS)
def test_marginal_beam_search_matches_the_reference(lib, kw):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, BEAM_SEED, **kw)
    B, K, T = feats.shape[0], 5, 12
    eps = _draws(p, K, B)
    got = gen.marginal_beam_search(feats, cv if spec.uses_ci(p) else None, eps, BOS, EOS, draws=K, beam_size=3, max_len=T)
    for b in range(B):
        sents, scores, gap = mr.marginal_beam_search(*_ref_args(P64, p, feats, cv, eps, b), BOS, EOS, c_means=cm, beam_size=3, max_len=T)
        print("image %d: %d beams, best %.6f (fp64 %.6f), smallest gap among the first 4 words %.3e" % (b, len(sents), got[b][0][1], scores[0], gap))
        assert gap >= 1e-4
        assert [s for s, _ in got[b]] == sents
        np.testing.assert_allclose([sc for _, sc in got[b]], scores, **SUMS)


@pytest.mark.parametrize("kw", PRIORS + [dict(no_encoder=True)], ids=IDS)
def test_one_draw_is_the_single_draw_decoders(lib, kw):
    p, eng, gen, P64, feats, cv, eps, cm = setup(lib, 7, **kw)
    c, T, K = (cv if spec.uses_ci(p) else None), 10, 4
    greedy, beams = gen.greedy(feats, c, eps, BOS, EOS, max_len=T), gen.beam_search(feats, c, eps, BOS, EOS, beam_size=3, max_len=T)
    for e in (eps[None], np.repeat(eps[None], K, axis=0)):   # one draw; the same draw K times
        k = e.shape[0]
        mg = gen.marginal_greedy(feats, c, e, BOS, EOS, draws=k, max_len=T)
        assert [r["tokens"] for r in mg] == greedy
        for r in mg:
            np.testing.assert_allclose(r["logprob"], r["marginal"], rtol=0, atol=1e-9)
        mb = gen.marginal_beam_search(feats, c, e, BOS, EOS, draws=k, beam_size=3, max_len=T)
        for b in range(feats.shape[0]):
            assert [s for s, _ in mb[b]] == [s for s, _ in beams[b]]
            np.testing.assert_allclose([sc for _, sc in mb[b]], [sc for _, sc in beams[b]], **SUMS)


@pytest.mark.parametrize("kw", PRIORS, ids=IDS)
def test_marginal_greedy_agrees_with_score(lib, kw):
    """the accumulated marginal and per-draw log-likelihoods are score()'s of the returned caption under the same eps"""
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, GREEDY_SEED, **kw)
    B, K = feats.shape[0], 5
    eps, c = _draws(p, K, B), (cv if spec.uses_ci(p) else None)
    got = gen.marginal_greedy(feats, c, eps, BOS, EOS, draws=K, max_len=12)
    sc = gen.score(feats, [[r["tokens"]] for r in got], c, eps, BOS, EOS, draws=K)
    for b in range(B):
        assert sc[b][0]["tokens"] == len(got[b]["tokens"])
        np.testing.assert_allclose(got[b]["logprob"], sc[b][0]["logprob"], **SUMS)
        np.testing.assert_allclose(got[b]["marginal"], sc[b][0]["marginal"], **SUMS)


def _same(a, b, **tol):
    """two results of marginal_greedy or marginal_beam_search: the same tokens; the same numbers, bit for bit unless a tolerance is given"""
    close = (lambda x, y: np.testing.assert_allclose(x, y, **tol)) if tol else np.testing.assert_array_equal
    if isinstance(a[0], dict):
        assert [r["tokens"] for r in a] == [r["tokens"] for r in b]
        close([r["marginal"] for r in a], [r["marginal"] for r in b])
        close(np.stack([r["logprob"] for r in a]), np.stack([r["logprob"] for r in b]))
    else:
        assert [[s for s, _ in beams] for beams in a] == [[s for s, _ in beams] for beams in b]
        close([sc for beams in a for _, sc in beams], [sc for beams in b for _, sc in beams])


@pytest.mark.parametrize("cap", [5, 12, 20], ids=["an-image-per-pass", "two-images", "ragged-last-pass"])
def test_pass_cuts_do_not_change_the_results(lib, cap, monkeypatch):
    """the same tokens and sentences however the images are cut into passes; the numbers within the project's bound on such sums (the
    last bits of the f32 logits depend on how many rows a product has: tests/test_gpu_decode_step.py measures it for diverse())"""
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 13, prior="AG", use_c_v=True)
    B, K = feats.shape[0], 5
    eps = _draws(p, K, B)
    whole = gen.marginal_greedy(feats, cv, eps, BOS, EOS, draws=K, max_len=10), gen.marginal_beam_search(feats, cv, eps, BOS, EOS, draws=K, beam_size=2, max_len=10)
    monkeypatch.setattr(gen, "diverse_rows", cap)   # 5: an image exceeds the cap alone in the beam search (10 rows): a pass of its own
    assert len(gen._marginal_passes(B, K)) == -(-B // max(1, cap // K)) > 1
    _same(gen.marginal_greedy(feats, cv, eps, BOS, EOS, draws=K, max_len=10), whole[0], **SUMS)
    _same(gen.marginal_beam_search(feats, cv, eps, BOS, EOS, draws=K, beam_size=2, max_len=10), whole[1], **SUMS)


def test_second_call_replays_captured_chunks_and_decodes_its_own_inputs(lib, monkeypatch):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 13, prior="GMM")
    B, K, T = feats.shape[0], 5, 10
    eps, eps2 = _draws(p, K, B), _draws(p, K, B, seed=99)
    feats2 = np.ascontiguousarray(feats[::-1])
    replayed = count_replays(monkeypatch)
    first = gen.marginal_greedy(feats, None, eps, BOS, EOS, draws=K, max_len=T), gen.marginal_beam_search(feats, None, eps, BOS, EOS, draws=K, beam_size=2, max_len=T)
    graphs = dict(gen._graphs)
    assert sorted(k[0] for k in graphs) == ["dvinit", "marginal_beam", "marginal_greedy"]
    replayed.clear()
    second = gen.marginal_greedy(feats2, None, eps2, BOS, EOS, draws=K, max_len=T), gen.marginal_beam_search(feats2, None, eps2, BOS, EOS, draws=K, beam_size=2, max_len=T)
    kinds = replayed_kinds(gen, replayed)
    print("replayed on the second call:", kinds)
    assert gen._graphs == graphs, "a second call of the same shapes captures nothing new"
    assert kinds.count("dvinit") == 2 and kinds.count("marginal_greedy") >= 1 and kinds.count("marginal_beam") >= 1
    monkeypatch.setenv("VC_DECODE_GRAPH", "0")
    replayed.clear()
    g = CaptionGenerator(eng)
    for (f, e), (mg, mb) in (((feats, eps), first), ((feats2, eps2), second)):   # the eager loop: same results, both inputs
        _same(g.marginal_greedy(f, None, e, BOS, EOS, draws=K, max_len=T), mg)
        _same(g.marginal_beam_search(f, None, e, BOS, EOS, draws=K, beam_size=2, max_len=T), mb)
    assert replayed == [] and len(g._graphs) == 0
    assert [r["tokens"] for r in first[0]] != [r["tokens"] for r in second[0]]   # (the two inputs do decode differently)


def test_a_memorised_model_returns_its_sixteen_captions(lib):
    """the memorisation recipe of tests/test_gpu_score.py's retrieval test (sixteen captions, 150 Adam steps at 4e-3, seeds 42 / 5 / 3)"""
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden = 64, 128, 128
    p.latent_size, p.gen_z_samples, p.cnn_feature_size = 20, 6, 96
    p.num_captions, p.batch_size, p.learning_rate, p.prior = 1, 16, 4e-3, "Normal"
    V, B, T, STEPS = 200, 16, 9, 150
    batch = synth.make_batch(np.random.default_rng(42), B, 1, T, V, variable_len=True, feature_size=p.cnn_feature_size)
    tr = Trainer(p, V, lib=lib, seed=5)
    tr.load_state_dict(spec.init_caption_params(p, V, seed=3))
    tr.set_batch(batch)
    for _ in range(STEPS):
        tr.train_step()
    assert tr.losses()[1] < 0.1
    caps = [batch["cap_enc"][b, :int(batch["lengths"][b])].tolist() for b in range(B)]
    got = CaptionGenerator(tr.cap).marginal_greedy(batch["features"], None, None, synth.BOS, synth.EOS, draws=8, max_len=T + 2)
    assert [r["tokens"] for r in got] == caps
    assert all(-2.0 < r["marginal"] <= 0.0 for r in got)


def test_main_cli_marginal_greedy(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--synthetic", "--vocab", "200", "--embed_dim", "32", "--enc_hid", "64", "--dec_hid", "64", "--latent", "10",
              "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "mx", "--seed", "11"]
    run = lambda extra: subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + common + extra,
                                       cwd=tmp_path, env=env, capture_output=True, text=True)
    r = run(["--epochs", "1", "--max_steps", "1"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = []
    for name in ("m1", "m2"):
        r = run(["--mode", "inference", "--sample_gen", "marginal_greedy", "--marginal_draws", "4", "--gen_name", name])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        recs.append(json.load(open(tmp_path / ("val_%s.json" % name))))
    assert len(recs[0]) == 8 and all(set(x) == {"image_id", "caption", "marginal", "draws"} for x in recs[0])
    assert all(x["draws"] == 4 and np.isfinite(x["marginal"]) and x["marginal"] < 0 for x in recs[0])
    assert recs[0] == recs[1]
