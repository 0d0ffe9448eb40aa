"""-m gpu: decoding controls -- vc_decode_controls_f32 (csrc/decode_controls.hip) against tests/controls_ref.py: process_row in float32,
bit for bit over the whole [rows, ld] array, and the `controls` keyword of CaptionGenerator's decoders against the float64 searches of
the same file on the cases tests/test_controls_host.py has shown to be safe; then what the keyword promises: no banned word, no
repeated n-gram, no early <EOS> in sampled captions, log-likelihoods under the processed distribution, the paths of today when the
controls are off, graph replay, a new banned list through a captured graph, the refusals, and the command line."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import abi, spec
from vae_captioning_amd.controls import DecodeControls
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.generate import CaptionGenerator

from . import controls_ref as ref
from .gpu_util import P, dev, host, stream

pytestmark = pytest.mark.gpu
BOS, EOS = ref.BOS, ref.EOS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL_LP = 1e-5          # per token: what tests/test_gpu_score.py holds a log-softmax term to
FLT_MAX = np.finfo(np.float32).max


# ------------------------------------------------------------------ the kernel
class Ctl(object):
    """what process_row reads of a DecodeControls, without its call-level limits (the kernel takes any table)"""
    def __init__(self, n, m, theta, banned):
        self.no_repeat_ngram, self.min_len, self.repetition_penalty, self.banned = n, m, theta, banned


def _table(rng, V, n_banned, flip):
    if n_banned == 0:
        return np.zeros(0, np.int32)
    if n_banned == 1:
        return np.array([V - 1 if flip else 0], np.int32)
    if V <= n_banned:   # (ids beyond the vocabulary are ignored)
        return np.arange(n_banned, dtype=np.int32)
    mid = rng.choice(np.arange(1, V - 1), n_banned - 2, replace=False)
    return np.sort(np.concatenate([[0, V - 1], mid])).astype(np.int32)


def _problem(rng, rows, V, ld, Lmax, skip, n, m):
    """logits [rows, ld] (positive, negative and exactly 0 at history words; the padding columns hold 7), histories [rows, Lmax + 3]
    from a 4-word alphabet with the ids -7 and V sprinkled in, lengths over 0, n-1, n, Lmax, -3, Lmax + 5, m-1, m, and done flags"""
    hist_ld = Lmax + 3
    alphabet = np.array([0, V - 1, rng.integers(0, V), rng.integers(0, V)])
    x = rng.standard_normal((rows, ld)).astype(np.float32) * 3
    x[:, V:] = 7.0
    hist = alphabet[rng.integers(0, 4, size=(rows, hist_ld))].astype(np.int32)
    wild = rng.random((rows, hist_ld)) < 0.08
    hist[wild] = np.where(rng.random(int(wild.sum())) < 0.5, -7, V)
    cycle = [skip, skip + n - 1, skip + n, Lmax, -3, Lmax + 5, skip + m - 1, skip + m, skip + 2 * n]
    lens = np.array([cycle[r % len(cycle)] if r < 2 * len(cycle) else rng.integers(0, Lmax + 1) for r in range(rows)], np.int32)
    for r in range(0, rows, 3):
        x[r, alphabet[r % 4]] = 0.0
    done = np.array([1 if (r % 7 == 5) else 0 for r in range(rows)], np.int32)
    return x, hist, hist_ld, lens, done


def _expected(x, V, hist, Lmax, skip, lens, done, ctl, eos):
    out = x.copy()
    for r in range(x.shape[0]):
        if done is not None and done[r]:
            continue
        W = min(max(int(lens[r]), skip), Lmax) - skip
        out[r, :V] = ref.process_row(x[r, :V], hist[r, skip:skip + W], ctl, eos)
    return out


def _launch(lib, x, V, hist, hist_ld, Lmax, skip, lens, done, ctl, eos, rows=None):
    dx, dh, dl = dev(x), dev(hist), dev(lens)
    dd = dev(done) if done is not None else None
    tab = dev(ctl.banned) if len(ctl.banned) else None
    lib.vc_decode_controls_f32(stream(), P(dx), x.shape[0] if rows is None else rows, V, x.shape[1], P(dh), hist_ld, Lmax, skip, P(dl), P(dd),
                               ctl.no_repeat_ngram, ctl.min_len, eos, ctl.repetition_penalty, P(tab), len(ctl.banned))
    return host(dx)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# every n with each penalty and each table size at least once (and the pairs that interact: a long table with a penalty, n = 8 with both)
COMBOS = [(0, 0, 1.0, 0), (0, 3, 1.3, 1), (1, 0, 1.0, 256), (1, 3, 1.3, 0), (2, 3, 1.0, 1), (2, 0, 1.3, 256), (3, 3, 1.3, 1), (3, 0, 1.0, 0),
          (4, 3, 1.0, 256), (4, 0, 1.3, 0), (8, 3, 1.3, 256), (8, 0, 1.0, 1)]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("Lmax", [1, 8, 32, 70])
@pytest.mark.parametrize("V,ld", [(7, 7), (40, 40), (1001, 1008), (10000, 10000)])
def test_kernel_is_process_row_bit_for_bit(lib, V, ld, Lmax, skip):
    rng = np.random.default_rng(V * 1000 + Lmax * 10 + skip)
    eos = 2
    for j, (n, m, theta, nb) in enumerate(COMBOS):
        for rows in (1, 5, 67):
            ctl = Ctl(n, m, theta, _table(rng, V, nb, j & 1))
            x, hist, hist_ld, lens, done = _problem(rng, rows, V, ld, Lmax, skip, n, m)
            use_done = done if (j + rows) % 4 else None
            got = _launch(lib, x, V, hist, hist_ld, Lmax, skip, lens, use_done, ctl, eos)
            want = _expected(x, V, hist, Lmax, skip, lens, use_done, ctl, eos)
            assert _same_bits(got, want), (n, m, theta, nb, rows, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])
            assert np.isfinite(got).all()   # banned is -FLT_MAX, never -inf


def test_kernel_resolves_penalised_and_banned_and_counts_overlaps(lib):
    """the cases of the definition, by hand: a a a with n = 2 bans a; a word penalised and banned is banned; the penalty acts once on a
    word emitted three times; W = m - 1 bans <EOS>, W = m frees it"""
    V, Lmax = 9, 6
    x = np.array([[2.0, -2.0, 0.0, 4.0, -4.0, 1.0, 8.0, -8.0, 0.5]] * 4, np.float32)
    hist = np.array([[3, 3, 3, 0, 0, 0], [3, 3, 3, 0, 0, 0], [4, 6, 4, 0, 0, 0], [4, 6, 4, 0, 0, 0]], np.int32)
    lens = np.array([3, 3, 2, 3], np.int32)
    ctl = Ctl(2, 3, 2.0, np.array([6], np.int32))
    got = _launch(lib, x, V, hist, Lmax, Lmax, 0, lens, None, ctl, 5)
    want = x.copy()
    want[:2, 3] = -FLT_MAX                 # a a a: the bigram (a, a) ends the history, a follows it at p = 1 and p = 2
    want[:, 6] = -FLT_MAX                  # the table, also where 6 is a penalised history word
    want[2, 4], want[3, 4] = -8.0, -8.0    # penalised once
    want[2, 5] = -FLT_MAX                  # W = 2 < 3
    assert _same_bits(got, want), (got, want)
    assert _same_bits(got, _expected(x, V, hist, Lmax, 0, lens, None, ctl, 5))


def test_a_row_alone_is_the_row_in_the_batch(lib):
    rng = np.random.default_rng(3)
    V, ld, Lmax, skip, eos = 1001, 1008, 32, 1, 2
    ctl = Ctl(2, 4, 1.3, _table(rng, V, 256, 0))
    x, hist, hist_ld, lens, done = _problem(rng, 67, V, ld, Lmax, skip, 2, 4)
    batch = _launch(lib, x, V, hist, hist_ld, Lmax, skip, lens, done, ctl, eos)
    for r in (0, 1, 2, 6, 33, 63, 64, 66):
        alone = _launch(lib, x[r:r + 1], V, hist[r:r + 1], hist_ld, Lmax, skip, lens[r:r + 1], done[r:r + 1], ctl, eos)
        assert _same_bits(alone[0], batch[r]), r
    again = _launch(lib, x, V, hist, hist_ld, Lmax, skip, lens, done, ctl, eos)
    assert _same_bits(again, batch)


def test_all_off_changes_nothing_and_no_rows_launch_nothing(lib):
    rng = np.random.default_rng(4)
    x, hist, hist_ld, lens, done = _problem(rng, 67, 40, 44, 8, 0, 0, 0)
    x[0, :4] = [-0.0, np.inf, -np.inf, np.nan]
    off = Ctl(0, 0, 1.0, np.zeros(0, np.int32))
    assert _same_bits(_launch(lib, x, 40, hist, hist_ld, 8, 0, lens, done, off, EOS), x)
    assert _same_bits(_launch(lib, x, 40, hist, hist_ld, 8, 0, lens, None, off, EOS), x)
    assert _same_bits(_launch(lib, x, 40, hist, hist_ld, 8, 0, lens, None, Ctl(2, 3, 1.3, np.array([4], np.int32)), EOS, rows=0), x)
    lib.vc_decode_controls_f32(stream(), None, 0, 40, 40, None, 8, 8, 0, None, None, 2, 3, EOS, 1.3, None, 0)


def test_argument_errors_launch_nothing(lib):
    rng = np.random.default_rng(5)
    x, hist, hist_ld, lens, done = _problem(rng, 5, 40, 40, 8, 0, 2, 3)
    dx, dh, dl, tab = dev(x), dev(hist), dev(lens), dev(np.array([4, 9], np.int32))
    ok = dict(logits=P(dx), rows=5, V=40, ld=40, hist=P(dh), hist_ld=hist_ld, Lmax=8, skip=0, len=P(dl), ngram=2, min_len=3, eos=EOS, penalty=1.3,
              banned=P(tab), n_banned=2)

    def call(**kw):
        a = dict(ok, **kw)
        lib.vc_decode_controls_f32(stream(), a["logits"], a["rows"], a["V"], a["ld"], a["hist"], a["hist_ld"], a["Lmax"], a["skip"], a["len"], None,
                                   a["ngram"], a["min_len"], a["eos"], a["penalty"], a["banned"], a["n_banned"])

    for kw, word in ((dict(ngram=-1), "ngram"), (dict(ngram=9), "ngram"), (dict(penalty=0.5), "penalty"), (dict(penalty=float("inf")), "penalty"),
                     (dict(penalty=float("nan")), "penalty"), (dict(n_banned=-1), "n_banned"), (dict(n_banned=257), "n_banned"),
                     (dict(banned=None), "n_banned"), (dict(eos=-1), "eos"), (dict(eos=40), "eos"), (dict(ld=39), "bad shape"), (dict(V=0), "bad shape"),
                     (dict(rows=-1), "bad shape"), (dict(min_len=-1), "min_len"), (dict(Lmax=0), "history"), (dict(hist_ld=7), "history"),
                     (dict(skip=-1), "history"), (dict(skip=9), "history"), (dict(logits=None), "null pointer"), (dict(hist=None), "null pointer"),
                     (dict(len=None), "null pointer")):
        with pytest.raises(abi.VaecapError, match=word):
            call(**kw)
    assert _same_bits(host(dx), x)
    call()
    assert not _same_bits(host(dx), x)


# ------------------------------------------------------------------ the decoders against the float64 searches
CASE_GRID = [(k, mode, name) for k in range(len(ref.CASES)) for mode in ref.MODES for name in ref.SETTINGS]
GRID_IDS = ["%s-%s-%s" % (ref.CASE_IDS[k], mode, name) for k, mode, name in CASE_GRID]


@functools.lru_cache(maxsize=None)
def engine(k):
    """one engine per prior case: every case of it decodes six images of the same model (controls_ref.pool)"""
    p, P0 = ref.pool(k)[:2]
    eng = CaptionEngine(p, 40, lib=abi.load())
    eng.load_params(P0)
    return eng


def case(k, mode, name):
    """(a fresh generator, features, cluster vectors or None, eps, constraint lists) of an end-to-end case"""
    feats, cv, eps, cons = ref.case_inputs(k, mode, name)
    eng = engine(k)
    return CaptionGenerator(eng), feats, (cv if spec.uses_ci(eng.p) else None), eps, [[[int(v) for v in st] for st in ci] for ci in cons]


def decode(gen, mode, feats, cv, eps, cons, controls="absent", **kw):
    kw = dict(kw) if isinstance(controls, str) else dict(kw, controls=controls)
    if mode == "greedy":
        return gen.greedy(feats, cv, eps, BOS, EOS, max_len=ref.MAX_LEN, **kw)
    if mode == "beam_search":
        return gen.beam_search(feats, cv, eps, BOS, EOS, beam_size=3, max_len=ref.MAX_LEN, **kw)
    if mode == "diverse_beam_search":
        return gen.diverse_beam_search(feats, cv, eps, BOS, EOS, groups=2, group_size=2, diversity=0.5, max_len=ref.MAX_LEN, **kw)
    return gen.constrained_beam_search(feats, cons, cv, eps, BOS, EOS, beam_size=3, max_len=ref.MAX_LEN, all_states=True, **kw)


def flatten(mode, res):
    """(per image its token sequences, every score in order) of a decoder's or the reference's result"""
    if mode == "greedy":
        return [list(r[0]) if isinstance(r, tuple) else list(r) for r in res], []
    if mode == "beam_search":
        if isinstance(res[0], tuple):   # the reference: (sentences, scores)
            return [r[0] for r in res], [sc for r in res for sc in r[1]]
        return [[s for s, _ in r] for r in res], [sc for r in res for _, sc in r]
    if isinstance(res[0][0], tuple):    # the reference: per bank (sentences, scores)
        return [[bank[0] for bank in r] for r in res], [sc for r in res for bank in r for sc in bank[1]]
    return [[[s for s, _ in bank] for bank in r] for r in res], [sc for r in res for bank in r for _, sc in bank]


def captions(mode, res):
    """every token sequence of a decoder's result"""
    seqs = flatten(mode, res)[0]
    if mode == "greedy":
        return seqs
    return [s for im in seqs for x in im for s in ([x] if mode == "beam_search" else x)]


@pytest.mark.parametrize("k,mode,name", CASE_GRID, ids=GRID_IDS)
def test_decoders_match_the_float64_reference(lib, k, mode, name):
    """each control alone and all together, the four prior cases, V = 40, B = 6, max_len 10: token sequences identical, scores within
    rtol 1e-4, atol 1e-5 (the cases are safe: tests/test_controls_host.py)"""
    gen, feats, cv, eps, cons = case(k, mode, name)
    want, _ = ref.run_case(k, mode, name)
    got = decode(gen, mode, feats, cv, eps, cons, ref.settings()[name])
    gs, gsc = flatten(mode, got)
    ws, wsc = flatten(mode, want)
    for b in range(6):
        assert gs[b] == ws[b], (b, gs[b], ws[b])
    np.testing.assert_allclose(gsc, wsc, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("temperature", [0.7, 1.5])
@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.CASE_IDS)
def test_sampled_captions_keep_the_promises(lib, k, temperature):
    """diverse(method="sample") and sample() with injected uniforms, untruncated and with top_k = 38 >= the 34 unbanned words: no
    caption holds a banned id, a repeated bigram or an <EOS> before five words, and a candidate's logprob is the float64 log-softmax of
    the PROCESSED logits along its tokens"""
    gen, feats, cv, eps1, _ = case(k, "greedy", "all")
    p, P0, _, _, _, cm, _ = ref.pool(k)
    cv_all = ref.case_inputs(k, "greedy", "all")[1]
    P64 = {kk: v.astype(np.float64) for kk, v in P0.items()}
    ctl = ref.settings()["all"]
    B, K, T = 6, 3, ref.MAX_LEN
    rng = np.random.default_rng(100 + k)
    eps = rng.standard_normal((K, p.gen_z_samples, B, p.latent_size)).astype(np.float32)
    u = rng.random((K, T, B)).astype(np.float32)
    before = gen.p.temperature
    gen.p.temperature = temperature
    try:
        for top_k in (0, 38):
            gen.diverse(feats, cv, eps, BOS, EOS, draws=K, method="sample", max_len=T, uniforms=u, top_k=top_k, controls=ctl)
            for b in range(B):
                for kk in range(K):
                    toks, lp, ended = gen.last_candidates[b][kk]
                    assert ref.properties(toks, ctl, EOS) == (True, True, True), (b, kk, toks)
                    assert len(toks) == T or (ended and len(toks) >= ctl.min_len + 1)
                    terms = ref.sequence_logprob(P64, p, feats[b].astype(np.float64), cv_all[b].astype(np.float64),
                                                 eps[kk][:, b:b + 1].astype(np.float64), BOS, EOS, ctl, toks, c_means=cm)
                    print("logprob %.9g reference %.9g" % (lp, sum(terms)))
                    assert abs(lp - sum(terms)) <= ATOL_LP * len(toks), (b, kk, lp, sum(terms))
            caps = gen.sample(feats, cv, eps1, BOS, EOS, max_len=T, uniforms=u[0], top_k=top_k, controls=ctl)
            assert len(caps) == B
            for toks in caps:
                assert ref.properties(toks, ctl, EOS) == (True, True, True), toks
                assert len(toks) == T or (toks[-1] == EOS and len(toks) >= ctl.min_len + 1)
    finally:
        gen.p.temperature = before


def test_diverse_greedy_is_greedy_per_draw(lib):
    """diverse(method="greedy") under controls: every draw is greedy() under the same controls with that draw's eps"""
    gen, feats, cv, eps1, _ = case(1, "greedy", "all")
    ctl = ref.settings()["all"]
    eps = np.stack([eps1, eps1[::-1].copy()])
    gen.diverse(feats, cv, eps, BOS, EOS, draws=2, max_len=ref.MAX_LEN, controls=ctl)
    cands = gen.last_candidates
    want = ref.run_case(1, "greedy", "all")[0]
    other = gen.greedy(feats, cv, eps[1], BOS, EOS, max_len=ref.MAX_LEN, controls=ctl)
    for b in range(6):
        assert cands[b][0][0] == want[b][0]
        assert abs(cands[b][0][1] - want[b][1]) <= ATOL_LP * len(want[b][0])
        assert cands[b][1][0] == other[b]


# ------------------------------------------------------------------ what the keyword leaves alone
@pytest.mark.parametrize("mode", ref.MODES)
def test_none_and_noop_take_todays_path(lib, mode):
    """no keyword, controls=None and DecodeControls() return equal results through the same graphs (no key is added); after a call with
    active controls the same call without them returns what it returned before"""
    gen, *inp = case(3, mode, "all")
    first = decode(gen, mode, *inp)
    again = decode(gen, mode, *inp)      # (a beam search captures its chunks at the end of its first call)
    keys = set(gen._graphs)
    assert again == first and keys
    assert decode(gen, mode, *inp, None) == first
    assert decode(gen, mode, *inp, DecodeControls()) == first
    assert set(gen._graphs) == keys
    on = decode(gen, mode, *inp, ref.settings()["all"])
    assert on != first
    assert decode(gen, mode, *inp) == first and keys <= set(gen._graphs)


def test_sampling_without_controls_is_unchanged(lib):
    gen, feats, cv, eps, _ = case(1, "greedy", "all")
    u = np.random.default_rng(2).random((ref.MAX_LEN, 6)).astype(np.float32)
    first = gen.sample(feats, cv, eps, BOS, EOS, max_len=ref.MAX_LEN, uniforms=u)
    assert gen.sample(feats, cv, eps, BOS, EOS, max_len=ref.MAX_LEN, uniforms=u, controls=DecodeControls()) == first
    assert gen.sample(feats, cv, eps, BOS, EOS, max_len=ref.MAX_LEN, uniforms=u, controls=ref.settings()["all"]) != first
    assert gen.sample(feats, cv, eps, BOS, EOS, max_len=ref.MAX_LEN, uniforms=u, controls=None) == first
    first = gen.diverse(feats, cv, None, BOS, EOS, draws=2, max_len=ref.MAX_LEN)
    keys = set(gen._graphs)
    assert gen.diverse(feats, cv, None, BOS, EOS, draws=2, max_len=ref.MAX_LEN, controls=DecodeControls()) == first
    assert gen.diverse(feats, cv, None, BOS, EOS, draws=2, max_len=ref.MAX_LEN, controls=None) == first and set(gen._graphs) == keys


@pytest.mark.parametrize("mode", ref.MODES + ("diverse",))
def test_graph_replay_is_the_eager_loop(lib, mode, monkeypatch):
    gen, feats, cv, eps, cons = case(3, mode if mode != "diverse" else "greedy", "all")
    ctl = ref.settings()["all"]

    def run(g):
        if mode != "diverse":
            return decode(g, mode, feats, cv, eps, cons, ctl)
        res = g.diverse(feats, cv, np.stack([eps, eps[::-1].copy()]), BOS, EOS, draws=2, max_len=ref.MAX_LEN, controls=ctl)
        return res, g.last_candidates

    first = run(gen)
    second = run(gen)
    n = len(gen._graphs)
    assert second == first and n >= 1
    assert run(gen) == first and len(gen._graphs) == n   # replayed, not captured again
    if mode != "diverse":
        assert flatten(mode, first)[0] == flatten(mode, ref.run_case(3, mode, "all")[0])[0]
    monkeypatch.setenv("VC_DECODE_GRAPH", "0")
    eager = CaptionGenerator(gen.e)
    assert run(eager) == first and len(eager._graphs) == 0


@pytest.mark.parametrize("mode", ["greedy", "beam_search"])
def test_a_new_banned_list_goes_through_the_captured_graph(lib, mode):
    gen, *inp = case(3, mode, "banned")
    said = sorted({t for s in captions(mode, decode(gen, mode, *inp)) for t in s} - {BOS, EOS})
    assert len(said) >= 4
    a, b = DecodeControls(banned=said[:2]), DecodeControls(banned=said[2:4])
    decode(gen, mode, *inp, a)
    ra = decode(gen, mode, *inp, a)
    n = len(gen._graphs)
    rb = decode(gen, mode, *inp, b)
    assert len(gen._graphs) == n and rb != ra
    assert rb == decode(CaptionGenerator(gen.e), mode, *inp, b)
    for res, ctl in ((ra, a), (rb, b)):
        for s in captions(mode, res):
            assert not set(s) & set(ctl.banned.tolist()), (s, ctl)


def test_refusals_launch_nothing(lib):
    gen, feats, cv, eps, cons = case(1, "constrained_beam_search", "all")
    bad = [DecodeControls(banned=[EOS]), DecodeControls(banned=range(3, 32)), DecodeControls(min_len=10), DecodeControls(banned=[40])]
    for ctl in bad:
        for call in (lambda c: gen.greedy(feats, cv, eps, BOS, EOS, max_len=10, controls=c),
                     lambda c: gen.sample(feats, cv, eps, BOS, EOS, max_len=10, controls=c),
                     lambda c: gen.diverse(feats, cv, None, BOS, EOS, draws=2, max_len=10, controls=c),
                     lambda c: gen.beam_search(feats, cv, eps, BOS, EOS, beam_size=3, max_len=10, controls=c),
                     lambda c: gen.diverse_beam_search(feats, cv, eps, BOS, EOS, groups=2, group_size=2, max_len=10, controls=c),
                     lambda c: gen.constrained_beam_search(feats, cons, cv, eps, BOS, EOS, beam_size=3, max_len=10, controls=c)):
            with pytest.raises(ValueError):
                call(ctl)
    with pytest.raises(ValueError):   # banned and required
        gen.constrained_beam_search(feats, cons, cv, eps, BOS, EOS, beam_size=3, max_len=10, controls=DecodeControls(banned=[cons[2][0][1]]))
    with pytest.raises(ValueError):
        gen.greedy(feats, cv, eps, BOS, EOS, max_len=10, controls=dict(min_len=3))
    for name in ("marginal_greedy", "marginal_beam_search"):   # the mixture searches do not take the keyword
        with pytest.raises(TypeError):
            getattr(gen, name)(feats, cv, None, BOS, EOS, draws=2, controls=DecodeControls(min_len=3))
    assert gen.buf == {} and gen._graphs == {}   # no buffer was made: nothing ran


def test_main_synthetic_inference_with_all_four_flags(tmp_path):
    """main.py --synthetic --mode inference with the four flags and --eval_captions in a fresh process (on a checkpoint written here):
    no written caption repeats a bigram, ends before five words or holds a banned word; the metrics file lists the flags"""
    from vae_captioning_amd.utils.parameters import Parameters
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden, p.latent_size, p.gen_z_samples = 32, 64, 64, 10, 4
    P0 = spec.init_caption_params(p, 200, seed=3)
    os.makedirs(tmp_path / "checkpoints")
    np.savez(str(tmp_path / "checkpoints" / "dc.ckpt.npz"), **{k: (v * 3).astype(np.float32) for k, v in P0.items()})
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "200", "--embed_dim", "32",
            "--enc_hid", "64", "--dec_hid", "64", "--latent", "10", "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "dc",
            "--mode", "inference", "--beam_size", "3", "--gen_name", "dc"]
    # what the model says when it may say anything: the banned words are taken from it
    r = subprocess.run(base, cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    free = [x["caption"].split() for x in json.load(open(tmp_path / "val_dc.json"))]
    words = sorted({w for c in free for w in c})
    banned = [words[0], int(words[-1][1:]), "zebra"]   # a word, a token id, a word the vocabulary lacks
    (tmp_path / "ban.json").write_text(json.dumps(banned))
    r = subprocess.run(base + ["--no_repeat_ngram", "2", "--min_len", "5", "--repetition_penalty", "1.2", "--banned_words", str(tmp_path / "ban.json"),
                               "--eval_captions"], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "banned words: 2 token ids; dropped 1 unknown words" in r.stdout
    assert "decoding controls: no_repeat_ngram 2, min_len 5, repetition_penalty 1.2, 2 banned words" in r.stdout
    recs = json.load(open(tmp_path / "val_dc.json"))
    assert len(recs) == 8 and all(set(x) == {"image_id", "caption"} for x in recs)   # the records gain nothing
    for x in recs:
        toks = x["caption"].split()
        grams = list(zip(toks, toks[1:]))
        assert len(grams) == len(set(grams)) and len(toks) >= 5, x
        assert not set(toks) & {words[0], words[-1]}, x
    m = json.load(open(tmp_path / "val_dc_metrics.json"))
    assert (m["no_repeat_ngram"], m["min_len"], m["repetition_penalty"]) == (2, 5, 1.2) and m["banned_words"].endswith("ban.json")
