"""-m gpu: constrained beam search -- vc_beam_update_constrained bit for bit against the Python reference of tests/cbs_ref.py, what its
banks mean, CaptionGenerator.constrained_beam_search against the float64 reference end to end, its identities with beam_search, graph
replay and slices, the argument checks and the command line."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from vae_captioning_amd import abi, spec
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.generate import CaptionGenerator

from . import cbs_ref
from .gpu_util import BeamState, P, dev, host, stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOS, EOS = 1, 2
SHAPES = [(0, 0, 5), (1, 1, 8), (1, 4, 2), (2, 2, 4), (3, 1, 2), (3, 4, 2), (2, 3, 3)]   # (C, Wc, w): tests/test_cbs_host.py shows float32 = float64 here


def start_state(lib, B, S, w, L):
    """vc_beam_init on junk-filled buffers for B*S virtual images, then only bank 0 of every image keeps its beam"""
    st = BeamState(lib, B * S, w, L, BOS)
    st.pcount.view(B, S)[:, 1:] = 0
    return st


def kernel_constraints(seed, B, V, C, Wc):
    """cbs_ref.constraints (for C >= 2 the last image has fewer sets than C) with image 0's sets all empty and, where a set has room, an
    entry outside the vocabulary (counts as absent)"""
    cons = cbs_ref.constraints(seed, B, V, C, Wc)
    if C:
        cons[0] = -1
        if Wc >= 2:
            cons[1, 0, 1] = 1000
    return cons


def level_rows(rng, rows, V, eos_ok):
    """[rows, V] float32 drawn from a few levels (1e-13 among them: skipped words): exact ties everywhere, which the stable sort breaks
    towards the lower id -- so <EOS> = 2 is listed often; eos_ok False: a vocabulary without <EOS> (its column is skipped)"""
    levels = np.array([0.5, 0.25, 0.25, 0.125, 1e-13], np.float32)
    probs = rng.choice(levels, size=(rows, V)).astype(np.float32)
    if not eos_ok:
        probs[:, EOS] = 1e-13
    return probs


def device_tables(probs, live, kc, ld):
    """what the kernel gets for one round: probs with stride ld, NaN in the rows of empty slots; the lists = the stable descending
    argsort's first kc of every live row, junk (NaN, an id far outside the vocabulary) for the others"""
    rows, V = probs.shape
    ti = np.argsort(-probs, axis=1, kind="stable")[:, :kc].astype(np.int32)
    tv = np.take_along_axis(probs, ti, axis=1)
    wide = np.full((rows, ld), np.nan, np.float32)
    wide[:, :V] = probs
    wide[~live] = np.nan
    tv[~live], ti[~live] = np.nan, 1 << 20
    return dev(wide), dev(tv), dev(ti)


def live_rows(pcount, w):
    """[Bv * w] bool from the banks' live counts: row v*w + i is read by the next round iff i < pcount[v]"""
    return (np.arange(w)[None, :] < np.asarray(pcount)[:, None]).reshape(-1)


def check_round(snap, partial, complete, B, S, w, L, where):
    """every bank of every image: the heap arrays, the complete heaps through their pool slots, the free mask, parent (GLOBAL rows:
    a beam's .state is its source row within its image) / tok -- scores bit for bit.  Returns how many live beams changed bank."""
    Bv = B * S
    ps, plp, pl = snap["p_score"].reshape(Bv, w), snap["p_logprob"].reshape(Bv, w), snap["p_len"].reshape(Bv, w)
    sn = snap["sent"].reshape(Bv, w, L)
    cs, clp, cl = snap["c_score"].reshape(Bv, w), snap["c_logprob"].reshape(Bv, w), snap["c_len"].reshape(Bv, w)
    csl, cst = snap["c_slot"].reshape(Bv, w), snap["c_sent"].reshape(Bv, w + 1, L)
    par, tk = snap["parent"].reshape(Bv, w), snap["tok"].reshape(Bv, w)
    moved = 0
    for b in range(B):
        for s in range(S):
            v, at = b * S + s, where + (b, s)
            heap = partial[b][s]._data
            assert snap["pcount"][v] == len(heap), at + (snap["pcount"][v], len(heap))
            for j, bm in enumerate(heap):   # heap ARRAY order, not sorted order
                assert sn[v, j, :pl[v, j]].tolist() == bm.sentence, at + (j,)
                assert ps[v, j] == bm.score and plp[v, j] == bm.logprob, at + (j, ps[v, j], bm.score, plp[v, j], bm.logprob)
                assert par[v, j] == b * S * w + bm.state and tk[v, j] == bm.sentence[-1], at + (j,)
                moved += bm.state // w != s
            assert (par[v, len(heap):] == v * w).all() and (tk[v, len(heap):] == 0).all(), at   # empty slots: the defaults
            cheap = complete[b][s]._data
            assert snap["ccount"][v] == len(cheap), at
            slots = [int(csl[v, j]) for j in range(len(cheap))]
            assert len(set(slots)) == len(slots) and all(0 <= x <= w for x in slots), at
            assert snap["c_free"][v] == ((1 << (w + 1)) - 1) & ~sum(1 << x for x in slots), at
            for j, bm in enumerate(cheap):
                assert cst[v, csl[v, j], :cl[v, j]].tolist() == bm.sentence, at + (j,)
                assert cs[v, j] == bm.score and clp[v, j] == bm.logprob, at + (j,)
    return moved


KERNEL_SHAPES = [(0, 1, 5, 6, 12, True), (1, 1, 1, 6, 12, True), (1, 1, 8, 6, 12, True), (1, 4, 2, 6, 12, True), (2, 2, 4, 6, 12, True),
                 (2, 3, 3, 6, 12, True), (3, 1, 2, 6, 12, True), (3, 4, 2, 6, 12, True), (1, 2, 2, 70, 80, False)]
KERNEL_IDS = ["no-constraints-is-vc_beam_update", "smallest", "two-banks-of-eight", "four-words-a-set", "all-sixteen-lanes", "twelve-of-sixteen",
              "eight-banks", "kc14-twelve-forced-words", "captions-longer-than-a-wave"]


@pytest.mark.parametrize("C,Wc,w,rounds,L,eos_ok", KERNEL_SHAPES, ids=KERNEL_IDS)
def test_kernel_replays_the_reference_bit_for_bit(lib, C, Wc, w, rounds, L, eos_ok):
    """vc_beam_update_constrained against tests/cbs_ref.py (table_rounds) after EVERY round, for every bank of every image: heap arrays
    (sentences, scores, log-probabilities, lengths), complete heaps and their pool slots, the free mask, parent / tok.  The rows are
    drawn from a few levels, so exact ties and skipped words are frequent; image 0 has no constraint, one image fewer than C, one entry
    lies outside the vocabulary; the rows of empty slots hold NaN and junk lists; the start state is vc_beam_init's on junk-filled
    buffers.  The last case: a vocabulary without <EOS>, so captions grow past 64 tokens."""
    B, V, lnf = 7, 24, 0.7
    ld, S = V + 3, 1 << C
    rng = np.random.default_rng(100 * C + 10 * Wc + w)
    cons = kernel_constraints(7 + C, B, V, C, Wc)
    kc = min(V, w + cbs_ref.n_words(cons[:, :C], V)) if C else w
    tables = [level_rows(rng, B * S * w, V, eos_ok) for _ in range(rounds)]
    st = start_state(lib, B, S, w, L)
    twin = BeamState(lib, B, w, L, BOS) if C == 0 else None   # C = 0: vc_beam_update itself on the same tables
    dcons = dev(cons) if C else None
    ref = cbs_ref.table_rounds(tables, cons, B, C, w, kc, BOS, EOS, lnf)
    finished = moved = 0
    live = live_rows(host(st.pcount), w)
    for it, probs in enumerate(tables):
        dprobs, dtv, dti = device_tables(probs, live, kc, ld)
        lib.vc_beam_update_constrained(stream(), B, C, Wc, w, kc, L, EOS, lnf, P(dcons), P(dtv), P(dti), P(dprobs), ld, V, *st.args(it))
        snap = st.snapshot(it)
        partial, complete = next(ref)
        moved += check_round(snap, partial, complete, B, S, w, L, (C, Wc, w, it))
        finished += sum(len(c._data) for cs in complete for c in cs)
        live = live_rows(snap["pcount"], w)
        if twin is not None:
            lib.vc_beam_update(stream(), B, w, L, EOS, lnf, P(dtv), P(dti), *twin.args(it))
            other = twin.snapshot(it)
            alive = np.arange(w)[None, :] < snap["pcount"][:, None]
            done = np.arange(w)[None, :] < snap["ccount"][:, None]
            for k in ("pcount", "ccount", "c_free", "parent", "tok"):
                assert np.array_equal(snap[k], other[k]), (k, it)
            for k in ("p_score", "p_logprob", "p_len"):
                assert np.array_equal(snap[k].reshape(B, w)[alive], other[k].reshape(B, w)[alive]), (k, it)
            for k in ("c_score", "c_logprob", "c_len", "c_slot"):
                assert np.array_equal(snap[k].reshape(B, w)[done], other[k].reshape(B, w)[done]), (k, it)
    assert (finished > 0) == eos_ok          # a caption finished in the <EOS> cases ...
    assert (moved > 0) == (C > 0)            # ... and some beam changed bank wherever there are constraints: else this shows nothing
    if not eos_ok:
        assert snap["p_len"].max() == rounds + 1 > 64


def test_banks_hold_what_their_state_says_and_the_models_log_probability(lib):
    """Meaning, not only parity: (C, Wc, w) = (2, 2, 4) on rows without <EOS> and p >= 1e-6.  After every round every live sentence of
    bank t contains a word of each set in t and of no other set, and its stored log-probability is the sum of its words' float32
    logs: followed here along the parent rows in float64 from numpy's float32 log.  The device's logf may differ from numpy's by an
    ulp or two of float32 at |log p| <= 13.9, i.e. <= 2 * 2^-23 * 13.9 = 3.4e-6 per word, 2e-5 over the six rounds."""
    B, V, C, Wc, w, L, rounds = 5, 24, 2, 2, 4, 12, 6
    S, ld = 1 << C, V
    rng = np.random.default_rng(11)
    cons = cbs_ref.constraints(5, B, V, C, Wc)
    sets = [cbs_ref.sets_of(cons[b], V) for b in range(B)]
    kc = w + C * Wc
    dcons = dev(cons)
    st = start_state(lib, B, S, w, L)
    live = live_rows(host(st.pcount), w)
    want_lp = np.zeros(B * S * w)
    moved = 0
    for it in range(rounds):
        probs = rng.uniform(1e-6, 0.5, size=(B * S * w, V)).astype(np.float32)
        probs[:, EOS] = 0.0
        dprobs, dtv, dti = device_tables(probs, live, kc, ld)
        lib.vc_beam_update_constrained(stream(), B, C, Wc, w, kc, L, EOS, 0.7, P(dcons), P(dtv), P(dti), P(dprobs), ld, V, *st.args(it))
        snap = st.snapshot(it)
        assert (snap["ccount"] == 0).all()
        new_lp = np.zeros_like(want_lp)
        for b in range(B):
            for t in range(S):
                v = b * S + t
                for j in range(snap["pcount"][v]):
                    r = v * w + j
                    sent = snap["sent"].reshape(-1, L)[r, :snap["p_len"][r]].tolist()
                    met = sum(1 << k for k, words in enumerate(sets[b]) if set(words) & set(sent))
                    assert met == t and len(sent) == it + 2, (it, b, t, sent, sets[b])
                    par, tok = snap["parent"][r], snap["tok"][r]
                    assert b * S * w <= par < (b + 1) * S * w and live[par] and tok == sent[-1]
                    moved += par // w != v
                    new_lp[r] = want_lp[par] + float(np.log(probs[par, tok]))
                    assert abs(snap["p_logprob"][r] - new_lp[r]) <= 3.4e-6 * (it + 1), (it, r, snap["p_logprob"][r], new_lp[r])
                    assert snap["p_score"][r] == snap["p_logprob"][r]
        want_lp, live = new_lp, live_rows(snap["pcount"], w)
        assert snap["pcount"].reshape(B, S)[:, 0].min() == w or it == 0   # bank 0 is full from round 2 on: 20 free words a row
    full = [cbs_ref.full_mask(cons[b], V) for b in range(B)]   # (the last image has one set of the two: its accepting bank is 1)
    assert full == [3] * (B - 1) + [1]
    assert moved > 0 and all(snap["pcount"][b * S + full[b]] == w for b in range(B))   # every image filled its accepting bank


# ---------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def inputs(case, seed=7):
    return cbs_ref.model_inputs(seed, V=40, B=6, **cbs_ref.CASES[case])


def cons_of(C, Wc, seed=None):
    return cbs_ref.constraints(100 + 10 * C + Wc if seed is None else seed, 6, 40, C, Wc)


def as_lists(cons):
    """the [B, C, Wc] table as constrained_beam_search takes it: per image its non-empty sets (an emptied set is an image's last)"""
    return [[st for st in cbs_ref.sets_of(ci) if st] for ci in cons]


@functools.lru_cache(maxsize=None)
def ref64(case, C, Wc, w, max_len=10, seed=7, cons_seed=None):
    return cbs_ref.reference(*inputs(case, seed), BOS, EOS, cons_of(C, Wc, cons_seed), beam_size=w, max_len=max_len)


def generator(lib, case, seed=7):
    p, P0, feats, cv, eps, cm = inputs(case, seed)
    eng = CaptionEngine(p, 40, lib=lib)
    eng.load_params(P0)
    return CaptionGenerator(eng), feats, (cv if spec.uses_ci(p) else None), eps


sents = lambda res: [[[s for s, _ in bank] for bank in im] for im in res]
scores = lambda res: [sc for im in res for bank in im for _, sc in bank]
ref_sents = lambda ref: [[bank[0] for bank in im] for im in ref]
ref_scores = lambda ref: [sc for im in ref for bank in im for sc in bank[1]]


@pytest.mark.parametrize("case", range(4), ids=cbs_ref.CASE_IDS)
@pytest.mark.parametrize("C,Wc,w", SHAPES)
def test_constrained_beam_search_matches_the_float64_reference(lib, case, C, Wc, w):
    """the four prior cases, seed 7, max_len 10: every bank's token sequences identical for every image, scores within the plain and
    group beam tests' tolerance; the default result is the selection rule applied to the reference"""
    gen, feats, cv, eps = generator(lib, case)
    cons = cons_of(C, Wc)
    lists = as_lists(cons)
    got = gen.constrained_beam_search(feats, lists, cv, eps, BOS, EOS, beam_size=w, max_len=10, all_states=True)
    ref = ref64(case, C, Wc, w)
    assert len(got) == 6 and all(len(im) == 1 << C for im in got)
    for b in range(6):
        assert sents(got)[b] == ref_sents(ref)[b], (b, got[b], ref[b])
    np.testing.assert_allclose(scores(got), ref_scores(ref), rtol=1e-4, atol=1e-5)
    best = gen.constrained_beam_search(feats, lists, cv, eps, BOS, EOS, beam_size=w, max_len=10)
    for b in range(6):
        (rs, rsc), rstate = cbs_ref.select(ref[b], cbs_ref.full_mask(cons[b]) if C else 0, EOS)
        beams, state = best[b]
        assert state == rstate and [s for s, _ in beams] == rs, (b, best[b], rs, rstate)
        np.testing.assert_allclose([sc for _, sc in beams], rsc, rtol=1e-4, atol=1e-5)
        assert beams == got[b][state]


@pytest.mark.parametrize("case", [1, 3], ids=["normal", "gmm"])
def test_identities_with_beam_search(lib, case):
    """no constraints is beam_search(beam_size = w) exactly, scores included -- with no image constrained and with an empty list; and
    beam_search afterwards is still what it was"""
    gen, feats, cv, eps = generator(lib, case)
    for w in (3, 5, 10):
        plain = gen.beam_search(feats, cv, eps, BOS, EOS, beam_size=w, max_len=10)
        free = gen.constrained_beam_search(feats, [[]] * 6, cv, eps, BOS, EOS, beam_size=w, max_len=10)
        assert [beams for beams, _ in free] == plain and all(state == 0 for _, state in free)
        banks = gen.constrained_beam_search(feats, [[]] * 6, cv, eps, BOS, EOS, beam_size=w, max_len=10, all_states=True)
        assert [im[0] for im in banks] == plain
        assert gen.beam_search(feats, cv, eps, BOS, EOS, beam_size=w, max_len=10) == plain


def test_replayed_graphs_decode_the_call_and_the_constraints(lib, monkeypatch):
    """A second and third call replay the captured chunks and return the first call's result; OTHER constraints of the same shape
    through the replayed graph decode THOSE; another shape, then back; VC_DECODE_GRAPH=0 gives the same with no graphs."""
    gen, feats, cv, eps = generator(lib, 3)
    kw = dict(beam_size=4, max_len=10, all_states=True)
    lists = as_lists(cons_of(2, 2))
    first = gen.constrained_beam_search(feats, lists, cv, eps, BOS, EOS, **kw)
    assert sents(first) == ref_sents(ref64(3, 2, 2, 4))
    n_graphs = len(gen._graphs)
    assert n_graphs >= 1
    for _ in range(2):
        assert gen.constrained_beam_search(feats, lists, cv, eps, BOS, EOS, **kw) == first
    assert len(gen._graphs) == n_graphs   # replayed, not captured again
    # other constraints of the same shape through the same graphs
    other = as_lists(cons_of(2, 2, seed=999))
    got2 = gen.constrained_beam_search(feats, other, cv, eps, BOS, EOS, **kw)
    assert len(gen._graphs) == n_graphs
    assert got2 == CaptionGenerator(gen.e).constrained_beam_search(feats, other, cv, eps, BOS, EOS, **kw) and got2 != first
    assert sents(got2) == ref_sents(ref64(3, 2, 2, 4, cons_seed=999))
    # another shape, and back
    for C, Wc, w in ((1, 4, 2), (3, 1, 2), (0, 0, 5)):
        ls, kw2 = as_lists(cons_of(C, Wc)), dict(kw, beam_size=w)
        fresh = CaptionGenerator(gen.e).constrained_beam_search(feats, ls, cv, eps, BOS, EOS, **kw2)
        assert gen.constrained_beam_search(feats, ls, cv, eps, BOS, EOS, **kw2) == fresh, (C, Wc, w)
        assert gen.constrained_beam_search(feats, ls, cv, eps, BOS, EOS, **kw2) == fresh, (C, Wc, w)   # (its own replay)
    assert gen.constrained_beam_search(feats, lists, cv, eps, BOS, EOS, **kw) == first
    monkeypatch.setenv("VC_DECODE_GRAPH", "0")
    eager = CaptionGenerator(gen.e)
    assert eager.constrained_beam_search(feats, lists, cv, eps, BOS, EOS, **kw) == first and len(eager._graphs) == 0


@pytest.mark.parametrize("slices", [2, 3])
def test_sliced_search_returns_the_single_slice_banks(lib, slices, monkeypatch):
    """six images as 2 x 3 and 3 x 2 slices on streams (row threshold lowered), cut between images, each with its own part of the
    constraint table: the banks of VC_DECODE_SLICES=1 and of the float64 reference, eager and replayed"""
    gen, feats, cv, eps = generator(lib, 3)
    kw = dict(beam_size=4, max_len=10, all_states=True)
    lists = as_lists(cons_of(2, 2))
    gen.slices, gen.slice_rows = slices, 1
    got = [gen.constrained_beam_search(feats, lists, cv, eps, BOS, EOS, **kw) for _ in range(3)]
    assert len(gen._side) == slices - 1
    monkeypatch.setenv("VC_DECODE_SLICES", "1")
    single = CaptionGenerator(gen.e).constrained_beam_search(feats, lists, cv, eps, BOS, EOS, **kw)
    assert got[0] == single and got[1] == single and got[2] == single
    assert sents(single) == ref_sents(ref64(3, 2, 2, 4))


@pytest.mark.parametrize("max_len,check_every", [(2, 4), (3, 4), (10, 0), (9, 2)], ids=["one-round", "two-rounds", "no-checks", "chunks-of-two"])
def test_edge_lengths_and_check_intervals(lib, max_len, check_every):
    gen, feats, cv, eps = generator(lib, 3)
    lists = as_lists(cons_of(2, 2))
    ref = ref_sents(ref64(3, 2, 2, 4, max_len))
    for call in range(2):
        got = gen.constrained_beam_search(feats, lists, cv, eps, BOS, EOS, beam_size=4, max_len=max_len, check_every=check_every, all_states=True)
        assert sents(got) == ref, call


def test_argument_errors_launch_nothing(lib):
    """every refused argument: a non-zero code and a message, the state untouched; the Python ValueErrors come before any device work"""
    B, C, Wc, w, L, V = 2, 2, 2, 4, 12, 24
    st = start_state(lib, B, 1 << C, w, L)
    before = st.snapshot(0)
    rows = B * (1 << C) * w
    cons = dev(np.full((B, 3, 4), 5, np.int32))
    tv, ti = dev(np.full((rows, 16), 0.25, np.float32)), dev(np.full((rows, 16), 3, np.int32))
    probs = dev(np.full((rows, V), 0.25, np.float32))
    ok = dict(C=C, Wc=Wc, w=w, kc=8, ld=V, V=V, cons=P(cons), tv=P(tv), ti=P(ti), probs=P(probs))

    def call(**kw):
        a = dict(ok, **kw)
        lib.vc_beam_update_constrained(stream(), B, a["C"], a["Wc"], a["w"], a["kc"], L, EOS, 0.7, a["cons"], a["tv"], a["ti"], a["probs"], a["ld"],
                                       a["V"], *st.args(0))

    for kw, word in ((dict(C=-1), "constraints per image"), (dict(C=4, w=1), "constraints per image"), (dict(Wc=0), "words per constraint"),
                     (dict(Wc=5), "words per constraint"), (dict(w=0), "beams per state"), (dict(w=5), "beams per state"), (dict(C=0, w=17, kc=17), "beams per state"),
                     (dict(kc=3), "candidates"), (dict(kc=9), "candidates"), (dict(V=6, ld=6, kc=7), "candidates"), (dict(ld=V - 1), "row stride"),
                     (dict(cons=None), "null pointer"), (dict(probs=None), "null pointer"), (dict(tv=None), "null pointer"), (dict(ti=None), "null pointer")):
        with pytest.raises(abi.VaecapError, match=word):
            call(**kw)
    with pytest.raises(abi.VaecapError, match="null pointer"):
        lib.vc_beam_update_constrained(stream(), B, C, Wc, w, 8, L, EOS, 0.7, P(cons), P(tv), P(ti), P(probs), V, V, *((None,) + st.args(0)[1:]))
    after = st.snapshot(0)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    gen, feats, cv, eps = generator(lib, 1)
    for bad, w in (([[[3], [4], [5], [6]]] * 6, 1), ([[[3, 4, 5, 6, 7]]] * 6, 2), ([[[]]] * 6, 2), ([[[3, 4], [4]]] * 6, 2), ([[[40]]] * 6, 2),
                   ([[[BOS]]] * 6, 2), ([[[EOS]]] * 6, 2), ([[[3], [4]]] * 6, 5), ([[[3]]] * 5, 2)):
        with pytest.raises(ValueError):
            gen.constrained_beam_search(feats, bad, cv, eps, BOS, EOS, beam_size=w)
    assert gen.buf == {} and gen._graphs == {}   # no buffer was made: nothing ran


def test_main_synthetic_inference_with_constrained_beam_search(tmp_path):
    """main.py --synthetic --mode inference --sample_gen constrained_beam in a fresh process (on a checkpoint written here), the
    constraints file a "*" entry of two integer sets: every record names its constraints, says which were satisfied and carries a score,
    and wherever a constraint is said to be satisfied the caption holds one of its words"""
    from vae_captioning_amd.utils.parameters import Parameters
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden, p.latent_size, p.gen_z_samples = 32, 64, 64, 10, 4
    P0 = spec.init_caption_params(p, 200, seed=3)
    os.makedirs(tmp_path / "checkpoints")
    np.savez(str(tmp_path / "checkpoints" / "cb.ckpt.npz"), **{k: (v * 3).astype(np.float32) for k, v in P0.items()})
    sets = [[17, 23], [101]]
    (tmp_path / "cons.json").write_text(json.dumps({"*": sets}))
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "200", "--embed_dim", "32",
           "--enc_hid", "64", "--dec_hid", "64", "--latent", "10", "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "cb",
           "--mode", "inference", "--sample_gen", "constrained_beam", "--constraints", str(tmp_path / "cons.json"), "--gen_name", "cb"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "dropped 0 unknown words and 0 emptied sets" in r.stdout
    recs = json.load(open(tmp_path / "val_cb.json"))
    assert len(recs) == 8
    for x in recs:
        assert x["constraints"] == sets and len(x["satisfied"]) == 2 and all(isinstance(s, bool) for s in x["satisfied"])
        assert isinstance(x["score"], float) and x["score"] <= 0.0 and x["image_id"].startswith("synthetic_")
        ids = [int(word[1:]) for word in x["caption"].split()]   # (the synthetic dictionary's word of id i is "w<i>")
        for j, st in enumerate(sets):
            if x["satisfied"][j]:
                assert set(st) & set(ids), x
    assert any(any(x["satisfied"]) for x in recs)
