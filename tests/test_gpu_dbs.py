"""-m gpu: group ("diverse") beam search -- vc_beam_update_groups bit for bit against the Python reference of tests/dbs_ref.py,
CaptionGenerator.diverse_beam_search against the float64 reference end to end, its identities with beam_search, graph replay and
slices, the argument checks and the command line."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import abi, spec
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.generate import CaptionGenerator

from . import dbs_ref
from .gpu_util import BeamState, P, dev, stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOS, EOS = 1, 2
SHAPES = [(3, 2), (2, 4), (5, 2), (4, 1)]   # the shapes tests/test_dbs_host.py shows float32 and float64 to agree on


def make_tables(rng, rows, kc, rounds, lo, hi):
    """top-k tables with probabilities quantised to a few levels (1e-13 among them: skipped words) and words from [lo, hi): exact key
    ties, <EOS> hits (lo = 2) and words repeated across groups are frequent."""
    levels = np.array([0.5, 0.25, 0.25, 0.125, 1e-13], np.float32)
    out = []
    for _ in range(rounds):
        tv = np.sort(rng.choice(levels, size=(rows, kc)).astype(np.float32), axis=1)[:, ::-1].copy()
        ti = rng.integers(lo, hi, size=(rows, kc)).astype(np.int32)
        out.append((tv, ti))
    return out


def check_round(snap, partial, complete, B, G, w, L, where):
    """every virtual image: the heap arrays, the complete heaps through their pool slots, parent / tok -- scores bit for bit"""
    Bv = B * G
    ps, plp, pl = snap["p_score"].reshape(Bv, w), snap["p_logprob"].reshape(Bv, w), snap["p_len"].reshape(Bv, w)
    sn = snap["sent"].reshape(Bv, w, L)
    cs, clp, cl = snap["c_score"].reshape(Bv, w), snap["c_logprob"].reshape(Bv, w), snap["c_len"].reshape(Bv, w)
    csl, cst = snap["c_slot"].reshape(Bv, w), snap["c_sent"].reshape(Bv, w + 1, L)
    par, tk = snap["parent"].reshape(Bv, w), snap["tok"].reshape(Bv, w)
    for b in range(B):
        for g in range(G):
            v, at = b * G + g, where + (b, g)
            heap = partial[b][g]._data
            assert snap["pcount"][v] == len(heap), at
            for j, bm in enumerate(heap):   # heap ARRAY order, not sorted order
                assert sn[v, j, :pl[v, j]].tolist() == bm.sentence, at + (j,)
                assert ps[v, j] == bm.score and plp[v, j] == bm.logprob, at + (j, ps[v, j], bm.score, plp[v, j], bm.logprob)
                assert par[v, j] == v * w + bm.state and tk[v, j] == bm.sentence[-1], at + (j,)
            assert (par[v, len(heap):] == v * w).all() and (tk[v, len(heap):] == 0).all(), at   # empty slots: the defaults
            cheap = complete[b][g]._data
            assert snap["ccount"][v] == len(cheap), at
            slots = [int(csl[v, j]) for j in range(len(cheap))]
            assert len(set(slots)) == len(slots) and all(0 <= s <= w for s in slots), at
            assert snap["c_free"][v] == ((1 << (w + 1)) - 1) & ~sum(1 << s for s in slots), at
            for j, bm in enumerate(cheap):
                assert cst[v, csl[v, j], :cl[v, j]].tolist() == bm.sentence, at + (j,)
                assert cs[v, j] == bm.score and clp[v, j] == bm.logprob, at + (j,)


KERNEL_SHAPES = [(1, 5, 6, 12, 2), (3, 3, 6, 12, 2), (2, 5, 6, 12, 2), (4, 4, 6, 12, 2), (2, 8, 5, 12, 2), (5, 2, 6, 12, 2), (16, 1, 6, 12, 2),
                 (2, 2, 70, 80, 3), (1, 9, 6, 12, 2), (1, 16, 5, 12, 2)]
KERNEL_IDS = ["one-group-is-vc_beam_update", "kc9-seven-rows-a-block", "kc10", "exactly-64-candidates", "128-candidates-two-blocks",
              "default-5x2", "longest-chosen-list", "captions-longer-than-a-wave", "one-group-of-nine", "one-group-of-sixteen"]


@pytest.mark.parametrize("lam", [0.5, 0.25, 0.3], ids=["lam0.5", "lam0.25", "lam0.3-not-dyadic"])
@pytest.mark.parametrize("G,w,rounds,L,lo", KERNEL_SHAPES, ids=KERNEL_IDS)
def test_kernel_replays_the_reference_bit_for_bit(lib, G, w, rounds, L, lo, lam):
    """vc_beam_update_groups against tests/dbs_ref.py (table_rounds) after EVERY round, for every group of every image: heap arrays
    (sentences, scores, model log-probabilities, lengths), complete heaps and their pool slots, the free mask, parent / tok.  The
    tables make exact ties frequent -- lambda 0.5 and 0.25 are exact in binary, so penalised and unpenalised keys tie too -- and 0.3
    tells a rounded product and difference from an fma.  The start state is vc_beam_init's on junk-filled buffers.  lo = 3: a
    vocabulary without <EOS>, so captions grow past 64 tokens."""
    B, lnf, kc = 7, 0.7, G * w
    rng = np.random.default_rng(1000 * G + w)
    tables = make_tables(rng, B * G * w, kc, rounds, lo, 6)
    st = BeamState(lib, B * G, w, L, BOS)
    twin = BeamState(lib, B, w, L, BOS) if G == 1 else None   # G = 1: vc_beam_update itself on the same tables
    ref = dbs_ref.table_rounds(tables, B, G, w, lam, BOS, EOS, lnf)
    finished = 0
    for it, (tv, ti) in enumerate(tables):
        dtv, dti = dev(tv), dev(ti)
        lib.vc_beam_update_groups(stream(), B, G, w, kc, L, EOS, lnf, lam, P(dtv), P(dti), *st.args(it))
        snap = st.snapshot(it)
        partial, complete = next(ref)
        check_round(snap, partial, complete, B, G, w, L, (G, w, lam, it))
        finished += sum(len(c._data) for cs in complete for c in cs)
        if twin is not None:
            lib.vc_beam_update(stream(), B, w, L, EOS, lnf, P(dtv), P(dti), *twin.args(it))
            other = twin.snapshot(it)
            live = np.arange(w)[None, :] < snap["pcount"][:, None]
            done = np.arange(w)[None, :] < snap["ccount"][:, None]
            for k in ("pcount", "ccount", "c_free", "parent", "tok"):
                assert np.array_equal(snap[k], other[k]), (k, it)
            for k in ("p_score", "p_logprob", "p_len"):
                assert np.array_equal(snap[k].reshape(B, w)[live], other[k].reshape(B, w)[live]), (k, it)
            for k in ("c_score", "c_logprob", "c_len", "c_slot"):
                assert np.array_equal(snap[k].reshape(B, w)[done], other[k].reshape(B, w)[done]), (k, it)
    assert (finished > 0) == (lo == 2)


def test_a_large_penalty_makes_the_live_words_of_an_image_distinct(lib):
    """Meaning, not only parity: six groups of one beam, lambda = 1000, rows of six DISTINCT words without <EOS> and p >= 1e-6 (a
    round costs a beam at most 13.9, six rounds far less than one penalty): every group finds an unpenalised word, so after every
    round the six live words of an image are pairwise distinct."""
    B, G, w, L, rounds = 5, 6, 1, 12, 6
    rng = np.random.default_rng(3)
    st = BeamState(lib, B * G, w, L, BOS)
    for it in range(rounds):
        tv = np.sort(rng.uniform(1e-6, 0.5, size=(B * G, G)).astype(np.float32), axis=1)[:, ::-1].copy()
        ti = np.stack([rng.permutation(np.arange(3, 11))[:G] for _ in range(B * G)]).astype(np.int32)
        lib.vc_beam_update_groups(stream(), B, G, w, G, L, EOS, 0.7, 1000.0, P(dev(tv)), P(dev(ti)), *st.args(it))
        snap = st.snapshot(it)
        assert (snap["pcount"] == 1).all() and (snap["ccount"] == 0).all()
        words = snap["tok"].reshape(B, G)
        assert all(len(set(words[b].tolist())) == G for b in range(B)), (it, words)
        assert (snap["p_logprob"] > -14.0 * (it + 1)).all()   # the stored log-probability carries no penalty


# ---------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def inputs(case, seed=7):
    return dbs_ref.model_inputs(seed, **dbs_ref.CASES[case])


@functools.lru_cache(maxsize=None)
def ref64(case, G, w, lam, max_len=10, seed=7):
    return dbs_ref.reference(*inputs(case, seed), BOS, EOS, groups=G, group_size=w, diversity=lam, max_len=max_len)


def generator(lib, case, seed=7):
    p, P0, feats, cv, eps, cm = inputs(case, seed)
    eng = CaptionEngine(p, 40, lib=lib)
    eng.load_params(P0)
    return CaptionGenerator(eng), feats, (cv if spec.uses_ci(p) else None), eps


sents = lambda res: [[[s for s, _ in g] for g in im] for im in res]
scores = lambda res: [sc for im in res for g in im for _, sc in g]
distinct = lambda res: [len({tuple(s) for g in im for s, _ in g}) for im in res]


@pytest.mark.parametrize("case", range(4), ids=dbs_ref.CASE_IDS)
@pytest.mark.parametrize("G,w", SHAPES)
def test_diverse_beam_search_matches_the_float64_reference(lib, case, G, w):
    """the four prior cases, seed 7, lambda 0.5, max_len 10: every group's token sequences identical, scores within the plain beam
    test's tolerance; at (5, 2) the penalty yields more distinct captions per image than lambda = 0 on the same shape"""
    gen, feats, cv, eps = generator(lib, case)
    got = gen.diverse_beam_search(feats, cv, eps, BOS, EOS, groups=G, group_size=w, diversity=0.5, max_len=10)
    ref = ref64(case, G, w, 0.5)
    assert len(got) == feats.shape[0] and all(len(im) == G for im in got)
    for b in range(feats.shape[0]):
        assert sents(got)[b] == [g[0] for g in ref[b]], (b, got[b], ref[b])
    np.testing.assert_allclose(scores(got), [sc for im in ref for g in im for sc in g[1]], rtol=1e-4, atol=1e-5)
    if (G, w) == (5, 2):
        flat = gen.diverse_beam_search(feats, cv, eps, BOS, EOS, groups=G, group_size=w, diversity=0.0, max_len=10)
        d0, d5 = distinct(flat), distinct(got)
        print("distinct captions per image: lambda 0 %s, lambda 0.5 %s" % (d0, d5))
        assert all(a <= w for a in d0) and all(b >= a for a, b in zip(d0, d5)) and sum(d5) > sum(d0), (d0, d5)


@pytest.mark.parametrize("case", [1, 3], ids=["normal", "gmm"])
def test_identities_with_beam_search(lib, case):
    """groups = 1 is beam_search(beam_size = w) exactly, scores included, whatever the penalty; diversity = 0 makes every group that
    search"""
    gen, feats, cv, eps = generator(lib, case)
    for w in (3, 5):
        plain = gen.beam_search(feats, cv, eps, BOS, EOS, beam_size=w, max_len=10)
        one = gen.diverse_beam_search(feats, cv, eps, BOS, EOS, groups=1, group_size=w, diversity=0.7, max_len=10)
        assert [im[0] for im in one] == plain
        same = gen.diverse_beam_search(feats, cv, eps, BOS, EOS, groups=3, group_size=w, diversity=0.0, max_len=10)
        assert all(g == plain[b] for b, im in enumerate(same) for g in im)
        assert gen.beam_search(feats, cv, eps, BOS, EOS, beam_size=w, max_len=10) == plain   # (and beam_search is what it was)


def test_replayed_graphs_decode_the_call_and_the_setting(lib, monkeypatch):
    """A second and third call replay the captured chunks and return the first call's result; so does VC_DECODE_GRAPH=0; other
    inputs on a replayed graph decode THOSE inputs; another diversity or group shape after a captured one returns its own result."""
    gen, feats, cv, eps = generator(lib, 3)
    kw = dict(groups=3, group_size=2, diversity=0.5, max_len=10)
    first = gen.diverse_beam_search(feats, cv, eps, BOS, EOS, **kw)
    assert sents(first) == [[g[0] for g in im] for im in ref64(3, 3, 2, 0.5)]
    n_graphs = len(gen._graphs)
    assert n_graphs >= 1
    for _ in range(2):
        assert gen.diverse_beam_search(feats, cv, eps, BOS, EOS, **kw) == first
    assert len(gen._graphs) == n_graphs   # replayed, not captured again
    # other inputs through the same graphs (seed 11's images)
    _, _, feats2, cv2, eps2, _ = inputs(3, 11)
    got2 = gen.diverse_beam_search(feats2, None, eps2, BOS, EOS, **kw)
    gen_b = CaptionGenerator(gen.e)
    assert got2 == gen_b.diverse_beam_search(feats2, None, eps2, BOS, EOS, **kw) and got2 != first
    # another penalty, another shape, and back
    for other in (dict(kw, diversity=0.25), dict(kw, diversity=0.0), dict(kw, groups=2, group_size=3), dict(kw, groups=2)):
        fresh = CaptionGenerator(gen.e).diverse_beam_search(feats, cv, eps, BOS, EOS, **other)
        assert gen.diverse_beam_search(feats, cv, eps, BOS, EOS, **other) == fresh, other
        assert gen.diverse_beam_search(feats, cv, eps, BOS, EOS, **other) == fresh, other   # (its own replay)
    assert sents(gen.diverse_beam_search(feats, cv, eps, BOS, EOS, **dict(kw, diversity=0.25))) == [[g[0] for g in im] for im in ref64(3, 3, 2, 0.25)]
    assert gen.diverse_beam_search(feats, cv, eps, BOS, EOS, **kw) == first
    monkeypatch.setenv("VC_DECODE_GRAPH", "0")
    eager = CaptionGenerator(gen.e)
    assert eager.diverse_beam_search(feats, cv, eps, BOS, EOS, **kw) == first and len(eager._graphs) == 0


@pytest.mark.parametrize("slices", [2, 3])
def test_sliced_group_search_returns_the_single_slice_groups(lib, slices, monkeypatch):
    """six images as 2 x 3 and 3 x 2 slices on streams (row threshold lowered; V = 40 >= the rows x rounds that switch the projection
    table on): the groups of VC_DECODE_SLICES=1 and of the float64 reference, eager and replayed"""
    gen, feats, cv, eps = generator(lib, 3)
    kw = dict(groups=3, group_size=2, diversity=0.5, max_len=10)
    gen.slices, gen.slice_rows = slices, 1
    got = [gen.diverse_beam_search(feats, cv, eps, BOS, EOS, **kw) for _ in range(3)]
    assert len(gen._side) == slices - 1
    monkeypatch.setenv("VC_DECODE_SLICES", "1")
    single = CaptionGenerator(gen.e).diverse_beam_search(feats, cv, eps, BOS, EOS, **kw)
    assert got[0] == single and got[1] == single and got[2] == single
    assert sents(single) == [[g[0] for g in im] for im in ref64(3, 3, 2, 0.5)]


@pytest.mark.parametrize("max_len,check_every,G,w", [(2, 4, 3, 2), (3, 4, 3, 2), (10, 0, 3, 2), (10, 4, 2, 5), (9, 2, 4, 1)],
                         ids=["one-round", "two-rounds", "no-checks", "ten-candidates-unfused-topk", "chunks-of-two"])
def test_edge_lengths_and_check_intervals(lib, max_len, check_every, G, w):
    gen, feats, cv, eps = generator(lib, 3)
    ref = [[g[0] for g in im] for im in ref64(3, G, w, 0.5, max_len)]
    for call in range(2):
        got = gen.diverse_beam_search(feats, cv, eps, BOS, EOS, groups=G, group_size=w, diversity=0.5, max_len=max_len, check_every=check_every)
        assert sents(got) == ref, call


def test_argument_errors_launch_nothing(lib):
    """G*w = 17, kc < w, kc > G*w, a negative / NaN / infinite penalty: a non-zero code and a message, before any device work"""
    raw = ctypes.CDLL(abi.LIB_PATH)
    raw.vc_last_error.restype = ctypes.c_char_p
    st = BeamState(lib, 4, 4, 12, BOS)
    before = st.snapshot(0)
    tv, ti = dev(np.full((16, 4), 0.25, np.float32)), dev(np.full((16, 4), 3, np.int32))
    for G, w, kc, lam, word in ((17, 1, 16, 0.5, "group size must be"), (1, 17, 17, 0.5, "group size must be"), (2, 2, 1, 0.5, "candidates"), (2, 2, 5, 0.5, "candidates"),
                                (2, 2, 4, -0.5, "diversity"), (2, 2, 4, float("nan"), "diversity"), (2, 2, 4, float("inf"), "diversity"),
                                (0, 2, 2, 0.5, "bad argument")):
        with pytest.raises(abi.VaecapError, match=word):
            lib.vc_beam_update_groups(stream(), 2, G, w, kc, 12, EOS, 0.7, lam, P(tv), P(ti), *st.args(0))
    after = st.snapshot(0)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    gen, feats, cv, eps = generator(lib, 1)
    with pytest.raises(ValueError):
        gen.diverse_beam_search(feats, cv, eps, BOS, EOS, groups=6, group_size=3)
    with pytest.raises(ValueError):
        gen.diverse_beam_search(feats, cv, eps, BOS, EOS, diversity=-1.0)


def test_main_synthetic_inference_with_group_beam_search(tmp_path):
    """main.py --synthetic --mode inference --sample_gen diverse_beam in a fresh process (on a checkpoint written here): the JSON holds
    per image the merged captions of its groups, ranked, with the groups that produced each"""
    from vae_captioning_amd.utils.parameters import Parameters
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden, p.latent_size, p.gen_z_samples = 32, 64, 64, 10, 4
    P0 = spec.init_caption_params(p, 200, seed=3)
    os.makedirs(tmp_path / "checkpoints")
    np.savez(str(tmp_path / "checkpoints" / "gb.ckpt.npz"), **{k: (v * 3).astype(np.float32) for k, v in P0.items()})
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "200", "--embed_dim", "32",
           "--enc_hid", "64", "--dec_hid", "64", "--latent", "10", "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "gb",
           "--mode", "inference", "--sample_gen", "diverse_beam", "--beam_size", "6", "--beam_groups", "3", "--gen_name", "gb"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = json.load(open(tmp_path / "val_gb.json"))
    assert recs == json.load(open(tmp_path / "val_gb_diverse.json")) and len(recs) == 8
    for x in recs:
        n = len(x["captions"])
        assert 1 <= n <= 6 and x["caption"] == x["captions"][0] and len(x["scores"]) == len(x["counts"]) == len(x["groups"]) == n
        assert x["scores"] == sorted(x["scores"], reverse=True) and x["counts"] == [len(g) for g in x["groups"]]
        assert 3 <= sum(x["counts"]) <= 6 and all(0 <= g < 3 for gs in x["groups"] for g in gs)
