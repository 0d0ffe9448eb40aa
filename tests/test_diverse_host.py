"""CPU: the host end of diverse captioning (K latent draws per image, ranked distinct captions).

`rank_rule` below is the numpy statement of the merge / rank contract that `vc_diverse_rank` implements on the device and the GPU
tests check against: score = logprob / (1 + n_tokens)**len_norm_f (the 1 counts <BOS>, vae_model/decoder.py:285-286); candidates
with identical token sequences merge into one entry (best score and its draw kept, equal scores: the lower draw; count = number of
draws); <EOS>-ended captions before captions cut at max_len (decoder.py:296-299 never mixes complete and partial), then score
descending, then lower draw.  Here it is checked on hand-made candidate sets, and `generate.diverse_from_host` (the parser of the
flat result buffers) against it.  Also: the new flags, the new C-ABI entries' argument checks (which run before any device work),
and diverse()'s own argument errors."""
import ctypes
import types

import numpy as np
import pytest

from vae_captioning_amd import abi
from vae_captioning_amd.generate import CaptionGenerator, diverse_fields, diverse_from_host
from vae_captioning_amd.utils.parameters import Parameters


def rank_rule(tokens, logprob, ended, len_norm_f=0.7):
    """One image's K candidates (token lists, float64 log-likelihoods, <EOS> flags) -> [(tokens, score, count, draw), ...] ranked."""
    K = len(tokens)
    score = [float(logprob[k]) / (1.0 + len(tokens[k])) ** len_norm_f for k in range(K)]
    groups = {}
    for k in range(K):
        groups.setdefault(tuple(int(t) for t in tokens[k]), []).append(k)
    entries = []
    for key, ks in groups.items():
        best = min(ks, key=lambda k: (-score[k], k))
        entries.append((list(key), score[best], len(ks), best, bool(ended[best])))
    entries.sort(key=lambda t: (not t[4], -t[1], t[3]))
    return [(t, s, c, d) for t, s, c, d, _ in entries]


def test_rule_merges_duplicates_keeping_the_best_score_and_its_draw():
    toks = [[5, 6, 2], [7, 2], [5, 6, 2], [5, 6, 2]]
    lp = [-3.0, -2.5, -1.0, -2.0]
    got = rank_rule(toks, lp, [1, 1, 1, 1])
    assert [(t, c, d) for t, _, c, d in got] == [([5, 6, 2], 3, 2), ([7, 2], 1, 1)]
    assert got[0][1] == -1.0 / 4 ** 0.7 and got[1][1] == -2.5 / 3 ** 0.7


def test_rule_equal_scores_go_to_the_lower_draw():
    toks = [[9, 2], [8, 2], [9, 2], [8, 2]]
    lp = [-1.0, -1.0, -1.0, -1.0]   # every score equal
    got = rank_rule(toks, lp, [1] * 4)
    assert [(t, c, d) for t, _, c, d in got] == [([9, 2], 2, 0), ([8, 2], 2, 1)]


def test_rule_ended_captions_rank_before_cut_ones():
    toks = [[4, 4, 4], [3, 2], [5, 5, 5], [6, 6, 2]]
    lp = [-0.1, -9.0, -0.2, -5.0]   # the cut captions score far better
    got = rank_rule(toks, lp, [0, 1, 0, 1])
    assert [d for *_, d in got] == [3, 1, 0, 2]   # ended: -5 / 4**0.7 before -9 / 3**0.7; then the cut ones by score


def test_rule_one_draw_and_one_distinct_caption():
    assert rank_rule([[7, 2]], [-0.5], [1]) == [([7, 2], -0.5 / 3 ** 0.7, 1, 0)]
    got = rank_rule([[7, 8, 2]] * 6, [-2.0, -1.0, -1.0, -3.0, -0.5, -0.5], [1] * 6)
    assert len(got) == 1 and got[0][2] == 6 and got[0][3] == 4


def test_rule_length_normalisation_counts_bos():
    got = rank_rule([[1, 2], [1, 1, 1, 1, 2]], [-2.0, -2.6], [1, 1], len_norm_f=0.7)
    assert got[0][3] == 1   # -2.6 / 6**0.7 = -0.74 beats -2.0 / 3**0.7 = -0.93


# ------------------------------------------------------------------ the flat result buffers
def _buffers(rng, B, K, L, cases):
    """Result buffers as vc_diverse_rank leaves them, built from rank_rule on `cases` (per image: tokens, logprob, ended); junk in every
    position that must not be read."""
    M = B * K
    fields = diverse_fields(B, K, L)
    io, o = {}, 0
    for name, n in fields:
        io[name] = o
        o += n
    ints = rng.integers(3, 5000, size=o).astype(np.int32)
    dbls = rng.standard_normal(2 * M)
    f = lambda name, n: ints[io[name]:io[name] + n]
    want = []
    for b, (toks, lp, en) in enumerate(cases):
        ranked = rank_rule(toks, lp, en)
        want.append(ranked)
        f("n_distinct", B)[b] = len(ranked)
        for j, (t, sc, c, d) in enumerate(ranked):
            f("rep", M)[b * K + j] = d
            f("count", M)[b * K + j] = c
            dbls[b * K + j] = sc
        for k in range(K):
            r = b * K + k
            f("len", M)[r] = len(toks[k])
            f("ended", M)[r] = en[k]
            ints[io["seq"] + r * L:io["seq"] + r * L + len(toks[k])] = toks[k]
            dbls[M + r] = lp[k]
    return ints, dbls, io, want


def _random_case(rng, K, L):
    pool = [list(rng.integers(3, 30, size=rng.integers(1, L))) + [2] for _ in range(max(1, K // 2))] + [list(rng.integers(3, 30, size=L))]
    toks = [pool[rng.integers(0, len(pool))] for _ in range(K)]
    lp = rng.choice(np.array([-1.5, -2.0, -2.0, -4.25]), size=K)   # few values: equal scores within groups and across
    en = [int(t[-1] == 2) for t in toks]
    return toks, lp, en


@pytest.mark.parametrize("B,K,L", [(1, 1, 4), (3, 5, 6), (4, 16, 8), (2, 64, 12)])
def test_result_buffers_become_the_rule_lists(B, K, L):
    rng = np.random.default_rng(B * 100 + K)
    cases = [_random_case(rng, K, L) for _ in range(B)]
    ints, dbls, io, want = _buffers(rng, B, K, L, cases)
    res, cands = diverse_from_host(ints, dbls, io, B, K, L, candidates=True)
    assert res == [[(t, sc, c) for t, sc, c, _ in w] for w in want]
    for b, (toks, lp, en) in enumerate(cases):
        assert cands[b] == [(list(toks[k]), float(lp[k]), bool(en[k])) for k in range(K)]
    top = diverse_from_host(ints, dbls, io, B, K, L, n_best=1)
    assert top == [r[:1] for r in res]


# ------------------------------------------------------------------ flags
def test_new_flags_parse_and_cast():
    p = Parameters().parse_args(["--sample_gen", "diverse", "--diverse_draws", "7", "--diverse_method", "sample"])
    assert p.sample_gen == "diverse" and p.diverse_draws == 7 and isinstance(p.diverse_draws, int) and p.diverse_method == "sample"
    q = Parameters().parse_args([])
    assert q.diverse_draws == 20 and q.diverse_method == "greedy" and q.sample_gen == "beam_search" and q.gen_z_samples == 100
    with pytest.raises(SystemExit):
        Parameters().parse_args(["--diverse_method", "beam"])


# ------------------------------------------------------------------ the C ABI: exported, and bad arguments refused before device work
NEW = ["vc_diverse_latent_f32", "vc_decode_pick_f32", "vc_decode_round_end_i32", "vc_diverse_rank"]


@pytest.fixture(scope="module")
def built():
    import os
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return abi.load()


def test_new_entries_are_declared_and_exported(built):
    protos = abi.parse_header()
    cdll = ctypes.CDLL(abi.LIB_PATH)
    for n in NEW:
        assert n in protos and hasattr(cdll, n), n
    assert built.vc_abi_version() == 4


X = 4096   # a non-null pointer value: the checks must refuse the call before anything dereferences it


@pytest.mark.parametrize("args", [
    (None, 10, 5, 3, 4, None, 0.1, None, 1, 0, None, None),        # null z
    (None, 10, 3, 3, 4, None, 0.1, None, 1, 0, None, X),           # rows not a multiple of K
    (None, 0, 1, 3, 4, None, 0.1, None, 1, 0, None, X),            # no rows
    (None, 10, 5, 0, 4, None, 0.1, None, 1, 0, None, X),           # S = 0
], ids=["null-z", "rows-not-BK", "no-rows", "no-samples"])
def test_latent_entry_rejects_bad_arguments(built, args):
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_diverse_latent_f32(*args)


@pytest.mark.parametrize("args", [
    (None, None, 4, 40, 40, 1.0, None, 0, None, 2, X, X, X, 8, X, X),   # null logits
    (None, X, 4, 40, 40, 1.0, None, 0, None, 2, X, None, X, 8, X, X),   # null done
    (None, X, 4, 40, 39, 1.0, None, 0, None, 2, X, X, X, 8, X, X),      # ld < V
    (None, X, 4, 40, 40, 1.0, None, 0, None, 2, X, X, X, 0, X, X),      # Lmax = 0
    (None, X, 4, 40, 40, 0.0, X, 8, None, 2, X, X, X, 8, X, X),         # sampling at temperature 0
    (None, X, 4, 40, 40, 1.0, X, 0, None, 2, X, X, X, 8, X, X),         # sampling without uniform rounds
], ids=["null-logits", "null-done", "ld", "lmax", "temperature", "u-rounds"])
def test_pick_entry_rejects_bad_arguments(built, args):
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_decode_pick_f32(*args)


def test_round_end_entry_rejects_bad_arguments(built):
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_decode_round_end_i32(None, None, 4, X, None)
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_decode_round_end_i32(None, X, 0, X, None)


@pytest.mark.parametrize("rows,B,K,Lmax,null", [(257 * 2, 2, 257, 8, None), (30, 3, 10, 8, "seq"), (31, 3, 10, 8, None), (20, 2, 10, 0, None),
                                                (0, 0, 1, 8, None), (12, 3, 4, 8, "score")],
                         ids=["K-over-256", "null-seq", "rows-not-BK", "lmax", "no-images", "null-score"])
def test_rank_entry_rejects_bad_arguments(built, rows, B, K, Lmax, null):
    ptr = {n: (None if n == null else X) for n in ("seq", "len", "ended", "logprob", "nd", "rep", "count", "score")}
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_diverse_rank(None, rows, B, K, Lmax, ptr["seq"], ptr["len"], ptr["ended"], ptr["logprob"], 0.7, ptr["nd"], ptr["rep"],
                              ptr["count"], ptr["score"])


# ------------------------------------------------------------------ diverse(): argument errors before any device work
def _gen():
    p = Parameters()
    p.gen_z_samples, p.latent_size = 4, 10
    return CaptionGenerator(types.SimpleNamespace(p=p, lib=None))


@pytest.mark.parametrize("draws", [0, 257, 1000])
def test_diverse_rejects_draw_counts_outside_1_to_256(draws):
    with pytest.raises(ValueError, match="draws"):
        _gen().diverse(np.zeros((2, 8), np.float32), draws=draws)


def test_diverse_rejects_unknown_methods_and_misshapen_noise():
    g = _gen()
    with pytest.raises(ValueError, match="method"):
        g.diverse(np.zeros((2, 8), np.float32), draws=3, method="beam_search")
    with pytest.raises(ValueError, match="eps"):
        g.diverse(np.zeros((2, 8), np.float32), draws=3, eps=np.zeros((3, 4, 3, 10), np.float32))
    with pytest.raises(ValueError, match="uniforms"):
        g.diverse(np.zeros((2, 8), np.float32), draws=3, method="sample", max_len=5, uniforms=np.zeros((3, 4, 2), np.float32))
