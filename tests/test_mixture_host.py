"""Marginal decoding without a GPU: the float64 reference of tests/mixture_ref.py against the chain-rule identity it rests on, its K = 1
reductions (the softmax; oracle.decode.beam_search), the command-line flags, and the C ABI's argument checks (which refuse a call before
any device work)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import decode as od
from vae_captioning_amd import abi
from vae_captioning_amd.utils.parameters import Parameters

from . import mixture_ref as mr
from .dbs_ref import model_inputs

BOS, EOS = 1, 2


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("K,V,T", [(1, 7, 5), (3, 40, 9), (20, 130, 12)])
def test_mixture_log_probabilities_sum_to_the_marginal(K, V, T):
    """Along ANY token sequence: sum_t log q_t(y_t) = logsumexp_k sum_t lsm_kt(y_t) - log K, to 1e-12."""
    rng = np.random.default_rng(K * 100 + V)
    logw, total, per_draw = np.zeros(K), 0.0, np.zeros(K)
    for _ in range(T):
        x = rng.standard_normal((K, V)) * 3.0
        y = int(rng.integers(0, V))
        tp, ti, stat, q = mr.mixture_topk(x, V, K, logw, 1)
        total += np.log(q[0, y])
        logw = mr.advance(x, V, K, None, [y], logw)[0]
        per_draw += (x[:, y] - stat[:, 0]) - stat[:, 1]
    np.testing.assert_allclose(logw, per_draw, rtol=0, atol=1e-12)
    assert abs(total - (np.logaddexp.reduce(per_draw) - np.log(K))) <= 1e-12


def test_one_draw_is_the_softmax():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 50)) * 2.5
    tp, ti, stat, q = mr.mixture_topk(x, 50, 1, -7.0 * rng.random(4), 5)
    e = np.exp(x - x.max(1, keepdims=True))
    sm = e / e.sum(1, keepdims=True)
    np.testing.assert_allclose(q, sm, rtol=1e-14, atol=0)
    assert (ti == np.argsort(-sm, axis=1, kind="stable")[:, :5]).all()
    np.testing.assert_array_equal(tp, np.take_along_axis(q, ti, 1))


def test_equal_columns_go_by_index_and_a_huge_weight_spread_leaves_one_draw():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 20))
    x[:, 11] = x[:, 4] = x.max() + 1.0                         # the same value in all K rows: the lower index first
    tp, ti, _, _ = mr.mixture_topk(x, 20, 3, np.zeros(3), 2)
    assert ti[0].tolist() == [4, 11] and tp[0, 0] == tp[0, 1]
    x = rng.standard_normal((3, 20))
    _, ti, _, q = mr.mixture_topk(x, 20, 3, np.array([-2000.0, 0.0, -2000.0]), 4)
    e = np.exp(x[1] - x[1].max())
    np.testing.assert_allclose(q[0], e / e.sum(), rtol=1e-14, atol=0)   # (the other draws' weights are exactly 0)
    assert ti[0].tolist() == np.argsort(-x[1], kind="stable")[:4].tolist()


def test_greedy_form_of_advance_leaves_done_groups_and_full_rows_alone():
    rng = np.random.default_rng(9)
    K, V, Lmax = 2, 10, 3
    x = rng.standard_normal((3 * K, V))
    logw = -rng.random(3 * K)
    done, seq, ln = np.array([0, 1, 0]), np.array([[5, 0, 0], [6, EOS, 0], [7, 8, 9]]), np.array([1, 2, 3])
    out, _, tok_rows, d2, s2, l2 = mr.advance(x, V, K, None, [EOS, 4, 3], logw, EOS, done, seq, ln)
    assert d2.tolist() == [1, 1, 0] and l2.tolist() == [2, 2, 3]
    assert s2.tolist() == [[5, EOS, 0], [6, EOS, 0], [7, 8, 9]]
    np.testing.assert_array_equal(out[2:], logw[2:])           # the done group and the group with a full row: copied through
    assert (out[:2] < logw[:2]).all() and tok_rows.tolist() == [EOS, EOS, 4, 4, 3, 3]


@pytest.mark.parametrize("kw", [dict(prior="Normal"), dict(prior="AG", use_c_v=True)], ids=["Normal", "AG-cv"])
@pytest.mark.parametrize("beam", [2, 3])
def test_reference_beam_search_with_one_draw_is_the_oracle_beam_search(kw, beam):
    p, P0, feats, cv, eps, cm = model_inputs(7, **kw)
    P64 = {k: v.astype(np.float64) for k, v in P0.items()}
    for b in range(3):
        args = (P64, p, feats[b].astype(np.float64), cv[b].astype(np.float64))
        e = eps[:, b:b + 1].astype(np.float64)
        sents, scores = od.beam_search(*args, e, BOS, EOS, c_means=cm, beam_size=beam, max_len=10)
        got_s, got_sc, _ = mr.marginal_beam_search(*args, e[None], BOS, EOS, c_means=cm, beam_size=beam, max_len=10)
        assert got_s == sents and got_sc == scores
        toks, logw, marg, _ = mr.marginal_greedy(*args, e[None], BOS, EOS, c_means=cm, max_len=10)
        assert toks == od.greedy(*args, e, BOS, EOS, c_means=cm, max_len=10) and marg == logw[0]


def test_reference_greedy_accumulates_the_marginal_of_its_caption():
    """the decoder's marginal is the chain-rule sum: re-scoring the returned tokens under every draw gives the same logw"""
    p, P0, feats, cv, _, cm = model_inputs(11, prior="Normal")
    P64 = {k: v.astype(np.float64) for k, v in P0.items()}
    K = 4
    eps = np.random.default_rng(2).standard_normal((K, p.gen_z_samples, 1, p.latent_size))
    toks, logw, marg, _ = mr.marginal_greedy(P64, p, feats[0].astype(np.float64), cv[0].astype(np.float64), eps, BOS, EOS, max_len=8)
    for k in range(K):
        state, tok, lp = od.initial_state(P64, p, feats[0].astype(np.float64), cv[0].astype(np.float64), eps[k], None, std=p.std), BOS, 0.0
        for t in toks:
            probs, state = od.step(P64, tok, state)
            lp += float(np.log(probs[t]))
            tok = t
        assert abs(lp - logw[k]) <= 1e-12
    assert abs(marg - (np.logaddexp.reduce(logw) - np.log(K))) <= 1e-12


# ------------------------------------------------------------------ flags
def test_flags_parse_and_reject():
    q = Parameters().parse_args([])
    assert q.marginal_draws == 20 and q.sample_gen == "beam_search"
    q = Parameters().parse_args(["--sample_gen", "marginal_greedy", "--marginal_draws", "4"])
    assert q.sample_gen == "marginal_greedy" and q.marginal_draws == 4
    q = Parameters().parse_args(["--sample_gen", "marginal_beam", "--marginal_draws", "256", "--beam_size", "5"])
    assert q.sample_gen == "marginal_beam" and q.marginal_draws == 256 and q.beam_size == 5
    for bad in (["--marginal_draws", "0"], ["--marginal_draws", "257"], ["--marginal_draws", "-3"],
                ["--sample_gen", "marginal_beam", "--beam_size", "17"], ["--sample_gen", "marginal_beam", "--beam_size", "0"]):
        with pytest.raises(SystemExit):
            Parameters().parse_args(bad)
    assert Parameters().parse_args(["--sample_gen", "beam_search", "--beam_size", "17"]).beam_size == 17   # (beam_search's own rule stays)


def test_inference_dispatches_the_marginal_modes():
    from vae_captioning_amd.ops.inference import _decode

    class Dec(object):
        def marginal_inference(self, sess, ids, images, placeholder, c_v):
            return [{"image_id": i, "caption": "", "marginal": 0.0, "draws": 3} for i in ids]

        def online_inference(self, sess, ids, images, placeholder, c_v=None):
            return ["online"], None

    p = Parameters()
    for mode in ("marginal_greedy", "marginal_beam"):
        p.sample_gen = mode
        assert [r["image_id"] for r in _decode(Dec(), p, None, None, [7, 8], None, None, allow_beam=True)] == [7, 8]
        assert _decode(Dec(), p, None, None, [7], None, None, allow_beam=False) == ["online"]   # the test set: online_inference, as always


# ------------------------------------------------------------------ the C ABI: exported, and bad arguments refused before device work
NEW = ["vc_mixture_topk_workspace_bytes", "vc_mixture_topk_f32", "vc_mixture_advance_f32"]
X = 4096   # a non-null pointer value: the checks must refuse the call before anything dereferences it


@pytest.fixture(scope="module")
def built():
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
    assert built.vc_mixture_topk_workspace_bytes(32, 10000, 1) == 32 * 10 * 8
    assert built.vc_mixture_topk_workspace_bytes(6, 1025, 16) == 6 * 2 * 16 * 8


@pytest.mark.parametrize("G,K,V,ld,kc,null", [(4, 0, 40, 40, 1, None), (4, 257, 40, 40, 1, None), (4, 3, 40, 39, 1, None), (4, 3, 40, 40, 0, None),
                                              (4, 3, 40, 40, 17, None), (4, 3, 8, 8, 9, None), (0, 3, 40, 40, 1, None), (4, 3, 40, 40, 1, "logw"),
                                              (4, 3, 40, 40, 1, "stat"), (4, 3, 40, 40, 1, "ws")],
                         ids=["K-0", "K-257", "ld", "kc-0", "kc-17", "kc-over-V", "no-groups", "null-logw", "null-stat", "null-ws"])
def test_topk_entry_rejects_bad_arguments(built, G, K, V, ld, kc, null):
    ptr = {n: (None if n == null else X) for n in ("logits", "logw", "top_p", "top_i", "stat", "ws")}
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_mixture_topk_f32(None, ptr["logits"], G, K, V, ld, ptr["logw"], kc, ptr["top_p"], ptr["top_i"], ptr["stat"], ptr["ws"], 1 << 30)


def test_topk_entry_rejects_a_small_workspace(built):
    with pytest.raises(abi.VaecapError, match="workspace too small"):
        built.vc_mixture_topk_f32(None, X, 4, 3, 2000, 2000, X, 5, X, X, X, X, 4 * 2 * 5 * 8 - 1)


@pytest.mark.parametrize("args", [
    (None, X, 40, 40, X, 4, 0, None, X, X, 2 * X, None, X, 2, None, None, 0, None),     # K = 0
    (None, X, 40, 40, X, 4, 257, None, X, X, 2 * X, None, X, 2, None, None, 0, None),   # K = 257
    (None, X, 40, 40, X, 4, 3, None, X, X, X, None, X, 2, None, None, 0, None),         # logw_in == logw_out
    (None, X, 40, 39, X, 4, 3, None, X, X, 2 * X, None, X, 2, None, None, 0, None),     # ld < V
    (None, X, 40, 40, X, 4, 3, None, None, X, 2 * X, None, X, 2, None, None, 0, None),  # null tok
    (None, X, 40, 40, X, 4, 3, None, X, X, 2 * X, None, None, 2, None, None, 0, None),  # null tok_rows
    (None, X, 40, 40, X, 4, 3, X, X, X, 2 * X, X, X, 2, X, X, 8, X),                    # the greedy form with a parent
    (None, X, 40, 40, X, 4, 3, None, X, X, 2 * X, None, X, 2, X, None, 8, X),           # the greedy form without seq
    (None, X, 40, 40, X, 4, 3, None, X, X, 2 * X, None, X, 2, X, X, 0, X),              # the greedy form with Lmax = 0
], ids=["K-0", "K-257", "in-place", "ld", "null-tok", "null-tok-rows", "greedy-with-parent", "greedy-without-seq", "greedy-lmax"])
def test_advance_entry_rejects_bad_arguments(built, args):
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_mixture_advance_f32(*args)
