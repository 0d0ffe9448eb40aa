"""CPU: the host end of caption scoring (generate.py: CaptionGenerator.score; csrc/score.hip) -- the new C-ABI entries and their
argument checks (which run before any device work), the size of the fused kernel's workspace (no [rows, V] logits anywhere), the new
flags, and the fp64 checker tests/score_ref.py on a case worked by hand."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from vae_captioning_amd import abi
from vae_captioning_amd.utils.parameters import Parameters

from . import score_ref as ref

NEW = ["vc_logits_logprob_f32", "vc_logits_logprob_workspace_bytes", "vc_score_reduce_f64"]
X = 4096   # a non-null pointer value: the checks must refuse the call before anything dereferences it


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return abi.load()


def test_new_entries_are_declared_exported_and_additive(built):
    protos = abi.parse_header()
    cdll = ctypes.CDLL(abi.LIB_PATH)
    for n in NEW:
        assert n in protos and hasattr(cdll, n), n
        getattr(built, n)   # binds: every argument type is one the ctypes layer knows
    assert built.vc_abi_version() == 4


def _logprob_args(**kw):
    a = dict(stream=None, rows=256, V=1000, H=64, hs=X, pitch=64, W=X, ldw=1000, bias=X, labels=X, lp=X, ws=X, ws_bytes=1 << 30)
    a.update(kw)
    return [a[k] for k in ("stream", "rows", "V", "H", "hs", "pitch", "W", "ldw", "bias", "labels", "lp", "ws", "ws_bytes")]


@pytest.mark.parametrize("kw", [dict(hs=None), dict(W=None), dict(labels=None), dict(lp=None), dict(H=48), dict(H=48, pitch=48), dict(ldw=999),
                                dict(pitch=32), dict(V=0), dict(rows=-1)],
                         ids=["null-hs", "null-W", "null-labels", "null-lp", "H-48", "H-48-pitch-48", "ldw-lt-V", "pitch-lt-H", "V-0", "rows-negative"])
def test_logits_logprob_rejects_bad_arguments_without_a_device(built, kw):
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_logits_logprob_f32(*_logprob_args(**kw))


def test_logits_logprob_reports_a_small_workspace_as_such(built):
    need = built.vc_logits_logprob_workspace_bytes(256, 1000, 64)
    for kw in (dict(ws=None), dict(ws_bytes=need - 4), dict(ws_bytes=0)):
        with pytest.raises(abi.VaecapError, match="code 10002"):
            built.vc_logits_logprob_f32(*_logprob_args(**kw))


def test_the_workspace_is_a_fiftieth_of_the_logits_it_replaces(built):
    R, V, H = 51200, 10000, 512
    need = built.vc_logits_logprob_workspace_bytes(R, V, H)
    assert 0 < need < R * V * 4 // 50, (need, R * V * 4)
    assert need >= R * (2 * 79 + 1) * 4              # a (max, sum) pair per 128-column tile and the label's logit, per row
    assert built.vc_logits_logprob_workspace_bytes(0, V, H) == 0


@pytest.mark.parametrize("kw", [dict(lp=None), dict(len=None), dict(logprob=None), dict(marginal=None), dict(K=0), dict(K=257), dict(T=-1), dict(C=-1)],
                         ids=["null-lp", "null-len", "null-logprob", "null-marginal", "K-0", "K-257", "T-negative", "C-negative"])
def test_score_reduce_rejects_bad_arguments_without_a_device(built, kw):
    a = dict(stream=None, lp=X, T=4, C=3, K=5, len=X, logprob=X, marginal=X)
    a.update(kw)
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_score_reduce_f64(*[a[k] for k in ("stream", "lp", "T", "C", "K", "len", "logprob", "marginal")])


# ------------------------------------------------------------------ flags
def test_score_flags_defaults_and_validation():
    q = Parameters().parse_args([])
    assert q.diverse_rerank == "likelihood" and q.score_draws == 0 and Parameters().score_draws == 0
    p = Parameters().parse_args(["--sample_gen", "diverse", "--diverse_rerank", "marginal", "--score_draws", "7"])
    assert p.diverse_rerank == "marginal" and p.score_draws == 7 and isinstance(p.score_draws, int)
    for bad in (["--score_draws", "257"], ["--score_draws", "-1"], ["--diverse_rerank", "cider"], ["--diverse_method", "beam"]):
        with pytest.raises(SystemExit):
            Parameters().parse_args(bad)
    assert Parameters().parse_args(["--score_draws", "256"]).score_draws == 256


# ------------------------------------------------------------------ the checker, by hand
def test_the_checker_on_a_case_worked_by_hand():
    # one caption of three tokens over a 4-word vocabulary, two draws with given per-step distributions:
    # draw 0 gives the tokens 0.5, 0.25, 0.8 (product 0.1), draw 1 gives them 0.2, 0.5, 0.4 (product 0.04)
    toks = [3, 0, 2]
    d0 = [[0.1, 0.2, 0.2, 0.5], [0.25, 0.25, 0.25, 0.25], [0.05, 0.05, 0.8, 0.1]]
    d1 = [[0.3, 0.3, 0.2, 0.2], [0.5, 0.1, 0.2, 0.2], [0.2, 0.2, 0.4, 0.2]]
    lp = [ref.logprob_from_step_probs(d0, toks), ref.logprob_from_step_probs(d1, toks)]
    assert abs(lp[0] - math.log(0.1)) < 1e-12 and abs(lp[1] - math.log(0.04)) < 1e-12
    m = ref.marginal(lp)
    assert abs(m - math.log(0.07)) < 1e-12                     # 1/2 (0.1 + 0.04)
    assert abs(ref.perplexity([m], [3]) - 0.07 ** (-1.0 / 3.0)) < 1e-12
    assert abs(ref.marginal([-1000.0, -1000.0]) + 1000.0) < 1e-12   # max-shifted: no underflow
    assert abs(ref.marginal([lp[0]]) - lp[0]) < 1e-12
    assert ref.strip_bos([1, 5, 2], 1) == [5, 2] and ref.strip_bos([5, 2], 1) == [5, 2] and ref.strip_bos([], 1) == []


def test_the_rerank_rule_puts_ended_captions_first_and_keeps_the_order_of_ties():
    EOS = 2
    entries = [([5, 6, 2], -1.0, 3), ([7, 8, 9], -1.5, 1), ([5, 2], -2.0, 2), ([9, 9, 2], -2.5, 1), ([4, 4, 2], -3.0, 1)]
    marg = [-4.0, -0.5, -3.0, -2.0, -2.0]
    got = ref.rerank_rule(entries, marg, EOS, len_norm_f=0.7)
    # the cut caption [7, 8, 9] has the best marginal and still goes last; [9, 9, 2] and [4, 4, 2] tie exactly and keep their order
    assert [t for t, _, _, _ in got] == [[9, 9, 2], [4, 4, 2], [5, 2], [5, 6, 2], [7, 8, 9]]
    assert [n for _, _, n, _ in got] == [1, 1, 2, 3, 1] and [m for _, _, _, m in got] == [-2.0, -2.0, -3.0, -4.0, -0.5]
    np.testing.assert_allclose([s for _, s, _, _ in got], [-2.0 / 4 ** 0.7, -2.0 / 4 ** 0.7, -3.0 / 3 ** 0.7, -4.0 / 4 ** 0.7, -0.5 / 4 ** 0.7], rtol=1e-15)
    from vae_captioning_amd.generate import rerank_by_marginal
    assert rerank_by_marginal(entries, marg, EOS, 0.7) == got     # the product's host rule is the same rule


# ------------------------------------------------------------------ score()'s own argument errors (raised before any device work)
def _gen():
    from vae_captioning_amd.generate import CaptionGenerator
    p = types.SimpleNamespace(gen_z_samples=4, latent_size=10, gen_max_len=12, decoder_hidden=64)
    return CaptionGenerator(types.SimpleNamespace(p=p, lib=None, V=40))


def test_score_argument_errors_name_the_image_and_the_caption():
    g = _gen()
    feats = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="draws"):
        g.score(feats, [[], []], draws=0)
    with pytest.raises(ValueError, match="draws"):
        g.score(feats, [[], []], draws=257)
    with pytest.raises(ValueError, match="eps"):
        g.score(feats, [[], []], eps=np.zeros((3, 4, 3, 10), np.float32), draws=3)
    with pytest.raises(ValueError, match="image 1 caption 0"):
        g.score(feats, [[[5, 2]], [[5, 40, 2]]], draws=2)
    with pytest.raises(ValueError, match="image 0 caption 1"):
        g.score(feats, [[[5, 2], [1] + [3] * 257], []], draws=2)
    with pytest.raises(ValueError, match="one list of captions per image"):
        g.score(feats, [[]], draws=2)
    with pytest.raises(ValueError, match="rerank"):
        g.diverse(feats, draws=2, rerank="cider")
    # nothing to score: no device work at all
    out = g.score(feats, [[[]], []], draws=3)
    assert out[1] == [] and out[0][0]["tokens"] == 0 and out[0][0]["marginal"] == 0.0 and out[0][0]["logprob"].tolist() == [0.0, 0.0, 0.0]
    assert g.score_rows * 8 * 64 * 4 <= 1 << 30


def test_human_captions_and_perplexity_of_the_inference_driver():
    from vae_captioning_amd.ops.inference import human_captions, perplexity
    lab = np.array([[[5, 6, 2, 0], [7, 2, 0, 0]], [[8, 9, 9, 2], [0, 0, 0, 0]]], np.int32)
    lens = np.array([[3, 2], [4, 0]], np.int32)
    assert human_captions((None, lab), lens) == [[[5, 6, 2], [7, 2]], [[8, 9, 9, 2]]]
    assert human_captions((None, lab[:, 0]), lens[:, 0]) == [[[5, 6, 2]], [[8, 9, 9, 2]]]
    recs = [{"image_id": 1, "captions": [{"tokens": 3, "marginal": -3.0, "logprob": -3.5}, {"tokens": 2, "marginal": -1.0, "logprob": -1.0}]},
            {"image_id": 2, "captions": [{"tokens": 5, "marginal": -6.0, "logprob": -7.0}]}]
    assert abs(perplexity(recs) - math.exp(1.0)) < 1e-12
    assert abs(perplexity(recs) - ref.perplexity([-3.0, -1.0, -6.0], [3, 2, 5])) < 1e-12
