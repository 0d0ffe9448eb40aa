"""Host half of in-set CIDEr-D (vae_captioning_amd/mbr.py): Self-CIDEr on matrices worked by hand and against tests/gram_ref.py,
the chunking of images, the re-ranking rule on a fake matrix pass, the flags, the decoder's guard and the metrics file."""
import contextlib
import io
import json
import math
import os
import types

import numpy as np
import pytest

from vae_captioning_amd import mbr
from vae_captioning_amd.utils.parameters import Parameters

from . import consensus_ref as cref
from . import gram_ref
from . import inference_fakes as fakes

BOS, EOS = 1, 2


# ------------------------------------------------------------------ Self-CIDEr
@pytest.mark.parametrize("m", [2, 3, 7, 20, 256])
def test_self_cider_of_known_matrices(m):
    assert abs(mbr.self_cider(10.0 * np.eye(m)) - 1.0) <= 1e-15          # m captions that share no n-gram: m equal eigenvalues
    assert mbr.self_cider(np.full((m, m), 10.0)) == 0.0                  # m identical captions: one eigenvalue m / 2, m - 1 zeros (what
    assert mbr.self_cider(np.full((m, m), np.float32(7.3))) == 0.0       # eigvalsh returns for them is O(1e-16), and cut as a zero)
    assert mbr.self_cider(np.zeros((m, m))) == 0.0                       # captions without words


def test_self_cider_edges():
    assert mbr.self_cider(np.array([[10.0]])) == 0.0 and mbr.self_cider(np.array([[0.0]])) == 0.0
    assert math.isnan(mbr.self_cider(np.zeros((0, 0))))
    # S = [[1, 2], [2, 1]] has eigenvalues 3 and -1 (after / 20 of 10x: 1.5 and -0.5); the negative one is clamped: r = 1
    assert mbr.self_cider(np.array([[10.0, 20.0], [20.0, 10.0]])) == 0.0
    A = np.array([[10.0, 8.0, 0.5], [2.0, 10.0, 3.0], [1.5, 1.0, 10.0]])
    assert mbr.self_cider(A) == mbr.self_cider((A + A.T) / 2)             # only the symmetric part counts
    assert 0.0 < mbr.self_cider(A) < 1.0
    assert isinstance(mbr.self_cider(A.astype(np.float32)), float)


def _related_caps(rng, n, vocab=30):
    base = rng.integers(3, vocab, size=12)
    out = []
    for _ in range(n):
        c = np.where(rng.random(12) < 0.3, rng.integers(3, vocab, size=12), base)[:rng.integers(5, 13)]
        out.append([BOS] + c.tolist() + [EOS])
    return out


def test_self_cider_against_the_reference_on_reference_grams():
    """both sides apply one float64 formula to the same float64 input"""
    rng = np.random.default_rng(3)
    corpus = [_related_caps(rng, 4) for _ in range(25)]
    idf, unseen = cref.df_idf(corpus, BOS, EOS)
    seen = []
    for n in (2, 3, 8, 20):
        G = gram_ref.gram(_related_caps(rng, n), idf, unseen)
        np.testing.assert_allclose(mbr.self_cider(G), gram_ref.self_cider(G), rtol=1e-12, atol=0)
        seen.append(mbr.self_cider(G))
    assert all(0.0 < s < 1.0 for s in seen)


# ------------------------------------------------------------------ chunks
def test_chunks_cover_the_images_in_order_within_the_block():
    per = [0, 1, 5, 256, 0, 64, 65, 2, 4]
    for block in (1, 4 * 8 * 8, 4 * 100 * 256, 4 * 256 * 256, 1 << 40):
        parts = mbr.chunks(per, block)
        assert [p[0] for p in parts] == [0] + [p[1] for p in parts[:-1]] and parts[-1][1] == len(per)
        for b0, b1, ld in parts:
            assert b1 > b0 and ld % 4 == 0 and ld == (max(per[b0:b1]) + 3) // 4 * 4
            assert b1 - b0 == 1 or sum(per[b0:b1]) * ld * 4 <= block
    assert len(mbr.chunks(per, 1)) == len(per) and len(mbr.chunks(per, 1 << 40)) == 1 and mbr.chunks([], 1) == []
    assert mbr.GRAM_BLOCK_BYTES == 256 << 20


# ------------------------------------------------------------------ rerank
class _FakeGram(mbr.CiderGram):
    def __init__(self, table):
        self.table, self.calls = table, []

    def gram(self, candidates_per_image, weights=None):
        self.calls.append((candidates_per_image, weights))
        G = [np.array([[self.table[tuple(a)][tuple(b)] for b in cs] for a in cs], np.float64).reshape(len(cs), len(cs)) for cs in candidates_per_image]
        return G, [gram_ref.mbr(g, w) for g, w in zip(G, weights)]


def test_rerank_orders_by_mbr_with_counts_as_weights():
    a, b, c, d = [3, 4, EOS], [5, EOS], [6, 7, EOS], [8, EOS]
    row = lambda *v: dict(zip(map(tuple, (a, b, c, d)), v))
    table = {tuple(a): row(10, 0, 0, 0), tuple(b): row(0, 10, 4, 0), tuple(c): row(0, 4, 10, 0), tuple(d): row(0, 0, 0, 10)}
    entries = [(a, -0.1, 3), (b, -0.2, 1), (c, -0.3, 2), (d, -0.4, 3)]
    g = _FakeGram(table)
    (out,), = [g.rerank([entries])]
    # counts 3 1 2 3 of 9: a 30/9, b (10 + 8)/9, c (4 + 20)/9, d 30/9 -- a and d tie exactly and keep the likelihood order
    assert [e[0] for e in out] == [a, d, c, b]
    assert [e[3] for e in out] == [30 / 9, 30 / 9, 24 / 9, 18 / 9] and all(e[:3] == entries[[0, 3, 2, 1][i]] for i, e in enumerate(out))
    assert g.calls[0][1] == [[3.0, 1.0, 2.0, 3.0]] and g.calls[0][0] == [[a, b, c, d]]
    assert g.rerank([entries], n_best=2)[0] == out[:2]                      # the cut comes after the ranking
    # given weights replace the counts: all the evidence on c
    top = g.rerank([entries, []], weights=[[0, 0, 1, 0], []])
    assert [e[0] for e in top[0]] == [c, b, a, d] and [e[3] for e in top[0]] == [10.0, 4.0, 0.0, 0.0] and top[1] == []
    uniform = g.rerank([entries], weights=[[1, 1, 1, 1]])[0]
    assert [e[0] for e in uniform] == [b, c, a, d]                          # 14/4 14/4 10/4 10/4: two exact ties in likelihood order


def test_gram_checks_its_limits_before_any_device_work():
    g = _FakeGram({})
    g.bos, g.eos = BOS, EOS        # (no library, no device: a check that got past would fail on the missing attributes)
    with pytest.raises(ValueError, match=r"at most 256 candidates per image \(DIVERSE_MAX_DRAWS; got 257\)"):
        mbr.CiderGram.gram(g, [[[3, EOS]] * 257])
    with pytest.raises(ValueError, match="candidate 1 of image 1 has 65 words"):
        mbr.CiderGram.gram(g, [[[3]], [[3], [4] * 65]])
    with pytest.raises(ValueError, match="token id 65536 outside 1..65535"):
        mbr.CiderGram.gram(g, [[[3, 65536]]])
    with pytest.raises(ValueError, match="one number per caption"):
        mbr.CiderGram.gram(g, [[[3]], [[4], [5]]], weights=[[1.0], [1.0]])


# ------------------------------------------------------------------ flags, the decoder's guard
def test_flags():
    q = Parameters().parse_args([])
    assert q.diverse_rerank == "likelihood" and q.eval_self_cider is False and Parameters().eval_self_cider is False
    p = Parameters().parse_args(["--sample_gen", "diverse", "--diverse_rerank", "mbr"])
    assert p.diverse_rerank == "mbr" and p.eval_self_cider is False
    p = Parameters().parse_args(["--mode", "inference", "--eval_captions", "--eval_self_cider"])
    assert p.eval_captions is True and p.eval_self_cider is True
    for bad in (["--diverse_rerank", "cider"], ["--diverse_rerank", "MBR"], ["--eval_self_cider"], ["--mode", "inference", "--eval_self_cider"]):
        with pytest.raises(SystemExit):
            Parameters().parse_args(bad)
    assert "mbr" in Parameters().build_parser().format_help()


def test_the_decoder_refuses_mbr_without_a_cider_gram():
    from vae_captioning_amd.vae_model.decoder import Decoder
    me = types.SimpleNamespace(params=types.SimpleNamespace(diverse_rerank="mbr"), consensus_index=None, mbr=None)
    with pytest.raises(RuntimeError, match=r"mbr\.CiderGram"):
        Decoder._rerank(me)
    me.mbr = object()
    assert Decoder._rerank(me) == "mbr"
    me.params.diverse_rerank = "likelihood"
    me.mbr = None
    assert Decoder._rerank(me) == "likelihood"


# ------------------------------------------------------------------ the metrics file
class _Evaluator(object):
    def __init__(self, log):
        self.log = log

    def evaluate(self, candidates, **kw):
        from vae_captioning_amd.evaluate import METRICS, SET_METRICS
        self.log.append(kw)
        out = {k: 0.125 * (i + 1) for i, k in enumerate(METRICS)}
        out["novel"] = None
        out["per_image"] = dict(captions=np.ones(len(candidates)))
        if kw.get("self_cider"):
            out.update({k: 0.0625 * (i + 1) for i, k in enumerate(SET_METRICS)})
        return out


class _Decoder(object):
    def __init__(self, log):
        self.log = log

    def caption_evaluator(self, references):
        return _Evaluator(self.log)


def _store(tmp, flag):
    from vae_captioning_amd.ops.inference import evaluate_decoded
    params = fakes.Params(use_c_v=False, prior="Normal", sample_gen="greedy")
    params.eval_captions = True
    if flag is not None:
        params.eval_self_cider = flag
    log, cwd, buf = [], os.getcwd(), io.StringIO()
    os.makedirs(tmp)
    os.chdir(tmp)
    try:
        with contextlib.redirect_stdout(buf):
            evaluate_decoded(params, _Decoder(log), [[[3, EOS]], [[4, EOS]]], [[[3, EOS]], [[5, EOS], [4, EOS]]])
        return open("val_%s_metrics.json" % params.gen_name, "rb").read(), log, buf.getvalue()
    finally:
        os.chdir(cwd)


def test_the_metrics_file_gains_the_two_numbers_only_with_the_flag(tmp_path):
    from vae_captioning_amd.evaluate import METRICS, SET_METRICS
    assert SET_METRICS == ("self_cider", "mbr_cider_d") and not set(SET_METRICS) & set(METRICS)
    plain, log0, out0 = _store(str(tmp_path / "plain"), None)      # params that never heard of the flag
    off, log1, out1 = _store(str(tmp_path / "off"), False)
    on, log2, out2 = _store(str(tmp_path / "on"), True)
    assert plain == off and out0 == out1 and log0 == log1 == [{}]   # evaluate(decoded), as before: no keyword at all
    assert log2 == [{"self_cider": True}]
    m0, m = json.loads(off), json.loads(on)
    assert not set(SET_METRICS) & set(m0) and "eval_self_cider" not in m0
    assert m["self_cider"] == 0.0625 and m["mbr_cider_d"] == 0.125 and m["eval_self_cider"] is True
    assert {k: v for k, v in m.items() if k not in SET_METRICS + ("eval_self_cider",)} == m0
    assert "self_cider" not in out1 and "mbr_cider_d" not in out1
    assert "\nself_cider: 0.062500\nmbr_cider_d: 0.125000\n" in out2
    assert [l for l in out2.splitlines() if not l.startswith(SET_METRICS)] == out1.splitlines()
