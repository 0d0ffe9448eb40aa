"""CaptionGenerator's launch trace against the recorded one (tests/golden/decode_launch_trace.json, made with tests/launch_trace.py's
recorder on the commit before generate.py's decoders were put through shared helpers): for every decode mode, every library launch of
two identical calls on a fresh generator -- the eager rounds and the captures of the first, the replays and the ragged tail of the
second -- keeps its entry, its scalar arguments, its null / non-null pointers, its stream and its place among the stream waits, event
records, captures and replays.  torch's own copy_ / fill_ / zero_ are not seen here: the output-equality tests of each mode cover them.

The model is tests/test_gpu_generate.py's (V = 40, six images, H = 64) with the AG prior and cluster vectors unless a case says
otherwise; the greedy family runs max_len 5 and the beam family max_len 6 (five rounds) in chunks of 2: two whole chunks and one
ragged round."""
import json
import os

import numpy as np
import pytest

from vae_captioning_amd import spec
from vae_captioning_amd.controls import DecodeControls

from . import launch_trace
from .test_gpu_generate import BOS, EOS, setup

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_launch_trace.json")
K = 3                                   # draws
AG = dict(prior="AG", use_c_v=True)
NOENC = dict(no_encoder=True)
CTL = dict(no_repeat_ngram=2, min_len=2, banned=(20,))
GREEDY, BEAM = dict(max_len=5, check_every=2), dict(max_len=6, check_every=2)
CONSTRAINTS = [[[5, 6], [7]], [], [[8], [9, 10, 11]], [], [[12, 13], [14]], []]
CAPTIONS = [[[5, 6, 7, EOS], [BOS, 8, 9, 10, 11, 12, EOS]], [[13, EOS], [14, 15, 16]], [], [[17, 18, 19, 21, EOS], [22]],
            [[23, 24, EOS], [25, 26, 27, 28]], []]   # (the AG model's last image has no cluster vector: no posterior)
SCORED = CAPTIONS[:2] + [[]] + CAPTIONS[3:5] + [CAPTIONS[0]]   # two captions of different lengths per image, one image with none


def _greedy(g, x, **kw):
    return g.greedy(x.feats, x.cv, x.eps, BOS, EOS, **GREEDY, **kw)


def _sample(g, x, **kw):
    return g.sample(x.feats, x.cv, x.eps, BOS, EOS, uniforms=x.u, **GREEDY, **kw)


def _diverse(g, x, **kw):
    if kw.get("method") == "sample":
        kw["uniforms"] = x.uK
    return g.diverse(x.feats, x.cv, x.epsK, BOS, EOS, draws=K, **GREEDY, **kw)


def _posterior(fn):
    def call(g, x):
        count = sum(len(c) for c in CAPTIONS)
        gmm = (np.arange(count, dtype=np.int32) * 7) % 90 if x.p.prior == "GMM" else None
        if fn == "encode":
            return g.encode(x.feats, CAPTIONS, x.cv, gmm, BOS)
        eps = x.rng.standard_normal((K, x.p.gen_z_samples, count, x.p.latent_size)).astype(np.float32)
        return g.bound(x.feats, CAPTIONS, x.cv, eps, gmm, BOS, EOS, draws=K)
    return call


def _beam(g, x, **kw):
    return g.beam_search(x.feats, x.cv, x.eps, BOS, EOS, **dict(dict(BEAM, beam_size=2), **kw))


def _sliced(g, x):
    g.slice_rows = 1   # (six images run as 2 x 3, as in test_sliced_beam_search_on_streams_returns_the_single_slice_beams)
    return _beam(g, x)


def _constrained(g, x, **kw):
    return g.constrained_beam_search(x.feats, CONSTRAINTS, x.cv, x.eps, BOS, EOS, beam_size=2, **BEAM, **kw)


def _stochastic(g, x, **kw):
    return g.stochastic_beam_search(x.feats, x.cv, x.eps, BOS, EOS, beam_size=3, seed=7, **BEAM, **kw)


ctl = lambda: DecodeControls(**CTL)
# case -> (model, environment, call(generator, inputs))
CASES = {
    "greedy": (AG, {}, _greedy),
    "greedy_no_encoder": (NOENC, {}, _greedy),
    "greedy_controls": (AG, {}, lambda g, x: _greedy(g, x, controls=ctl())),
    "sample": (AG, {}, _sample),
    "sample_truncated": (AG, {}, lambda g, x: _sample(g, x, top_k=5, top_p=0.9)),
    "sample_controls": (AG, {}, lambda g, x: _sample(g, x, controls=ctl())),
    "diverse_greedy": (AG, {}, _diverse),
    "diverse_sample_truncated_controls": (AG, {}, lambda g, x: _diverse(g, x, method="sample", top_k=5, top_p=0.9, controls=ctl())),
    "diverse_rerank_marginal": (AG, {}, lambda g, x: _diverse(g, x, rerank="marginal")),
    "diverse_greedy_no_encoder": (NOENC, {}, _diverse),
    "score": (AG, {}, lambda g, x: g.score(x.feats, SCORED, x.cv, x.epsK, BOS, EOS, draws=K)),
    "encode_normal": (dict(prior="Normal"), {}, _posterior("encode")),
    "encode_ag": (AG, {}, _posterior("encode")),
    "encode_gmm": (dict(prior="GMM"), {}, _posterior("encode")),
    "bound_normal": (dict(prior="Normal"), {}, _posterior("bound")),
    "bound_ag": (AG, {}, _posterior("bound")),
    "bound_gmm": (dict(prior="GMM"), {}, _posterior("bound")),
    "marginal_greedy": (AG, {}, lambda g, x: g.marginal_greedy(x.feats, x.cv, x.epsK, BOS, EOS, draws=K, **GREEDY)),
    "marginal_beam": (AG, {}, lambda g, x: g.marginal_beam_search(x.feats, x.cv, x.epsK, BOS, EOS, draws=K, beam_size=2, **BEAM)),
    "beam_2": (AG, {}, _beam),
    "beam_9_not_fused": (AG, {}, lambda g, x: _beam(g, x, beam_size=9)),
    "beam_2_controls": (AG, {}, lambda g, x: _beam(g, x, controls=ctl())),
    "beam_2_xproj_off": (AG, {"VC_DECODE_XPROJ": "0"}, _beam),
    "beam_2_graph_off": (AG, {"VC_DECODE_GRAPH": "0"}, _beam),
    "beam_2_sliced": (AG, {"VC_DECODE_SLICES": "2"}, _sliced),
    "diverse_beam": (AG, {}, lambda g, x: g.diverse_beam_search(x.feats, x.cv, x.eps, BOS, EOS, groups=3, group_size=2, diversity=0.5, **BEAM)),
    "constrained_beam": (AG, {}, _constrained),
    "constrained_beam_controls": (AG, {}, lambda g, x: _constrained(g, x, controls=ctl())),
    "stochastic_beam": (AG, {}, _stochastic),
    "stochastic_beam_controls": (AG, {}, lambda g, x: _stochastic(g, x, controls=ctl())),
}


class Inputs(object):
    pass


def trace_case(lib, case, setenv):
    """The launch trace of two identical calls of `case` on a fresh engine and generator, every draw injected.  setenv(name, value) sets
    an environment variable for the duration of the caller's test."""
    import torch
    model, env, call = CASES[case]
    for k, v in env.items():
        setenv(k, v)
    x = Inputs()
    x.p, eng, gen, _, x.feats, cv, x.eps, _ = setup(lib, 13, **model)
    x.cv = cv if spec.uses_ci(x.p) else None
    x.rng = np.random.default_rng(17)
    B, S, L, T = x.feats.shape[0], x.p.gen_z_samples, x.p.latent_size, GREEDY["max_len"]
    x.epsK = x.rng.standard_normal((K, S, B, L)).astype(np.float32)
    x.uK = x.rng.random((K, T, B)).astype(np.float32)
    x.u = x.uK[0]
    state = x.rng.bit_generator.state
    log = []
    with launch_trace.recording([eng, gen], log) as rec:
        rec.on = True
        for _ in range(2):
            x.rng.bit_generator.state = state   # (a case that draws more inputs draws the same ones in both calls)
            call(gen, x)
    torch.cuda.synchronize()
    return log


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_trace_equals_the_recorded_one(lib, golden, monkeypatch, case):
    got = json.loads(json.dumps(trace_case(lib, case, monkeypatch.setenv)))   # (tuples -> lists, as stored)
    want = golden[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (case, i, got[max(i - 2, 0):i + 1], want[max(i - 2, 0):i + 1])
    assert len(got) == len(want), (case, len(got), len(want))
