"""Contrastive search on the GPU: vc_contrastive_pick_f32 against tests/contrastive_ref.py: pick_rows on junk-filled buffers, and
CaptionGenerator.contrastive_search against the float64 reference on cases whose decisions are safe (tests/test_contrastive_host.py
proves that on the CPU)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import abi, spec
from vae_captioning_amd.abi import VaecapError
from vae_captioning_amd.controls import DecodeControls
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.generate import CaptionGenerator

from . import contrastive_ref as ref
from . import controls_ref
from .gpu_util import P, dev, host, release, stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMS = dict(rtol=1e-4, atol=1e-6)   # float64 sums of f32 log terms (tests/test_gpu_sbs.py)
BOS, EOS, LMAX = ref.BOS, ref.EOS, ref.LMAX


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def launch(lib, c, k, H, alpha, eos, emit, rows=None, Lmax=None, want_pick=True, **override):
    """vc_contrastive_pick_f32 on device copies of the case's buffers; h_sel / parent / pick / score start as junk.  -> dict of host arrays"""
    rows = c["tok"].shape[0] if rows is None else rows
    Lmax = c["seq"].shape[1] if Lmax is None else Lmax
    d = {n: dev(c[n]) for n in ("h2", "tok", "p", "hist", "len", "done", "seq", "logprob")}
    nb = max(rows, 1)   # (rows = 0 still takes pointers)
    d["h_sel"] = torch.full((nb, H), -55.5, device="cuda")
    d["parent"] = torch.full((nb * k,), -7, dtype=torch.int32, device="cuda")
    d["pick"] = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
    d["score"] = torch.full((nb, k), -55.5, device="cuda")
    d.update(override)
    lib.vc_contrastive_pick_f32(stream(), rows, k, H, Lmax, P(d["h2"]), P(d["tok"]), P(d["p"]), P(d["hist"]), P(d["len"]), P(d["done"]),
                                P(d["seq"]), P(d["logprob"]), alpha, eos, emit, P(d["h_sel"]), P(d["parent"]),
                                P(d["pick"]) if want_pick else None, P(d["score"]) if want_pick else None)
    out = {n: host(t) for n, t in d.items()}
    release()
    return out


def check(c, got, want, safe, k, emit):
    """a launch's outputs against pick_rows': scores within ATOL + RTOL * |s|; on the rows whose decision is safe every output exactly
    (h_sel bit for bit, the appended unit vector to 1e-6, logprob within SUMS); rows that did not run and every slot the kernel has no
    business in keep their junk bit for bit"""
    rows = c["tok"].shape[0]
    ran, idle = want["ran"], ~want["ran"]
    assert (np.abs(got["score"][ran] - want["score"][ran]) <= ref.ATOL + ref.RTOL * np.abs(want["score"][ran])).all()
    ok = ran & safe
    np.testing.assert_array_equal(got["pick"][ok], want["pick"][ok])
    np.testing.assert_array_equal(got["parent"].reshape(rows, k)[ok], want["parent"].reshape(rows, k)[ok])
    np.testing.assert_array_equal(got["seq"][ok], want["seq"][ok])
    np.testing.assert_array_equal(got["len"][ok], want["len"][ok])
    np.testing.assert_array_equal(got["done"][ok], want["done"][ok])
    np.testing.assert_allclose(got["logprob"][ok], want["logprob"][ok], **SUMS)
    h2 = c["h2"].reshape(rows, k, -1)
    for r in np.nonzero(ok)[0]:
        n = int(c["len"][r]) + emit
        assert np.array_equal(_bits(got["h_sel"][r]), _bits(h2[r, want["pick"][r]]))
        assert abs(float(np.sqrt((got["hist"][r, n].astype(np.float64) ** 2).sum())) - 1.0) <= 1e-6
        np.testing.assert_allclose(got["hist"][r, n], want["hist"][r, n], rtol=0, atol=1e-6)
    for r in np.nonzero(ran)[0]:   # (an unsafe row too: whatever it picked, it wrote one slot)
        n = int(c["len"][r]) + emit
        keep = np.ones(c["hist"].shape[1], bool)
        keep[n] = False
        assert np.array_equal(_bits(got["hist"][r, keep]), _bits(c["hist"][r, keep]))
    for name, junk in (("h_sel", np.float32(-55.5)), ("pick", -7), ("score", np.float32(-55.5))):
        assert (got[name][idle] == junk).all(), name
    assert (got["parent"].reshape(rows, k)[idle] == -7).all()
    for name in ("hist", "seq", "len", "done", "logprob"):
        assert np.array_equal(_bits(got[name][idle]), _bits(c[name][idle])), name
    if not emit:   # the <BOS> round leaves the captions alone
        for name in ("seq", "len", "done", "logprob"):
            assert np.array_equal(_bits(got[name]), _bits(c[name])), name
    else:
        keep = np.ones(c["seq"].shape, bool)
        keep[np.nonzero(ran)[0], c["len"][ran]] = False
        assert np.array_equal(got["seq"][keep], c["seq"][keep])


@pytest.mark.parametrize("rows,k,n,H,alpha", ref.KERNEL_GRID, ids=["r%d-k%d-n%d-H%d-a%g" % key for key in ref.KERNEL_GRID])
def test_kernel_matches_pick_rows(lib, rows, k, n, H, alpha):
    c, emit = ref.kernel_case(rows, k, n, H, alpha)
    want, safe = ref.kernel_reference(rows, k, n, H, alpha)
    assert int((want["ran"] & ~safe).sum()) <= 0.02 * rows
    got = launch(lib, c, k, H, alpha, ref.KERNEL_EOS, emit)
    check(c, got, want, safe, k, emit)


def _edge(h, p, hist, tok, alpha, H=32, n_pad=LMAX):
    """a one-row case from candidate vectors h [k, <= H], probabilities, history vectors and words (zero-padded to H)"""
    k, n = len(h), len(hist)
    pad = lambda a, rows: np.concatenate([np.asarray(a, np.float32).reshape(rows, -1), np.zeros((rows, H - np.shape(a)[-1]), np.float32)], 1)
    full = np.full((1, n_pad + 1, H), 7777.0, np.float32)
    if n:
        full[0, :n] = pad(hist, n)
    return dict(h2=pad(h, k), tok=np.asarray(tok, np.int32).reshape(1, k), p=np.asarray(p, np.float32).reshape(1, k), hist=full,
                len=np.array([n - 1], np.int32), done=np.zeros(1, np.int32), seq=np.full((1, n_pad), 9, np.int32), logprob=np.array([-2.0]))


def test_constructed_edge_rows(lib):
    def run(c, alpha):
        k = c["tok"].shape[1]
        want = ref.pick_rows(c["h2"], c["tok"], c["p"], c["hist"], c["len"], c["done"], c["seq"], c["logprob"], alpha, EOS, 1)
        got = launch(lib, c, k, 32, alpha, EOS, 1)
        assert (np.abs(got["score"] - want["score"]) <= ref.ATOL + ref.RTOL * np.abs(want["score"])).all()
        return got, want

    g = [[0.6, 0.8], [1.0, 0.0]]
    # identical candidates with equal p: the tie goes to the lower rank
    got, _ = run(_edge([[1, 2]] * 3, [0.25] * 3, g, [7, 8, 9], 0.6), 0.6)
    assert got["pick"][0] == 0 and got["score"][0, 0] == got["score"][0, 1] == got["score"][0, 2] and got["seq"][0, 1] == 7
    got, _ = run(_edge([[0.6, 0.8], [1, 2], [1, 2]], [0.25] * 3, g, [7, 8, 9], 1.0), 1.0)   # rank 0 is the history itself
    assert got["pick"][0] == 1
    # a zero vector: similarity 0, appended as it is
    got, want = run(_edge([[0, 0], [0.6, 0.8]], [0.5, 0.5], g, [7, 8], 1.0), 1.0)
    assert got["score"][0, 0] == 0.0 and got["pick"][0] == 0 and not got["hist"][0, 2].any() and not got["h_sel"][0].any()
    # a candidate equal to a history vector: similarity 1
    got, _ = run(_edge([[1.2, 1.6], [0, 3]], [0.5, 0.5], g, [7, 8], 1.0), 1.0)
    assert abs(got["score"][0, 0] + 1.0) <= 1e-6 and got["pick"][0] == 1
    # all-negative similarities: the maximum is the least negative, not 0
    got, want = run(_edge([[-0.6, -0.8], [-1, 0.5]], [0.5, 0.5], g, [7, 8], 1.0), 1.0)
    assert (got["score"][0] > 0).all() and got["pick"][0] == want["pick"][0] == 0 and abs(got["score"][0, 1] - 0.2 / np.sqrt(1.25)) <= 1e-6
    # <EOS> picked
    got, _ = run(_edge([[0, 1], [1, 0]], [0.9, 0.1], g, [EOS, 8], 0.0), 0.0)
    assert got["done"][0] == 1 and got["seq"][0, 1] == EOS and got["len"][0] == 2
    assert got["logprob"][0] == pytest.approx(-2.0 + float(np.log(np.float32(0.9))), rel=1e-6)
    # a row that already holds Lmax words has no slot left: nothing is written
    c = _edge([[0, 1], [1, 0]], [0.9, 0.1], g, [7, 8], 0.6)
    c["len"][0] = LMAX
    got = launch(lib, c, 2, 32, 0.6, EOS, 1)
    assert got["len"][0] == LMAX and got["pick"][0] == -7 and (got["h_sel"] == -55.5).all() and np.array_equal(_bits(got["hist"]), _bits(c["hist"]))


@pytest.mark.parametrize("H", [36, 512])
def test_a_row_alone_is_the_row_in_the_batch(lib, H):
    """one row's outputs are bit-equal in a launch of 1 row and as row 77 of 130"""
    k, n, alpha = 16, LMAX, 0.6
    c, emit = ref.kernel_case(130, k, n, H, alpha)
    c = dict(c, done=np.zeros(130, np.int32))
    r = 77
    one = {name: (a.reshape(130, k, H)[r].copy() if name == "h2" else a[r:r + 1].copy()) for name, a in c.items()}
    full, alone = launch(lib, c, k, H, alpha, ref.KERNEL_EOS, emit), launch(lib, one, k, H, alpha, ref.KERNEL_EOS, emit)
    for name in ("score", "pick", "h_sel", "hist", "seq", "len", "done", "logprob"):
        assert np.array_equal(_bits(full[name][r]), _bits(alone[name][0])), name
    assert (full["parent"].reshape(130, k)[r] - r * k == alone["parent"]).all()


def test_null_outputs_and_no_rows(lib):
    c, emit = ref.kernel_case(3, 5, 2, 36, 0.6)
    a, b = launch(lib, c, 5, 36, 0.6, ref.KERNEL_EOS, emit), launch(lib, c, 5, 36, 0.6, ref.KERNEL_EOS, emit, want_pick=False)
    assert (b["pick"] == -7).all() and (b["score"] == -55.5).all()
    for name in ("h_sel", "parent", "hist", "seq", "len", "done", "logprob"):
        assert np.array_equal(_bits(a[name]), _bits(b[name])), name
    z = launch(lib, c, 5, 36, 0.6, ref.KERNEL_EOS, emit, rows=0)
    assert np.array_equal(_bits(z["hist"]), _bits(c["hist"])) and np.array_equal(z["len"], c["len"])


def test_argument_errors_launch_nothing(lib):
    c, emit = ref.kernel_case(3, 5, 2, 32, 0.6)

    def call(k=5, H=32, alpha=0.6, Lmax=LMAX, **null):
        d = {n: dev(c[n]) for n in ("h2", "tok", "p", "hist", "len", "done", "seq", "logprob")}
        d["h_sel"], d["parent"] = torch.zeros((3, 32), device="cuda"), torch.zeros((48,), dtype=torch.int32, device="cuda")
        d.update(null)
        lib.vc_contrastive_pick_f32(stream(), 3, k, H, Lmax, P(d["h2"]), P(d["tok"]), P(d["p"]), P(d["hist"]), P(d["len"]), P(d["done"]), P(d["seq"]),
                                    P(d["logprob"]), alpha, EOS, 1, P(d["h_sel"]), P(d["parent"]), None, None)
        return d

    for bad in (dict(k=0), dict(k=17), dict(H=30), dict(H=0), dict(alpha=1.5), dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf")),
                dict(Lmax=0)) + tuple({n: None} for n in ("h2", "tok", "p", "hist", "len", "done", "seq", "logprob", "h_sel", "parent")):
        with pytest.raises(VaecapError):
            call(**bad)
    with pytest.raises(VaecapError):   # 16-byte alignment
        call(h_sel=torch.zeros((3 * 32 + 4,), device="cuda")[1:])
    d = call()   # (the valid call does run)
    np.testing.assert_array_equal(host(d["len"]), ref.kernel_reference(3, 5, 2, 32, 0.6)[0]["len"])
    assert host(d["len"])[0] == c["len"][0] + 1
    release()


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def engine(case):
    p, P0 = controls_ref.pool(case)[:2]
    eng = CaptionEngine(p, 40, lib=abi.load())
    eng.load_params(P0)
    return eng


def inputs(case, name):
    feats, cv, eps = ref.case_inputs(case, name)
    eng = engine(case)
    return CaptionGenerator(eng), feats, (cv if spec.uses_ci(eng.p) else None), eps


def decode(gen, name, feats, cv, eps, **kw):
    k, alpha, ctl = ref.SETTINGS[name]
    kw = dict(dict(k=k, alpha=alpha, controls=controls_ref.settings()[ctl] if ctl is not None else None), **kw)
    return gen.contrastive_search(feats, cv, eps, BOS, EOS, max_len=ref.MAX_LEN, **kw)


CASES = sorted(ref.IMAGES)
IDS = ["%s-%s" % (controls_ref.CASE_IDS[c], n) for c, n in CASES]


@pytest.mark.parametrize("case,name", CASES, ids=IDS)
def test_contrastive_search_matches_the_float64_reference(lib, case, name):
    """the four prior cases (k = 5, alpha = 0.6), k = 16 (softmax and top-k as two calls), alpha = 1, and all four controls together:
    V = 40, B = 6, max_len 10; the same tokens, logprob within SUMS; twice (the second call replays the captured chunks)"""
    gen, feats, cv, eps = inputs(case, name)
    want, _ = ref.run_case(case, name)
    for _ in range(2):
        got = decode(gen, name, feats, cv, eps)
        assert [list(t) for t, _ in got] == [w[0] for w in want]
        np.testing.assert_allclose([lp for _, lp in got], [w[1] for w in want], **SUMS)
    assert len(gen._graphs) >= 1
    ctl = ref.SETTINGS[name][2]
    if ctl is not None:
        for toks, _ in got:
            assert all(controls_ref.properties(toks, controls_ref.settings()[ctl], EOS))


@pytest.mark.parametrize("case", range(len(controls_ref.CASES)), ids=controls_ref.CASE_IDS)
def test_alpha_zero_and_k_one_are_greedy(lib, case):
    gen, feats, cv, eps = inputs(case, "plain")
    want = gen.greedy(feats, cv, eps, BOS, EOS, max_len=ref.MAX_LEN)
    assert [t for t, _ in decode(gen, "plain", feats, cv, eps, alpha=0.0)] == want
    assert [t for t, _ in decode(gen, "plain", feats, cv, eps, k=1)] == want
    assert [t for t, _ in decode(gen, "plain", feats, cv, eps)] != want


@pytest.mark.parametrize("name", ["plain", "all"])
def test_graph_replay_is_the_eager_loop(lib, name, monkeypatch):
    """identical tokens and identical logprob bits"""
    gen, feats, cv, eps = inputs(3, name)
    first = decode(gen, name, feats, cv, eps)
    n = len(gen._graphs)
    assert n >= 1 and decode(gen, name, feats, cv, eps) == first and len(gen._graphs) == n   # replayed, not captured again
    monkeypatch.setenv("VC_DECODE_GRAPH", "0")
    eager = CaptionGenerator(gen.e)
    got = decode(eager, name, feats, cv, eps)
    assert len(eager._graphs) == 0 and [t for t, _ in got] == [t for t, _ in first]
    assert np.array_equal(_bits(np.array([lp for _, lp in got])), _bits(np.array([lp for _, lp in first])))


def test_new_parameters_are_packed_and_projected_again(lib):
    """a second call after the engine's parameters change decodes with the new ones (the packed Wh and the [V, 4H] table are per
    parameter version), and going back gives the first result again"""
    p, P0 = controls_ref.pool(1)[:2]
    eng = CaptionEngine(p, 40, lib=lib)
    eng.load_params(P0)
    feats, cv, eps = ref.case_inputs(1, "plain")
    gen = CaptionGenerator(eng)
    first = decode(gen, "plain", feats, None, eps)
    assert gen._xproj is not None   # (6 * 5 rows x 10 rounds >= V = 40: the table is in use)
    P1 = {k: (v[::-1].copy() if k.endswith("dec_embeddings") else v) for k, v in P0.items()}   # every word takes another word's embedding
    eng.load_params(P1)
    second = decode(gen, "plain", feats, None, eps)
    fresh = CaptionGenerator(eng)
    assert second != first and second == decode(fresh, "plain", feats, None, eps)
    eng.load_params(P0)
    assert decode(gen, "plain", feats, None, eps) == first


def test_max_len_reached_without_eos(lib):
    gen, feats, cv, eps = inputs(0, "plain")
    want, _ = ref.run_case(0, "plain")
    assert all(EOS not in w[0] and len(w[0]) == ref.MAX_LEN for w in want)
    for max_len in (3, 4, 5):   # a ragged chunk, one whole chunk, a chunk and a round
        got = gen.contrastive_search(feats, cv, eps, BOS, EOS, k=5, alpha=0.6, max_len=max_len)
        assert [t for t, _ in got] == [w[0][:max_len] for w in want]
    lp = ref.run_image(0, "plain", ref.IMAGES[(0, "plain")][0])[0][1]
    assert gen.contrastive_search(feats, cv, eps, BOS, EOS, k=5, alpha=0.6, max_len=ref.MAX_LEN, check_every=0)[0][1] == pytest.approx(lp, rel=1e-4)


def test_value_errors_launch_nothing(lib):
    gen, feats, cv, eps = inputs(1, "plain")
    for kw in (dict(k=0), dict(k=17), dict(k=2.5), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float("nan")), dict(alpha=float("inf")),
               dict(controls=DecodeControls(min_len=10)), dict(controls=DecodeControls(banned=[EOS])), dict(controls=dict(min_len=3))):
        with pytest.raises(ValueError):
            gen.contrastive_search(feats, cv, eps, BOS, EOS, max_len=ref.MAX_LEN, **kw)
    assert gen.buf == {} and gen._graphs == {}


def test_main_synthetic_inference(tmp_path):
    """main.py --synthetic --mode inference --sample_gen contrastive with --eval_captions in a fresh process (on a checkpoint written
    here): every record carries logprob, the metrics file names both flags"""
    from vae_captioning_amd.utils.parameters import Parameters
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden, p.latent_size, p.gen_z_samples = 32, 64, 64, 10, 4
    P0 = spec.init_caption_params(p, 200, seed=3)
    os.makedirs(tmp_path / "checkpoints")
    np.savez(str(tmp_path / "checkpoints" / "cs.ckpt.npz"), **{k: (v * 3).astype(np.float32) for k, v in P0.items()})
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "200", "--embed_dim", "32",
           "--enc_hid", "64", "--dec_hid", "64", "--latent", "10", "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "cs",
           "--mode", "inference", "--gen_name", "cs", "--sample_gen", "contrastive", "--contrastive_k", "4", "--contrastive_alpha", "0.5",
           "--eval_captions"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = json.load(open(tmp_path / "val_cs.json"))
    assert len(recs) == 8 and all(set(x) == {"image_id", "caption", "logprob"} for x in recs)
    assert all(isinstance(x["logprob"], float) and x["logprob"] < 0 and x["caption"] for x in recs)
    m = json.load(open(tmp_path / "val_cs_metrics.json"))
    assert (m["sample_gen"], m["contrastive_k"], m["contrastive_alpha"]) == ("contrastive", 4, 0.5)
