"""-m gpu: stochastic beam search -- vc_sbs_expand_f32 / vc_sbs_update against the float64 reference of tests/sbs_ref.py after every
round (injected noise, junk-filled buffers), garbage rows, the Philox path against host-built noise, the sampler's statistics on the
device, CaptionGenerator.stochastic_beam_search end to end (eager and replayed), its argument checks and the command line."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import spec
from vae_captioning_amd.controls import DecodeControls
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.generate import CaptionGenerator, sbs_weights

from . import dbs_ref, sbs_ref
from .gpu_util import P, dev, host, stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOS, EOS = sbs_ref.BOS, sbs_ref.EOS
SUMS = dict(rtol=1e-4, atol=1e-6)   # float64 sums of f32 log-softmax terms (tests/test_gpu_mixture.py)
STREAM_ID = 9 << 32


class SbsState(object):
    """the state of B images of beam n, junk-filled and then started by vc_sbs_init; the candidate arrays stay junk until a row is
    expanded"""
    FIELDS = ("count", "phi", "G", "len", "done", "kappa", "parent", "tok", "rnd")

    def __init__(self, lib, B, n, L, kc, bos, H=8):
        M = B * n
        junk_i = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
        junk_d = lambda *shape: torch.full(shape, 3.5, dtype=torch.float64, device="cuda")
        self.B, self.n, self.L, self.M, self.kc = B, n, L, M, kc
        self.count, self.len, self.done, self.parent, self.tok, self.rnd = junk_i(B), junk_i(M), junk_i(M), junk_i(M), junk_i(M), junk_i(1)
        self.phi, self.G, self.kappa = junk_d(M), junk_d(M), junk_d(B)
        self.sent = [junk_i(M, L), junk_i(M, L)]
        self.ck, self.cl, self.ci = junk_d(M, kc), torch.full((M, kc), 3.5, device="cuda"), junk_i(M, kc)
        c_in, h_in = torch.randn(B, H, device="cuda"), torch.randn(B, H, device="cuda")
        c_out, h_out = torch.zeros(M, H, device="cuda"), torch.zeros(M, H, device="cuda")
        lib.vc_sbs_init(stream(), B, n, L, bos, H, P(c_in), P(h_in), P(c_out), P(h_out), P(self.count), P(self.phi), P(self.G), P(self.len),
                        P(self.done), P(self.sent[0]), P(self.sent[1]), P(self.kappa), P(self.parent), P(self.tok), P(self.rnd))
        assert torch.equal(c_out, c_in.repeat_interleave(n, 0)) and torch.equal(h_out, h_in.repeat_interleave(n, 0))

    def round(self, lib, it, logits, V, gumbel=None, g_rounds=0, seed=0, step=None, ld=None):
        before = {"old_" + k: host(getattr(self, k)).copy() for k in ("ck", "cl", "ci")}
        lib.vc_sbs_expand_f32(stream(), P(logits), self.M, self.n, V, ld or V, P(self.count), P(self.done), self.kc, P(gumbel), g_rounds,
                              P(self.rnd), seed, STREAM_ID, P(step), P(self.ck), P(self.cl), P(self.ci))
        cands = {k: host(getattr(self, k)).copy() for k in ("ck", "cl", "ci")}
        cands.update(before)
        lib.vc_sbs_update(stream(), self.B, self.n, self.kc, self.L, BOS, EOS, P(self.ck), P(self.cl), P(self.ci), P(self.count), P(self.phi),
                          P(self.G), P(self.len), P(self.done), P(self.sent[it & 1]), P(self.sent[1 - (it & 1)]), P(self.kappa),
                          P(self.parent), P(self.tok), P(self.rnd))
        snap = {k: host(getattr(self, k)).copy() for k in self.FIELDS}
        snap["sent"] = host(self.sent[1 - (it & 1)]).copy()
        snap.update(cands)
        return snap


def check_round(snap, ref, info, B, n, L, kc, it, where):
    """a round's device state against the reference's: selections exactly, float64 fields within SUMS"""
    live = info["live"]
    assert np.array_equal(snap["ci"][live], info["cand_idx"][live]), where
    np.testing.assert_allclose(snap["cl"][live], info["cand_lsm"][live], err_msg=str(where), **SUMS)
    # (a key is lsm + g with the reference's own g: its error is lsm's, so the bound is taken on lsm's size)
    assert (np.abs(snap["ck"][live] - info["cand_key"][live]) <= SUMS["atol"] + SUMS["rtol"] * np.abs(info["cand_lsm"][live])).all(), where
    for k in ("ck", "cl", "ci"):   # rows that are not expanded are not written: junk until their first expansion, then what that left
        assert np.array_equal(snap[k][~live], snap["old_" + k][~live]), (k,) + where
    if it == 0:
        assert (snap["ck"][~live] == 3.5).all() and (snap["ci"][~live] == -7).all() and (snap["cl"][~live] == 3.5).all(), where
    assert snap["rnd"][0] == it + 1, where
    assert np.array_equal(snap["count"], ref["count"]), where
    for k in ("len", "done"):
        assert np.array_equal(snap[k].reshape(B, n), ref[k]), (k,) + where
    for k in ("parent", "tok"):
        assert np.array_equal(snap[k], ref[k]), (k,) + where
    sent = snap["sent"].reshape(B, n, L)
    for b in range(B):
        for j in range(int(ref["count"][b])):
            ln = int(ref["len"][b, j])
            assert sent[b, j, :ln].tolist() == ref["sent"][b, j, :ln].tolist(), where + (b, j)
    worst = {}
    for k in ("phi", "G", "kappa"):
        got, want = snap[k].reshape(ref[k].shape), ref[k]
        fin = np.isfinite(want)
        worst[k] = float(np.max(np.abs(got[fin] - want[fin]) / (SUMS["atol"] + SUMS["rtol"] * np.abs(want[fin])), initial=0.0))
        np.testing.assert_allclose(got, want, err_msg=str((k,) + where), **SUMS)
    return worst


@pytest.mark.parametrize("name", list(sbs_ref.CASES))
def test_kernels_follow_the_reference_after_every_round(lib, name):
    """the committed cases of tests/sbs_ref.py (tests/test_sbs_host.py proves each safe): injected float64 noise, junk-filled buffers,
    vc_sbs_init's start state; after EVERY round the candidates of the expanded rows, count, len, done, parent, tok and the sentences
    exactly, phi / G / kappa within SUMS; rows that are not expanded keep their junk"""
    B, n, V, L, rounds, _, _ = sbs_ref.CASES[name]
    kc = min(n + 1, V)
    logits, gumbel = sbs_ref.case_inputs(name)
    st = SbsState(lib, B, n, L, kc, BOS)
    gd = dev(gumbel)
    refs = sbs_ref.case_rounds(name)
    worst = {}
    for it in range(rounds):
        snap = st.round(lib, it, dev(logits[it]), V, gd, rounds)
        w = check_round(snap, refs[it][0], refs[it][1], B, n, L, kc, it, (name, it))
        worst = {k: max(w[k], worst.get(k, 0.0)) for k in w}
    print("%s: worst error / bound %s" % (name, worst))
    if n == 1:   # one exact sample: the arg-max of lsm + g every round, and G never changes
        assert (host(st.G) == 0.0).all()


def test_garbage_rows_change_nothing_and_no_index_leaves_the_vocabulary(lib):
    """rows at or past count and rows with done set hold NaN and huge logits: the other rows' outputs are what they are without the
    garbage, bit for bit, and no index leaves [0, V); then NaN / inf inside LIVE rows: indices still valid and distinct"""
    B, n, V, kc = 3, 4, 70, 5
    rng = np.random.default_rng(11)
    x = (2.0 * rng.standard_normal((B * n, V))).astype(np.float32)
    g = dev(rng.gumbel(size=(1, B * n, V)))
    count = np.array([4, 2, 3], np.int32)
    done = np.zeros((B, n), np.int32)
    done[0, 1] = done[2, 0] = 1
    skip = ((np.arange(n)[None, :] >= count[:, None]) | (done != 0)).reshape(-1)
    bad = x.copy()
    bad[skip] = np.resize(np.array([np.nan, 3e38, -3e38, np.inf], np.float32), (int(skip.sum()), V))
    outs = []
    for rows in (x, bad):
        ck, cl, ci = dev(np.full((B * n, kc), 3.5)), dev(np.full((B * n, kc), 3.5, np.float32)), dev(np.full((B * n, kc), -7, np.int32))
        lib.vc_sbs_expand_f32(stream(), P(dev(rows)), B * n, n, V, V, P(dev(count)), P(dev(done)), kc, P(g), 1, None, 0, STREAM_ID, None,
                              P(ck), P(cl), P(ci))
        outs.append((host(ck), host(cl), host(ci)))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    ci = outs[1][2]
    assert (ci[skip] == -7).all() and ((ci[~skip] >= 0) & (ci[~skip] < V)).all()
    for r in np.nonzero(~skip)[0]:
        key, l, idx, _ = sbs_ref.expand_row(x[r], host(g)[0, r], kc)
        assert ci[r].tolist() == idx.tolist()
    # garbage in rows that ARE expanded
    worse = x.copy()
    worse[0, ::3], worse[4, 5], worse[5, :] = np.nan, np.inf, np.nan
    ck, cl, ci = dev(np.zeros((B * n, kc))), dev(np.zeros((B * n, kc), np.float32)), dev(np.full((B * n, kc), -7, np.int32))
    lib.vc_sbs_expand_f32(stream(), P(dev(worse)), B * n, n, V, V, P(dev(count)), P(dev(done)), kc, P(g), 1, None, 0, STREAM_ID, None,
                          P(ck), P(cl), P(ci))
    ci = host(ci)[~skip]
    assert ((ci >= 0) & (ci < V)).all() and all(len(set(row.tolist())) == kc for row in ci)


@pytest.mark.parametrize("B,n,V,ld", [(2, 3, 70, 70), (3, 2, 1025, 1032), (1, 2, 12301, 12301)],
                         ids=["V70", "V1025-rows-start-inside-a-quad", "V12301-two-tiles-unstaged"])
def test_philox_noise_is_the_documented_stream(lib, B, n, V, ld):
    """gumbel = NULL against noise built on the host from vc_philox_u32's words, u = (w + 0.5) 2^-32, g = -log(-log u): the same
    selections, values within SUMS; against the host reference too; another round or another step base gives other noise"""
    rows, kc, seed = B * n, n + 1, (77 << 32) | 12345
    rng = np.random.default_rng(V)
    x = np.zeros((rows, ld), np.float32)
    x[:, :V] = (2.0 * rng.standard_normal((rows, V))).astype(np.float32)
    x[:, V:] = 1e30   # the padding of a row is never read
    xd = dev(x)
    count, done = dev(np.full(B, n, np.int32)), dev(np.zeros(rows, np.int32))

    def expand(rd, base, gumbel=None):
        ck, cl, ci = torch.zeros(rows, kc, dtype=torch.float64, device="cuda"), torch.zeros(rows, kc, device="cuda"), torch.zeros(rows, kc, dtype=torch.int32, device="cuda")
        lib.vc_sbs_expand_f32(stream(), P(xd), rows, n, V, ld, P(count), P(done), kc, P(gumbel), 1 if gumbel is not None else 0,
                              P(dev(np.array([rd], np.int32))), seed, STREAM_ID, P(dev(np.array([base], np.int32))), P(ck), P(cl), P(ci))
        return host(ck), host(cl), host(ci)

    words = torch.zeros(rows * V, dtype=torch.int32, device="cuda")
    lib.vc_philox_u32(stream(), P(words), rows * V, seed, STREAM_ID, P(dev(np.array([3 + 4096], np.int32))))
    g = sbs_ref.gumbel_from_words(host(words).view(np.uint32)).reshape(1, rows, V)
    assert np.isfinite(g).all() and g.max() < 23.0   # (the tail ends at -log(2^-33) = 22.9)
    a, b = expand(3, 4096), expand(0, 0, dev(g))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])
    np.testing.assert_allclose(a[0], b[0], **SUMS)
    for r in range(rows):
        key, l, idx, gap = sbs_ref.expand_row(x[r, :V], g[0, r], kc)
        assert gap >= sbs_ref.ROW_GAP and a[2][r].tolist() == idx.tolist(), r
        assert (np.abs(a[0][r] - key) <= SUMS["atol"] + SUMS["rtol"] * np.abs(l)).all()
    other, base2 = expand(4, 4096), expand(3, 8192)
    assert not np.array_equal(other[0], a[0]) and not np.array_equal(base2[0], a[0]) and not np.array_equal(other[0], base2[0])
    again = expand(3, 4096)
    assert all(np.array_equal(u, v) for u, v in zip(a, again))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_device_samples_without_replacement(lib, seed):
    """the table model of tests/test_sbs_host.py (4 words, 3 rounds, 40 captions) as fixed logits, 4096 images in ONE search of width 2
    with Philox noise: the first-ranked caption is distributed as p (chi-square, 39 degrees of freedom, below its 99.9 % point 72.05)
    and every caption's inclusion count is within 4.5 standard deviations of exact sampling without replacement"""
    tables = sbs_ref.table_model()
    caps, p = sbs_ref.table_captions(tables)
    B, n, V, L = 4096, 2, sbs_ref.T_V, sbs_ref.T_LEN + 1
    st = SbsState(lib, B, n, L, 3, sbs_ref.T_BOS)
    sent, ln = np.full((B * n, L), sbs_ref.T_BOS, np.int32), np.ones(B * n, np.int32)
    for it in range(sbs_ref.T_LEN):
        snap = st.round(lib, it, dev(sbs_ref.table_logits(tables, sent, ln)), V, seed=1000 + seed)
        sent, ln = snap["sent"], snap["len"]
    assert (snap["done"] == 1).all() and (snap["count"] == n).all()
    state = dict(count=snap["count"], phi=snap["phi"].reshape(B, n), G=snap["G"].reshape(B, n), len=ln.reshape(B, n),
                 sent=sent.reshape(B, n, L), kappa=snap["kappa"])
    chi2, worst, est = sbs_ref.table_stats(sbs_ref.results(state, sbs_ref.T_EOS), caps, p)
    print("seed %d: chi-square %.1f, largest inclusion deviation %.2f sd" % (seed, chi2, worst))
    assert chi2 < 72.05 and worst < 4.5
    assert (np.diff(state["G"], axis=1) < 0).all()   # rank order


# ---------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def inputs(case, seed=7):
    return dbs_ref.model_inputs(seed, **dbs_ref.CASES[case])


def generator(lib, case, seed=7):
    p, P0, feats, cv, eps, cm = inputs(case, seed)
    eng = CaptionEngine(p, 40, lib=lib)
    eng.load_params(P0)
    return CaptionGenerator(eng), feats, (cv if spec.uses_ci(p) else None), eps


def traced(lib, monkeypatch, case, n, max_len, gumbel, **kw):
    """an eager search that keeps every round's logits"""
    monkeypatch.setenv("VC_DECODE_GRAPH", "0")
    gen, feats, cv, eps = generator(lib, case)
    gen.sbs_trace = []
    got = gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, beam_size=n, max_len=max_len, gumbel=gumbel, **kw)
    monkeypatch.delenv("VC_DECODE_GRAPH")
    return got, list(gen.sbs_trace)


@pytest.mark.parametrize("case,n", [(1, 3), (3, 5), (0, 8)], ids=["normal-n3", "gmm-n5", "no-encoder-n8"])
def test_search_matches_the_reference_on_its_own_logits(lib, monkeypatch, case, n):
    """stochastic_beam_search with injected noise against the float64 reference driven by the engine's own per-round logits: the same
    captions in the same order, logprob / perturbed / kappa within SUMS, the weights sbs_weights'; graph replay returns the eager
    result; all captions of an image are distinct"""
    V, max_len = 40, 8
    B = inputs(case)[2].shape[0]
    gumbel = np.random.default_rng(100 + n).gumbel(size=(max_len, B * n, V))
    got, trace = traced(lib, monkeypatch, case, n, max_len, gumbel)
    st = sbs_ref.init_state(B, n, max_len + 1, BOS)
    for it, lg in enumerate(trace):
        st, info = sbs_ref.round_(st, lg, gumbel[it], min(n + 1, V), BOS, EOS)
        # (the reference sees the kernel's own logits: the two differ by the float32 rounding of lsm alone, <= 2 ulp of |lsm| < 16 per
        # round; what is compared below rests on which candidates are taken and in which order -- two near-equal keys of a row whose
        # words are both taken or both left show up in these two margins, or change nothing)
        assert min(info["boundary"], info["order"]) >= 4e-5, (it, info["boundary"], info["order"])
    ref = sbs_ref.results(st, EOS)
    assert len(got) == B
    for b in range(B):
        kap, caps = ref[b]
        np.testing.assert_allclose(got[b]["kappa"], kap, **SUMS)
        assert [c[0] for c in got[b]["captions"]] == [c[0] for c in caps], b
        assert [c[3] for c in got[b]["captions"]] == [c[3] for c in caps], b
        assert len({tuple(c[0]) for c in caps}) == len(caps) == min(n, len(caps))
        for k in (1, 2):
            np.testing.assert_allclose([c[k] for c in got[b]["captions"]], [c[k] for c in caps], **SUMS)
        w, nw = sbs_weights([c[1] for c in got[b]["captions"]], got[b]["kappa"])
        assert [c[4] for c in got[b]["captions"]] == w.tolist() and [c[5] for c in got[b]["captions"]] == nw.tolist()
        np.testing.assert_allclose(nw, [c[5] for c in caps], rtol=1e-3)
    gen, feats, cv, eps = generator(lib, case)
    for call in range(3):   # eager + capture, then replays
        assert gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, beam_size=n, max_len=max_len, gumbel=gumbel) == got, call
    assert len(gen._graphs) >= 1


def test_width_one_is_the_gumbel_max_sample(lib, monkeypatch):
    """n = 1 with injected noise: every round's word is the arg-max of lsm + g on the round's own logits, G stays 0"""
    V, max_len = 40, 8
    B = inputs(1)[2].shape[0]
    gumbel = np.random.default_rng(5).gumbel(size=(max_len, B, V))
    got, trace = traced(lib, monkeypatch, 1, 1, max_len, gumbel)
    for b in range(B):
        (words, lp, G, ended, w, nw), = got[b]["captions"]
        assert G == 0.0 and nw == 1.0
        want, phi = [], 0.0
        for it in range(len(trace)):
            l = sbs_ref.lsm64(trace[it][b])
            v = int(np.argmax(l + gumbel[it, b]))
            want.append(v)
            phi += l[v]
            if v == EOS:
                break
        assert words == want and ended == (want[-1] == EOS)
        np.testing.assert_allclose(lp, phi, **SUMS)


def test_calls_draw_fresh_noise_and_a_seed_repeats(lib):
    gen, feats, cv, eps = generator(lib, 1)
    kw = dict(beam_size=4, max_len=8)
    a, b = gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, **kw), gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, **kw)
    assert a != b
    c, d = gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, seed=5, **kw), gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, seed=5, **kw)
    assert c == d and c != a and gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, seed=6, **kw) != c
    for res in (a, b, c):
        for im in res:
            caps = im["captions"]
            assert len({tuple(x[0]) for x in caps}) == len(caps) == 4
            assert [x[2] for x in caps] == sorted((x[2] for x in caps), reverse=True) and all(x[2] > im["kappa"] for x in caps)
            np.testing.assert_allclose(sum(x[5] for x in caps), 1.0, rtol=1e-12)


def test_controls_hold_in_every_caption(lib):
    gen, feats, cv, eps = generator(lib, 1)
    banned = [3, 4, 5, 6, 7]
    res = gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, beam_size=5, max_len=8, seed=3, controls=DecodeControls(0, 4, 1.0, banned))
    free = gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, beam_size=5, max_len=8, seed=3)
    assert any(set(c[0]) & set(banned) for im in free for c in im["captions"])   # (the controls had something to do)
    for im in res:
        for words, lp, G, ended, w, nw in im["captions"]:
            assert not set(words) & set(banned) and (not ended or len(words) - 1 >= 4), words
            assert EOS not in words[:4]


def test_argument_errors(lib):
    gen, feats, cv, eps = generator(lib, 1)
    for n in (0, 33):
        with pytest.raises(ValueError, match="beam_size"):
            gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, beam_size=n)
    gen.p.temperature = 1.2
    with pytest.raises(ValueError, match="temperature"):
        gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, beam_size=2)
    gen.p.temperature = 1.0
    with pytest.raises(ValueError, match="gumbel"):
        gen.stochastic_beam_search(feats, cv, eps, BOS, EOS, beam_size=2, max_len=8, gumbel=np.zeros((8, 3, 40)))


# ---------------------------------------------------------------- command line
def main_cmd(tmp_path, *extra):
    from vae_captioning_amd.utils.parameters import Parameters
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden, p.latent_size, p.gen_z_samples = 32, 64, 64, 10, 4
    P0 = spec.init_caption_params(p, 200, seed=3)
    os.makedirs(tmp_path / "checkpoints", exist_ok=True)
    np.savez(str(tmp_path / "checkpoints" / "sb.ckpt.npz"), **{k: (v * 3).astype(np.float32) for k, v in P0.items()})
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "200", "--embed_dim", "32",
           "--enc_hid", "64", "--dec_hid", "64", "--latent", "10", "--gen_z_samples", "4", "--bs", "3", "--ckpt_format", "npz", "--checkpoint", "sb",
           "--mode", "inference", "--sample_gen", "stochastic_beam", "--gen_name", "sb"] + list(extra)
    return subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True)


def test_main_synthetic_inference_with_stochastic_beam_search(tmp_path):
    """main.py --synthetic --mode inference --sample_gen stochastic_beam --beam_size 4 --eval_captions in a fresh process: both caption
    files with the new fields, and the metrics file"""
    r = main_cmd(tmp_path, "--beam_size", "4", "--eval_captions")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = json.load(open(tmp_path / "val_sb_diverse.json"))
    assert recs == json.load(open(tmp_path / "val_sb.json")) and len(recs) == 6
    for x in recs:
        m = len(x["captions"])
        assert m == 4 and x["caption"] == x["captions"][0] and x["counts"] == [1] * m
        assert all(len(x[k]) == m for k in ("scores", "logprob", "perturbed", "weight", "norm_weight"))
        assert all(g > x["kappa"] for g in x["perturbed"]) and all(lp < 0 for lp in x["logprob"])
        assert abs(sum(x["norm_weight"]) - 1.0) < 1e-9
        w, nw = sbs_weights(x["logprob"], x["kappa"])
        np.testing.assert_allclose(x["weight"], w, rtol=1e-12)
    metrics = json.load(open(tmp_path / "val_sb_metrics.json"))
    assert metrics["sample_gen"] == "stochastic_beam" and metrics["images"] == 6 and metrics["captions"] == 24


@pytest.mark.parametrize("extra,word", [(("--beam_size", "33"), "1..32"), (("--beam_size", "0"), "1..32"),
                                        (("--beam_size", "4", "--temperature", "1.2"), "--temperature must be 1")],
                         ids=["beam-33", "beam-0", "temperature"])
def test_main_parse_errors(tmp_path, extra, word):
    r = main_cmd(tmp_path, *extra)
    assert r.returncode == 2 and word in r.stderr, r.stderr[-1000:]
