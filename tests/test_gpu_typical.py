"""-m gpu: typical / min-p / eta sampling (csrc/diverse.hip: vc_decode_pick_typical_f32, generate.py: sample / diverse with typical_p /
min_p / eta).  The kernel against the float64 reference of tests/typical_ref.py (exactly on the rows the reference marks safe, inside
the kept set widened by the margins elsewhere; entropy[] within DMARGIN * (1 + H) on every row), its degenerate settings against the
existing kernels bit for bit, its bookkeeping, determinism and batch independence, the drawn distribution, and the feature through the
generator and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd.generate import CaptionGenerator

from . import typical_ref as ty
from .test_gpu_generate import setup

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL_LP = 1e-5          # per token against float64: what tests/test_gpu_score.py holds the log-softmax terms to
SUMS = dict(rtol=1e-4, atol=1e-6)   # what tests/test_gpu_score.py holds score()'s sums to against diverse()'s
SHAPE_IDS = ["v7", "v40", "v1001-padded", "v10000", "v13000-unstaged"]


def _i32(*shape, fill=0):
    return torch.full(shape, fill, dtype=torch.int32, device="cuda")


def _pick(lib, dx, V, ld, t, tau, min_p, eta, du, rows=None, eos=EOS, plain=False):
    """One round on fresh candidates (Lmax 1) -> dict of host arrays.  plain: vc_decode_pick_f32 in sampling mode instead."""
    from .gpu_util import P, host, stream
    R = int(rows if rows is not None else dx.shape[0])
    tok, done, seq, ln, kept = _i32(R, fill=-7), _i32(R), _i32(R, fill=-7), _i32(R), _i32(R, fill=-7)
    lp = torch.zeros(R, dtype=torch.float64, device="cuda")
    ent = torch.full((R,), -7.0, device="cuda")
    if plain:
        lib.vc_decode_pick_f32(stream(), P(dx), R, V, ld, t, P(du), 1, None, eos, P(tok), P(done), P(seq), 1, P(ln), P(lp))
    else:
        lib.vc_decode_pick_typical_f32(stream(), P(dx), R, V, ld, t, tau, min_p, eta, P(du), 1, None, eos, P(tok), P(done), P(seq), 1, P(ln),
                                       P(lp), P(kept), P(ent))
    return dict(tok=host(tok), done=host(done), seq=host(seq), len=host(ln), lp=host(lp), kept=host(kept), ent=host(ent))


_REF = {}


def _case(shape_i, setting_i):
    """(inputs, reference rows) of one case, computed once"""
    key = (shape_i, setting_i)
    if key not in _REF:
        c = ty.make_case(shape_i, setting_i)
        x, V, ld, tau, min_p, eta, t, u = c
        _REF[key] = (c, ty.typical_rows(x[:, :V], t, tau, min_p, eta, u))
    return _REF[key]


# ------------------------------------------------------------------ 1. tokens, kept counts and entropy against the reference
@pytest.mark.parametrize("shape_i", range(len(ty.SHAPES)), ids=SHAPE_IDS)
@pytest.mark.parametrize("setting_i", range(len(ty.SETTINGS)), ids=ty.SETTING_IDS)
def test_tokens_kept_counts_and_entropy_match_the_reference(lib, shape_i, setting_i):
    from .gpu_util import dev
    (x, V, ld, tau, min_p, eta, t, u), ref = _case(shape_i, setting_i)
    unsafe = [r for r in range(ty.ROWS) if not ref[r]["safe"]]
    assert len(unsafe) <= ty.MAX_UNSAFE * ty.ROWS, unsafe
    got = _pick(lib, dev(x), V, ld, t, tau, min_p, eta, dev(u))
    bad = [(r, int(got["tok"][r]), int(got["kept"][r]), ref[r]["token"], ref[r]["kept"]) for r in range(ty.ROWS)
           if ref[r]["safe"] and (got["tok"][r] != ref[r]["token"] or got["kept"][r] != ref[r]["kept"])]
    H = np.array([q["H"] for q in ref])
    herr = np.abs(got["ent"].astype(np.float64) - H) / (ty.DMARGIN * (1.0 + H))
    print("V %d tau %g min_p %g eta %g t %g: unsafe rows %s, mismatches (row, token, kept, ref token, ref kept) %s, worst entropy error "
          "%.3f of its bound (row %d)" % (V, tau, min_p, eta, t, unsafe, bad, herr.max(), int(herr.argmax())))
    assert not bad, bad
    for r in unsafe:
        assert got["tok"][r] in ref[r]["wide_set"], (r, got["tok"][r], ref[r]["token"])
    assert np.isfinite(got["ent"]).all() and (herr <= 1.0).all(), (int(herr.argmax()), herr.max())
    banned = np.nonzero(x[ty.BANNED_ROW, :V] == -ty.FLT_MAX)[0]
    assert got["tok"][ty.BANNED_ROW] not in banned
    assert np.array_equal(got["seq"], got["tok"]) and (got["len"] == 1).all()
    lsm = ty.log_softmax64(x[:, :V])
    np.testing.assert_allclose(got["lp"], lsm[np.arange(ty.ROWS), got["tok"]], rtol=0, atol=ATOL_LP)


# ------------------------------------------------------------------ 2. exact degenerate cases
@pytest.mark.parametrize("shape_i", [1, 2, 3, 4], ids=SHAPE_IDS[1:])
def test_all_cuts_off_is_the_plain_pick_bit_for_bit(lib, shape_i):
    from .gpu_util import dev
    (x, V, ld, _, _, _, _, u), _ = _case(shape_i, 0)
    dx, du = dev(x), dev(u)
    for t in (1.0, 0.7):
        eos = int(np.argmax(x[0, :V]))
        want = _pick(lib, dx, V, ld, t, 1.0, 0.0, 0.0, du, eos=eos, plain=True)
        got = _pick(lib, dx, V, ld, t, 1.0, 0.0, 0.0, du, eos=eos)
        for k in ("tok", "seq", "len", "done"):
            assert np.array_equal(got[k], want[k]), (t, k)
        assert np.array_equal(got["lp"].view(np.uint64), want["lp"].view(np.uint64))
        assert (got["kept"] == V).all() and (got["ent"] == -7.0).all()   # (entropy is left untouched by the dispatch)


@pytest.mark.parametrize("shape_i", [0, 1, 2, 3, 4], ids=SHAPE_IDS)
def test_min_p_1_keeps_the_maxima_and_one_kept_word_is_the_first_maximum_whatever_u(lib, shape_i):
    """min_p = 1 keeps the maxima of y: one word on a row with a single maximum, every tied word otherwise (the rounded, the all-equal
    and the planted row), and then the draw picks among them.  tau = 1e-6 with min_p = 1 keeps one word on every row -- the intersection
    is the first maximum or empty, which falls back to it -- so the token is vc_argmax_rows_f32's whatever u."""
    from .gpu_util import P, dev, host, stream
    (x, V, ld, _, _, _, _, u), _ = _case(shape_i, 0)
    x = x.copy()
    x[20, :V] = -50.0
    x[20, [V // 3, V // 2, V - 1]] = 9.0       # a three-way tie at the top (rows 3 and 7: rounded and all-equal logits)
    dx = dev(x)
    ref = _i32(ty.ROWS)
    lib.vc_argmax_rows_f32(stream(), P(dx), ty.ROWS, V, ld, P(ref))
    ref = host(ref)
    assert ref[7] == 0 and ref[20] == V // 3
    n_max = (x[:, :V] == x[:, :V].max(1, keepdims=True)).sum(1)
    assert n_max[20] == 3 and n_max[7] == V
    single = n_max == 1
    for uu in (u, np.zeros_like(u), np.full_like(u, 0.999999)):
        for t in (1.0, 0.7):
            got = _pick(lib, dx, V, ld, t, 1.0, 1.0, 0.0, dev(uu))
            assert np.array_equal(got["kept"], n_max), t
            assert np.array_equal(got["tok"][single], ref[single]), t
            assert all(x[r, got["tok"][r]] == x[r, :V].max() for r in range(ty.ROWS))
            got = _pick(lib, dx, V, ld, t, 1e-6, 1.0, 0.0, dev(uu))
            assert np.array_equal(got["tok"], ref), t
            assert (got["kept"] == 1).all()


# ------------------------------------------------------------------ 3. bookkeeping and rounds
def test_pick_skips_ended_and_full_rows_and_rounds_select_uniforms(lib):
    from .gpu_util import P, dev, host, stream
    rng = np.random.default_rng(2)
    R, V, Rounds, cuts = 8, 50, 3, (0.9, 0.02, 1e-3)
    x = (rng.standard_normal((R, V)) * 4.0).astype(np.float32)
    u = rng.random((Rounds, R)).astype(np.float32)
    dx, du = dev(x), dev(u)
    done = dev(np.array([0, 1, 0, 1, 0, 0, 0, 0], np.int32))
    tok, seq, ln, rnd, kept = _i32(R), _i32(R * 4, fill=-1), _i32(R), _i32(1), _i32(R)
    ln[5] = 4   # a full row: nothing appended
    lp = torch.zeros(R, dtype=torch.float64, device="cuda")
    pending = torch.zeros(1, device="cuda")
    lsm = ty.log_softmax64(x)
    want_lp, toks = np.zeros(R), []
    for r in range(Rounds):
        ref = ty.typical_rows(x, 1.0, *cuts, u[r])
        assert all(q["safe"] for q in ref)
        lib.vc_decode_pick_typical_f32(stream(), P(dx), R, V, V, 1.0, *cuts, P(du), Rounds, P(rnd), -1, P(tok), P(done), P(seq), 4, P(ln), P(lp),
                                       P(kept), None)
        lib.vc_decode_round_end_i32(stream(), P(done), R, P(pending), P(rnd))
        t = host(tok)
        assert t.tolist() == [q["token"] for q in ref] and host(kept).tolist() == [q["kept"] for q in ref], r
        toks.append(t)
        want_lp += lsm[np.arange(R), t]
    assert len({tuple(t) for t in toks}) > 1   # (the rounds drew with different uniforms)
    assert int(host(rnd)[0]) == Rounds and float(host(pending)[0]) == 6.0
    assert host(ln).tolist() == [3, 0, 3, 0, 3, 4, 3, 3]
    S = host(seq).reshape(R, 4)
    assert (S[[1, 3, 5], :] == -1).all() and (host(lp)[[1, 3, 5]] == 0).all()
    live = [0, 2, 4, 6, 7]
    assert np.array_equal(S[live, :3], np.stack(toks, 1)[live]) and (S[live, 3] == -1).all()
    np.testing.assert_allclose(host(lp)[live], want_lp[live], rtol=0, atol=Rounds * ATOL_LP)
    # a round counter past the uniforms is clamped to the last round's
    lib.vc_decode_pick_typical_f32(stream(), P(dx), R, V, V, 1.0, *cuts, P(du), Rounds, P(rnd), -1, P(tok), P(done), P(seq), 4, P(ln), P(lp),
                                   None, None)
    assert np.array_equal(host(tok), toks[-1])


def test_the_stop_word_ends_a_row(lib):
    from .gpu_util import dev
    (x, V, ld, tau, min_p, eta, t, u), ref = _case(2, 4)
    eos = ref[0]["token"]
    got = _pick(lib, dev(x), V, ld, t, tau, min_p, eta, dev(u), eos=eos)
    assert got["done"][0] == 1 and np.array_equal(got["done"], (got["tok"] == eos).astype(np.int32))


# ------------------------------------------------------------------ 4. determinism and batch independence
@pytest.mark.parametrize("shape_i,setting_i", [(3, 4), (3, 0), (4, 0), (2, 3)], ids=["v10000-all", "v10000-tau", "unstaged-tau", "v1001-eta"])
def test_two_calls_agree_and_a_row_does_not_depend_on_the_batch(lib, shape_i, setting_i):
    from .gpu_util import dev
    (x, V, ld, tau, min_p, eta, t, u), _ = _case(shape_i, setting_i)
    dx, du = dev(x), dev(u)
    a = _pick(lib, dx, V, ld, t, tau, min_p, eta, du)
    b = _pick(lib, dx, V, ld, t, tau, min_p, eta, du)
    for k in ("tok", "kept", "seq", "len", "done"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["lp"].view(np.uint64), b["lp"].view(np.uint64)) and np.array_equal(a["ent"].view(np.uint32), b["ent"].view(np.uint32))
    part = _pick(lib, dev(x[8:24]), V, ld, t, tau, min_p, eta, dev(u[8:24]))
    assert np.array_equal(part["tok"], a["tok"][8:24]) and np.array_equal(part["kept"], a["kept"][8:24])
    assert np.array_equal(part["lp"].view(np.uint64), a["lp"][8:24].view(np.uint64))
    assert np.array_equal(part["ent"].view(np.uint32), a["ent"][8:24].view(np.uint32))
    one = _pick(lib, dev(x[63:]), V, ld, t, tau, min_p, eta, dev(u[63:]))
    assert one["tok"][0] == a["tok"][63] and one["kept"][0] == a["kept"][63]


# ------------------------------------------------------------------ 5. distribution
@pytest.mark.parametrize("cuts", [(0.8, 0.0, 0.0), (1.0, 0.1, 0.0), (0.9, 0.0, 0.02)], ids=["tau-0.8", "min_p-0.1", "tau-0.9-eta-0.02"])
def test_draws_follow_the_renormalised_distribution_of_the_kept_set(lib, cuts):
    """(the bound tests/test_gpu_trunc.py applies to its own distribution test: max |frequency - p| < 5e-3 over 200 000 draws)"""
    from .gpu_util import P, dev, host, stream
    n = 200000
    row = np.random.default_rng(3).standard_normal(16).astype(np.float32)
    lg = np.tile(row, (n, 1))
    uu = torch.empty(n, device="cuda")
    lib.vc_philox_uniform_f32(stream(), P(uu), n, 5, 0, None)
    tok, done, seq, ln, kept = _i32(n), _i32(n), _i32(n), _i32(n), _i32(n)
    lp = torch.zeros(n, dtype=torch.float64, device="cuda")
    lib.vc_decode_pick_typical_f32(stream(), P(dev(lg)), n, 16, 16, 1.0, *cuts, P(uu), 1, None, -1, P(tok), P(done), P(seq), 1, P(ln), P(lp),
                                   P(kept), None)
    want = ty.typical_probs(row, 1.0, *cuts)
    n_kept = int((want > 0).sum())
    assert 1 < n_kept < 16
    counts = np.bincount(host(tok), minlength=16)
    print("cuts %s: kept %d words; max |freq - p| = %.2e" % (cuts, n_kept, np.abs(counts / n - want).max()))
    assert counts[want == 0].sum() == 0                      # not one draw outside the kept set
    assert np.abs(counts / n - want).max() < 5e-3
    assert (host(kept) == n_kept).all()


# ------------------------------------------------------------------ 6. through the generator
def _ids(cands, B, K):
    return [[cands[b][k][0] for b in range(B)] for k in range(K)]


def _eps(rng, p, K, B):
    return rng.standard_normal((K, p.gen_z_samples, B, p.latent_size)).astype(np.float32)


def test_defaults_are_the_call_without_the_keywords(lib):
    p, eng, gen, P64, feats, cv, eps, cm = setup(lib, 13, prior="Normal")
    B, K, T = feats.shape[0], 4, 10
    rng = np.random.default_rng(8)
    p.temperature = 1.2
    u = rng.random((T, B)).astype(np.float32)
    off = dict(typical_p=1.0, min_p=0.0, eta=0.0)
    assert gen.sample(feats, None, eps, BOS, EOS, max_len=T, uniforms=u, **off) == gen.sample(feats, None, eps, BOS, EOS, max_len=T, uniforms=u)
    epsK, U = _eps(rng, p, K, B), rng.random((K, T, B)).astype(np.float32)
    a = gen.diverse(feats, None, epsK, BOS, EOS, draws=K, method="sample", max_len=T, uniforms=U)
    ca = gen.last_candidates
    n_graphs = len(gen._graphs) if hasattr(gen, "_graphs") else None
    b = gen.diverse(feats, None, epsK, BOS, EOS, draws=K, method="sample", max_len=T, uniforms=U, **off)
    assert a == b and ca == gen.last_candidates
    if n_graphs is not None:
        assert len(gen._graphs) == n_graphs   # (the same graph keys: nothing new was captured)


@pytest.mark.parametrize("kw", [dict(prior="Normal"), dict(no_encoder=True)], ids=["normal", "lstm"])
def test_min_p_1_is_greedy(lib, kw):
    p, eng, gen, P64, feats, cv, eps, cm = setup(lib, 13, **kw)
    B, K, T = feats.shape[0], 4, 10
    rng = np.random.default_rng(8)
    p.temperature = 0.8
    u = rng.random((T, B)).astype(np.float32)
    assert gen.sample(feats, None, eps, BOS, EOS, max_len=T, uniforms=u, min_p=1.0) == gen.greedy(feats, None, eps, BOS, EOS, max_len=T)
    epsK, U = _eps(rng, p, K, B), rng.random((K, T, B)).astype(np.float32)
    a = gen.diverse(feats, None, epsK, BOS, EOS, draws=K, method="sample", max_len=T, uniforms=U, min_p=1.0)
    ca = gen.last_candidates
    b = gen.diverse(feats, None, epsK, BOS, EOS, draws=K, method="greedy", max_len=T)
    assert a == b and ca == gen.last_candidates   # entries (tokens, scores, counts) and candidates (tokens, logprob, ended)


def test_diverse_draws_are_what_sample_gives_for_them_and_score_returns_their_logprob(lib):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 13, prior="Normal")
    B, K, T = feats.shape[0], 4, 10
    rng = np.random.default_rng(9)
    p.temperature = 1.3
    cuts = dict(typical_p=0.9, min_p=0.02, eta=1e-3)
    eps, U = _eps(rng, p, K, B), rng.random((K, T, B)).astype(np.float32)
    gen.diverse(feats, None, eps, BOS, EOS, draws=K, method="sample", max_len=T, uniforms=U, **cuts)
    cands = gen.last_candidates
    ref = CaptionGenerator(eng)
    assert _ids(cands, B, K) == [ref.sample(feats, None, eps[k], BOS, EOS, max_len=T, uniforms=U[k], **cuts) for k in range(K)]
    plain = [ref.sample(feats, None, eps[k], BOS, EOS, max_len=T, uniforms=U[k]) for k in range(K)]
    assert _ids(cands, B, K) != plain   # (at this temperature the cuts change some draw)
    got = gen.score(feats, [[[BOS] + toks for toks, _, _ in cands[b]] for b in range(B)], None, eps, BOS, EOS, draws=K)
    for b in range(B):
        for k in range(K):
            assert got[b][k]["tokens"] == len(cands[b][k][0])
            np.testing.assert_allclose(got[b][k]["logprob"][k], cands[b][k][1], **SUMS)


def test_another_setting_captures_its_own_chunk_and_returns_its_own_result(lib):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 23, no_encoder=True)
    B, K, T = feats.shape[0], 4, 11
    p.temperature = 1.5
    U = np.random.default_rng(3).random((K, T, B)).astype(np.float32)
    g = CaptionGenerator(eng)
    run = lambda gen, **kw: (gen.diverse(feats, None, None, BOS, EOS, draws=K, method="sample", max_len=T, uniforms=U, **kw),
                             _ids(gen.last_candidates, B, K))
    first = run(g, typical_p=0.9)
    again = run(g, typical_p=0.9)              # replayed chunks
    other = run(g, typical_p=0.3)              # same shapes and buffers, another cut: its own chunks
    floor = run(g, min_p=0.2)
    back = run(g, typical_p=0.9)
    assert again == first and back == first
    assert other == run(CaptionGenerator(eng), typical_p=0.3) and floor == run(CaptionGenerator(eng), min_p=0.2)
    assert other[1] != first[1] and floor[1] != first[1]
    # every token of the narrower cut is one the per-draw sample() call picks with the same settings
    ref = CaptionGenerator(eng)
    assert other[1] == [ref.sample(feats, None, None, BOS, EOS, max_len=T, uniforms=U[k], typical_p=0.3) for k in range(K)]


# ------------------------------------------------------------------ 7. command line
def test_main_synthetic_inference_with_typical_diverse_sampling(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    common = ["--synthetic", "--vocab", "200", "--embed_dim", "32", "--enc_hid", "64", "--dec_hid", "64", "--latent", "10",
              "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "ty"]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + common + ["--epochs", "1", "--max_steps", "1"],
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + common +
                       ["--mode", "inference", "--sample_gen", "diverse", "--diverse_method", "sample", "--typical_p", "0.9", "--eval_captions",
                        "--diverse_draws", "4", "--gen_name", "ty"], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    full = json.load(open(tmp_path / "val_ty_diverse.json"))
    coco = json.load(open(tmp_path / "val_ty.json"))
    assert len(full) == 8 and all(sum(x["counts"]) == 4 and len(x["captions"]) == len(x["scores"]) >= 1 for x in full)
    assert [x["caption"] for x in coco] == [x["captions"][0] for x in full]
    m = json.load(open(tmp_path / "val_ty_metrics.json"))
    assert (m["typical_p"], m["min_p"], m["eta"]) == (0.9, 0.0, 0.0) and m["diverse_method"] == "sample"
