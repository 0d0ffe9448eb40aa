"""CPU: the posterior bounds' checker (tests/bound_ref.py) obeys the identities of DESIGN.md "Bounds", the --bound_draws flag parses and
refuses as documented, and the inference driver writes ./val_{gen_name}_bound.json -- and nothing new with the flag off -- on recording
stand-ins for its decoder and batch generator."""
import contextlib
import io
import json
import math
import os

import numpy as np
import pytest

from vae_captioning_amd.ops import inference as inf
from vae_captioning_amd.utils.parameters import Parameters

from . import bound_ref as ref
from . import score_ref

EOS = 2


# ------------------------------------------------------------------ the checker's identities
@pytest.mark.parametrize("K", [1, 2, 7, 256])
def test_reduction_identities_on_random_terms(K):
    rng = np.random.default_rng(K)
    for spread in (0.1, 5.0, 300.0):
        lp, lw = -rng.random(K) * spread - 1.0, rng.standard_normal(K) * spread
        r = ref.reduce(lp, lw)
        assert r["iwae"] >= r["elbo"] - 1e-12 * max(1.0, abs(r["elbo"]))          # Jensen: log-mean-exp >= mean
        assert 1.0 - 1e-12 <= r["ess"] <= K + 1e-9
        assert abs(r["elbo"] - (r["rec"] - r["kl_mc"])) <= 1e-12 * max(1.0, abs(r["rec"]) + abs(r["kl_mc"]))
        if K == 1:
            assert abs(r["iwae"] - r["elbo"]) <= 1e-14 * max(1.0, abs(r["elbo"])) and r["ess"] == 1.0
    same = ref.reduce(np.full(K, -3.5), np.full(K, -1.25))                         # equal weights: no gap, full sample size
    assert abs(same["iwae"] - same["elbo"]) <= 1e-13 and abs(same["ess"] - K) <= 1e-9 * K


def test_the_prior_as_proposal_has_unit_weights_and_gives_score_s_marginal():
    rng = np.random.default_rng(3)
    K, S, L, sp = 6, 4, 10, float(np.float32(0.1))
    pm = rng.standard_normal(L) * 0.05
    eps = rng.standard_normal((K, S, L))
    z = pm[None, None] + sp * eps
    lw = np.array([ref.logw(z[k], eps[k], np.full(L, sp), pm, sp) for k in range(K)])
    scale = 0.5 * (eps ** 2).sum(axis=(1, 2))                                      # the size of the terms that cancel
    assert (np.abs(lw) <= 1e-13 * scale).all(), lw                                 # (z - pm) / sp == eps to float64 rounding
    assert abs(ref.kl(pm, np.full(L, sp), pm, sp, S)) <= 1e-13
    lp = -rng.random(K) * 40
    assert abs(ref.reduce(lp, lw)["iwae"] - score_ref.marginal(lp)) <= 1e-12


def test_monte_carlo_kl_agrees_with_the_closed_form_within_five_standard_errors():
    rng = np.random.default_rng(2016)
    n, S, L, sp = 200000, 1, 3, 0.1
    mean, std, pm = np.array([0.03, -0.08, 0.0]), np.array([0.02, 0.1, 0.25]), np.array([0.01, 0.0, -0.02])
    eps = rng.standard_normal((n, S, L))
    z = mean[None, None] + std[None, None] * eps
    sample = -ref.logw_terms(z.reshape(n, L), eps.reshape(n, L), std, pm, sp).sum(axis=1)   # -logw of every draw
    closed = ref.kl(mean, std, pm, sp, S)
    se = sample.std(ddof=1) / math.sqrt(n)
    print("closed-form KL %.6f, Monte-Carlo %.6f +- %.6f (one standard error)" % (closed, sample.mean(), se))
    assert closed > 1.0 and abs(sample.mean() - closed) <= 5 * se


# ------------------------------------------------------------------ the flag
def test_bound_draws_flag_parses_and_refuses():
    assert Parameters().bound_draws == 0 and Parameters().parse_args([]).bound_draws == 0
    p = Parameters().parse_args(["--mode", "inference", "--bound_draws", "20"])
    assert p.bound_draws == 20 and isinstance(p.bound_draws, int)
    assert Parameters().parse_args(["--mode", "inference", "--bound_draws", "256", "--score_draws", "3"]).bound_draws == 256
    for bad in (["--mode", "inference", "--bound_draws", "257"], ["--mode", "inference", "--bound_draws", "-1"],
                ["--bound_draws", "4"],                                            # training mode
                ["--mode", "inference", "--no_encoder", "--bound_draws", "4"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            Parameters().parse_args(bad)
    assert Parameters().parse_args(["--mode", "inference", "--no_encoder"]).bound_draws == 0   # off: nothing to refuse


# ------------------------------------------------------------------ the driver on stand-ins
class _Params(object):
    checkpoint, fine_tune, beam_size, gen_name, sample_gen, prior, use_c_v, latent_size = "ck", False, 3, "bd", "greedy", "AG", False, 4

    def __init__(self, bound_draws=0, score_draws=0):
        self.bound_draws, self.score_draws = bound_draws, score_draws


class _Val(object):
    """two validation batches with label rows `w.. <EOS>` (two captions per image, then one)"""
    lab = np.array([[[5, 6, EOS, 0], [7, EOS, 0, 0]], [[8, 9, 9, EOS], [0, 0, 0, 0]], [[3, EOS, 0, 0], [4, 4, EOS, 0]]], np.int32)
    lens = np.array([[3, 2], [4, 0], [2, 3]], np.int32)

    def next_val_batch(self, get_image_ids=True, use_obj_vectors=False):
        cv = np.zeros((2, 91), np.float32)
        cv[:, 0], cv[0, 5] = 1000.0, 1.0                                           # image 12 has no cluster vector
        yield np.ones((2, 4), np.float32), (self.lab[:2], self.lab[:2]), self.lens[:2], [11, 12], cv
        yield np.ones((1, 4), np.float32), (self.lab[2:, 0], self.lab[2:, 0]), self.lens[2:, 0], [13], np.full((1, 91), 0.5, np.float32)


class _Decoder(object):
    """records every call; bound_captions behaves as the facade documents: images without a cluster vector are skipped and counted"""
    def __init__(self):
        self.trace, self.bound_stats = [], None

    def online_inference(self, sess, ids, images, placeholder, c_v=None):
        self.trace.append(["online_inference", list(ids)])
        return [{"image_id": int(i), "caption": "c%d" % i} for i in ids], None

    def score_captions(self, ids, images, captions, c_v=None, draws=None):
        self.trace.append(["score_captions", list(ids), draws])
        return [{"image_id": int(i), "captions": [{"tokens": len(t), "marginal": -1.0 * len(t), "logprob": -1.5 * len(t)} for t in cl]}
                for i, cl in zip(ids, captions)]

    def bound_captions(self, ids, images, captions, c_v=None, draws=None):
        self.trace.append(["bound_captions", list(ids), [[list(t) for t in cl] for cl in captions], list(np.asarray(c_v).shape), draws])
        st = self.bound_stats = self.bound_stats or {"skipped_images": 0, "captions": 0, "mu_sum": np.zeros(4), "mu_sq": np.zeros(4)}
        out = []
        for b, (i, cl) in enumerate(zip(ids, captions)):
            if not np.asarray(c_v)[b].any():
                st["skipped_images"] += 1
                continue
            for t in cl:
                mu = np.array([0.0, 0.5 * len(t), 0.05 * len(t), 1.0])              # dimension 1 varies a lot, 2 a little, 0 and 3 not
                st["mu_sum"] += mu
                st["mu_sq"] += mu * mu
                st["captions"] += 1
            out.append({"image_id": int(i), "captions": [{"tokens": len(t), "elbo": -2.0 * len(t), "iwae": -1.5 * len(t), "rec": -1.0 * len(t),
                                                           "kl": 1.0 * len(t), "ess": 1.0 + 0.5 * draws} for t in cl]})
        return out


def _drive(tmp_path, monkeypatch, **kw):
    monkeypatch.chdir(tmp_path)
    dec, out = _Decoder(), io.StringIO()
    with contextlib.redirect_stdout(out):
        inf.inference(_Params(**kw), dec, _Val(), None)
    return dec, out.getvalue()


def test_driver_writes_the_bound_file_with_the_documented_keys(tmp_path, monkeypatch):
    dec, out = _drive(tmp_path, monkeypatch, bound_draws=4, score_draws=2)
    calls = [c for c in dec.trace if c[0] == "bound_captions"]
    assert [c[1] for c in calls] == [[11, 12], [13]] and all(c[4] == 4 for c in calls)
    assert calls[0][2] == [[[5, 6, EOS], [7, EOS]], [[8, 9, 9, EOS]]] and calls[1][2] == [[[3, EOS]]]     # the human captions, <EOS> included
    assert calls[0][3] == [2, 90]                                                  # columns 1..90 of the generator's 91-vectors
    recs = json.load(open(tmp_path / "val_bd_bound.json"))
    assert recs[0] == {"draws": 4, "skipped_images": 1, "active_units": 1, "latent_size": 4}
    assert [r["image_id"] for r in recs[1:]] == [11, 13]
    for r in recs[1:]:
        assert set(r) == {"image_id", "captions"}
        assert all(set(c) == {"tokens", "elbo", "iwae", "rec", "kl", "ess"} for c in r["captions"])
    assert [[c["tokens"] for c in r["captions"]] for r in recs[1:]] == [[3, 2], [2]]
    lines = out.splitlines()
    for want in ("Perplexity bound of the human captions from the importance-weighted bound, 4 posterior draws: %.17g" % math.exp(1.5),
                 "Perplexity bound of the human captions from the ELBO, 4 posterior draws: %.17g" % math.exp(2.0),
                 "Mean KL(q || p) per caption: %.6f nats" % (7.0 / 3.0), "Mean effective sample size / draws: %.6f" % 0.75,
                 "Active latent units: 1 of 4 (1 images without a cluster vector skipped)"):
        assert want in lines, (want, lines)
    assert (tmp_path / "val_bd_scores.json").exists() and (tmp_path / "val_bd.json").exists()


def test_driver_writes_nothing_new_with_the_flag_off(tmp_path, monkeypatch):
    dec, out = _drive(tmp_path, monkeypatch, score_draws=2)
    assert not any(c[0] == "bound_captions" for c in dec.trace)
    assert sorted(os.listdir(tmp_path)) == ["val_bd.json", "val_bd_scores.json"]
    assert "bound" not in out and "Active latent units" not in out and "KL" not in out
    dec, out = _drive(tmp_path, monkeypatch)
    assert [c[0] for c in dec.trace] == ["online_inference", "online_inference"]


# ------------------------------------------------------------------ the driver's arithmetic
def test_perplexity_bounds_and_active_units_on_hand_made_records():
    recs = [{"image_id": 1, "captions": [{"tokens": 4, "elbo": -10.0, "iwae": -8.0, "rec": -7.0, "kl": 3.0, "ess": 2.0},
                                         {"tokens": 6, "elbo": -20.0, "iwae": -12.0, "rec": -15.0, "kl": 5.0, "ess": 4.0}]},
            {"image_id": 2, "captions": []}]
    ppl_iwae, ppl_elbo, kl, ess = inf.bound_summary(recs, 4)
    assert ppl_iwae == math.exp(20.0 / 10.0) and ppl_elbo == math.exp(30.0 / 10.0) and kl == 4.0 and ess == 0.75
    assert ppl_iwae <= ppl_elbo
    assert all(math.isnan(v) for v in inf.bound_summary([{"image_id": 2, "captions": []}], 4))
    # three captions, two dimensions: means (0, 0.3), (0, 0.6), (0.15, 0.0) -> variances 0.005 (inactive) and 0.06 (active)
    mu = np.array([[0.0, 0.3], [0.0, 0.6], [0.15, 0.0]])
    assert np.allclose(mu.var(axis=0), [0.005, 0.06])
    assert inf.active_units(mu.sum(0), (mu * mu).sum(0), 3) == 1
    assert inf.active_units(mu.sum(0), (mu * mu).sum(0), 3, threshold=0.001) == 2
    assert inf.active_units(np.zeros(2), np.zeros(2), 0) == 0
