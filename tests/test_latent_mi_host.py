"""CPU: the mutual-information checker (tests/latent_mi_ref.py) on Gaussian tables whose answer is known, the --bound_mi flag, the
header and the printed line store_bounds adds (the device call replaced by a recording stand-in), and the stand-alone host check of
vc_gauss_mix_lse_f64's argument contract (make mi-hostcheck: AddressSanitizer + UBSan on the host code, no GPU, no Python)."""
import contextlib
import io
import json
import math
import os
import subprocess

import numpy as np
import pytest

from vae_captioning_amd import latent_mi
from vae_captioning_amd.ops import inference as inf
from vae_captioning_amd.utils.parameters import Parameters

from . import latent_mi_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, L = 300, 3, 10


def _mi(mean, std, seed, samples=S):
    eps = np.random.default_rng(seed).standard_normal((mean.shape[0], samples, mean.shape[1])).astype(np.float32)
    r = ref.mutual_information(mean, std, eps)
    print("mi %.4f, mi_block %.4f (log N = %.4f)" % (r["mi"], r["mi_block"], r["mi_ceiling"]))
    assert r["captions"] == mean.shape[0] and r["mi_ceiling"] == math.log(mean.shape[0])
    return r


# ------------------------------------------------------------------ the checker on tables whose answer is known
# Both estimates take E_q[log q(z | x)] in closed form (h) and log q(z) from the draws.  Where a draw's own posterior carries the
# mixture (identical posteriors; separated ones), log q(z) - log q(z | x_n) is a constant and h[n] - log q(z_ns | x_n) =
# 0.5 (sum_l eps^2 - L), of variance L / 2 per block: the means have the standard errors below, and the checks allow four of them.
SE_BLOCK = math.sqrt(L / (2.0 * N * S))      # 0.075
SE_FULL = math.sqrt(S * L / (2.0 * N))       # 0.224


def test_identical_posteriors_carry_no_information():
    r = _mi(np.full((N, L), 0.3, np.float32), np.full((N, L), 0.1, np.float32), 1)   # away from the prior, all at one place: KL > 0, MI = 0
    assert abs(r["mi"]) < 4 * SE_FULL and abs(r["mi_block"]) < 4 * SE_BLOCK


def test_well_separated_posteriors_sit_at_the_ceiling():
    rng = np.random.default_rng(2)
    mean = (rng.standard_normal((N, L)) * 5.0).astype(np.float32)                     # 50 std apart per dimension
    r = _mi(mean, np.full((N, L), 0.1, np.float32), 3)
    assert abs(r["mi"] - math.log(N)) < 4 * SE_FULL and abs(r["mi_block"] - math.log(N)) < 4 * SE_BLOCK


def test_one_informative_dimension_lies_in_between_and_the_full_code_knows_more_than_a_block():
    rng = np.random.default_rng(4)
    mean = np.zeros((N, L), np.float32)
    mean[:, 0] = 5.0 * rng.standard_normal(N)                                         # a scalar Gaussian channel, signal / noise = 25
    r = _mi(mean, np.ones((N, L), np.float32), 5)
    block, full = 0.5 * math.log(1.0 + 25.0), 0.5 * math.log(1.0 + 25.0 * S)         # S looks at the same x: signal / noise = 25 S
    assert abs(r["mi_block"] - block) < 4 * SE_BLOCK and abs(r["mi"] - full) < 4 * SE_FULL
    assert 4 * SE_BLOCK < block < full < math.log(N) - 4 * SE_FULL                   # (the bands around 0, the two and log N are apart)
    assert r["mi_block"] < r["mi"]


def test_sharp_posteriors_are_finite_at_the_ceiling():
    rng = np.random.default_rng(6)
    mean = (rng.standard_normal((N, L)) * 0.1).astype(np.float32)
    r = _mi(mean, np.full((N, L), 1e-4, np.float32), 7)                               # the far terms underflow after the max is taken out
    assert math.isfinite(r["mi"]) and math.isfinite(r["mi_block"])
    assert abs(r["mi"] - math.log(N)) < 4 * SE_FULL and abs(r["mi_block"] - math.log(N)) < 4 * SE_BLOCK


def test_one_draw_per_caption_makes_the_block_the_code():
    rng = np.random.default_rng(8)
    mean = (rng.standard_normal((40, 4)) * 0.5).astype(np.float32)
    std = np.exp(rng.uniform(math.log(0.05), math.log(2.0), (40, 4))).astype(np.float32)
    r = _mi(mean, std, 9, samples=1)
    assert r["mi_block"] == r["mi"]
    z = ref.draws(mean, std, rng.standard_normal((40, 1, 4)))
    blk, full = ref.gauss_mix_lse(z, mean, std)
    assert np.array_equal(blk[:, 0], full)
    assert np.array_equal(latent_mi.block_entropy_term(std), ref.block_entropy_term(std))


def test_summarise_is_the_reference_s_arithmetic():
    rng = np.random.default_rng(10)
    mean, std = rng.standard_normal((9, 5)).astype(np.float32), np.exp(rng.standard_normal((9, 5))).astype(np.float32)
    z = ref.draws(mean, std, rng.standard_normal((9, 4, 5)))
    blk, full = ref.gauss_mix_lse(z, mean, std)
    assert latent_mi.summarise(blk, full, std) == ref.mutual_information(mean, std, z=z)


# ------------------------------------------------------------------ the flag
def test_bound_mi_flag_parses_and_refuses():
    assert Parameters().bound_mi == 0 and Parameters().parse_args([]).bound_mi == 0
    assert Parameters().parse_args(["--mode", "inference", "--bound_draws", "4"]).bound_mi == 0
    p = Parameters().parse_args(["--mode", "inference", "--bound_draws", "4", "--bound_mi", "5000"])
    assert p.bound_mi == 5000 and isinstance(p.bound_mi, int)
    assert Parameters().parse_args(["--mode", "inference", "--bound_draws", "4", "--bound_mi", "65536"]).bound_mi == 65536
    for bad in (["--mode", "inference", "--bound_draws", "4", "--bound_mi", "-1"],
                ["--mode", "inference", "--bound_draws", "4", "--bound_mi", "65537"],
                ["--mode", "inference", "--bound_mi", "16"],                                     # without --bound_draws
                ["--bound_draws", "4", "--bound_mi", "16"],                                      # training mode
                ["--mode", "inference", "--no_encoder", "--bound_draws", "4", "--bound_mi", "16"],
                ["--mode", "inference", "--bound_draws", "4", "--bound_mi", "16", "--gen_z_samples", "129"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            Parameters().parse_args(bad)


# ------------------------------------------------------------------ store_bounds on a stand-in for the device call
class _Params(object):
    gen_name, latent_size, gen_z_samples, seed = "mi", 4, 3, 77

    def __init__(self, bound_mi=0):
        self.bound_draws, self.bound_mi = 4, bound_mi


RECORDS = [{"image_id": 11, "captions": [{"tokens": 3, "elbo": -6.0, "iwae": -4.5, "rec": -3.0, "kl": 3.0, "ess": 3.0}]}]


def _stats(rows):
    mu = np.array([[0.0, 0.5 * i, 0.05 * i, 1.0] for i in range(rows)], np.float32).reshape(rows, 4)
    st = {"skipped_images": 2, "captions": rows, "mu_sum": mu.astype(np.float64).sum(0), "mu_sq": (mu.astype(np.float64) ** 2).sum(0)}
    return st, mu


def _store(tmp_path, monkeypatch, params, stats):
    calls = []

    def fake(mean, std, samples, eps=None, seed=0, lib=None):
        calls.append((np.array(mean), np.array(std), samples, eps, seed, lib))
        return {"mi": 1.25, "mi_block": 0.75, "mi_ceiling": math.log(len(mean)), "captions": len(mean)}

    monkeypatch.setattr(latent_mi, "mutual_information", fake)
    monkeypatch.chdir(tmp_path)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        header = inf.store_bounds(params, RECORDS, stats)
    recs = json.load(open(tmp_path / "val_mi_bound.json"))
    assert recs[0] == header and recs[1:] == RECORDS
    return header, out.getvalue().splitlines(), calls


TODAY = {"draws": 4, "skipped_images": 2, "active_units": 1, "latent_size": 4}


def test_store_bounds_adds_the_four_keys_and_the_line(tmp_path, monkeypatch):
    st, mu = _stats(3)
    st.update(mi_mean=[m for m in mu], mi_std=[np.full(4, 0.5 + i, np.float32) for i in range(3)])
    header, lines, calls = _store(tmp_path, monkeypatch, _Params(bound_mi=16), st)
    assert header == dict(TODAY, mi=1.25, mi_block=0.75, mi_captions=3, mi_ceiling=math.log(3))
    assert len(calls) == 1                                                            # once, at the end
    mean, std, samples, eps, seed, lib = calls[0]
    assert np.array_equal(mean, mu) and np.array_equal(std, np.array([[0.5] * 4, [1.5] * 4, [2.5] * 4], np.float32))
    assert mean.dtype == std.dtype == np.float32
    assert samples == 3 and eps is None and seed == 77                               # gen_z_samples draws, seeded by params.seed
    assert len(lines) == 7                                                            # "wrote ...", today's five and the new one
    assert lines[-1] == ("Mutual information of caption and latent code: mi 1.250000 nats, mi_block 0.750000 nats per block "
                         "(mi_ceiling %.6f = log of mi_captions 3)" % math.log(3))
    assert all(k in lines[-1] for k in ("mi ", "mi_block", "mi_captions", "mi_ceiling"))


def test_store_bounds_without_mi_statistics_is_today_s(tmp_path, monkeypatch):
    st, _ = _stats(3)
    for params, stats in ((_Params(), st),                                            # flag off
                          (_Params(bound_mi=16), st),                                 # flag on, nothing kept (a decoder that keeps none)
                          (_Params(bound_mi=16), dict(st, mi_mean=[], mi_std=[])),    # flag on, every image skipped
                          (_Params(), dict(st, mi_mean=[np.zeros(4, np.float32)], mi_std=[np.ones(4, np.float32)]))):   # kept, flag off
        header, lines, calls = _store(tmp_path, monkeypatch, params, stats)
        assert header == TODAY and not calls
        assert len(lines) == 6 and lines[-1] == "Active latent units: 1 of 4 (2 images without a cluster vector skipped)"
        assert not any("Mutual information" in ln for ln in lines)
    header, lines, calls = _store(tmp_path, monkeypatch, _Params(bound_mi=16), None)  # nothing was bounded at all
    assert header == dict(TODAY, skipped_images=0, active_units=0) and not calls


# ------------------------------------------------------------------ the stand-alone host check
def test_gauss_mix_lse_argument_checks_under_the_host_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "vae_captioning_amd", "csrc"), "mi-hostcheck", "OBJ=%s" % tmp_path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "gauss mix lse argument checks: all passed" in r.stdout
    assert "FAIL" not in r.stdout + r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
