"""-m gpu: the training objective options (free bits, KL weight, cyclical annealing, label smoothing) -- their kernels through
the C ABI against the float64 reference (tests/objective_ref.py), whole training steps against float64 autograd, and the promise
that every option at its default launches exactly what was launched before.

Tolerances are those of the plain forms' tests: 1e-5 of the tensor maximum for the KL, latent-backward and cross-entropy kernels
(tests/test_gpu_ops.py), 2e-4 relative on losses and 2e-4 of each tensor's maximum on gradients for whole steps
(tests/test_gpu_engine.py).  Integer results (the floored counts) and everything compared between two runs of the same kernels are exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import spec, synth
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.trainer import Trainer

from . import objective_ref as R
from .gpu_util import P, assert_close, dev, host, stream, zeros
from .test_gpu_engine import make_case, small_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("vc_softmax_xent_smooth_f32", "vc_kl_rows_fb_f32", "vc_latent_bwd_fb_f32", "vc_objective_stats_f32",
               "vc_loss_finalize_kl_f32", "vc_step_update_cyclical")


# ------------------------------------------------------------------------------------------------ KL kernels
@pytest.mark.parametrize("shape", R.KL_SHAPES, ids=lambda s: "N%d-L%d-mode%d" % s)
def test_free_bits_kl_rows(lib, shape):
    N, L, mode = shape
    c = R.kl_case(N, L, mode)
    rk, raw, nf = zeros(N), zeros(N), torch.full((N,), -1, dtype=torch.int32, device="cuda")
    lib.vc_kl_rows_fb_f32(stream(), N, L, mode, P(dev(c["mean"])), P(dev(c["std"])), P(dev(c["mu_p"])), c["lam"], P(rk), P(raw), P(nf))
    np.testing.assert_array_equal(host(nf), c["row_floored"])
    assert_close(host(rk), c["row_kl"], 1e-5, msg="row_kl")
    assert_close(host(raw), c["row_raw"], 1e-5, atol_scale=np.abs(c["row_kl"]).max(), msg="row_kl_raw")
    # the unclamped sum is the plain entry's row KL
    plain = zeros(N)
    lib.vc_kl_rows_f32(stream(), N, L, mode, P(dev(c["mean"])), P(dev(c["std"])), P(dev(c["mu_p"])), P(plain))
    assert_close(host(raw), host(plain), 1e-5, atol_scale=np.abs(c["row_kl"]).max(), msg="row_kl_raw vs vc_kl_rows_f32")
    st = zeros(2)
    lib.vc_objective_stats_f32(stream(), N, L, P(raw), P(nf), P(st))
    np.testing.assert_allclose(host(st), [host(raw).astype(np.float64).mean(), c["row_floored"].sum() / (N * L)], rtol=1e-5)


@pytest.mark.parametrize("shape", R.KL_SHAPES, ids=lambda s: "N%d-L%d-mode%d" % s)
def test_free_bits_latent_bwd(lib, shape):
    N, L, mode = shape
    c = R.kl_case(N, L, mode)
    ann, kl_scale = 0.37, (0.1 / N if mode == 0 else 0.1)
    annd = dev(np.array([ann], np.float32))
    w = float(np.float32(ann)) * float(np.float32(kl_scale))
    fl = c["kl"] <= c["lam"]
    rng = np.random.default_rng(N + L + mode)
    pre_m, pre_s = rng.standard_normal((N, L), dtype=np.float32), rng.standard_normal((N, L), dtype=np.float32)
    dmean, dstd, dmu = dev(c["mean"]), dev(c["std"]), dev(c["mu_p"])
    for S in (0, 5, 9):          # the "already summed" path, the tail loop alone, the unrolled loop plus tail
        dz, eps = np.ascontiguousarray(c["dz"][:S]), np.ascontiguousarray(c["eps"][:S])
        ddz, deps = (dev(dz), dev(eps)) if S else (None, None)
        for out_logstd in (0, 1):
            def run(entry, scale, *fb):
                dm, ds = dev(pre_m.copy()), dev(pre_s.copy())   # S > 0 overwrites them, S == 0 adds to them
                entry(stream(), S, N, L, mode, out_logstd, P(ddz), P(deps), P(dmean), P(dstd), P(dmu), P(annd), scale, *fb, P(dm), P(ds))
                return host(dm), host(ds)
            gm, gs = run(lib.vc_latent_bwd_fb_f32, kl_scale, c["lam"])
            pre = dict(dmean0=pre_m, dstd0=pre_s) if S == 0 else {}
            rm, rs = R.latent_bwd(mode, out_logstd, dz, eps, c["mean"], c["std"], c["mu_p"], w, c["lam"], **pre)
            tag = "S=%d logstd=%d" % (S, out_logstd)
            assert_close(gm, rm, 1e-5, msg="dmean " + tag)
            assert_close(gs, rs, 1e-5, msg="dstd " + tag)
            # floored elements carry the sums over the samples alone: the plain entry with kl_scale = 0, bit for bit
            zm, zs = run(lib.vc_latent_bwd_f32, 0.0)
            np.testing.assert_array_equal(gm[fl], zm[fl], err_msg="floored dmean " + tag)
            np.testing.assert_array_equal(gs[fl], zs[fl], err_msg="floored dstd " + tag)
            assert (gm[~fl] != zm[~fl]).any(), "no KL gradient anywhere: " + tag


# ------------------------------------------------------------------------------------------------ smoothed cross-entropy
def _xent_buffers(V, ld, off, R_):
    buf, labels = R.xent_case(V, ld, off, R_)
    flat = torch.zeros(R_ * ld + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + R_ * ld].view(R_, ld)
    view.copy_(torch.from_numpy(buf))
    return buf, labels, flat, view


@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("shape", R.XENT_SHAPES, ids=lambda s: "V%d-ld%d-off%d-R%d" % s)
def test_smoothed_xent(lib, shape, eps):
    V, ld, off, R_ = shape
    buf, labels, flat, view = _xent_buffers(V, ld, off, R_)
    gscale = 3.0
    loss_ref, d_ref = R.smooth_xent(buf[:, :V], labels, eps, gscale)
    dl, den, rl = dev(labels), zeros(1), zeros(R_)
    lib.vc_count_nonzero_i32(stream(), P(dl), R_, P(den))
    nden = float((labels != 0).sum())
    # forward only: the logits -- padding included -- stay as they are
    lib.vc_softmax_xent_smooth_f32(stream(), view.data_ptr(), P(dl), R_, V, ld, P(den), gscale, eps, P(rl), 0)
    np.testing.assert_array_equal(host(view), buf)
    np.testing.assert_allclose(host(rl).astype(np.float64).sum() / nden, loss_ref.sum() / nden, rtol=1e-5)
    assert_close(host(rl), loss_ref, 1e-5, msg="row_loss")
    assert host(rl)[0] == 0.0   # the PAD row
    rl.fill_(-1.0)
    lib.vc_softmax_xent_smooth_f32(stream(), view.data_ptr(), P(dl), R_, V, ld, P(den), gscale, eps, P(rl), 1)
    got = host(view)
    assert_close(host(rl), loss_ref, 1e-5, msg="row_loss (with gradient)")
    assert_close(got[:, :V], d_ref, 1e-5, msg="dlogits")
    assert (got[:, V:] == 0).all(), "pitch padding must come back exactly 0"
    assert (got[0] == 0).all()   # PAD row
    assert (host(flat)[:off] == 0).all() and (host(flat)[off + R_ * ld:] == 0).all()   # nothing outside the rows


@pytest.mark.parametrize("shape", R.XENT_SHAPES, ids=lambda s: "V%d-ld%d-off%d-R%d" % s)
def test_smoothed_xent_with_tiny_eps_is_the_plain_loss(lib, shape):
    V, ld, off, R_ = shape
    buf, labels, flat, view = _xent_buffers(V, ld, off, R_)
    dl, den, a, b = dev(labels), zeros(1), zeros(R_), zeros(R_)
    lib.vc_count_nonzero_i32(stream(), P(dl), R_, P(den))
    lib.vc_softmax_xent_f32(stream(), view.data_ptr(), P(dl), R_, V, ld, P(den), 1.0, P(a), 0)
    lib.vc_softmax_xent_smooth_f32(stream(), view.data_ptr(), P(dl), R_, V, ld, P(den), 1.0, 1e-30, P(b), 0)
    np.testing.assert_allclose(host(b).astype(np.float64).sum(), host(a).astype(np.float64).sum(), rtol=1e-5)
    assert_close(host(b), host(a), 1e-5, msg="row_loss")


# ------------------------------------------------------------------------------------------------ schedule, finalize
def test_cyclical_step_update(lib):
    """scalars[1] is the cyclical coefficient; every other scalar and the counter are vc_step_update's, to the bit"""
    Pd, Rr, M = 1000, 0.25, 3
    for gs in (0, 1, 249, 250, 251, 999, 1000, 1001, 2999, 3000, 3001, 50000):
        a, b = zeros(8), zeros(8)
        sa, sb = dev(np.array([gs], np.int32)), dev(np.array([gs], np.int32))
        lib.vc_step_update(stream(), P(sa), P(a), 5e-4, 1e-5, 0.8, 0.999, 0.0, 0, 700)
        lib.vc_step_update_cyclical(stream(), P(sb), P(b), 5e-4, 1e-5, 0.8, 0.999, 700, Pd, Rr, M)
        ha, hb = host(a), host(b)
        assert int(host(sa)[0]) == int(host(sb)[0]) == gs + 1
        np.testing.assert_array_equal(np.delete(ha, 1), np.delete(hb, 1))
        assert ha[1] == 1.0
        np.testing.assert_allclose(hb[1], R.cyclical_ann(gs, Pd, Rr, M), rtol=1e-6, atol=0)
    b, sb = zeros(8), dev(np.array([3000], np.int32))
    lib.vc_step_update_cyclical(stream(), P(sb), P(b), 5e-4, 1e-5, 0.8, 0.999, 700, Pd, Rr, 0)   # M = 0: forever
    assert host(b)[1] == 0.0


def test_loss_finalize_with_kl_coefficient(lib):
    red = dev(np.array([30.0, 6.0, 8.0, 0.0], np.float32))
    ann, out, out0 = dev(np.array([0.6], np.float32)), zeros(4), zeros(4)
    lib.vc_loss_finalize_kl_f32(stream(), P(red), red.data_ptr() + 4, None, 0.0, red.data_ptr() + 8, 0.25, P(ann), 0.05, P(out))
    np.testing.assert_allclose(host(out), [5.0, 2.0, 5.0 + 0.6 * 0.05 * 2.0, 0.6], rtol=1e-6)
    lib.vc_loss_finalize_f32(stream(), P(red), red.data_ptr() + 4, None, 0.0, red.data_ptr() + 8, 0.25, P(ann), P(out0))
    lib.vc_loss_finalize_kl_f32(stream(), P(red), red.data_ptr() + 4, None, 0.0, red.data_ptr() + 8, 0.25, P(ann), 0.1, P(out))
    np.testing.assert_allclose(host(out), host(out0), rtol=1e-6)   # kl_coef = 1 / 10: the plain lower bound


# ------------------------------------------------------------------------------------------------ whole steps
PRIORS = {"Normal": dict(prior="Normal"), "GMM": dict(prior="GMM"), "AG_cv": dict(prior="AG", use_c_v=True)}
# seeds at which the float64 reference keeps every kl[n,l] of all three steps at least 1e-4 away from the floor (found with the
# reference alone; asserted below)
SEEDS = {("Normal", "all"): 9, ("Normal", "free_bits"): 8, ("GMM", "free_bits"): 8}


@pytest.mark.parametrize("options", list(R.STEP_OPTIONS), ids=str)
@pytest.mark.parametrize("prior", list(PRIORS), ids=str)
def test_train_steps_with_options_match_autograd(lib, prior, options):
    p = small_params(**PRIORS[prior], **R.STEP_OPTIONS[options])
    V, B, T = 203, 4, 6
    P0, batch, noise = make_case(p, V, B, T, seed=SEEDS.get((prior, options), 7))
    hist, Pref = R.reference_steps(p, P0, batch, noise, 3)
    eng = CaptionEngine(p, V, lib=lib)
    eng.load_params(P0)
    for s, h in enumerate(hist):
        if p.kl_free_bits > 0:
            assert h["tie_margin"] >= 1e-4, ("reference element on the floor at step %d: reseed" % s, h["tie_margin"])
        eng.set_batch(batch, noise)
        eng.forward()
        eng.backward()
        eng.pack_tail()
        G = eng.grads_dict()
        for name, ref in h["grads"].items():
            tol = 2e-4 * (np.abs(ref).max() + 1e-12)
            err = np.abs(G[name] - ref).max()
            assert err <= tol, "step %d grad %s: err %.3e tol %.3e (max %.3e)" % (s, name, err, tol, np.abs(ref).max())
        eng.apply_gradients()
        kld, rec, lb, ann = eng.losses()
        assert ann == pytest.approx(h["ann"], abs=1e-7), ("annealing step %d" % s, ann, h["ann"])
        assert abs(rec - h["rec"]) <= 2e-4 * abs(h["rec"]), ("rec_loss step %d" % s, rec, h["rec"])
        assert abs(kld - h["kld"]) <= 2e-4 * abs(h["kld"]) + 1e-6, ("kld step %d" % s, kld, h["kld"])
        assert abs(lb - h["lb"]) <= 2e-4 * abs(h["lb"]), ("lower_bound step %d" % s, lb, h["lb"])
        norm = float(eng.ns[0].item())
        assert abs(norm - h["norm"]) <= 3e-4 * h["norm"], ("global norm step %d" % s, norm, h["norm"])
        assert h["norm"] > p.lstm_clip_by_norm, "clip not active in this case"
        o = eng.objective_stats()
        if p.kl_free_bits > 0:
            assert abs(o["kl_raw"] - h["kl_raw"]) <= 2e-4 * abs(h["kl_raw"]) + 1e-6
            assert o["floored_share"] == pytest.approx(h["floored_share"], abs=1e-6)
        else:
            assert o is None
    Pg = eng.state_dict()
    for name, ref in Pref.items():
        upd = np.abs(ref - P0[name]).max()
        err = np.abs(Pg[name] - ref).max()
        assert err <= 2e-3 * upd + 1e-7, "param %s after 3 steps: err %.3e, update size %.3e" % (name, err, upd)


def test_validation_forward_keeps_the_plain_loss(lib):
    """fw_loss(train=False) -- Trainer.eval_rec_loss -- is unsmoothed whatever --label_smoothing says"""
    V, B, T = 203, 4, 6
    rec = []
    for eps in (0.0, 0.3):
        p = small_params(prior="Normal", label_smoothing=eps)
        P0, batch, noise = make_case(p, V, B, T, seed=7)
        eng = CaptionEngine(p, V, lib=lib)
        eng.load_params(P0)
        eng.set_batch(batch, noise)
        eng.forward(train=False)
        rec.append(eng.losses()[1])
    assert rec[0] == rec[1]


# ------------------------------------------------------------------------------------------------ off means off
class _NoNewEntries(object):
    """the loaded library, except that resolving any entry of this feature is an error"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in NEW_ENTRIES:
            raise AssertionError("%s resolved with every objective option at its default" % name)
        return getattr(self._lib, name)


def test_defaults_launch_none_of_the_new_entries(lib):
    guard = _NoNewEntries(lib)
    with pytest.raises(AssertionError):
        guard.vc_kl_rows_fb_f32
    V, B, T = 203, 4, 6
    for kw in PRIORS.values():
        p = small_params(**kw)
        P0, batch, noise = make_case(p, V, B, T, seed=7)
        eng = CaptionEngine(p, V, lib=guard)
        eng.load_params(P0)
        for _ in range(3):
            eng.set_batch(batch, noise)
            eng.forward(); eng.backward(); eng.pack_tail(); eng.apply_gradients()
        assert all(np.isfinite(eng.losses())) and eng.objective_stats() is None
    p = small_params(prior="Normal")
    tr = Trainer(p, V, lib=guard, seed=3)
    tr.load_state_dict(spec.init_caption_params(p, V, seed=8))
    tr.set_batch(synth.make_batch(np.random.default_rng(2), B, p.num_captions, T, V, variable_len=True, feature_size=p.cnn_feature_size))
    tr.capture(warmup=1)
    tr.train_step()
    assert all(np.isfinite(tr.losses())) and tr.eval_rec_loss() > 0


def test_options_resolve_the_new_entries(lib):
    """... and the guard is not vacuous: with the options on, the same steps do go through them"""
    p = small_params(prior="Normal", **R.ALL_ON)
    P0, batch, noise = make_case(p, 203, 4, 6, seed=7)
    eng = CaptionEngine(p, 203, lib=_NoNewEntries(lib))
    eng.load_params(P0)
    eng.set_batch(batch, noise)
    with pytest.raises(AssertionError, match="vc_step_update_cyclical"):
        eng.forward()


# ------------------------------------------------------------------------------------------------ capture, collectives, CLI
def test_captured_step_with_every_option_equals_eager(lib):
    p = small_params(prior="Normal", **R.ALL_ON)
    V, B, T = 203, 4, 6
    rng = np.random.default_rng(31)
    P0 = spec.init_caption_params(p, V, seed=4)
    batches = [synth.make_batch(rng, B, p.num_captions, T, V, variable_len=True, feature_size=p.cnn_feature_size) for _ in range(3)]
    res = []
    for graph in (False, True):
        tr = Trainer(p, V, lib=lib, seed=9)
        tr.load_state_dict(P0)
        tr.set_batch(batches[0])
        if graph:
            tr.capture(warmup=1)
            tr.cap.step.zero_()      # the warm-up ran the step once: rewind to the same starting point
            tr.load_state_dict(P0)
            for s in tr.cap.store.slots.values():
                s.zero_()
        losses = []
        for b in batches:
            tr.set_batch(b)
            tr.train_step()
            losses.append(tr.losses() + (tr.objective_stats()["kl_raw"], tr.objective_stats()["floored_share"]))
        res.append((losses, tr.state_dict()))
    assert res[0][0] == res[1][0]
    assert [l[3] for l in res[1][0]] == [0.0, 1.0, 0.0]   # the schedule advances inside the replayed graph
    for k in res[0][1]:
        np.testing.assert_array_equal(res[0][1][k], res[1][1][k], err_msg=k)


def test_forced_single_rank_collectives_with_every_option(lib):
    """the deferred finalisation behind the gradient all-reduce (apply_gradients) reports what the plain engine reports"""
    p = small_params(prior="Normal", **R.ALL_ON)
    V, B, T = 203, 4, 6
    P0, batch, noise = make_case(p, V, B, T, seed=9)
    res = []
    for force in (False, True):
        tr = Trainer(p, V, lib=lib, force_collectives=force)
        tr.load_state_dict(P0)
        for _ in range(2):     # the second step has annealing 1: the KL term is in the bound
            tr.set_batch(batch, noise)
            tr.train_step()
        res.append(tr.losses())
        if tr.comm is not None:
            tr.comm.destroy()
    assert res[0][3] == res[1][3] == 1.0
    for a, b in zip(res[0], res[1]):
        assert abs(a - b) <= 2e-4 * abs(a), (res[0], res[1])


def test_main_cli_with_every_flag(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "120", "--bs", "2", "--embed_dim", "32", "--enc_hid", "32",
           "--dec_hid", "32", "--latent", "8", "--gen_z_samples", "3", "--gpu", "0", "--checkpoint", "objtest", "--ckpt_format", "npz",
           "--epochs", "1", "--max_steps", "2", "--kl_free_bits", "0.05", "--kl_weight", "0.5", "--kl_cycle_steps", "2", "--kl_cycle_ramp", "0.5",
           "--kl_cycles", "3", "--label_smoothing", "0.1", "--word_drop", "0.3"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if "kl_raw" in l and "floored_share" in l]
    assert lines, r.stdout
    share = float(lines[-1].split("floored_share:")[1])
    assert 0.0 <= share <= 1.0
    assert "Validation reconstruction loss" in r.stdout
