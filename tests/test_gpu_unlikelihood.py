"""-m gpu: unlikelihood training -- vc_softmax_xent_ul_f32 through the C ABI against the float64 reference (tests/unlikelihood_ref.py),
whole training steps against float64 autograd, the promise that the option at its default launches nothing of it, and what it is
for: after the same steps from the same start the model puts less probability on the words a caption has already said.

Tolerances are those of the smoothed cross-entropy's tests (tests/test_gpu_objective.py): 1e-5 of the tensor maximum for the kernel,
2e-4 relative on losses and 2e-4 of each tensor's maximum on gradients for whole steps.  The candidate counts and everything compared
between two runs of the same kernels are exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import abi, spec, synth
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.trainer import Trainer

from . import unlikelihood_ref as R
from .gpu_util import P, assert_close, dev, host, stream, zeros
from .test_gpu_engine import make_case, small_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("vc_softmax_xent_ul_f32", "vc_ul_stats_f32")
T_, N_ = R.T_CASE, R.N_CASE
ROWS = T_ * N_


# ------------------------------------------------------------------------------------------------ the kernel
def _buffers(buf, ld, off):
    flat = torch.zeros(ROWS * ld + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + ROWS * ld].view(ROWS, ld)
    view.copy_(torch.from_numpy(buf))
    return flat, view


def _call(lib, view, dl, V, ld, den, gscale, eps, alpha, window, write_grad, N=N_, rows=ROWS):
    rl, ru, rm = zeros(ROWS).fill_(-1.0), zeros(ROWS).fill_(-1.0), zeros(ROWS).fill_(-1.0)
    rc = torch.full((ROWS,), -1, dtype=torch.int32, device="cuda")
    lib.vc_softmax_xent_ul_f32(stream(), view.data_ptr(), P(dl), rows, N, V, ld, P(den), gscale, eps, alpha, window, P(rl), P(ru), P(rc), P(rm),
                               write_grad)
    return rl, ru, rc, rm


@pytest.mark.parametrize("eps,alpha", [(0.0, 0.5), (0.1, 2.0)], ids=["eps0-a0.5", "eps0.1-a2"])
@pytest.mark.parametrize("window", [1, 2, 128])
@pytest.mark.parametrize("shape", R.UL_SHAPES, ids=lambda s: "V%d-ld%d-off%d" % s)
def test_kernel_matches_the_reference(lib, shape, window, eps, alpha):
    V, ld, off = shape
    buf, labels = R.ul_case(V, ld, off)
    gscale = 3.0
    c = R.ul_rows(buf[:, :V], labels, eps, alpha, window, gscale)
    assert c["min_om"] >= R.MIN_OM
    flat, view = _buffers(buf, ld, off)
    dl, den = dev(labels.reshape(-1)), zeros(1)
    lib.vc_count_nonzero_i32(stream(), P(dl), ROWS, P(den))
    pad = labels.reshape(-1) == 0
    # forward only: the logits -- padding included -- stay as they are
    rl, ru, rc, rm = _call(lib, view, dl, V, ld, den, gscale, eps, alpha, window, 0)
    np.testing.assert_array_equal(host(view), buf)
    for got, name in ((rl, "row_loss"), (ru, "row_ul"), (rm, "row_mass")):
        print(name, "max err", np.abs(host(got) - c[name]).max(), "of", np.abs(c[name]).max())
        assert_close(host(got), c[name], 1e-5, msg=name)
    np.testing.assert_array_equal(host(rc), c["row_cand"])
    # with the gradient
    rl, ru, rc, rm = _call(lib, view, dl, V, ld, den, gscale, eps, alpha, window, 1)
    got = host(view)
    for g, name in ((rl, "row_loss"), (ru, "row_ul"), (rm, "row_mass")):
        assert_close(host(g), c[name], 1e-5, msg=name + " (with gradient)")
        assert (host(g)[pad] == 0).all(), name
    np.testing.assert_array_equal(host(rc), c["row_cand"])
    print("dlogits max err", np.abs(got[:, :V] - c["dlogits"]).max(), "of", np.abs(c["dlogits"]).max())
    assert_close(got[:, :V], c["dlogits"], 1e-5, msg="dlogits")
    assert (got[:, V:] == 0).all(), "pitch padding must come back exactly 0"
    assert (got[pad] == 0).all(), "PAD rows must come back all-zero"
    assert (host(flat)[:off] == 0).all() and (host(flat)[off + ROWS * ld:] == 0).all()   # nothing outside the rows


@pytest.mark.parametrize("shape", [(203, 204, 0), (203, 205, 0)], ids=["reg", "mem"])
def test_clamped_candidate(lib, shape):
    """row 3 = (t = 1, n = 0) has label V - 1 and the sole candidate word 1; row 4 * 3 = (t = 4, n = 0) has candidates {1, V - 1}: with
    word 1's logit 40 above the rest, 1 - p_1 rounds below the clamp -- -log(1e-5) in row_ul and no gradient term of its own"""
    V, ld, off = shape
    buf, labels = R.ul_case(V, ld, off)
    for r in (3, 12):
        buf[r, 1] = buf[r, :V].max() + np.float32(40)
    eps, alpha, gscale = 0.1, 2.0, 3.0
    c = R.ul_rows(buf[:, :V], labels, eps, alpha, 128, gscale)
    assert c["min_om"] <= R.CLAMP
    other = -np.log1p(-np.exp(np.float64(buf[12, V - 1]) - np.float64(buf[12, 1])))   # 1 - p_{V-1}, p_{V-1} = e^{x - x_1} to 1e-17
    assert c["row_ul"][3] == pytest.approx(-np.log(1e-5), rel=1e-12) and c["row_ul"][12] == pytest.approx(-np.log(1e-5) + other, rel=1e-9)
    flat, view = _buffers(buf, ld, off)
    dl, den = dev(labels.reshape(-1)), zeros(1)
    lib.vc_count_nonzero_i32(stream(), P(dl), ROWS, P(den))
    rl, ru, rc, rm = _call(lib, view, dl, V, ld, den, gscale, eps, alpha, 128, 1)
    got = host(view)
    assert_close(host(ru), c["row_ul"], 1e-5, msg="row_ul")
    assert abs(host(ru)[3] + np.log(1e-5)) <= 1e-5 * -np.log(1e-5)
    assert_close(got[:, :V], c["dlogits"], 1e-5, msg="dlogits")
    # the clamped candidate's own term is absent: its gradient is k (p_1 (1 - alpha R) - eps / V) with R over the OTHER candidates
    k = gscale / float((labels != 0).sum())
    for r in (3, 12):
        p1 = 1.0   # to 1e-17
        Rr = 0.0 if r == 3 else np.exp(np.float64(buf[12, V - 1]) - np.float64(buf[12, 1]))
        assert abs(got[r, 1] - k * (p1 * (1 - alpha * Rr) - eps / V)) <= 1e-5 * np.abs(c["dlogits"]).max()
    np.testing.assert_array_equal(host(rc), c["row_cand"])


@pytest.mark.parametrize("shape", R.UL_SHAPES, ids=lambda s: "V%d-ld%d-off%d" % s)
def test_tiny_alpha_is_the_smoothed_kernel(lib, shape):
    V, ld, off = shape
    buf, labels = R.ul_case(V, ld, off)
    dl, den = dev(labels.reshape(-1)), zeros(1)
    lib.vc_count_nonzero_i32(stream(), P(dl), ROWS, P(den))
    for eps in (0.0, 0.1):
        fa, va = _buffers(buf, ld, off)
        fb, vb = _buffers(buf, ld, off)
        a = zeros(ROWS)
        lib.vc_softmax_xent_smooth_f32(stream(), va.data_ptr(), P(dl), ROWS, V, ld, P(den), 3.0, eps, P(a), 1)
        b = _call(lib, vb, dl, V, ld, den, 3.0, eps, 1e-30, 128, 1)[0]
        assert_close(host(b), host(a), 1e-5, msg="row_loss")
        assert_close(host(vb)[:, :V], host(va)[:, :V], 1e-5, msg="dlogits")
        assert (host(vb)[:, V:] == 0).all()


def test_bad_arguments_are_errors_before_any_launch(lib):
    V, ld = 203, 204
    buf, labels = R.ul_case(V, ld, 0)
    flat, view = _buffers(buf, ld, 0)
    dl, den = dev(labels.reshape(-1)), zeros(1).fill_(1.0)
    ok = dict(eps=0.1, alpha=1.0, window=128, N=N_, rows=ROWS)
    for bad in (dict(window=0), dict(window=129), dict(window=-1), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("inf")),
                dict(alpha=float("nan")), dict(N=4), dict(N=0), dict(eps=1.0), dict(eps=-0.1)):
        kw = dict(ok, **bad)
        with pytest.raises(abi.VaecapError):
            _call(lib, view, dl, V, ld, den, 3.0, kw["eps"], kw["alpha"], kw["window"], 1, N=kw["N"], rows=kw["rows"])
    rl = zeros(ROWS)
    for args in ((None, P(rl), P(rl)), (P(rl), None, P(rl)), (P(rl), P(rl), None)):   # row_ul / row_cand / row_mass
        with pytest.raises(abi.VaecapError):
            lib.vc_softmax_xent_ul_f32(stream(), view.data_ptr(), P(dl), ROWS, N_, V, ld, P(den), 3.0, 0.1, 1.0, 128, P(rl), args[0], args[1], args[2], 1)
    with pytest.raises(abi.VaecapError):   # the smoothed entry's own: the gradient needs den
        lib.vc_softmax_xent_ul_f32(stream(), view.data_ptr(), P(dl), ROWS, N_, V, ld, None, 3.0, 0.1, 1.0, 128, P(rl), P(rl), P(rl), P(rl), 1)
    np.testing.assert_array_equal(host(view), buf)   # nothing ran


# ------------------------------------------------------------------------------------------------ whole steps
PRIORS = {"Normal": dict(prior="Normal"), "GMM": dict(prior="GMM"), "AG_cv": dict(prior="AG", use_c_v=True)}
STEP_OPTIONS = {"ul": dict(unlikelihood=1.0), "ul_ls_fb": dict(unlikelihood=1.0, label_smoothing=0.1, kl_free_bits=0.05)}
# seeds at which the float64 reference keeps every kl[n,l] of all three steps at least 1e-4 away from the floor (found with the
# reference alone; asserted below)
SEEDS = {("Normal", "ul_ls_fb"): 8, ("GMM", "ul_ls_fb"): 8}
V_, B_, TT = 203, 4, 6


@pytest.mark.parametrize("options", list(STEP_OPTIONS), ids=str)
@pytest.mark.parametrize("prior", list(PRIORS), ids=str)
def test_train_steps_match_autograd(lib, prior, options):
    p = small_params(**PRIORS[prior], **STEP_OPTIONS[options])
    P0, batch, noise = make_case(p, V_, B_, TT, seed=SEEDS.get((prior, options), 7))
    hist, Pref = R.reference_steps(p, P0, batch, noise, 3)
    eng = CaptionEngine(p, V_, lib=lib)
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
        assert abs(rec - h["rec"]) <= 2e-4 * abs(h["rec"]), ("rec_loss step %d" % s, rec, h["rec"])
        assert abs(kld - h["kld"]) <= 2e-4 * abs(h["kld"]) + 1e-6, ("kld step %d" % s, kld, h["kld"])
        assert abs(lb - h["lb"]) <= 2e-4 * abs(h["lb"]), ("lower_bound step %d" % s, lb, h["lb"])
        norm = float(eng.ns[0].item())
        assert abs(norm - h["norm"]) <= 3e-4 * h["norm"], ("global norm step %d" % s, norm, h["norm"])
        assert h["norm"] > p.lstm_clip_by_norm, "clip not active in this case"
        o = eng.objective_stats()
        for key in ("ul", "ul_candidates", "repeat_mass"):
            assert abs(o[key] - h[key]) <= 2e-4 * abs(h[key]), (key, s, o[key], h[key])
        assert ("kl_raw" in o) == (p.kl_free_bits > 0)
    Pg = eng.state_dict()
    for name, ref in Pref.items():
        upd = np.abs(ref - P0[name]).max()
        err = np.abs(Pg[name] - ref).max()
        assert err <= 2e-3 * upd + 1e-7, "param %s after 3 steps: err %.3e, update size %.3e" % (name, err, upd)


def test_validation_forward_keeps_the_plain_loss(lib):
    rec = []
    for alpha in (0.0, 1.0):
        p = small_params(prior="Normal", unlikelihood=alpha)
        P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
        eng = CaptionEngine(p, V_, lib=lib)
        eng.load_params(P0)
        eng.set_batch(batch, noise)
        eng.forward(train=False)
        rec.append(eng.losses()[1])
    assert rec[0] == rec[1]


class _NoNewEntries(object):
    """the loaded library, except that resolving an entry of this feature is an error (the guard of tests/test_gpu_objective.py)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in NEW_ENTRIES:
            raise AssertionError("%s resolved with --unlikelihood at its default" % name)
        return getattr(self._lib, name)


def test_defaults_launch_none_of_the_new_entries(lib):
    guard = _NoNewEntries(lib)
    for kw in PRIORS.values():
        p = small_params(**kw)
        P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
        eng = CaptionEngine(p, V_, lib=guard)
        eng.load_params(P0)
        for _ in range(2):
            eng.set_batch(batch, noise)
            eng.forward(); eng.backward(); eng.pack_tail(); eng.apply_gradients()
        assert all(np.isfinite(eng.losses())) and eng.objective_stats() is None
        assert not any(k in eng.buf for k in ("row_ul", "row_cand", "row_mass"))
    # ... and the guard is not vacuous: with the option on, the same step goes through the new entry
    p = small_params(prior="Normal", unlikelihood=1.0)
    P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
    eng = CaptionEngine(p, V_, lib=guard)
    eng.load_params(P0)
    eng.set_batch(batch, noise)
    with pytest.raises(AssertionError, match="vc_softmax_xent_ul_f32"):
        eng.forward()


def test_captured_step_equals_eager(lib):
    p = small_params(prior="Normal", unlikelihood=1.0, ul_window=3, label_smoothing=0.1)
    rng = np.random.default_rng(31)
    P0 = spec.init_caption_params(p, V_, seed=4)
    batches = [synth.make_batch(rng, B_, p.num_captions, TT, V_, variable_len=True, feature_size=p.cnn_feature_size) for _ in range(3)]
    res = []
    for graph in (False, True):
        tr = Trainer(p, V_, lib=lib, seed=9)
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
            o = tr.objective_stats()
            losses.append(tr.losses() + (o["ul"], o["ul_candidates"], o["repeat_mass"]))
        res.append((losses, tr.state_dict()))
    assert res[0][0] == res[1][0]
    assert all(l[4] > 0 and l[5] > 0 and 0 < l[6] < 1 for l in res[0][0])
    for k in res[0][1]:
        np.testing.assert_array_equal(res[0][1][k], res[1][1][k], err_msg=k)


def test_forced_single_rank_collectives(lib):
    p = small_params(prior="Normal", unlikelihood=1.0)
    P0, batch, noise = make_case(p, V_, B_, TT, seed=9)
    res = []
    for force in (False, True):
        tr = Trainer(p, V_, lib=lib, force_collectives=force)
        tr.load_state_dict(P0)
        for _ in range(2):
            tr.set_batch(batch, noise)
            tr.train_step()
        o = tr.objective_stats()
        res.append(tr.losses() + (o["ul"], o["ul_candidates"], o["repeat_mass"]))
        if tr.comm is not None:
            tr.comm.destroy()
    for a, b in zip(res[0], res[1]):
        assert abs(a - b) <= 2e-4 * abs(a), (res[0], res[1])


def test_one_step_with_scheduled_sampling(lib):
    """the second pass trains against the unchanged labels: the candidates are the labels' alone"""
    p = small_params(prior="Normal", unlikelihood=1.0, sched_sampling=0.5, sched_schedule="constant")
    P0 = spec.init_caption_params(p, V_, seed=4)
    batch = synth.make_batch(np.random.default_rng(5), B_, p.num_captions, TT, V_, variable_len=True, feature_size=p.cnn_feature_size)
    tr = Trainer(p, V_, lib=lib, seed=9)
    tr.load_state_dict(P0)
    tr.set_batch(batch)
    tr.train_step()
    o, s = tr.objective_stats(), tr.sched_stats()
    assert all(np.isfinite(tr.losses())) and all(np.isfinite(v) for v in o.values())
    assert s["replaced"] > 0
    sets = R.candidate_sets(batch["cap_enc"].T, V_, 128)
    ref = sum(len(c) for c in sets) / float((batch["cap_enc"] != 0).sum())
    assert o["ul_candidates"] == pytest.approx(ref, rel=1e-6)


# ------------------------------------------------------------------------------------------------ behaviour
def _device_repeat_mass(lib, eng, window=128):
    """forward-only call of the new entry on the logits of a forward(train=False) pass: the logits stay as they are"""
    N, T, V = eng.N, eng.T, eng.V
    R_ = T * N
    eng.forward(train=False)
    ld = (V + 3) // 4 * 4
    rl, ru, rm, st = zeros(R_), zeros(R_), zeros(R_), zeros(3)
    rc = torch.zeros(R_, dtype=torch.int32, device="cuda")
    labels = eng.buf["cap_enc_t"]
    lib.vc_softmax_xent_ul_f32(stream(), P(eng.buf["logits"]), P(labels), R_, N, V, ld, None, 1.0, 0.0, 1.0, window, P(rl), P(ru), P(rc), P(rm), 0)
    lib.vc_ul_stats_f32(stream(), R_, V, P(labels), P(ru), P(rc), P(rm), P(st))
    return float(host(st)[2])


def test_training_with_the_term_lowers_the_repeat_mass(lib):
    """Same start, same batch, 60 eager steps with alpha = 1 and with alpha = 0; then the probability on already-said words of each
    trained model, measured the same way for both: a forward pass (train=False) and a forward-only call of the new entry.  The seed was
    chosen with the float64 reference alone (tests/test_unlikelihood_host.py: its two values differ by more than 10 %).
    Reference: 0.0608503 (alpha = 1) against 0.0688512 (alpha = 0).  Device values: DESIGN.md "Unlikelihood training"."""
    b = R.BEHAVIOUR
    mass = {}
    for alpha in (1.0, 0.0):
        p = small_params(prior=b["prior"], unlikelihood=alpha)
        P0, batch, noise = make_case(p, b["V"], b["B"], b["T"], seed=b["seed"])
        eng = CaptionEngine(p, b["V"], lib=lib)
        eng.load_params(P0)
        for _ in range(b["steps"]):
            eng.set_batch(batch, noise)
            eng.forward(); eng.backward(); eng.pack_tail(); eng.apply_gradients()
        if alpha > 0:
            last = eng.objective_stats()["repeat_mass"]   # (of the last step's forward: one update behind the measurement below)
        eng.set_batch(batch, noise)
        mass[alpha] = _device_repeat_mass(lib, eng)
    print("device repeat_mass after %d steps: alpha=1 %.6g (last training forward %.6g), alpha=0 %.6g" % (b["steps"], mass[1.0], last, mass[0.0]))
    assert mass[1.0] < mass[0.0], mass


# ------------------------------------------------------------------------------------------------ CLI
def test_main_cli_prints_the_new_line(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "120", "--bs", "2", "--embed_dim", "32", "--enc_hid", "32",
           "--dec_hid", "32", "--latent", "8", "--gen_z_samples", "3", "--gpu", "0", "--checkpoint", "ultest", "--ckpt_format", "npz",
           "--max_steps", "3", "--epochs", "1", "--unlikelihood", "1", "--ul_window", "4"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("Unlikelihood: ul:") and "candidates:" in l and "repeat_mass:" in l]
    assert lines, r.stdout
    mass = float(lines[-1].split("repeat_mass:")[1])
    assert 0.0 < mass < 1.0
