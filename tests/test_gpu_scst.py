"""-m gpu: self-critical training (DESIGN.md "Self-critical training").

1. vc_softmax_xent_policy_f32 against the float64 reference (tests/scst_ref.py) at every dispatch edge, 1e-5 of each tensor's maximum
   (the smoothed kernel's tolerance, tests/test_gpu_objective.py); 2. against vc_softmax_xent_f32 where the two coincide;
3. whole policy steps of CaptionEngine against float64 autograd with the tolerances of test_train_steps_with_options_match_autograd,
   the encoder's parameters and optimiser slots bit-identical; 4. the policy forward reproduces the log-probabilities the sampler
   recorded (the z and the row order are carried over); 5. CiderReward against the float64 CIDEr-D; 6. it learns; 7. with the flags
   off nothing resolves the new entry; 8. the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import scst, spec, synth
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.generate import CaptionGenerator
from vae_captioning_amd.trainer import Trainer
from vae_captioning_amd.utils.parameters import Parameters

from . import scst_ref as R
from .gpu_util import P, assert_close, dev, host, stream, zeros
from .test_gpu_engine import make_case, small_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOS, EOS = synth.BOS, synth.EOS
NEW_ENTRIES = ("vc_softmax_xent_policy_f32",)
SUMS = dict(rtol=1e-4, atol=1e-6)   # tests/test_gpu_score.py: log-likelihood sums of the decoders against the same model
IDS = lambda s: "V%d-ld%d-off%d-T%d-N%d" % s


# ------------------------------------------------------------------------------------------------ 1, 2: the kernel
def _buffers(V, ld, off, T, N):
    buf, labels, adv, plants = R.policy_case(V, ld, off, T, N)
    rows = T * N
    flat = torch.zeros(rows * ld + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + rows * ld].view(rows, ld)
    view.copy_(torch.from_numpy(buf))
    return buf, labels, adv, plants, flat, view


@pytest.mark.parametrize("beta", [0.0, 0.25])
@pytest.mark.parametrize("shape", R.POLICY_SHAPES, ids=IDS)
def test_policy_xent_matches_the_reference(lib, shape, beta):
    V, ld, off, T, N = shape
    buf, labels, adv, plants, flat, view = _buffers(*shape)
    rows, scale = T * N, 1.0 / N
    lp_ref, ent_ref, g_ref = R.policy_xent(buf[:, :V], labels, adv, N, scale, beta)
    dl, da = dev(labels), dev(adv)
    lp, ent = torch.full((rows,), -7.0, device="cuda"), (torch.full((rows,), -7.0, device="cuda") if beta > 0 else None)
    # forward only: the logits -- padding included -- stay as they are
    lib.vc_softmax_xent_policy_f32(stream(), view.data_ptr(), P(dl), rows, V, ld, P(da), N, scale, beta, P(lp), P(ent), 0)
    np.testing.assert_array_equal(host(view), buf)
    lp0 = host(lp).copy()
    print("row_lp max err %.3e (max %.3e)" % (np.abs(lp0 - lp_ref).max(), np.abs(lp_ref).max()))
    assert_close(lp0, lp_ref, 1e-5, msg="row_lp")
    assert (lp0 <= 0).all()
    if beta > 0:
        print("row_ent max err %.3e (max %.3e)" % (np.abs(host(ent) - ent_ref).max(), np.abs(ent_ref).max()))
        assert_close(host(ent), ent_ref, 1e-5, msg="row_ent")
    lp.fill_(-7.0)
    if ent is not None:
        ent.fill_(-7.0)
    lib.vc_softmax_xent_policy_f32(stream(), view.data_ptr(), P(dl), rows, V, ld, P(da), N, scale, beta, P(lp), P(ent), 1)
    got = host(view)
    np.testing.assert_array_equal(host(lp), lp0, err_msg="row_lp with and without the gradient")
    print("dlogits max err %.3e (max %.3e)" % (np.abs(got[:, :V] - g_ref).max(), np.abs(g_ref).max()))
    assert_close(got[:, :V], g_ref, 1e-5, msg="dlogits")
    assert (got[:, V:] == 0).all(), "pitch padding must come back exactly 0"
    assert (host(flat)[:off] == 0).all() and (host(flat)[off + rows * ld:] == 0).all()   # nothing outside the rows
    if beta > 0:
        assert_close(host(ent), ent_ref, 1e-5, msg="row_ent (with gradient)")
    if plants:
        assert lp0[plants["pad"]] == 0.0 and (got[plants["pad"]] == 0).all()
        if beta > 0:
            e = host(ent)
            assert e[plants["pad"]] == 0.0 and 0.0 <= e[plants["spike"]] < 1e-6
            assert e[plants["equal"]] == pytest.approx(np.log(V), rel=1e-5)


def test_policy_xent_argument_checks(lib):
    x, lab, adv, lp = zeros(6, 8), dev(np.ones(6, np.int32)), zeros(3), zeros(6)
    from vae_captioning_amd.abi import VaecapError
    call = lambda rows, N, beta, ent: lib.vc_softmax_xent_policy_f32(stream(), P(x), P(lab), rows, 8, 8, P(adv), N, 1.0, beta, P(lp), ent, 1)
    for bad in ((6, 4, 0.0, None), (6, 0, 0.0, None), (6, 3, 0.1, None), (6, 3, -1.0, P(lp)), (6, 3, float("inf"), P(lp))):
        with pytest.raises(VaecapError):
            call(*bad)
    call(6, 3, 0.0, None)
    call(0, 3, 0.0, None)


@pytest.mark.parametrize("shape", R.POLICY_SHAPES, ids=IDS)
def test_policy_xent_with_unit_advantages_is_the_plain_kernel(lib, shape):
    """adv = 1, beta = 0, scale = gscale / den: the gradient of vc_softmax_xent_f32, and row_lp = -row_loss"""
    V, ld, off, T, N = shape
    rows, gscale = T * N, 3.0
    outs = []
    for policy in (False, True):
        buf, labels, adv, plants, flat, view = _buffers(*shape)
        dl, den, rl = dev(labels), zeros(1), zeros(rows)
        lib.vc_count_nonzero_i32(stream(), P(dl), rows, P(den))
        if policy:
            lib.vc_softmax_xent_policy_f32(stream(), view.data_ptr(), P(dl), rows, V, ld, P(dev(np.ones(N, np.float32))), N,
                                           gscale / float((labels != 0).sum()), 0.0, P(rl), None, 1)
        else:
            lib.vc_softmax_xent_f32(stream(), view.data_ptr(), P(dl), rows, V, ld, P(den), gscale, P(rl), 1)
        outs.append((host(view)[:, :V].copy(), host(rl).copy()))
    assert_close(outs[1][0], outs[0][0], 1e-5, msg="dlogits")
    assert_close(outs[1][1], -outs[0][1], 1e-5, msg="row_lp vs -row_loss")


# ------------------------------------------------------------------------------------------------ 3: policy steps vs autograd
PRIORS = {"Normal": dict(prior="Normal"), "GMM": dict(prior="GMM"), "AG_cv": dict(prior="AG", use_c_v=True),
          "no_encoder": dict(prior="Normal", no_encoder=True)}
STEP_V, STEP_B, STEP_T = 203, 4, 6


def _step_case(p, seed=7):
    P0, batch, _ = make_case(p, STEP_V, STEP_B, STEP_T, seed=seed)
    rng = np.random.default_rng(seed + 100)
    N = STEP_B * p.num_captions
    _, dec, enc, lens = R.sample_case(rng, N, STEP_T, STEP_V, BOS, EOS)
    pb = dict(features=batch["features"], cap_dec=dec, cap_enc=enc, lengths=lens)
    if "c_v" in batch:
        pb["c_v"] = batch["c_v"]
    z = None if p.no_encoder else (rng.standard_normal((N, p.gen_z_samples * p.latent_size)) * 0.3).astype(np.float32)
    advs = [rng.standard_normal(N).astype(np.float32) for _ in range(3)]
    for a in advs:
        a[2] = 0.0   # a caption the batch mean baseline leaves without a gradient
    return P0, pb, z, advs


def _encoder_state(eng):
    """every encoder/* range of the parameters and of each optimiser slot, as host copies"""
    S = eng.store
    torch.cuda.synchronize()
    return {(buf, n): S._view(t, n).detach().cpu().numpy().copy() for n in S.names() if n.startswith("encoder/")
            for buf, t in [("p", S.p)] + sorted(S.slots.items())}


def _plant_encoder_slots(eng, slots):
    """optimiser slots of encoder/* as an earlier XE run would have left them: non-zero, so that "untouched" means something"""
    g = torch.Generator(device="cuda").manual_seed(5)
    for s in slots:
        t = eng.store.slot(s)
        for n in eng.store.names():
            if n.startswith("encoder/"):
                v = eng.store._view(t, n)
                v.copy_(torch.rand(v.shape, device="cuda", generator=g) * 1e-3)


def _run_policy_steps(lib, p, beta, optimizer="Adam", precision="f32", steps=3, grad_tol=2e-4, check_params=True):
    P0, pb, z, advs = _step_case(p)
    hist, Pref = R.reference_policy_steps(p, P0, pb, z, advs, beta, steps, optimizer=optimizer)
    eng = CaptionEngine(p, STEP_V, lib=lib)
    eng.set_precision(precision)
    eng.load_params(P0)
    _plant_encoder_slots(eng, ("m", "v") if optimizer == "Adam" else ("a",))
    before = _encoder_state(eng)
    assert p.no_encoder or len(before) >= 3 * (2 if optimizer == "Adam" else 1)
    for s, h in enumerate(hist):
        eng.set_batch(pb)
        eng.policy_forward(advs[s], z, beta)
        eng.backward(policy=True)
        eng.pack_tail()
        G = eng.grads_dict()
        assert set(h["grads"]) == {n for n in P0 if R.trained(n, p)}
        for name, ref in h["grads"].items():
            tol = grad_tol * (np.abs(ref).max() + 1e-12)
            err = np.abs(G[name] - ref).max()
            assert err <= tol, "step %d grad %s: err %.3e tol %.3e (max %.3e)" % (s, name, err, tol, np.abs(ref).max())
        np.testing.assert_allclose(host(eng.buf["cap_lp"]), h["cap_lp"], rtol=2e-4 if precision == "f32" else 1e-3, atol=1e-5)
        eng.policy_apply_gradients()
        kld, rec, lb, ann = eng.losses()
        assert kld == 0.0 and rec == lb and np.isfinite(rec)
        if check_params:
            norm = float(eng.ns[0].item())
            assert abs(norm - h["norm"]) <= 3e-4 * h["norm"], ("global norm step %d" % s, norm, h["norm"])
            assert h["norm"] > p.lstm_clip_by_norm, "clip not active in this case"
        st = eng.policy_stats()
        assert st["tokens"] == int((pb["cap_enc"] != 0).sum()) and (st["entropy"] is None) == (beta == 0)
        if beta > 0:
            assert 0.0 < st["entropy"] <= np.log(STEP_V) + 1e-4
    assert int(eng.step.item()) == steps   # the global step advanced like in any training step
    after = _encoder_state(eng)
    for k, v in before.items():
        np.testing.assert_array_equal(after[k], v, err_msg="%s of %s changed in a policy step" % k)
    if check_params:
        Pg = eng.state_dict()
        moved = 0
        for name, ref in Pref.items():
            upd = np.abs(ref - P0[name]).max()
            err = np.abs(Pg[name] - ref).max()
            assert err <= 2e-3 * upd + 1e-7, "param %s after %d steps: err %.3e, update size %.3e" % (name, steps, err, upd)
            assert (upd > 0) == R.trained(name, p), name
            moved += upd > 0
        assert moved >= 6


@pytest.mark.parametrize("beta", [0.0, 0.1])
@pytest.mark.parametrize("prior", list(PRIORS), ids=str)
def test_policy_steps_match_autograd(lib, prior, beta):
    _run_policy_steps(lib, small_params(**PRIORS[prior]), beta)


def test_policy_steps_with_momentum_leave_the_encoder_alone(lib):
    _run_policy_steps(lib, small_params(prior="Normal", optimizer="Momentum"), 0.1, optimizer="Momentum")


def test_policy_step_in_bf16x3(lib):
    """the trainer's precision flows through engine.gemm / lstm_flags: one step, gradients within 1e-3 of each tensor's maximum
    (what tests/test_gpu_bf16x3.py holds a whole training step's gradients to)"""
    _run_policy_steps(lib, small_params(prior="Normal"), 0.1, precision="bf16x3", steps=1, grad_tol=1e-3, check_params=False)


def test_policy_step_errors(lib):
    p = small_params(prior="Normal")
    with pytest.raises(RuntimeError, match="data-parallel"):
        e = CaptionEngine(p, STEP_V, lib=lib, force_collectives=True)
        e.reduce_fn = lambda t: None
        e.policy_forward(np.zeros(12, np.float32), None)
    with pytest.raises(RuntimeError, match="fine_tune"):
        CaptionEngine(small_params(prior="Normal", fine_tune=True), STEP_V, lib=lib).policy_forward(np.zeros(12, np.float32), None)
    P0, pb, z, advs = _step_case(p)
    eng = CaptionEngine(p, STEP_V, lib=lib)
    eng.load_params(P0)
    eng.set_batch(pb)
    with pytest.raises(ValueError, match="needs the z"):
        eng.policy_forward(advs[0], None)
    eng.set_batch(pb)
    with pytest.raises(ValueError, match="advantages"):
        eng.policy_forward(advs[0][:5], z)


# ------------------------------------------------------------------------------------------------ 4: sampler and step agree
def _corpus(rng, n, V, per=3):
    return [[[BOS] + rng.integers(3, V, size=rng.integers(4, 9)).tolist() + [EOS] for _ in range(per)] for _ in range(n)]


def _scst_trainer(lib, p, V, baseline="average", beta=0.0, max_len=8, seed=3, P0=None, corpus=None):
    tr = Trainer(p, V, lib=lib, seed=seed)
    tr.load_state_dict(P0 if P0 is not None else spec.init_caption_params(p, V, seed=8))
    corpus = corpus if corpus is not None else _corpus(np.random.default_rng(1), 20, V)
    tr.enable_scst(scst.CiderReward(tr.cap, corpus, BOS, EOS, V), BOS, EOS, baseline=baseline, beta=beta, max_len=max_len)
    return tr


@pytest.mark.parametrize("inject", [True, False], ids=["injected-eps", "philox-eps"])
@pytest.mark.parametrize("prior", list(PRIORS), ids=str)
def test_policy_forward_reproduces_the_samplers_logprobs(lib, prior, inject):
    p = small_params(**PRIORS[prior])
    V, B, T, K = 203, 4, 6, p.num_captions
    rng = np.random.default_rng(11)
    batch = synth.make_batch(rng, B, K, T, V, use_ci=spec.uses_ci(p), variable_len=True, feature_size=p.cnn_feature_size)
    tr = _scst_trainer(lib, p, V)
    # (the logits layer's bias favours <EOS> a little, so that some samples end inside max_len and some do not)
    # ... and id 0 is out of reach, as in a trained model (PAD is never a target): a sampled 0 would be a masked label of the step
    tr.cap.store.param("decoder/rnn_logits/bias")[EOS] += 3.0
    tr.cap.store.param("decoder/rnn_logits/bias")[0] -= 30.0
    eps = rng.standard_normal((K, p.gen_z_samples, B, p.latent_size)).astype(np.float32) if inject and not p.no_encoder else None
    cands, z = tr.scst_sample(batch, "sample", eps)
    assert (z is None) == bool(p.no_encoder)
    zc = z.clone() if z is not None else None
    ended = [c[2] for cs in cands for c in cs]
    assert any(ended) and not all(ended)
    pb = scst.policy_batch([list(c[0]) for cs in cands for c in cs], BOS, EOS)
    pb["features"] = batch["features"]
    if "c_v" in batch:
        pb["c_v"] = batch["c_v"]
    tr.set_batch(pb)
    tr.cap.policy_forward(np.zeros(B * K, np.float32), zc, 0.0)
    np.testing.assert_allclose(host(tr.cap.buf["cap_lp"]), [c[1] for cs in cands for c in cs], **SUMS)
    if z is not None and eps is not None:   # the greedy baseline decodes under the same z (the step counter has moved: injected eps only)
        _, z2 = tr.scst_sample(batch, "greedy", eps)
        assert torch.equal(z2, zc)


def test_greedy_pass_of_the_same_step_sees_the_samplers_z(lib):
    """device Philox eps: a greedy pass that follows the sample pass before the step counter moves decodes under the same z"""
    p = small_params(prior="AG", use_c_v=True)
    V, B, K = 203, 4, p.num_captions
    batch = synth.make_batch(np.random.default_rng(12), B, K, 6, V, use_ci=True, variable_len=True, feature_size=p.cnn_feature_size)
    tr = _scst_trainer(lib, p, V)
    _, z = tr.scst_sample(batch, "sample")
    zc = z.clone()
    _, z2 = tr.scst_sample(batch, "greedy")
    assert torch.equal(z2, zc) and float(zc.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5: the reward
def test_cider_reward_matches_the_float64_reference(lib):
    rng = np.random.default_rng(21)
    V = 30
    corpus = _corpus(rng, 40, V)
    refs = [list(c) for c in corpus[:7]]
    cands = [[[BOS] + rng.permutation(r[0][1:-1]).tolist()[:rng.integers(2, 9)] + [EOS] for _ in range(4)] + [list(r[1])] for r in refs]
    cands[0][0] = [EOS]                                  # an empty sample
    cands[2][1] = [BOS, EOS]
    same = [3, 4, 5, 6, 7, 8, EOS]
    refs[3] = [list(same)] * 3                           # an image whose references all equal the candidate
    cands[3][2] = list(same)
    rw = scst.CiderReward(lib, corpus, BOS, EOS, V)
    got = rw.rewards(cands, refs)
    want = np.concatenate(R.cider_rewards(cands, refs, corpus, BOS, EOS))
    assert got.dtype == np.float64 and got.shape == want.shape == (35,)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    assert got[0] == 0.0 and got[11] == 0.0 and got[17] == pytest.approx(10.0, rel=1e-5) and want.max() > 1.0
    assert rw.rewards([[] for _ in refs], refs).shape == (0,)
    with pytest.raises(ValueError):
        rw.rewards(cands, refs[:3])


# ------------------------------------------------------------------------------------------------ 6: it learns
LEARN = dict(V=200, B=16, K=4, T=9, xe_steps=20, scst_steps=150, lr=2e-3, scst_lr=1e-3)


def learn(lib, baseline, xe_steps=LEARN["xe_steps"], scst_steps=LEARN["scst_steps"], lr=LEARN["lr"], scst_lr=LEARN["scst_lr"], beta=0.0, seed=5,
          log=None):
    """Sixteen images, each with one fixed caption (its K batch rows are that caption, so a perfect caption scores 10): a few XE steps,
    then self-critical steps on the same batch.  -> dict(before, after: mean CIDEr-D of the greedy captions; rewards: the mean sampled
    reward of every step)"""
    V, B, K, T = LEARN["V"], LEARN["B"], LEARN["K"], LEARN["T"]
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden = 64, 128, 128
    p.latent_size, p.gen_z_samples, p.cnn_feature_size = 20, 6, 96       # dims of tests/test_gpu_learning.py
    p.num_captions, p.batch_size, p.learning_rate, p.prior = K, B, lr, "Normal"
    rng = np.random.default_rng(42)
    one = synth.make_batch(rng, B, 1, T, V, variable_len=True, feature_size=p.cnn_feature_size)
    assert one["lengths"].min() >= 6
    batch = dict(features=one["features"], cap_dec=np.repeat(one["cap_dec"], K, axis=0), cap_enc=np.repeat(one["cap_enc"], K, axis=0),
                 lengths=np.repeat(one["lengths"], K))
    refs = scst.batch_references(batch["cap_enc"], batch["lengths"], K)
    tr = _scst_trainer(lib, p, V, baseline=baseline, beta=beta, max_len=T + 3, seed=seed, P0=spec.init_caption_params(p, V, seed=3), corpus=refs)
    eps = rng.standard_normal((p.gen_z_samples, B, p.latent_size)).astype(np.float32)
    gen = CaptionGenerator(tr.cap)
    reward = tr.scst["reward"]
    greedy = lambda: float(reward.rewards([[g] for g in gen.greedy(batch["features"], None, eps, BOS, EOS, max_len=T + 3)], refs).mean())
    for _ in range(xe_steps):
        tr.set_batch(batch)
        tr.train_step()
    out = dict(before=greedy(), rewards=[])
    p.learning_rate = scst_lr   # (read by every step: what a --restore run with its own --lr does)
    for s in range(scst_steps):
        out["rewards"].append(tr.scst_step(batch)["reward"])
        if log is not None and s % 25 == 24:
            log("  %s step %3d: sampled reward (last 10) %.4f, greedy %.4f, stats %r" % (baseline, s, np.mean(out["rewards"][-10:]), greedy(), tr.scst_stats))
    out["after"] = greedy()
    return out


@pytest.mark.parametrize("baseline", ["average", "greedy"])
def test_self_critical_steps_raise_the_reward(lib, baseline):
    """Twenty XE steps at lr 2e-3 leave the greedy captions at a mean CIDEr-D of 0.23 of 10; 150 self-critical steps at lr 1e-3 follow.
    Observed on an MI355X (seeds fixed; a second trainer seed gave the same picture):
      average: greedy CIDEr-D 0.2323 -> 0.7225, mean sampled reward of the first 10 steps 0.3355, of the last 10 steps 1.0351
      greedy:  greedy CIDEr-D 0.2323 -> 0.5698, mean sampled reward of the first 10 steps 0.3290, of the last 10 steps 0.8042
    (At lr 2e-3 the sampled reward rises as steadily but the greedy captions of sixteen images jump from step to step; with more XE
    steps the model has memorised its captions and there is little left for sampling to find.)"""
    r = learn(lib, baseline)
    print("%s: greedy CIDEr-D %.4f -> %.4f, sampled reward first 10 %.4f, last 10 %.4f" % (
        baseline, r["before"], r["after"], np.mean(r["rewards"][:10]), np.mean(r["rewards"][-10:])))
    assert 0.0 < r["before"] < 10.0, r["before"]        # the XE steps left something to learn and something to start from
    assert len(r["rewards"]) <= 200
    assert r["after"] > r["before"], (r["before"], r["after"])
    assert np.mean(r["rewards"][-10:]) > np.mean(r["rewards"][:10])


# ------------------------------------------------------------------------------------------------ 7: off means off
class _NoNewEntries(object):
    """the loaded library, except that resolving the entry of this feature is an error"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in NEW_ENTRIES:
            raise AssertionError("%s resolved" % name)
        return getattr(self._lib, name)


def test_defaults_never_resolve_the_policy_entry(lib):
    guard = _NoNewEntries(lib)
    with pytest.raises(AssertionError):
        guard.vc_softmax_xent_policy_f32
    V, B, T = 203, 4, 6
    for kw in PRIORS.values():
        p = small_params(**kw)
        P0, batch, noise = make_case(p, V, B, T, seed=7)
        eng = CaptionEngine(p, V, lib=guard)
        eng.load_params(P0)
        for _ in range(2):
            eng.set_batch(batch, noise)
            eng.forward(); eng.backward(); eng.pack_tail(); eng.apply_gradients()
        assert all(np.isfinite(eng.losses()))
    p = small_params(prior="Normal")
    batch = synth.make_batch(np.random.default_rng(2), B, p.num_captions, T, V, variable_len=True, feature_size=p.cnn_feature_size)
    for captured in (False, True):
        tr = Trainer(p, V, lib=guard, seed=3)
        tr.load_state_dict(spec.init_caption_params(p, V, seed=8))
        tr.set_batch(batch)
        if captured:
            tr.capture(warmup=1)
        tr.train_step()
        assert all(np.isfinite(tr.losses())) and tr.eval_rec_loss() > 0
    with pytest.raises(RuntimeError, match="hipGraph"):      # (the captured trainer: its graph bakes the XE step)
        tr.policy_step(np.zeros(B * p.num_captions, np.float32), None)


def test_scst_resolves_the_policy_entry(lib):
    """... and the guard is not vacuous: a self-critical step of the same trainer goes through it"""
    p = small_params(prior="Normal")
    V, B, T = 203, 4, 6
    batch = synth.make_batch(np.random.default_rng(2), B, p.num_captions, T, V, variable_len=True, feature_size=p.cnn_feature_size)
    tr = _scst_trainer(_NoNewEntries(lib), p, V)
    with pytest.raises(AssertionError, match="vc_softmax_xent_policy_f32"):
        tr.scst_step(batch)
    tr = _scst_trainer(lib, p, V, baseline="greedy", beta=0.01)
    st = tr.scst_step(batch)
    assert set(st) == {"reward", "baseline", "sample_len", "ended_share", "entropy", "logprob"}
    assert st["entropy"] > 0 and st["logprob"] < 0 and 1 <= st["sample_len"] <= 8 and 0 <= st["ended_share"] <= 1 and st is tr.scst_stats


# ------------------------------------------------------------------------------------------------ 8: the command line
def test_main_cli_scst_after_an_xe_run(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "120", "--bs", "2", "--embed_dim", "32", "--enc_hid", "32",
            "--dec_hid", "32", "--latent", "8", "--gen_z_samples", "3", "--gpu", "0", "--checkpoint", "scsttest", "--ckpt_format", "npz",
            "--epochs", "1", "--max_steps", "2"]
    r = subprocess.run(base, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ckpt = tmp_path / "checkpoints" / "scsttest.ckpt.npz"
    with np.load(ckpt) as z:
        xe = {k: z[k] for k in z.files}
    r = subprocess.run(base + ["--scst", "--restore", "--scst_baseline", "greedy", "--scst_entropy", "0.01"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if "SCST: reward:" in l]
    assert lines and all(k in lines[-1] for k in ("baseline:", "sample_len:", "entropy:")), r.stdout
    assert "Warning" not in r.stdout and "Validation reconstruction loss" in r.stdout and "Model saved" in r.stdout
    with np.load(ckpt) as z:
        new = {k: z[k] for k in z.files}
    assert set(new) == set(xe)
    enc = [k for k in xe if k.startswith("encoder/")]
    assert len(enc) >= 7
    for k in enc:
        np.testing.assert_array_equal(new[k], xe[k], err_msg=k)
    assert any(not np.array_equal(new[k], xe[k]) for k in xe if k.startswith("decoder/"))
    # without --restore the run warns
    r = subprocess.run(base + ["--scst", "--max_steps", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Warning: --scst without --restore" in r.stdout, r.stdout + r.stderr
