"""-m gpu: weight averaging -- the fused Adam + average entries, the stand-alone average and the in-place swap through the C ABI against
their unfused partners (bit for bit) and the float64 recurrence of tests/ema_ref.py (a derived rounding bound); the engines with the flag
on against the same run with it off; the promise that the flag at its default resolves nothing of it; capture, collectives, fine-tuning,
Trainer.ema_weights(), checkpoints of both formats and the command line.

Everything compared between two runs of the same kernels is exact.  The averages are compared with the float64 recurrence over the
float32 parameter history read back from the device, within ema_ref.bound: 3 * steps * 2^-24 * max(|p|, |e|) per element."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import spec, synth
from vae_captioning_amd.engine import EMA_SUFFIX, CaptionEngine
from vae_captioning_amd.generate import CaptionGenerator
from vae_captioning_amd.trainer import Trainer
from vae_captioning_amd.utils.parameters import Parameters

from . import ema_ref as R
from .gpu_util import P, assert_close, dev, host, stream, zeros
from .test_gpu_engine import make_case, small_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("vc_adam_ema_f32", "vc_adam_sumsq_ema_f32", "vc_ema_update_f32", "vc_swap_f32")
GUARD = 64
NAN_BITS = 0x7FC0BEEF   # a quiet NaN with a payload: a guard band nobody may write


# ------------------------------------------------------------------------------------------------ the kernels
def banded(values, off=0):
    """-> (the whole allocation as int32, the float32 view of `values` in it): `off` floats, a guard band, the values, a guard band"""
    n = len(values)
    flat = torch.full((off + GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    view = flat[off + GUARD:off + GUARD + n].view(torch.float32)
    assert view.data_ptr() % 16 == 0
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)))
    return flat, view


def bands_intact(flat, n, off=0):
    return bool((host(flat[:off + GUARD]) == NAN_BITS).all() and (host(flat[off + GUARD + n:]) == NAN_BITS).all())


# n: 3 = the scalar tail alone; 4 = one group; 1027 = the single-group path + a tail of 3; the last = past the grid cap of 2048 x 256
# threads (2 097 152 floats): the first 300 threads take one paired iteration, the others the single-group path, 3 floats the tail
SIZES = [3, 4, 1027, 2_097_152 + 1203]
# name -> (scale, l2, sumsq, offset in floats of the base pointers into their allocations)
VARIANTS = {"plain": (False, 0.0, False, 0), "scale": (True, 0.0, False, 0), "l2": (False, 0.01, False, 0), "sumsq": (False, 0.01, True, 0),
            "offset": (True, 0.01, False, 64)}
# decay 0.5: 9 / (10 + t) crosses 1 - decay at t = 8, so both sides of the max run in 12 steps; 0.999: the warm-up wins throughout
MODES = {"d0.5": (0.5, True), "d0.999": (0.999, True), "nostep": (0.5, False)}
STEPS = 12


@pytest.mark.parametrize("mode", list(MODES), ids=str)
@pytest.mark.parametrize("variant", list(VARIANTS), ids=str)
@pytest.mark.parametrize("n", SIZES, ids=lambda n: "n%d" % n)
def test_fused_adam_average(lib, n, variant, mode):
    scale_on, l2, sumsq, off = VARIANTS[variant]
    decay, warmup = MODES[mode]
    omd = 1.0 - decay
    rng = np.random.default_rng(n % 1000 + 17)
    init = dict(p=rng.standard_normal(n, dtype=np.float32), m=0.01 * rng.standard_normal(n, dtype=np.float32),
                v=1e-4 * rng.random(n, dtype=np.float32))
    init["e"] = init["p"] + 0.1 * rng.standard_normal(n, dtype=np.float32)
    # three buffer sets: [0] the fused entry, [1] the plain Adam entry alone, [2] the plain entry followed by the stand-alone average
    sets = [{k: banded(a, off) for k, a in init.items()} for _ in range(3)]
    lr, sc = dev(np.float32([1e-3])), (dev(np.float32([0.37])) if scale_on else None)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    sp = P(step) if warmup else None
    nb = lib.vc_adam_blocks(n)
    parts = [banded(np.zeros(nb, np.float32)) for _ in range(3)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n)
    hist = []
    for s in range(STEPS):
        g = torch.randn(n, generator=gen, device="cuda")    # fresh gradients each step
        step += 1                                            # the counter holds the number of updates including this one
        a = {k: P(t[1]) for k, t in sets[0].items()}
        if sumsq:
            lib.vc_adam_sumsq_ema_f32(stream(), a["p"], P(g), a["m"], a["v"], a["e"], n, P(lr), P(sc), 0.8, 0.999, 1e-8, l2, omd, sp, P(parts[0][1]))
        else:
            lib.vc_adam_ema_f32(stream(), a["p"], P(g), a["m"], a["v"], a["e"], n, P(lr), P(sc), 0.8, 0.999, 1e-8, l2, omd, sp)
        for i in (1, 2):   # (the unfused partner of each fused entry is the plain entry of the same form: vc_adam_f32 / vc_adam_sumsq_f32)
            a = {k: P(t[1]) for k, t in sets[i].items()}
            if sumsq:
                lib.vc_adam_sumsq_f32(stream(), a["p"], P(g), a["m"], a["v"], n, P(lr), P(sc), 0.8, 0.999, 1e-8, l2, P(parts[i][1]))
            else:
                lib.vc_adam_f32(stream(), a["p"], P(g), a["m"], a["v"], n, P(lr), P(sc), 0.8, 0.999, 1e-8, l2)
        lib.vc_ema_update_f32(stream(), P(sets[2]["e"][1]), P(sets[2]["p"][1]), n, omd, sp)
        hist.append(host(sets[0]["p"][1]).copy())
    # 1. the update itself is the plain entry's, bit for bit
    for k in ("p", "m", "v"):
        np.testing.assert_array_equal(host(sets[0][k][1]), host(sets[1][k][1]), err_msg=k)
        np.testing.assert_array_equal(host(sets[2][k][1]), host(sets[1][k][1]), err_msg=k)
    assert not np.array_equal(hist[-1], init["p"])
    if sumsq:
        np.testing.assert_array_equal(host(parts[0][1]), host(parts[1][1]), err_msg="sumsq partials")
        assert host(parts[0][1]).sum() > 0 and all(bands_intact(f, nb) for f, _ in parts)
    # 2. the fused average is the two-launch form's, bit for bit
    got = host(sets[0]["e"][1])
    np.testing.assert_array_equal(got, host(sets[2]["e"][1]), err_msg="fused against adam + ema_update")
    np.testing.assert_array_equal(host(sets[1]["e"][1]), init["e"])    # (the plain entry knows no average)
    # 3. ... and the float64 recurrence over the parameter history, within the derived bound
    R.assert_within_bound(got, init["e"], hist, omd, 1, warmup, msg="ema n=%d %s %s" % (n, variant, mode))
    if warmup and decay == 0.5:   # the constant-weight recurrence is another one: the warm-up was applied
        const, M = R.ema_steps(init["e"], hist, omd, warmup=False)
        assert (np.abs(got - const) > R.bound(M, STEPS)).any()
    # 4. nothing outside the buffers
    for i, bufs in enumerate(sets):
        for k, (flat, _) in bufs.items():
            assert bands_intact(flat, n, off), "guard band of %s (set %d) written" % (k, i)


@pytest.mark.parametrize("n", [3, 4, 1027, 2 ** 20 + 5], ids=lambda n: "n%d" % n)
def test_swap(lib, n):
    rng = np.random.default_rng(n)
    a0, b0 = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    (fa, a), (fb, b) = banded(a0), banded(b0, 64)
    lib.vc_swap_f32(stream(), P(a), P(b), n)
    np.testing.assert_array_equal(host(a), b0)
    np.testing.assert_array_equal(host(b), a0)
    lib.vc_swap_f32(stream(), P(a), P(b), n)
    np.testing.assert_array_equal(host(a), a0)
    np.testing.assert_array_equal(host(b), b0)
    assert bands_intact(fa, n) and bands_intact(fb, n, 64)


# ------------------------------------------------------------------------------------------------ engines
V_, B_, TT = 203, 4, 6
DECAY = 0.9
BOS, EOS = 1, 2


def _engine_steps(lib, nsteps=3, **kw):
    p = small_params(prior="Normal", **kw)
    P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
    eng = CaptionEngine(p, V_, lib=lib)
    eng.load_params(P0)
    hist = [host(eng.store.p).copy()]
    for _ in range(nsteps):
        eng.set_batch(batch, noise)
        eng.forward(); eng.backward(); eng.pack_tail(); eng.apply_gradients()
        hist.append(host(eng.store.p).copy())
    return eng, hist


@pytest.mark.parametrize("optimizer", ["Adam", "SGD", "Momentum"])
def test_engine_steps_average_without_changing_the_update(lib, optimizer):
    off, h_off = _engine_steps(lib, optimizer=optimizer)
    on, h_on = _engine_steps(lib, optimizer=optimizer, ema_decay=DECAY)
    assert "ema" not in off.store.slots and "ema" in on.store.slots
    for a, b in zip(h_off, h_on):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(h_on[0], h_on[-1])
    assert int(on.step.item()) == 3 and on.ema_warmup
    got = host(on.store.slots["ema"])
    R.assert_within_bound(got, h_on[0], h_on[1:], 1.0 - DECAY, 1, True, msg="caption store, " + optimizer)
    assert np.abs(got - h_on[-1]).max() > 0
    assert on.Vp > on.V
    for name in ("decoder/rnn_logits/kernel", "decoder/rnn_logits/bias"):   # the padded vocabulary columns stay zero
        assert (host(on.store.average(name))[..., on.V:] == 0).all() and np.abs(host(on.store.average(name))[..., :on.V]).max() > 0
    avg = on.averages_dict()
    assert set(avg) == set(on.state_dict()) and avg["decoder/rnn_logits/kernel"].shape == (on.p.decoder_hidden, V_)


class _NoNewEntries(object):
    """the loaded library, except that resolving an entry of this feature is an error (the guard of tests/test_gpu_bow.py)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in NEW_ENTRIES:
            raise AssertionError("%s resolved with --ema_decay at its default" % name)
        return getattr(self._lib, name)


def test_defaults_resolve_none_of_the_new_entries(lib):
    guard = _NoNewEntries(lib)
    for optimizer in ("Adam", "SGD", "Momentum"):
        p = small_params(prior="Normal", optimizer=optimizer)
        P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
        tr = Trainer(p, V_, lib=guard)
        tr.load_state_dict(P0)
        for _ in range(2):
            tr.set_batch(batch, noise)
            tr.train_step()
        assert all(np.isfinite(tr.losses()))
        assert "ema" not in tr.cap.store.slots and tr.ema_decay == 0
        assert not any(k.endswith(EMA_SUFFIX) for k in tr.state_dict())
    # ... and the guard is not vacuous: with the flag on, the same step goes through the new entry
    p = small_params(prior="Normal", ema_decay=DECAY)
    P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
    eng = CaptionEngine(p, V_, lib=guard)
    eng.load_params(P0)
    eng.set_batch(batch, noise)
    eng.forward(); eng.backward(); eng.pack_tail()
    with pytest.raises(AssertionError, match="vc_adam_ema_f32"):
        eng.apply_gradients()


def test_captured_step_equals_eager(lib):
    p = small_params(prior="Normal", ema_decay=DECAY)
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
            tr.load_state_dict(P0)   # (also puts the averages back on the parameters)
            for name, s in tr.cap.store.slots.items():
                if name != "ema":
                    s.zero_()
        e0 = host(tr.cap.store.slots["ema"]).copy()
        hist = []
        for b in batches:
            tr.set_batch(b)
            tr.train_step()
            hist.append(host(tr.cap.store.p).copy())
        res.append((e0, hist, host(tr.cap.store.slots["ema"]).copy(), tr.losses()))
    (e0, hist, ema, losses), (e0g, histg, emag, lossesg) = res
    np.testing.assert_array_equal(e0, e0g)
    for a, b in zip(hist, histg):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ema, emag)
    assert losses == lossesg
    # the replays advanced the warm-up: the averages are the warm-up recurrence's, and not what a constant weight would give
    R.assert_within_bound(emag, e0g, histg, 1.0 - DECAY, 1, True, msg="captured step")
    const, M = R.ema_steps(e0g, histg, 1.0 - DECAY, warmup=False)
    assert (np.abs(emag - const) > 100 * R.bound(M, 3)).any()


def test_forced_single_rank_collectives(lib):
    p = small_params(prior="Normal", ema_decay=DECAY)
    P0, batch, noise = make_case(p, V_, B_, TT, seed=9)
    res = []
    for force in (False, True):
        tr = Trainer(p, V_, lib=lib, force_collectives=force)
        tr.load_state_dict(P0)
        for _ in range(2):
            tr.set_batch(batch, noise)
            tr.train_step()
        res.append(tr.cap.averages_dict())
        if tr.comm is not None:
            tr.comm.destroy()
    assert set(res[0]) == set(res[1])
    for k in res[0]:   # (the tolerance that pattern uses for its losses, here of each tensor's maximum)
        assert_close(res[1][k], res[0][k], 2e-4, msg=k)


def test_fine_tune_averages_both_parts(lib, monkeypatch):
    """Two fine-tune steps of the two-image trainer with weight decay (so the update is the sum-of-squares form) on both `part`s: the
    cnn/* parameters and the regulariser's sum are the flag-off run's, the averages the recurrence's.  The whole 134 M-element store is
    checked against the recurrence in float64 on the device; the convolution part and fc2 also against tests/ema_ref.py on the host
    (which the device recurrence, made of the same separately rounded operations, must equal there exactly)."""
    from .gpu_util_step import tiny_finetune_trainer
    out = {}
    for decay in (0.0, DECAY):
        monkeypatch.setattr(Parameters, "ema_decay", decay)
        tr = tiny_finetune_trainer()
        S = tr.vgg.store
        assert tr.vgg.wd > 0 and tr.vgg.train
        hist = [S.p.clone()]
        for _ in range(2):
            tr.train_step()
            hist.append(S.p.clone())
        assert tr.vgg.w2_valid
        reg = zeros(1)
        tr.vgg.reg_sumsq(P(reg))       # the next step's L2 term, from the sum-of-squares partials of the last update
        out[decay] = dict(hist=hist, reg=host(reg).copy(), ema=S.slots.get("ema"), cap=host(tr.cap.store.p).copy(), o_fc=tr.vgg.o_fc,
                          fc2=S.offset("cnn/fc2/weights"), slots=set(S.slots), cap_slots=set(tr.cap.store.slots), step=int(tr.cap.step.item()))
        del tr
    off, on = out[0.0], out[DECAY]
    assert "ema" not in off["slots"] and "ema" in on["slots"] and "ema" in on["cap_slots"] and on["step"] == 2
    for a, b in zip(off["hist"], on["hist"]):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(off["cap"], on["cap"])
    np.testing.assert_array_equal(off["reg"], on["reg"])
    assert float(on["reg"][0]) > 0
    hist, ema = on["hist"], on["ema"]
    e = hist[0].double()
    M = e.abs()
    for t, p in enumerate(hist[1:], 1):
        w = float(R.weight(1.0 - DECAY, t))
        d = p.double() - e
        d = d * w
        e = e + d
        M = torch.maximum(M, torch.maximum(p.double().abs(), e.abs()))
    err = (ema.double() - e).abs()
    tol = R.ULP_BOUND * 2 * M
    print("cnn/* averages: max err %.3e, max bound %.3e" % (float(err.max()), float(tol.max())))
    assert bool(torch.isfinite(ema).all()) and bool((err <= tol).all())
    assert float((ema - hist[-1]).abs().max()) > 0
    for lo, hi in ((0, on["o_fc"]), (on["fc2"], ema.numel())):   # the conv part; fc2 (the tail of the fc part)
        h = [host(x[lo:hi]) for x in hist]
        ref, _ = R.ema_steps(h[0], h[1:], 1.0 - DECAY, 1, True)
        np.testing.assert_array_equal(host(e[lo:hi]), ref)
        R.assert_within_bound(host(ema[lo:hi]), h[0], h[1:], 1.0 - DECAY, 1, True, msg="cnn/* [%d, %d)" % (lo, hi))


# ------------------------------------------------------------------------------------------------ Trainer.ema_weights()
def _peaked(p, seed):
    """parameters with peaked predictions (tests/test_gpu_generate.py), so that two sets of them decode to different captions"""
    rng = np.random.default_rng(seed)
    P0 = spec.init_caption_params(p, V_, seed=seed)
    return {k: (v * 3).astype(np.float32) if not k.endswith("bias") else rng.normal(0, 0.5, v.shape).astype(np.float32) for k, v in P0.items()}


def test_ema_weights_swaps_the_model(lib):
    p = small_params(prior="Normal", ema_decay=DECAY)
    _, batch, noise = make_case(p, V_, B_, TT, seed=7)
    tr = Trainer(p, V_, lib=lib)
    tr.load_state_dict(_peaked(p, 5))
    for _ in range(2):
        tr.set_batch(batch, noise)
        tr.train_step()
    # averages far from the parameters (another model altogether), so that a stale cache shows
    tr.cap._load_into(tr.cap.store.average, _peaked(p, 6), [])
    rng = np.random.default_rng(3)
    feats = np.maximum(rng.standard_normal((B_, p.cnn_feature_size)), 0).astype(np.float32)
    eps = rng.standard_normal((p.gen_z_samples, B_, p.latent_size)).astype(np.float32)
    decode = lambda g: g.greedy(feats, None, eps, BOS, EOS, max_len=12)
    gen = CaptionGenerator(tr.cap)
    caps_p = decode(gen)                                   # builds the generator's derived operands on the PARAMETERS
    tr.set_batch(batch, noise)
    loss_p = tr.eval_rec_loss()
    p_before, e_before = host(tr.cap.store.p).copy(), host(tr.cap.store.slots["ema"]).copy()
    # the reference: a fresh trainer (flag off) whose parameters are the first one's averages
    fresh = Trainer(small_params(prior="Normal"), V_, lib=lib)
    fresh.load_state_dict(tr.cap.averages_dict())
    fresh.cap.step.copy_(tr.cap.step)
    fresh.set_batch(batch, noise)
    loss_ref = fresh.eval_rec_loss()
    caps_ref = decode(CaptionGenerator(fresh.cap))
    assert caps_ref != caps_p and loss_ref != loss_p       # (otherwise nothing below could show a stale cache)
    v0 = tr.cap.param_version
    with tr.ema_weights() as same:
        assert same is tr
        v1 = tr.cap.param_version
        np.testing.assert_array_equal(host(tr.cap.store.p), e_before)
        np.testing.assert_array_equal(host(tr.cap.store.slots["ema"]), p_before)
        tr.set_batch(batch, noise)
        assert tr.eval_rec_loss() == loss_ref
        assert decode(gen) == caps_ref
        with pytest.raises(RuntimeError, match="does not nest"):
            with tr.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="no training step inside ema_weights"):
            tr.train_step()
        np.testing.assert_array_equal(host(tr.cap.store.p), e_before)   # (the refused calls changed nothing)
    v2 = tr.cap.param_version
    assert v0 != v1 and v1 != v2
    np.testing.assert_array_equal(host(tr.cap.store.p), p_before)
    np.testing.assert_array_equal(host(tr.cap.store.slots["ema"]), e_before)
    assert decode(gen) == caps_p
    tr.set_batch(batch, noise)
    assert tr.eval_rec_loss() == loss_p
    with tr.ema_weights():                                  # ... and it can be entered again
        assert decode(gen) == caps_ref
    # an exception inside the block still swaps back
    with pytest.raises(ZeroDivisionError):
        with tr.ema_weights():
            1 / 0
    np.testing.assert_array_equal(host(tr.cap.store.p), p_before)
    with pytest.raises(RuntimeError, match="--ema_decay"):
        with fresh.ema_weights():
            pass


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("fmt", ["npz", "bundle"])
def test_checkpoints_carry_the_averages(lib, tmp_path, capsys, fmt):
    path = lambda name: str(tmp_path / (name + (".npz" if fmt == "npz" else ".ckpt")))
    off, on = small_params(prior="GMM"), small_params(prior="GMM", ema_decay=DECAY)   # (GMM: the encoder heads are stored fused)
    P0, batch, noise = make_case(on, V_, B_, TT, seed=7)
    host_cnn = {"cnn/fc2/biases": np.arange(4096, dtype=np.float32)}   # VGG16 constants carried on the host: not trained, no averages
    tr = Trainer(on, V_, lib=lib)
    tr.load_state_dict(dict(P0, **host_cnn))
    for _ in range(2):
        tr.set_batch(batch, noise)
        tr.train_step()
    sd = tr.state_dict()
    old = Trainer(off, V_, lib=lib)
    old.load_state_dict(dict(P0, **host_cnn))
    plain = set(old.state_dict())
    trained = plain - set(host_cnn)
    assert plain == set(P0) | set(host_cnn) and "encoder/gmm_ll_0/dense/kernel" in plain and "encoder/heads/kernel" in tr.cap.store.names()
    assert set(sd) == plain | {k + EMA_SUFFIX for k in trained}
    assert sd["decoder/rnn_logits/kernel" + EMA_SUFFIX].shape == (on.decoder_hidden, V_)          # padded columns cut
    heads = [k for k in trained if "_ll_" in k]
    assert heads and all(sd[k + EMA_SUFFIX].shape == sd[k].shape for k in heads)                 # fused heads split again
    assert any(not np.array_equal(sd[k], sd[k + EMA_SUFFIX]) for k in trained)
    # save -> restore: parameters and averages exactly, constant decay from then on
    tr.save(path("new"))
    tr2 = Trainer(on, V_, lib=lib, seed=4)
    capsys.readouterr()
    tr2.restore(path("new"))
    out = capsys.readouterr().out
    assert out.count("weight averaging: averages loaded") == 1 and "constant decay" in out and not tr2.cap.ema_warmup
    sd2 = tr2.state_dict()
    assert set(sd2) == set(sd)
    for k in sd:
        np.testing.assert_array_equal(sd2[k], sd[k], err_msg=k)
    # a checkpoint from before the flag: the averages start from the parameters, and a line says so
    old.save(path("old"))
    tr3 = Trainer(on, V_, lib=lib, seed=5)
    capsys.readouterr()
    tr3.restore(path("old"))
    out = capsys.readouterr().out
    assert out.count("the averages start from the parameters") == 1 and tr3.cap.ema_warmup
    sd3 = tr3.state_dict()
    for k in trained:
        np.testing.assert_array_equal(sd3[k], P0[k], err_msg=k)
        np.testing.assert_array_equal(sd3[k + EMA_SUFFIX], P0[k], err_msg=k)
    np.testing.assert_array_equal(host(tr3.cap.store.slots["ema"]), host(tr3.cap.store.p))
    # use_ema: the averages AS the parameters
    tr4 = Trainer(off, V_, lib=lib)
    tr4.restore(path("new"), use_ema=True)
    sd4 = tr4.state_dict()
    assert set(sd4) == plain
    for k in trained:
        np.testing.assert_array_equal(sd4[k], sd[k + EMA_SUFFIX], err_msg=k)
    np.testing.assert_array_equal(sd4["cnn/fc2/biases"], host_cnn["cnn/fc2/biases"])
    with pytest.raises(KeyError, match="--use_ema"):
        tr4.restore(path("old"), use_ema=True)
    # the flag off: averages in the checkpoint are ignored, a line says so, and the next save has none
    capsys.readouterr()
    old.restore(path("new"))
    out = capsys.readouterr().out
    assert out.count("ignored") == 1 and EMA_SUFFIX in out
    sd5 = old.state_dict()
    assert set(sd5) == plain
    for k in plain:
        np.testing.assert_array_equal(sd5[k], sd[k], err_msg=k)
    old.save(path("again"))
    if fmt == "npz":
        with np.load(path("again")) as z:
            keys = set(z.files)
    else:
        from vae_captioning_amd import tf_bundle
        keys = set(tf_bundle.read_bundle(path("again")))
    assert keys == plain


# ------------------------------------------------------------------------------------------------ command line
def test_main_cli_trains_with_averages_and_decodes_with_them(tmp_path):
    import main as M
    from vae_captioning_amd.vae_model.decoder import Decoder
    env = dict(os.environ, PYTHONPATH=ROOT)
    model = ["--synthetic", "--vocab", "120", "--bs", "2", "--embed_dim", "32", "--enc_hid", "32", "--dec_hid", "32", "--latent", "8",
             "--gen_z_samples", "3", "--checkpoint", "ematest", "--ckpt_format", "npz"]
    cmd = [sys.executable, os.path.join(ROOT, "main.py")] + model
    r = subprocess.run(cmd + ["--epochs", "1", "--max_steps", "6", "--ema_decay", "0.9"], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(l.startswith("Weight averaging: decay 0.9") for l in lines), r.stdout
    first = [l for l in lines if l.startswith("Validation reconstruction loss: ")]
    second = [l for l in lines if l.startswith("Validation reconstruction loss (averaged weights, decay 0.9): ")]
    assert len(first) == 1 and len(second) == 1, r.stdout
    assert np.isfinite(float(second[0].split(": ")[1])) and second[0].split(": ")[1] != first[0].split(": ")[1]
    ckpt = str(tmp_path / "checkpoints" / "ematest.ckpt.npz")
    with np.load(ckpt) as z:
        keys = set(z.files)
    avgs = {k for k in keys if k.endswith(EMA_SUFFIX)}
    assert avgs and {k[:-len(EMA_SUFFIX)] for k in avgs} == {k for k in keys - avgs if not k.startswith("cnn/")}
    infer = ["--mode", "inference", "--use_ema", "--sample_gen", "greedy", "--gen_name", "e1", "--eval_captions"]
    r = subprocess.run(cmd + infer, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "restoring the averaged weights" in r.stdout
    caps = json.load(open(tmp_path / "val_e1.json"))
    assert json.load(open(tmp_path / "val_e1_metrics.json"))["use_ema"] is True
    # the same decode in this process, on a trainer restored with use_ema=True
    params = Parameters().parse_args(model + infer)
    tr = Trainer(params, params.vocab_size, seed=params.seed)
    params._vc_trainer = tr
    tr.restore(ckpt, use_ema=True)
    with np.load(ckpt) as z:
        np.testing.assert_array_equal(tr.state_dict()["decoder/rnn_logits/bias"], z["decoder/rnn_logits/bias" + EMA_SUFFIX])
    decoder = Decoder(None, None, None, params, M.SyntheticDictionary(params.vocab_size))
    rng = np.random.default_rng(params.seed + 5)
    want = []
    for it in range(2):
        b = synth.make_batch(rng, params.batch_size, 1, 20, params.vocab_size, use_ci=spec.uses_ci(params), images=False)
        ids = ["synthetic_%06d" % (it * params.batch_size + i) for i in range(params.batch_size)]
        want += decoder.decode(params.sample_gen, ids, b["features"], b.get("c_v"))
    assert caps == want and len(caps) == 4
