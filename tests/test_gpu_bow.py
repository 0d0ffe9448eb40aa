"""-m gpu: the bag-of-words auxiliary loss -- vc_bow_xent_f32 through the C ABI against the float64 reference (tests/bow_ref.py), whole
training steps with the head against float64 autograd, the promise that the option at its default resolves nothing of it, capture,
collectives, scheduled sampling, checkpoints from before the head, and what it is for: a head trained on z_rnn(z) predicts the words of
ITS caption better than those of another image's.

Tolerances are the logits-row family's (tests/test_gpu_unlikelihood.py): 1e-5 of the tensor maximum for the kernel, 2e-4 relative on
losses and 2e-4 of each tensor's maximum on gradients for whole steps.  row_words and everything compared between two runs of the same
kernels are exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import abi, spec, synth
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.trainer import Trainer
from vae_captioning_amd.utils.parameters import Parameters

from . import bow_ref as R
from .gpu_util import P, assert_close, dev, host, stream, zeros
from .test_gpu_engine import make_case, small_params
from .unlikelihood_ref import UL_SHAPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("vc_bow_xent_f32", "vc_bow_stats_f32")
ROWS = R.N_CASE
POISON = -7.0


# ------------------------------------------------------------------------------------------------ the kernel
def _buffers(buf, ld, off, rows=ROWS):
    flat = torch.zeros(rows * ld + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + rows * ld].view(rows, ld)
    view.copy_(torch.from_numpy(buf))
    return flat, view


def _outputs(rows=ROWS):
    """row_loss, row_mass, row_words with two poisoned elements behind the rows"""
    return zeros(rows + 2).fill_(POISON), zeros(rows + 2).fill_(POISON), torch.full((rows + 2,), int(POISON), dtype=torch.int32, device="cuda")


def _untouched(rl, rm, rw, rows=ROWS):
    return (host(rl)[rows:] == POISON).all() and (host(rm)[rows:] == POISON).all() and (host(rw)[rows:] == int(POISON)).all()


def _call(lib, view, dl, V, ld, T, den, gscale, write_grad, rows=ROWS, ldl=ROWS):
    rl, rm, rw = _outputs()
    lib.vc_bow_xent_f32(stream(), view.data_ptr(), rows, V, ld, P(dl), T, ldl, P(den), gscale, P(rl), P(rm), P(rw), write_grad)
    return rl, rm, rw


@pytest.mark.parametrize("T", [1, 7, 64, 65, 256])
@pytest.mark.parametrize("shape", UL_SHAPES, ids=lambda s: "V%d-ld%d-off%d" % s)
def test_kernel_matches_the_reference(lib, shape, T):
    V, ld, off = shape
    buf, labels = R.bow_case(V, ld, off, T)
    gscale = 3.0
    c = R.bow_rows(buf[:, :V], labels, gscale)
    flat, view = _buffers(buf, ld, off)
    dl, den = dev(labels.reshape(-1)), zeros(1)
    lib.vc_count_nonzero_i32(stream(), P(dl), T * ROWS, P(den))
    assert float(host(den)[0]) == float((labels != 0).sum())
    # forward only: the logits -- padding included -- stay as they are
    rl, rm, rw = _call(lib, view, dl, V, ld, T, den, gscale, 0)
    np.testing.assert_array_equal(host(view), buf)
    for got, name in ((rl, "row_loss"), (rm, "row_mass")):
        print(name, "max err", np.abs(host(got)[:ROWS] - c[name]).max(), "of", np.abs(c[name]).max())
        assert_close(host(got)[:ROWS], c[name], 1e-5, msg=name)
    np.testing.assert_array_equal(host(rw)[:ROWS], c["row_words"])
    assert _untouched(rl, rm, rw)
    # with the gradient
    rl, rm, rw = _call(lib, view, dl, V, ld, T, den, gscale, 1)
    got = host(view)
    for g, name in ((rl, "row_loss"), (rm, "row_mass")):
        assert_close(host(g)[:ROWS], c[name], 1e-5, msg=name + " (with gradient)")
    np.testing.assert_array_equal(host(rw)[:ROWS], c["row_words"])
    assert _untouched(rl, rm, rw)
    print("dlogits max err", np.abs(got[:, :V] - c["dlogits"]).max(), "of", np.abs(c["dlogits"]).max())
    assert_close(got[:, :V], c["dlogits"], 1e-5, msg="dlogits")
    assert (got[:, V:] == 0).all(), "pitch padding must come back exactly 0"
    assert (got[3] == 0).all() and host(rl)[3] == 0 and host(rm)[3] == 0 and host(rw)[3] == 0, "the all-PAD caption must come back all-zero"
    assert (host(flat)[:off] == 0).all() and (host(flat)[off + ROWS * ld:] == 0).all()   # nothing outside the rows


@pytest.mark.parametrize("T", [64, 256])
@pytest.mark.parametrize("shape", [(203, 204, 0), (203, 205, 0)], ids=["reg", "mem"])
def test_multiplicity(lib, shape, T):
    """a caption that is one word T times has gradient k T (p_v - [v = w]) and one distinct word"""
    V, ld, off = shape
    w, rows, gscale = V - 1, 2, 2.0
    rng = np.random.default_rng(T + ld)
    buf = np.full((rows, ld), R.GUARD, np.float32)
    buf[:, :V] = rng.standard_normal((rows, V), dtype=np.float32) * np.float32(3)
    labels = np.zeros((T, rows), np.int32)
    labels[:, 1] = w
    flat, view = _buffers(buf, ld, off, rows)
    dl, den = dev(labels.reshape(-1)), zeros(1).fill_(float(T))
    rl, rm, rw = _outputs(rows)
    lib.vc_bow_xent_f32(stream(), view.data_ptr(), rows, V, ld, P(dl), T, rows, P(den), gscale, P(rl), P(rm), P(rw), 1)
    x = buf[1, :V].astype(np.float64)
    p = np.exp(x - x.max()); p /= p.sum()
    ref = gscale / T * T * (p - (np.arange(V) == w))
    got = host(view)
    assert_close(got[1, :V], ref, 1e-5, msg="dlogits")
    assert (got[0] == 0).all() and (got[:, V:] == 0).all()
    assert list(host(rw)[:rows]) == [0, 1]
    assert abs(host(rm)[1] - p[w]) <= 1e-5 * p[w] + 1e-7
    assert abs(host(rl)[1] - T * -np.log(p[w])) <= 1e-5 * T * -np.log(p[w])


def test_bad_arguments_are_errors_before_any_launch(lib):
    V, ld, T = 203, 204, 7
    buf, labels = R.bow_case(V, ld, 0, T)
    flat, view = _buffers(buf, ld, 0)
    big = dev(np.zeros(257 * ROWS, np.int32))
    dl, den = dev(labels.reshape(-1)), zeros(1).fill_(1.0)
    rl, rm, rw = _outputs()
    ok = dict(logits=view.data_ptr(), rows=ROWS, V=V, ld=ld, labels=P(dl), T=T, ldl=ROWS, den=P(den), rl=P(rl), rm=P(rm), rw=P(rw))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vc_bow_xent_f32(stream(), a["logits"], a["rows"], a["V"], a["ld"], a["labels"], a["T"], a["ldl"], a["den"], 3.0, a["rl"], a["rm"],
                                   a["rw"], 1)
    for bad in (dict(T=257, labels=P(big)), dict(T=0), dict(T=-1), dict(ldl=ROWS - 1), dict(V=0), dict(V=-3), dict(ld=V - 1), dict(rows=-1),
                dict(logits=None), dict(labels=None), dict(den=None), dict(rl=None), dict(rm=None), dict(rw=None)):
        with pytest.raises(abi.VaecapError, match="vc_bow_xent_f32"):
            call(**bad)
    assert call(rows=0) == 0 and call(rows=0, ldl=0) == 0          # a successful no-op
    np.testing.assert_array_equal(host(view), buf)                 # nothing ran
    assert (host(rl) == POISON).all() and (host(rm) == POISON).all() and (host(rw) == int(POISON)).all()
    assert call(T=256, labels=P(big)) == 0                         # ... and the largest T is no error


def test_stats_entry(lib):
    V, ld, T = 203, 204, 7
    buf, labels = R.bow_case(V, ld, 0, T)
    c = R.bow_rows(buf[:, :V], labels)
    flat, view = _buffers(buf, ld, 0)
    dl = dev(labels.reshape(-1))
    rl, rm, rw = _call(lib, view, dl, V, ld, T, None, 1.0, 0)
    out = zeros(3).fill_(POISON)
    lib.vc_bow_stats_f32(stream(), ROWS, V, P(dl), T, ROWS, P(rl), P(rm), P(rw), P(out))
    s = R.bow_stats(c)
    assert_close(host(out), np.array([s["bow"], s["bow_words"], s["bow_mass"]]), 1e-5, msg="stats")
    # every bag empty: zeros
    dz = dev(np.zeros(T * ROWS, np.int32))
    rl, rm, rw = _call(lib, view, dz, V, ld, T, None, 1.0, 0)
    lib.vc_bow_stats_f32(stream(), ROWS, V, P(dz), T, ROWS, P(rl), P(rm), P(rw), P(out))
    assert (host(out) == 0).all()


# ------------------------------------------------------------------------------------------------ whole steps
PRIORS = {"Normal": dict(prior="Normal"), "GMM": dict(prior="GMM"), "AG_cv": dict(prior="AG", use_c_v=True)}
STEP_OPTIONS = {"bow": dict(bow_loss=1.0), "bow_ls_fb": dict(bow_loss=1.0, label_smoothing=0.1, kl_free_bits=0.05)}
# at seed 7 the float64 reference keeps every kl[n,l] of all three steps at least 1e-4 away from the floor (asserted below)
V_, B_, TT = 203, 4, 6
STATS = ("bow", "bow_words", "bow_mass")


@pytest.mark.parametrize("options", list(STEP_OPTIONS), ids=str)
@pytest.mark.parametrize("prior", list(PRIORS), ids=str)
def test_train_steps_match_autograd(lib, prior, options):
    p = small_params(**PRIORS[prior], **STEP_OPTIONS[options])
    P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
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
        assert {"bow/kernel", "bow/bias", "decoder/net/z_rnn/kernel", "encoder/enc_embeddings", spec.ENC_CELL + "kernel"} <= set(h["grads"])
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
        for key in STATS:
            assert abs(o[key] - h[key]) <= 2e-4 * abs(h[key]), (key, s, o[key], h[key])
        assert ("kl_raw" in o) == (p.kl_free_bits > 0)
    Pg = eng.state_dict()
    assert set(Pg) == set(Pref)
    for name, ref in Pref.items():
        upd = np.abs(ref - P0[name]).max()
        err = np.abs(Pg[name] - ref).max()
        assert err <= 2e-3 * upd + 1e-7, "param %s after 3 steps: err %.3e, update size %.3e" % (name, err, upd)


def test_training_step_in_bf16x3_mode(lib):
    """one step with every dense product (the head's three among them) on the split-bf16 path: loss / KL within 1e-3, gradients within 1e-3
    of their maximum (the step bounds of tests/test_gpu_bf16x3.py)"""
    p = small_params(prior="Normal", bow_loss=1.0)
    P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
    h = R.reference_steps(p, P0, batch, noise, 1)[0][0]
    eng = CaptionEngine(p, V_, lib=lib)
    eng.set_precision("bf16x3")
    eng.load_params(P0)
    eng.set_batch(batch, noise)
    eng.forward()
    eng.backward()
    eng.pack_tail()
    G = eng.grads_dict()
    eng.apply_gradients()
    kld, rec, lb, ann = eng.losses()
    assert abs(rec - h["rec"]) < 1e-3 and abs(kld - h["kld"]) < 1e-3
    assert abs(eng.objective_stats()["bow"] - h["bow"]) < 1e-3
    for name, g in h["grads"].items():
        err = np.abs(G[name] - g).max()
        assert err <= 1e-3 * (np.abs(g).max() + 1e-12), (name, err)


def _with_head(p_on, P0, V):
    """P0 of a flag-off case plus the head's two arrays (make_case with the flag on would draw another batch: bow/bias moves its stream)"""
    extra = spec.init_caption_params(p_on, V, seed=8)
    return dict(P0, **{k: extra[k] for k in ("bow/kernel", "bow/bias")})


def test_validation_forward_is_bit_identical_with_the_flag_on(lib):
    rec = []
    for A in (0.0, 1.0):
        p = small_params(prior="Normal")
        P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
        if A > 0:
            p = small_params(prior="Normal", bow_loss=A)
            P0 = _with_head(p, P0, V_)
        eng = CaptionEngine(p, V_, lib=lib)
        eng.load_params(P0)
        eng.set_batch(batch, noise)
        eng.forward(train=False)
        rec.append(eng.losses())
        assert "bow_logits" not in eng.buf
    assert rec[0] == rec[1]


class _NoNewEntries(object):
    """the loaded library, except that resolving an entry of this feature is an error (the guard of tests/test_gpu_objective.py)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in NEW_ENTRIES:
            raise AssertionError("%s resolved with --bow_loss at its default" % name)
        return getattr(self._lib, name)


def test_defaults_resolve_none_of_the_new_entries(lib):
    guard = _NoNewEntries(lib)
    for kw in PRIORS.values():
        p = small_params(**kw)
        P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
        assert not any(k.startswith("bow/") for k in P0)
        eng = CaptionEngine(p, V_, lib=guard)
        eng.load_params(P0)
        for _ in range(2):
            eng.set_batch(batch, noise)
            eng.forward(); eng.backward(); eng.pack_tail(); eng.apply_gradients()
        assert all(np.isfinite(eng.losses())) and eng.objective_stats() is None
        assert not any(k.startswith("bow") for k in eng.buf)
        assert not any(k.startswith("bow/") for k in eng.state_dict()) and not any(k.startswith("bow/") for k in eng.store.names())
    # ... and the guard is not vacuous: with the option on, the same step goes through the new entry
    p = small_params(prior="Normal", bow_loss=1.0)
    P0, batch, noise = make_case(p, V_, B_, TT, seed=7)
    eng = CaptionEngine(p, V_, lib=guard)
    eng.load_params(P0)
    eng.set_batch(batch, noise)
    with pytest.raises(AssertionError, match="vc_bow_xent_f32"):
        eng.forward()


def test_captured_step_equals_eager(lib):
    p = small_params(prior="Normal", bow_loss=1.0, label_smoothing=0.1)
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
            losses.append(tr.losses() + tuple(o[k] for k in STATS))
        res.append((losses, tr.state_dict()))
    assert res[0][0] == res[1][0]
    assert all(l[4] > 0 and l[5] > 0 and 0 < l[6] < 1 for l in res[0][0])
    assert "bow/kernel" in res[0][1]
    for k in res[0][1]:
        np.testing.assert_array_equal(res[0][1][k], res[1][1][k], err_msg=k)


def test_forced_single_rank_collectives(lib):
    p = small_params(prior="Normal", bow_loss=1.0)
    P0, batch, noise = make_case(p, V_, B_, TT, seed=9)
    res = []
    for force in (False, True):
        tr = Trainer(p, V_, lib=lib, force_collectives=force)
        tr.load_state_dict(P0)
        for _ in range(2):
            tr.set_batch(batch, noise)
            tr.train_step()
        o = tr.objective_stats()
        res.append(tr.losses() + tuple(o[k] for k in STATS))
        if tr.comm is not None:
            tr.comm.destroy()
    for a, b in zip(res[0], res[1]):
        assert abs(a - b) <= 2e-4 * abs(a), (res[0], res[1])


class _Counting(object):
    """the loaded library, counting the calls of every entry"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_one_step_with_scheduled_sampling_launches_the_head_once(lib):
    p = small_params(prior="Normal", bow_loss=1.0, sched_sampling=0.5, sched_schedule="constant")
    P0 = spec.init_caption_params(p, V_, seed=4)
    batch = synth.make_batch(np.random.default_rng(5), B_, p.num_captions, TT, V_, variable_len=True, feature_size=p.cnn_feature_size)
    count = _Counting(lib)
    tr = Trainer(p, V_, lib=count, seed=9)
    tr.load_state_dict(P0)
    tr.set_batch(batch)
    count.calls.clear()
    tr.train_step()
    o, s = tr.objective_stats(), tr.sched_stats()
    assert all(np.isfinite(tr.losses())) and all(np.isfinite(v) for v in o.values())
    assert s["replaced"] > 0
    assert count.calls["vc_lstm_seq_fwd_f32"] == 3                                   # the encoder and BOTH decoder passes ran
    assert count.calls["vc_bow_xent_f32"] == 1 and count.calls["vc_bow_stats_f32"] == 1
    assert count.calls["vc_count_nonzero_i32"] == 1                                  # the label count moved, it was not doubled
    c = R.bow_rows(np.zeros((B_ * p.num_captions, V_)), batch["cap_enc"].T)
    assert o["bow_words"] == pytest.approx(c["row_words"].sum() / float((c["row_words"] > 0).sum()), rel=1e-6)


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("fmt", ["npz", "bundle"])
def test_checkpoint_from_before_the_head(lib, tmp_path, capsys, fmt):
    off, on = small_params(prior="Normal"), small_params(prior="Normal", bow_loss=1.0)
    path = str(tmp_path / ("old.npz" if fmt == "npz" else "old.ckpt"))
    old = Trainer(off, V_, lib=lib)
    old.load_state_dict(spec.init_caption_params(off, V_, seed=4))
    old.save(path)
    sd_old = old.state_dict()
    assert not any(k.startswith("bow/") for k in sd_old)
    tr = Trainer(on, V_, lib=lib, seed=3)
    fresh = tr.state_dict()
    assert np.abs(fresh["bow/kernel"]).max() > 0 and fresh["bow/kernel"].shape == (on.embed_size, V_)
    capsys.readouterr()
    tr.restore(path)
    out = capsys.readouterr().out
    assert out.count("bag-of-words head keeps its fresh initialisation") == 1 and "bow/kernel" in out and "bow/bias" in out
    sd = tr.state_dict()
    for k in sd_old:
        np.testing.assert_array_equal(sd[k], sd_old[k], err_msg=k)
    np.testing.assert_array_equal(sd["bow/kernel"], fresh["bow/kernel"])
    # the new checkpoint carries the head and restores it; the flag-off trainer ignores it
    sd["bow/bias"] = np.arange(V_, dtype=np.float32)
    tr.load_state_dict(sd)
    new = str(tmp_path / ("new.npz" if fmt == "npz" else "new.ckpt"))
    tr.save(new)
    tr2 = Trainer(on, V_, lib=lib, seed=4)
    tr2.restore(new)
    np.testing.assert_array_equal(tr2.state_dict()["bow/bias"], sd["bow/bias"])
    np.testing.assert_array_equal(tr2.state_dict()["bow/kernel"], sd["bow/kernel"])
    old.restore(new)
    assert not any(k.startswith("bow/") for k in old.state_dict())
    # any other missing name is still the KeyError it was
    lacking = {k: v for k, v in sd_old.items() if k != "decoder/net/z_rnn/bias"}
    with pytest.raises(KeyError, match="z_rnn/bias"):
        tr.load_state_dict(lacking)
    with pytest.raises(KeyError, match="z_rnn/bias"):
        tr.load_state_dict({k: v for k, v in sd.items() if k != "decoder/net/z_rnn/bias"})


# ------------------------------------------------------------------------------------------------ what it is for
def _head_eval(lib, eng, X, labels_t):
    """the head forward-only through the C ABI on the rows X [N, E]: -> (nats per bag word, bow_words, bow_mass)"""
    N, E, V, Vp, T = eng.N, eng.p.embed_size, eng.V, eng.Vp, eng.T
    S = eng.store
    bl = zeros(N, Vp)
    eng.gemm(0, 0, N, Vp, E, X, E, S.param("bow/kernel"), Vp, bl, Vp, S.param("bow/bias"))
    rl, rm, out = zeros(N), zeros(N), zeros(3)
    rw = torch.zeros(N, dtype=torch.int32, device="cuda")
    lib.vc_bow_xent_f32(stream(), P(bl), N, V, Vp, P(labels_t), T, N, None, 1.0, P(rl), P(rm), P(rw), 0)
    lib.vc_bow_stats_f32(stream(), N, V, P(labels_t), T, N, P(rl), P(rm), P(rw), P(out))
    return tuple(float(v) for v in host(out))


# measured on an MI355X (DESIGN.md "Bag-of-words loss"): after the recipe's steps, nats per bag word on matched / deranged rows (gap
# 4.3536; the matched bow_mass went from 0.0372 to 0.5797, the deranged one is 0.2016).  The asserted margin is half the gap.
MEASURED_MATCHED, MEASURED_DERANGED = 2.8250, 7.1786


def test_the_trained_head_reads_its_own_caption_from_z(lib):
    """The sixteen-caption memorisation recipe of tests/test_gpu_score.py (150 Adam steps at 4e-3, seeds 42 / 5 / 3) with bow_loss = 1
    and kl_weight = 0.1 (the test is about the head, not the schedule).  Then the head alone, forward-only, on the z step of a
    validation forward: on Xd[zi] as it is, and on Xd[zi] with its rows moved one image on (a derangement: no caption keeps its own
    z).  A head fed nothing caption-specific scores the two alike."""
    from .test_gpu_score import _params
    p = _params(num_captions=1, batch_size=16, learning_rate=4e-3, prior="Normal", bow_loss=1.0, kl_weight=0.1)
    V, B, T, STEPS = 200, 16, 9, 150
    rng = np.random.default_rng(42)
    batch = synth.make_batch(rng, B, 1, T, V, variable_len=True, feature_size=p.cnn_feature_size)
    tr = Trainer(p, V, lib=lib, seed=5)
    tr.load_state_dict(spec.init_caption_params(p, V, seed=3))
    tr.set_batch(batch)
    eng = tr.cap

    def evaluate():
        eng.forward(train=False)
        zi = eng.n_init_d - 1
        X = eng.buf["Xd"][zi].clone()
        return _head_eval(lib, eng, X, eng.buf["cap_enc_t"]), _head_eval(lib, eng, torch.roll(X, 1, 0).contiguous(), eng.buf["cap_enc_t"])
    before, _ = evaluate()
    for _ in range(STEPS):
        tr.train_step()
    matched, deranged = evaluate()
    print("bow per word: matched %.4f deranged %.4f (gap %.4f); bow_mass matched %.4f -> %.4f, deranged %.4f; rec_loss %.4f"
          % (matched[0], deranged[0], deranged[0] - matched[0], before[2], matched[2], deranged[2], tr.losses()[1]))
    assert matched[2] > before[2]
    margin = 0.5 * (MEASURED_DERANGED - MEASURED_MATCHED)
    assert margin > 0
    assert matched[0] + margin < deranged[0], (matched, deranged, margin)


# ------------------------------------------------------------------------------------------------ CLI
def test_main_cli_prints_the_new_line(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "120", "--bs", "2", "--embed_dim", "32", "--enc_hid", "32",
           "--dec_hid", "32", "--latent", "8", "--gen_z_samples", "3", "--gpu", "0", "--checkpoint", "bowtest", "--ckpt_format", "npz",
           "--max_steps", "3", "--epochs", "1", "--bow_loss", "1"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("BoW: bow:") and "words:" in l and "mass:" in l]
    assert lines, r.stdout
    mass = float(lines[-1].split("mass:")[1])
    assert 0.0 < mass < 1.0
