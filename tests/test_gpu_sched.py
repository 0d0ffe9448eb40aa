"""-m gpu: scheduled sampling in its two-pass form (csrc/sched.hip: vc_sched_mix_f32; CaptionEngine.fw_decode_train; DESIGN.md "Scheduled
sampling").

The kernel alone: exact against two independent kernels (vc_multinomial_rows_f32 / vc_argmax_rows_f32 on the same row and uniform) and,
nothing excluded, against the float64 reference (tests/sched_ref.py) under its delta rule:

    delta = (ceil(V / 256) + 256 + 8) * 2^-23   -- the chunk sums of at most ceil(V / 256) terms, the 256-term serial sum and the final
    comparison each lose at most one ulp per addition, __expf adds a few ulp per term; the bound takes twice their sum.

The step: the mixed inputs a Trainer step leaves are the reference's mix of the first pass's logits; the second pass is, bit for bit, the
plain step on those inputs; a captured step equals the eager one; validation, the policy step and a trainer with the mode off launch what
they launched before."""
import collections
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import abi, spec, synth
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.trainer import Trainer

from . import sched_ref as R
from .gpu_util import P, dev, host, stream, zeros
from .test_gpu_engine import make_case, small_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("vc_sched_mix_f32",)
VOCABS = (1, 2, 255, 256, 257, 1021, 4099, 11313, 19456)
TEMPS = (0.5, 1.0, 2.0)
RATES = (0.0, 0.25, 1.0)
U_MAX = float(np.nextafter(np.float32(1), np.float32(0)))   # the largest float below 1
POISON = -7


def ld_of(V, kind):
    return (V, (V + 3) // 4 * 4, V + 3)[kind]


# ------------------------------------------------------------------------------------------------ the kernel alone
@functools.lru_cache(maxsize=None)
def kernel_case(V, ld, off, T, N, seed, dominant=False):
    """Host arrays of one case (built once, never modified): the flat logits allocation (row 0 starts `off` floats in), the [T, N] gold
    tokens, lens holding 0, 1, 2, T and values in between, coins with one exactly at 0.25 and one at 0, uniforms holding 0, 0.5 and the
    largest float below 1 at eligible positions."""
    rng = np.random.default_rng(seed)
    Rr = T * N
    flat = np.zeros(Rr * ld + 8, np.float32)
    rows = flat[off:off + Rr * ld].reshape(Rr, ld)
    rows[:] = np.float32(1e30)   # the pitch padding: huge, so a read past column V would show
    rows[:, :V] = (3.0 * rng.standard_normal((Rr, V))).astype(np.float32)
    if dominant:
        rows[:, V // 2] = 60.0
    lens = np.array(([0, 1, 2, T, 3, T - 1, 4, T] * (N // 8 + 1))[:N], np.int32).clip(0, T)
    if N == 1:
        lens[:] = min(2, T)
    cap = np.zeros((T, N), np.int32)
    for n in range(N):
        cap[:lens[n], n] = np.concatenate([[1], rng.integers(max(V - 1, 0), max(V, 1), size=T) if V < 4 else rng.integers(3, V, size=T)])[:lens[n]]
    coin, u = rng.random((T, N), dtype=np.float32), rng.random((T, N), dtype=np.float32)
    el = list(zip(*np.nonzero(R.eligible(T, N, lens))))
    for (t, n), v in zip(el[::max(len(el) // 3, 1)], (0.0, 0.5, U_MAX)):
        u[t, n] = v
    if len(el) >= 2:
        coin[el[1]] = np.float32(0.25)   # exactly at the rate: not selected (strict comparison)
        coin[el[-1]] = 0.0               # selected at any positive rate
    for a in (flat, lens, cap, coin, u):
        a.setflags(write=False)
    return dict(flat=flat, view=rows[:, :V], lens=lens, cap=cap, coin=coin, u=u)


def run_mix(lib, c, V, ld, off, T, N, rate, temp, sample, step=1, schedule=0, ramp=1):
    flat = dev(c["flat"])
    assert flat.data_ptr() % 16 == 0
    out = torch.full((T, N), POISON, dtype=torch.int32, device="cuda")
    stats, rate_out, stepd = zeros(2, dtype=torch.int32), zeros(1), dev(np.array([step], np.int32))
    cap, lens, coin, u = dev(c["cap"]), dev(c["lens"]), dev(c["coin"]), dev(c["u"])
    lib.vc_sched_mix_f32(stream(), flat.data_ptr() + 4 * off, ld, V, T, N, P(cap), P(lens), P(coin), P(u) if sample else None, temp, P(stepd),
                         schedule, rate, ramp, P(out), P(stats), P(rate_out))
    chk = torch.full((T * N,), POISON, dtype=torch.int32, device="cuda")   # the independent kernels on rows 0 .. (T-1) N - 1: position (t, n)'s row
    if T > 1:
        if sample:
            lib.vc_multinomial_rows_f32(stream(), flat.data_ptr() + 4 * off, (T - 1) * N, V, ld, temp, u.data_ptr() + 4 * N, chk.data_ptr() + 4 * N)
        else:
            lib.vc_argmax_rows_f32(stream(), flat.data_ptr() + 4 * off, (T - 1) * N, V, ld, chk.data_ptr() + 4 * N)
    assert int(host(stepd)[0]) == step
    return host(out), host(chk).reshape(T, N), host(stats), float(host(rate_out)[0])


def check_mix(c, V, T, N, rate, temp, sample, out, chk, stats, tag):
    """rate: the float32 value the kernel compared the coins with"""
    el = R.eligible(T, N, c["lens"])
    sel = el & (c["coin"] < np.float32(rate))
    np.testing.assert_array_equal(out[~sel], c["cap"][~sel], err_msg="unselected positions copy the gold token: " + tag)
    np.testing.assert_array_equal(out[sel], chk[sel], err_msg="selected positions: the independent kernel's token: " + tag)
    assert tuple(stats) == (int(el.sum()), int(sel.sum())), (tag, stats, el.sum(), sel.sum())
    ref, cdfs = R.mix(c["view"], c["cap"], c["lens"], c["coin"], c["u"] if sample else None, temp, rate)
    np.testing.assert_array_equal(ref[~sel], out[~sel])
    for t, n in zip(*np.nonzero(sel)):
        w, row = int(out[t, n]), c["view"][(t - 1) * N + n]
        if sample:
            cdf = cdfs[(t, n)]
            lo = cdf[w - 1] if 0 < w < V else 0.0
            assert R.accepts(cdf, w, c["u"][t, n]), "%s: (t %d, n %d) word %d for u %.9g outside [%.9g, %.9g) +- %.3g" % (
                tag, t, n, w, c["u"][t, n], lo, cdf[min(max(w, 0), V - 1)], R.delta(V))
        else:
            assert 0 <= w < V and row[w] == row.max() and not (row[:w] == row.max()).any(), (tag, t, n, w)
    return int(sel.sum())


# (V, ld, row-0 offset in floats, T, N): every V with ld == V, the next multiple of 4 and V + 3 (where those differ), at both offsets
KERNEL_CASES = list(dict.fromkeys((V, ld_of(V, kind), off, 5, 7) for V in VOCABS for kind in range(3) for off in (0, 1))) + \
               [(257, 257, 1, 1, 3), (1021, 1024, 0, 2, 1), (257, 260, 0, 21, 64), (4099, 4099, 1, 21, 64), (4099, 4100, 0, 21, 64)]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "V%d-ld%d-off%d-T%d-N%d" % c)
def test_mix_kernel(lib, case):
    V, ld, off, T, N = case
    c = kernel_case(V, ld, off, T, N, seed=V + 7 * ld + off)
    temp = TEMPS[(VOCABS.index(V) + ld + off) % 3]
    nsel = 0
    for sample in (True, False):
        for rate in RATES:
            out, chk, stats, rate_out = run_mix(lib, c, V, ld, off, T, N, rate, temp, sample)
            assert rate_out == rate
            nsel += check_mix(c, V, T, N, rate, temp, sample, out, chk, stats, "sample %s rate %g temp %g" % (sample, rate, temp))
            if rate == 0.0 or T == 1:
                np.testing.assert_array_equal(out, c["cap"])
    assert nsel > 0 or T == 1


@pytest.mark.parametrize("temp", TEMPS)
def test_mix_kernel_at_every_temperature_and_with_a_dominant_logit(lib, temp):
    V, T, N = 1021, 5, 7
    for dominant in (False, True):
        c = kernel_case(V, V + 3, 1, T, N, seed=3, dominant=dominant)
        out, chk, stats, _ = run_mix(lib, c, V, V + 3, 1, T, N, 1.0, temp, True)
        check_mix(c, V, T, N, 1.0, temp, True, out, chk, stats, "temp %g dominant %s" % (temp, dominant))
        if dominant:   # every other word together holds < 1e-8 of the mass: any u above that draws the dominant word (u = 0 draws the first
            el = R.eligible(T, N, c["lens"])   # word whose float32 mass has not underflowed: check_mix's business)
            assert (out[el & (c["u"] >= 2.0 ** -24)] == V // 2).all()


def test_rate_zero_reads_no_logits(lib):
    V, T, N = 257, 5, 7
    c = dict(kernel_case(V, 260, 0, T, N, seed=1))
    c["flat"] = np.full_like(c["flat"], np.nan)
    for sample in (True, False):
        out, _, stats, _ = run_mix(lib, c, V, 260, 0, T, N, 0.0, 1.0, sample)
        np.testing.assert_array_equal(out, c["cap"])
        assert tuple(stats) == (int(R.eligible(T, N, c["lens"]).sum()), 0)


@pytest.mark.parametrize("schedule", [0, 1, 2], ids=R.SCHEDULES)
def test_schedule_from_the_device_step_counter(lib, schedule):
    V, T, N, ramp, rmax = 257, 21, 64, 50, 0.6
    c = kernel_case(V, 260, 0, T, N, seed=2)
    seen = []
    for step in (1, ramp + 1, 10 * ramp):
        out, chk, stats, rate = run_mix(lib, c, V, 260, 0, T, N, rmax, 1.0, True, step=step, schedule=schedule, ramp=ramp)
        ref = R.sched_rate(step - 1, schedule, rmax, ramp)   # the counter has already been incremented: the first step has s = 0
        assert rate == pytest.approx(ref, rel=1e-5, abs=1e-9), (step, rate, ref)
        check_mix(c, V, T, N, rate, 1.0, True, out, chk, stats, "schedule %d step %d" % (schedule, step))
        seen.append(rate)
    if schedule == 0:
        assert seen == [float(np.float32(rmax))] * 3
    elif schedule == 1:
        assert seen[0] == 0.0 and seen[1] == seen[2] == float(np.float32(rmax))
    else:
        assert seen[0] == pytest.approx(rmax / (ramp + 1), rel=1e-5) and seen[0] < seen[1] < seen[2] < rmax and seen[2] > 0.99 * rmax


def test_stats_accumulate_and_are_optional(lib):
    V, T, N = 257, 5, 7
    c = kernel_case(V, 260, 0, T, N, seed=1)
    flat, cap, lens, coin, u, stepd = dev(c["flat"]), dev(c["cap"]), dev(c["lens"]), dev(c["coin"]), dev(c["u"]), dev(np.array([1], np.int32))
    out, stats = zeros(T, N, dtype=torch.int32), dev(np.array([100, 1000], np.int32))
    for st_ptr in (P(stats), None, P(stats)):
        lib.vc_sched_mix_f32(stream(), P(flat), 260, V, T, N, P(cap), P(lens), P(coin), P(u), 1.0, P(stepd), 0, 1.0, 1, P(out), st_ptr, None)
    el = int(R.eligible(T, N, c["lens"]).sum())
    assert tuple(host(stats)) == (100 + 2 * el, 1000 + 2 * el)


def test_argument_errors_leave_the_outputs_alone(lib):
    V, T, N = 8, 3, 2
    c = kernel_case(V, 8, 0, T, N, seed=1)
    flat, cap, lens, coin, u, stepd = dev(c["flat"]), dev(c["cap"]), dev(c["lens"]), dev(c["coin"]), dev(c["u"]), dev(np.array([1], np.int32))
    out = torch.full((T, N), POISON, dtype=torch.int32, device="cuda")
    stats, rate_out = dev(np.array([POISON, POISON], np.int32)), dev(np.array([-7.0], np.float32))
    good = dict(logits=P(flat), ld=8, V=V, T=T, N=N, cap=P(cap), lens=P(lens), coin=P(coin), u=P(u), temp=1.0, step=P(stepd), schedule=1, rate_max=0.5,
                ramp=10, out=P(out), stats=P(stats), rate_out=P(rate_out))
    bad = [dict(V=0), dict(ld=7), dict(T=0), dict(N=0), dict(temp=0.0), dict(temp=-1.0), dict(rate_max=-0.01), dict(rate_max=1.01), dict(schedule=3),
           dict(schedule=-1), dict(schedule=1, ramp=0), dict(schedule=2, ramp=-3), dict(logits=None), dict(cap=None), dict(lens=None),
           dict(coin=None), dict(step=None)]
    for kw in bad:
        with pytest.raises(abi.VaecapError, match="code 10001"):
            lib.vc_sched_mix_f32(stream(), *dict(good, **kw).values())
    with pytest.raises(abi.VaecapError, match="code 10001"):
        lib.vc_sched_mix_f32(stream(), *dict(good, out=None).values())
    assert (host(out) == POISON).all() and (host(stats) == POISON).all() and host(rate_out)[0] == -7.0
    lib.vc_sched_mix_f32(stream(), *dict(good, temp=0.0, u=None).values())   # argmax takes no temperature
    lib.vc_sched_mix_f32(stream(), *dict(good, schedule=0, ramp=0).values())  # the constant schedule ignores the ramp
    assert (host(out) != POISON).all()


# ------------------------------------------------------------------------------------------------ the step
V_, B_, T_ = 203, 4, 9
SCHED = dict(sched_sampling=0.5, sched_schedule="constant")
STEP_CASES = {"Normal": (dict(prior="Normal"), "f32"), "Normal_dropout": (dict(prior="Normal", dec_keep_rate=0.8, dec_lstm_drop=0.7), "f32"),
              "AG_cv": (dict(prior="AG", use_c_v=True), "f32"), "GMM": (dict(prior="GMM"), "f32"),
              "no_encoder": (dict(prior="Normal", no_encoder=True), "f32"), "Normal_bf16x3": (dict(prior="Normal"), "bf16x3")}


def with_ss(noise, T, N, seed):
    rng = np.random.default_rng(seed)
    return dict(noise, ss_coin=rng.random((T, N), dtype=np.float32), ss_u=rng.random((T, N), dtype=np.float32))


def step_cases(kw, n=3):
    """[(P0, batch, noise incl. ss_coin / ss_u)] x n: each step its own batch and noise"""
    p = small_params(**kw, **SCHED)
    out = []
    for k in range(n):
        P0, batch, noise = make_case(p, V_, B_, T_, seed=7 + k)
        out.append((P0, batch, with_ss(noise, T_, B_ * p.num_captions, 100 + k)))
    return p, out


@pytest.mark.parametrize("name", list(STEP_CASES), ids=str)
def test_step_mixes_pass_one_and_trains_pass_two(lib, name):
    """(a) dec_mix_t of a Trainer step = the reference's mix of the first pass's logits (a second engine's train=False forward on the
    same parameters, batch and noise), under the delta rule; (b) the step is, bit for bit, the plain step of a trainer with the mode off
    that is fed the mixed inputs: losses, gradient norm and every parameter, over three consecutive steps with their own batches"""
    kw, prec = STEP_CASES[name]
    p, cases = step_cases(kw)
    P0 = cases[0][0]
    N = B_ * p.num_captions
    on = Trainer(p, V_, lib=lib, seed=5, precision=prec)
    on.load_state_dict(P0)
    off = Trainer(small_params(**kw), V_, lib=lib, seed=5, precision=prec)
    off.load_state_dict(P0)
    assert off.sched_stats() is None
    for k, (_, batch, noise) in enumerate(cases):
        if k == 0:   # pass 1 of the first step, from an engine of its own
            eng = CaptionEngine(p, V_, lib=lib)
            eng.set_precision(prec)
            eng.load_params(P0)
            eng.set_batch(batch, noise)
            eng.forward(train=False)
            logits1 = host(eng.buf["logits"])[:, :V_].copy()
        on.set_batch(batch, noise)
        on.train_step()
        mix = host(on.cap.buf["dec_mix_t"]).copy()
        st = on.sched_stats()
        cap_t, lens = np.ascontiguousarray(batch["cap_dec"].T), batch["lengths"]
        el = R.eligible(T_, N, lens)
        sel = el & (noise["ss_coin"] < np.float32(0.5))
        assert st == {"rate": 0.5, "eligible": int(el.sum()), "replaced": int(sel.sum())} and sel.sum() >= 10, (st, el.sum(), sel.sum())
        np.testing.assert_array_equal(mix[~sel], cap_t[~sel])
        assert (mix[sel] != cap_t[sel]).any()
        if k == 0:
            ref, cdfs = R.mix(logits1, cap_t, lens, noise["ss_coin"], noise["ss_u"], 1.0, 0.5)
            for t, n in zip(*np.nonzero(sel)):
                assert R.accepts(cdfs[(t, n)], int(mix[t, n]), noise["ss_u"][t, n]), (t, n, mix[t, n], ref[t, n])
        off.set_batch(dict(batch, cap_dec=np.ascontiguousarray(mix.T)), noise)
        off.train_step()
        assert on.losses() == off.losses(), (k, on.losses(), off.losses())
        assert float(on.cap.ns[0].item()) == float(off.cap.ns[0].item()), k
        assert int(on.cap.step.item()) == int(off.cap.step.item()) == k + 1
    a, b = on.state_dict(), off.state_dict()
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert any(not np.array_equal(a[key], P0[key]) for key in P0)


def test_argmax_pick_in_the_step(lib):
    p = small_params(prior="Normal", sched_sampling=1.0, sched_schedule="constant", sched_pick="argmax")
    P0, batch, noise = make_case(p, V_, B_, T_, seed=7)
    N = B_ * p.num_captions
    noise = dict(noise, ss_coin=np.random.default_rng(1).random((T_, N), dtype=np.float32))   # no ss_u: argmax draws nothing
    eng = CaptionEngine(p, V_, lib=lib)
    eng.load_params(P0)
    eng.set_batch(batch, noise)
    eng.forward(train=False)
    logits1 = host(eng.buf["logits"])[:, :V_].copy()
    eng.set_batch(batch, noise)
    eng.forward()
    ref, _ = R.mix(logits1, batch["cap_dec"].T, batch["lengths"], noise["ss_coin"], None, 1.0, 1.0)
    np.testing.assert_array_equal(host(eng.buf["dec_mix_t"]), ref)
    st = eng.sched_stats()
    assert st["replaced"] == st["eligible"] == int(R.eligible(T_, N, batch["lengths"]).sum())


def test_captured_step_equals_eager(lib):
    p = small_params(prior="Normal", sched_sampling=0.5, sched_schedule="linear", sched_ramp_steps=2, dec_keep_rate=0.8)
    V, B, T = 203, 4, 9
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
        rec = []
        for b in batches:
            tr.set_batch(b)
            tr.train_step()
            st = tr.sched_stats()
            rec.append((tr.losses(), st["rate"], st["eligible"], st["replaced"], host(tr.cap.buf["dec_mix_t"]).tolist()))
        res.append((rec, tr.state_dict()))
    assert res[0][0] == res[1][0]
    assert [r[1] for r in res[1][0]] == [0.0, 0.25, 0.5]   # the schedule advances inside the replayed graph
    assert res[1][0][0][3] == 0 and res[1][0][2][3] > 0
    for k in res[0][1]:
        np.testing.assert_array_equal(res[0][1][k], res[1][1][k], err_msg=k)


def _count_collectives(tr):
    calls = collections.Counter()
    for nm in ("reduce_fn", "gather_fn", "rscatter_fn"):
        def counted(*a, _f=getattr(tr.cap, nm), _n=nm):
            calls[_n] += 1
            return _f(*a)
        setattr(tr.cap, nm, counted)
    return calls


def test_forced_single_rank_collectives(lib):
    """mode on: the forced-collective step reports what the plain one reports (that file's tolerance for the same comparison:
    tests/test_gpu_objective.py, 2e-4 relative), and a step issues as many collective calls as it does with the mode off"""
    V, B, T = 203, 4, 9
    counts, res = {}, []
    for mode_on, force in ((True, False), (True, True), (False, True)):
        p = small_params(prior="Normal", **(SCHED if mode_on else {}))
        P0, batch, noise = make_case(p, V, B, T, seed=9)
        noise = with_ss(noise, T, B * p.num_captions, 3)
        tr = Trainer(p, V, lib=lib, force_collectives=force)
        tr.load_state_dict(P0)
        calls = _count_collectives(tr)
        for _ in range(2):
            tr.set_batch(batch, noise)
            tr.train_step()
        if mode_on:
            res.append(tr.losses())
        counts[(mode_on, force)] = dict(calls)
        if tr.comm is not None:
            tr.comm.destroy()
    for a, b in zip(res[0], res[1]):
        assert abs(a - b) <= 2e-4 * abs(a), res
    assert counts[(True, False)] == {} and counts[(True, True)] == counts[(False, True)] and sum(counts[(True, True)].values()) >= 2, counts


class _NoNewEntries(object):
    """the loaded library, except that resolving any entry of this feature is an error"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in NEW_ENTRIES:
            raise AssertionError("%s resolved with scheduled sampling off" % name)
        return getattr(self._lib, name)


def test_defaults_launch_none_of_the_new_entries(lib):
    guard = _NoNewEntries(lib)
    with pytest.raises(AssertionError):
        guard.vc_sched_mix_f32
    V, B, T = 203, 4, 6
    for kw in (dict(prior="Normal"), dict(prior="GMM"), dict(prior="AG", use_c_v=True), dict(prior="Normal", no_encoder=True)):
        p = small_params(**kw)
        P0, batch, noise = make_case(p, V, B, T, seed=7)
        eng = CaptionEngine(p, V, lib=guard)
        eng.load_params(P0)
        for _ in range(3):
            eng.set_batch(batch, noise)
            eng.forward(); eng.backward(); eng.pack_tail(); eng.apply_gradients()
        assert all(np.isfinite(eng.losses())) and eng.sched_stats() is None
        assert not any(k in eng.buf for k in ("lens", "dec_mix_t", "ss_coin", "ss_u", "order_mix"))
    p = small_params(prior="Normal")
    tr = Trainer(p, V, lib=guard, seed=3)
    tr.load_state_dict(spec.init_caption_params(p, V, seed=8))
    tr.set_batch(synth.make_batch(np.random.default_rng(2), B, p.num_captions, T, V, variable_len=True, feature_size=p.cnn_feature_size))
    tr.capture(warmup=1)
    tr.train_step()
    assert all(np.isfinite(tr.losses())) and tr.eval_rec_loss() > 0 and tr.sched_stats() is None


def test_the_mode_resolves_the_new_entry_and_validation_does_not(lib):
    """... and the guard is not vacuous; validation (train=False) never mixes"""
    p = small_params(prior="Normal", **SCHED)
    P0, batch, noise = make_case(p, 203, 4, 6, seed=7)
    eng = CaptionEngine(p, 203, lib=_NoNewEntries(lib))
    eng.load_params(P0)
    eng.set_batch(batch, with_ss(noise, 6, 12, 1))
    eng.forward(train=False)
    assert "dec_mix_t" not in eng.buf
    with pytest.raises(AssertionError, match="vc_sched_mix_f32"):
        eng.forward()


def test_validation_loss_is_the_one_with_the_mode_off(lib):
    V, B, T = 203, 4, 9
    for inject in (True, False):
        rec = []
        for kw in ({}, SCHED):
            p = small_params(prior="Normal", dec_keep_rate=0.8, **kw)
            P0, batch, noise = make_case(p, V, B, T, seed=7)
            tr = Trainer(p, V, lib=lib, seed=11)
            tr.load_state_dict(P0)
            tr.set_batch(batch, with_ss(noise, T, B * p.num_captions, 1) if inject else None)
            rec.append(tr.eval_rec_loss())
            assert "dec_mix_t" not in tr.cap.buf and int(tr.cap.step.item()) == 0
        assert rec[0] == rec[1], (inject, rec)


def test_device_noise(lib):
    """rate 0.5 constant: the replaced share of one step of >= 2000 eligible positions within five binomial standard deviations of
    0.5; the draws are a function of the seed"""
    p = small_params(prior="Normal", **SCHED)
    V, B, T = 203, 80, 16
    P0 = spec.init_caption_params(p, V, seed=4)
    batch = synth.make_batch(np.random.default_rng(5), B, p.num_captions, T, V, variable_len=True, feature_size=p.cnn_feature_size)
    mixes = []
    for seed in (21, 21, 22):
        tr = Trainer(p, V, lib=lib, seed=seed)
        tr.load_state_dict(P0)
        tr.set_batch(batch)
        tr.train_step()
        st = tr.sched_stats()
        n = st["eligible"]
        assert n >= 2000 and n == int(R.eligible(T, B * p.num_captions, batch["lengths"]).sum()) and st["rate"] == 0.5
        assert abs(st["replaced"] / n - 0.5) <= 5 * np.sqrt(0.25 / n), st
        mixes.append(host(tr.cap.buf["dec_mix_t"]).copy())
        assert int((mixes[-1] != batch["cap_dec"].T).sum()) >= 0.4 * n   # and the replaced positions did get other words (V = 203: a few coincide)
    np.testing.assert_array_equal(mixes[0], mixes[1])
    assert (mixes[0] != mixes[2]).any()


def test_vocabulary_beyond_the_device_index_is_refused(lib):
    p = small_params(prior="Normal", **SCHED)
    with pytest.raises(ValueError, match="embedding-gradient index"):
        CaptionEngine(p, int(lib.vc_embedding_index_max_vocab()) + 1, lib=lib)


def test_main_cli(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--vocab", "120", "--bs", "2", "--embed_dim", "32", "--enc_hid", "32",
           "--dec_hid", "32", "--latent", "8", "--gen_z_samples", "3", "--gpu", "0", "--checkpoint", "schedtest", "--ckpt_format", "npz",
           "--epochs", "1", "--max_steps", "3", "--sched_sampling", "0.3", "--sched_schedule", "sigmoid", "--sched_ramp_steps", "2"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("Sched sampling:") and "rate:" in l and "replaced_share:" in l]
    assert lines, r.stdout
    rate = float(lines[-1].split("rate:")[1].split()[0])
    share = float(lines[-1].split("replaced_share:")[1])
    assert rate == pytest.approx(R.sched_rate(2, "sigmoid", 0.3, 2), rel=1e-5) and 0.0 <= share <= 1.0   # the third step: s = 2
    assert "Validation reconstruction loss" in r.stdout
    assert os.path.exists(os.path.join(tmp_path, "checkpoints", "schedtest.ckpt.npz"))
