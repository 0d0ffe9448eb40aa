"""-m gpu: the contract of csrc/row_ops.h across the entries that run one workgroup per row of logits.  The entries are separate
kernels in separate translation units; what they share is one header, and these tests say what that buys:

* the float32 log-softmax (temperature 1) of a chosen word is the same BITS from vc_decode_pick_f32's logprob increment,
  vc_sbs_expand_f32's cand_lsm and (x - M) - log S formed in float32 from vc_mixture_topk_f32's stat;
* the arg-max token is the same from vc_argmax_rows_f32, vc_decode_pick_f32 (u = NULL) and vc_sched_mix_f32 (u = NULL);
* the drawn token is the same from vc_multinomial_rows_f32, vc_decode_pick_f32 and vc_sched_mix_f32 for the same uniform.

Nothing here has a tolerance.  Shapes: every vocabulary size at which a row kernel changes path -- one word, one short of / exactly /
one past the 256 chunks, the widest row staged in LDS (12 288) and the first one read in place -- and a pitch larger than V behind a
base pointer one float off a 16-byte boundary.  Eight rows: five random (x 2.5), a rounded one (ties), a constant one and one with a
single logit at +80; temperatures 1 and 0.7; uniforms 0, 0.5 and 0.9999999."""
import functools

import numpy as np
import pytest
import torch

from .gpu_util import P, dev, host, stream, zeros

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 0), (255, 255, 0), (256, 256, 0), (257, 257, 0), (12288, 12288, 0), (12289, 12289, 0), (1003, 1008, 1)]   # (V, ld, offset)
IDS = ["v%d-ld%d-off%d" % s for s in SHAPES]
ROWS = 8
TEMPS = (1.0, 0.7)
UNIFORMS = (0.0, 0.5, 0.9999999)
DRAWS = [(t, u) for t in TEMPS for u in UNIFORMS]
EOS = 2
I32 = dict(dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def case(V, ld, off):
    """-> (flat, view): the host allocation (row 0 starts `off` floats in; the pitch padding holds a LARGER value than any logit, so a
    read past column V would show) and its [ROWS, V] view.  Built once, never modified."""
    rng = np.random.default_rng(V * 31 + ld + off)
    flat = np.full(ROWS * ld + 8, 99.0, np.float32)
    rows = flat[off:off + ROWS * ld].reshape(ROWS, ld)
    rows[:, :V] = rng.standard_normal((ROWS, V)).astype(np.float32) * 2.5
    rows[5, :V] = np.round(rows[5, :V])
    rows[6, :V] = 0.5
    rows[7, V // 2] = 80.0
    flat.setflags(write=False)
    return flat, rows[:, :V]


def upload(V, ld, off):
    flat = dev(case(V, ld, off)[0])
    assert flat.data_ptr() % 16 == 0
    return flat.data_ptr() + 4 * off


def argmax_rows(lib, x, V, ld):
    out = torch.full((ROWS,), -7, **I32)
    lib.vc_argmax_rows_f32(stream(), x, ROWS, V, ld, P(out))
    return host(out)


def multinomial_rows(lib, x, V, ld, temp, u):
    out = torch.full((ROWS,), -7, **I32)
    lib.vc_multinomial_rows_f32(stream(), x, ROWS, V, ld, temp, P(dev(np.full(ROWS, u, np.float32))), P(out))
    return host(out)


def decode_pick(lib, x, V, ld, temp=1.0, u=None):
    """-> (tok, the float32 log-softmax increment): logprob starts at 0, so the float64 sum holds the float32 term exactly"""
    tok, done, seq, ln = torch.full((ROWS,), -7, **I32), zeros(ROWS, dtype=torch.int32), zeros(ROWS, dtype=torch.int32), zeros(ROWS, dtype=torch.int32)
    lp = zeros(ROWS, dtype=torch.float64)
    du = dev(np.full(ROWS, u, np.float32)) if u is not None else None
    lib.vc_decode_pick_f32(stream(), x, ROWS, V, ld, temp, P(du), 1, None, EOS, P(tok), P(done), P(seq), 1, P(ln), P(lp))
    lp64 = host(lp)
    lp32 = lp64.astype(np.float32)
    assert np.array_equal(lp32.astype(np.float64), lp64)
    return host(tok), lp32


def sched_mix(lib, x, V, ld, temp=1.0, u=None):
    """T = 2, N = ROWS: position (1, n) reads row n; every position behind <BOS> is selected (coin 0 < rate 1)"""
    T, N = 2, ROWS
    cap, lens, coin = torch.full((T, N), -3, **I32), torch.full((N,), T, **I32), zeros(T, N)
    out, step = torch.full((T, N), -7, **I32), dev(np.array([1], np.int32))
    du = dev(np.full((T, N), u, np.float32)) if u is not None else None
    lib.vc_sched_mix_f32(stream(), x, ld, V, T, N, P(cap), P(lens), P(coin), P(du), temp, P(step), 0, 1.0, 1, P(out), None, None)
    o = host(out)
    assert (o[0] == -3).all()
    return o[1]


def sbs_lsm(lib, x, V, ld, words):
    """cand_lsm of `words` (one per row): kc = 1 and an injected Gumbel that lets the row's word win"""
    g = np.zeros((ROWS, V), np.float64)
    g[np.arange(ROWS), words] = 1e4
    count, done = torch.ones(ROWS, **I32), zeros(ROWS, dtype=torch.int32)
    ck, cl, ci = zeros(ROWS, dtype=torch.float64), torch.full((ROWS,), 3.5, device="cuda"), torch.full((ROWS,), -7, **I32)
    lib.vc_sbs_expand_f32(stream(), x, ROWS, 1, V, ld, P(count), P(done), 1, P(dev(g)), 1, None, 0, 0, None, P(ck), P(cl), P(ci))
    assert np.array_equal(host(ci), words)
    return host(cl)


def mixture_stat(lib, x, V, ld):
    """stat [ROWS, 2] = (M, log S) of every row: ROWS groups of one draw, one word each"""
    logw, tp, ti, stat = zeros(ROWS, dtype=torch.float64), zeros(ROWS), zeros(ROWS, dtype=torch.int32), zeros(ROWS, 2)
    need = lib.vc_mixture_topk_workspace_bytes(ROWS, V, 1)
    ws = zeros(need // 4 + 4)
    lib.vc_mixture_topk_f32(stream(), x, ROWS, 1, V, ld, P(logw), 1, P(tp), P(ti), P(stat), P(ws), need)
    return host(stat)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("V,ld,off", SHAPES, ids=IDS)
def test_log_softmax_of_the_chosen_word_is_the_same_bits_from_pick_sbs_and_mixture(lib, V, ld, off):
    x, view = upload(V, ld, off), case(V, ld, off)[1]
    stat = mixture_stat(lib, x, V, ld)
    for temp, u in [(1.0, None)] + DRAWS:
        tok, lp = decode_pick(lib, x, V, ld, temp, u)
        mix = (view[np.arange(ROWS), tok] - stat[:, 0]) - stat[:, 1]
        assert mix.dtype == np.float32
        sbs = sbs_lsm(lib, x, V, ld, tok)
        assert np.array_equal(bits(lp), bits(sbs)), (temp, u, lp, sbs)
        assert np.array_equal(bits(lp), bits(mix)), (temp, u, lp, mix)


@pytest.mark.parametrize("V,ld,off", SHAPES, ids=IDS)
def test_argmax_token_is_the_same_from_argmax_pick_and_sched(lib, V, ld, off):
    x, view = upload(V, ld, off), case(V, ld, off)[1]
    ref = argmax_rows(lib, x, V, ld)
    assert np.array_equal(ref, view.argmax(1))   # the first maximum
    assert np.array_equal(decode_pick(lib, x, V, ld)[0], ref)
    assert np.array_equal(sched_mix(lib, x, V, ld), ref)


@pytest.mark.parametrize("V,ld,off", SHAPES, ids=IDS)
def test_drawn_token_is_the_same_from_multinomial_pick_and_sched(lib, V, ld, off):
    x = upload(V, ld, off)
    for temp, u in DRAWS:
        ref = multinomial_rows(lib, x, V, ld, temp, u)
        assert ((ref >= 0) & (ref < V)).all()
        assert np.array_equal(decode_pick(lib, x, V, ld, temp, u)[0], ref), (temp, u)
        assert np.array_equal(sched_mix(lib, x, V, ld, temp, u), ref), (temp, u)
