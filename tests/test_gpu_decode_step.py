"""-m gpu: the kernels of the decode path, at the decoder's full size, against fp64 references.

  * single LSTM steps (vc_lstm_pack_wh_f32 + vc_lstm_step_fwd_packed_f32, vc_lstm_step_fwd_f32, vc_lstm_step_bwd_f32) against the
    fp64 cell of oracle/ops.py, at row counts on each side of every launch-shape boundary of csrc/lstm.hip (the test mirrors the
    dispatch arithmetic and asserts that each case lands on the path its id names);
  * the row moves of a beam round (vc_beam_gather_f32, bit-exact) and the vocabulary projection table of beam search
    (CaptionGenerator._project_vocab, against fp64 emb . Wx + b);
  * diverse captioning at the product's largest shapes (3200 and 4800 candidate rows at H = 512, V = 10000).

Tolerances as tests/test_gpu_ops.py: 2e-5 of the tensor max for h / c / gate activations, 5e-5 for gradients, 2e-6 sqrt(K) for
f32 products (6e-5 flat for split-bf16 ones, tests/test_gpu_bf16x3.py), bit-exact for copies."""
import numpy as np
import pytest
import torch

from oracle import decode as od
from oracle import ops as O
from vae_captioning_amd import spec
from vae_captioning_amd.engine import CaptionEngine
from vae_captioning_amd.generate import CaptionGenerator
from vae_captioning_amd.utils.parameters import Parameters

from .gpu_util import P, assert_close, dev, host, stream, zeros

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
SENTINEL = np.float32(-7.25)   # fills the rows past N of every output buffer: they must be left alone
PAD = 3


def cdiv(a, b):
    return -(-a // b)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ----------------------------------------------------------------------------- dispatch arithmetic (csrc/lstm.hip)
def row_groups(N, UG):
    """rec_row_groups: one workgroup per CU over UG column slices, at least 16 rows per group"""
    return min(max(cus() // UG, 1), cdiv(N, 16))


def packed_path(N):
    """vc_lstm_step_fwd_packed_f32 at H = 512 -> (kernel, rows per workgroup, passes): rec8_fwd above 400 rows (80-row passes), else
    rec_fwd with RT = 5 row tiles when a workgroup has more than 48 rows (16 RT-row passes), RT = 3 otherwise"""
    if N > 400:
        rows = cdiv(N, row_groups(N, 32))
        return "rec8", rows, cdiv(rows, 80)
    rows = cdiv(N, row_groups(N, 64))
    rt = 5 if rows > 48 else 3
    return "rec-rt%d" % rt, rows, cdiv(rows, 16 * rt)


def _g4():
    return max(cus() // 64, 1)


def _g8():
    return max(cus() // 32, 1)


# (id, N from the CU count, check of (kernel, rows, passes)); on 256 CUs: 1, 16, 17, 48, 192, 193, 320, 321, 400, 401, 640, 3200,
# 4096, 997
PACKED_CASES = [
    ("rec-rt3-1row", lambda: 1, lambda k, r, p: k == "rec-rt3" and r == 1),
    ("rec-rt3-one-tile", lambda: 16, lambda k, r, p: k == "rec-rt3" and r == 16),
    ("rec-rt3-2groups", lambda: 17, lambda k, r, p: k == "rec-rt3" and r == 9),
    ("rec-rt3-groups-below-CUs", lambda: 16 * max(_g4() - 1, 1), lambda k, r, p: k == "rec-rt3" and r == 16),
    ("rec-rt3-48rows", lambda: 48 * _g4(), lambda k, r, p: k == "rec-rt3" and r == 48 and p == 1),
    ("rec-rt5-49rows", lambda: 48 * _g4() + 1, lambda k, r, p: k == "rec-rt5" and r == 49 and p == 1),
    ("rec-rt5-1pass-full", lambda: 80 * _g4(), lambda k, r, p: k == "rec-rt5" and r == 80 and p == 1),
    ("rec-rt5-2pass", lambda: 80 * _g4() + 1, lambda k, r, p: k == "rec-rt5" and p == 2),
    ("rec-rt5-400rows", lambda: 400, lambda k, r, p: k == "rec-rt5" and p >= 2),
    ("rec8-401rows", lambda: 401, lambda k, r, p: k == "rec8"),
    ("rec8-1pass-full", lambda: 80 * _g8(), lambda k, r, p: k == "rec8" and r == 80 and p == 1),
    ("rec8-5pass", lambda: 3200, lambda k, r, p: k == "rec8" and p >= 2),
    ("rec8-7pass", lambda: 4096, lambda k, r, p: k == "rec8" and p >= 2 and r % 80 != 0),
    ("rec8-prime", lambda: 997, lambda k, r, p: k == "rec8" and p >= 2),
]


def _lens_for(rng, N, t):
    """mixed effective lengths around step t: rows with lens <= t are inactive (their state is carried), row 0 is active"""
    lens = rng.integers(0, 2 * t + 3, size=N).astype(np.int32)
    lens[0] = t + 1
    if N > 1:
        lens[1] = t
    return lens


def _padded(a):
    """device copy of a [N, ...] array with PAD sentinel rows behind it"""
    out = np.full((a.shape[0] + PAD,) + a.shape[1:], SENTINEL, np.float32)
    out[:a.shape[0]] = a
    return dev(out)


def _check_pad(t, N, msg):
    tail = host(t)[N:]
    assert (tail == SENTINEL).all(), "%s: rows past N were written" % msg


def _fwd_case(N, H, t, seed, E=16):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((1, N, E), dtype=np.float32)
    W = rng.standard_normal((E + H, 4 * H), dtype=np.float32) * np.float32(1.0 / np.sqrt(E + H))
    b = rng.standard_normal(4 * H, dtype=np.float32) * np.float32(0.1)
    c0 = rng.standard_normal((N, H), dtype=np.float32)
    h0 = np.tanh(rng.standard_normal((N, H))).astype(np.float32)
    lens = _lens_for(rng, N, t)
    gx = (X[0].astype(np.float64) @ W[:E].astype(np.float64) + b).astype(np.float32)   # the x-projection + bias the step adds
    # the fp64 cell: one step from (c0, h0); the oracle's step 0 is active where the kernel's step t is
    ref = O.lstm_seq_fwd(X.astype(np.float64), (lens > t).astype(np.int32), W.astype(np.float64), b.astype(np.float64),
                         c0=c0.astype(np.float64), h0=h0.astype(np.float64))
    return W[E:], gx, c0, h0, lens, ref


def _fwd_check(N, H, t, c0, h0, lens, gact, c_out, h_out, ref, what):
    assert_close(host(h_out)[:N], ref["hs"][1], 2e-5, msg="%s h_out" % what)
    assert_close(host(c_out)[:N], ref["cs"][1], 2e-5, msg="%s c_out" % what)
    assert_close(host(gact)[:N], ref["act"][0], 2e-5, msg="%s gate activations" % what)
    idle = lens <= t
    assert idle.any() or N == 1
    assert np.array_equal(host(h_out)[:N][idle], h0[idle]) and np.array_equal(host(c_out)[:N][idle], c0[idle]), \
        "%s: inactive rows must carry their state unchanged" % what
    for name, buf in (("gact", gact), ("c_out", c_out), ("h_out", h_out)):
        _check_pad(buf, N, "%s %s" % (what, name))


@pytest.mark.parametrize("t", [0, 3], ids=["t0", "t3"])
@pytest.mark.parametrize("case", PACKED_CASES, ids=[c[0] for c in PACKED_CASES])
def test_packed_step_against_the_fp64_cell(lib, case, t):
    name, n_of, want = case
    N, H = n_of(), 512
    path = packed_path(N)
    assert want(*path), "case %s: N = %d lands on %s on %d CUs" % (name, N, path, cus())
    assert lib.vc_lstm_step_packed_supported(N, H)
    Wh, gx, c0, h0, lens, ref = _fwd_case(N, H, t, seed=N * 4 + t)
    whp = zeros(2 * H * 4 * H)
    lib.vc_lstm_pack_wh_f32(stream(), H, P(dev(Wh)), P(whp))
    gact, c_out, h_out = _padded(gx), _padded(np.zeros((N, H), np.float32)), _padded(np.zeros((N, H), np.float32))
    lib.vc_lstm_step_fwd_packed_f32(stream(), N, H, t, P(dev(h0)), P(dev(c0)), P(whp), P(gact), P(dev(lens)), P(c_out), P(h_out))
    _fwd_check(N, H, t, c0, h0, lens, gact, c_out, h_out, ref, "packed %s N=%d" % (path[0], N))


STEP_HS = [(32, "H32"), (96, "H96-partial"), (512, "H512")]
FWD_NS = [(1, "tile64-1row"), (63, "tile64-63"), (64, "tile64-64"), (65, "tile64-65"), (640, "tile64-640"), (641, "tile128-641"),
          (700, "tile128-700")]


@pytest.mark.parametrize("N", [n for n, _ in FWD_NS], ids=[i for _, i in FWD_NS])
@pytest.mark.parametrize("H", [32, 96, 512], ids=["H32", "H96", "H512"])
def test_step_fwd_against_the_fp64_cell(lib, H, N):
    """vc_lstm_step_fwd_f32: 64-row tiles up to 640 rows, 128-row tiles above; H / 32 column slices of 32 units x 4 gates"""
    t = 2
    Wh, gx, c0, h0, lens, ref = _fwd_case(N, H, t, seed=N * 7 + H)
    gact, c_out, h_out = _padded(gx), _padded(np.zeros((N, H), np.float32)), _padded(np.zeros((N, H), np.float32))
    lib.vc_lstm_step_fwd_f32(stream(), N, H, t, P(dev(h0)), P(dev(c0)), P(dev(Wh)), P(gact), P(dev(lens)), P(c_out), P(h_out))
    _fwd_check(N, H, t, c0, h0, lens, gact, c_out, h_out, ref, "step fwd %s N=%d H=%d" % ("tile128" if N > 640 else "tile64", N, H))


BWD_NS = [(1, "1row"), (64, "64"), (65, "65-ragged"), (700, "700")]


@pytest.mark.parametrize("N", [n for n, _ in BWD_NS], ids=[i for _, i in BWD_NS])
@pytest.mark.parametrize("H", [h for h, _ in STEP_HS], ids=[i for _, i in STEP_HS])
def test_step_bwd_over_a_sequence_against_the_fp64_bptt(lib, H, N):
    """vc_lstm_step_bwd_f32 driven as vc_lstm_seq_bwd_data_f32 mode 0 drives it: t = T-1 with first = 1, then down to 0; 64 x 64
    tiles over (rows, units): cdiv(H, 64) column tiles, half of the last one out of range at H = 32 and 96"""
    T, E = 3, 8
    rng = np.random.default_rng(N * 3 + H)
    X = rng.standard_normal((T, N, E))
    W = (rng.standard_normal((E + H, 4 * H)) / np.sqrt(E + H)).astype(np.float32).astype(np.float64)
    b = rng.normal(0, 0.1, 4 * H)
    lens = rng.integers(0, T + 1, size=N).astype(np.int32)
    lens[0] = T
    if N > 2:
        lens[1], lens[2] = 0, 1
    c0 = rng.standard_normal((N, H)).astype(np.float32).astype(np.float64)
    h0 = np.tanh(rng.standard_normal((N, H))).astype(np.float32).astype(np.float64)
    cache = O.lstm_seq_fwd(X, lens, W, b, c0=c0, h0=h0)
    # the fp32 inputs of the device steps ARE the reference's forward values (rounded once)
    f32 = lambda a: a.astype(np.float32)
    act, cs = f32(cache["act"]), f32(cache["cs"])
    cache["act"], cache["cs"] = act.astype(np.float64), cs.astype(np.float64)
    ext = {2: rng.standard_normal((N, H)) * 0.1, 0: rng.standard_normal((N, H)) * 0.1}   # dh_ext on steps 2 and 0, nullptr on step 1
    ext = {t: f32(v) for t, v in ext.items()}
    dH0 = f32(rng.standard_normal((N, H)) * 0.1)     # gradient w.r.t. the final state hs[T] on entry
    dC0 = f32(rng.standard_normal((N, H)) * 0.1)     # ... and w.r.t. cs[T]
    dhs = np.zeros((T + 1, N, H))
    dhs[T] = dH0.astype(np.float64) + ext[2]
    dhs[1] = ext[0]
    _, _, _, rdc, _ = O.lstm_seq_bwd(cache, dhs, dc_last=dC0.astype(np.float64))
    # recompute dG with the oracle's loop on the same values (lstm_seq_bwd returns only the reductions of it)
    Wh = W[E:]
    dG_ref = np.zeros((T, N, 4 * H))
    dh, dc = dhs[T].copy(), dC0.astype(np.float64).copy()
    for t in range(T - 1, -1, -1):
        i, j, f, o = (cache["act"][t][:, k * H:(k + 1) * H] for k in range(4))
        m = (t < lens)[:, None]
        tc = np.tanh(cache["cs"][t + 1])
        dct = dc + dh * o * (1 - tc * tc)
        g = np.concatenate([dct * j * i * (1 - i), dct * i * (1 - j * j), dct * cache["cs"][t] * f * (1 - f), dh * tc * o * (1 - o)], 1)
        dG_ref[t] = np.where(m, g, 0)
        dc = np.where(m, dct * f, dc)
        if t > 0:
            dh = np.where(m, dG_ref[t] @ Wh.T, dh) + dhs[t]   # -> gradient w.r.t. hs[t]: what dH_run holds after the last step
    assert_close(dc, rdc, 1e-12, msg="restated loop == oracle (dc0)")

    dWh, dl, tact, tcs = dev(f32(Wh)), dev(lens), dev(act), dev(cs)
    dH, dC = _padded(dH0), _padded(dC0)
    dG = dev(np.full((T, N + PAD, 4 * H), SENTINEL, np.float32))
    text = {t: dev(v) for t, v in ext.items()}
    NG = (N + PAD) * 4 * H * 4
    for t in range(T - 1, -1, -1):
        first = int(t == T - 1)
        lib.vc_lstm_step_bwd_f32(stream(), N, H, t, first, None if first else P(dG) + (t + 1) * NG, P(dWh), P(dl),
                                 P(text[t]) if t in text else None, P(dH), P(dC), P(tact[t]), P(tcs[t]), P(tcs[t + 1]), P(dG) + t * NG)
    got = host(dG)
    assert (got[:, N:] == SENTINEL).all(), "rows past N of dG were written"
    assert_close(got[:, :N], dG_ref, 5e-5, msg="dG H=%d N=%d" % (H, N))
    assert_close(host(dH)[:N], dh, 5e-5, msg="final dH_run (d hs[1])")
    assert_close(host(dC)[:N], rdc, 5e-5, msg="final dC_run (d cs[0])")
    _check_pad(dH, N, "dH_run")
    _check_pad(dC, N, "dC_run")


# ----------------------------------------------------------------------------- beam round row moves
@pytest.mark.parametrize("xp", [False, True], ids=["state-only", "with-xproj"])
@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("rows", [37, 1001])
def test_beam_gather_is_an_exact_row_copy(lib, rows, H, xp):
    G, V = 4 * H, 997
    rng = np.random.default_rng(rows + H + xp)
    c = rng.standard_normal((rows, H), dtype=np.float32)
    h = rng.standard_normal((rows, H), dtype=np.float32)
    parent = rng.permutation(rows).astype(np.int32)
    parent[rows // 2:] = parent[:rows - rows // 2]          # repeated parents (a beam that keeps several children)
    parent[-1] = parent[0]
    tok = rng.integers(0, V, size=rows).astype(np.int32)
    tok[0], tok[-1], tok[rows // 3] = 0, V - 1, V - 1
    table = rng.standard_normal((V, G), dtype=np.float32)
    cg, hg = _padded(np.zeros((rows, H), np.float32)), _padded(np.zeros((rows, H), np.float32))
    gact = _padded(np.zeros((rows, G), np.float32))
    lib.vc_beam_gather_f32(stream(), P(dev(c)), P(dev(h)), P(dev(parent)), rows, H, P(cg), P(hg),
                           P(dev(table)) if xp else None, P(dev(tok)) if xp else None, V if xp else 0, G if xp else 0, P(gact))
    assert np.array_equal(host(cg)[:rows], c[parent])
    assert np.array_equal(host(hg)[:rows], h[parent])
    if xp:
        assert np.array_equal(host(gact)[:rows], table[tok])
        _check_pad(gact, rows, "gact")
    else:
        assert (host(gact)[:rows] == 0).all(), "no xproj: gact must be left alone"
    _check_pad(cg, rows, "cg")
    _check_pad(hg, rows, "hg")


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("E", [256, 512])
def test_vocabulary_projection_table_against_fp64(lib, E, precision):
    """CaptionGenerator._project_vocab: xproj [V, 4H] = dec_embeddings . Wx + b, the table beam search looks its rows up in"""
    p = Parameters()
    p.mode, p.num_captions, p.prior, p.embed_size, p.decoder_hidden = "inference", 1, "Normal", E, 512
    V, H = 10000, 512
    eng = CaptionEngine(p, V, lib=lib)
    eng.set_precision(precision)
    P0 = spec.init_caption_params(p, V, seed=E)
    eng.load_params(P0)
    got = host(CaptionGenerator(eng)._project_vocab())
    W = P0[spec.DEC_CELL + "kernel"].astype(np.float64)
    ref = P0["decoder/net/dec_embeddings"].astype(np.float64) @ W[:E] + P0[spec.DEC_CELL + "bias"].astype(np.float64)
    tol = 2e-6 * np.sqrt(E) + 1e-6 if precision == "f32" else 6e-5
    assert_close(got, ref, tol, msg="xproj E=%d %s" % (E, precision))


# ----------------------------------------------------------------------------- diverse captioning at full size
def _full_engine(lib, seed):
    p = Parameters()
    p.mode, p.num_captions, p.prior, p.gen_z_samples = "inference", 1, "Normal", 10
    V = 10000
    rng = np.random.default_rng(seed)
    P0 = spec.init_caption_params(p, V, seed=3)
    for k in P0:  # larger weights -> peaked distributions (test_gpu_fullsize.py cfg5)
        P0[k] = (P0[k] * 3).astype(np.float32) if not k.endswith("bias") else rng.normal(0, 0.5, P0[k].shape).astype(np.float32)
    eng = CaptionEngine(p, V, lib=lib)
    eng.load_params(P0)
    return p, eng, {k: v.astype(np.float64) for k, v in P0.items()}, rng


def _oracle_logprobs(P64, p, feats, eps, rows, toks):
    """fp64 log-likelihood of the given token sequences, all rows batched: initial state per (image, draw), then the tokens
    teacher-forced through the cell (<BOS> first), the log-softmax of each emitted token summed"""
    st = [od.initial_state(P64, p, feats[b].astype(np.float64), None, eps[k][:, b:b + 1].astype(np.float64), std=p.std) for b, k in rows]
    c = np.concatenate([s[0] for s in st])
    h = np.concatenate([s[1] for s in st])
    n = len(rows)
    lens = np.array([len(t) for t in toks])
    L = lens.max()
    fed = np.full((n, L), BOS)
    for r, t in enumerate(toks):
        fed[r, 1:len(t)] = t[:-1]
    W, bias = P64[spec.DEC_CELL + "kernel"], P64[spec.DEC_CELL + "bias"]
    lp = np.zeros(n)
    for s in range(L):
        x = P64["decoder/net/dec_embeddings"][fed[:, s]][None]
        r = O.lstm_seq_fwd(x, (s < lens).astype(np.int32), W, bias, c, h)
        c, h = r["cs"][-1], r["hs"][-1]
        lg = h @ P64["decoder/rnn_logits/kernel"] + P64["decoder/rnn_logits/bias"]
        lg = lg - lg.max(1, keepdims=True)
        lsm = lg - np.log(np.exp(lg).sum(1, keepdims=True))
        act = s < lens
        lp[act] += lsm[np.nonzero(act)[0], [toks[r][s] for r in np.nonzero(act)[0]]]
    return lp


def test_diverse_3200_rows_at_full_size(lib):
    """B = 32 images x K = 100 draws = 3200 candidate rows in one pass: the decoder steps on the eight-wave kernel, several 80-row
    passes per workgroup"""
    p, eng, P64, rng = _full_engine(lib, 21)
    B, K, T = 32, 100, 16
    assert packed_path(B * K)[0] == "rec8" and packed_path(B * K)[2] >= 2
    feats = np.maximum(rng.standard_normal((B, p.cnn_feature_size)), 0).astype(np.float32)
    eps = rng.standard_normal((K, p.gen_z_samples, B, p.latent_size)).astype(np.float32)
    gen = CaptionGenerator(eng)
    res = gen.diverse(feats, None, eps, BOS, EOS, draws=K, max_len=T)
    cands = gen.last_candidates
    assert len(res) == B and all(1 <= len(r) <= K and sum(n for _, _, n in r) == K for r in res)
    ref = CaptionGenerator(eng)
    for k in np.linspace(0, K - 1, 10).astype(int):   # ten draws over k: this build's greedy on B = 32 rows (the four-wave kernel)
        assert [cands[b][k][0] for b in range(B)] == ref.greedy(feats, None, eps[k], BOS, EOS, max_len=T), k
    pick = np.random.default_rng(1).choice(B * K, size=64, replace=False)
    rows = [(int(r) // K, int(r) % K) for r in pick]
    toks = [cands[b][k][0] for b, k in rows]
    lp = _oracle_logprobs(P64, p, feats, eps, rows, toks)
    for (b, k), want in zip(rows, lp):
        np.testing.assert_allclose(cands[b][k][1], want, rtol=1e-4, atol=1e-6, err_msg="image %d draw %d" % (b, k))


def test_diverse_two_passes_at_full_size_equal_one_pass(lib):
    """B = 48 x K = 100 = 4800 rows: two passes at the default diverse_rows (4096: 4000 + 800 rows), one when it is raised.  Every
    candidate's tokens are identical.  The log-likelihoods are fp32 log-softmax terms of logits whose last bits depend on how many
    rows the pass decodes (measured: up to 4.3e-6 on sums of about -14, second-pass images only), so the scores and the ranking
    are held to 1e-6 relative instead of bit equality: the same distinct captions with the same counts per image."""
    p, eng, P64, rng = _full_engine(lib, 22)
    B, K, T = 48, 100, 12
    feats = np.maximum(rng.standard_normal((B, p.cnn_feature_size)), 0).astype(np.float32)
    eps = rng.standard_normal((K, p.gen_z_samples, B, p.latent_size)).astype(np.float32)
    two = CaptionGenerator(eng)
    assert cdiv(B, two.diverse_rows // K) == 2
    got = two.diverse(feats, None, eps, BOS, EOS, draws=K, max_len=T)
    got_c = two.last_candidates
    one = CaptionGenerator(eng)
    one.diverse_rows = B * K
    want = one.diverse(feats, None, eps, BOS, EOS, draws=K, max_len=T)
    want_c = one.last_candidates
    for b in range(B):
        assert [(t, e) for t, _, e in got_c[b]] == [(t, e) for t, _, e in want_c[b]], b
        np.testing.assert_allclose([lp for _, lp, _ in got_c[b]], [lp for _, lp, _ in want_c[b]], rtol=1e-6, err_msg=str(b))
        g = {tuple(t): (s, n) for t, s, n in got[b]}
        w = {tuple(t): (s, n) for t, s, n in want[b]}
        assert g.keys() == w.keys() and all(g[t][1] == w[t][1] for t in g), b
        np.testing.assert_allclose([g[t][0] for t in g], [w[t][0] for t in g], rtol=1e-6, err_msg=str(b))
        ranked = [w[tuple(t)][0] for t, _, _ in got[b] if t[-1] == EOS]   # ended captions first, each group by descending score
        assert all(x >= y - 1e-6 * abs(y) for x, y in zip(ranked, ranked[1:])), b
