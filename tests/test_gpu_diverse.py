"""-m gpu: diverse captioning -- K latent draws per image, each decoded (greedy or sampled), identical captions merged and ranked
(generate.py: CaptionGenerator.diverse; csrc/diverse.hip).  Checked against the oracle's per-image decoding of each draw
(oracle/decode.py), against K separate greedy / sample calls of this build, and kernel by kernel against the existing kernels
(argmax, multinomial, Philox normals + latent sample) and the numpy merge / rank rule of tests/test_diverse_host.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import decode as od
from vae_captioning_amd import spec
from vae_captioning_amd.generate import CaptionGenerator
from vae_captioning_amd.utils.parameters import Parameters

from .test_diverse_host import rank_rule
from .test_gpu_generate import count_replays, replayed_kinds, setup, whole_chunks

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIORS = [dict(prior="Normal"), dict(prior="AG", use_c_v=True), dict(prior="GMM")]


def _eps(rng, p, K, B):
    return rng.standard_normal((K, p.gen_z_samples, B, p.latent_size)).astype(np.float32)


def _oracle_candidate(P64, p, feat, cv_row, eps_kb, cm, max_len):
    """tokens (od.greedy) and the fp64 sum of their log-probabilities"""
    state = od.initial_state(P64, p, feat, cv_row, eps_kb, cm, std=p.std)
    tok, out, lp = BOS, [], 0.0
    for _ in range(max_len):
        probs, state = od.step(P64, tok, state)
        tok = int(np.argmax(probs))
        lp += float(np.log(probs[tok]))
        out.append(tok)
        if tok == EOS:
            break
    return out, lp


@pytest.mark.parametrize("kw", PRIORS, ids=lambda k: "-".join("%s=%s" % i for i in k.items()))
def test_candidates_and_ranking_match_the_oracle_per_draw(lib, kw):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 31, **kw)
    B, K, T = feats.shape[0], 5, 12
    eps = _eps(np.random.default_rng(4), p, K, B)
    c = cv if spec.uses_ci(p) else None
    res = gen.diverse(feats, c, eps, BOS, EOS, draws=K, max_len=T)
    cands = gen.last_candidates
    for b in range(B):
        ref = [_oracle_candidate(P64, p, feats[b].astype(np.float64), cv[b].astype(np.float64), eps[k][:, b:b + 1].astype(np.float64), cm, T)
               for k in range(K)]
        for k in range(K):
            toks, lp, ended = cands[b][k]
            assert toks == ref[k][0], (b, k, toks, ref[k][0])
            assert ended == (toks[-1] == EOS)
            np.testing.assert_allclose(lp, ref[k][1], rtol=1e-4, atol=1e-6)
        want = rank_rule([t for t, _ in ref], [lp for _, lp in ref], [t[-1] == EOS for t, _ in ref])
        assert [(t, n) for t, _, n in res[b]] == [(t, n) for t, _, n, _ in want], (b, res[b], want)
        np.testing.assert_allclose([s for _, s, _ in res[b]], [s for _, s, _, _ in want], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("kw", [dict(prior="Normal"), dict(prior="AG", use_c_v=True)], ids=["normal", "ag_cv"])
def test_each_draw_is_what_greedy_and_sample_give_for_it(lib, kw):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 13, **kw)
    B, K, T = feats.shape[0], 4, 10
    rng = np.random.default_rng(8)
    eps = _eps(rng, p, K, B)
    c = cv if spec.uses_ci(p) else None
    gen.diverse(feats, c, eps, BOS, EOS, draws=K, max_len=T)
    got = [[gen.last_candidates[b][k][0] for b in range(B)] for k in range(K)]
    ref = CaptionGenerator(eng)
    assert got == [ref.greedy(feats, c, eps[k], BOS, EOS, max_len=T) for k in range(K)]
    p.temperature = 0.8
    U = rng.random((K, T, B)).astype(np.float32)
    gen.diverse(feats, c, eps, BOS, EOS, draws=K, method="sample", max_len=T, uniforms=U)
    got = [[gen.last_candidates[b][k][0] for b in range(B)] for k in range(K)]
    assert got == [ref.sample(feats, c, eps[k], BOS, EOS, max_len=T, uniforms=U[k]) for k in range(K)]


@pytest.mark.parametrize("V,ld", [(40, 40), (10000, 10000), (1003, 1008), (13000, 13000)], ids=["v40", "v10000", "ld-gt-v", "unstaged"])
def test_pick_tokens_equal_argmax_and_multinomial_bit_for_bit(lib, V, ld):
    from .gpu_util import P, dev, host, stream
    rng = np.random.default_rng(V)
    R = 24
    x = np.full((R, ld), 77.0, np.float32)   # (padding columns hold a LARGER value: never read)
    x[:, :V] = rng.standard_normal((R, V)).astype(np.float32) * 2.5
    x[1, :V] = np.round(x[1, :V])             # ties: the first maximum wins
    x[2, :V] = 0.5                            # constant row
    x[3, :V] = -50.0
    x[3, [V // 3, V // 2, V - 1]] = 9.0       # a three-way tie at the top
    u = rng.random(R).astype(np.float32)
    u[:3] = [0.0, 0.9999999, 0.5]
    dx, du = dev(x), dev(u)
    i32 = dict(dtype=torch.int32, device="cuda")
    for temp, uu in ((1.0, None), (1.0, du), (0.7, du)):
        ref = torch.zeros(R, **i32)
        if uu is None:
            lib.vc_argmax_rows_f32(stream(), P(dx), R, V, ld, P(ref))
        else:
            lib.vc_multinomial_rows_f32(stream(), P(dx), R, V, ld, temp, P(uu), P(ref))
        tok, done, seq, ln = torch.zeros(R, **i32), torch.zeros(R, **i32), torch.zeros(R, **i32), torch.zeros(R, **i32)
        lp = torch.zeros(R, dtype=torch.float64, device="cuda")
        lib.vc_decode_pick_f32(stream(), P(dx), R, V, ld, temp, P(uu) if uu is not None else None, 1, None, EOS, P(tok), P(done), P(seq), 1,
                               P(ln), P(lp))
        t = host(tok)
        assert np.array_equal(t, host(ref)), (temp, uu is None)
        assert np.array_equal(host(seq), t) and (host(ln) == 1).all() and np.array_equal(host(done), (t == EOS).astype(np.int32))
        xd = x[:, :V].astype(np.float64)
        lsm = xd - xd.max(1, keepdims=True)
        lsm -= np.log(np.exp(lsm).sum(1, keepdims=True))
        np.testing.assert_allclose(host(lp), lsm[np.arange(R), t], rtol=0, atol=1e-5)
    assert host(tok)[3] in (V // 3, V // 2, V - 1)


def test_pick_skips_ended_rows_and_rounds_select_uniforms(lib):
    from .gpu_util import P, dev, host, stream
    rng = np.random.default_rng(2)
    R, V, Rounds = 8, 50, 3
    x = (rng.standard_normal((R, V)) * 2).astype(np.float32)
    u = rng.random((Rounds, R)).astype(np.float32)
    dx, du = dev(x), dev(u)
    i32 = dict(dtype=torch.int32, device="cuda")
    done = dev(np.array([0, 1, 0, 1, 0, 0, 0, 0], np.int32))
    tok, seq, ln, rnd = torch.zeros(R, **i32), torch.full((R * 4,), -1, **i32), torch.zeros(R, **i32), torch.zeros(1, **i32)
    ln[5] = 4   # a full row: nothing appended
    lp = torch.zeros(R, dtype=torch.float64, device="cuda")
    pending = torch.zeros(1, device="cuda")
    for r in range(Rounds):
        ref = torch.zeros(R, **i32)
        lib.vc_multinomial_rows_f32(stream(), P(dx), R, V, V, 1.0, P(du[r]), P(ref))
        lib.vc_decode_pick_f32(stream(), P(dx), R, V, V, 1.0, P(du), Rounds, P(rnd), -1, P(tok), P(done), P(seq), 4, P(ln), P(lp))
        lib.vc_decode_round_end_i32(stream(), P(done), R, P(pending), P(rnd))
        assert np.array_equal(host(tok), host(ref))
    assert int(host(rnd)[0]) == Rounds and float(host(pending)[0]) == 6.0
    L = host(ln)
    assert L.tolist() == [3, 0, 3, 0, 3, 4, 3, 3]
    assert (host(seq).reshape(R, 4)[[1, 3], :] == -1).all() and (host(lp)[[1, 3, 5]] == 0).all()


@pytest.mark.parametrize("pm", [False, True], ids=["zero-mean", "image-means"])
def test_generated_latent_equals_philox_normal_plus_sample_bit_for_bit(lib, pm):
    from .gpu_util import P, dev, host, stream
    B, K, S, L = 3, 5, 7, 11
    M, n = B * K, B * K * S * L
    rng = np.random.default_rng(1)
    pmh = rng.standard_normal((B, L)).astype(np.float32)
    step = dev(np.array([3], np.int32))
    seed, off, std = 1234 * 1000003 + 17, 6 << 32, 0.1
    z = torch.zeros(n, device="cuda")
    lib.vc_diverse_latent_f32(stream(), M, K, S, L, P(dev(pmh)) if pm else None, std, None, seed, off, P(step), P(z))
    eps = torch.zeros(n, device="cuda")
    lib.vc_philox_normal_f32(stream(), P(eps), n, seed, off, P(step))
    mean = np.repeat(pmh if pm else np.zeros_like(pmh), K * S, axis=0)   # [rows*S, L]: row (b*K + k)*S + s
    ref = torch.zeros(n, device="cuda")
    lib.vc_latent_sample_f32(stream(), 1, M * S, L, P(dev(mean)), P(dev(np.full_like(mean, std))), P(eps), P(ref))
    assert np.array_equal(host(z).view(np.uint32), host(ref).view(np.uint32))
    z2 = torch.zeros(n, device="cuda")   # injected eps: the same values
    lib.vc_diverse_latent_f32(stream(), M, K, S, L, P(dev(pmh)) if pm else None, std, P(eps), 0, 0, None, P(z2))
    assert np.array_equal(host(z2).view(np.uint32), host(ref).view(np.uint32))


@pytest.mark.parametrize("K", [1, 7, 64, 256])
def test_rank_kernel_matches_the_rule(lib, K):
    from .gpu_util import P, dev, host, stream
    rng = np.random.default_rng(K)
    B, L = 3, 9
    seq = rng.integers(3, 40, size=(B * K, L)).astype(np.int32)
    ln = np.zeros(B * K, np.int32)
    en = np.zeros(B * K, np.int32)
    lp = rng.choice(np.array([-1.0, -2.5, -2.5, -7.0]), size=B * K)
    pool = [[5, 2], [7], [9, 9, 9, 2], list(range(3, 3 + L)), list(range(3, 3 + L - 1)) + [4], [6, 6, 6, 6, 6, 6, 6, 6, 2]]
    # (pool[3] / pool[4]: length Lmax, differing only in the last token)
    for r in range(B * K):
        t = pool[rng.integers(0, len(pool))] if rng.random() < 0.8 else list(rng.integers(3, 40, size=rng.integers(1, L + 1)))
        ln[r] = len(t)
        seq[r, :len(t)] = t
        en[r] = int(t[-1] == EOS)
    nd, rep, cnt = (torch.zeros(n, dtype=torch.int32, device="cuda") for n in (B, B * K, B * K))
    sc = torch.zeros(B * K, dtype=torch.float64, device="cuda")
    lib.vc_diverse_rank(stream(), B * K, B, K, L, P(dev(seq)), P(dev(ln)), P(dev(en)), P(dev(lp)), 0.7, P(nd), P(rep), P(cnt), P(sc))
    nd, rep, cnt, sc = host(nd), host(rep), host(cnt), host(sc)
    for b in range(B):
        rows = range(b * K, (b + 1) * K)
        want = rank_rule([seq[r, :ln[r]].tolist() for r in rows], lp[b * K:(b + 1) * K], en[b * K:(b + 1) * K])
        assert nd[b] == len(want)
        got = [(seq[b * K + rep[b * K + j], :ln[b * K + rep[b * K + j]]].tolist(), cnt[b * K + j], rep[b * K + j]) for j in range(nd[b])]
        assert got == [(t, c, d) for t, _, c, d in want]
        np.testing.assert_allclose(sc[b * K:b * K + nd[b]], [s for _, s, _, _ in want], rtol=1e-12)
        assert (rep[b * K + nd[b]:(b + 1) * K] == -1).all() and (cnt[b * K + nd[b]:(b + 1) * K] == 0).all()


def test_lstm_baseline_greedy_gives_one_caption_from_every_draw(lib):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 5, no_encoder=True)
    K = 6
    res = gen.diverse(feats, None, None, BOS, EOS, draws=K, max_len=12)
    ref = gen.greedy(feats, None, None, BOS, EOS, max_len=12)
    for b in range(feats.shape[0]):
        assert len(res[b]) == 1 and res[b][0][2] == K and res[b][0][0] == ref[b]


@pytest.mark.parametrize("kw", [dict(prior="GMM"), dict(prior="AG", use_c_v=True)], ids=["gmm", "ag_cv"])
def test_replay_equals_eager_and_decodes_the_inputs_of_the_call(lib, kw, monkeypatch):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 23, **kw)
    B, K, T = feats.shape[0], 4, 11
    rng = np.random.default_rng(3)
    eps, eps2 = _eps(rng, p, K, B), _eps(rng, p, K, B)
    feats2 = np.maximum(rng.standard_normal(feats.shape), 0).astype(np.float32)
    cv2 = np.zeros_like(cv)
    for b in range(B):
        cv2[b, rng.choice(90, size=3, replace=False)] = 0.3
    c, c2 = (cv, cv2) if spec.uses_ci(p) else (None, None)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("VC_DECODE_GRAPH", mode)
        g = CaptionGenerator(eng)
        first = g.diverse(feats, c, eps, BOS, EOS, draws=K, max_len=T)
        again = g.diverse(feats, c, eps, BOS, EOS, draws=K, max_len=T)          # (replayed graphs in mode 1)
        second = g.diverse(feats2, c2, eps2, BOS, EOS, draws=K, max_len=T)      # replayed graphs, new inputs
        fresh = CaptionGenerator(eng).diverse(feats2, c2, eps2, BOS, EOS, draws=K, max_len=T)
        assert again == first and second == fresh and second != first
        out[mode] = (first, second)
    assert out["1"] == out["0"]


def test_passes_over_image_groups_equal_one_pass(lib):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 17, prior="Normal")
    K = 5
    eps = _eps(np.random.default_rng(6), p, K, feats.shape[0])
    whole = gen.diverse(feats, None, eps, BOS, EOS, draws=K, max_len=10)
    g = CaptionGenerator(eng)
    g.diverse_rows = 2 * K   # two images per pass: three passes
    assert g.diverse(feats, None, eps, BOS, EOS, draws=K, max_len=10) == whole


def test_full_dimension_draws_equal_per_draw_greedy(lib):
    from vae_captioning_amd.engine import CaptionEngine
    p = Parameters()
    p.mode, p.num_captions, p.prior = "inference", 1, "Normal"
    V, B, K, T = 10000, 32, 20, 16
    rng = np.random.default_rng(0)
    eng = CaptionEngine(p, V, lib=lib)
    eng.load_params(spec.init_caption_params(p, V, seed=3))
    gen = CaptionGenerator(eng)
    feats = np.maximum(rng.standard_normal((B, p.cnn_feature_size)), 0).astype(np.float32)
    eps = _eps(rng, p, K, B)
    res = gen.diverse(feats, None, eps, BOS, EOS, draws=K, max_len=T)
    got = [[gen.last_candidates[b][k][0] for b in range(B)] for k in range(K)]
    ref = CaptionGenerator(eng)
    assert got == [ref.greedy(feats, None, eps[k], BOS, EOS, max_len=T) for k in range(K)]
    assert all(1 <= len(r) <= K and sum(n for _, _, n in r) == K for r in res)


# ------------------------------------------------------------------ facade, driver, command line
class _Dict(object):
    word2idx = {"<BOS>": BOS, "<EOS>": EOS, "<PAD>": 0}
    idx2word = {i: "w%d" % i for i in range(40)}
    idx2word.update({BOS: "<BOS>", EOS: "<EOS>", 0: "<PAD>"})


def _facade_params():
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden = 32, 64, 64
    p.latent_size, p.gen_z_samples, p.cnn_feature_size = 10, 4, 48
    p.mode, p.num_captions, p.vocab_size, p.gen_max_len = "inference", 1, 40, 10
    p.sample_gen, p.diverse_draws = "diverse", 6
    return p


def test_decoder_diverse_inference_record_shape(lib):
    from vae_captioning_amd.vae_model.decoder import Decoder
    p = _facade_params()
    dec = Decoder(None, None, None, p, _Dict)
    feats = np.maximum(np.random.default_rng(0).standard_normal((3, 48)), 0).astype(np.float32)
    recs = dec.diverse_inference(None, ["a", "b", "c"], feats, None)
    assert [r["image_id"] for r in recs] == ["a", "b", "c"]
    for r in recs:
        assert set(r) == {"image_id", "caption", "captions", "scores", "counts"}
        assert r["caption"] == r["captions"][0] and len(r["captions"]) == len(r["scores"]) == len(r["counts"])
        assert sum(r["counts"]) == 6 and all(isinstance(t, str) for t in r["captions"])
    two = dec.diverse_inference(None, ["a", "b", "c"], feats, None, draws=4, method="sample", n_best=2)
    assert all(1 <= len(r["captions"]) <= 2 for r in two)


def test_inference_driver_writes_the_coco_file_and_the_diverse_file(lib, tmp_path, monkeypatch):
    from vae_captioning_amd.ops.inference import inference
    from vae_captioning_amd.vae_model.decoder import Decoder
    p = _facade_params()
    p.gen_name = "dv"
    feats = np.maximum(np.random.default_rng(1).standard_normal((4, 48)), 0).astype(np.float32)

    class Val(object):
        def next_val_batch(self, get_image_ids=True, use_obj_vectors=False):
            yield feats[:2], None, None, [11, 12], np.zeros((2, 91), np.float32)
            yield feats[2:], None, None, [13, 14], np.zeros((2, 91), np.float32)

    monkeypatch.chdir(tmp_path)
    inference(p, Decoder(None, None, None, p, _Dict), Val(), None)
    coco = json.load(open(tmp_path / "val_dv.json"))
    full = json.load(open(tmp_path / "val_dv_diverse.json"))
    assert [r["image_id"] for r in coco] == [11, 12, 13, 14] and all(set(r) == {"image_id", "caption"} for r in coco)
    assert [r["caption"] for r in coco] == [r["captions"][0] for r in full] and all(sum(r["counts"]) == 6 for r in full)


def test_main_synthetic_inference_with_diverse_captions(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    ck = tmp_path / "checkpoints"
    common = ["--synthetic", "--vocab", "200", "--embed_dim", "32", "--enc_hid", "64", "--dec_hid", "64", "--latent", "10",
              "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "dv"]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + common + ["--epochs", "1", "--max_steps", "1"],
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert any(ck.iterdir())
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + common +
                       ["--mode", "inference", "--sample_gen", "diverse", "--diverse_draws", "4", "--gen_name", "dv"],
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = json.load(open(tmp_path / "val_dv.json"))
    assert len(recs) == 8 and all(sum(x["counts"]) == 4 for x in recs)


def _diverse_args(p, feats, method, max_len, K=3):
    rng = np.random.default_rng(41)
    eps = _eps(rng, p, K, feats.shape[0])
    U = rng.random((K, max_len, feats.shape[0])).astype(np.float32) if method == "sample" else None
    return dict(eps=eps, bos=BOS, eos=EOS, draws=K, method=method, max_len=max_len, uniforms=U)


@pytest.mark.parametrize("max_len,check_every", [(10, 4), (10, 2), (3, 4)], ids=["chunks-of-4", "chunks-of-2", "shorter-than-a-chunk"])
@pytest.mark.parametrize("method", ["greedy", "sample"])
@pytest.mark.parametrize("seed", [23, 19], ids=["to-max-len", "early-exit"])   # (seed 19: every greedy candidate ends within three tokens)
def test_second_call_replays_the_init_graph_and_every_whole_chunk(lib, seed, method, max_len, check_every, monkeypatch):
    """As tests/test_gpu_generate.py pins it for greedy(): the second diverse() call of a shape captures nothing and replays
    _diverse_init's graph, then one chunk graph per whole chunk of `check_every` rounds up to the early exit."""
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, seed, prior="GMM")
    kw = _diverse_args(p, feats, method, max_len)
    replayed = count_replays(monkeypatch)
    first = gen.diverse(feats, None, check_every=check_every, **kw)
    graphs = dict(gen._graphs)
    assert sorted(k[0] for k in graphs) == ["diverse", "dvinit"]
    replayed.clear()
    assert gen.diverse(feats, None, check_every=check_every, **kw) == first
    assert gen._graphs == graphs, "an identical second call captures nothing new"
    cands = [c for img in gen.last_candidates for c in img]
    n = whole_chunks([len(t) for t, _, _ in cands], [en for _, _, en in cands], max_len, check_every)
    print("diverse %s max_len %d check_every %d: longest %d, %d chunk replays expected, replayed %s"
          % (method, max_len, check_every, max(len(t) for t, _, _ in cands), n, replayed_kinds(gen, replayed)))
    assert n <= max_len // check_every and (n >= 1 or max_len < check_every)
    assert replayed_kinds(gen, replayed) == ["dvinit"] + ["diverse"] * n


@pytest.mark.parametrize("method", ["greedy", "sample"])
def test_with_graphs_off_nothing_is_captured_or_replayed(lib, method, monkeypatch):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, 23, prior="GMM")
    kw = _diverse_args(p, feats, method, 10)
    on = [(gen.diverse(feats, None, check_every=4, **kw), gen.last_candidates) for _ in range(2)]
    monkeypatch.setenv("VC_DECODE_GRAPH", "0")
    replayed = count_replays(monkeypatch)
    g = CaptionGenerator(eng)
    assert [(g.diverse(feats, None, check_every=4, **kw), g.last_candidates) for _ in range(2)] == on
    assert replayed == [] and len(g._graphs) == 0
