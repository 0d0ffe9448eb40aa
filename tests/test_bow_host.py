"""CPU: the bag-of-words auxiliary loss -- the flag, the two variables it adds (and everything it must leave alone), the float64
reference against itself (hand-derived gradient vs torch autograd), the kernel cases' promises, and the checkpoint containers."""
import pickle

import numpy as np
import pytest
import torch

from vae_captioning_amd import spec
from vae_captioning_amd.utils.parameters import Parameters

from . import bow_ref as R

NEW_DEFAULTS = dict(bow_loss=0.0)


# ------------------------------------------------------------------------------------------------ flags
def test_flag_parses_and_defaults_to_off():
    p = Parameters().parse_args([])
    assert p.bow_loss == 0.0 and "bow_loss" in vars(p)
    assert Parameters().parse_args("--bow_loss 0.5".split()).bow_loss == 0.5
    assert Parameters().parse_args("--bow_loss 0 --no_encoder".split()).bow_loss == 0.0   # off goes with everything
    for extra in ("--fine_tune", "--sched_sampling 0.5", "--label_smoothing 0.1 --kl_free_bits 0.05", "--prior GMM", "--prior AG --c_v",
                  "--unlikelihood 1", "--kl_weight 0.1"):
        assert Parameters().parse_args(["--bow_loss", "1"] + extra.split()).bow_loss == 1.0


@pytest.mark.parametrize("argv", ["--bow_loss -0.1", "--bow_loss inf", "--bow_loss nan", "--bow_loss 1 --no_encoder", "--bow_loss 1 --scst",
                                  "--bow_loss 1 --mode inference"], ids=lambda a: a.replace(" ", "_"))
def test_parse_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        Parameters().parse_args(argv.split())
    assert e.value.code == 2
    assert "--bow_loss" in capsys.readouterr().err


def test_defaults_leave_parameters_as_they_were():
    p = Parameters().parse_args([])
    q = Parameters().parse_args("--bow_loss 1".split())
    assert {k: v for k, v in vars(p).items() if k not in NEW_DEFAULTS} == {k: v for k, v in vars(q).items() if k not in NEW_DEFAULTS}
    old = Parameters()
    assert "bow_loss" not in vars(old)
    assert pickle.loads(pickle.dumps(old)).bow_loss == 0.0


# ------------------------------------------------------------------------------------------------ variables
def _params(**kw):
    p = Parameters()
    p.embed_size, p.encoder_hidden, p.decoder_hidden = 16, 32, 32
    p.latent_size, p.gen_z_samples, p.cnn_feature_size = 6, 3, 20
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw", [dict(prior="Normal"), dict(prior="GMM"), dict(prior="AG", use_c_v=True)], ids=["Normal", "GMM", "AG_cv"])
def test_variables_with_and_without_the_flag(kw):
    V = 57
    off, on = _params(**kw), _params(bow_loss=0.5, **kw)
    a, b = spec.caption_variables(off, V), spec.caption_variables(on, V)
    assert a == spec.caption_variables(_params(bow_loss=0.0, **kw), V)                    # off: the identical list
    assert b == a + [("bow/kernel", (off.embed_size, V)), ("bow/bias", (V,))]             # on: the same list plus two names at the end
    Pa, Pb = spec.init_caption_params(off, V, seed=3), spec.init_caption_params(on, V, seed=3)
    assert list(Pb)[:len(Pa)] == list(Pa) and list(Pb)[len(Pa):] == ["bow/kernel", "bow/bias"]
    for k in Pa:
        np.testing.assert_array_equal(Pa[k], Pb[k], err_msg=k)                            # every shared name draws what it drew
    assert Pb["bow/kernel"].shape == (off.embed_size, V) and np.abs(Pb["bow/kernel"]).max() > 0 and not Pb["bow/bias"].any()


def test_no_encoder_never_has_the_head():
    V = 57
    p = _params(no_encoder=True, bow_loss=1.0)
    assert spec.caption_variables(p, V) == spec.caption_variables(_params(no_encoder=True), V)
    assert not spec.uses_bow(p) and spec.uses_bow(_params(bow_loss=1.0)) and not spec.uses_bow(_params())


def test_internal_layout_pads_the_vocabulary_and_keeps_the_head_in_the_dense_prefix():
    from vae_captioning_amd.engine import flat_offsets, internal_caption_variables
    V = 57
    off, on = _params(), _params(bow_loss=1.0)
    a, b = internal_caption_variables(off, V), internal_caption_variables(on, V)
    names = [n for n, _ in b]
    emb0 = min(i for i, n in enumerate(names) if n.endswith("embeddings"))
    assert names.index("bow/kernel") < emb0 and names.index("bow/bias") < emb0               # inside the prefix the global norm runs over
    assert dict(b)["bow/kernel"] == (on.embed_size, 60) and dict(b)["bow/bias"] == (60,)       # padded like decoder/rnn_logits/*
    assert [e for e in b if not e[0].startswith("bow/")] == a
    oa, ob = flat_offsets(a)[0], flat_offsets(b)[0]
    for n, _ in a:
        if not n.endswith("embeddings"):
            assert oa[n] == ob[n], n                                                          # the dense variables in front keep their offsets


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("T", [1, 7, 65])
@pytest.mark.parametrize("V", [203, 204])
def test_hand_derived_gradient_is_autograd(V, T):
    buf, labels = R.bow_case(V, V + 5, 0, T)
    x = buf[:, :V].astype(np.float64)
    c = R.bow_rows(x, labels, gscale=3.0)
    xt = torch.tensor(x, requires_grad=True)
    loss = R.torch_row_loss(xt, labels, gscale=3.0)
    loss.backward()
    g = xt.grad.numpy()
    assert np.abs(c["dlogits"] - g).max() <= 1e-9 * np.abs(g).max()
    den = float((labels != 0).sum())
    assert float(loss.detach()) == pytest.approx(3.0 / den * c["row_loss"].sum(), rel=1e-12)
    assert not c["dlogits"][3].any() and c["row_loss"][3] == 0 and c["row_mass"][3] == 0 and c["row_words"][3] == 0   # the all-PAD caption


def test_the_kernel_grid_holds_every_case_it_promises():
    V = 203
    buf, labels = R.bow_case(V, 204, 0, 7)
    b = R.bags(labels, V)
    assert b[0] == [1, 1, 1, V - 1]                                             # a word three times, plus word V - 1
    assert b[1] == [20, 21, 22, 23] and len({w // 4 for w in b[1]}) == 1        # one float4; PAD, the id >= V and the negative id left out
    assert (labels[:, 1] == 0).any() and (labels[:, 1] >= V).any() and (labels[:, 1] < 0).any()
    assert len(b[2]) == 7 and b[3] == []
    assert (buf[:, V:] == R.GUARD).all()
    c = R.bow_rows(buf[:, :V], labels)
    assert list(c["row_words"]) == [2, 4, len(set(b[2])), 0] and list(c["m"]) == [4, 4, 7, 0]
    # T = 1: every list is cut to its first word; T = 256 repeats words in caption (c)
    assert [len(x) for x in R.bags(R.bow_case(V, 204, 0, 1)[1], V)] == [1, 1, 1, 0]
    c256 = R.bow_rows(*[a[:, :V] if i == 0 else a for i, a in enumerate(R.bow_case(V, 204, 0, 256))])
    assert c256["m"][2] == 256 and c256["row_words"][2] < 256
    s = R.bow_stats(c)
    assert s["bow_words"] == pytest.approx((2 + 4 + len(set(b[2]))) / 3.0) and 0 < s["bow_mass"] < 1 and s["bow"] > 0


def test_multiplicity():
    """a caption that is one word T times: gradient k T (p_v - [v = w]) and one distinct word"""
    V, T, w = 50, 9, 17
    x = np.random.default_rng(0).standard_normal((1, V))
    labels = np.full((T, 1), w, np.int32)
    c = R.bow_rows(x, labels, gscale=2.0)
    p = np.exp(x[0] - x[0].max()); p /= p.sum()
    onehot = np.zeros(V); onehot[w] = 1.0
    np.testing.assert_allclose(c["dlogits"][0], 2.0 / T * T * (p - onehot), rtol=1e-12, atol=1e-15)
    assert c["row_words"][0] == 1 and c["row_mass"][0] == pytest.approx(p[w])


# ------------------------------------------------------------------------------------------------ checkpoints
def test_both_containers_round_trip_the_two_names(tmp_path):
    from vae_captioning_amd import tf_bundle
    p = _params(bow_loss=1.0)
    d = spec.init_caption_params(p, 57, seed=2)
    d["bow/bias"] = np.random.default_rng(1).standard_normal(57).astype(np.float32)
    np.savez(tmp_path / "c.npz", **d)
    with np.load(tmp_path / "c.npz") as z:
        back = {k: z[k] for k in z.files}
    tf_bundle.write_bundle(str(tmp_path / "c.ckpt"), d)
    back2 = tf_bundle.read_bundle(str(tmp_path / "c.ckpt"))
    for got in (back, back2):
        assert set(got) == set(d)
        for k in ("bow/kernel", "bow/bias"):
            np.testing.assert_array_equal(got[k], d[k])
            assert got[k].dtype == np.float32
