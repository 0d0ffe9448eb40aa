"""The fp64 checker of the posterior bounds (generate.py: CaptionGenerator.encode / bound; definitions in DESIGN.md "Bounds"): a numpy
restatement on the oracle (oracle/caption_model.py for q(z | caption, image), oracle/decode.py for the decoder).  TEST INFRASTRUCTURE --
the product never imports it.

Per draw k of a caption: logw_k = log p(z_k | image) - log q(z_k | caption, image), rec_k = log p(caption | z_k, image), a_k = rec_k +
logw_k; per caption: elbo = mean a, iwae = log mean exp a, rec = mean rec_k, kl_mc = -mean logw, kl in closed form, ess = (sum v)^2 /
sum v^2 with v = exp(a - max a)."""
from types import SimpleNamespace

import numpy as np

from oracle import caption_model as cm
from oracle import decode as od


def posterior(P64, p, feat, cv_row, tokens, bos, gmm_k=None, c_means=None):
    """(mean, std) [L] float64 of q(z | caption, image) for ONE caption (tokens without <BOS>): the encoder of the oracle's training graph
    on a batch of one row, cap_enc = tokens, no dropout"""
    t = [int(w) for w in tokens]
    n, S, L = len(t), p.gen_z_samples, p.latent_size
    cfg = SimpleNamespace(prior=p.prior, no_encoder=False, use_c_v=p.use_c_v, num_captions=1, mode="inference", embed_size=p.embed_size,
                          latent_size=L, gen_z_samples=S, dec_keep_rate=1.0, dec_lstm_drop=1.0, ann_param=0.0, fine_tune=False, restore=False)
    batch = {"features": np.asarray(feat, np.float64)[None], "cap_dec": np.array([[bos] + t[:-1]], np.int32),
             "cap_enc": np.array([t], np.int32), "lengths": np.array([n], np.int32)}
    if cm.uses_ci(cfg):
        batch["c_v"] = np.asarray(cv_row, np.float64)[None]
    noise = {"eps": np.zeros((S, 1, L)), "gmm_idx": None if gmm_k is None else np.array([int(gmm_k)]), "c_means": c_means}
    enc = cm.forward_backward(P64, batch, noise, cfg, want_grads=False).aux.enc
    return enc.mean[0], enc.std[0]


def decoder_state(P64, p, feat, cv_row, z):
    """(c, h) after the init chain image -> (c_v) -> z with a GIVEN z [S, L]: od.initial_state with z injected (a zero prior mean and
    std 1 make its z = mean + std * eps the eps it is handed, exactly)"""
    cfg = SimpleNamespace(prior="Normal", use_c_v=p.use_c_v, no_encoder=False, latent_size=p.latent_size)
    z = np.asarray(z, np.float64)
    return od.initial_state(P64, cfg, np.asarray(feat, np.float64), None if cv_row is None else np.asarray(cv_row, np.float64),
                            z[:, None, :], None, std=1.0)


def rec(P64, state, tokens, bos):
    """log p(caption | state): teacher-forced from <BOS>, as tests/score_ref.py: caption_logprob sums it"""
    tok, lp = bos, 0.0
    for w in tokens:
        probs, state = od.step(P64, tok, state)
        lp += float(np.log(probs[w]))
        tok = w
    return lp


def logw_terms(z, eps, std, pm, sigma_p):
    """the [S, L] float64 terms of logw = log p(z | I) - log q(z | x, I), the 2 pi terms cancelled: z, eps [S, L]; std, pm [L] (pm None: 0)"""
    z, eps, std = np.asarray(z, np.float64), np.asarray(eps, np.float64), np.asarray(std, np.float64)
    pm = np.zeros_like(std) if pm is None else np.asarray(pm, np.float64)
    sp = float(np.float32(sigma_p))   # (the prior's std is a float32 like every other operand)
    return -0.5 * ((z - pm) / sp) ** 2 - np.log(sp) + 0.5 * eps ** 2 + np.log(std)[None]


def logw(z, eps, std, pm, sigma_p):
    return float(logw_terms(z, eps, std, pm, sigma_p).sum())


def kl(mean, std, pm, sigma_p, S):
    """KL(q || p) of the S independent [L] blocks in closed form"""
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    pm = np.zeros_like(std) if pm is None else np.asarray(pm, np.float64)
    sp = float(np.float32(sigma_p))
    return float(S * (np.log(sp / std) + (std ** 2 + (mean - pm) ** 2) / (2 * sp * sp) - 0.5).sum())


def reduce(logprob, logw_):
    """the per-caption numbers from the K per-draw terms"""
    r, w = np.asarray(logprob, np.float64), np.asarray(logw_, np.float64)
    a = r + w
    m = a.max()
    v = np.exp(a - m)
    return {"elbo": float(a.mean()), "iwae": float(np.log(v.sum()) + m - np.log(a.size)), "rec": float(r.mean()), "kl_mc": float(-w.mean()),
            "ess": float(v.sum() ** 2 / (v * v).sum())}


def bound(P64, p, feat, cv_row, tokens, bos, eps, pm, gmm_k=None, c_means=None, mean=None, std=None, z=None):
    """One caption's record from eps [K, S, L]: the posterior from the oracle unless (mean, std) are given, z = mean + std * eps unless
    given ([K, S, L]).  pm: the generation-time prior mean [L] or None."""
    if mean is None:
        mean, std = posterior(P64, p, feat, cv_row, tokens, bos, gmm_k, c_means)
    eps = np.asarray(eps, np.float64)
    if z is None:
        z = np.asarray(mean, np.float64)[None, None] + np.asarray(std, np.float64)[None, None] * eps
    lp = np.array([rec(P64, decoder_state(P64, p, feat, cv_row, z[k]), tokens, bos) for k in range(len(eps))])
    lw = np.array([logw(z[k], eps[k], std, pm, p.std) for k in range(len(eps))])
    out = reduce(lp, lw)
    out.update(logprob=lp, logw=lw, kl=kl(mean, std, pm, p.std, p.gen_z_samples), tokens=len(tokens))
    return out
