"""Host reference of the mutual-information estimate (vc_gauss_mix_lse_f64, csrc/latent_mi.hip; vae_captioning_amd/latent_mi.py;
DESIGN.md "Bounds", "Mutual information"): numpy float64 written from the definitions, no call into the library.

    t[n, s, m]      = sum_l [ -0.5 ((z[n,s,l] - mean[m,l]) / std[m,l])^2 - log std[m,l] ] - 0.5 L log(2 pi)
    lse_block[n, s] = log sum_m exp(t[n, s, m])                     (max-subtracted)
    lse_full[n]     = log sum_m exp(sum_s t[n, s, m])               (max-subtracted)
    h[n]            = -0.5 L (1 + log 2 pi) - sum_l log std[n, l]
    mi_block        = mean_{n,s} ( h[n] - (lse_block[n, s] - log N) )
    mi              = mean_n ( S h[n] - (lse_full[n] - log N) )

Every operation is float64 on the float32 inputs converted to float64.  The [N, S, M, L] terms are formed one caption at a time."""
import math

import numpy as np

LOG_2PI = math.log(2.0 * math.pi)


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _lse(a, axis):
    top = a.max(axis=axis, keepdims=True)
    return np.squeeze(top, axis) + np.log(np.exp(a - top).sum(axis=axis))


def terms(z_n, mean, std):
    """t[s, m] of one caption's draws z_n [S, L] under the table (mean, std) [M, L]"""
    z_n, mean, std = _f64(z_n), _f64(mean), _f64(std)
    u = (z_n[:, None, :] - mean[None]) / std[None]                 # [S, M, L]
    return (-0.5 * u * u - np.log(std)[None]).sum(axis=2) - 0.5 * mean.shape[1] * LOG_2PI


def gauss_mix_lse(z, mean, std):
    """-> lse_block [N, S], lse_full [N]"""
    z = np.asarray(z, np.float32)
    N, S, _ = z.shape
    blk, full = np.zeros((N, S)), np.zeros(N)
    for n in range(N):
        t = terms(z[n], mean, std)
        blk[n], full[n] = _lse(t, 1), _lse(t.sum(axis=0), 0)
    return blk, full


def draws(mean, std, eps):
    """z[n, s] = mean[n] + std[n] * eps[n, s] in float32, the multiply and the add each rounded.  (The device may fuse the two: a test
    that compares device numbers takes z from vc_latent_sample_f32 and hands it in as `z`.)"""
    mean, std, eps = (np.asarray(a, np.float32) for a in (mean, std, eps))
    return (mean[:, None, :] + (std[:, None, :] * eps).astype(np.float32)).astype(np.float32)


def block_entropy_term(std):
    s = _f64(std)
    return -0.5 * s.shape[1] * (1.0 + LOG_2PI) - np.log(s).sum(axis=1)


def mutual_information(mean, std, eps=None, z=None):
    """the dict latent_mi.mutual_information returns, from injected eps [N, S, L] (or from the draws z themselves)"""
    z = draws(mean, std, eps) if z is None else np.asarray(z, np.float32)
    N, S, _ = z.shape
    blk, full = gauss_mix_lse(z, mean, std)
    h, log_n = block_entropy_term(std), math.log(N)
    return {"mi": float(np.mean(S * h - (full - log_n))), "mi_block": float(np.mean(h[:, None] - (blk - log_n))), "mi_ceiling": log_n,
            "captions": int(N)}
