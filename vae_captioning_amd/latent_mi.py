"""Mutual information I(x; z) between a caption and its latent code under the aggregated posterior q(z) = 1/N sum_n q(z | x_n)
(Hoffman & Johnson 2016, "ELBO surgery"; He et al. 2019, "Lagging inference networks"): the fourth number of the posterior-collapse
quartet beside NLL, KL and active units.  KL is large when every posterior sits at the same place away from the prior, and the
active-units count ignores the posteriors' widths; MI is near 0 whenever the code says nothing about the caption.

With the posterior table (mean, std) [N, L] of N captions and S draws z[n, s] = mean[n] + std[n] * eps[n, s] of every caption (the S
blocks the decoder is given as one S*L-dimensional code), t[n, s, m] = log N(z[n, s]; mean[m], std[m]^2) and
h[n] = -0.5 L (1 + log 2 pi) - sum_l log std[n, l] (the negative entropy of one block):

    mi_block = mean_{n,s} ( h[n] - (log sum_m exp t[n, s, m] - log N) )            one L-dimensional block; its S blocks are S draws
    mi       = mean_n ( S h[n] - (log sum_m exp (sum_s t[n, s, m]) - log N) )      the S*L-dimensional code

Both estimate E_x E_q[log q(z | x)] - E_q(z)[log q(z)]; they lie near 0 for a collapsed posterior and cannot exceed about
mi_ceiling = log N: an estimate at the ceiling says that N captions were too few to tell, not that the code holds log N nats.
Every draw is scored under every posterior (N^2 S L Gaussian terms) by csrc/latent_mi.hip: vc_gauss_mix_lse_f64, in float64.
DESIGN.md, "Bounds", "Mutual information"."""
import math

import numpy as np
import torch

from .abi import ptr as P

MI_MAX_CAPTIONS = 65536   # the z buffer [N, S, L] f32 of one call: about 0.4 GB at S = 10, L = 150
MI_MAX_SAMPLES = 128      # vc_gauss_mix_lse_f64: the rows of one caption a workgroup keeps in registers
MI_PHILOX_STREAM = 12     # offset >> 32 of the draws (1..11: the trainer's and the generator's; bound() draws with 8)


def _lib(lib):
    if lib is None:
        from . import abi
        lib = abi.load()
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _f32(a, name, ndim):
    """a numpy array or tensor -> contiguous float32 device tensor with `ndim` axes"""
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.float32:
            raise ValueError("%s must be float32 (got %s)" % (name, a.dtype))
        t = a.to(_device()).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(_device())
    if t.dim() != ndim:
        raise ValueError("%s must have %d axes (got shape %s)" % (name, ndim, tuple(t.shape)))
    return t


def _launch(lib, z, mean, std):
    """vc_gauss_mix_lse_f64 on device tensors -> one float64 device buffer [N*S + N]: lse_block, then lse_full"""
    N, S, L = (int(d) for d in z.shape)
    out = torch.empty(N * S + N, dtype=torch.float64, device=z.device)
    lib.vc_gauss_mix_lse_f64(_stream(), N, int(mean.shape[0]), S, L, P(z), P(mean), P(std), P(out), P(out) + 8 * N * S)
    return out


def gauss_mix_lse(z, mean, std, lib=None):
    """z [N, S, L] scored under the M Gaussians (mean, std) [M, L] (numpy arrays or device tensors, float32): the float64 host arrays
    lse_block [N, S] = log sum_m N(z[n, s]; mean[m], std[m]^2) and lse_full [N] = log sum_m prod_s N(z[n, s]; mean[m], std[m]^2).
    ValueError: shapes that do not fit, an empty table, S above MI_MAX_SAMPLES, a std that is not finite and > 0, a mean or z that is
    not finite."""
    lib = _lib(lib)
    z, mean, std = _f32(z, "z", 3), _f32(mean, "mean", 2), _f32(std, "std", 2)
    N, S, L = (int(d) for d in z.shape)
    if tuple(mean.shape) != tuple(std.shape) or int(mean.shape[1]) != L:
        raise ValueError("mean and std must both be [M, %d] (got %s and %s)" % (L, tuple(mean.shape), tuple(std.shape)))
    if int(mean.shape[0]) < 1 or L < 1:
        raise ValueError("the posterior table must hold at least one row and one dimension (got %s)" % (tuple(mean.shape),))
    if not 1 <= S <= MI_MAX_SAMPLES:
        raise ValueError("1 <= S <= %d draws per caption (got %d)" % (MI_MAX_SAMPLES, S))
    if not (bool(torch.isfinite(std).all()) and bool((std > 0).all())):
        raise ValueError("std must be finite and > 0")
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(z).all())):
        raise ValueError("mean and z must be finite")
    if N == 0:
        return np.zeros((0, S), np.float64), np.zeros(0, np.float64)
    h = _launch(lib, z, mean, std).cpu().numpy()
    return h[:N * S].reshape(N, S).copy(), h[N * S:].copy()


def block_entropy_term(std):
    """h[n] = -0.5 L (1 + log 2 pi) - sum_l log std[n, l]: E_q[log q(z_s | x_n)] of one block, float64 on the host"""
    s = np.asarray(std, np.float32).astype(np.float64)
    return -0.5 * s.shape[1] * (1.0 + math.log(2.0 * math.pi)) - np.log(s).sum(axis=1)


def mutual_information(mean, std, samples, eps=None, seed=0, lib=None):
    """(mean, std) [N, L]: the posteriors of N captions (float32; what bound(..., return_latents="stats") returns); samples = S draws
    per caption.  -> {"mi", "mi_block", "mi_ceiling" = log N, "captions" = N} (module docstring).
    z is drawn for all N rows by one vc_posterior_latent_f32 call (K = 1, no prior mean, its logw to a scratch buffer): from the
    injected eps [N, S, L], or from Philox draws under `seed` on a stream of their own (MI_PHILOX_STREAM).  The kernel's N * S + N
    float64 values come back in one copy and are averaged on the host.
    ValueError: mean / std shapes that differ or are not [N, L] with L >= 1; N outside 1..MI_MAX_CAPTIONS (the z buffer [N, S, L] f32
    is about 0.4 GB at N = 65 536, S = 10, L = 150); samples outside 1..MI_MAX_SAMPLES; a std that is not finite and > 0; a mean that
    is not finite; an eps of another shape."""
    lib = _lib(lib)
    mh, sh = np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(std, np.float32)
    if mh.ndim != 2 or mh.shape != sh.shape or mh.shape[1] < 1:
        raise ValueError("mean and std must both be [N, L] with L >= 1 (got %s and %s)" % (mh.shape, sh.shape))
    N, L = (int(d) for d in mh.shape)
    if not 1 <= N <= MI_MAX_CAPTIONS:
        raise ValueError("1 <= N <= %d captions (got %d): the draws' buffer [N, S, L] f32 is about 0.4 GB at N = %d, S = 10, L = 150; "
                         "pass a subset" % (MI_MAX_CAPTIONS, N, MI_MAX_CAPTIONS))
    S = int(samples)
    if S != samples or not 1 <= S <= MI_MAX_SAMPLES:
        raise ValueError("samples must be an integer in 1..%d (got %r)" % (MI_MAX_SAMPLES, samples))
    if not (np.isfinite(sh).all() and (sh > 0).all()):
        raise ValueError("std must be finite and > 0")
    if not np.isfinite(mh).all():
        raise ValueError("mean must be finite")
    dev = _device()
    epsd = None
    if eps is not None:
        eh = np.ascontiguousarray(eps, np.float32)
        if eh.shape != (N, S, L):
            raise ValueError("eps must be [N, samples, L] = %s (got %s)" % ((N, S, L), eh.shape))
        epsd = torch.from_numpy(eh).to(dev)
    md, sd = torch.from_numpy(mh).to(dev), torch.from_numpy(sh).to(dev)
    z = torch.empty((N, S, L), dtype=torch.float32, device=dev)
    logw = torch.empty(N, dtype=torch.float64, device=dev)   # log p - log q against a unit prior: not used
    lib.vc_posterior_latent_f32(_stream(), N, 1, S, L, P(md), P(sd), None, None, 1.0, P(epsd), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                MI_PHILOX_STREAM << 32, None, P(z), P(logw))
    out = _launch(lib, z, md, sd).cpu().numpy()
    return summarise(out[:N * S].reshape(N, S), out[N * S:], sh)


def summarise(lse_block, lse_full, std):
    """the two means of the module docstring from the kernel's outputs and the table's std, float64 on the host"""
    N, S = lse_block.shape
    h, log_n = block_entropy_term(std), math.log(N)
    return {"mi": float(np.mean(S * h - (lse_full - log_n))), "mi_block": float(np.mean(h[:, None] - (lse_block - log_n))),
            "mi_ceiling": log_n, "captions": int(N)}
