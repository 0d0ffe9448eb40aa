"""Host references of the kernels that close a training step (csrc/optim.hip, the latent and loss-scalar kernels of csrc/loss.hip, the
reductions of csrc/elementwise.hip): numpy float64, shared by tests/test_step_tail_host.py (CPU) and tests/test_gpu_step_tail.py.

Adam / SGD / Momentum / the clip scale and the single-rank latent sample and its gradient are oracle/optim.py and oracle/ops.py; this file
adds what the oracle does not have:

  * the data-parallel shard forms of the latent sample (dp.py, quirk Q1 under sharding).  The GLOBAL sample tensor [S, Ng, L] is read as
    flat rows q = s*Ng + n; a rank owns the rows [q0, q0 + nq) and holds eps / dz for those rows only:
        z[q - q0, :]    = mean_g[q % Ng, :] + std_g[q % Ng, :] * eps[q - q0, :]
        dmean_part[n,:] = sum over the rank's q with q % Ng == n of dz[q - q0, :]           (rows that do not occur: zeros)
        dstd_part[n,:]  = the same sum of dz * eps
  * the device-resident step scalars of vc_step_update;
  * the four loss scalars of vc_loss_finalize_f32.
"""
import numpy as np

from oracle import optim as OO


def sample_mixed(mean_g, std_g, eps_local, q0):
    """mean_g, std_g [Ng, L]; eps_local [nq, L] = the rows [q0, q0 + nq) of the global [S*Ng, L] noise -> z_local [nq, L] (float64)."""
    mean_g, std_g, eps_local = (np.asarray(a, np.float64) for a in (mean_g, std_g, eps_local))
    Ng = mean_g.shape[0]
    n = (int(q0) + np.arange(eps_local.shape[0])) % Ng
    return mean_g[n] + std_g[n] * eps_local


def sums_mixed(dz_local, eps_local, Ng, q0):
    """dz_local, eps_local [nq, L] (the rank's rows) -> (dmean_part, dstd_part), each [Ng, L] float64."""
    dz_local, eps_local = np.asarray(dz_local, np.float64), np.asarray(eps_local, np.float64)
    nq, L = dz_local.shape
    n = (int(q0) + np.arange(nq)) % Ng
    dmean, dstd = np.zeros((Ng, L)), np.zeros((Ng, L))
    np.add.at(dmean, n, dz_local)
    np.add.at(dstd, n, dz_local * eps_local)
    return dmean, dstd


def adam_lr_t(lr, t, beta1=0.8, beta2=0.999):
    """The float32 lr_t that oracle.optim.adam_step(lr=lr, t=t) uses (same expression): what a test hands to the kernel as its device scalar."""
    f = np.float32
    return f(f(lr) * np.sqrt(f(1) - f(beta2) ** f(t)) / (f(1) - f(beta1) ** f(t)))


def step_scalars(gs, lr, cnn_lr, b1, b2, ann_param, ann_on, decay_steps):
    """vc_step_update for the step counter value gs (BEFORE the step) -> float64 [5]:
         [0] lr * sqrt(1 - b2^t) / (1 - b1^t), t = gs + 1     [1] (tanh((gs - 1000*ann_param) / 1000) + 1) / 2, or 1 when ann_on == 0
         [2] lr * 0.5^floor(gs / decay_steps) (decay_steps == 0: lr)     [3], [4] the same two with cnn_lr.
    float64 arithmetic on the float32 VALUES of lr, cnn_lr, b1, b2 and ann_param: the kernel receives them as floats."""
    lr, cnn_lr, b1, b2, ann_param = (float(np.float32(a)) for a in (lr, cnn_lr, b1, b2, ann_param))
    gs = int(gs)
    t = float(gs + 1)
    corr = np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    ann = (np.tanh((gs - 1000.0 * ann_param) / 1000.0) + 1.0) * 0.5 if ann_on else 1.0
    dec = 0.5 ** float(gs // decay_steps if decay_steps > 0 else 0)
    return np.array([lr * corr, ann, lr * dec, cnn_lr * corr, cnn_lr * dec], np.float64)


def loss_scalars(ce_num, ce_den, reg=None, reg_scale=0.0, kl_sum=None, inv_n=0.0, ann=None):
    """vc_loss_finalize_f32 -> float64 [4]: rec = ce_num / ce_den (+ reg * reg_scale), mean KL = kl_sum * inv_n (0 without kl_sum),
    lower bound = rec + ann * KL / 10 (rec without kl_sum), annealing coefficient (1 without ann).  Scalars at their float32 values."""
    v = lambda a: float(np.float32(a))
    rec = v(ce_num) / v(ce_den)
    if reg is not None:
        rec += v(reg) * v(reg_scale)
    a = v(ann) if ann is not None else 1.0
    kld = v(kl_sum) * v(inv_n) if kl_sum is not None else 0.0
    return np.array([rec, kld, rec + a * kld / 10.0 if kl_sum is not None else rec, a], np.float64)


def masked_rows(touched_rows, n, E):
    """row mask [ceil(n / E)] -> elementwise boolean [n] (element i belongs to row i // E), the `touched` form that
    oracle.optim.momentum_step takes for a flat parameter buffer whose last row is partial."""
    return np.asarray(touched_rows, bool)[np.arange(n) // E]


clip_scale = OO.clip_scale
