"""Float64 reference of the training objective options (free bits, KL weight, cyclical annealing, label smoothing, word dropout),
restated from their definitions (DESIGN.md "Training objective options") and sharing no code with the product:

  * numpy: per-dimension KL of both modes, the floor, both KL gradients, the latent backward pass, the smoothed cross-entropy and its
    gradient, the cyclical schedule, word dropout;
  * torch: the training graph of tests/torch_ref.py with the options in it, so that autograd differentiates what the numpy
    formulas differentiate by hand (tests/test_objective_host.py) and what the engine computes (tests/test_gpu_objective.py).
"""
import numpy as np

AG_SIGMA = 0.1


# ------------------------------------------------------------------------------------------------ KL, free bits
def kl_elements(mode, mean, std, mu_p=None):
    """kl[n,l]: mode 0 (Normal, GMM) -0.5 (1 + log(std^2 + 1e-5) - mean^2 - std^2); mode 1 (AG) the summand of the AG prior's KL."""
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    if mode == 0:
        return -0.5 * (1.0 + np.log(std ** 2 + 1e-5) - mean ** 2 - std ** 2)
    d = mean - np.asarray(mu_p, np.float64)
    return -0.5 * (0.5 + np.log(std + 1e-5) - np.log(AG_SIGMA + 1e-5) - (d ** 2 + std ** 2) / (2 * AG_SIGMA ** 2 + 1e-7))


def kl_element_grads(mode, mean, std, mu_p=None):
    """(d kl[n,l] / d mean[n,l], d kl[n,l] / d std[n,l])"""
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    if mode == 0:
        return mean, -(std / (std ** 2 + 1e-5) - std)
    den = 2 * AG_SIGMA ** 2 + 1e-7
    return (mean - np.asarray(mu_p, np.float64)) / den, -0.5 * (1.0 / (std + 1e-5) - 2.0 * std / den)


def free_bits_fwd(mode, mean, std, mu_p, lam):
    """-> (row_kl [N] = sum_l max(lam, kl), row_kl_raw [N] = sum_l kl, row_floored [N] int = #{l: kl <= lam}, kl [N, L])"""
    kl = kl_elements(mode, mean, std, mu_p)
    floored = kl <= lam
    return np.where(floored, lam, kl).sum(1), kl.sum(1), floored.sum(1).astype(np.int64), kl


def latent_bwd(mode, out_logstd, dz, eps, mean, std, mu_p, w, lam=None, dmean0=None, dstd0=None):
    """dmean = sum_s dz (+ dmean0) + w * keep * dkl/dmean, dstd likewise (times std when out_logstd); keep = kl > lam (all ones
    when lam is None: the plain objective).  dz / eps [S, N, L] (S may be 0)."""
    std = np.asarray(std, np.float64)
    dm = np.zeros_like(std) if dmean0 is None else np.asarray(dmean0, np.float64).copy()
    ds = np.zeros_like(std) if dstd0 is None else np.asarray(dstd0, np.float64).copy()
    if len(dz):
        dm = dm + np.asarray(dz, np.float64).sum(0)
        ds = ds + (np.asarray(dz, np.float64) * np.asarray(eps, np.float64)).sum(0)
    gm, gs = kl_element_grads(mode, mean, std, mu_p)
    keep = 1.0 if lam is None else (kl_elements(mode, mean, std, mu_p) > lam).astype(np.float64)
    dm, ds = dm + w * keep * gm, ds + w * keep * gs
    return dm, (ds * std if out_logstd else ds)


def tie_margin(kl, lam):
    """smallest |kl - lam| relative to max(1, lam): fp32 and fp64 may disagree about elements closer to the floor than rounding"""
    return float(np.abs(np.asarray(kl) - lam).min() / max(1.0, lam))


# ------------------------------------------------------------------------------------------------ label smoothing
def smooth_xent(logits, labels, eps, gscale=1.0, den=None):
    """logits [R, V] (real columns only), labels [R].  -> (row_loss [R], dlogits [R, V]) with
    row_loss = mask (lse - (1 - eps) x[label] - eps / V sum_v x[v]),  dlogits = mask gscale / den (softmax - (1 - eps) onehot - eps / V);
    mask = label != 0, den defaults to the number of non-PAD labels."""
    x = np.asarray(logits, np.float64)
    R, V = x.shape
    labels = np.asarray(labels)
    mask = (labels != 0).astype(np.float64)
    den = float(mask.sum()) if den is None else float(den)
    mx = x.max(1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(1)) + mx[:, 0]
    onehot = np.zeros_like(x)
    onehot[np.arange(R), labels] = 1.0
    loss = mask * (lse - (1.0 - eps) * x[np.arange(R), labels] - eps / V * x.sum(1))
    p = np.exp(x - lse[:, None])
    return loss, (mask * gscale / den)[:, None] * (p - (1.0 - eps) * onehot - eps / V)


# ------------------------------------------------------------------------------------------------ schedule, word dropout
def cyclical_ann(step, P, R=0.5, M=0):
    if P <= 0:
        return 1.0
    if M > 0 and step >= M * P:
        return 1.0
    return min(1.0, (step % P) / (R * P))


def word_dropout(cap_dec, lengths, rate, unk_id, rng):
    """position by position: one uniform per element of cap_dec, drawn as one [N, T] array"""
    cap_dec = np.asarray(cap_dec)
    N, T = cap_dec.shape
    u = rng.random((N, T)) if rate > 0 else None
    out = cap_dec.copy()
    for n in range(N):
        for t in range(1, min(int(lengths[n]), T)):
            if rate > 0 and u[n, t] < rate:
                out[n, t] = unk_id
    return out


# ------------------------------------------------------------------------------------------------ the graph with options, in torch
def torch_forward(P, batch, noise, cfg, ann, lam=0.0, beta=1.0, eps_ls=0.0):
    """tests/torch_ref.py's forward with the objective options.  -> dict(kld (reported: unweighted, floored mean KL; a vector for AG),
    rec, lb (what is differentiated, summed), kl [N, L] elements, emb_rows {table name: gathered rows with retained gradient})."""
    import torch
    from .torch_ref import DEC, ENC, cell, dynamic_rnn
    feats = batch["features"]
    nc = cfg.num_captions
    B = feats.shape[0]
    feats = feats.unsqueeze(1).repeat(1, nc, 1).reshape(B * nc, -1)
    N = feats.shape[0]
    images_fv = feats @ P["imf_emb/kernel"] + P["imf_emb/bias"]
    use_ci = cfg.use_c_v or cfg.prior in ("GMM", "AG")
    ci = batch["c_v"] if use_ci else None
    ci_emb = ci @ P["cv_emb/kernel"] + P["cv_emb/bias"] if use_ci else None
    lengths = batch["lengths"]
    rows = {}
    He = P[ENC + "kernel"].shape[1] // 4
    x = P["encoder/enc_embeddings"][batch["cap_enc"].long()]
    x.retain_grad()
    rows["encoder/enc_embeddings"] = x
    z0 = torch.zeros(N, He, dtype=feats.dtype)
    c, h = cell(images_fv, z0, z0, P[ENC + "kernel"], P[ENC + "bias"])
    if cfg.use_c_v:
        c, h = cell(ci_emb, c, h, P[ENC + "kernel"], P[ENC + "bias"])
    _, (c, h) = dynamic_rnn(x, lengths, c, h, P[ENC + "kernel"], P[ENC + "bias"])
    if cfg.prior == "Normal":
        mean = h @ P["encoder/dense/kernel"] + P["encoder/dense/bias"]
        std = torch.exp(h @ P["encoder/dense_1/kernel"] + P["encoder/dense_1/bias"])
    else:
        sc = "encoder/gmm_ll_%d/" if cfg.prior == "GMM" else "encoder/ag_ll_%d/"
        tm = torch.stack([h @ P[sc % k + "dense/kernel"] + P[sc % k + "dense/bias"] for k in range(90)], 1)
        tl = torch.stack([h @ P[sc % k + "dense_1/kernel"] + P[sc % k + "dense_1/bias"] for k in range(90)], 1)
        if cfg.prior == "GMM":
            idx = noise["gmm_idx"].long()
            mean = tm[torch.arange(N), idx]
            std = torch.exp(tl)[torch.arange(N), idx]
        else:
            mean = torch.bmm(ci.unsqueeze(1), tm).squeeze(1)
            std = torch.bmm(ci.unsqueeze(1), torch.exp(tl)).squeeze(1)
    z = mean.unsqueeze(0) + std.unsqueeze(0) * noise["eps"]
    if cfg.prior in ("Normal", "GMM"):
        kl = -0.5 * (1 + torch.log(std ** 2 + 0.00001) - mean ** 2 - std ** 2)
    else:
        kl = -0.5 * (0.5 + torch.log(std + 0.00001) - np.log(AG_SIGMA + 0.00001) - (
            (mean - ci @ noise["c_means"]) ** 2 + std ** 2) / (2 * AG_SIGMA ** 2 + 0.0000001))
    row_kl = (torch.clamp(kl, min=lam) if lam > 0 else kl).sum(1)
    kld = row_kl.mean() if cfg.prior in ("Normal", "GMM") else row_kl
    Hd = P[DEC + "kernel"].shape[1] // 4
    xd = P["decoder/net/dec_embeddings"][batch["cap_dec"].long()]
    xd.retain_grad()
    rows["decoder/net/dec_embeddings"] = xd
    z0 = torch.zeros(N, Hd, dtype=feats.dtype)
    c, h = cell(images_fv, z0, z0, P[DEC + "kernel"], P[DEC + "bias"])
    if cfg.use_c_v:
        c, h = cell(ci_emb, c, h, P[DEC + "kernel"], P[DEC + "bias"])
    zin = z.reshape(-1, cfg.latent_size * cfg.gen_z_samples)
    z_dec = zin @ P["decoder/net/z_rnn/kernel"] + P["decoder/net/z_rnn/bias"]
    c, h = cell(z_dec, c, h, P[DEC + "kernel"], P[DEC + "bias"])
    outs, _ = dynamic_rnn(xd, lengths, c, h, P[DEC + "kernel"], P[DEC + "bias"])
    logits = outs.reshape(-1, Hd) @ P["decoder/rnn_logits/kernel"] + P["decoder/rnn_logits/bias"]
    labels = batch["cap_enc"].reshape(-1).long()
    V = logits.shape[1]
    lse = torch.logsumexp(logits, 1)
    ce = lse - (1.0 - eps_ls) * logits[torch.arange(logits.shape[0]), labels] - eps_ls / V * logits.sum(1)
    mask = (labels != 0).to(feats.dtype)
    rec = torch.sum(ce * mask) / torch.sum(mask)
    lb = rec + ann * beta * kld / 10
    return dict(kld=kld, rec=rec, lb=lb, kl=kl, rows=rows)


# ------------------------------------------------------------------------------------------------ shared test cases
KL_SHAPES = [(N, L, mode) for N in (1, 5, 8) for L in (12, 64, 150) for mode in (0, 1)]
KL_S = 9   # samples generated per case; the backward tests use the first 0, 5 and 9 of them


def _kl_inputs(N, L, mode, seed):
    rng = np.random.default_rng(seed)
    if mode == 0:
        mean = rng.standard_normal((N, L), dtype=np.float32) * np.float32(0.3)
        std = np.exp(rng.standard_normal((N, L), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
        mu_p = np.zeros((N, L), np.float32)
    else:   # the AG prior's sigma is 0.1: posteriors of that scale around the cluster mean
        mu_p = rng.standard_normal((N, L), dtype=np.float32) * np.float32(0.1)
        mean = mu_p + rng.standard_normal((N, L), dtype=np.float32) * np.float32(0.04)
        std = (0.1 * np.exp(rng.standard_normal((N, L), dtype=np.float32) * np.float32(0.3))).astype(np.float32)
    eps = rng.standard_normal((KL_S, N, L), dtype=np.float32)
    dz = rng.standard_normal((KL_S, N, L), dtype=np.float32)
    return mean, std, mu_p, eps, dz


def kl_case(N, L, mode):
    """One free-bits case (float32 inputs, float64 reference) for the kernels of csrc/loss.hip.  The floor is 0.05 nats.  Asserted
    here, on the CPU, with the reference alone: no element within 1e-4 * max(1, lam) of the floor (fp32 and fp64 could disagree
    about its side), and both branches -- floored and not -- hold at least 10 % of the elements.  A seed whose draw misses either
    is passed over for the next one (the choice depends on the reference alone, never on the code under test)."""
    lam = 0.05
    for attempt in range(64):
        mean, std, mu_p, eps, dz = _kl_inputs(N, L, mode, 1000 * N + 10 * L + mode + 100000 * attempt)
        row_kl, row_raw, row_floored, kl = free_bits_fwd(mode, mean, std, mu_p, lam)
        share = float((kl <= lam).mean())
        if tie_margin(kl, lam) >= 1e-4 and 0.1 <= share <= 0.9:
            break
    assert tie_margin(kl, lam) >= 1e-4, ("an element sits on the floor", N, L, mode, tie_margin(kl, lam))
    assert 0.1 <= share <= 0.9, ("both branches need 10 % of the elements", N, L, mode, share)
    return dict(lam=lam, mean=mean, std=std, mu_p=mu_p, eps=eps, dz=dz, row_kl=row_kl, row_raw=row_raw, row_floored=row_floored, kl=kl)


def roundup(n, m):
    return (n + m - 1) // m * m


# (V, ld, offset in floats of the first logit from a 16-byte boundary, rows): register kernel with every quad tail, the memory kernel
# by size (V > 12288), by pitch (ld % 4 != 0) and by alignment; the last register size and the first memory size (labels >= 1024:
# the label sits in a later quad of its thread)
XENT_SHAPES = [(203, 204, 0, 7), (204, 204, 0, 7), (205, 208, 0, 7), (203, 212, 0, 7), (12300, 12300, 0, 3), (203, 205, 0, 7), (204, 204, 1, 7),
               (12288, 12288, 0, 3), (12289, 12292, 0, 3)]


def xent_case(V, ld, off, R):
    """logits [R, ld] float32 with the pitch padding pre-filled with a sentinel, labels with a PAD row, label V - 1 and label 1"""
    rng = np.random.default_rng(V * 31 + ld + off)
    buf = np.full((R, ld), 777.0, np.float32)
    buf[:, :V] = rng.standard_normal((R, V), dtype=np.float32) * np.float32(3)
    labels = rng.integers(1, V, size=R).astype(np.int32)
    labels[0], labels[1], labels[2] = 0, V - 1, 1
    return buf, labels


# ------------------------------------------------------------------------------------------------ whole steps
ALL_ON = dict(kl_free_bits=0.05, kl_weight=0.5, label_smoothing=0.1, kl_cycle_steps=2, kl_cycle_ramp=0.5)
STEP_OPTIONS = {"all": ALL_ON, "free_bits": dict(kl_free_bits=0.05), "kl_weight": dict(kl_weight=0.5),
                "label_smoothing": dict(label_smoothing=0.1), "cyclical": dict(kl_cycle_steps=2, kl_cycle_ramp=0.5)}


def reference_steps(p, P0, batch, noise, nsteps):
    """`nsteps` training steps of the graph with p's objective options: float64 forward and autograd, then the clip and Adam of
    oracle/optim.py in float32 (as tests/test_gpu_engine.oracle_steps does).  -> list of dict(grads, kld, rec, lb, ann, norm,
    tie_margin, floored_share) per step and the final parameters."""
    import torch
    from oracle import decode as odec
    from oracle import optim as oo
    lam, beta, eps_ls = float(p.kl_free_bits), float(p.kl_weight), float(p.label_smoothing)
    tt = lambda d: {k: torch.tensor(np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in d.items()}
    tb, tn = tt(batch), tt(noise)
    if p.prior == "AG":
        tn["c_means"] = torch.tensor(odec.init_clusters(90, p.latent_size).astype(np.float64))
    P32 = {k: v.astype(np.float32).copy() for k, v in P0.items()}
    st, hist = {}, []
    for s in range(nsteps):
        P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in P32.items()}
        ann = cyclical_ann(s, int(p.kl_cycle_steps), float(p.kl_cycle_ramp), int(p.kl_cycles))
        out = torch_forward(P, tb, tn, p, ann, lam=lam, beta=beta, eps_ls=eps_ls)
        out["lb"].sum().backward()
        grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
        sparse = {k: r.grad.numpy().reshape(-1, r.shape[-1]) for k, r in out["rows"].items()}
        g32 = {k: v.astype(np.float32) for k, v in grads.items()}
        norm = float(oo.global_norm(g32, {k: v.astype(np.float32) for k, v in sparse.items()}))
        scale = float(np.float64(p.lstm_clip_by_norm) * min(1.0 / norm, 1.0 / p.lstm_clip_by_norm))
        kl = out["kl"].detach().numpy()
        hist.append(dict(grads=grads, kld=float(out["kld"].detach().mean()), rec=float(out["rec"].detach()), lb=float(out["lb"].detach().mean()),
                         ann=ann, norm=norm, tie_margin=tie_margin(kl, lam) if lam > 0 else None,
                         floored_share=float((kl <= lam).mean()) if lam > 0 else None, kl_raw=float(kl.sum(1).mean())))
        oo.adam_step(P32, g32, st, p.learning_rate, s + 1, scale=scale)
    return hist, P32
