"""Float64 reference of the bag-of-words auxiliary loss (DESIGN.md "Bag-of-words loss"; Zhao, Zhao & Eskenazi 2017), restated from its
definition and sharing no code with the product:

  * numpy: the bags, what the row kernel leaves per caption (row_loss, row_mass, row_words) and the hand-derived gradient;
  * torch: the same loss for autograd (tests/test_bow_host.py compares the two), and the training graph of tests/torch_ref.py with the
    head on the decoder's z step in it, so that whole steps of the engine can be held against float64 autograd
    (tests/test_gpu_bow.py).

labels are time-major [T, N] in the numpy half, as the kernel reads them; logits have one row per CAPTION: [N, V].
"""
import numpy as np

AG_SIGMA = 0.1
GUARD = 777.0
N_CASE = 4


# ------------------------------------------------------------------------------------------------ the row kernel
def bags(labels, V):
    """labels [T, N] -> per caption n the sorted multiset (a list with repeats) of its words: labels[t, n] with 0 < label < V"""
    labels = np.asarray(labels)
    return [sorted(int(w) for w in labels[:, n] if 0 < w < V) for n in range(labels.shape[1])]


def bow_rows(logits, labels, gscale=1.0, den=None):
    """logits [N, V] (real columns only), labels [T, N].  -> dict(row_loss, row_mass, row_words, dlogits, m) with, per caption, m = the
    bag's size with multiplicity, c_w = the count of word w in it, p = softmax(x), k = gscale / den:
      row_loss = m lse(x) - sum_w c_w x_w;  row_mass = sum over the distinct bag words of p_w;  row_words = their number;
      d[v] = k (m p_v - c_v)
    den defaults to the number of non-PAD labels (labels != 0), the cross-entropy's denominator."""
    x = np.asarray(logits, np.float64)
    labels = np.asarray(labels)
    N, V = x.shape
    den = float((labels != 0).sum()) if den is None else float(den)
    mx = x.max(1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(1)) + mx[:, 0]
    p = np.exp(x - lse[:, None])
    C = np.zeros((N, V), np.float64)
    for n, bag in enumerate(bags(labels, V)):
        for w in bag:
            C[n, w] += 1.0
    m = C.sum(1)
    k = gscale / den if den > 0 else 0.0
    return dict(row_loss=m * lse - (C * x).sum(1), row_mass=((C > 0) * p).sum(1), row_words=(C > 0).sum(1).astype(np.int64),
                dlogits=k * (m[:, None] * p - C), m=m)


def bow_stats(c):
    """the three reported numbers from bow_rows' output: nats per bag word; mean distinct words and mean mass per non-empty caption"""
    ne = float((c["row_words"] > 0).sum())
    return dict(bow=c["row_loss"].sum() / c["m"].sum(), bow_words=c["row_words"].sum() / ne, bow_mass=c["row_mass"].sum() / ne)


def torch_row_loss(logits, labels, gscale=1.0, den=None):
    """the scalar whose gradient bow_rows derives by hand: gscale / den * sum over captions and their bag words of -log p_w (float64)"""
    import torch
    labels = np.asarray(labels)
    den = float((labels != 0).sum()) if den is None else float(den)
    lsm = torch.log_softmax(logits, 1)
    tot = torch.zeros((), dtype=logits.dtype)
    for n, bag in enumerate(bags(labels, logits.shape[1])):
        for w in bag:
            tot = tot - lsm[n, w]
    return gscale / den * tot


# ------------------------------------------------------------------------------------------------ shared kernel cases
def bow_labels(V, T, rng):
    """labels [T, 4]: caption (a) says word 1 three times and word V - 1 once (multiplicity; columns 1 and V - 1, the latter in the last
    quad next to the pitch padding when V % 4 != 0); caption (b) walks through one float4 (20, 21, 22, 23) with a PAD in the middle, an
    id >= V and a negative id, none of which is in the bag; caption (c) is random words over the full length T; caption (d) is all PAD.
    A list longer than T is cut at T."""
    g = np.zeros((T, N_CASE), np.int32)
    a = [1, V - 1, 1, 1][:T]
    b = [20, 21, 0, 22, 23, V + 3, -2][:T]
    g[:len(a), 0] = a
    g[:len(b), 1] = b
    g[:, 2] = rng.integers(1, V, size=T)
    return g


def bow_case(V, ld, off, T):
    """logits [4, ld] float32 = 3 * N(0, 1) with the pitch padding pre-filled with GUARD, and the label grid [T, 4]"""
    rng = np.random.default_rng(V * 31 + ld + off + 1000 * T)
    buf = np.full((N_CASE, ld), GUARD, np.float32)
    buf[:, :V] = rng.standard_normal((N_CASE, V), dtype=np.float32) * np.float32(3)
    return buf, bow_labels(V, T, rng)


# ------------------------------------------------------------------------------------------------ the graph with the head, in torch
def torch_forward(P, batch, noise, cfg, ann, A, lam=0.0, beta=1.0, eps_ls=0.0):
    """tests/torch_ref.py's forward with the bag-of-words head on the decoder's z step z_rnn(z) (and the free-bits / KL-weight /
    label-smoothing options beside it).  -> dict(kld, rec (cross-entropy alone), bow (sum row_loss / den), lb (reported: rec + ann *
    beta * kld / 10), obj (differentiated: lb + A * bow), kl [N, L], rows {table name: gathered rows with retained gradient},
    bow_logits [N, V])."""
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
    cap = batch["cap_enc"]
    labels = cap.reshape(-1).long()
    V = logits.shape[1]
    lse = torch.logsumexp(logits, 1)
    ce = lse - (1.0 - eps_ls) * logits[torch.arange(logits.shape[0]), labels] - eps_ls / V * logits.sum(1)
    mask = (labels != 0).to(feats.dtype)
    den = torch.sum(mask)
    rec = torch.sum(ce * mask) / den
    # the head: sees z_rnn(z) alone; every word of the caption (with repeats) is a target of the one softmax
    bow_logits = z_dec @ P["bow/kernel"] + P["bow/bias"]
    lsm = torch.log_softmax(bow_logits, 1)
    inbag = ((cap > 0) & (cap < V)).to(feats.dtype)                      # [N, T]
    bow = -(torch.gather(lsm, 1, cap.long().clamp(0, V - 1)) * inbag).sum() / den
    lb = rec + ann * beta * kld / 10
    return dict(kld=kld, rec=rec, bow=bow, lb=lb, obj=lb + A * bow, kl=kl, rows=rows, bow_logits=bow_logits)


def tie_margin(kl, lam):
    return float(np.abs(np.asarray(kl) - lam).min() / max(1.0, lam))


def reference_steps(p, P0, batch, noise, nsteps, grads=True):
    """`nsteps` training steps of the graph with p's bag-of-words weight (and free bits, KL weight, label smoothing beside it; the
    annealing coefficient is 1, as in the engine without a schedule): float64 forward and autograd, then the clip and Adam of
    oracle/optim.py in float32 (as tests/unlikelihood_ref.reference_steps does).  -> list of dict(grads, kld, rec, lb, bow, bow_words,
    bow_mass, norm, tie_margin) per step and the final parameters."""
    import torch
    from oracle import decode as odec
    from oracle import optim as oo
    lam, beta, eps_ls, A = float(p.kl_free_bits), float(p.kl_weight), float(p.label_smoothing), float(p.bow_loss)
    tt = lambda d: {k: torch.tensor(np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in d.items()}
    tb, tn = tt(batch), tt(noise)
    if p.prior == "AG":
        tn["c_means"] = torch.tensor(odec.init_clusters(90, p.latent_size).astype(np.float64))
    P32 = {k: v.astype(np.float32).copy() for k, v in P0.items()}
    st, hist = {}, []
    for s in range(nsteps):
        P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in P32.items()}
        out = torch_forward(P, tb, tn, p, 1.0, A, lam=lam, beta=beta, eps_ls=eps_ls)
        out["obj"].sum().backward()
        g = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
        sparse = {k: r.grad.numpy().reshape(-1, r.shape[-1]) for k, r in out["rows"].items()}
        g32 = {k: v.astype(np.float32) for k, v in g.items()}
        norm = float(oo.global_norm(g32, {k: v.astype(np.float32) for k, v in sparse.items()}))
        scale = float(np.float64(p.lstm_clip_by_norm) * min(1.0 / norm, 1.0 / p.lstm_clip_by_norm))
        h = dict(kld=float(out["kld"].detach().mean()), rec=float(out["rec"].detach()), lb=float(out["lb"].detach().mean()), norm=norm,
                 tie_margin=tie_margin(out["kl"].detach().numpy(), lam) if lam > 0 else None)
        c = bow_rows(out["bow_logits"].detach().numpy(), np.asarray(batch["cap_enc"]).T)
        h.update(bow_stats(c))
        den = float((np.asarray(batch["cap_enc"]) != 0).sum())
        assert abs(c["row_loss"].sum() / den - float(out["bow"].detach())) <= 1e-9 * max(1.0, abs(float(out["bow"].detach())))   # numpy and torch agree
        if grads:
            h["grads"] = g
        hist.append(h)
        oo.adam_step(P32, g32, st, p.learning_rate, s + 1, scale=scale)
    return hist, P32
