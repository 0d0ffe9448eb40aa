"""Float64 reference of unlikelihood training (DESIGN.md "Unlikelihood training"; Welleck et al. 2020, token level), restated from its
definition and sharing no code with the product:

  * numpy: the candidate sets, what the row kernel leaves per row (row_loss, row_ul, row_cand, row_mass) and the hand-derived gradient
    with the clamp;
  * torch: the same row loss for autograd (tests/test_unlikelihood_host.py compares the two), and the training graph of
    tests/torch_ref.py with the term in it, so that whole steps of the engine can be held against float64 autograd
    (tests/test_gpu_unlikelihood.py).

Rows are time-major everywhere in the numpy half: labels [T, N], logits [T * N, V], row r = t * N + n.
"""
import numpy as np

CLAMP = 1e-5
AG_SIGMA = 0.1


# ------------------------------------------------------------------------------------------------ candidate sets
def candidate_sets(labels, V, window):
    """labels [T, N] -> list over rows r = t * N + n of sorted int arrays: the distinct labels[t', n], max(0, t - window) <= t' < t,
    that are words (0 < c < V) and not the row's own label; empty for a row whose own label is not a word."""
    labels = np.asarray(labels)
    T, N = labels.shape
    out = []
    for t in range(T):
        for n in range(N):
            y = int(labels[t, n])
            if not 0 < y < V:
                out.append(np.zeros(0, np.int64))
                continue
            prev = labels[max(0, t - window):t, n]
            out.append(np.array(sorted({int(c) for c in prev if 0 < c < V and c != y}), np.int64))
    return out


def candidate_mask(labels, V, window):
    """the same as a 0/1 array [T * N, V]"""
    sets = candidate_sets(labels, V, window)
    M = np.zeros((len(sets), V), np.float64)
    for r, c in enumerate(sets):
        M[r, c] = 1.0
    return M


# ------------------------------------------------------------------------------------------------ the row kernel
def ul_rows(logits, labels, eps, alpha, window, gscale=1.0, den=None):
    """logits [T * N, V] (real columns only), labels [T, N].  -> dict(row_loss, row_ul, row_cand, row_mass, dlogits, min_om) with
    live = 0 < y < V, p = softmax(x), om = 1 - p, a candidate clamped when om <= 1e-5 (then -log(1e-5) in the loss, nothing in the
    gradient), r = p / om otherwise, R = sum r over the unclamped candidates, k = live * gscale / den:
      row_loss = live (lse - (1 - eps) x[y] - eps / V sum_v x[v]);  row_ul = live sum_c -log(max(om_c, 1e-5))
      d[v] = k (p_v - (1 - eps) [v == y] - eps / V + alpha (r_v [v in C, unclamped] - p_v R))
    den defaults to the number of live rows; min_om is the smallest 1 - p_c over all candidates (1.0 without any)."""
    x = np.asarray(logits, np.float64)
    labels = np.asarray(labels)
    R_, V = x.shape
    y = labels.reshape(-1)
    live = ((y > 0) & (y < V)).astype(np.float64)
    den = float(live.sum()) if den is None else float(den)
    M = candidate_mask(labels, V, window)
    mx = x.max(1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(1)) + mx[:, 0]
    p = np.exp(x - lse[:, None])
    om = 1.0 - p
    yy = np.where(live > 0, y, 0)
    row_loss = live * (lse - (1.0 - eps) * x[np.arange(R_), yy] - eps / V * x.sum(1))
    clamped = om <= CLAMP
    row_ul = (M * -np.log(np.maximum(om, CLAMP))).sum(1)
    row_mass = (M * p).sum(1)
    r = np.where(clamped, 0.0, p / np.where(clamped, 1.0, om)) * M
    Rsum = r.sum(1, keepdims=True)
    onehot = np.zeros_like(x)
    onehot[np.arange(R_), yy] = 1.0
    k = (live * gscale / den)[:, None]
    d = k * (p - (1.0 - eps) * onehot - eps / V + alpha * (r - p * Rsum))
    min_om = float(om[M > 0].min()) if M.any() else 1.0
    return dict(row_loss=row_loss, row_ul=row_ul, row_cand=M.sum(1).astype(np.int64), row_mass=row_mass, dlogits=d, min_om=min_om)


def ul_stats(c, labels, V):
    """the three reported numbers from ul_rows' output: means over the live rows"""
    y = np.asarray(labels).reshape(-1)
    n = float(((y > 0) & (y < V)).sum())
    return dict(ul=c["row_ul"].sum() / n, ul_candidates=c["row_cand"].sum() / n, repeat_mass=c["row_mass"].sum() / n)


def torch_row_loss(logits, labels, eps, alpha, window, gscale=1.0, den=None):
    """the scalar whose gradient ul_rows derives by hand: gscale / den * sum_live (ce_smooth + alpha * ul), in torch (float64)"""
    import torch
    labels = np.asarray(labels)
    R_, V = logits.shape
    y = torch.as_tensor(labels.reshape(-1)).long()
    live = ((y > 0) & (y < V)).to(logits.dtype)
    den = float(live.sum()) if den is None else float(den)
    M = torch.as_tensor(candidate_mask(labels, V, window))
    lse = torch.logsumexp(logits, 1)
    p = torch.softmax(logits, 1)
    yy = torch.where(live > 0, y, torch.zeros_like(y))
    ce = lse - (1.0 - eps) * logits[torch.arange(R_), yy] - eps / V * logits.sum(1)
    ul = -(M * torch.log(torch.clamp(1.0 - p, min=CLAMP))).sum(1)
    return gscale / den * torch.sum(live * (ce + alpha * ul))


# ------------------------------------------------------------------------------------------------ shared kernel cases
T_CASE, N_CASE = 7, 3
# (V, ld, offset in floats of the first logit from a 16-byte boundary): the smoothed kernel's shapes (register kernel with every quad
# tail; the generic kernel by pitch and by alignment), the widest row of the register kernel, and the generic kernel by size
UL_SHAPES = [(203, 204, 0), (204, 204, 0), (205, 208, 0), (203, 212, 0), (203, 205, 0), (204, 204, 1), (12288, 12288, 0), (12300, 12300, 0)]
MIN_OM = 0.05


def label_grid(V, rng):
    """labels [7, 3]: caption 0 says word 1 three times before t = 4 (dedupe), has label 1 at t = 2 and t = 3 with word 1 behind it
    (an earlier word equal to the label: excluded), carries the candidates in column 1 and column V - 1, and ends in PAD; caption 1
    walks through one float4 (20, 21, 22, 23: at t = 3 three candidates share the label's float4; at t = 2 and t = 4 two candidates share
    one) and ends in a PAD tail of two; caption 2 is random words with one PAD.  Every caption has the t = 0 row without candidates."""
    g = np.zeros((T_CASE, N_CASE), np.int32)
    g[:, 0] = [1, V - 1, 1, 1, 10, 1, 0]
    g[:, 1] = [20, 21, 22, 23, 5, 0, 0]
    g[:6, 2] = rng.integers(1, V, size=6)
    return g


def ul_case(V, ld, off, window=128):
    """logits [21, ld] float32 = 3 * N(0, 1) with the pitch padding pre-filled with a sentinel, and the label grid.  Asserted here, on the
    CPU, with the reference alone: the smallest 1 - p_c over all candidates is at least MIN_OM (far from the clamp).  A seed whose
    draw misses that is passed over for the next one (the choice depends on the reference alone, never on the code under test)."""
    R_ = T_CASE * N_CASE
    for attempt in range(64):
        rng = np.random.default_rng(V * 31 + ld + off + 100000 * attempt)
        buf = np.full((R_, ld), 777.0, np.float32)
        buf[:, :V] = rng.standard_normal((R_, V), dtype=np.float32) * np.float32(3)
        labels = label_grid(V, rng)
        if ul_rows(buf[:, :V], labels, 0.0, 1.0, 128)["min_om"] >= MIN_OM:
            break
    assert ul_rows(buf[:, :V], labels, 0.0, 1.0, window)["min_om"] >= MIN_OM, ("a candidate near the clamp", V, ld, off)
    return buf, labels


# ------------------------------------------------------------------------------------------------ the graph with the term, in torch
def torch_forward(P, batch, noise, cfg, ann, alpha, window, lam=0.0, beta=1.0, eps_ls=0.0):
    """tests/torch_ref.py's forward with the unlikelihood term (and the free-bits / KL-weight / label-smoothing options beside it).
    -> dict(kld, rec (cross-entropy alone), ul (sum row_ul / den), lb (reported: rec + ann * beta * kld / 10), obj (differentiated:
    lb + alpha * ul), kl [N, L], rows {table name: gathered rows with retained gradient}, logits [N * T, V] batch-major)."""
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
    kl = None
    kld = torch.zeros((), dtype=feats.dtype)
    if not cfg.no_encoder:
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
    if not cfg.no_encoder:
        zin = z.reshape(-1, cfg.latent_size * cfg.gen_z_samples)
        z_dec = zin @ P["decoder/net/z_rnn/kernel"] + P["decoder/net/z_rnn/bias"]
        c, h = cell(z_dec, c, h, P[DEC + "kernel"], P[DEC + "bias"])
    outs, _ = dynamic_rnn(xd, lengths, c, h, P[DEC + "kernel"], P[DEC + "bias"])
    logits = outs.reshape(-1, Hd) @ P["decoder/rnn_logits/kernel"] + P["decoder/rnn_logits/bias"]
    cap = batch["cap_enc"]
    labels = cap.reshape(-1).long()
    V = logits.shape[1]
    T = cap.shape[1]
    lse = torch.logsumexp(logits, 1)
    ce = lse - (1.0 - eps_ls) * logits[torch.arange(logits.shape[0]), labels] - eps_ls / V * logits.sum(1)
    mask = (labels != 0).to(feats.dtype)
    den = torch.sum(mask)
    rec = torch.sum(ce * mask) / den
    # candidate masks are built time-major [T, N] and laid out batch-major like the logits rows (n * T + t)
    M = candidate_mask(cap.numpy().T, V, window).reshape(T, N, V).transpose(1, 0, 2).reshape(N * T, V)
    om = torch.clamp(1.0 - torch.softmax(logits, 1), min=CLAMP)
    ul = torch.sum(-(torch.as_tensor(M) * torch.log(om)).sum(1) * mask) / den
    lb = rec if cfg.no_encoder else rec + ann * beta * kld / 10
    return dict(kld=kld, rec=rec, ul=ul, lb=lb, obj=lb + alpha * ul, kl=kl, rows=rows, logits=logits)


def stats_of_logits(logits_bm, cap_enc, window):
    """{"ul", "ul_candidates", "repeat_mass"} of batch-major logits [N * T, V] and labels [N, T] through the numpy reference"""
    cap_enc = np.asarray(cap_enc)
    N, T = cap_enc.shape
    x = np.asarray(logits_bm, np.float64)
    V = x.shape[1]
    x_tm = x.reshape(N, T, V).transpose(1, 0, 2).reshape(T * N, V)
    return ul_stats(ul_rows(x_tm, cap_enc.T, 0.0, 1.0, window), cap_enc.T, V)


def tie_margin(kl, lam):
    return float(np.abs(np.asarray(kl) - lam).min() / max(1.0, lam))


def reference_steps(p, P0, batch, noise, nsteps, grads=True):
    """`nsteps` training steps of the graph with p's unlikelihood weight and window (and free bits, KL weight, label smoothing beside
    them; the annealing coefficient is 1, as in the engine without a schedule): float64 forward and autograd, then the clip and Adam of
    oracle/optim.py in float32 (as tests/objective_ref.reference_steps does).  -> list of dict(grads, kld, rec, lb, ul, ul_candidates,
    repeat_mass, norm, tie_margin) per step and the final parameters.  grads=False keeps the per-step gradients out of the history."""
    import torch
    from oracle import decode as odec
    from oracle import optim as oo
    lam, beta, eps_ls = float(p.kl_free_bits), float(p.kl_weight), float(p.label_smoothing)
    alpha, window = float(p.unlikelihood), int(p.ul_window)
    tt = lambda d: {k: torch.tensor(np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in d.items()}
    tb, tn = tt(batch), tt(noise)
    if p.prior == "AG":
        tn["c_means"] = torch.tensor(odec.init_clusters(90, p.latent_size).astype(np.float64))
    P32 = {k: v.astype(np.float32).copy() for k, v in P0.items()}
    st, hist = {}, []
    for s in range(nsteps):
        P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in P32.items()}
        out = torch_forward(P, tb, tn, p, 1.0, alpha, window, lam=lam, beta=beta, eps_ls=eps_ls)
        out["obj"].sum().backward()
        g = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
        sparse = {k: r.grad.numpy().reshape(-1, r.shape[-1]) for k, r in out["rows"].items()}
        g32 = {k: v.astype(np.float32) for k, v in g.items()}
        norm = float(oo.global_norm(g32, {k: v.astype(np.float32) for k, v in sparse.items()}))
        scale = float(np.float64(p.lstm_clip_by_norm) * min(1.0 / norm, 1.0 / p.lstm_clip_by_norm))
        h = dict(kld=float(out["kld"].detach().mean()), rec=float(out["rec"].detach()), lb=float(out["lb"].detach().mean()), norm=norm,
                 tie_margin=tie_margin(out["kl"].detach().numpy(), lam) if lam > 0 else None)
        h.update(stats_of_logits(out["logits"].detach().numpy(), batch["cap_enc"], window))
        assert abs(h["ul"] - float(out["ul"].detach())) <= 1e-9 * max(1.0, abs(h["ul"]))   # the numpy and the torch statement agree
        if grads:
            h["grads"] = g
        hist.append(h)
        oo.adam_step(P32, g32, st, p.learning_rate, s + 1, scale=scale)
    return hist, P32


def reference_repeat_mass(p, P, batch, noise):
    """repeat_mass of the model with parameters P on the batch: a forward pass alone"""
    import torch
    from oracle import decode as odec
    tt = lambda d: {k: torch.tensor(np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in d.items()}
    tb, tn = tt(batch), tt(noise)
    if p.prior == "AG":
        tn["c_means"] = torch.tensor(odec.init_clusters(90, p.latent_size).astype(np.float64))
    Pt = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in P.items()}
    out = torch_forward(Pt, tb, tn, p, 1.0, 1.0, int(p.ul_window))
    return stats_of_logits(out["logits"].detach().numpy(), batch["cap_enc"], int(p.ul_window))["repeat_mass"]


# the behaviour case (tests/test_gpu_unlikelihood.py, DESIGN.md "Unlikelihood training"): prior, sizes, steps and the seed at which the
# float64 reference's repeat_mass after the steps differs by at least 10 % between alpha = 1 and alpha = 0 (found with the reference
# alone: tests/test_unlikelihood_host.py asserts it)
BEHAVIOUR = dict(prior="Normal", V=203, B=4, T=6, steps=60, seed=24)
