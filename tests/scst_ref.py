"""Float64 reference of self-critical training (DESIGN.md "Self-critical training"), restated from the definitions and sharing no code
with the product:

  * numpy: the policy loss kernel's three outputs (row_lp, row_ent, the in-place gradient) and the scalar J they differentiate;
  * torch: tests/torch_ref.py's decoder fed a GIVEN z, the policy loss on fixed token samples, autograd, and the clip + optimiser of
    oracle/optim.py over the trained variables only;
  * CIDEr-D rewards from tests/consensus_ref.py with document frequencies from a corpus.
"""
import numpy as np

from . import consensus_ref as cref


# ------------------------------------------------------------------------------------------------ the loss kernel
def policy_J(x, labels, adv, N, scale, beta):
    """J = scale * sum over live rows (-adv[r % N] * log p(label) - beta * H);  x [R, V] float64, rows time-major [T, N]"""
    x = np.asarray(x, np.float64)
    R, V = x.shape
    labels = np.asarray(labels)
    live = (labels > 0) & (labels < V)
    mx = x.max(1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(1)) + mx[:, 0]
    p = np.exp(x - lse[:, None])
    H = lse - (p * x).sum(1)
    lp = x[np.arange(R), np.where(live, labels, 0)] - lse
    a = np.asarray(adv, np.float64)[np.arange(R) % N]
    return float(scale * np.sum(np.where(live, -a * lp - beta * H, 0.0)))


def policy_xent(x, labels, adv, N, scale, beta):
    """-> (row_lp [R], row_ent [R], dlogits [R, V]) of vc_softmax_xent_policy_f32 over the V real columns.  A probability that is 0 in
    float64 contributes exactly 0 to H and to the gradient (H is never computed as log p)."""
    x = np.asarray(x, np.float64)
    R, V = x.shape
    labels = np.asarray(labels)
    live = (labels > 0) & (labels < V)
    mx = x.max(1, keepdims=True)
    e = np.exp(x - mx)
    s = e.sum(1)
    lse = np.log(s) + mx[:, 0]
    p = e / s[:, None]
    H = lse - np.where(p > 0, p * x, 0.0).sum(1)
    lab = np.where(live, labels, 0)
    lp = x[np.arange(R), lab] - lse
    onehot = np.zeros_like(x)
    onehot[np.arange(R), lab] = 1.0
    a = np.asarray(adv, np.float64)[np.arange(R) % N]
    g = a[:, None] * (p - onehot) + beta * np.where(p > 0, p * ((x - lse[:, None]) + H[:, None]), 0.0)
    g = np.where(live[:, None], scale * g, 0.0)
    return np.where(live, lp, 0.0), np.where(live, H, 0.0), g


# (V, ld, offset in floats of the first logit from a 16-byte boundary, T, N)
POLICY_SHAPES = [(203, 204, 0, 3, 3), (204, 204, 0, 3, 3), (205, 208, 0, 3, 3), (203, 212, 0, 3, 3),
                 (203, 205, 0, 3, 3),      # the pitch forces the memory kernel
                 (204, 204, 1, 3, 3),      # misalignment forces the memory kernel
                 (1028, 1028, 0, 2, 1),    # labels 1023 and 1024: the label's quad index changes
                 (12288, 12288, 0, 3, 1),  # last register-kernel size
                 (12289, 12292, 0, 3, 1)]  # first memory-kernel size
SPIKE = 50.0


def policy_case(V, ld, off, T, N):
    """logits [T*N, ld] float32 with the pitch padding pre-filled with a sentinel (as objective_ref.xent_case), labels, advantages
    [N] (negative, zero and positive where N allows) and the planted rows: a PAD row, label V - 1, label 1, one logit raised by 50,
    all-equal logits.  With nine rows each plant has a row of its own; with three, the spike shares the row of label V - 1 and the
    all-equal logits the row of label 1; the two-row case carries the labels 1023 and 1024 its shape is about."""
    R = T * N
    rng = np.random.default_rng(V * 31 + ld + off)
    buf = np.full((R, ld), 777.0, np.float32)
    buf[:, :V] = rng.standard_normal((R, V), dtype=np.float32) * np.float32(3)
    labels = rng.integers(1, V, size=R).astype(np.int32)
    plants = {}
    if R >= 9:
        labels[0], labels[1], labels[2] = 0, V - 1, 1
        plants = dict(pad=0, last=1, first=2, spike=3, equal=4)
    elif R >= 3:
        labels[0], labels[1], labels[2] = 0, V - 1, 1
        plants = dict(pad=0, last=1, first=2, spike=1, equal=2)
    else:
        labels[0], labels[1] = 1023, 1024
    if "spike" in plants:
        buf[plants["spike"], int(rng.integers(0, V - 1))] += np.float32(SPIKE)
        buf[plants["equal"], :V] = np.float32(0.75)
    adv = np.array([-0.8, 0.0, 1.3][:N] if N > 1 else [0.7], np.float32)
    return buf, labels, adv, plants


# ------------------------------------------------------------------------------------------------ fixed samples for whole steps
def sample_case(rng, N, T, V, bos=1, eos=2):
    """Fixed "sampled" captions: N token lists of 1..T tokens over ids 3..V-1, most ended by <EOS>, some cut at T without one, one
    empty sample (<EOS> first); -> (samples, cap_dec [N, T], cap_enc [N, T], lengths [N]) in the layout of a training batch."""
    samples = []
    for n in range(N):
        l = int(rng.integers(1, T + 1))
        s = rng.integers(3, V, size=l).tolist()
        if n == 1:
            s = [eos]
        elif l < T or n % 3:
            s[-1] = eos
        samples.append(s)
    samples[0] = rng.integers(3, V, size=T).tolist()   # a full-length sample without <EOS>
    cap_dec, cap_enc = np.zeros((N, T), np.int32), np.zeros((N, T), np.int32)
    for n, s in enumerate(samples):
        cap_enc[n, :len(s)] = s
        cap_dec[n, :len(s)] = [bos] + s[:-1]
    return samples, cap_dec, cap_enc, np.array([len(s) for s in samples], np.int32)


def trained(name, cfg):
    """does a policy step train this variable?  decoder/*, imf_emb/*, and cv_emb/* where it is fed; never encoder/*"""
    if name.startswith("encoder/"):
        return False
    if name.startswith("cv_emb/"):
        return bool(cfg.use_c_v)
    return True


def torch_policy_forward(P, batch, z, adv, cfg, beta, noise=None):
    """tests/torch_ref.py's decoder (batch-major) fed the given z [N, S*L]; -> dict(J, row_lp [N, T], row_ent [N, T], rows)"""
    import torch
    from .torch_ref import DEC, cell, dynamic_rnn
    feats = batch["features"]
    nc = cfg.num_captions
    B = feats.shape[0]
    feats = feats.unsqueeze(1).repeat(1, nc, 1).reshape(B * nc, -1)
    N = feats.shape[0]
    images_fv = feats @ P["imf_emb/kernel"] + P["imf_emb/bias"]
    Hd = P[DEC + "kernel"].shape[1] // 4
    xd = P["decoder/net/dec_embeddings"][batch["cap_dec"].long()]
    xd.retain_grad()
    x = xd
    if cfg.dec_keep_rate < 1:
        x = x * noise["drop_in"].permute(1, 0, 2) / cfg.dec_keep_rate
    z0 = torch.zeros(N, Hd, dtype=feats.dtype)
    c, h = cell(images_fv, z0, z0, P[DEC + "kernel"], P[DEC + "bias"])
    if cfg.use_c_v:
        c, h = cell(batch["c_v"] @ P["cv_emb/kernel"] + P["cv_emb/bias"], c, h, P[DEC + "kernel"], P[DEC + "bias"])
    if not cfg.no_encoder:
        z_dec = z.reshape(N, -1) @ P["decoder/net/z_rnn/kernel"] + P["decoder/net/z_rnn/bias"]
        c, h = cell(z_dec, c, h, P[DEC + "kernel"], P[DEC + "bias"])
    outs, _ = dynamic_rnn(x, batch["lengths"], c, h, P[DEC + "kernel"], P[DEC + "bias"])
    if cfg.dec_lstm_drop < 1:
        outs = outs * noise["drop_out"].permute(1, 0, 2) / cfg.dec_lstm_drop
    logits = outs.reshape(-1, Hd) @ P["decoder/rnn_logits/kernel"] + P["decoder/rnn_logits/bias"]
    labels = batch["cap_enc"].reshape(-1).long()
    T = batch["cap_enc"].shape[1]
    logp = torch.log_softmax(logits, 1)
    lp = logp[torch.arange(logits.shape[0]), labels]
    H = -(torch.exp(logp) * logp).sum(1)
    live = (labels != 0).to(feats.dtype)
    a = adv.repeat_interleave(T)                      # batch-major rows: row n*T + t belongs to caption n
    J = torch.sum(live * (-a * lp - beta * H)) / N
    return dict(J=J, row_lp=(live * lp).reshape(N, T), row_ent=(live * H).reshape(N, T), rows={"decoder/net/dec_embeddings": xd})


def reference_policy_steps(p, P0, batch, z, advs, beta, nsteps, optimizer="Adam", noise=None):
    """`nsteps` policy steps: float64 forward and autograd, then the clip and optimiser of oracle/optim.py in float32 over the trained
    variables alone (a variable whose gradient is None is skipped by tf.train.Optimizer: no parameter or slot change).
    advs: one [N] advantage vector per step.  -> (per step dict(grads, norm, J, cap_lp), final parameters)"""
    import torch
    from oracle import optim as oo
    tt = lambda d: {k: torch.tensor(np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in d.items()}
    tb = tt(batch)
    tn = tt(noise) if noise else None
    tz = torch.tensor(np.asarray(z, np.float64)) if z is not None else None
    P32 = {k: v.astype(np.float32).copy() for k, v in P0.items()}
    st, hist = {}, []
    for s in range(nsteps):
        P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in P32.items()}
        out = torch_policy_forward(P, tb, tz, torch.tensor(np.asarray(advs[s], np.float64)), p, beta, tn)
        out["J"].backward()
        names = [k for k in P if trained(k, p)]
        assert all(P[k].grad is not None for k in names) and all(P[k].grad is None for k in P if k not in names)
        grads = {k: P[k].grad.numpy() for k in names}
        sparse = {k: r.grad.numpy().reshape(-1, r.shape[-1]) for k, r in out["rows"].items()}
        g32 = {k: v.astype(np.float32) for k, v in grads.items()}
        norm = float(oo.global_norm(g32, {k: v.astype(np.float32) for k, v in sparse.items()}))
        scale = float(np.float64(p.lstm_clip_by_norm) * min(1.0 / norm, 1.0 / p.lstm_clip_by_norm))
        hist.append(dict(grads=grads, norm=norm, J=float(out["J"].detach()), cap_lp=out["row_lp"].detach().numpy().sum(1)))
        if optimizer == "Adam":
            oo.adam_step(P32, g32, st, p.learning_rate, s + 1, scale=scale)
        else:
            lr = oo.decayed_lr(p.learning_rate, s, p.num_ex_per_epoch, p.batch_size, p.num_epochs_per_decay)
            touched = {"decoder/net/dec_embeddings": np.isin(np.arange(P32["decoder/net/dec_embeddings"].shape[0]), batch["cap_dec"])}
            oo.momentum_step(P32, g32, st, lr, scale=scale, touched=touched)
    return hist, P32


# ------------------------------------------------------------------------------------------------ rewards
def cider_rewards(candidates, references, corpus, bos, eos, idf=None, unseen=None):
    """per image a float64 array: each candidate's mean over the image's references of consensus_ref.cider_d, document
    frequencies over the CORPUS images (or the idf table given)"""
    if idf is None:
        idf, unseen = cref.df_idf(corpus, bos, eos)
    out = []
    for cands, refs in zip(candidates, references):
        rv = [cref.vector(r, bos, eos, idf, unseen) for r in refs]
        out.append(np.array([np.mean([cref.cider_d(cref.vector(c, bos, eos, idf, unseen), r) for r in rv]) for c in cands], np.float64))
    return out
