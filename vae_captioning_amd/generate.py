"""Caption generation on device: batched greedy decoding and beam search
(vae_model/decoder.py:145-320, ops/inference.py).

The reference decodes ONE image and ONE beam per `sess.run` (batch 1, one Python<->runtime
crossing per token per beam).  Here every round advances all images x all live beams in one
batched LSTM step + logits GEMM + softmax + top-k on the GPU, and the O(beam) bookkeeping (TopN
heaps, sentence lists, length-normalised scores) runs in `vc_beam_update`, one wave per image,
with the reference's exact semantics: stable top-`beam_size` expansion, p < 1e-12 skipped, heapq
tie order, score = logprob / len**0.7 for completed captions, `<BOS>` consumed twice
(decoder.py:230-262).  The host is not involved between decoder steps.
Per-image semantics of the z input are those of batch 1: row b of the z_rnn input is the S
samples of image b (the Q1 reshape is the identity at N = 1).
"""
import gc
import os
import types

import numpy as np
import torch

from . import spec
from .abi import ptr as P
from .controls import MAX_BANNED, active as active_controls
from .decode_host import (CBS_MAX_SETS, CBS_MAX_WORDS, DIVERSE_MAX_DRAWS, SCORE_MAX_TOKENS, FieldLayout, beam_fields, beams_from_host,  # noqa: F401 (re-exported)
                          check_constraints, check_truncation, check_typical, diverse_fields, diverse_from_host, marginal_greedy_from_host, merge_groups,
                          rerank_by_marginal, sbs_from_host, sbs_weights, select_bank)
from .engine import K_CL, _stream

# vae_model/decoder.py:56 -- category ids absent from MSCOCO (obj_vectors/category_index.pickle)
UN_CLUSTERS = {0, 66, 68, 69, 71, 12, 45, 83, 26, 29, 30}

PHASE_TIMES = None   # diagnostics (tools/experiments/prof_beam.py, score_time.py): a dict here makes beam_search / score synchronise at its phase boundaries and add up seconds


def _phase(name, t0):
    if PHASE_TIMES is None:
        return t0
    import time
    torch.cuda.synchronize()
    t = time.perf_counter()
    PHASE_TIMES[name] = PHASE_TIMES.get(name, 0.0) + (t - t0)
    return t


def _cut(a, sl, axis=0):
    """A pass's share a[sl] along `axis` of an optional array (c_v [B, 90]; eps [K, S, B, L], uniforms [K, T, B]: axis 2); None stays None."""
    return None if a is None else a[(slice(None),) * axis + (sl,)]


class _BeamSlice(object):
    """The TopN state of B images x n beams, sentences of <= L tokens (vae_model/decoder.py:238-247), in persistent buffers of the generator.
    What the host reads lives in TWO flat buffers (ibuf: beam_fields; dbuf: float64 p_score, c_score, p_logprob, c_logprob [B, n], then
    `extra`): two copies into pinned memory bring it back, no gathering launches.  sent: the stores that alternate with the round's parity."""
    def __init__(self, gen, tag, B, n, L, extra=()):
        M, i32 = B * n, torch.int32
        self.B, self.n, self.L = B, n, L
        self.lay = FieldLayout(beam_fields(B, n, L))
        self.dlay = FieldLayout([(k_, M) for k_ in ("p_score", "c_score", "p_logprob", "c_logprob")] + list(extra))
        self.ibuf, self.dbuf = gen._b(tag + "ibuf", (self.lay.total,), i32), gen._b(tag + "dbuf", (self.dlay.total,), torch.float64)
        self.i, self.d = self.lay.views(self.ibuf), self.dlay.views(self.dbuf)
        self.sent = [self.i["sent0"], self.i["sent1"]]
        self.c_free, self.parent, self.tok = gen._b(tag + "c_free", (B,), i32), gen._b(tag + "parent", (M,), i32), gen._b(tag + "tok", (M,), i32)
        self.tensors = [self.ibuf, self.dbuf, self.c_free, self.parent, self.tok]
        self.scores = self.dbuf[:self.dlay.off["p_logprob"]]   # (the host reads the scores only)

    def init(self, lib, bos, H, c, h, c2, h2):
        """One launch: partial = [Beam([bos], state b, 0.0, 0.0)], every row of c2, h2 [B*n, H] = its image's row of c, h; parent = identity"""
        i, d = self.i, self.d
        lib.vc_beam_init(_stream(), self.B, self.n, self.L, int(bos), H, P(c), P(h), P(c2), P(h2), P(i["pcount"]), P(i["ccount"]), P(d["p_score"]),
                         P(d["p_logprob"]), P(i["p_len"]), P(self.sent[0]), P(self.sent[1]), P(d["c_score"]), P(d["c_logprob"]), P(i["c_len"]),
                         P(i["c_slot"]), P(self.c_free), P(i["c_sent"]), P(self.parent), P(self.tok))

    def update_args(self, parity):
        """the state pointers that end vc_beam_update's (_groups', _constrained's) arguments in a round that reads sent[parity]"""
        i, d = self.i, self.d
        return (P(i["pcount"]), P(i["ccount"]), P(d["p_score"]), P(d["p_logprob"]), P(i["p_len"]), P(self.sent[parity]), P(self.sent[1 - parity]),
                P(d["c_score"]), P(d["c_logprob"]), P(i["c_len"]), P(i["c_slot"]), P(self.c_free), P(i["c_sent"]), P(self.parent), P(self.tok))


class CaptionGenerator(object):
    def __init__(self, engine):
        self.e = engine
        self.p = engine.p
        self.lib = engine.lib
        self.buf = {}
        self._ones = {}
        self._whp = None        # decoder Wh in the recurrence kernel's operand order
        self._whp_version = None  # engine.param_version the pack was made at (the weights may have been trained in between)
        self._graphs = {}        # captured decode rounds (hipGraphs), keyed by shapes + the addresses they bake
        self._xproj = None       # [V, 4H] input projection of every word (beam search with many rows x rounds)
        self._xproj_version = None
        self._side = []          # extra streams of a sliced beam search
        self.slices, self.slice_rows = 2, 256   # beam search: images decoded as `slices` independent slices when each has >= slice_rows rows
        self.diverse_rows = 4096  # diverse captioning: candidate rows (images x draws) per pass
        self.last_candidates = None   # diverse(): per image the K candidates (tokens, logprob, ended) of the last call, in draw order
        # score(): row-steps (sequence rows x steps) per pass; act [T, N, 4H] + cs, hs [T + 1, N, H] are <= 8 H floats per row-step: 1 GiB
        self._t_score = 0.0   # (diagnostics: PHASE_TIMES)
        self.score_rows = max(1, (1 << 30) // (32 * int(engine.p.decoder_hidden)))
        self.bound_rows = self.score_rows   # bound(): the same budget (its teacher forcing is score()'s; the encoder pass has 1 / K of the rows)

    def _b(self, name, shape, dtype=torch.float32):
        t = self.buf.get(name)
        shape = tuple(int(s) for s in shape)
        if t is None or tuple(t.shape) != shape or t.dtype != dtype:
            t = torch.zeros(shape, dtype=dtype, device=self.e.dev)
            self.buf[name] = t
        return t

    def _dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(self.e.dev)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.e.dev)

    def _load(self, dst, a):
        """host array or tensor -> the persistent device buffer dst (same shape), which it returns"""
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        return dst.copy_(a.reshape(dst.shape), non_blocking=True)

    def prior_mean(self, c_v):
        """decoder.py:42-71: zeros, or for the AG prior the mean of the image's cluster means
        (empty cluster vector -> every used category id; ids beyond the 90-row matrix, quirk Q16,
        are dropped)."""
        p = self.p
        B = c_v.shape[0] if c_v is not None else 0
        if p.prior != "AG" or c_v is None:
            return None
        cm = self.e.c_means.cpu().numpy()
        out = np.zeros((B, p.latent_size), np.float32)
        for b in range(B):
            idx = np.nonzero(c_v[b] > 0)[0]
            if idx.size == 0:
                idx = np.array([i for i in range(p.num_clusters + 1) if i not in UN_CLUSTERS and i < cm.shape[0]])
            out[b] = cm[idx].mean(axis=0)
        return out

    # ------------------------------------------------------------------ init chain
    def _image_rows(self, tag, n, features, c_v, z_rows, encoder=False):
        """What both init chains do on their B image rows, n LSTM steps long: features, cluster vectors and AG prior means (host-computed) go
        into the persistent buffers feats, cv, pmd (None where the model has none), the workspace is sized (z_rows: rows of the z_rnn
        product), and two launch lists are made: embed(tg), X[0] = imf_emb(features), X[1] = cv_emb(c_v); lstm(st), the n steps over X from
        a zero state, to cs[n] / hs[n].  Returns them all (a captured chain bakes the buffers' addresses).
        encoder=True: the same chain through the ENCODER cell (encoder.py:38-50: the image-only steps of q_net; no prior mean)."""
        e, p, lib, S = self.e, self.p, self.lib, self.e.store
        B, E, Hd, F = int(features.shape[0]), p.embed_size, (p.encoder_hidden if encoder else p.decoder_hidden), p.cnn_feature_size
        cell = spec.ENC_CELL if encoder else spec.DEC_CELL
        feats = self._load(self._b(tag + "feats", (B, F)), features)
        cv = self._load(self._b(tag + "cv", (B, K_CL)), c_v) if e.feed_cv else None
        pm = self.prior_mean(np.asarray(c_v) if c_v is not None else None) if e.enc and not encoder else None
        pmd = self._load(self._b(tag + "pm", (B, p.latent_size)), pm) if pm is not None else None
        X, act = self._b(tag + "X", (n, B, E)), self._b(tag + "act0", (n, B, 4 * Hd))
        cs, hs, lens = self._b(tag + "cs0", (n + 1, B, Hd)), self._b(tag + "hs0", (n + 1, B, Hd)), self._ones_for(B, n)
        e._need_ws(lib.vc_lstm_seq_workspace_bytes(n, B, E, Hd))
        for sh in ((B, E, F), (B, E, K_CL), (z_rows, E, p.gen_z_samples * p.latent_size)):
            e._need_ws(lib.vc_gemm_workspace_bytes(*sh))

        def embed(tg):
            e.gemm(0, 0, B, E, F, feats, F, S.param("imf_emb/kernel"), E, X[0], E, S.param("imf_emb/bias"), tag=tg)
            if e.feed_cv:
                e.gemm(0, 0, B, E, K_CL, cv, K_CL, S.param("cv_emb/kernel"), E, X[1], E, S.param("cv_emb/bias"), tag=tg)

        def lstm(st):
            lib.vc_fill_f32(st, P(cs[0]), B * Hd, 0.0)
            lib.vc_fill_f32(st, P(hs[0]), B * Hd, 0.0)
            lib.vc_lstm_seq_fwd_f32(st, n, B, E, Hd, P(X), P(S.param(cell + "kernel")), P(S.param(cell + "bias")),
                                    P(lens), P(act), P(cs), P(hs), P(e.ws), e.ws_bytes, e.lstm_flags)

        return types.SimpleNamespace(feats=feats, cv=cv, pmd=pmd, X=X, act=act, cs=cs, hs=hs, lens=lens, embed=embed, lstm=lstm)

    def _replay_or_capture(self, key, launches):
        """Replay the hipGraph of a launch list or, on the first call of its key, run it eagerly and capture it for the next (a capture
        executes nothing: the eager launches are this call's).  launches(timed): timed = False inside the capture (no timer events)."""
        graph = self._graphs.get(key)
        if graph is not None:
            graph.replay()
        else:
            launches(True)
            self._capture(key, lambda: launches(False))

    def init_state(self, features, c_v=None, eps=None):
        """State after image -> (c_v) -> z (decoder.py:96-114), batched over B images.
        eps: [S, B, L] N(0,1) draws (generated on device when None).
        Returns (c, h) [B, H] in PERSISTENT buffers of this generator (valid until its next call).  The dozen launches (three small
        products, the sampling, two or three LSTM steps) replay as one hipGraph from the second call of a shape on: at 32-128 images
        they are ~50 us of kernels behind ~250 us of launch calls.  VC_DECODE_GRAPH=0 keeps the eager launches."""
        e, p, lib, S = self.e, self.p, self.lib, self.e.store
        B = int(features.shape[0])
        E, L, Sm = p.embed_size, p.latent_size, p.gen_z_samples
        n_init = e.n_init_d
        tag = "in%d_" % B
        im = self._image_rows(tag, n_init, features, c_v, B)
        pmd, have_pm = im.pmd, im.pmd is not None
        epsd = mean = std = z = None
        if e.enc:
            z, epsd = self._b(tag + "z", (B, Sm, L)), self._b(tag + "eps", (B, Sm, L))
            if eps is not None:
                self._load(epsd, np.transpose(np.asarray(eps, np.float32), (1, 0, 2)))
            mean, std = self._b(tag + "zmean", (B * Sm, L)), self._b(tag + "zstd", (B * Sm, L))

        def launches(timed):
            st, tg = _stream(), ("gemm" if timed else None)
            im.embed(tg)
            if e.enc:
                if eps is None:
                    lib.vc_philox_normal_f32(st, P(epsd), epsd.numel(), e.seed * 1000003 + 17, 5 << 32, P(e.step))
                if have_pm:
                    lib.vc_tile_rows_f32(st, P(pmd), B, Sm, L, P(mean))
                else:
                    lib.vc_fill_f32(st, P(mean), mean.numel(), 0.0)
                lib.vc_fill_f32(st, P(std), std.numel(), float(p.std))
                lib.vc_latent_sample_f32(st, 1, B * Sm, L, P(mean), P(std), P(epsd), P(z))  # decoder.py:72-74
                # (not _z_step: here z is row n_init - 1 of X, inside the ONE sequence call below -- a step of its own would be another launch)
                e.gemm(0, 0, B, E, Sm * L, z, Sm * L, S.param("decoder/net/z_rnn/kernel"), E, im.X[n_init - 1], E, S.param("decoder/net/z_rnn/bias"), tag=tg)
            im.lstm(st)

        key = self._graph_key("init", B, eps is None, have_pm, float(p.std), e.lstm_flags, e.seed,
                              tensors=[im.feats, im.X, im.cv, epsd, mean, std, z, im.act, im.cs, im.hs, im.lens] + ([pmd] if have_pm else []))
        self._replay_or_capture(key, launches)
        return im.cs[n_init], im.hs[n_init]

    def _z_step(self, tag, rows):
        """The z step of `rows` decoder rows (decoder.py:111): persistent z [rows, S, L], Xz, act1 (None without z) and the state pair cs1 / hs1
        [2, rows, H] -- the caller tiles or gathers the image states into [0] and fills z with its own latent kernel -- the workspace
        request, and run(st, tg): the z_rnn product and the ONE LSTM step from [0] to [1]."""
        e, p, lib, S = self.e, self.p, self.lib, self.e.store
        E, Hd, L, Sm = p.embed_size, p.decoder_hidden, p.latent_size, p.gen_z_samples
        zs = types.SimpleNamespace(z=None, Xz=None, act1=None, ones=self._ones_for(rows))
        if e.enc:
            zs.z, zs.Xz, zs.act1 = self._b(tag + "z", (rows, Sm, L)), self._b(tag + "Xz", (1, rows, E)), self._b(tag + "act1", (1, rows, 4 * Hd))
        zs.cs1, zs.hs1 = self._b(tag + "cs1", (2, rows, Hd)), self._b(tag + "hs1", (2, rows, Hd))
        e._need_ws(lib.vc_lstm_seq_workspace_bytes(1, rows, E, Hd))

        def run(st, tg):
            e.gemm(0, 0, rows, E, Sm * L, zs.z, Sm * L, S.param("decoder/net/z_rnn/kernel"), E, zs.Xz[0], E, S.param("decoder/net/z_rnn/bias"), tag=tg)
            lib.vc_lstm_seq_fwd_f32(st, 1, rows, E, Hd, P(zs.Xz), P(S.param(spec.DEC_CELL + "kernel")), P(S.param(spec.DEC_CELL + "bias")),
                                    P(zs.ones), P(zs.act1), P(zs.cs1), P(zs.hs1), P(e.ws), e.ws_bytes, e.lstm_flags)

        zs.run = run
        return zs

    def _xproj_for(self, rows, rounds):
        """_project_vocab's table for a decode of rows x rounds word lookups, or None when they are fewer than the V rows of the one product
        that makes it (or H is no multiple of 4: the gather moves float4s).  VC_DECODE_XPROJ=0: never (A/B runs)."""
        pays = rows * rounds >= self.e.V and self.p.decoder_hidden % 4 == 0 and os.environ.get("VC_DECODE_XPROJ", "1") != "0"
        return self._project_vocab() if pays else None

    # ------------------------------------------------------------------ one decoder step
    def _round_bufs(self, tag, M):
        """Persistent buffers of one decoder step over M rows (a captured round bakes their addresses)."""
        p, e = self.p, self.e
        E, Hd, V = p.embed_size, p.decoder_hidden, e.V
        return {"x": self._b(tag + "x", (M, E)), "gact": self._b(tag + "gact", (M, 4 * Hd)), "c2": self._b(tag + "c2", (M, Hd)),
                "h2": self._b(tag + "h2", (M, Hd)), "logits": self._b(tag + "logits", (M, V))}

    def _ones_for(self, M, n=1):
        """[M] int32 of n: the "every row runs n steps" lengths of an LSTM launch, 1 for a decoder step (persistent: captured graphs bake it)"""
        t = self._ones.get((M, n))
        if t is None:
            t = self._ones[(M, n)] = torch.full((M,), n, dtype=torch.int32, device=self.e.dev)
        return t

    def _pack_wh(self, M):
        """decoder Wh in the recurrence step kernel's operand order, once per parameter version (engine.param_version)"""
        e, p, lib = self.e, self.p, self.lib
        E, Hd = p.embed_size, p.decoder_hidden
        if self._whp_version == e.param_version or not lib.vc_lstm_step_packed_supported(M, Hd):
            return
        if self._whp is None or self._whp.numel() != 2 * Hd * 4 * Hd:
            self._whp = torch.empty(2 * Hd * 4 * Hd, dtype=torch.float32, device=e.dev)
        lib.vc_lstm_pack_wh_f32(_stream(), Hd, e.store.param(spec.DEC_CELL + "kernel").data_ptr() + E * 4 * Hd * 4, P(self._whp))
        self._whp_version = e.param_version

    def _project_vocab(self):
        """xproj [V, 4H] = dec_embeddings . Wx + b: the LSTM input projection of EVERY word, once per parameter version
        (engine.param_version: the weights may have been trained or reloaded since the last call).  A round then looks its rows up (vc_beam_gather_f32) instead of gathering embeddings and
        multiplying: one product of V rows (0.1 ms at V = 10 000) against rows x rounds of them -- callers use it when rows x rounds >= V."""
        e, p, S = self.e, self.p, self.e.store
        E, Hd, V = p.embed_size, p.decoder_hidden, e.V
        if self._xproj_version != e.param_version:
            if self._xproj is None or tuple(self._xproj.shape) != (V, 4 * Hd):
                self._xproj = torch.empty((V, 4 * Hd), dtype=torch.float32, device=e.dev)
            e.gemm(0, 0, V, 4 * Hd, E, S.param("decoder/net/dec_embeddings"), E, S.param(spec.DEC_CELL + "kernel"), 4 * Hd, self._xproj, 4 * Hd,
                   S.param(spec.DEC_CELL + "bias"))
            self._xproj_version = e.param_version
        return self._xproj

    def step(self, tokens, c, h, want="probs", bufs=None, timed=True, projected=False):
        """Feed one token per row: returns (softmax probs [M, V], c', h').  bufs (from _round_bufs): write x / gate activations / new
        state / logits into these persistent tensors instead of fresh ones (c, h must not alias bufs["c2"] / bufs["h2"]).
        projected: bufs["gact"] already holds the tokens' input projections (vc_beam_gather_f32 from _project_vocab's table)."""
        e, p, lib, st, S = self.e, self.p, self.lib, _stream(), self.e.store
        M = int(tokens.shape[0])
        E, Hd, V = p.embed_size, p.decoder_hidden, e.V
        new = lambda k, shape: bufs[k] if bufs is not None else torch.empty(shape, dtype=torch.float32, device=e.dev)
        W = S.param(spec.DEC_CELL + "kernel")
        gact = new("gact", (M, 4 * Hd))
        if not projected:
            x = new("x", (M, E))
            lib.vc_embedding_gather_f32(st, P(S.param("decoder/net/dec_embeddings")), P(tokens), M, E, V, P(x))
            e.gemm(0, 0, M, 4 * Hd, E, x, E, W, 4 * Hd, gact, 4 * Hd, S.param(spec.DEC_CELL + "bias"), tag="gemm" if timed else None)
        c2, h2 = new("c2", (M, Hd)), new("h2", (M, Hd))
        ones = self._ones_for(M)
        if lib.vc_lstm_step_packed_supported(M, Hd):  # the recurrence step kernel on Wh packed once per weight version
            self._pack_wh(M)
            lib.vc_lstm_step_fwd_packed_f32(st, M, Hd, 0, P(h), P(c), P(self._whp), P(gact), P(ones), P(c2), P(h2))
        else:
            lib.vc_lstm_step_fwd_f32(st, M, Hd, 0, P(h), P(c), W.data_ptr() + E * 4 * Hd * 4, P(gact), P(ones), P(c2), P(h2))
        if want == "state":   # (beam search's first step: decoder.py:230-236 runs it for the state only)
            return None, c2, h2
        logits = new("logits", (M, V))
        e.gemm(0, 0, M, V, Hd, h2, Hd, S.param("decoder/rnn_logits/kernel"), e.Vp, logits, V, S.param("decoder/rnn_logits/bias"),
               tag="logits_gemm" if timed else None)   # (None inside a hipGraph capture: no timer events)
        if want == "logits":
            return logits, c2, h2
        probs = torch.empty_like(logits)
        lib.vc_softmax_rows_f32(st, P(logits), M, V, V, P(probs), V)
        return probs, c2, h2

    # ------------------------------------------------------------------ captured rounds
    def _pinned(self, name, n, dtype):
        t = self.buf.get(name)
        if t is None or t.numel() != n or t.dtype != dtype:
            t = self.buf[name] = torch.zeros(int(n), dtype=dtype).pin_memory()
        return t

    def _to_host(self, tag, ibuf, dbuf, wait=True):
        """A pass's flat result buffers (int32 fields or None, float64 companion) as numpy views of pinned memory: two non-blocking copies
        and ONE stream synchronise (wait=False: left to a later call -- the slices of a beam search share one), no gathering launches."""
        hosts = [None, None]
        for j, (name, buf) in enumerate((("ihost", ibuf), ("dhost", dbuf))):
            if buf is not None:
                hosts[j] = self._pinned(tag + name, buf.numel(), buf.dtype).copy_(buf, non_blocking=True).numpy()
        if wait:
            torch.cuda.current_stream().synchronize()
        return hosts

    def _pinned_alive(self, n):
        t = self.buf.get("bm_host_alive")
        if t is None or t.numel() < n:
            t = self.buf["bm_host_alive"] = torch.ones(max(n, 16), dtype=torch.float32).pin_memory()
        t.fill_(1.0)
        return t

    def _graph_key(self, kind, *shape, tensors=()):
        """A captured chunk is valid while EVERY address it baked is: the parameter store, the packed Wh, the engine's workspace and
        each persistent buffer of the round (`tensors`: a buffer re-allocated by a call of another shape gets a new address, and a
        graph that still holds the old one must never be replayed)."""
        e = self.e
        return ((kind,) + tuple(shape) + (e.store.p.data_ptr(), P(self._whp) if self._whp is not None else 0, P(e.ws) if e.ws is not None else 0, e.gemm_flags)
                + tuple(P(t) if t is not None else 0 for t in tensors))

    def _capture(self, key, fn):
        """hipGraph of fn() (launches on the current stream only, no allocations, no host reads).  Returns None when graphs are off
        (VC_DECODE_GRAPH=0: A/B runs)."""
        if os.environ.get("VC_DECODE_GRAPH", "1") == "0":
            return None
        g = self._graphs.get(key)
        if g is None:
            if len(self._graphs) > 16:
                self._graphs.clear()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # no cyclic garbage collection inside the capture: a collected object that owns device memory or a graph (a generator in a
            # reference cycle, say) would free it in the middle of the capture, which the runtime answers with an abort
            gc_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g):
                    fn()
            finally:
                if gc_on:
                    gc.enable()
            self._graphs[key] = g
        return g

    @staticmethod
    def _chunk_rounds(check_every):
        """rounds per captured chunk: check_every when it is even (the ping-ponged state then ends where it started), else 4"""
        return int(check_every) if check_every and check_every % 2 == 0 else 4

    def _round_state(self, tag, M, c0, h0):
        """What step() needs for rounds over M rows that ping-pong the decoder state between two _round_bufs sets: the state before round 0
        (c0, h0) lives in set B; round r reads set (B, A, B, ...) and writes the other.  Re-packs Wh (the weights may have been trained
        since the last call).  Returns (sets, tensors): sets(r) = round r's (source, destination); tensors = what a captured round bakes."""
        A, Bb = self._round_bufs(tag + "A_", M), self._round_bufs(tag + "B_", M)
        Bb["c2"].copy_(c0); Bb["h2"].copy_(h0)
        self._pack_wh(M)
        return (lambda r: (Bb, A) if r % 2 == 0 else (A, Bb)), [self._ones_for(M)] + list(A.values()) + list(Bb.values())

    def _run_chunks(self, kind_key, baked, one, reset, K, max_len, check_every, pending, after=lambda steps, k: None):
        """The round loop of greedy() and diverse(): up to max_len rounds one(r, timed), r = the round's index in its chunk, as replays of
        ONE hipGraph of K rounds while a whole chunk fits and eagerly for the ragged rest (VC_DECODE_GRAPH=0: throughout).  after(steps, k)
        follows every chunk of k rounds; then, with check_every, the 4-byte read of `pending`: 0 once every row has ended.  The first call
        of a key (kind_key + the addresses of `baked`, the packed Wh and the workspace) runs round 0 eagerly, since that may grow the
        workspace: reset(), which restores what round 0 starts from, undoes it and the key is taken again.  Returns the rounds run."""
        key = self._graph_key(*kind_key, tensors=baked)
        reset()
        if key not in self._graphs:
            one(0, True)
            reset()
            key = self._graph_key(*kind_key, tensors=baked)
        graph = self._capture(key, lambda: [one(r, False) for r in range(K)])
        steps = 0
        while steps < max_len:
            k = min(K, max_len - steps)
            if graph is not None and k == K:
                graph.replay()
            else:
                for r in range(k):
                    one(r, True)
            after(steps, k)
            steps += k
            if steps < max_len and check_every and pending.item() == 0:
                break
        return steps

    # ------------------------------------------------------------------ decoding controls
    def _controls_table(self, tag, ctl):
        """The banned words of THIS call in the persistent buffer the rounds of `tag` read (a captured chunk bakes its address and the
        number of words, not the words: it serves another list of the same length)."""
        table = self._b(tag + "banned", (MAX_BANNED,), torch.int32)
        if ctl.banned.size:
            table[:ctl.banned.size].copy_(torch.from_numpy(ctl.banned), non_blocking=True)
        return table

    def _apply_controls(self, ctl, table, logits, rows, hist, hist_ld, skip, lens, done, eos):
        """One vc_decode_controls_f32 launch on a round's logits [rows, V], in place, between the logits product and the round's pick /
        softmax / top-k.  hist [rows, hist_ld] / lens / done: the rows' histories (skip = 1: position 0 is <BOS>)."""
        n = int(ctl.banned.size)
        self.lib.vc_decode_controls_f32(_stream(), P(logits), rows, self.e.V, self.e.V, P(hist), hist_ld, hist_ld, skip, P(lens),
                                        P(done) if done is not None else None, ctl.no_repeat_ngram, ctl.min_len, int(eos),
                                        ctl.repetition_penalty, P(table) if n else None, n)

    def _candidates(self, tag, rows, max_len):
        """The candidate a round's pick keeps per row (the history the controls read) in persistent buffers: seq [rows, max_len], len, ended
        [rows] int32, logprob [rows] float64.  (diverse() keeps the same four inside its result buffers.)"""
        i32 = torch.int32
        return types.SimpleNamespace(seq=self._b(tag + "seq", (rows, max_len), i32), len=self._b(tag + "len", (rows,), i32),
                                     ended=self._b(tag + "ended", (rows,), i32), logprob=self._b(tag + "lp", (rows,), torch.float64))

    def _pick(self, logits, rows, cand, tok, eos, temp=1.0, u=None, u_ld=1, rnd=None, top_k=0, top_p=1.0, typical_p=1.0, min_p=0.0, eta=0.0):
        """A round's pick from its logits [rows, V] into tok and the rows' candidates: the argmax (u None) or the inverse-CDF draw at u
        [.., u_ld] (row `rnd` of it, a device counter, or row 0) from softmax(logits / temp), truncated to top_k / top_p or cut by
        typical_p / min_p / eta when asked (one family: check_typical)."""
        V, c = self.e.V, cand
        if typical_p != 1.0 or min_p != 0.0 or eta != 0.0:
            self.lib.vc_decode_pick_typical_f32(_stream(), P(logits), rows, V, V, temp, typical_p, min_p, eta, P(u), u_ld, P(rnd), int(eos), P(tok),
                                                P(c.ended), P(c.seq), c.seq.shape[1], P(c.len), P(c.logprob), None, None)
        elif top_k != 0 or top_p != 1.0:
            self.lib.vc_decode_pick_trunc_f32(_stream(), P(logits), rows, V, V, temp, top_k, top_p, P(u), u_ld, P(rnd), int(eos), P(tok), P(c.ended),
                                              P(c.seq), c.seq.shape[1], P(c.len), P(c.logprob), None)
        else:
            self.lib.vc_decode_pick_f32(_stream(), P(logits), rows, V, V, temp, P(u), u_ld, P(rnd), int(eos), P(tok), P(c.ended), P(c.seq), c.seq.shape[1],
                                        P(c.len), P(c.logprob))

    def _greedy_controls(self, ctl, features, c_v, eps, bos, eos, max_len, check_every):
        """greedy() under decoding controls: the rounds keep a candidate per row, which is the history the controls read, and pick with
        vc_decode_pick_f32 (argmax) -- still hipGraph chunks of check_every rounds."""
        lib = self.lib
        c0, h0 = self.init_state(features, c_v, eps)
        B = int(c0.shape[0])
        tag = "gc%d_%d_" % (B, max_len)
        cand = self._candidates(tag, B, max_len)
        tok, pending = self._b(tag + "tok", (B,), torch.int32), self._b(tag + "pending", (1,))
        table = self._controls_table(tag, ctl)
        sets, state = self._round_state(tag, B, c0, h0)

        def reset():
            tok.fill_(bos); cand.ended.zero_(); cand.len.zero_(); cand.logprob.zero_()

        def one(r, timed):
            src, dst = sets(r)
            logits, _, _ = self.step(tok, src["c2"], src["h2"], want="logits", bufs=dst, timed=timed)
            self._apply_controls(ctl, table, logits, B, cand.seq, max_len, 0, cand.len, cand.ended, eos)
            self._pick(logits, B, cand, tok, eos)
            lib.vc_decode_round_end_i32(_stream(), P(cand.ended), B, P(pending), None)

        K = self._chunk_rounds(check_every)
        self._run_chunks(("greedy_controls", B, K, max_len, int(eos)) + ctl.key(), [cand.seq, cand.len, cand.ended, tok, cand.logprob, pending, table] + state,
                         one, reset, K, max_len, check_every, pending)
        rows, lens = cand.seq.cpu().numpy(), cand.len.cpu().numpy()
        return [rows[b, :lens[b]].tolist() for b in range(B)]

    # ------------------------------------------------------------------ greedy (online_inference)
    def _trim(self, ids, eos):
        """[steps, B] token ids -> per image the tokens up to and including its first <EOS>."""
        ids = ids.cpu().numpy()
        out = []
        for b in range(ids.shape[1]):
            col = ids[:, b].tolist()
            out.append(col[:col.index(eos) + 1] if eos in col else col)
        return out

    def greedy(self, features, c_v=None, eps=None, bos=1, eos=2, max_len=None, check_every=4, controls=None):
        """decoder.py:145-201 with sample_gen='greedy' for a batch of images: returns the list
        of generated token-id lists (each ends with <EOS> unless max_len was hit).  Tokens stay on the
        device; the host only asks "has every image emitted <EOS>?" every `check_every` steps (4 bytes, vc_eos_track_i32).
        Rounds run as hipGraph replays of `check_every` decoder steps each (embedding gather, input projection, LSTM step, logits,
        argmax, stop-word tracking: six launches per step otherwise); VC_DECODE_GRAPH=0 keeps the eager loop -- same kernels, same ids.
        controls: a controls.DecodeControls (no repeated n-gram, minimum length, repetition penalty, banned words; DESIGN.md "Decoding
        controls"): every round's logits are processed from the row's words so far before the argmax.  None or a no-op value: this path."""
        lib, e = self.lib, self.e
        max_len = max_len or self.p.gen_max_len
        ctl = self._checked_controls(controls, eos, max_len)
        if ctl is not None:
            return self._greedy_controls(ctl, features, c_v, eps, bos, eos, int(max_len), check_every)
        c0, h0 = self.init_state(features, c_v, eps)
        B, V = c0.shape[0], e.V
        K = self._chunk_rounds(check_every)
        ids = torch.zeros((max_len, B), dtype=torch.int32, device=e.dev)
        chunk = self._b("g_chunk", (K + 1, B), torch.int32)    # row 0: the token fed to the chunk's first step; rows 1..K: its outputs
        done, pending = self._b("g_done", (B,), torch.int32), self._b("g_pending", (1,))
        sets, state = self._round_state("g", B, c0, h0)
        chunk.zero_(); chunk[0].fill_(bos)

        def one(r, timed):
            src, dst = sets(r)
            logits, _, _ = self.step(chunk[r], src["c2"], src["h2"], want="logits", bufs=dst, timed=timed)  # argmax(softmax**(1/t)/sum) == argmax(logits)
            lib.vc_argmax_rows_f32(_stream(), P(logits), B, V, V, P(chunk[r + 1]))
            lib.vc_eos_track_i32(_stream(), P(chunk[r + 1]), B, int(eos), P(done), P(pending))

        def keep(steps, k):   # the chunk's k tokens; its last one feeds the next chunk (a ragged chunk is the last: nothing follows it)
            ids[steps:steps + k].copy_(chunk[1:k + 1])
            if steps + k < max_len:
                chunk[0].copy_(chunk[k])

        steps = self._run_chunks(("greedy", B, K, int(eos)), [chunk, done, pending] + state, one, done.zero_, K, max_len, check_every, pending, keep)
        return self._trim(ids[:steps], eos)

    def sample(self, features, c_v=None, eps=None, bos=1, eos=2, max_len=None, uniforms=None, check_every=4, top_k=0, top_p=1.0,
               controls=None, typical_p=1.0, min_p=0.0, eta=0.0):
        """decoder.py:145-201 with sample_gen='sample': tokens drawn from softmax(logits / temperature)
        (tf.multinomial).  uniforms [max_len, B] in [0,1) may be injected; otherwise Philox.
        top_k > 0 / top_p < 1: the draw is truncated to the top_k best words and / or the smallest set of best words holding a share
        top_p of the probability (vc_decode_pick_trunc_f32; DESIGN.md "Truncated sampling"); the defaults leave it as it is.
        typical_p < 1 / min_p > 0 / eta > 0: the draw is cut to the words whose surprisal is closest to the row's entropy (the smallest such
        set holding a share typical_p) and / or to the words with p >= max(min_p * p_max, min(eta, sqrt(eta) * exp(-entropy)))
        (vc_decode_pick_typical_f32; DESIGN.md "Typical / min-p / eta sampling"); not together with top_k / top_p.
        controls: a controls.DecodeControls; the draw is from the softmax of the processed logits (then truncated, if asked).  The
        rows' candidates are then always kept, and an untruncated draw is vc_decode_pick_f32's (vc_multinomial_rows_f32's token)."""
        top_k, top_p = check_truncation(top_k, top_p)
        typical_p, min_p, eta = check_typical(typical_p, min_p, eta, "sample", top_k, top_p)
        max_len = max_len or self.p.gen_max_len
        ctl = self._checked_controls(controls, eos, max_len)
        c, h = self.init_state(features, c_v, eps)
        B = c.shape[0]
        tok = torch.full((B,), bos, dtype=torch.int32, device=self.e.dev)
        ids = torch.zeros((max_len, B), dtype=torch.int32, device=self.e.dev)
        u = torch.empty((B,), dtype=torch.float32, device=self.e.dev)
        ud = self._dev(uniforms, np.float32) if uniforms is not None else None
        steps = 0
        trunc = top_k != 0 or top_p != 1.0 or typical_p != 1.0 or min_p != 0.0 or eta != 0.0
        if trunc or ctl is not None:   # the pick keeps a candidate per row: scratch here, the ids are what sample() returns
            cand = self._candidates("st_", B, max_len)
            cand.ended.zero_(); cand.len.zero_(); cand.logprob.zero_()
            table = self._controls_table("st_", ctl) if ctl is not None else None
        for it in range(max_len):
            logits, c, h = self.step(tok, c, h, want="logits")
            if ctl is not None:
                self._apply_controls(ctl, table, logits, B, cand.seq, max_len, 0, cand.len, cand.ended, eos)
            if ud is not None:
                u = ud[it]
            else:
                self.lib.vc_philox_uniform_f32(_stream(), P(u), B, self.e.seed * 1000003 + 29, (16 + it) << 32, P(self.e.step))
            tok = ids[it]
            if trunc or ctl is not None:
                self._pick(logits, B, cand, tok, eos, float(self.p.temperature), u, 1, None, top_k, top_p, typical_p, min_p, eta)
            else:
                self.lib.vc_multinomial_rows_f32(_stream(), P(logits), B, self.e.V, self.e.V, float(self.p.temperature), P(u), P(tok))
            steps = it + 1
            if check_every and steps % check_every == 0 and bool((ids[:steps] == eos).any(0).all().item()):
                break
        return self._trim(ids[:steps], eos)

    # ------------------------------------------------------------------ diverse captioning (K latent draws per image)
    def _diverse_init(self, features, c_v, eps, K):
        """The decoder state of B images x K latent draws ([B*K, H], rows b*K + k), as init_state(features[b:b+1], c_v[b:b+1],
        eps[k][:, None]) would give it: imf_emb, cv_emb and the LSTM steps before the z step run on the B image rows; their state is
        tiled to B*K rows and only the draws (vc_diverse_latent_f32: no [rows*S, L] mean / std tensors), the z_rnn product and the z
        step run on B*K rows.  eps: [K, S, B, L] or None (Philox on device).  One hipGraph from the second call of a shape on."""
        e, p, lib = self.e, self.p, self.lib
        B = int(features.shape[0])
        M = B * K
        Hd, L, Sm = p.decoder_hidden, p.latent_size, p.gen_z_samples
        n_pre = e.n_init_d - int(e.enc)   # steps that depend on the image only
        tag = "dvi%d_%d_" % (B, K)
        im = self._image_rows(tag, n_pre, features, c_v, M)
        pmd, cs0, hs0 = im.pmd, im.cs, im.hs
        zs = self._z_step(tag, M)
        cs1, hs1, epsd = zs.cs1, zs.hs1, None
        if e.enc and eps is not None:
            epsd = self._load(self._b(tag + "eps", (M, Sm, L)), np.transpose(np.asarray(eps, np.float32), (2, 0, 1, 3)))   # [K, S, B, L] -> rows b*K + k

        def launches(timed):
            st, tg = _stream(), ("gemm" if timed else None)
            im.embed(tg)
            im.lstm(st)
            dst = (cs1[0], hs1[0]) if e.enc else (cs1[1], hs1[1])
            lib.vc_tile_rows_f32(st, P(cs0[n_pre]), B, K, Hd, P(dst[0]))
            lib.vc_tile_rows_f32(st, P(hs0[n_pre]), B, K, Hd, P(dst[1]))
            if e.enc:   # decoder.py:72-74 and 111, per draw
                lib.vc_diverse_latent_f32(st, M, K, Sm, L, P(pmd), float(p.std), P(epsd), e.seed * 1000003 + 17, 6 << 32, P(e.step), P(zs.z))
                zs.run(st, tg)

        key = self._graph_key("dvinit", B, K, eps is None, pmd is not None, float(p.std), e.lstm_flags, e.seed,
                              tensors=[im.feats, im.X, im.cv, epsd, zs.z, zs.Xz, pmd, im.act, zs.act1, cs0, hs0, cs1, hs1, im.lens, zs.ones])
        self._replay_or_capture(key, launches)
        return cs1[1], hs1[1]

    def _diverse_pass(self, features, c_v, eps, K, method, bos, eos, max_len, len_norm_f, n_best, uniforms, check_every, rerank="likelihood",
                      top_k=0, top_p=1.0, ctl=None, typical_p=1.0, min_p=0.0, eta=0.0):
        """One pass of diverse(): the B*K candidate rows of B images decoded together, ranked per image on device (vc_diverse_rank),
        results in two flat buffers brought back by two copies into pinned memory."""
        lib, e, p = self.lib, self.e, self.p
        c0, h0 = self._diverse_init(features, c_v, eps, K)
        M = int(c0.shape[0])
        B = M // K
        i32 = torch.int32
        tag = "dv%d_%d_%d_" % (B, K, max_len)
        lay, dlay = FieldLayout(diverse_fields(B, K, max_len)), FieldLayout([("score", M), ("logprob", M)])
        ibuf, dbuf = self._b(tag + "ibuf", (lay.total,), i32), self._b(tag + "dbuf", (dlay.total,), torch.float64)
        f, (score, logprob) = lay.views(ibuf), dlay.views(dbuf).values()
        cand = types.SimpleNamespace(seq=f["seq"].view(M, max_len), len=f["len"], ended=f["ended"], logprob=logprob)
        tok, rnd, pending = self._b(tag + "tok", (M,), i32), self._b(tag + "round", (1,), i32), self._b(tag + "pending", (1,))
        ud = None
        if method == "sample":
            ud = self._b(tag + "u", (max_len, M))
            if uniforms is not None:
                self._load(ud, np.transpose(np.asarray(uniforms, np.float32), (1, 2, 0)))   # [K, T, B] -> [T, rows b*K + k]
            else:
                lib.vc_philox_uniform_f32(_stream(), P(ud), ud.numel(), e.seed * 1000003 + 29, 7 << 32, P(e.step))
        temp = float(p.temperature) if method == "sample" else 1.0
        table = self._controls_table(tag, ctl) if ctl is not None else None

        def reset():
            tok.fill_(bos); cand.ended.zero_(); cand.len.zero_(); cand.logprob.zero_(); rnd.zero_()

        sets, state = self._round_state(tag, M, c0, h0)

        def one(r, timed):
            src, dst = sets(r)
            logits, _, _ = self.step(tok, src["c2"], src["h2"], want="logits", bufs=dst, timed=timed)
            if ctl is not None:   # the candidates so far are the histories
                self._apply_controls(ctl, table, logits, M, cand.seq, max_len, 0, cand.len, cand.ended, eos)
            self._pick(logits, M, cand, tok, eos, temp, ud, max_len, rnd, top_k, top_p, typical_p, min_p, eta)
            lib.vc_decode_round_end_i32(_stream(), P(cand.ended), M, P(pending), P(rnd))

        Kc = self._chunk_rounds(check_every)
        cuts = (typical_p, min_p, eta)
        self._run_chunks(("diverse", B, K, Kc, max_len, int(eos), method, temp, top_k, top_p) + (("typical",) + cuts if cuts != (1.0, 0.0, 0.0) else ())
                         + (ctl.key() if ctl is not None else ()),   # (a captured chunk bakes the truncation, the cuts and the controls)
                         [tok, rnd, pending, ibuf, dbuf, ud] + ([table] if ctl is not None else []) + state, one, reset, Kc, max_len, check_every, pending)
        lib.vc_diverse_rank(_stream(), M, B, K, max_len, P(cand.seq), P(cand.len), P(cand.ended), P(logprob), float(len_norm_f),
                            P(f["n_distinct"]), P(f["rep"]), P(f["count"]), P(score))
        res, cands = diverse_from_host(*self._to_host(tag, ibuf, dbuf), lay.off, B, K, max_len, n_best if rerank != "marginal" else None, candidates=True)
        if rerank != "marginal":
            return res, cands
        # re-score every distinct caption under ALL K draws of the pass: their initial states are still in _diverse_init's buffers
        caps = [[list(t) for t, _, _ in r] for r in res]
        self._t_score = _phase("", 0.0)
        _, marg = self._score_states(c0, h0, K, caps, bos)
        out, o = [], 0
        for b in range(B):
            out.append(rerank_by_marginal(res[b], marg[o:o + len(res[b])].tolist(), eos, len_norm_f)[:n_best])
            o += len(res[b])
        return out, cands

    # ------------------------------------------------------------------ scoring given captions
    def _score_states(self, c0, h0, K, caps, bos):
        """Teacher-forced log-likelihood of caps[b] (token lists without <BOS>) under the K draws of image b whose decoder states are rows
        b*K + k of c0 / h0 [B*K, H]: (logprob float64 [C, K], marginal float64 [C]) over the C captions in image order.  Sequence rows are
        caption-major, draw-minor; one upload of the indices, one copy of the results into pinned memory."""
        C = sum(len(cl) for cl in caps)
        tf = self._teacher_force(c0, h0, K, caps, bos)
        if tf is None:
            return np.zeros((C, K), np.float64), np.zeros((C,), np.float64)
        dlay = FieldLayout([("logprob", C * K), ("marginal", C)])
        dbuf = self._b(tf.tag + "dbuf", (dlay.total,), torch.float64)
        logprob, marginal = dlay.views(dbuf).values()
        self.lib.vc_score_reduce_f64(_stream(), P(tf.lp), tf.T, C, K, P(tf.clen), P(logprob), P(marginal))
        logprob, marginal = dlay.views(self._to_host(tf.tag, None, dbuf)[1].copy()).values()
        self._t_score = _phase("score: reduce + copy-back", tf.t_ph)
        return logprob.reshape(C, K), marginal

    def _teacher_force(self, c0, h0, K, caps, bos, own_rows=False):
        """The device half of _score_states: every caption of caps[b] teacher-forced from <BOS> under K draws, the tokens' log-softmax terms
        left in lp [T, C*K] (time-major, f32; rows caption-major, draw-minor).  Row c*K + k starts from row b*K + k of c0 / h0 [B*K, H], the
        state of draw k of the caption's IMAGE, or with own_rows from row c*K + k of c0 / h0 [C*K, H], a state of its own (bound(): the
        posterior draws belong to the caption).  Returns lp, T, clen [C] (device) and the buffers' tag; None when there is nothing to score."""
        e, p, lib, S = self.e, self.p, self.lib, self.e.store
        E, Hd, V = p.embed_size, p.decoder_hidden, e.V
        flat = [(b, t) for b, cl in enumerate(caps) for t in cl]
        C = len(flat)
        T = max([len(t) for _, t in flat] + [0])
        if C == 0 or T == 0:
            return None
        N = C * K
        i32 = torch.int32
        # int32 upload: parent row, row lengths, caption lengths, step inputs [T, N], labels [T, N]
        lay = FieldLayout([("parent", N), ("len", N), ("clen", C), ("tok_in", T * N), ("label", T * N)])
        host = np.zeros(lay.total, np.int32)
        h_parent, h_len, h_clen, h_in, h_lab = lay.views(host).values()
        toks_in, labels = np.zeros((T, C), np.int32), np.full((T, C), -1, np.int32)
        for c, (b, t) in enumerate(flat):
            n = len(t)
            h_parent[c * K:(c + 1) * K] = (c if own_rows else b) * K + np.arange(K)
            h_clen[c] = n
            if n:
                labels[:n, c] = t
                toks_in[0, c] = bos
                toks_in[1:n, c] = t[:n - 1]
        h_len[:] = np.repeat(h_clen, K)
        h_in[:] = np.repeat(toks_in, K, axis=1).ravel()
        h_lab[:] = np.repeat(labels, K, axis=1).ravel()
        tag = "sc%d_%d_%d_" % (C, K, T)
        idx = self._b(tag + "idx", (host.size,), i32)
        idx.copy_(torch.from_numpy(host), non_blocking=False)
        parent, lens, clen, tin, lab = lay.views(idx).values()
        X, act = self._b("sc_X", (T, N, E)), self._b("sc_act", (T, N, 4 * Hd))
        cs, hs = self._b("sc_cs", (T + 1, N, Hd)), self._b("sc_hs", (T + 1, N, Hd))
        lp = self._b("sc_lp", (T * N,))
        st = _stream()
        t_ph = _phase("score: init chain", self._t_score)
        lib.vc_beam_gather_f32(st, P(c0), P(h0), P(parent), N, Hd, P(cs[0]), P(hs[0]), None, None, V, 4 * Hd, None)
        lib.vc_embedding_gather_f32(st, P(S.param("decoder/net/dec_embeddings")), P(tin), T * N, E, V, P(X))
        for nb in (lib.vc_lstm_seq_workspace_bytes(T, N, E, Hd), lib.vc_gemm_workspace_bytes(T * N, 4 * Hd, E),
                   lib.vc_logits_logprob_workspace_bytes(T * N, V, Hd)):
            e._need_ws(nb)
        lib.vc_lstm_seq_fwd_f32(st, T, N, E, Hd, P(X), P(S.param(spec.DEC_CELL + "kernel")), P(S.param(spec.DEC_CELL + "bias")), P(lens),
                                P(act), P(cs), P(hs), P(e.ws), e.ws_bytes, e.lstm_flags)
        t_ph = _phase("score: sequence", t_ph)
        # (the f32 products on a bf16x3 engine too; the [T*N, V] logits are never written)
        lib.vc_logits_logprob_f32(st, T * N, V, Hd, P(hs[1]), Hd, P(S.param("decoder/rnn_logits/kernel")), e.Vp,
                                  P(S.param("decoder/rnn_logits/bias")), P(lab), P(lp), P(e.ws), e.ws_bytes)
        t_ph = _phase("score: logits + log-probability", t_ph)
        return types.SimpleNamespace(lp=lp, T=T, clen=clen, tag=tag, t_ph=t_ph)

    def _check_draws(self, K, eps, B, per="images"):
        """ValueError unless K latent draws are 1..DIVERSE_MAX_DRAWS and eps, when given, is [K, S, B, L] (score(), diverse(): B images;
        bound(): B captions)"""
        want = (K, self.p.gen_z_samples, B, self.p.latent_size)
        if not 1 <= K <= DIVERSE_MAX_DRAWS:
            raise ValueError("draws must be 1..%d (got %d)" % (DIVERSE_MAX_DRAWS, K))
        if eps is not None and tuple(np.shape(eps)) != want:
            raise ValueError("eps must be [draws, gen_z_samples, %s, latent_size] = %s" % (per, want))

    def score(self, features, captions, c_v=None, eps=None, bos=1, eos=2, draws=1):
        """How likely are given captions for their images: per image, per caption {"logprob": float64 [K], "marginal": float, "tokens": n}.
        captions[b]: token-id lists for image b, with or without the leading <BOS> (stripped), scored up to and including the last token
        (pass the <EOS> to have it counted, as diverse() does for ended captions); n = tokens scored (empty caption: logprob 0, n 0).
        logprob[k] = sum of the tokens' log-softmax at temperature 1 (f32 terms, f64 sum in token order) under diverse()'s draw k of the
        image: z = prior_mean + std * eps[k], state as init_state(features[b:b+1], c_v[b:b+1], eps[k][:, None]); marginal =
        log 1/K sum_k exp(logprob[k]), the model's likelihood estimate over the draws.  eps: [K, S, B, L] (Philox on device when None: those
        draws depend on how the passes are cut).  --no_encoder models have no z: every draw gives the same number.
        Passes: an image goes with all its captions and draws into one pass of <= score_rows row-steps (sequence rows x steps of its
        longest caption); an image that exceeds it alone gets a pass of its own.  ValueError: a token id outside [0, V), more than
        SCORE_MAX_TOKENS scored tokens (names image and caption), draws outside 1..DIVERSE_MAX_DRAWS, a wrong eps shape."""
        K, B = int(draws), int(features.shape[0])
        self._check_draws(K, eps, B)
        caps = self._caption_lists(captions, B, bos)
        c_v, eps = (np.asarray(a) if a is not None else None for a in (c_v, eps))
        res = []
        for g0, g1, rows, steps in self._passes(caps, K, self.score_rows):
            sl = slice(g0, g1)
            if rows * steps == 0:
                lp, marg = np.zeros((rows // K, K), np.float64), np.zeros((rows // K,), np.float64)
            else:
                self._t_score = _phase("", 0.0)
                c0, h0 = self._diverse_init(features[sl], _cut(c_v, sl), _cut(eps, sl, 2), K)
                lp, marg = self._score_states(c0, h0, K, caps[sl], bos)
            o = 0
            for b in range(g0, g1):
                res.append([{"logprob": lp[o + j].copy(), "marginal": float(marg[o + j]), "tokens": len(t)} for j, t in enumerate(caps[b])])
                o += len(caps[b])
        return res

    def _caption_lists(self, captions, B, bos, empty_ok=True):
        """captions as score() / encode() / bound() take them (per image a list of token-id lists) -> the same lists as ints without the
        leading <BOS>.  ValueError: not one list per image, more than SCORE_MAX_TOKENS tokens, a token id outside [0, V), and, unless
        empty_ok, a caption without a token (the message names image and caption)."""
        V = self.e.V
        if len(captions) != B:
            raise ValueError("captions must hold one list of captions per image (%d images, %d lists)" % (B, len(captions)))
        caps = []
        for b, cl in enumerate(captions):
            row = []
            for j, t in enumerate(cl):
                t = [int(w) for w in t]
                if t and t[0] == bos:
                    t = t[1:]
                if len(t) > SCORE_MAX_TOKENS:
                    raise ValueError("image %d caption %d: %d tokens to score, at most %d" % (b, j, len(t), SCORE_MAX_TOKENS))
                if any(w < 0 or w >= V for w in t):
                    raise ValueError("image %d caption %d: token id outside [0, %d)" % (b, j, V))
                if not t and not empty_ok:
                    raise ValueError("image %d caption %d: an empty caption has no posterior" % (b, j))
                row.append(t)
            caps.append(row)
        return caps

    @staticmethod
    def _passes(caps, K, limit):
        """The passes of score() / bound() over the images of caps: (g0, g1, rows, steps) per pass, images g0 .. g1-1 with rows = their
        captions x K sequence rows and steps = their longest caption.  Greedy cut: images are added while rows x steps <= limit; an
        image that exceeds it alone gets a pass of its own."""
        B, g0 = len(caps), 0
        while g0 < B:
            g1, rows, steps = g0, 0, 0
            while g1 < B:
                r2 = rows + len(caps[g1]) * K
                s2 = max([steps] + [len(t) for t in caps[g1]])
                if g1 > g0 and r2 * s2 > limit:
                    break
                g1, rows, steps = g1 + 1, r2, s2
            yield g0, g1, rows, steps
            g0 = g1

    # ------------------------------------------------------------------ the posterior at inference: encode(), bound()
    def _posterior_inputs(self, features, captions, c_v, gmm_idx, bos):
        """The checks encode() and bound() share (their ValueError cases) -> (caps without <BOS>, c_v as an array or None, gmm_idx as a
        flat int32 array over the captions or None)."""
        e, p = self.e, self.p
        if not e.enc:
            raise ValueError("a --no_encoder model has no posterior q(z | caption, image)")
        B = int(features.shape[0])
        caps = self._caption_lists(captions, B, bos, empty_ok=False)
        C = sum(len(cl) for cl in caps)
        if e.use_ci:
            if c_v is None or tuple(np.shape(c_v)) != (B, K_CL):
                raise ValueError("a %s model%s needs the images' cluster vectors c_v [%d, %d]" % (p.prior, " with use_c_v" if p.use_c_v else "", B, K_CL))
            c_v = np.ascontiguousarray(c_v, dtype=np.float32)
        else:
            c_v = None
        if p.prior in ("AG", "GMM"):
            for b in range(B):
                if caps[b] and not c_v[b].any():
                    raise ValueError("image %d: an all-zero cluster vector gives its captions no %s posterior (the std would be 0)" % (b, p.prior))
        if p.prior == "GMM":
            if gmm_idx is None:
                raise ValueError("a GMM model needs gmm_idx: the mixture component (0..%d) of every caption, flat in image order" % (K_CL - 1))
            g = np.asarray(gmm_idx).reshape(-1)
            if g.size != C or (C and (g.dtype.kind not in "iu" or g.min() < 0 or g.max() >= K_CL)):
                raise ValueError("gmm_idx must hold one integer in 0..%d per caption (%d captions)" % (K_CL - 1, C))
            gmm_idx = g.astype(np.int32)
        else:
            gmm_idx = None
        return caps, c_v, gmm_idx

    def _encode_pass(self, features, c_v, caps, gmm_idx):
        """q(z | caption, image) of the C captions of one pass (caps[b]: the non-empty token lists of image b): mean, std [C, L] in
        persistent device buffers, computed as CaptionEngine.fw_encode_stats does for a training row (encoder.py:24-110, no dropout).
        The image-only steps of the encoder run on the B image rows; their state is gathered to the caption rows (parent = the caption's
        image), where ONE length-masked LSTM call runs the token steps; then the heads.  Returns (mean, std, img, h_img): img [C] int32,
        the image of every caption, on the device and on the host."""
        e, p, lib, S = self.e, self.p, self.lib, self.e.store
        B, E, He, L, V = int(features.shape[0]), p.embed_size, p.encoder_hidden, p.latent_size, e.V
        flat = [(b, t) for b, cl in enumerate(caps) for t in cl]
        C, T, n_e = len(flat), max(len(t) for _, t in flat), e.n_init_e
        im = self._image_rows("bde_", n_e, features, c_v, 1, encoder=True)
        gmm, ag = p.prior == "GMM", p.prior == "AG"
        lay = FieldLayout([("img", C), ("len", C), ("gmm", C), ("tok", T * C)])
        host = np.zeros(lay.total, np.int32)
        h_img, h_len, h_gmm, h_tok = lay.views(host).values()
        toks = h_tok.reshape(T, C)
        for c, (b, t) in enumerate(flat):
            h_img[c], h_len[c] = b, len(t)
            toks[:len(t), c] = t
        if gmm:
            h_gmm[:] = gmm_idx
        idx = self._b("bdq_idx", (host.size,), torch.int32)
        idx.copy_(torch.from_numpy(host), non_blocking=False)
        img, lens, gidx, tok = lay.views(idx).values()
        X, act = self._b("bdq_X", (T, C, E)), self._b("bdq_act", (T, C, 4 * He))
        cs, hs = self._b("bdq_cs", (T + 1, C, He)), self._b("bdq_hs", (T + 1, C, He))
        mean, std = self._b("bdq_mean", (C, L)), self._b("bdq_std", (C, L))
        st = _stream()
        im.embed("gemm")
        im.lstm(st)
        lib.vc_beam_gather_f32(st, P(im.cs[n_e]), P(im.hs[n_e]), P(img), C, He, P(cs[0]), P(hs[0]), None, None, V, 4 * He, None)
        lib.vc_embedding_gather_f32(st, P(S.param("encoder/enc_embeddings")), P(tok), T * C, E, V, P(X))
        nh = L if p.prior == "Normal" else 2 * K_CL * L
        for nb in (lib.vc_lstm_seq_workspace_bytes(T, C, E, He), lib.vc_gemm_workspace_bytes(C, nh, He)):
            e._need_ws(nb)
        lib.vc_lstm_seq_fwd_f32(st, T, C, E, He, P(X), P(S.param(spec.ENC_CELL + "kernel")), P(S.param(spec.ENC_CELL + "bias")), P(lens),
                                P(act), P(cs), P(hs), P(e.ws), e.ws_bytes, e.lstm_flags)
        hT = hs[T]   # (rows shorter than T carry their last state forward)
        if p.prior == "Normal":
            logstd = self._b("bdq_logstd", (C, L))
            e.gemm(0, 0, C, L, He, hT, He, S.param("encoder/dense/kernel"), L, mean, L, S.param("encoder/dense/bias"))
            e.gemm(0, 0, C, L, He, hT, He, S.param("encoder/dense_1/kernel"), L, logstd, L, S.param("encoder/dense_1/bias"))
            lib.vc_exp_f32(st, P(logstd), C * L, P(std))
        else:
            heads = self._b("bdq_heads", (C, nh))
            e.gemm(0, 0, C, nh, He, hT, He, S.param("encoder/heads/kernel"), nh, heads, nh, S.param("encoder/heads/bias"))
            cvr = self._load(self._b("bdq_cvrows", (C, K_CL)), c_v[h_img]) if ag else None   # the c_v-weighted mix takes a row per caption
            lib.vc_heads_mix_fwd_f32(st, C, K_CL, L, P(heads), P(cvr), P(gidx) if gmm else None, P(mean), P(std))
        return mean, std, img, h_img

    def encode(self, features, captions, c_v=None, gmm_idx=None, bos=1):
        """The posterior q(z | caption, image) of given captions: per image, per caption (mean, std), float32 [L] each -- what the encoder
        of a training step computes for the row (cap_enc = the caption without <BOS>, its <EOS> included when present; no dropout).
        captions[b]: token-id lists of image b, with or without the leading <BOS> (stripped).  c_v [B, 90]: the cluster vectors of a
        model that uses them.  gmm_idx (GMM prior): the mixture component 0..89 of every caption, flat over all captions in image order
        (training draws it from the cluster vector; here the caller does).  Passes are cut by bound_rows with score()'s rule at one row
        per caption.  ValueError: a --no_encoder model; a token id outside [0, V); an empty caption; more than SCORE_MAX_TOKENS tokens;
        GMM without gmm_idx (or values outside 0..89); AG / GMM with an all-zero cluster vector for an image that has captions."""
        caps, c_v, gmm_idx = self._posterior_inputs(features, captions, c_v, gmm_idx, bos)
        res, o = [], 0
        for g0, g1, rows, _ in self._passes(caps, 1, self.bound_rows):
            if rows:
                sl = slice(g0, g1)
                mean, std, _, _ = self._encode_pass(features[sl], _cut(c_v, sl), caps[sl], _cut(gmm_idx, slice(o, o + rows)))
                mean, std = mean.cpu().numpy(), std.cpu().numpy()
            j = 0
            for b in range(g0, g1):
                res.append([(mean[j + i].copy(), std[j + i].copy()) for i in range(len(caps[b]))])
                j += len(caps[b])
            o += rows
        return res

    def _bound_pass(self, features, c_v, caps, gmm_idx, eps, K, bos, return_latents):
        """One pass of bound() over the C > 0 captions of B images: float64 host arrays logprob, logw [C, K], out [C, 5] (elbo, iwae, rec,
        kl_mc, ess) and kl [C] from ONE copy-back, plus with return_latents (mean, std [C, L], z [C, K, S, L]) as float32 host arrays.
        eps: [K, S, C, L] or None (Philox on device)."""
        e, p, lib = self.e, self.p, self.lib
        Hd, L, Sm = p.decoder_hidden, p.latent_size, p.gen_z_samples
        t_ph = _phase("", 0.0)
        mean, std, img, h_img = self._encode_pass(features, c_v, caps, gmm_idx)
        t_ph = _phase("bound: encoder", t_ph)
        C = int(mean.shape[0])
        N = C * K
        n_pre = e.n_init_d - 1   # the decoder's steps that depend on the image only
        tag = "bd_"
        im = self._image_rows(tag, n_pre, features, c_v, N)
        zs = self._z_step(tag, N)
        z, cs1, hs1, epsd = zs.z, zs.cs1, zs.hs1, None
        if eps is not None:
            epsd = self._load(self._b("bd_eps", (N, Sm, L)), np.transpose(np.asarray(eps, np.float32), (2, 0, 1, 3)))   # [K, S, C, L] -> rows c*K + k
        rowimg = self._b(tag + "rowimg", (N,), torch.int32)
        rowimg.copy_(torch.from_numpy(np.repeat(h_img, K)), non_blocking=False)   # the image whose state row c*K + k continues
        dlay = FieldLayout([("logprob", N), ("logw", N), ("out", 5 * C), ("kl", C)])
        dbuf = self._b(tag + "dbuf", (dlay.total,), torch.float64)
        logprob, logw, out, kl = dlay.views(dbuf).values()
        st = _stream()
        im.embed("gemm")
        im.lstm(st)
        lib.vc_beam_gather_f32(st, P(im.cs[n_pre]), P(im.hs[n_pre]), P(rowimg), N, Hd, P(cs1[0]), P(hs1[0]), None, None, e.V, 4 * Hd, None)
        pm_args = (P(im.pmd), P(img)) if im.pmd is not None else (None, None)
        lib.vc_posterior_latent_f32(st, N, K, Sm, L, P(mean), P(std), pm_args[0], pm_args[1], float(p.std), P(epsd), e.seed * 1000003 + 17,
                                    8 << 32, P(e.step), P(z), P(logw))
        zs.run(st, "gemm")
        self._t_score = _phase("bound: posterior draws, z step", t_ph)
        tf = self._teacher_force(cs1[1], hs1[1], K, caps, bos, own_rows=True)
        lib.vc_bound_reduce_f64(st, P(tf.lp), tf.T, C, K, P(tf.clen), P(logw), P(logprob), P(out))
        lib.vc_gauss_kl_rows_f64(st, C, Sm, L, P(mean), P(std), pm_args[0], pm_args[1], float(p.std), P(kl))
        h = dlay.views(self._to_host(tag, None, dbuf)[1].copy())
        self._t_score = _phase("bound: reduce + copy-back", tf.t_ph)
        lat = None
        if return_latents:
            lat = (mean.cpu().numpy(), std.cpu().numpy(), z.cpu().numpy().reshape(C, K, Sm, L) if return_latents != "stats" else None)
        return h["logprob"].reshape(C, K), h["logw"].reshape(C, K), h["out"].reshape(C, 5), h["kl"], lat

    def bound(self, features, captions, c_v=None, eps=None, gmm_idx=None, bos=1, eos=2, draws=1, return_latents=False):
        """Variational bounds on log p(caption | image) with the model's own posterior as proposal (DESIGN.md "Bounds"): per image, per
        caption a dict of tokens (n scored, as score() counts them), elbo, iwae, rec, kl, kl_mc, ess (floats), logprob and logw (float64
        [K]); with return_latents also mean, std (float32 [L]) and z (float32 [K, S, L]; return_latents="stats": mean and std only).
        Draw k of a caption is z_k = mean + std * eps_k with (mean, std) = encode()'s posterior; its decoder state is init_state's with
        z_k in place of the prior draw.  logprob[k] = log p(caption | z_k, image) exactly as score() defines it; logw[k] = log p(z_k |
        image) - log q(z_k | caption, image) against the generation-time prior N(prior_mean, params.std^2) that score() and diverse()
        draw from (float64, from the f32 z, eps, std).  With a_k = logprob[k] + logw[k]: elbo = mean_k a_k; iwae = log 1/K sum_k
        exp(a_k) (Burda et al. 2016; iwae >= elbo, equal at K = 1); rec = mean_k logprob[k]; kl_mc = -mean_k logw[k]; kl = KL(q || p) in
        closed form; ess = (sum_k v_k)^2 / sum_k v_k^2 of the importance weights v_k = exp(a_k - max a), in [1, K].
        eps: [K, S, C, L] over all C captions in image order (Philox on device when None: those draws depend on how the passes are
        cut).  Passes: score()'s rule on bound_rows row-steps.  ValueError: encode()'s cases, draws outside 1..DIVERSE_MAX_DRAWS, a
        wrong eps shape."""
        K = int(draws)
        caps, c_v, gmm_idx = self._posterior_inputs(features, captions, c_v, gmm_idx, bos)
        C = sum(len(cl) for cl in caps)
        self._check_draws(K, eps, C, per="captions")
        eps = np.asarray(eps) if eps is not None else None
        res, o = [], 0
        for g0, g1, rows, _ in self._passes(caps, K, self.bound_rows):
            n = rows // K
            if n:
                sl = slice(g0, g1)
                own = slice(o, o + n)   # (gmm_idx and eps are per caption)
                lp, lw, out, kl, lat = self._bound_pass(features[sl], _cut(c_v, sl), caps[sl], _cut(gmm_idx, own), _cut(eps, own, 2), K, bos, return_latents)
            j = 0
            for b in range(g0, g1):
                recs = []
                for t in caps[b]:
                    r = {"tokens": len(t), "elbo": float(out[j, 0]), "iwae": float(out[j, 1]), "rec": float(out[j, 2]), "kl": float(kl[j]),
                         "kl_mc": float(out[j, 3]), "ess": float(out[j, 4]), "logprob": lp[j].copy(), "logw": lw[j].copy()}
                    if return_latents:
                        r.update(mean=lat[0][j].copy(), std=lat[1][j].copy())
                        if lat[2] is not None:
                            r["z"] = lat[2][j].copy()
                    recs.append(r)
                    j += 1
                res.append(recs)
            o += n
        return res

    def diverse(self, features, c_v=None, eps=None, bos=1, eos=2, draws=20, method="greedy", n_best=None, max_len=None, len_norm_f=0.7,
                uniforms=None, check_every=4, rerank="likelihood", top_k=0, top_p=1.0, controls=None, typical_p=1.0, min_p=0.0, eta=0.0):
        """Diverse captioning (the AG-CVAE paper's purpose of z): per image `draws` = K independent latent draws, each decoded with
        `greedy` (argmax) or `sample` (inverse CDF at params.temperature) up to and including its first <EOS> (at most max_len tokens),
        log-likelihood = sum of the emitted tokens' log-softmax at temperature 1 (f32 terms, f64 sum), score = logprob / (1 + n)**len_norm_f
        (the 1 counts <BOS>, decoder.py:285-286).  Candidates with identical tokens are merged (best score and its draw kept, ties: lower
        draw; count = draws that produced it); <EOS>-ended captions rank before captions cut at max_len (decoder.py:296-299), then score
        descending, then lower draw.  Returns per image the first n_best (None: all) entries (tokens, score, count).
        eps: [K, S, B, L] N(0,1) draws (Philox on device when None); uniforms: [K, max_len, B] in [0, 1) for method="sample" (draw k
        consumes uniforms[k] as sample(..., uniforms=uniforms[k]) does; Philox when None).  Rounds replay as hipGraph chunks of
        check_every rounds with a 4-byte "all ended" read between chunks; VC_DECODE_GRAPH=0 keeps the eager loop (same outputs).  Images
        are decoded in passes of <= diverse_rows candidate rows, every image with all of its draws in one pass.
        self.last_candidates: per image the K candidates (tokens, logprob, ended) in draw order.
        rerank="marginal": every distinct caption of an image is re-scored under ALL K draws of its pass (score()'s marginal
        log 1/K sum_k p(caption | z_k, image), nothing drawn again) and the entries are ordered by marginal / (1 + n)**len_norm_f:
        <EOS>-ended first, then that score descending, exact ties in the likelihood order; entries become (tokens, score, count, marginal)
        with `score` the new one.  n_best cuts after the re-ranking.  "likelihood" (default) is the order described above.
        top_k > 0 / top_p < 1 (method="sample" only): every draw's tokens come from the truncated distribution (the top_k best words and /
        or the smallest set of best words holding a share top_p of the probability; DESIGN.md "Truncated sampling"); log-likelihoods stay
        the model's, over the full vocabulary, so score() of a candidate under its own draw still returns its logprob.
        typical_p < 1 / min_p > 0 / eta > 0 (method="sample" only, not with top_k / top_p): every draw's tokens come from the words closest
        in surprisal to the round's entropy and / or above the min-p / eta floor (DESIGN.md "Typical / min-p / eta sampling"); the
        log-likelihoods stay the model's in the same way.
        controls: a controls.DecodeControls; every draw is decoded from the softmax of its PROCESSED logits and `logprob` is taken
        under it (DESIGN.md "Decoding controls": a penalty has no "model's own" reading); rerank="marginal" still re-scores under the
        unprocessed model.  None or a no-op value: the launches and graph keys of a call without the keyword."""
        K, B = int(draws), int(features.shape[0])
        self._check_draws(K, eps, B)
        if method not in ("greedy", "sample"):
            raise ValueError("method must be 'greedy' or 'sample' (got %r)" % (method,))
        if rerank not in ("likelihood", "marginal"):
            raise ValueError("rerank must be 'likelihood' or 'marginal' (got %r)" % (rerank,))
        top_k, top_p = check_truncation(top_k, top_p, method)
        typical_p, min_p, eta = check_typical(typical_p, min_p, eta, method, top_k, top_p)
        max_len = int(max_len or self.p.gen_max_len)
        ctl = self._checked_controls(controls, eos, max_len)
        if uniforms is not None and tuple(np.shape(uniforms)) != (K, max_len, B):
            raise ValueError("uniforms must be [draws, max_len, images] = %s" % ((K, max_len, B),))
        c_v, eps, uniforms = (np.asarray(a) if a is not None else None for a in (c_v, eps, uniforms))
        res, cands = [], []
        for sl in self._marginal_passes(B, K):
            r, c = self._diverse_pass(features[sl], _cut(c_v, sl), _cut(eps, sl, 2), K, method, bos, eos, max_len, len_norm_f, n_best,
                                      _cut(uniforms, sl, 2), check_every, rerank, top_k, top_p, ctl, typical_p, min_p, eta)
            res += r
            cands += c
        self.last_candidates = cands
        return res

    # ------------------------------------------------------------------ marginal decoding (search under the K-draw mixture)
    def _mixture_ws(self, tag, G, kc):
        """vc_mixture_topk_f32's workspace for G groups of kc words, a persistent buffer of the pass (a captured round bakes it)"""
        nbytes = int(self.lib.vc_mixture_topk_workspace_bytes(G, self.e.V, kc))
        return self._b(tag + "mixws", (nbytes // 4,), torch.int32), nbytes

    def _marginal_passes(self, B, rows_per_image):
        """The passes of diverse() and of marginal decoding: slices of images whose rows together stay within diverse_rows; an image that
        exceeds the cap alone gets a pass of its own"""
        G = max(1, self.diverse_rows // rows_per_image)
        return [slice(g0, min(B, g0 + G)) for g0 in range(0, B, G)]

    def _marginal_greedy_pass(self, features, c_v, eps, K, bos, eos, max_len, check_every):
        """One pass of marginal_greedy(): the B*K rows of B images decoded together, one hypothesis group per image."""
        lib, e = self.lib, self.e
        c0, h0 = self._diverse_init(features, c_v, eps, K)
        M, V = int(c0.shape[0]), e.V
        B = M // K
        i32 = torch.int32
        tag = "mg%d_%d_%d_" % (B, K, max_len)
        lay, dlay = FieldLayout([("done", B), ("len", B), ("seq", B * max_len)]), FieldLayout([("logw0", M), ("logw1", M)])
        ibuf, dbuf = self._b(tag + "ibuf", (lay.total,), i32), self._b(tag + "dbuf", (dlay.total,), torch.float64)
        f, logw = lay.views(ibuf), list(dlay.views(dbuf).values())
        tok_rows, tok, tv = self._b(tag + "tok_rows", (M,), i32), self._b(tag + "tok", (B,), i32), self._b(tag + "tv", (B,))
        stat, pending = self._b(tag + "stat", (M, 2)), self._b(tag + "pending", (1,))
        ws, ws_bytes = self._mixture_ws(tag, B, 1)

        def reset():
            tok_rows.fill_(bos); ibuf.zero_(); dbuf.zero_()

        sets, state = self._round_state(tag, M, c0, h0)

        def one(r, timed):   # round r of a chunk reads logw[r & 1] and writes the other (chunks hold an even number of rounds)
            src, dst = sets(r)
            logits, _, _ = self.step(tok_rows, src["c2"], src["h2"], want="logits", bufs=dst, timed=timed)
            st = _stream()
            lib.vc_mixture_topk_f32(st, P(logits), B, K, V, V, P(logw[r & 1]), 1, P(tv), P(tok), P(stat), P(ws), ws_bytes)
            lib.vc_mixture_advance_f32(st, P(logits), V, V, P(stat), B, K, None, P(tok), P(logw[r & 1]), P(logw[1 - (r & 1)]), None, P(tok_rows),
                                       int(eos), P(f["done"]), P(f["seq"]), max_len, P(f["len"]))
            lib.vc_decode_round_end_i32(st, P(f["done"]), B, P(pending), None)

        Kc = self._chunk_rounds(check_every)
        steps = self._run_chunks(("marginal_greedy", B, K, Kc, max_len, int(eos)), [tok_rows, tok, tv, stat, pending, ibuf, dbuf, ws] + state,
                                 one, reset, Kc, max_len, check_every, pending)
        return marginal_greedy_from_host(*self._to_host(tag, ibuf, dbuf), lay.off, B, K, max_len, steps)

    def marginal_greedy(self, features, c_v=None, eps=None, bos=1, eos=2, draws=20, max_len=None, check_every=4):
        """Greedy decoding under the K-draw mixture p(y | I) ~ 1/K sum_k p(y | z_k, I) (DESIGN.md "Marginal decoding"): per image
        {"tokens": ids up to and including the first <EOS> (at most max_len), "marginal": float, "logprob": float64 [K]}.
        The K = `draws` draws of an image are diverse()'s and score()'s (z = prior_mean + std * eps[k]; eps [K, S, B, L], Philox on
        device when None: those draws depend on how the passes are cut).  Every round steps all B*K rows, mixes each image's K next-word
        distributions with the draws' posterior weights w_k ~ p(prefix | z_k) (vc_mixture_topk_f32), takes the mixture's best word,
        feeds it to all K rows and adds its log-softmax to each draw's logprob (vc_mixture_advance_f32).  By the chain rule
        marginal = logsumexp_k logprob - log K is the sum of the mixture's conditional log-probabilities of the tokens: score()'s
        marginal of the returned caption for the same eps.  <BOS> is fed once, as in greedy().  Rounds replay as hipGraph chunks of
        check_every rounds (VC_DECODE_GRAPH=0: the eager loop, same ids); images are decoded in passes of <= diverse_rows rows, an
        image with all its draws in one pass.  A --no_encoder model has no z: every draw is the same and the ids are greedy()'s."""
        K, B = int(draws), int(features.shape[0])
        self._check_draws(K, eps, B)
        max_len = int(max_len or self.p.gen_max_len)
        c_v, eps = (np.asarray(a) if a is not None else None for a in (c_v, eps))
        res = []
        for sl in self._marginal_passes(B, K):
            res += self._marginal_greedy_pass(features[sl], _cut(c_v, sl), _cut(eps, sl, 2), K, bos, eos, max_len, check_every)
        return res

    def _marginal_beam_pass(self, features, c_v, eps, K, n, bos, eos, max_len, len_norm_f, check_every):
        """One pass of marginal_beam_search(): B images x n hypothesis groups x K draws; rows (b*n + j)*K + k.  _beam_run's procedure
        on ONE slice: the TopN bookkeeping is vc_beam_update's on the B*n groups, every row move goes through parent_rows / tok_rows."""
        lib, e = self.lib, self.e
        c0, h0 = self._diverse_init(features, c_v, eps, K)
        BK, Hd, V = int(c0.shape[0]), self.p.decoder_hidden, e.V
        B = BK // K
        G = B * n
        M = G * K
        i32 = torch.int32
        tok0 = self._b("mb_tok0_%d" % BK, (BK,), i32)
        tok0.fill_(bos)
        _, c1, h1 = self.step(tok0, c0, h0, want="state", bufs=self._round_bufs("mb0_%d_" % BK, BK))   # decoder.py:230-236: the state only
        L, rounds = max_len + 2, max_len - 1
        xproj = self._xproj_for(M, rounds)
        tag = "mb%d_%d_%d_%d_" % (B, K, n, L)
        bs = _BeamSlice(self, tag, B, n, L, extra=[("logw0", M), ("logw1", M)])
        logw, pcount = [bs.d["logw0"], bs.d["logw1"]], bs.i["pcount"]
        parent_rows, tok_rows, rows0 = self._b(tag + "parent_rows", (M,), i32), self._b(tag + "tok_rows", (M,), i32), self._b(tag + "rows0", (M,), i32)
        rows0.copy_(torch.arange(M, dtype=i32, device=e.dev))
        tv, ti, stat = self._b(tag + "tv", (G, n)), self._b(tag + "ti", (G, n), i32), self._b(tag + "stat", (M, 2))
        bufs = self._round_bufs(tag, M)
        cg, hg, alive = self._b(tag + "cg", (M, Hd)), self._b(tag + "hg", (M, Hd)), self._b(tag + "alive", (1,))
        ws, ws_bytes = self._mixture_ws(tag, G, n)
        self._pack_wh(M)

        def reset():   # vc_beam_init with H = K * Hd: group b*n + j starts from the K states of image b, i.e. row (b*n + j)*K + k from row b*K + k
            bs.init(lib, bos, K * Hd, c1, h1, bufs["c2"], bufs["h2"])
            parent_rows.copy_(rows0); tok_rows.fill_(bos); logw[0].zero_(); logw[1].zero_()

        def one(it, timed):
            s_, par = _stream(), it & 1
            lib.vc_beam_gather_f32(s_, P(bufs["c2"]), P(bufs["h2"]), P(parent_rows), M, Hd, P(cg), P(hg), P(xproj), P(tok_rows), V, 4 * Hd, P(bufs["gact"]))
            logits, _, _ = self.step(tok_rows, cg, hg, want="logits", bufs=bufs, timed=timed, projected=xproj is not None)
            lib.vc_mixture_topk_f32(s_, P(logits), G, K, V, V, P(logw[par]), n, P(tv), P(ti), P(stat), P(ws), ws_bytes)
            lib.vc_beam_update(s_, B, n, L, int(eos), float(len_norm_f), P(tv), P(ti), *bs.update_args(par))
            lib.vc_mixture_advance_f32(s_, P(logits), V, V, P(stat), G, K, P(bs.parent), P(bs.tok), P(logw[par]), P(logw[1 - par]), P(parent_rows),
                                       P(tok_rows), int(eos), None, None, 0, None)

        def count_alive(steps, k):
            lib.vc_count_nonzero_i32(_stream(), P(pcount), B, P(alive))

        Kc = self._chunk_rounds(check_every)
        steps = 0
        if rounds > 0:
            steps = self._run_chunks(("marginal_beam", B, K, n, L, Kc, int(eos), float(len_norm_f)),
                                     bs.tensors + [parent_rows, tok_rows, tv, ti, stat, cg, hg, alive, ws, xproj, self._ones_for(M)]
                                     + list(bufs.values()), one, reset, Kc, rounds, check_every, alive, count_alive)
        else:
            reset()
        return beams_from_host(*self._to_host(tag, bs.ibuf, bs.scores), bs.lay.off, B, n, L, steps & 1)

    def marginal_beam_search(self, features, c_v=None, eps=None, bos=1, eos=2, draws=20, beam_size=2, max_len=None, len_norm_f=0.7,
                             check_every=4):
        """Beam search under the K-draw mixture (DESIGN.md "Marginal decoding"): beam_search's procedure and return shape -- per image
        the (sentence, score) of the kept beams, descending -- with a hypothesis = one sentence carried by K decoder states, one per
        latent draw (marginal_greedy's draws; eps [K, S, B, L]).  A round gathers the rows of the kept hypotheses (vc_beam_gather_f32 by
        parent_rows / tok_rows), steps them, reduces each hypothesis's K rows to the mixture's beam_size best words
        (vc_mixture_topk_f32), runs the unchanged TopN bookkeeping (vc_beam_update: its log-probabilities are now the mixture's, so a
        caption's logprob is log 1/K sum_k p(caption | z_k)) and advances the draws' weights (vc_mixture_advance_f32).  As in
        beam_search, <BOS> is consumed twice (the first time for the state only) and max_len - 1 rounds run.  One slice, one stream;
        passes of <= diverse_rows rows (images x beam_size x draws), an image with all its rows in one pass.  beam_size is 1..16."""
        K, B, n = int(draws), int(features.shape[0]), int(beam_size)
        self._check_draws(K, eps, B)
        if not 1 <= n <= min(16, self.e.V):
            raise ValueError("marginal_beam_search: beam_size must be 1..16 and at most the vocabulary (got %d)" % n)
        max_len = int(max_len or self.p.gen_max_len)
        c_v, eps = (np.asarray(a) if a is not None else None for a in (c_v, eps))
        res = []
        for sl in self._marginal_passes(B, n * K):
            res += self._marginal_beam_pass(features[sl], _cut(c_v, sl), _cut(eps, sl, 2), K, n, bos, eos, max_len, len_norm_f, check_every)
        return res

    # ------------------------------------------------------------------ beam search
    def _beam_part(self, k, nparts, c, h, n, L, rounds, K, bos, eos, len_norm_f, xproj, fused, groups=None, cons=None, ctl=None):
        """The persistent device state of one slice of images (vae_model/decoder.py:238-247) and its round function.  A call decodes its
        images as `nparts` independent slices on `nparts` streams (beam_search): buffers are per (slice, beam width, length) and a
        captured chunk of rounds bakes their addresses.
        groups = (G, diversity): group beam search (diverse_beam_search).  c, h then hold one row per "virtual image" b*G + g, a beam
        search of width n of its own; a row has kc = min(G*n, V) candidates and the round's bookkeeping is vc_beam_update_groups.
        cons = (C, Wc, kc, table [images, C, Wc]): constrained beam search.  c, h hold one row per virtual image b*S + s, the bank of state
        s (S = 2^C) of image b; the round is softmax + top-kc into persistent buffers + vc_beam_update_constrained, which reads the forced
        words' probabilities from the softmax rows; the table is a persistent buffer, loaded here.
        ctl = an active controls.DecodeControls: one vc_decode_controls_f32 launch on the round's logits, the histories being the live
        beams' sentences (sent[it & 1] / p_len, position 0 = <BOS>); its banned table is a persistent buffer too."""
        lib, e = self.lib, self.e
        B, Hd, V = int(c.shape[0]), self.p.decoder_hidden, e.V
        M = B * n
        i32 = torch.int32
        tag = "bm%d_%d_%dof%d_" % (n, L, k, nparts)
        kc = n
        if groups is not None:
            G, lam = int(groups[0]), float(groups[1])
            kc = min(G * n, V)
            tag = "bmg%d_%r_" % (G, lam) + tag   # (per setting: a captured chunk of one setting is never replayed for another)
        if cons is not None:
            C, Wc, kc, table = cons
            S = 1 << C
            tag = "bmc%d_%d_%d_" % (C, Wc, kc) + tag
        bs = _BeamSlice(self, tag, B, n, L)
        pt = types.SimpleNamespace(B=B, k=k, tag=tag, state=bs)
        pcount, p_len, sent, tok = bs.i["pcount"], bs.i["p_len"], bs.sent, bs.tok
        tv, ti = self._b(tag + "tv", (M, kc)), self._b(tag + "ti", (M, kc), i32)
        bufs = self._round_bufs(tag, M)
        bs.init(lib, bos, Hd, c, h, bufs["c2"], bufs["h2"])   # re-initialised per call
        cg, hg, alive = self._b(tag + "cg", (M, Hd)), self._b(tag + "hg", (M, Hd)), self._b(tag + "alive", (1,))
        cons_t = probs_t = None
        if cons is not None:   # only bank 0 starts with a beam; the constraint table of THIS call into the buffer the rounds read
            pcount.view(B // S, S)[:, 1:] = 0
            cons_t, probs_t = self._b(tag + "cons", (B // S, C, Wc), i32), self._b(tag + "probs", (M, V))
            if C > 0:
                cons_t.copy_(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)), non_blocking=True)
        ban_t = self._controls_table(tag, ctl) if ctl is not None else None

        def one(it, timed):
            s_ = _stream()
            # every new beam continues its parent's state and feeds its last word: three row moves, one launch
            lib.vc_beam_gather_f32(s_, P(bufs["c2"]), P(bufs["h2"]), P(bs.parent), M, Hd, P(cg), P(hg), P(xproj), P(tok), V, 4 * Hd, P(bufs["gact"]))
            logits, _, _ = self.step(tok, cg, hg, want="logits", bufs=bufs, timed=timed, projected=xproj is not None)
            if ctl is not None:   # the logits processed in place from the live beams' sentences
                self._apply_controls(ctl, ban_t, logits, M, sent[it & 1], L, 1, p_len, None, eos)
            if cons is not None:   # the two calls for every kc: the bookkeeping reads the forced words' probabilities from the rows
                lib.vc_softmax_rows_f32(s_, P(logits), M, V, V, P(probs_t), V)
                lib.vc_topk_rows_f32(s_, P(probs_t), M, V, V, kc, P(tv), P(ti))
            elif fused:   # softmax + top-k in one read of the logits (vc_softmax_topk_rows_f32: bit-identical to the two calls)
                lib.vc_softmax_topk_rows_f32(s_, P(logits), M, V, V, kc, P(tv), P(ti))
            else:
                probs = torch.empty_like(logits)
                lib.vc_softmax_rows_f32(s_, P(logits), M, V, V, P(probs), V)
                lib.vc_topk_rows_f32(s_, P(probs), M, V, V, kc, P(tv), P(ti))
            state = bs.update_args(it & 1)
            if cons is not None:   # the S banks of an image inside one wave; a beam may move to the bank of one more constraint
                lib.vc_beam_update_constrained(s_, B // S, C, Wc, n, kc, L, int(eos), float(len_norm_f), P(cons_t) if C else None, P(tv), P(ti),
                                               P(probs_t), V, V, *state)
            elif groups is None:
                lib.vc_beam_update(s_, B, n, L, int(eos), float(len_norm_f), P(tv), P(ti), *state)
            else:   # the G groups of an image in order inside one wave, each penalised by the words the earlier ones have just taken
                lib.vc_beam_update_groups(s_, B // G, G, n, kc, L, int(eos), float(len_norm_f), lam, P(tv), P(ti), *state)

        def chunk_fn():
            for r in range(K):
                one(r, False)
            lib.vc_count_nonzero_i32(_stream(), P(pcount), B, P(alive))

        pt.one, pt.chunk_fn, pt.alive, pt.pcount = one, chunk_fn, alive, pcount
        # (the key names the engine's workspace: recomputed before the capture, since the eager rounds of a first call may grow it)
        kind = ("beam",) if groups is None else ("beam_groups", G, kc, lam)
        if cons is not None:
            kind = ("beam_constrained", C, Wc, kc)
        if ctl is not None:
            kind = kind + ctl.key()
        pt.key_fn = lambda: self._graph_key(*kind, B, n, L, K, int(eos), float(len_norm_f),
                                            tensors=bs.tensors + [tv, ti, cg, hg, alive, xproj, self._ones_for(M), cons_t, probs_t]
                                            + ([ban_t] if ctl is not None else []) + list(bufs.values()))
        pt.graph = self._graphs.get(pt.key_fn()) if fused else None
        pt.it, pt.last, pt.done, pt.pending = 0, 0, rounds <= 0, []
        return pt

    def beam_search(self, features, c_v=None, eps=None, bos=1, eos=2, beam_size=2, max_len=None, len_norm_f=0.7, check_every=4, controls=None):
        """decoder.py:203-320 for a batch of images.  Returns per image the list of
        (sentence, score) of the kept beams in descending score order.

        Rows are [B, beam_size] throughout; every round is gather-state -> LSTM step -> logits -> softmax ->
        top-k -> vc_beam_update (the TopN bookkeeping, on device), with no host synchronisation except a
        4-byte "is any beam alive" read every `check_every` rounds.

        Images are independent, and a round is a chain of one throughput-bound kernel (the logits product) and four latency-bound
        ones (state gather, LSTM step, top-k, the heap bookkeeping: together half the round's time at 640 rows, on a fraction of
        the CUs).  A batch of >= 512 rows is therefore decoded as TWO slices of images on two streams: while one slice is in its
        latency-bound kernels the other's logits product has the CUs.  VC_DECODE_SLICES=1 keeps one slice -- same beams.

        controls: a controls.DecodeControls; every round's logits are processed from each live beam's words so far (one
        vc_decode_controls_f32 launch before the softmax), and probabilities, the p < 1e-12 skip and scores are taken under the softmax
        of the processed logits (DESIGN.md "Decoding controls").  None or a no-op value: the launches and graph keys of today."""
        return self._beam_run(features, c_v, eps, bos, eos, int(beam_size), max_len, len_norm_f, check_every, ctl=self._checked_controls(controls, eos, max_len))

    def diverse_beam_search(self, features, c_v=None, eps=None, bos=1, eos=2, groups=5, group_size=2, diversity=0.5, max_len=None,
                            len_norm_f=0.7, check_every=4, controls=None):
        """Group beam search (Diverse Beam Search, Vijayakumar et al. 2016, Hamming dissimilarity) for a batch of images: `groups`
        beam searches of width `group_size` per image advance in lock step; within a round the groups run in order, and a word that
        c live beams of the round's earlier groups have just taken costs a candidate diversity * c of its heap key (the stored
        log-probability stays the model's; finished captions are scored without the penalty).  Returns per image a list of `groups`
        lists of (sentence, score) in descending score order.  groups=1 is beam_search(beam_size=group_size); diversity=0 makes every
        group that search.

        The loop is beam_search's: rows [B, groups, group_size], groups * group_size candidates per row, and vc_beam_update_groups
        for the bookkeeping (one wave per image, its groups in order) -- same graph replay, alive check and slices.
        controls: a controls.DecodeControls, as in beam_search (the diversity penalty acts on the processed probabilities)."""
        G, w, lam = int(groups), int(group_size), float(diversity)
        if G < 1 or w < 1 or G * w > 16:
            raise ValueError("diverse_beam_search: groups * group_size must be 1..16, got %d x %d" % (G, w))
        if not (lam >= 0.0 and lam < float("inf")):
            raise ValueError("diverse_beam_search: diversity must be finite and >= 0, got %r" % (diversity,))
        flat = self._beam_run(features, c_v, eps, bos, eos, w, max_len, len_norm_f, check_every, groups=(G, lam),
                              ctl=self._checked_controls(controls, eos, max_len))
        return [flat[b * G:(b + 1) * G] for b in range(len(flat) // G)]

    def constrained_beam_search(self, features, constraints, c_v=None, eps=None, bos=1, eos=2, beam_size=2, max_len=None, len_norm_f=0.7,
                                check_every=4, all_states=False, controls=None):
        """Constrained beam search (Anderson et al., EMNLP 2017) for a batch of images: captions that must mention given words.
        `constraints` is, per image, a list of at most 3 lists of 1..4 token ids; a list is satisfied once ANY of its words has been
        emitted.  Every state -- the bit mask of satisfied constraints, 2^C of them -- has a beam search of width `beam_size` of its own
        (beam_size << C <= 16).  Per round a state's beams are extended by their most probable words outside the sets they have not
        satisfied yet, and a beam one constraint short of a state enters it by emitting a word of the missing set, whatever its rank.
        Returns per image (beams, state): the (sentence, score) list, descending, of the state with the most satisfied constraints that
        holds a complete caption (ties: the smaller mask; no complete caption anywhere: the first such state with live beams), and that
        state's mask -- bit j tells whether constraint j was met.  all_states=True returns per image the 2^C states' lists instead (each
        its complete captions if it has any, else its live beams).  No constraints at all is beam_search(beam_size) move for move.

        The loop is beam_search's: rows [B, 2^C, beam_size]; a round is softmax + the kc = min(V, beam_size + constraint words of an
        image) best words + vc_beam_update_constrained (one wave per image, a beam may move between its image's banks) -- same graph
        replay, alive check and slices.  The constraint table is a persistent buffer: a captured chunk serves other constraints of
        the same shape.
        controls: a controls.DecodeControls, as in beam_search; a forced word's probability is read from the processed rows too, so a
        constraint word that an n-gram ban or min_len rules out in a round is not forced in it.  A word both banned and in a constraint
        set is a ValueError."""
        B, V = int(features.shape[0]), self.e.V
        C, Wc, table, NW = check_constraints(constraints, B, V, bos, eos, beam_size)
        ctl = self._checked_controls(controls, eos, max_len, constraints)
        w, S = int(beam_size), 1 << C
        flat = self._beam_run(features, c_v, eps, bos, eos, w, max_len, len_norm_f, check_every, cons=(C, Wc, min(V, w + NW), table), ctl=ctl)
        banks = [flat[b * S:(b + 1) * S] for b in range(B)]
        if all_states:
            return banks
        full = [sum(1 << j for j in range(C) if (table[b, j] >= 0).any()) for b in range(B)]
        return [select_bank(banks[b], full[b], int(eos)) for b in range(B)]

    def _checked_controls(self, controls, eos, max_len, constraints=None):
        """`controls` of a decoding call as an active, checked DecodeControls, or None (ValueError before any launch)"""
        ctl = active_controls(controls)
        if ctl is not None:
            ctl.check(self.e.V, eos, max_len or self.p.gen_max_len, constraints)
        return ctl

    def _beam_run(self, features, c_v, eps, bos, eos, n, max_len, len_norm_f, check_every, groups=None, cons=None, ctl=None):
        """beam_search's loop over B * G "virtual images" of beam n (G = 1: beam_search itself; groups = (G, diversity): group beam
        search, virtual image b*G + g = group g of image b; cons = (C, Wc, kc, table [B, C, Wc]): constrained beam search, G = 2^C and
        virtual image b*G + s = the bank of state s of image b).  Returns the virtual images' beams in order."""
        lib, e = self.lib, self.e
        max_len = max_len or self.p.gen_max_len
        t_ph = _phase("", 0.0)
        c, h = self.init_state(features, c_v, eps)
        t_ph = _phase("init_state", t_ph)
        B, Hd, V = c.shape[0], self.p.decoder_hidden, e.V
        tok0 = self._b("bm_tok0", (B,), torch.int32)
        tok0.fill_(bos)
        _, c, h = self.step(tok0, c, h, want="state", bufs=self._round_bufs("bm0_", B))  # :230-236 -- probabilities discarded, state kept
        L, rounds = max_len + 2, max_len - 1
        G = 1
        if groups is not None:   # every group of an image starts from the image's state
            G = int(groups[0])
            c, h = c.repeat_interleave(G, 0), h.repeat_interleave(G, 0)
            B *= G
        if cons is not None:   # every bank of an image starts from the image's state (only bank 0 with a beam)
            G = 1 << int(cons[0])
            c, h = c.repeat_interleave(G, 0), h.repeat_interleave(G, 0)
            B *= G
        fused = (n if groups is None else min(G * n, V)) <= 8   # (candidates per row: the fused softmax-top-k holds 8)
        if cons is not None:   # (its round writes the probabilities to a persistent buffer: every kc can be captured)
            fused = True
        # the words' input projections from a table (rows x rounds of lookups against ONE product over the vocabulary)
        xproj = self._xproj_for(B * n, rounds)
        # Rounds run as hipGraph replays of K rounds each (nine launches per round otherwise): every buffer of a slice is persistent and
        # the sentence buffers alternate with the round's parity, so a chunk that starts at an even round is the same graph every time.
        # The FIRST call of a shape runs eagerly and captures the chunks at its end (a capture executes nothing); later calls replay
        # them.  VC_DECODE_GRAPH=0 keeps the eager loop -- same kernels, same beams.
        K = self._chunk_rounds(check_every)
        want = int(os.environ.get("VC_DECODE_SLICES", self.slices))
        nparts = want if (want > 1 and (B // G) % want == 0 and B * n >= self.slice_rows * want and xproj is not None) else 1
        nb = B // nparts
        if nparts > 1 and lib.vc_gemm_workspace_bytes(nb * n, V, Hd) != 0:
            nparts, nb = 1, B    # (a K-split logits product writes the engine's ONE workspace: slices on two streams would share it)
        part_cons = lambda k: None if cons is None else cons[:3] + (cons[3][k * nb // G:(k + 1) * nb // G],)   # (slices cut between images)
        parts = [self._beam_part(k, nparts, c[k * nb:(k + 1) * nb], h[k * nb:(k + 1) * nb], n, L, rounds, K, bos, eos, len_norm_f, xproj, fused, groups,
                                 part_cons(k), ctl) for k in range(nparts)]
        main = torch.cuda.current_stream()
        while len(self._side) < nparts - 1:
            self._side.append(torch.cuda.Stream())
        streams = [main] + self._side[:nparts - 1]
        for s in streams[1:]:
            s.wait_stream(main)
        # "is any beam alive" without idling the GPU: after every replayed chunk the 4-byte count is copied to pinned memory behind an
        # event; the host looks at the count of the PREVIOUS chunk before it launches the next (rounds of an image whose beams have all
        # ended are no-ops of vc_beam_update, so a chunk too many changes nothing)
        per = rounds // K + 2
        host_alive = self._pinned_alive(nparts * per)

        t_ph = _phase("bos step, vocabulary projection, slice set-up", t_ph)

        def advance(pt):
            if pt.graph is not None and pt.it % 2 == 0 and pt.it + K <= rounds:
                pend = pt.pending
                if check_every and len(pend) >= 2 and pend[-2][1].query() and float(host_alive[pend[-2][0]]) == 0.0:
                    pt.done = True
                    return
                pt.graph.replay()
                pt.it += K
                pt.last = 0
                if check_every:
                    slot = pt.k * per + len(pend)
                    host_alive[slot:slot + 1].copy_(pt.alive, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record()
                    pend.append((slot, ev))
            else:
                pt.one(pt.it, True)
                pt.last = 1 - (pt.it & 1)
                pt.it += 1
                if check_every and pt.it % check_every == 0:
                    lib.vc_count_nonzero_i32(_stream(), P(pt.pcount), pt.B, P(pt.alive))
                    if pt.alive.item() == 0:
                        pt.done = True
            if pt.it >= rounds:
                pt.done = True

        while not all(pt.done for pt in parts):
            for pt, s in zip(parts, streams):
                if not pt.done:
                    with torch.cuda.stream(s):
                        advance(pt)
        for s in streams[1:]:
            main.wait_stream(s)
        t_ph = _phase("rounds", t_ph)
        # results: two asynchronous copies per slice into pinned memory, one wait
        hosts = [self._to_host(pt.tag, pt.state.ibuf, pt.state.scores, wait=pt is parts[-1]) for pt in parts]
        t_ph = _phase("results: copies to pinned memory", t_ph)
        res = []
        for pt, (ints, dbls) in zip(parts, hosts):
            res += beams_from_host(ints, dbls, pt.state.lay.off, pt.B, n, L, pt.last)
        t_ph = _phase("results to host lists", t_ph)
        if fused and rounds > K:
            for pt in parts:
                if pt.graph is None:
                    self._capture(pt.key_fn(), pt.chunk_fn)   # (the results are on the host: the capture touches no state)
        return res

    # ------------------------------------------------------------------ stochastic beam search (Gumbel top-k)
    def stochastic_beam_search(self, features, c_v=None, eps=None, bos=1, eos=2, beam_size=10, max_len=None, len_norm_f=0.7, gumbel=None,
                               seed=None, check_every=4, controls=None):
        """Stochastic beam search (Kool, van Hoof, Welling, ICML 2019) for a batch of images: per image `beam_size` = n DISTINCT captions,
        an exact sample WITHOUT replacement from the model p(y | z, image), for the cost of one beam search of width n (DESIGN.md
        "Stochastic beam search").  Every entry carries phi (the log-probability of its words; f32 log-softmax terms, f64 sum) and G
        (its Gumbel-perturbed score); a round perturbs the log-softmax of every live entry's row, conditions the children on their
        parent's G and keeps the best n by G; finished captions stay in the beam and compete.  The search starts from the image's
        state like diverse() (<BOS> fed once) and runs until every entry has ended or holds max_len words.
        Returns per image {"kappa": the (n+1)-th largest perturbed score (-inf: nothing was ever rejected), "captions": [(words without
        <BOS>, logprob, perturbed, ended, weight, norm_weight), ...]} in rank order of `perturbed`; the weights are sbs_weights'
        (w = p / q, q = P(perturbed > kappa)): sum_i w_i f(y_i) is an unbiased estimate of E f(y), sum_i norm_weight_i f(y_i) its
        normalised form.  len_norm_f is not used by the search (the command line ranks its files with it).
        The round is vc_beam_gather_f32 -> step -> (controls) -> vc_sbs_expand_f32 -> vc_sbs_update, replayed as hipGraph chunks of
        check_every rounds with a 4-byte "all ended" read between chunks (VC_DECODE_GRAPH=0: the eager loop, same result); the round
        counter is a device int, so replays draw fresh noise.
        gumbel: [max_len, B * n, V] float64 noise to inject (row b*n + i of round t perturbs entry i of image b); None: Philox stream
        9 << 32 under seed (None: engine seed * 1000003 + 29, and every call of this generator draws another stream; a given seed
        repeats its result).  controls: a controls.DecodeControls; every round's logits are processed from each entry's words so far and
        phi is taken under the processed distribution, as in the other decoders.  There is no temperature in this mode: the weights
        need phi under the distribution that was sampled."""
        lib, e, p = self.lib, self.e, self.p
        n = int(beam_size)
        if n < 1 or n > 32:
            raise ValueError("stochastic_beam_search: beam_size must be 1..32, got %r" % (beam_size,))
        if float(p.temperature) != 1.0:
            raise ValueError("stochastic_beam_search samples the model itself: --temperature must be 1 (got %r)" % (p.temperature,))
        max_len = int(max_len or p.gen_max_len)
        ctl = self._checked_controls(controls, eos, max_len)
        c0, h0 = self.init_state(features, c_v, eps)
        B, Hd, V = int(c0.shape[0]), p.decoder_hidden, e.V
        M, L, kc = B * n, max_len + 1, min(n + 1, V)
        i32, f64 = torch.int32, torch.float64
        tag = "sbs%d_%d_%d_" % (B, n, L)
        lay = FieldLayout([("count", B), ("len", M), ("done", M), ("sent0", M * L), ("sent1", M * L)])
        dlay = FieldLayout([("phi", M), ("G", M), ("kappa", B)])
        ibuf, dbuf = self._b(tag + "ibuf", (lay.total,), i32), self._b(tag + "dbuf", (dlay.total,), f64)
        iv, (phi, G, kappa) = lay.views(ibuf), dlay.views(dbuf).values()
        count, p_len, p_done, sent = iv["count"], iv["len"], iv["done"], [iv["sent0"].view(M, L), iv["sent1"].view(M, L)]
        parent, tok = self._b(tag + "parent", (M,), i32), self._b(tag + "tok", (M,), i32)
        ck, cl, ci = self._b(tag + "ck", (M, kc), f64), self._b(tag + "cl", (M, kc)), self._b(tag + "ci", (M, kc), i32)
        rnd, base, pending = self._b(tag + "round", (1,), i32), self._b(tag + "base", (1,), i32), self._b(tag + "pending", (1,))
        bufs = self._round_bufs(tag, M)
        cg, hg = self._b(tag + "cg", (M, Hd)), self._b(tag + "hg", (M, Hd))
        gd = None
        if gumbel is not None:
            if tuple(np.shape(gumbel)) != (max_len, M, V):
                raise ValueError("gumbel must be [max_len, images * beam_size, V] = %s" % ((max_len, M, V),))
            gd = self._b(tag + "gumbel", (max_len, M, V), f64)
            gd.copy_(torch.from_numpy(np.ascontiguousarray(gumbel, dtype=np.float64)), non_blocking=True)
        if seed is None:   # another stream per call: the key's step is the round counter plus this base
            self._sbs_calls = getattr(self, "_sbs_calls", 0) + 1
            seed_, base_ = e.seed * 1000003 + 29, (self._sbs_calls << 12) & 0x7fffffff
        else:
            seed_, base_ = int(seed), 0
        seed_ &= (1 << 64) - 1
        xproj = self._xproj_for(M, max_len)
        self._pack_wh(M)
        ban_t = self._controls_table(tag, ctl) if ctl is not None else None
        trace = getattr(self, "sbs_trace", None)   # (tests: a list here receives every eager round's logits as a host array)

        def reset():
            lib.vc_sbs_init(_stream(), B, n, L, int(bos), Hd, P(c0), P(h0), P(bufs["c2"]), P(bufs["h2"]), P(count), P(phi), P(G), P(p_len),
                            P(p_done), P(sent[0]), P(sent[1]), P(kappa), P(parent), P(tok), P(rnd))
            base.fill_(base_)
            if trace is not None:
                del trace[:]

        def one(r, timed):
            s_ = _stream()
            lib.vc_beam_gather_f32(s_, P(bufs["c2"]), P(bufs["h2"]), P(parent), M, Hd, P(cg), P(hg), P(xproj), P(tok), V, 4 * Hd, P(bufs["gact"]))
            logits, _, _ = self.step(tok, cg, hg, want="logits", bufs=bufs, timed=timed, projected=xproj is not None)
            if ctl is not None:
                self._apply_controls(ctl, ban_t, logits, M, sent[r & 1], L, 1, p_len, p_done, eos)
            if trace is not None and timed:
                trace.append(logits.cpu().numpy().copy())
            lib.vc_sbs_expand_f32(s_, P(logits), M, n, V, V, P(count), P(p_done), kc, P(gd), max_len, P(rnd), seed_, 9 << 32, P(base),
                                  P(ck), P(cl), P(ci))
            lib.vc_sbs_update(s_, B, n, kc, L, int(bos), int(eos), P(ck), P(cl), P(ci), P(count), P(phi), P(G), P(p_len), P(p_done),
                              P(sent[r & 1]), P(sent[1 - (r & 1)]), P(kappa), P(parent), P(tok), P(rnd))
            lib.vc_decode_round_end_i32(s_, P(p_done), M, P(pending), None)

        K = self._chunk_rounds(check_every)
        steps = self._run_chunks(("sbs", B, n, L, K, kc, int(bos), int(eos), gd is None, seed_) + (ctl.key() if ctl is not None else ()),
                                 [ibuf, dbuf, parent, tok, ck, cl, ci, rnd, base, pending, cg, hg, xproj, gd, c0, h0, self._ones_for(M)]
                                 + ([ban_t] if ctl is not None else []) + list(bufs.values()), one, reset, K, max_len, check_every, pending)
        return sbs_from_host(*self._to_host(tag, ibuf, dbuf), lay.off, B, n, L, steps, int(eos))

    # ------------------------------------------------------------------ contrastive search
    def contrastive_search(self, features, c_v=None, eps=None, bos=1, eos=2, k=5, alpha=0.6, max_len=None, check_every=4, controls=None):
        """Contrastive search (Su et al., NeurIPS 2022; DESIGN.md "Contrastive search"; the definition is in include/vaecap.h) for a batch
        of images: every round looks one decoder step ahead for the k most likely next words of a row and takes the word that is likely
        AND whose decoder state is unlike every state the caption has produced so far: the largest (1 - alpha) * p(v) - alpha * max_j
        cos(h_v, g_j), equal scores to the more likely word.  The states are the decoder LSTM's outputs (what rnn_logits reads).
        Deterministic; alpha = 0 or k = 1 is greedy().  Returns per image (tokens, logprob): the words up to and including <EOS> (max_len
        of them without it) and the sum of their log-probabilities (f32 terms, f64 sum).
        One round, all on the current stream: vc_beam_gather_f32 (the picked state to the B*k look-ahead rows, the candidates' input
        projections from _project_vocab's table when _xproj_for says it pays) -> step(want="state") on B*k rows ->
        vc_contrastive_pick_f32 -> the logits product on the B picked rows only -> (controls, against the rows' words so far) ->
        softmax + top-k into the candidate buffers -> vc_decode_round_end_i32.  Rounds replay as hipGraph chunks of check_every rounds
        with a 4-byte "all ended" read between chunks (VC_DECODE_GRAPH=0: the eager loop, same kernels, same result).  The <BOS> round
        runs once before them on B rows: the pick kernel with k = 1 and emit = 0 starts the history.
        There is no temperature in this mode: p is the model's distribution (after the controls).  controls: a
        controls.DecodeControls; p, the top k and logprob are then taken under the processed distribution, as in the other decoders."""
        lib, e, p = self.lib, self.e, self.p
        k_, alpha = int(k), float(alpha)
        if k_ != k or k_ < 1 or k_ > 16:
            raise ValueError("contrastive_search: k must be 1..16, got %r" % (k,))
        if not (0.0 <= alpha <= 1.0):   # (a NaN fails both comparisons)
            raise ValueError("contrastive_search: alpha must be finite and in [0, 1], got %r" % (alpha,))
        max_len = int(max_len or p.gen_max_len)
        ctl = self._checked_controls(controls, eos, max_len)
        c0, h0 = self.init_state(features, c_v, eps)
        B, Hd, V, E = int(c0.shape[0]), p.decoder_hidden, e.V, p.embed_size
        k = min(k_, V)
        M, i32 = B * k, torch.int32
        fused = k <= 8   # (the fused softmax-top-k holds 8 candidates: _beam_part's rule)
        tag = "cs%d_%d_%d_" % (B, k, max_len)
        cand = self._candidates(tag, B, max_len)
        hist, h_sel = self._b(tag + "hist", (B, max_len + 1, Hd)), self._b(tag + "h_sel", (B, Hd))
        logits, probs = self._b(tag + "logits", (B, V)), (None if fused else self._b(tag + "probs", (B, V)))
        tv, ti, parent = self._b(tag + "tv", (B, k)), self._b(tag + "ti", (B, k), i32), self._b(tag + "parent", (M,), i32)
        tv0, ti0, parent0 = self._b(tag + "tv0", (B, k)), self._b(tag + "ti0", (B, k), i32), self._b(tag + "parent0", (M,), i32)
        tok0, pending = self._b(tag + "tok0", (B,), i32), self._b(tag + "pending", (1,))
        cg, hg = self._b(tag + "cg", (M, Hd)), self._b(tag + "hg", (M, Hd))
        bufs = {"x": self._b(tag + "x", (M, E)), "gact": self._b(tag + "gact", (M, 4 * Hd)), "c2": self._b(tag + "c2", (M, Hd)),
                "h2": self._b(tag + "h2", (M, Hd))}
        bufs0 = {"x": self._b(tag + "x0", (B, E)), "gact": self._b(tag + "gact0", (B, 4 * Hd)), "c2": self._b(tag + "c20", (B, Hd)),
                 "h2": self._b(tag + "h20", (B, Hd))}
        ban_t = self._controls_table(tag, ctl) if ctl is not None else None
        xproj = self._xproj_for(M, max_len)
        self._pack_wh(M)
        e._need_ws(lib.vc_gemm_workspace_bytes(B, V, Hd))
        W, bias = e.store.param("decoder/rnn_logits/kernel"), e.store.param("decoder/rnn_logits/bias")

        def tail(timed):   # h_sel -> the rows' next candidates: the logits product runs over B rows, not B*k
            s_ = _stream()
            e.gemm(0, 0, B, V, Hd, h_sel, Hd, W, e.Vp, logits, V, bias, tag="logits_gemm" if timed else None)
            if ctl is not None:
                self._apply_controls(ctl, ban_t, logits, B, cand.seq, max_len, 0, cand.len, cand.ended, eos)
            if fused:
                lib.vc_softmax_topk_rows_f32(s_, P(logits), B, V, V, k, P(tv), P(ti))
            else:
                lib.vc_softmax_rows_f32(s_, P(logits), B, V, V, P(probs), V)
                lib.vc_topk_rows_f32(s_, P(probs), B, V, V, k, P(tv), P(ti))

        # ---- the <BOS> round, once per call on B rows: g_0 starts the history (k = 1, emit = 0: no word is emitted, ti / tv are not read
        # for a decision), its logits give the first candidates; every look-ahead row r*k + i of round 0 continues row r of its state
        cand.ended.zero_(); cand.len.zero_(); cand.logprob.zero_()
        tok0.fill_(bos)
        _, c1, h1 = self.step(tok0, c0, h0, want="state", bufs=bufs0)
        lib.vc_contrastive_pick_f32(_stream(), B, 1, Hd, max_len, P(h1), P(ti), P(tv), P(hist), P(cand.len), P(cand.ended), P(cand.seq),
                                    P(cand.logprob), alpha, int(eos), 0, P(h_sel), P(parent0), None, None)
        tail(True)
        tv0.copy_(tv); ti0.copy_(ti)
        parent0.copy_(torch.arange(M, dtype=i32, device=e.dev) // k)

        def reset():   # what round 0 starts from (the history's slot 0 is never written again)
            tv.copy_(tv0); ti.copy_(ti0); parent.copy_(parent0)
            bufs["c2"][:B].copy_(c1); bufs["h2"][:B].copy_(h1)
            cand.ended.zero_(); cand.len.zero_(); cand.logprob.zero_()

        def one(r, timed):
            s_ = _stream()
            lib.vc_beam_gather_f32(s_, P(bufs["c2"]), P(bufs["h2"]), P(parent), M, Hd, P(cg), P(hg), P(xproj), P(ti), V, 4 * Hd, P(bufs["gact"]))
            self.step(ti.view(M), cg, hg, want="state", bufs=bufs, timed=timed, projected=xproj is not None)
            lib.vc_contrastive_pick_f32(s_, B, k, Hd, max_len, P(bufs["h2"]), P(ti), P(tv), P(hist), P(cand.len), P(cand.ended), P(cand.seq),
                                        P(cand.logprob), alpha, int(eos), 1, P(h_sel), P(parent), None, None)
            tail(timed)
            lib.vc_decode_round_end_i32(s_, P(cand.ended), B, P(pending), None)

        K = self._chunk_rounds(check_every)
        self._run_chunks(("contrastive", B, k, max_len, K, float(alpha), int(eos)) + (ctl.key() if ctl is not None else ()),
                         [cand.seq, cand.len, cand.ended, cand.logprob, hist, h_sel, logits, probs, tv, ti, parent, tv0, ti0, parent0, pending,
                          cg, hg, xproj, c1, h1, self._ones_for(M), ban_t] + list(bufs.values()), one, reset, K, max_len, check_every, pending)
        rows, lens, lps = cand.seq.cpu().numpy(), cand.len.cpu().numpy(), cand.logprob.cpu().numpy()
        return [(rows[b, :lens[b]].tolist(), float(lps[b])) for b in range(B)]
