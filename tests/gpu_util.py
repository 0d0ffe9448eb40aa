"""Helpers for the -m gpu parity tests: everything goes through the C ABI."""
import numpy as np
import torch

from vae_captioning_amd import abi


def stream():
    return torch.cuda.current_stream().cuda_stream


# Tensors created by dev() stay alive until the end of the test: `P(dev(x))` hands a raw
# pointer to the library, and a temporary freed before the next dev() call would have its
# block recycled by the caching allocator (the next upload would overwrite it).
_KEEP = []


def dev(x, dtype=None):
    a = np.ascontiguousarray(x)
    if dtype is not None:
        a = a.astype(dtype)
    t = torch.from_numpy(a).cuda()
    _KEEP.append(t)
    return t


def release():
    del _KEEP[:]


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def empty_bytes(nbytes):
    return torch.empty(max(int(nbytes), 16) // 4 + 4, dtype=torch.float32, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


P = abi.ptr


class BeamState(object):
    """vc_beam_update's state for Bv (virtual) images of beam n, junk-filled and then started by vc_beam_init (whose LSTM state
    inputs and outputs are kept as c_in / h_in / c_out / h_out)."""
    FIELDS = ("pcount", "ccount", "p_score", "p_logprob", "p_len", "c_score", "c_logprob", "c_len", "c_slot", "c_free", "c_sent", "parent", "tok")

    def __init__(self, lib, Bv, n, L, bos, H=8):
        M = Bv * n
        junk_i = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")
        junk_d = lambda *shape: torch.full(shape, 3.5, dtype=torch.float64, device="cuda")
        self.Bv, self.n, self.L, self.M = Bv, n, L, M
        self.pcount, self.ccount, self.c_free = junk_i(Bv), junk_i(Bv), junk_i(Bv)
        self.p_score, self.p_logprob, self.p_len = junk_d(M), junk_d(M), junk_i(M)
        self.sent = [junk_i(M, L), junk_i(M, L)]
        self.c_score, self.c_logprob, self.c_len, self.c_slot = junk_d(M), junk_d(M), junk_i(M), junk_i(M)
        self.c_sent = junk_i(Bv * (n + 1), L)
        self.parent, self.tok = junk_i(M), junk_i(M)
        self.c_in, self.h_in = torch.randn(Bv, H, device="cuda"), torch.randn(Bv, H, device="cuda")
        self.c_out, self.h_out = torch.zeros(M, H, device="cuda"), torch.zeros(M, H, device="cuda")
        lib.vc_beam_init(stream(), Bv, n, L, bos, H, P(self.c_in), P(self.h_in), P(self.c_out), P(self.h_out), P(self.pcount), P(self.ccount),
                         P(self.p_score), P(self.p_logprob), P(self.p_len), P(self.sent[0]), P(self.sent[1]), P(self.c_score), P(self.c_logprob),
                         P(self.c_len), P(self.c_slot), P(self.c_free), P(self.c_sent), P(self.parent), P(self.tok))

    def args(self, it):
        return (P(self.pcount), P(self.ccount), P(self.p_score), P(self.p_logprob), P(self.p_len), P(self.sent[it & 1]), P(self.sent[1 - (it & 1)]),
                P(self.c_score), P(self.c_logprob), P(self.c_len), P(self.c_slot), P(self.c_free), P(self.c_sent), P(self.parent), P(self.tok))

    def snapshot(self, it):
        d = {k: host(getattr(self, k)) for k in self.FIELDS}
        d["sent"] = host(self.sent[1 - (it & 1)])
        return d


def assert_close(got, ref, rtol, atol_scale=None, msg=""):
    """max|got-ref| <= rtol * max|ref| (+ tiny); prints where the worst element is."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (msg, got.shape, ref.shape)
    scale = np.abs(ref).max() if atol_scale is None else atol_scale
    err = np.abs(got - ref)
    if err.size == 0:
        return
    worst = np.unravel_index(np.argmax(err), err.shape)
    tol = rtol * scale + 1e-30
    assert np.isfinite(got).all(), "%s: non-finite output" % msg
    assert err.max() <= tol, "%s: max err %.3e > tol %.3e at %s (got %r ref %r), %d/%d elements off" % (
        msg, err.max(), tol, worst, got[worst], ref[worst], int((err > tol).sum()), err.size)


# ---- the C4 activation layout of the Winograd kernels (include/vaecap.h): [B][C/4][H][W][4] ----
def to_c4(a):
    """NHWC numpy array [B,H,W,C] -> C4 [B, C/4, H, W, 4]."""
    a = np.asarray(a)
    B, H, W, C = a.shape
    return np.ascontiguousarray(a.reshape(B, H, W, C // 4, 4).transpose(0, 3, 1, 2, 4))


def from_c4(a, shape=None):
    """C4 array (any shape holding B*C/4*H*W*4 elements; `shape` = the NHWC shape [B,H,W,C]) -> NHWC numpy array."""
    a = np.asarray(a)
    if shape is None:
        B, C4, H, W, _ = a.shape
        shape = (B, H, W, C4 * 4)
    B, H, W, C = shape
    return np.ascontiguousarray(a.reshape(B, C // 4, H, W, 4).transpose(0, 2, 3, 1, 4).reshape(B, H, W, C))


def dev_c4(x, dtype=None):
    return dev(to_c4(x), dtype)


def host_c4(t, shape):
    """device tensor holding a C4 activation -> NHWC numpy array of `shape` [B,H,W,C]."""
    return from_c4(host(t), shape)


def grads_only(tr):
    """Trainer.gall with the two REPORTING scalars of the data-parallel step (ce_num, kl_sum: tail slots 1 and 2, written only when
    collectives are on) zeroed -- what must be identical between a collective and a collective-free step."""
    g = tr.gall.clone()
    n = tr.cap.store.n
    g[n + 1:n + 3] = 0
    return g
