"""CPU: the host parsers of stochastic beam search and marginal greedy decoding (decode_host.sbs_from_host, marginal_greedy_from_host) on
hand-made result buffers whose layout is spelt out here, independently of decode_host's: an image with fewer entries than the beam,
kappa = -inf, an entry cut at max_len, and both parities of the number of rounds (which of sent0 / sent1 and logw0 / logw1 the last
round wrote).  And decode_host itself: importable without torch, its names re-exported by generate."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from vae_captioning_amd import decode_host

BOS, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pack(fields):
    """[(name, array)] -> (the arrays back to back, {name: offset})"""
    io, o = {}, 0
    for name, a in fields:
        io[name] = o
        o += np.asarray(a).size
    return np.concatenate([np.asarray(a).ravel() for _, a in fields]), io


# ------------------------------------------------------------------ stochastic beam search
# int32: count [B], len [B*n], done [B*n], sent0 [B*n, L], sent1 [B*n, L]; float64: phi [B*n], G [B*n], kappa [B]
B, n, L = 3, 3, 5                                   # max_len 4: a sentence holds <BOS> + at most 4 words
SENT = [[BOS, 5, 6, EOS, 99], [BOS, 7, 8, 9, 10], [BOS, EOS, 99, 99, 99],      # image 0: full beam; entry 1 is cut at max_len
        [BOS, 11, EOS, 99, 99], [BOS, 12, 13, 99, 99], [77, 77, 77, 77, 77],    # image 1: two entries of three; entry 1 still open
        [BOS, 14, 15, 16, EOS], [88, 88, 88, 88, 88], [88, 88, 88, 88, 88]]     # image 2: one entry, ended by its last word
LEN = [4, 5, 2, 3, 3, 5, 5, 4, 4]                                                # (rows past an image's count hold junk)
COUNT = [3, 2, 1]
PHI = [-1.5, -4.0, -0.75, -0.5, -2.25, -9.0, -3.0, -9.0, -9.0]
GUM = [0.5, -1.0, 2.0, 1.25, 0.0, 7.0, -0.5, 7.0, 7.0]
KAPPA = [-2.0, -math.inf, -math.inf]
WANT_WORDS = [[[5, 6, EOS], [7, 8, 9, 10], [EOS]], [[11, EOS], [12, 13]], [[14, 15, 16, EOS]]]
WANT_ENDED = [[True, False, True], [True, False], [True]]


@pytest.mark.parametrize("steps", [3, 4], ids=["odd-rounds-sent1", "even-rounds-sent0"])
def test_sbs_from_host_reads_the_entries_of_the_store_the_last_round_wrote(steps):
    junk = np.full((B * n, L), 55, np.int32)
    stores = (SENT, junk) if steps % 2 == 0 else (junk, SENT)
    ints, io = _pack([("count", COUNT), ("len", LEN), ("done", np.ones(B * n)), ("sent0", stores[0]), ("sent1", stores[1])])
    dbls = np.array(PHI + GUM + KAPPA, np.float64)
    got = decode_host.sbs_from_host(ints.astype(np.int32), dbls, io, B, n, L, steps, EOS)
    assert len(got) == B
    for b, r in enumerate(got):
        assert r["kappa"] == KAPPA[b] and len(r["captions"]) == COUNT[b]
        rows = range(b * n, b * n + COUNT[b])
        q = [1.0 if KAPPA[b] == -math.inf else 1.0 - math.exp(-math.exp(PHI[i] - KAPPA[b])) for i in rows]   # P(perturbed > kappa)
        w = [math.exp(PHI[i]) / qi for i, qi in zip(rows, q)]
        for j, (i, cap) in enumerate(zip(rows, r["captions"])):
            words, logprob, perturbed, ended, weight, norm = cap
            assert words == WANT_WORDS[b][j] and all(isinstance(t, int) for t in words)
            assert (logprob, perturbed, ended) == (PHI[i], GUM[i], WANT_ENDED[b][j])
            assert weight == pytest.approx(w[j], rel=1e-12) and norm == pytest.approx(w[j] / sum(w), rel=1e-12)
    assert [c[4] for c in got[1]["captions"]] == [pytest.approx(math.exp(p), rel=1e-15) for p in PHI[3:5]]   # kappa = -inf: w = p


# ------------------------------------------------------------------ marginal greedy
# int32: done [B], len [B], seq [B, L]; float64: logw0 [B*K], logw1 [B*K]
def test_marginal_greedy_from_host_takes_the_log_weights_the_last_round_wrote():
    Bm, K, Lm = 3, 2, 4
    seq = [[5, 6, EOS, 99], [7, 8, 9, 10], [EOS, 99, 99, 99]]          # image 1 is cut at max_len
    ln = [3, 4, 1]
    last = [-1.0, -3.0, -2.5, -2.5, -700.0, -0.25]                     # [B, K]
    other = [9.0] * (Bm * K)
    ints, io = _pack([("done", [1, 0, 1]), ("len", ln), ("seq", seq)])
    for steps in (3, 4):
        dbls = np.array(other + last if steps % 2 else last + other, np.float64)
        got = decode_host.marginal_greedy_from_host(ints.astype(np.int32), dbls, io, Bm, K, Lm, steps)
        assert [r["tokens"] for r in got] == [[5, 6, EOS], [7, 8, 9, 10], [EOS]]
        for b, r in enumerate(got):
            lw = last[b * K:(b + 1) * K]
            assert r["logprob"].dtype == np.float64 and r["logprob"].tolist() == lw
            assert r["marginal"] == pytest.approx(math.log(sum(math.exp(v) for v in lw) / K), rel=1e-12)
        got[0]["logprob"][0] = 0.0
        assert dbls[(steps % 2) * Bm * K] == -1.0, "logprob is a copy, not a view of the pinned buffer"


# ------------------------------------------------------------------ the module
def test_decode_host_imports_without_torch_or_the_engine(tmp_path):
    (tmp_path / "torch.py").write_text("raise ImportError('torch must not be imported')\n")
    code = ("import sys; import vae_captioning_amd.decode_host; "
            "assert not [m for m in sys.modules if m == 'torch' or m.startswith('vae_captioning_amd.engine')]")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_generate_re_exports_every_host_name():
    from vae_captioning_amd import generate
    for name in ("beams_from_host", "FieldLayout", "beam_fields", "diverse_fields", "diverse_from_host", "rerank_by_marginal", "sbs_weights",
                 "merge_groups", "check_truncation", "check_constraints", "select_bank", "sbs_from_host", "marginal_greedy_from_host",
                 "DIVERSE_MAX_DRAWS", "SCORE_MAX_TOKENS", "CBS_MAX_SETS", "CBS_MAX_WORDS"):
        assert getattr(generate, name) is getattr(decode_host, name), name
