"""Host side of the training objective options (DESIGN.md "Training objective options"): word dropout on the decoder inputs
(Bowman et al. 2016) and the cyclical annealing schedule as a host function (the device computes it from its own step counter,
csrc/optim.hip: cyclical_ann_kernel; this one is for logs and tests).

Free bits, the KL weight and label smoothing have no host part: they are kernels of csrc/loss.hip chosen by CaptionEngine.
"""
import math

import numpy as np


def word_dropout(cap_dec, lengths, rate, unk_id, rng):
    """A copy of the decoder inputs cap_dec [N, T] ("<BOS> w..", PAD = 0 behind position lengths[n] - 1) in which each word at the
    positions 1 .. lengths[n] - 1 is replaced by unk_id with probability `rate`.  <BOS> at position 0 and the PAD positions are
    never touched; the labels (cap_enc) are not an argument.  rng: numpy Generator -- one uniform per position of the array is
    drawn whatever the lengths are, so the stream position after a batch depends on its shape alone."""
    cap_dec = np.asarray(cap_dec)
    if not 0.0 <= rate < 1.0:
        raise ValueError("word dropout rate must be in [0, 1), not %r" % (rate,))
    out = cap_dec.copy()
    if rate == 0.0:
        return out
    N, T = cap_dec.shape
    pos = np.arange(T)[None, :]
    eligible = (pos >= 1) & (pos < np.asarray(lengths).reshape(N, 1))
    out[eligible & (rng.random((N, T)) < rate)] = unk_id
    return out


def unk_id(word2idx, vocab_size):
    """The id word dropout writes: the vocabulary's <UNK>, or the last id where there is no word list (--synthetic)."""
    return int(word2idx["<UNK>"]) if word2idx is not None and "<UNK>" in word2idx else int(vocab_size) - 1


SCHED_SCHEDULES = ("constant", "linear", "sigmoid")


def sched_rate(step, schedule, rate_max, ramp_steps):
    """The scheduled-sampling rate of global step `step` (0 = the first optimiser step of the run): the host statement of what
    vc_sched_mix_f32 computes from the device step counter (csrc/sched.hip; for logs and tests).  schedule: a name of
    SCHED_SCHEDULES or its index.  constant: rate_max (ramp_steps is ignored); linear: rate_max * min(1, step / ramp_steps);
    sigmoid: rate_max * (1 - k / (k + exp(step / k))), k = ramp_steps (Bengio et al. 2015, eq. 3, turned into a sampling rate)."""
    name = SCHED_SCHEDULES[schedule] if isinstance(schedule, int) else schedule
    if name not in SCHED_SCHEDULES:
        raise ValueError("schedule must be one of %s (got %r)" % (", ".join(SCHED_SCHEDULES), schedule))
    if not 0.0 <= rate_max <= 1.0:
        raise ValueError("rate_max must be in [0, 1], not %r" % (rate_max,))
    if name == "constant":
        return float(rate_max)
    if ramp_steps < 1:
        raise ValueError("ramp_steps must be >= 1 for the %s schedule (got %r)" % (name, ramp_steps))
    s, k = max(float(step), 0.0), float(ramp_steps)
    if name == "linear":
        return float(rate_max) * min(1.0, s / k)
    return float(rate_max) / (1.0 + k * math.exp(-s / k))   # == 1 - k / (k + exp(s / k)), without the overflow far behind the ramp


def cyclical_annealing(step, period, ramp=0.5, cycles=0):
    """min(1, (step mod P) / (R * P)) while step < M * P or M == 0, 1 afterwards (Fu et al. 2019); P <= 0: 1."""
    if period <= 0 or (cycles > 0 and step >= cycles * period):
        return 1.0
    return min(1.0, (step % period) / (ramp * period))
