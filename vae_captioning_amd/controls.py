"""Decoding controls (generate.py: the `controls` keyword of the decoders; csrc/decode_controls.hip): what a caption may NOT say.

Before a round chooses words for a row, the row's logits are processed from the caption words the row has emitted so far:
repetition penalty (every distinct word once), no-repeat n-gram bans, banned words, <EOS> banned below a minimum length -- in that
order, a ban always winning over the penalty (DESIGN.md "Decoding controls").  The decoder's distribution is the softmax of the
processed logits; score(), bound() and the re-rankers keep the unprocessed model."""
import json

import numpy as np

from .constraints import lookup_word

MAX_NGRAM, MAX_PENALTY, MAX_BANNED = 8, 10.0, 256   # vc_decode_controls_f32: n-gram length, penalty, table entries


class DecodeControls(object):
    """no_repeat_ngram n (0..8, 0 = off): no n-gram twice in a caption; min_len m (>= 0, 0 = off): no <EOS> before m words;
    repetition_penalty t (1..10, 1 = off): the logit of every word already emitted is divided (positive) or multiplied (negative)
    by t; banned: at most 256 token ids that are never emitted (kept as a sorted unique int32 array).  ValueError outside these."""

    def __init__(self, no_repeat_ngram=0, min_len=0, repetition_penalty=1.0, banned=()):
        for name, v in (("no_repeat_ngram", no_repeat_ngram), ("min_len", min_len)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer (got %r)" % (name, v))
        if not 0 <= int(no_repeat_ngram) <= MAX_NGRAM:
            raise ValueError("no_repeat_ngram must be 0..%d (0 = off; got %r)" % (MAX_NGRAM, no_repeat_ngram))
        if int(min_len) < 0:
            raise ValueError("min_len must be >= 0 (0 = off; got %r)" % (min_len,))
        if isinstance(repetition_penalty, bool) or not isinstance(repetition_penalty, (int, float, np.integer, np.floating)):
            raise ValueError("repetition_penalty must be a number (got %r)" % (repetition_penalty,))
        t = float(np.float32(repetition_penalty))   # (what the kernel gets)
        if not 1.0 <= t <= MAX_PENALTY:
            raise ValueError("repetition_penalty must be in [1, %g] (1 = off; got %r)" % (MAX_PENALTY, repetition_penalty))
        ids = []
        for v in (banned if banned is not None else ()):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
                raise ValueError("banned must hold token ids >= 0 (got %r)" % (v,))
            ids.append(int(v))
        ids = np.unique(np.asarray(ids, np.int64)).astype(np.int32)
        if ids.size > MAX_BANNED:
            raise ValueError("banned holds %d distinct ids (at most %d)" % (ids.size, MAX_BANNED))
        self.no_repeat_ngram, self.min_len, self.repetition_penalty, self.banned = int(no_repeat_ngram), int(min_len), t, ids

    def is_noop(self):
        return self.no_repeat_ngram == 0 and self.min_len == 0 and self.repetition_penalty == 1.0 and self.banned.size == 0

    def key(self):
        """what a captured round bakes of the controls (the banned WORDS live in a buffer loaded per call: only their number counts)"""
        return ("controls", self.no_repeat_ngram, self.min_len, self.repetition_penalty, int(self.banned.size))

    def check(self, V, eos, max_len, constraints=None):
        """The checks of a decoding call, before any launch: ValueError for a banned id outside the vocabulary, <EOS> banned,
        n_banned + max_len + 1 >= V (a row could lose every word), min_len >= max_len, a word both banned and in a constraint set."""
        ids = self.banned.tolist()
        if ids and ids[-1] >= int(V):
            raise ValueError("controls: banned id %d outside the vocabulary [0, %d)" % (ids[-1], V))
        if int(eos) in ids:
            raise ValueError("controls: <EOS> (%d) cannot be banned (min_len keeps a caption from ending early)" % int(eos))
        if len(ids) + int(max_len) + 1 >= int(V):
            raise ValueError("controls: %d banned words + max_len %d + 1 >= vocabulary %d: a row could lose every word" % (len(ids), max_len, V))
        if self.min_len >= int(max_len):
            raise ValueError("controls: min_len %d must be below max_len %d" % (self.min_len, max_len))
        if constraints is not None:
            both = sorted(set(ids) & {int(v) for sets in constraints for st in sets for v in st})
            if both:
                raise ValueError("controls: word %d is both banned and in a constraint set" % both[0])

    def summary(self):
        return "decoding controls: no_repeat_ngram %d, min_len %d, repetition_penalty %g, %d banned words" % (
            self.no_repeat_ngram, self.min_len, self.repetition_penalty, self.banned.size)

    def __repr__(self):
        return "DecodeControls(no_repeat_ngram=%d, min_len=%d, repetition_penalty=%r, banned=%r)" % (
            self.no_repeat_ngram, self.min_len, self.repetition_penalty, self.banned.tolist())


def active(controls):
    """`controls` of a decoding call as a DecodeControls that changes something, or None (None or a no-op value: the call takes the
    path it takes without the keyword)"""
    if controls is None:
        return None
    if not isinstance(controls, DecodeControls):
        raise ValueError("controls must be a DecodeControls or None (got %r)" % (controls,))
    return None if controls.is_noop() else controls


def parse_banned(spec, vocab):
    """A banned-words list as the command line gives it -> sorted list of token ids.  spec: a list of words (strings looked up in the
    vocabulary) or integer token ids, or a string of comma-separated words; vocab: the dictionary (word2idx, vocab_size).  Unknown
    words (strings the vocabulary lacks, ids outside it) are dropped, counted and the count printed, like --constraints."""
    if isinstance(spec, str):
        spec = [w.strip() for w in spec.split(",") if w.strip()]
    if not isinstance(spec, (list, tuple)):
        raise ValueError("banned words: a list of words or token ids (got %r)" % (spec,))
    ids, dropped = set(), 0
    for word in spec:
        try:
            v = lookup_word(word, vocab.word2idx, int(vocab.vocab_size))
        except ValueError as err:
            raise ValueError("banned words: %s" % err)
        if v is None:
            dropped += 1
        else:
            ids.add(v)
    print("banned words: %d token ids; dropped %d unknown words" % (len(ids), dropped))
    return sorted(ids)


def load_banned(path, vocab):
    """--banned_words FILE: a JSON list of words or ids -> parse_banned"""
    with open(path) as fh:
        spec = json.load(fh)
    if not isinstance(spec, list):
        raise ValueError("banned words: the file must hold a JSON list of words or token ids")
    return parse_banned(spec, vocab)


def from_params(params, vocab):
    """The DecodeControls of a run's flags (None when every flag is at its default)"""
    path = getattr(params, "banned_words", None)
    c = DecodeControls(getattr(params, "no_repeat_ngram", 0), getattr(params, "min_len", 0), getattr(params, "repetition_penalty", 1.0),
                       load_banned(path, vocab) if path else ())
    return None if c.is_noop() else c
