"""Word constraints of constrained beam search (generate.py: constrained_beam_search) as the command line gives them.

A constraints file is JSON: {image_id: [[word, ...], ...]}; an image's entry is a list of at most 3 sets of at most 4 words, and a set
is satisfied once ANY of its words is in the caption.  The entry "*" applies to every image without an entry of its own.  A word is
a string looked up in the vocabulary, or an integer taken as a token id.  Unknown words (strings the vocabulary lacks, ids outside it,
<BOS> / <EOS>) are dropped, and so are sets left empty; both are counted and the counts printed."""
import json

MAX_SETS, MAX_WORDS, MAX_ROWS = 3, 4, 16   # vc_beam_update_constrained: constraints per image, words per constraint, beams x states


def lookup_word(word, word2idx, V, special=()):
    """A word of a constraints or banned-words list as a token id: a string is looked up in the vocabulary, an integer is taken as an
    id.  None for an unknown word (a string the vocabulary lacks, an id outside [0, V), an id in `special`); ValueError for anything
    that is neither a string nor an integer."""
    if isinstance(word, bool) or not isinstance(word, (int, str)):
        raise ValueError("a word must be a string or an integer id (got %r)" % (word,))
    v = word2idx.get(word) if isinstance(word, str) else word
    if v is None or not 0 <= int(v) < V or int(v) in special:
        return None
    return int(v)


class Constraints(object):
    """by_id {str(image_id): [[token id, ...], ...]}, default (the "*" entry or []), C = the largest number of sets of an entry,
    width = beams per state, dropped_words / dropped_sets = what cleaning removed."""

    def __init__(self, entries, word2idx, vocab_size, bos, eos, width=0):
        self.by_id, self.default, self.dropped_words, self.dropped_sets = {}, [], 0, 0
        if not isinstance(entries, dict):
            raise ValueError("constraints: the file must hold a JSON object {image_id: [[word, ...], ...]}")
        for key, sets in entries.items():
            clean = self._clean(key, sets, word2idx, int(vocab_size), (int(bos), int(eos)))
            if key == "*":
                self.default = clean
            else:
                self.by_id[str(key)] = clean
        self.C = max([len(s) for s in self.by_id.values()] + [len(self.default)])
        width = int(width)
        if width < 0:
            raise ValueError("constraints: beams per state must be >= 0 (0 = the largest that fits; got %d)" % width)
        if width and (width << self.C) > MAX_ROWS:
            raise ValueError("constraints: %d beams per state x 2^%d states exceed %d rows per image" % (width, self.C, MAX_ROWS))
        self.width = width or (MAX_ROWS >> self.C)

    def _clean(self, key, sets, word2idx, V, special):
        if not isinstance(sets, list) or not all(isinstance(st, list) for st in sets):
            raise ValueError("constraints: entry %r must be a list of word lists" % (key,))
        out, seen = [], set()
        for st in sets:
            ids = []
            for word in st:
                if isinstance(word, bool) or not isinstance(word, (int, str)):
                    raise ValueError("constraints: entry %r: a word must be a string or an integer id (got %r)" % (key, word))
                v = lookup_word(word, word2idx, V, special)
                if v is None:
                    self.dropped_words += 1
                    continue
                if int(v) in ids:
                    continue
                if int(v) in seen:
                    raise ValueError("constraints: entry %r: word %r appears in two sets (sets must be disjoint)" % (key, word))
                ids.append(int(v))
            if not ids:
                self.dropped_sets += 1
                continue
            if len(ids) > MAX_WORDS:
                raise ValueError("constraints: entry %r has a set of %d words (at most %d)" % (key, len(ids), MAX_WORDS))
            seen.update(ids)
            out.append(ids)
        if len(out) > MAX_SETS:
            raise ValueError("constraints: entry %r has %d sets (at most %d)" % (key, len(out), MAX_SETS))
        return out

    def for_images(self, image_ids):
        """per image its sets of token ids (copies)"""
        return [[list(st) for st in self.by_id.get(str(i), self.default)] for i in image_ids]

    def summary(self):
        return "constraints: %d image entries%s, at most %d sets per image, %d beams per state; dropped %d unknown words and %d emptied sets" % (
            len(self.by_id), " and a default" if self.default else "", self.C, self.width, self.dropped_words, self.dropped_sets)


def load_constraints(path, word2idx, vocab_size, bos, eos, width=0):
    """--constraints FILE (+ --cbs_width W) -> Constraints; ValueError for a malformed file, too many or too large sets, overlapping sets
    or an explicit width with width << C > 16."""
    with open(path) as fh:
        entries = json.load(fh)
    return Constraints(entries, word2idx, vocab_size, bos, eos, width)


def parse_must_include(text, word2idx, vocab_size, bos, eos):
    """gen_caption.py --must_include "dog,puppy;frisbee": ';' separates sets, ',' words -> Constraints with that default entry"""
    sets = [[w.strip() for w in part.split(",") if w.strip()] for part in text.split(";") if part.strip()]
    return Constraints({"*": sets}, word2idx, vocab_size, bos, eos)
