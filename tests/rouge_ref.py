"""Plain-Python reference of ROUGE-L (tests only), written from the definitions: words = token ids without <BOS>, <EOS> and PAD;
LCS(a, b) = the length of the longest common subsequence by the quadratic dynamic programme.  Against a range of reference rows a
hypothesis gets three integers: the largest LCS, and the (LCS, words) pair of the row with the largest LCS / words among the rows
with at least one word -- ratios compared by integer cross-multiplication, a tie going to the shorter row; all 0 when no row has a
word.  coco-caption's score: P = lcs_max / hyp_len, R = rec_lcs / rec_len, (1 + beta^2) P R / (R + beta^2 P) with beta = 1.2, 0.0 when
hyp_len, rec_len or either LCS is 0.  Nothing here imports the product's arithmetic."""
import numpy as np

from . import consensus_ref as cref

words = cref.words
MASK = (1 << 64) - 1


def lcs(a, b):
    """length of the longest common subsequence of two sequences: the quadratic dynamic programme, one row at a time"""
    row = [0] * (len(a) + 1)
    for y in b:
        prev = 0                                   # the cell up-left of the one being written
        for i, x in enumerate(a):
            keep = row[i + 1]
            row[i + 1] = prev + 1 if x == y else max(row[i + 1], row[i])
            prev = keep
    return row[len(a)]


def lcs_bitparallel(a, b):
    """the same length by the bit-parallel recurrence (Crochemore et al. 2001, Hyyro 2004) on Python ints masked to 64 bits, for
    len(a) <= 64.  Bit i of V belongs to a[i]; V starts as all ones.  For each y of b, M = the mask of the positions of a that hold y
    (positions at and past len(a) never match), U = V & M, V = (V + U) | (V - U) modulo 2^64: the carry out of bit 63 is dropped.  A
    zero bit of V marks a position where the LCS of a[:i + 1] with the consumed part of b is one longer than that of a[:i], so the
    length is the number of zero bits among the low len(a) bits.  The low mask of 64 positions is all ones, not (1 << 64) - 1 taken
    in 64-bit arithmetic (where the shift is no shift)."""
    n = len(a)
    assert n <= 64
    low = MASK if n == 64 else (1 << n) - 1
    V = MASK
    for y in b:
        M = 0
        for i, x in enumerate(a):
            if x == y:
                M |= 1 << i
        M &= low
        U = V & M
        V = (((V + U) & MASK) | ((V - U) & MASK)) & MASK
    return n - bin(V & low).count("1")


def overlap(c_rows, r_rows, lo, hi, skip):
    """c_rows / r_rows: word lists; hypothesis c against r_rows[lo[c]:hi[c]] without row skip[c] -> per hypothesis (lcs_max, rec_lcs,
    rec_len)"""
    out = []
    for c, h in enumerate(c_rows):
        best_max, best = 0, None
        for r in range(max(lo[c], 0), min(hi[c], len(r_rows))):
            if r == skip[c] or not r_rows[r]:
                continue
            l, n = lcs(h, r_rows[r]), len(r_rows[r])
            best_max = max(best_max, l)
            if best is None or l * best[1] > best[0] * n or (l * best[1] == best[0] * n and n < best[1]):
                best = (l, n)
        out.append((best_max,) + (best or (0, 0)))
    return out


def rouge_l(lcs_max, rec_lcs, rec_len, hyp_len, beta=1.2):
    """one caption's score from its four integers, in float64, in the order the definition is written"""
    if not (lcs_max and rec_lcs and rec_len and hyp_len):
        return 0.0
    P = lcs_max / hyp_len
    R = rec_lcs / rec_len
    return (1 + beta ** 2) * P * R / (R + beta ** 2 * P)


def scores(cands, refs, bos, eos):
    """per image a float64 array: each caption's ROUGE-L against the image's references"""
    out = []
    for cs, rs in zip(cands, refs):
        cw, rw = [words(c, bos, eos) for c in cs], [words(r, bos, eos) for r in rs]
        o = overlap(cw, rw, [0] * len(cw), [len(rw)] * len(cw), [-1] * len(cw))
        out.append(np.array([rouge_l(*o[i], len(cw[i])) for i in range(len(cw))], np.float64))
    return out


def _mean(x):
    return float(np.mean(x)) if len(x) else 0.0


def evaluate_rouge(cands, refs, bos, eos):
    """-> (rouge_l: mean over the images that list a caption of the first caption's score, oracle_rouge_l: mean over the same images
    of the best score of the list, mean_rouge_l: mean over all captions, the per-caption scores per image)"""
    sc = scores(cands, refs, bos, eos)
    return _mean([s[0] for s in sc if len(s)]), _mean([s.max() for s in sc if len(s)]), _mean([v for s in sc for v in s]), sc
