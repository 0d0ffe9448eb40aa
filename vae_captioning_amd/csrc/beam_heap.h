// What the beam-search bookkeeping kernels share (beam.hip, beam_groups.hip, beam_constrained.hip; the init loops also sbs.hip):
//   - arrays spread over the lanes of a wave, and WaveHeap: a TopN heap of one image held in the registers of one wave;
//   - CPython's heapq sift moves and the TopN.push rule, written once for every heap type;
//   - BeamArgs, the kernels' argument block, with its host-side filler and null check;
//   - beam_candidate: the arithmetic of one candidate (decoder.py:279/282);
//   - BeamBank: the pair of TopN heaps of one (virtual) image for one round with its caption pool -- open / push / close (beam.hip's
//     general kernel; the group and constrained kernels keep their own copy of these steps, see their headers);
//   - beam_rows_init: the start of every beam row (the LSTM state of its image, <BOS>).
#pragma once
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int BEAM_MAX = 16;

struct BeamItem {
    double score, logprob;
    int parent, tok, len, slot;
    __device__ __forceinline__ int leaving() const { return slot; }   // what TopN.push reports of an item that leaves: its pool slot
};

// ---- a value that every lane of the wave holds alike, and arrays spread over the lanes (element p in lane p)
__device__ __forceinline__ int lane_get(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int lane_set(int old, int l, int x) { return (int)threadIdx.x == l ? x : old; }   // (x: the same in every lane)
__device__ __forceinline__ double lane_get(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double lane_set(double old, int l, double x) {
    return (int)threadIdx.x == l ? x : old;
}

// A TopN heap of one image IN REGISTERS: one wave works on one image, and heap position p is lane p of six registers.  The walk below
// is sequential (heapq's sift order decides ties) and every lane runs it alike; `heap[pos]` with the wave-uniform pos is a
// v_readlane / a one-lane select -- a few cycles -- where the LDS heaps of rounds 4-6 paid one ~120-cycle round trip per dependent access,
// ~20 of them per push (1.2 us per candidate, 33-40 us per round at beam 5: the longest latency-bound kernel of a decode round).
struct WaveHeap {
    double sc, lp;
    int par, tok, len, slot;
    __device__ __forceinline__ BeamItem get(int pos) const {
        BeamItem it;
        it.score = lane_get(sc, pos); it.logprob = lane_get(lp, pos);
        it.parent = lane_get(par, pos); it.tok = lane_get(tok, pos); it.len = lane_get(len, pos); it.slot = lane_get(slot, pos);
        return it;
    }
    __device__ __forceinline__ void put(int pos, const BeamItem& it) {
        sc = lane_set(sc, pos, it.score); lp = lane_set(lp, pos, it.logprob);
        par = lane_set(par, pos, it.parent); tok = lane_set(tok, pos, it.tok); len = lane_set(len, pos, it.len); slot = lane_set(slot, pos, it.slot);
    }
    __device__ __forceinline__ void move(int dst, int src) { put(dst, get(src)); }   // heap[dst] = heap[src]
    __device__ __forceinline__ double score(int pos) const { return lane_get(sc, pos); }
};

// CPython Lib/heapq.py _siftdown / _siftup, move for move (comparisons by score only), for any heap that has score(pos), get(pos),
// move(dst, src) and put(pos, item) (WaveHeap of BeamItem; beam.hip's SlimHeap of (score, id) pairs).  `newitem` is the item heapq has
// just stored at `pos` (heappush: appended at the end; heappushpop: written over the root): it is carried in scalars and stored once,
// where it settles.
template <class Heap, class Item>
__device__ __forceinline__ void sift_down(Heap& heap, int startpos, int pos, const Item& newitem) {
    while (pos > startpos) {
        const int parentpos = (pos - 1) >> 1;
        if (newitem.score < heap.score(parentpos)) {
            heap.move(pos, parentpos);
            pos = parentpos;
            continue;
        }
        break;
    }
    heap.put(pos, newitem);
}

template <class Heap, class Item>
__device__ __forceinline__ void sift_up(Heap& heap, int n, int pos, const Item& newitem) {
    const int startpos = pos;
    int childpos = 2 * pos + 1;
    while (childpos < n) {
        const int rightpos = childpos + 1;
        if (rightpos < n && !(heap.score(childpos) < heap.score(rightpos))) childpos = rightpos;
        heap.move(pos, childpos);
        pos = childpos;
        childpos = 2 * pos + 1;
    }
    sift_down(heap, startpos, pos, newitem);
}

// TopN.push: returns leaving() of the item that left the heap (the popped root, or the rejected newcomer), -1 if none
template <class Heap, class Item>
__device__ __forceinline__ int topn_push(Heap& heap, int& count, int cap, const Item& item) {
    if (count < cap) {
        ++count;
        sift_down(heap, 0, count - 1, item);
        return -1;
    }
    if (count > 0 && heap.score(0) < item.score) {
        const int out = heap.get(0).leaving();
        sift_up(heap, count, 0, item);
        return out;
    }
    return item.leaving();
}

struct BeamArgs {
    int B, n, k, Lmax, eos;
    double len_norm_f;
    const float* tv;
    const int32_t* ti;
    int32_t *pcount, *ccount, *p_len, *c_len, *c_slot, *c_free;
    double *p_score, *p_logprob, *c_score, *c_logprob;
    const int32_t* sent_cur;
    int32_t *sent_next, *c_sent, *parent, *tok;
};

// the entry points' arguments as the kernels' block (the state pointers in the order every vc_beam_* prototype lists them)
inline BeamArgs beam_args(int B, int n, int k, int Lmax, int eos, double len_norm_f, const float* tv, const int32_t* ti, int32_t* pcount,
                          int32_t* ccount, double* p_score, double* p_logprob, int32_t* p_len, const int32_t* sent_cur, int32_t* sent_next,
                          double* c_score, double* c_logprob, int32_t* c_len, int32_t* c_slot, int32_t* c_free, int32_t* c_sent,
                          int32_t* parent, int32_t* tok) {
    BeamArgs a;
    a.B = B; a.n = n; a.k = k; a.Lmax = Lmax; a.eos = eos; a.len_norm_f = len_norm_f;
    a.tv = tv; a.ti = ti; a.pcount = pcount; a.ccount = ccount; a.p_len = p_len; a.c_len = c_len; a.c_slot = c_slot;
    a.c_free = c_free; a.p_score = p_score; a.p_logprob = p_logprob; a.c_score = c_score; a.c_logprob = c_logprob;
    a.sent_cur = sent_cur; a.sent_next = sent_next; a.c_sent = c_sent; a.parent = parent; a.tok = tok;
    return a;
}

inline bool beam_state_given(const BeamArgs& a) {   // every state pointer is set (tv / ti are the caller's to check)
    return a.pcount && a.ccount && a.p_score && a.p_logprob && a.p_len && a.sent_cur && a.sent_next && a.c_score && a.c_logprob && a.c_len &&
           a.c_slot && a.c_free && a.c_sent && a.parent && a.tok;
}

// One candidate: a beam (running log-probability p_logprob, p_len words so far) extended by the word `tok` of probability p.
struct BeamCand {
    double lp;      // decoder.py:282: np.log of a float32 is a float32; the SUM is a float64
    double score;   // what a finished caption is ranked by: lp / len**len_norm_f if tok is <EOS> (and len_norm_f > 0), else lp
    int skip;       // decoder.py:279: float32 p against the Python float 1e-12
};
__device__ __forceinline__ BeamCand beam_candidate(const BeamArgs& a, double p_logprob, int p_len, float p, int tok) {
    BeamCand c;
    c.lp = p_logprob + (double)logf(p);
    c.score = c.lp;
    if (tok == a.eos && a.len_norm_f > 0) c.score = c.lp / pow((double)(p_len + 1), a.len_norm_f);
    c.skip = (double)p < 1e-12 ? 1 : 0;
    return c;
}

// rows of virtual image v that stay empty this round: continue the image's first row with token 0 (ignored)
__device__ __forceinline__ void beam_next_defaults(const BeamArgs& a, long v) {
    if ((int)threadIdx.x < a.n) {
        a.parent[v * a.n + threadIdx.x] = (int)(v * a.n);
        a.tok[v * a.n + threadIdx.x] = 0;
    }
}

// The bank of virtual image v for one round: its `partial` heap (rebuilt from empty) and `complete` heap (carried over), the free mask
// of its pool of n + 1 caption slots, and per pool slot (lane s) the caption recorded for it this round.  A kept beam's sentence and a
// finished caption are only RECORDED during the walk (parent + last word); close() copies the tokens with the 64 lanes.  A slot freed
// and taken again within the round keeps its last writer's record, which is the caption the sequential code left there.
struct BeamBank {
    WaveHeap part{0.0, 0.0, 0, 0, 0, -1}, comp{0.0, 0.0, 0, 0, 0, -1};
    int hn = 0, cn = 0, freemask = 0;
    int rec_src = 0, rec_len0 = -1, rec_tok = 0;   // lane s: the caption recorded for pool slot s this round (len0 < 0: none)

    __device__ __forceinline__ void open(const BeamArgs& a, long v, int cn_, int freemask_) {
        const int lane = threadIdx.x;
        cn = cn_;
        freemask = freemask_;
        if (lane < cn) {
            const long o = v * a.n + lane;
            comp.sc = a.c_score[o];
            comp.lp = a.c_logprob[o];
            comp.len = a.c_len[o];
            comp.slot = a.c_slot[o];
        }
    }

    // one candidate of the walk (wave-uniform arguments): `parent` is the row it extends, relative to close()'s parent_base and cur
    __device__ __forceinline__ void push(const BeamArgs& a, int tok, int parent, int len0, double lp, double score) {
        BeamItem it;
        it.tok = tok;
        it.parent = parent;
        it.len = len0 + 1;
        it.logprob = lp;
        it.score = score;
        it.slot = -1;
        if (tok == a.eos) {
            // take a free pool slot, record the caption for it, give the slot back if the heap does not keep it
            const int s = __builtin_ctz(freemask);
            freemask &= ~(1 << s);
            it.slot = s;
            rec_src = lane_set(rec_src, s, parent); rec_len0 = lane_set(rec_len0, s, len0); rec_tok = lane_set(rec_tok, s, tok);
            const int freed = topn_push(comp, cn, a.n, it);
            if (freed >= 0) freemask |= 1 << freed;
        } else {
            topn_push(part, hn, a.n, it);
        }
    }

    // the heaps and counters back to the state; then the copies, from the rows at `cur` (row i of it is parent i).  Both copy loops stop
    // at Lmax: a no-op for every state the host code produces (it runs at most Lmax - 1 rounds, so a caption's last word lands at
    // index <= Lmax - 1), a bound for a state it did not.
    __device__ __forceinline__ void close(const BeamArgs& a, long v, int parent_base, const int32_t* cur) {
        const int lane = threadIdx.x, n = a.n, L = a.Lmax;
        if (lane < hn) {
            const long o = v * n + lane;
            a.p_score[o] = part.sc;
            a.p_logprob[o] = part.lp;
            a.p_len[o] = part.len;
            a.parent[o] = parent_base + part.par;
            a.tok[o] = part.tok;
        }
        if (lane < cn) {
            const long o = v * n + lane;
            a.c_score[o] = comp.sc;
            a.c_logprob[o] = comp.lp;
            a.c_len[o] = comp.len;
            a.c_slot[o] = comp.slot;
        }
        if (lane == 0) {
            a.pcount[v] = hn;
            a.ccount[v] = cn;
            a.c_free[v] = freemask;
        }
        for (int s = 0; s <= n; ++s) {   // finished captions, per pool slot
            const int len0 = lane_get(rec_len0, s);
            if (len0 < 0) continue;
            const int i = lane_get(rec_src, s), tk = lane_get(rec_tok, s);
            int32_t* dst = a.c_sent + (v * (n + 1) + s) * L;
            for (int t = lane; t <= len0 && t < L; t += 64) dst[t] = t < len0 ? cur[i * L + t] : tk;
        }
        int32_t* nxt = a.sent_next + v * n * L;
        for (int j = 0; j < hn; ++j) {   // live beams, per heap position
            const int len = lane_get(part.len, j), src = lane_get(part.par, j), tk = lane_get(part.tok, j);
            for (int t = lane; t < len && t < L; t += 64) nxt[j * L + t] = t < len - 1 ? cur[src * L + t] : tk;
        }
    }
};

// vae_model/decoder.py:238-247 for every image at once, the part every search with n rows per image starts from: the image's LSTM
// state in each of its rows, <BOS> as every row's sentence, an empty next-round buffer.  (t0, stride): the caller's grid-stride loop.
__device__ __forceinline__ void beam_rows_init(long M, int n, int Lmax, int H, int bos, long t0, long stride, const float* __restrict__ c_in,
                                               const float* __restrict__ h_in, float* __restrict__ c_out, float* __restrict__ h_out,
                                               int32_t* __restrict__ sent_cur, int32_t* __restrict__ sent_next) {
    for (long i = t0; i < M * H; i += stride) {
        const long src = (i / H) / n * H + i % H;
        c_out[i] = c_in[src];
        h_out[i] = h_in[src];
    }
    for (long i = t0; i < M * Lmax; i += stride) {
        sent_cur[i] = bos;
        sent_next[i] = 0;
    }
}

}  // namespace vc
