// What the beam-search bookkeeping kernels share (beam.hip, beam_groups.hip): a TopN heap of one image held in the registers of
// one wave, CPython's heapq sift moves on it, and the kernels' argument block.
#pragma once
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int BEAM_MAX = 16;

struct BeamItem {
    double score, logprob;
    int parent, tok, len, slot;
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
    __device__ __forceinline__ double score(int pos) const { return lane_get(sc, pos); }
};

// CPython Lib/heapq.py _siftdown / _siftup, move for move (comparisons by score only).  `newitem` is the item heapq has just stored at
// `pos` (heappush: appended at the end; heappushpop: written over the root): it is carried in scalars and stored once, where it settles.
__device__ __forceinline__ void sift_down(WaveHeap& heap, int startpos, int pos, const BeamItem& newitem) {
    while (pos > startpos) {
        const int parentpos = (pos - 1) >> 1;
        if (newitem.score < heap.score(parentpos)) {
            heap.put(pos, heap.get(parentpos));
            pos = parentpos;
            continue;
        }
        break;
    }
    heap.put(pos, newitem);
}

__device__ __forceinline__ void sift_up(WaveHeap& heap, int n, int pos, const BeamItem& newitem) {
    const int startpos = pos;
    int childpos = 2 * pos + 1;
    while (childpos < n) {
        const int rightpos = childpos + 1;
        if (rightpos < n && !(heap.score(childpos) < heap.score(rightpos))) childpos = rightpos;
        heap.put(pos, heap.get(childpos));
        pos = childpos;
        childpos = 2 * pos + 1;
    }
    sift_down(heap, startpos, pos, newitem);
}

// TopN.push: returns the slot field of the item that left the heap (the popped root, or the rejected newcomer), -1 if none
__device__ __forceinline__ int topn_push(WaveHeap& heap, int& count, int cap, const BeamItem& item) {
    if (count < cap) {
        ++count;
        sift_down(heap, 0, count - 1, item);
        return -1;
    }
    if (count > 0 && heap.score(0) < item.score) {
        const int freed = lane_get(heap.slot, 0);
        sift_up(heap, count, 0, item);
        return freed;
    }
    return item.slot;
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

}  // namespace vc
