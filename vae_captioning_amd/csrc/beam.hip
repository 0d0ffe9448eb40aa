// Beam-search bookkeeping on device (vae_model/decoder.py:238-300 + utils/top_n.py:4-43).
//
// One wave per image replays, for its image, exactly what the reference's Python does after every
// decoder step: walk the image's live beams in the order TopN.extract() returned them (the heap ARRAY order),
// walk each beam's top-`beam_size` words in descending probability, skip p < 1e-12, and push the extended
// caption into the image's `complete` (word == <EOS>, score = logprob / len**len_norm_f) or `partial`
// (score = logprob) TopN.  TopN is a min-heap keyed by score only, driven with heapq's heappush /
// heappushpop; ties are therefore resolved by heapq's sift order, which this file reproduces move for move
// (CPython Lib/heapq.py: _siftdown, _siftup).  Each word's log-probability is a float32 log (np.log of a float32
// probability), accumulated in double like the reference's Python / numpy float64 sums.
//
// Nothing here needs the host between decoder steps: the kernel also emits, for the next step, each new
// beam's parent row (whose LSTM state it continues) and its last token.
#include "beam_heap.h"

namespace vc {

// One wave per image.  Per round:
//   1. in parallel, lane q prepares candidate q (beam q / k, its j-th word): float32 log of the word's probability added to the beam's
//      float64 running sum, the length-normalised score if the word is <EOS> -- the transcendental work of the whole round at once;
//   2. the walk over the candidates in the reference's order (beams in heap-array order, words by descending probability), heaps in
//      registers (WaveHeap): a kept beam's sentence and a finished caption are only RECORDED (parent + last word; per pool slot);
//   3. the token copies by the 64 lanes: each kept beam's sentence into the next round's buffer, each recorded caption into its pool
//      slot (a slot freed and taken again within the round keeps its last writer's record, which is the caption the sequential
//      code left there).
__global__ __launch_bounds__(64) void beam_update_kernel(BeamArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.n, k = a.k;
    const int np = __builtin_amdgcn_readfirstlane(a.pcount[b]);
    beam_next_defaults(a, b);
    if (np == 0) return;   // every beam of this image has ended
    BeamBank bank;
    bank.open(a, b, __builtin_amdgcn_readfirstlane(a.ccount[b]), __builtin_amdgcn_readfirstlane(a.c_free[b]));
    const int total = np * k;
    for (int base = 0; base < total; base += 64) {
        // ---- 1. candidate base + lane
        const int q = base + lane;
        const bool have = q < total;
        const long row = (long)b * n + (have ? q / k : 0);
        const int tok_q = have ? a.ti[(long)b * n * k + q] : 0;
        const int len0_q = a.p_len[row];
        const BeamCand cd = beam_candidate(a, a.p_logprob[row], len0_q, have ? a.tv[(long)b * n * k + q] : 0.f, tok_q);
        const int skip_q = have ? cd.skip : 1;
        // ---- 2. the walk
        const int cnt = total - base < 64 ? total - base : 64;
        for (int c = 0; c < cnt; ++c) {
            if (lane_get(skip_q, c)) continue;
            bank.push(a, lane_get(tok_q, c), (base + c) / k, lane_get(len0_q, c), lane_get(cd.lp, c), lane_get(cd.score, c));
        }
    }
    // ---- 3. the stores and the copies
    bank.close(a, b, b * n, a.sent_cur + (long)b * n * a.Lmax);
}

// ---- beam x beam <= 64 (beam <= 8): every candidate of the round has a lane of its own for the whole kernel, so the heaps hold
// (score, id) PAIRS -- three registers per move instead of eight -- and an item's other fields are read where they already are: id < 64
// is candidate id (lane id of the registers step 1 filled), id >= 64 a complete caption carried in from earlier rounds (lane id - 64 of
// the registers loaded from c_*).  Same pushes, same sift moves, same order; what leaves the kernel is gathered by id at the end.
struct SlimItem {
    double score;
    int id;
    __device__ __forceinline__ int leaving() const { return id; }   // what TopN.push reports of an item that leaves: its id
};

struct SlimHeap {   // (beam_heap.h's sifts and topn_push work on it as on WaveHeap)
    double sc;
    int id;
    __device__ __forceinline__ double score(int pos) const { return lane_get(sc, pos); }
    __device__ __forceinline__ SlimItem get(int pos) const { return SlimItem{lane_get(sc, pos), lane_get(id, pos)}; }
    __device__ __forceinline__ void put(int pos, const SlimItem& it) { sc = lane_set(sc, pos, it.score); id = lane_set(id, pos, it.id); }
    __device__ __forceinline__ void move(int dst, int src) { put(dst, get(src)); }   // heap[dst] = heap[src]
};

__global__ __launch_bounds__(64) void beam_update_slim_kernel(BeamArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.n, k = a.k, L = a.Lmax;
    const int np = __builtin_amdgcn_readfirstlane(a.pcount[b]);
    beam_next_defaults(a, b);
    if (np == 0) return;   // every beam of this image has ended
    int hn = 0, cn = __builtin_amdgcn_readfirstlane(a.ccount[b]);
    // complete captions carried in (lane j < cn): they start as the complete heap, ids 64 + j
    double cc_lp = 0.0;
    int cc_len = 0, cc_slot = -1;
    SlimHeap part{0.0, 0}, comp{0.0, 0};
    if (lane < cn) {
        comp.sc = a.c_score[b * n + lane];
        comp.id = 64 + lane;
        cc_lp = a.c_logprob[b * n + lane];
        cc_len = a.c_len[b * n + lane];
        cc_slot = a.c_slot[b * n + lane];
    }
    int freemask = __builtin_amdgcn_readfirstlane(a.c_free[b]);
    // ---- 1. candidate `lane`: beam lane / k, its (lane % k)-th word
    const int total = np * k;
    const bool have = lane < total;
    const long row = (long)b * n + (have ? lane / k : 0);
    const int tok_q = have ? a.ti[(long)b * n * k + lane] : 0;
    const int len0_q = a.p_len[row];
    const BeamCand cd = beam_candidate(a, a.p_logprob[row], len0_q, have ? a.tv[(long)b * n * k + lane] : 0.f, tok_q);
    const double lp_q = cd.lp;
    const int skip_q = have ? cd.skip : 1;
    int slot_q = -1;     // pool slot of candidate `lane`, if it is a finished caption the walk gave one
    int rec_cand = -1;   // lane s: the candidate whose caption pool slot s receives this round (-1: none)
    // ---- 2. the walk
    for (int c = 0; c < total; ++c) {
        if (lane_get(skip_q, c)) continue;
        const SlimItem it{lane_get(cd.score, c), c};
        if (lane_get(tok_q, c) == a.eos) {
            // take a free pool slot, record the caption for it, give the slot back if the heap does not keep it
            const int sl = __builtin_ctz(freemask);
            freemask &= ~(1 << sl);
            slot_q = lane_set(slot_q, c, sl);
            rec_cand = lane_set(rec_cand, sl, c);
            const int out = topn_push(comp, cn, n, it);
            if (out >= 0) freemask |= 1 << (out < 64 ? lane_get(slot_q, out) : lane_get(cc_slot, out - 64));
        } else {
            topn_push(part, hn, n, it);
        }
    }
    // ---- what the heaps hold, gathered by id (lane j: heap position j)
    {   // (the exchanges run with every lane active; the stores are per heap position)
        const int id = lane < hn ? part.id : 0;
        const double lp = __shfl(lp_q, id, 64);
        const int len0 = __shfl(len0_q, id, 64), tk = __shfl(tok_q, id, 64);
        if (lane < hn) {
            const long o = (long)b * n + lane;
            a.p_score[o] = part.sc;
            a.p_logprob[o] = lp;
            a.p_len[o] = len0 + 1;
            a.parent[o] = b * n + id / k;
            a.tok[o] = tk;
        }
    }
    {
        const int id = lane < cn ? comp.id : 0;
        const int cq = id < 64 ? id : 0, cj = id < 64 ? 0 : id - 64;
        const double lp_new = __shfl(lp_q, cq, 64), lp_old = __shfl(cc_lp, cj, 64);
        const int len_new = __shfl(len0_q, cq, 64) + 1, len_old = __shfl(cc_len, cj, 64);
        const int slot_new = __shfl(slot_q, cq, 64), slot_old = __shfl(cc_slot, cj, 64);
        if (lane < cn) {
            const long o = (long)b * n + lane;
            a.c_score[o] = comp.sc;
            a.c_logprob[o] = id < 64 ? lp_new : lp_old;
            a.c_len[o] = id < 64 ? len_new : len_old;
            a.c_slot[o] = id < 64 ? slot_new : slot_old;
        }
    }
    if (lane == 0) {
        a.pcount[b] = hn;
        a.ccount[b] = cn;
        a.c_free[b] = freemask;
    }
    // ---- 3. the copies
    const int32_t* cur = a.sent_cur + (long)b * n * L;
    for (int sl = 0; sl <= n; ++sl) {   // finished captions, per pool slot
        const int c = lane_get(rec_cand, sl);
        if (c < 0) continue;
        const int len0 = lane_get(len0_q, c), i = c / k;
        int32_t* dst = a.c_sent + ((long)b * (n + 1) + sl) * L;
        for (int t = lane; t <= len0 && t < L; t += 64) dst[t] = t < len0 ? cur[i * L + t] : a.eos;
    }
    int32_t* nxt = a.sent_next + (long)b * n * L;
    for (int j = 0; j < hn; ++j) {
        const int id = lane_get(part.id, j);
        const int len = lane_get(len0_q, id) + 1, src = id / k, tk = lane_get(tok_q, id);
        for (int t = lane; t < len && t < L; t += 64) nxt[j * L + t] = t < len - 1 ? cur[src * L + t] : tk;
    }
}

// vae_model/decoder.py:238-247 for every image at once: the state the first round's vc_beam_update reads (twenty fills, two state
// gathers and two index ramps as torch / library launches before: ~0.2 ms of a 5 ms call at 128 images)
__global__ __launch_bounds__(256) void beam_init_kernel(BeamArgs a, int bos, int H, const float* __restrict__ c_in, const float* __restrict__ h_in,
                                                        float* __restrict__ c_out, float* __restrict__ h_out, int32_t* __restrict__ sent_cur) {
    const long M = (long)a.B * a.n, stride = (long)gridDim.x * 256, t0 = (long)blockIdx.x * 256 + threadIdx.x;
    beam_rows_init(M, a.n, a.Lmax, H, bos, t0, stride, c_in, h_in, c_out, h_out, sent_cur, a.sent_next);
    for (long i = t0; i < (long)a.B * (a.n + 1) * a.Lmax; i += stride) a.c_sent[i] = 0;
    for (long i = t0; i < M; i += stride) {
        a.p_score[i] = 0.0; a.p_logprob[i] = 0.0; a.p_len[i] = 1;
        a.c_score[i] = 0.0; a.c_logprob[i] = 0.0; a.c_len[i] = 0; a.c_slot[i] = 0;
        a.parent[i] = (int)i; a.tok[i] = bos;
    }
    for (long i = t0; i < a.B; i += stride) {
        a.pcount[i] = 1; a.ccount[i] = 0; a.c_free[i] = (1 << (a.n + 1)) - 1;
    }
}

// greedy / sampled decoding (vae_model/decoder.py:186-194: the loop ends at the stop word): done[b] |= (tok[b] == eos); pending[0] = rows not done
// yet.  One workgroup; lets a captured chunk of decoder steps report "has every image emitted <EOS>" in 4 bytes.
__global__ __launch_bounds__(256) void eos_track_kernel(const int32_t* __restrict__ tok, int B, int eos, int32_t* __restrict__ done,
                                                        float* __restrict__ pending) {
    __shared__ float sh[4];
    float open = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const int d = done[b] | (tok[b] == eos ? 1 : 0);
        done[b] = d;
        open += d ? 0.f : 1.f;
    }
    open = block_sum<256>(open, sh);
    if (threadIdx.x == 0) pending[0] = open;
}

}  // namespace vc

extern "C" int vc_eos_track_i32(void* stream, const int32_t* tok, int B, int eos, int32_t* done, float* pending) {
    using namespace vc;
    VC_CHECK_ARG(tok && done && pending && B > 0, "bad argument");
    hipLaunchKernelGGL(eos_track_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, tok, B, eos, done, pending);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_beam_init(void* stream, int B, int beam, int Lmax, int bos, int H, const float* c_in, const float* h_in, float* c_out,
                            float* h_out, int32_t* pcount, int32_t* ccount, double* p_score, double* p_logprob, int32_t* p_len,
                            int32_t* sent_cur, int32_t* sent_next, double* c_score, double* c_logprob, int32_t* c_len, int32_t* c_slot,
                            int32_t* c_free, int32_t* c_sent, int32_t* parent, int32_t* tok) {
    using namespace vc;
    VC_CHECK_ARG(B > 0 && beam > 0 && beam <= BEAM_MAX && Lmax > 1 && H > 0, "beam size must be 1..16");
    const BeamArgs a = beam_args(B, beam, beam, Lmax, 0, 0, nullptr, nullptr, pcount, ccount, p_score, p_logprob, p_len, sent_cur, sent_next, c_score,
                                 c_logprob, c_len, c_slot, c_free, c_sent, parent, tok);
    VC_CHECK_ARG(c_in && h_in && c_out && h_out && beam_state_given(a), "null pointer");
    const long work = (long)B * beam * (H > Lmax ? H : Lmax);
    hipLaunchKernelGGL(beam_init_kernel, dim3((unsigned)(cdiv(work, 256L) < 1024 ? cdiv(work, 256L) : 1024)), dim3(256), 0, (hipStream_t)stream,
                       a, bos, H, c_in, h_in, c_out, h_out, sent_cur);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_beam_update(void* stream, int B, int beam, int Lmax, int eos, double len_norm_f, const float* top_p,
                              const int32_t* top_i, int32_t* pcount, int32_t* ccount, double* p_score, double* p_logprob,
                              int32_t* p_len, const int32_t* sent_cur, int32_t* sent_next, double* c_score, double* c_logprob,
                              int32_t* c_len, int32_t* c_slot, int32_t* c_free, int32_t* c_sent, int32_t* parent, int32_t* tok) {
    using namespace vc;
    VC_CHECK_ARG(B > 0 && beam > 0 && beam <= BEAM_MAX && Lmax > 1, "beam size must be 1..16");
    const BeamArgs a = beam_args(B, beam, beam, Lmax, eos, len_norm_f, top_p, top_i, pcount, ccount, p_score, p_logprob, p_len, sent_cur, sent_next,
                                 c_score, c_logprob, c_len, c_slot, c_free, c_sent, parent, tok);
    VC_CHECK_ARG(top_p && top_i && beam_state_given(a), "null pointer");
    if (beam * beam <= 64) hipLaunchKernelGGL(beam_update_slim_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(beam_update_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    VC_LAUNCH_CHECK();
    return 0;
}
