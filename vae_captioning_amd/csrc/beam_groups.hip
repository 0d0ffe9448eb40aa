// Group ("diverse") beam search bookkeeping on device: Diverse Beam Search (Vijayakumar et al. 2016) with the Hamming
// dissimilarity, on the TopN semantics of beam.hip.
//
// An image has G groups; group g is a beam search of width w of its own (a pair of TopN heaps), laid out as "virtual image"
// v = b*G + g of vc_beam_update's state.  All groups advance in lock step; within a round they run IN ORDER, and a word that c
// live beams of the round's earlier groups have just taken costs a candidate lambda * c of its heap key:
//
//   chosen = []
//   for g in 0..G-1:
//       for beam in partial[g].extract():                      (heap ARRAY order)
//           cand = the kc = min(G*w, V) most probable words of the beam's row, descending, stable
//           lp   = beam.logprob + float64(float32 log p)        (vc_beam_update's expression)
//           key  = lp if c == 0 else lp - lambda * c            (c = chosen.count(word); product and difference each rounded)
//           the first w of cand under (key descending, raw rank ascending), in that order:
//               skip if p < 1e-12
//               <EOS>: complete[g].push(score = lp / len**len_norm_f)       (never penalised)
//               else : partial[g].push(logprob = lp, score = key)
//       chosen += last words of partial[g]'s heap array
//
// The stored logprob is always the model's; the penalty lives in a live beam's key for the round it was chosen in and is not
// accumulated.  The kc = G*w best raw words are enough: at most (G-1)*w distinct words are penalised, so at least w of the kc are
// not, their key is their raw value (>= anything outside the list), and they come earlier in rank.
//
// One wave per IMAGE; its G groups run one after the other inside the wave.  A group's candidates are prepared in blocks of
// floor(64 / kc) whole rows (a lane per candidate, a row never split between blocks), so a candidate's position within its row is a
// rank count over its row's kc keys by shuffles, in parallel, before the sequential walk.  The chosen words (<= 15 matter) live in
// lanes; a candidate's c is a handful of readlane compares.  Heaps, sifts and the argument block are beam_heap.h's.
//
// The bank's bookkeeping (pool slot, stores, copies) and the candidate's arithmetic are written out here and are NOT beam_heap.h's
// BeamBank / beam_candidate: through them this kernel ran 1-2 % slower alone (19.76 against 19.61 us per round at 5x2, 38.09 against
// 37.28 at 4x4, profiles/beam_bank_time.md), and so did this body with only the helper and the Lmax clamp of the copy loops added (19.86,
// 38.07).  Keep the steps in step with BeamBank's; the copy loops rely on the host's Lmax (captions end below it), as they always have.
#include "beam_heap.h"

#include <cmath>

namespace vc {

__global__ __launch_bounds__(64) void beam_update_groups_kernel(BeamArgs a, int G, double lambda) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int w = a.n, kc = a.k, L = a.Lmax;
    const int rpb = 64 / kc;                       // whole rows per block of candidates (kc <= 16: at least 4)
    const int rl = lane / kc, r = lane - rl * kc;  // this lane's row within a block and raw rank within the row
    int chosen = -1, nch = 0;                      // lane j < nch: the j-th word taken by the round's earlier groups
    // the groups' counters in one round trip (lane g: group g) instead of one per group in front of its dependent loads
    const int pc_all = lane < G ? a.pcount[(long)b * G + lane] : 0;
    const int cc_all = lane < G ? a.ccount[(long)b * G + lane] : 0;
    const int fr_all = lane < G ? a.c_free[(long)b * G + lane] : 0;
    for (int g = 0; g < G; ++g) {
        const long v = (long)b * G + g;
        const int np = lane_get(pc_all, g);
        if (lane < w) {   // defaults for slots that stay empty: continue row v*w with token 0 (ignored)
            a.parent[v * w + lane] = (int)(v * w);
            a.tok[v * w + lane] = 0;
        }
        if (np == 0) continue;   // every beam of this group has ended: nothing chosen
        WaveHeap part{0.0, 0.0, 0, 0, 0, -1}, comp{0.0, 0.0, 0, 0, 0, -1};
        int hn = 0, cn = lane_get(cc_all, g);
        if (lane < cn) {
            comp.sc = a.c_score[v * w + lane];
            comp.lp = a.c_logprob[v * w + lane];
            comp.len = a.c_len[v * w + lane];
            comp.slot = a.c_slot[v * w + lane];
        }
        int freemask = lane_get(fr_all, g);
        int rec_src = 0, rec_len0 = -1, rec_tok = 0;   // lane s: the caption recorded for pool slot s this round (len0 < 0: none)
        for (int r0 = 0; r0 < np; r0 += rpb) {
            // ---- 1. candidate (row r0 + rl, raw rank r)
            const bool have = rl < rpb && r0 + rl < np;
            const long row = v * w + (have ? r0 + rl : 0);
            const float pw = have ? a.tv[row * kc + r] : 0.f;
            const int tok_q = have ? a.ti[row * kc + r] : 0;
            const int len0_q = a.p_len[row];
            const double lp_q = a.p_logprob[row] + (double)logf(pw);   // decoder.py:282: np.log of a float32 is a float32; the SUM is a float64
            int c_q = 0;
            for (int j = 0; j < nch; ++j) c_q += tok_q == lane_get(chosen, j) ? 1 : 0;
            // (a rounded product, then a rounded difference: never an fma, and c == 0 keeps lp itself)
            const double key_q = c_q == 0 ? lp_q : __dsub_rn(lp_q, __dmul_rn(lambda, (double)c_q));
            double sc_q = key_q;
            if (tok_q == a.eos) sc_q = a.len_norm_f > 0 ? lp_q / pow((double)(len0_q + 1), a.len_norm_f) : lp_q;
            const int skip_q = (!have || (double)pw < 1e-12) ? 1 : 0;   // decoder.py:279: float32 p against the Python float 1e-12
            // position within the row under (key descending, raw rank ascending)
            const int rs = have ? rl * kc : 0;
            int pos_q = 0;
            for (int j = 0; j < kc; ++j) {
                const double ko = __shfl(key_q, rs + j, 64);
                pos_q += (ko > key_q || (ko == key_q && j < r)) ? 1 : 0;
            }
            const bool sel_q = have && pos_q < w;
            // ---- 2. the walk: rows in heap-array order, each row's first w candidates in key order
            const int nrows = np - r0 < rpb ? np - r0 : rpb;
            for (int rr = 0; rr < nrows; ++rr) {
                for (int p = 0; p < w; ++p) {
                    const unsigned long long m = __ballot(sel_q && rl == rr && pos_q == p);
                    if (m == 0) continue;   // (keys that do not order, NaN: no candidate claims the position)
                    const int c = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
                    if (lane_get(skip_q, c)) continue;
                    BeamItem it;
                    it.tok = lane_get(tok_q, c);
                    it.parent = r0 + rr;
                    const int len0 = lane_get(len0_q, c);
                    it.len = len0 + 1;
                    it.logprob = lane_get(lp_q, c);
                    it.score = lane_get(sc_q, c);
                    it.slot = -1;
                    if (it.tok == a.eos) {
                        // take a free pool slot, record the caption for it, give the slot back if the heap does not keep it
                        const int s = __builtin_ctz(freemask);
                        freemask &= ~(1 << s);
                        it.slot = s;
                        rec_src = lane_set(rec_src, s, it.parent); rec_len0 = lane_set(rec_len0, s, len0); rec_tok = lane_set(rec_tok, s, it.tok);
                        const int freed = topn_push(comp, cn, w, it);
                        if (freed >= 0) freemask |= 1 << freed;
                    } else {
                        topn_push(part, hn, w, it);
                    }
                }
            }
        }
        if (lane < hn) {
            const long o = v * w + lane;
            a.p_score[o] = part.sc;
            a.p_logprob[o] = part.lp;
            a.p_len[o] = part.len;
            a.parent[o] = (int)(v * w) + part.par;
            a.tok[o] = part.tok;
        }
        if (lane < cn) {
            const long o = v * w + lane;
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
        // ---- 3. the copies
        const int32_t* cur = a.sent_cur + v * w * L;
        for (int s = 0; s <= w; ++s) {   // finished captions, per pool slot
            const int len0 = lane_get(rec_len0, s);
            if (len0 < 0) continue;
            const int i = lane_get(rec_src, s), tk = lane_get(rec_tok, s);
            int32_t* dst = a.c_sent + (v * (w + 1) + s) * L;
            for (int t = lane; t <= len0; t += 64) dst[t] = t < len0 ? cur[i * L + t] : tk;
        }
        int32_t* nxt = a.sent_next + v * w * L;
        for (int j = 0; j < hn; ++j) {
            const int len = lane_get(part.len, j), src = lane_get(part.par, j), tk = lane_get(part.tok, j);
            for (int t = lane; t < len; t += 64) nxt[j * L + t] = t < len - 1 ? cur[src * L + t] : tk;
        }
        // ---- the words this group's new live beams end in, for the groups after it (nch + hn <= G*w <= 16 lanes)
        const int tk = __shfl(part.tok, (lane - nch) & 63, 64);
        if (lane >= nch && lane < nch + hn) chosen = tk;
        nch += hn;
    }
}

}  // namespace vc

extern "C" int vc_beam_update_groups(void* stream, int B, int groups, int w, int kc, int Lmax, int eos, double len_norm_f, double diversity,
                                     const float* top_p, const int32_t* top_i, int32_t* pcount, int32_t* ccount, double* p_score,
                                     double* p_logprob, int32_t* p_len, const int32_t* sent_cur, int32_t* sent_next, double* c_score,
                                     double* c_logprob, int32_t* c_len, int32_t* c_slot, int32_t* c_free, int32_t* c_sent, int32_t* parent,
                                     int32_t* tok) {
    using namespace vc;
    VC_CHECK_ARG(B > 0 && groups > 0 && w > 0 && Lmax > 1, "bad argument");
    VC_CHECK_ARG(groups <= BEAM_MAX && w <= BEAM_MAX && groups * w <= BEAM_MAX, "groups * group size must be 1..16");
    VC_CHECK_ARG(kc >= w && kc <= groups * w, "candidates per row must be min(groups * group size, vocabulary) and at least the group size");
    VC_CHECK_ARG(std::isfinite(diversity) && diversity >= 0, "diversity must be finite and >= 0");
    VC_CHECK_ARG((long)B * groups * w <= 0x7fffffffL, "too many rows");
    const BeamArgs a = beam_args(B, w, kc, Lmax, eos, len_norm_f, top_p, top_i, pcount, ccount, p_score, p_logprob, p_len, sent_cur, sent_next,
                                 c_score, c_logprob, c_len, c_slot, c_free, c_sent, parent, tok);
    VC_CHECK_ARG(top_p && top_i && beam_state_given(a), "null pointer");
    hipLaunchKernelGGL(beam_update_groups_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a, groups, diversity);
    VC_LAUNCH_CHECK();
    return 0;
}
