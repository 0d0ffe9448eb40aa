// Constrained beam search bookkeeping on device (Anderson et al., EMNLP 2017: "Guided open vocabulary image captioning with
// constrained beam search"), on the TopN semantics of beam.hip.
//
// An image has C <= 3 constraints; constraint j is a set of <= Wc words and is satisfied once ANY of them has been emitted.  A state is
// the bit mask s of satisfied constraints; every state has a beam search of width w of its own (a "bank": a pair of TopN heaps), laid
// out as "virtual image" v = b*S + s, S = 2^C, of vc_beam_update's state.  A round of one image:
//
//   old = [partial[s].extract() for s in 0..S-1]                (heap ARRAY order); every partial[s] reset
//   for t in 0..S-1:                                            target bank
//       for s in [t] + [t without bit j, j ascending over the bits of t]:
//           for i, beam in enumerate(old[s]):
//               s == t: cand = the first w of the row's kc listed words (descending, stable) that belong to no set j with bit j NOT in s
//               else  : cand = the words of set j (the bit t has and s lacks), in table order, all of them
//               for v in cand: p = probs[row][v] (s == t: the list's value, the same number); skip if p < 1e-12
//                   lp = beam.logprob + float64(float32 log p)  (vc_beam_update's expression)
//                   v == <EOS>: complete[t].push(score = lp / len**len_norm_f)      else: partial[t].push(logprob = lp, score = lp)
//
// kc = min(V, w + the call's largest number of constraint words per image): at most that many listed words are barred, so the first w
// admissible words of the whole vocabulary are in the list.
//
// One wave per IMAGE.  The <= 16 old beams of the image (log-probability, length) are loaded into lanes first (lane s*w + i), with the
// S banks' counters, so the banks are rewritten in place one target at a time.  A target's candidates are prepared a lane each: the
// same-state rows in blocks of floor(64 / kc) whole rows (a word's place among its row's admissible words is a population count over a
// ballot), a forced source's w * Wc <= 32 words in one block.  The lanes of a block are in the reference's walk order, so the sequential
// walk is over the set bits of one ballot.  Heaps, sifts, the candidate's arithmetic and the argument block are beam_heap.h's; a new beam's
// parent is its source row s*w + i of the image, which may lie in another bank.
//
// The bank's bookkeeping (pool slot, stores, copies) is written out here, as in beam_groups.hip, and is NOT beam_heap.h's BeamBank:
// through BeamBank this kernel ran 3 % slower alone (41.2 against 40.0 us per round at C2 w4, profiles/beam_bank_time.md), the wait
// for a bank's loads landing at the head of the bank loop.  Keep the three steps in step with BeamBank's.
#include "beam_heap.h"

namespace vc {

struct ConsArgs {
    int C, Wc, V;
    long ld;
    const int32_t* cons;
    const float* probs;
};

__global__ __launch_bounds__(64) void beam_update_constrained_kernel(BeamArgs a, ConsArgs ca) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int w = a.n, kc = a.k, L = a.Lmax, C = ca.C, Wc = ca.Wc, V = ca.V;
    const int S = 1 << C, NW = C * Wc;
    const long v0 = (long)b * S, row0 = v0 * w;   // the image's first virtual image and first row
    // ---- the image's constraint words (lane j*Wc + k; -1: absent) and its banks' counters (lane s)
    int cw = -1;
    if (lane < NW) {
        cw = ca.cons[(long)b * NW + lane];
        if (cw < 0 || cw >= V) cw = -1;
    }
    int pc_all = 0, cc_all = 0, fr_all = 0;
    if (lane < S) {
        pc_all = a.pcount[v0 + lane]; cc_all = a.ccount[v0 + lane]; fr_all = a.c_free[v0 + lane];
        pc_all = pc_all < 0 ? 0 : (pc_all > w ? w : pc_all);
        cc_all = cc_all < 0 ? 0 : (cc_all > w ? w : cc_all);
    }
    // ---- the old beams (lane s*w + i): what the round reads of the state it rewrites
    double old_lp = 0.0;
    int old_len = 0;
    {
        const int s = lane / w, i = lane - s * w;
        const int np_s = __shfl(pc_all, s < S ? s : 0, 64);
        if (s < S && i < np_s) {
            old_lp = a.p_logprob[row0 + lane];
            old_len = a.p_len[row0 + lane];
        }
    }
    const int32_t* cur = a.sent_cur + row0 * L;
    const int rpb = 64 / kc;                       // whole same-state rows per block of candidates (kc <= 14: at least 4)
    const int rl = lane / kc, r = lane - rl * kc;  // this lane's row within such a block and raw rank within the row
    const int fi = lane / Wc, fk = lane - fi * Wc; // this lane's beam and word within a forced block
    for (int t = 0; t < S; ++t) {
        const long v = v0 + t;
        beam_next_defaults(a, v);
        const int np_t = lane_get(pc_all, t);
        int feeders = np_t;
        for (int j = 0; j < C; ++j) feeders += ((t >> j) & 1) ? lane_get(pc_all, t ^ (1 << j)) : 0;
        if (feeders == 0) continue;   // no live beam can reach this bank this round: its heaps stay as they are (partial empty)
        WaveHeap part{0.0, 0.0, 0, 0, 0, -1}, comp{0.0, 0.0, 0, 0, 0, -1};
        int hn = 0, cn = lane_get(cc_all, t);
        if (lane < cn) {
            comp.sc = a.c_score[v * w + lane];
            comp.lp = a.c_logprob[v * w + lane];
            comp.len = a.c_len[v * w + lane];
            comp.slot = a.c_slot[v * w + lane];
        }
        int freemask = lane_get(fr_all, t);
        int rec_src = 0, rec_len0 = -1, rec_tok = 0;   // lane s: the caption recorded for pool slot s this round (len0 < 0: none)
        // one block of candidates: lane q holds (ok_q, source row src_q of the image, word tok_q, probability pw); lanes in walk order
        auto walk = [&](bool ok_q, int src_q, int tok_q, float pw) {
            const int len0_q = __shfl(old_len, ok_q ? src_q : 0, 64);
            const BeamCand cd = beam_candidate(a, __shfl(old_lp, ok_q ? src_q : 0, 64), len0_q, pw, tok_q);
            const double lp_q = cd.lp, sc_q = cd.score;
            unsigned long long m = __ballot(ok_q && !cd.skip);
            while (m) {
                const int c = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
                m &= m - 1;
                BeamItem it;
                it.tok = lane_get(tok_q, c);
                it.parent = lane_get(src_q, c);
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
        };
        // ---- 1. the same state: each live row's first w listed words that no unsatisfied set holds
        for (int r0 = 0; r0 < np_t; r0 += rpb) {
            const bool have = rl < rpb && r0 + rl < np_t;
            const int src_q = have ? t * w + r0 + rl : 0;
            const long row = row0 + src_q;
            const float pw = have ? a.tv[row * kc + r] : 0.f;
            const int tok_q = have ? a.ti[row * kc + r] : -1;
            bool adm = have && tok_q >= 0 && tok_q < V;
            for (int q = 0; q < NW; ++q) {
                const int word = lane_get(cw, q);
                if (!((t >> (q / Wc)) & 1) && word >= 0 && word == tok_q) adm = false;
            }
            const unsigned long long bal = __ballot(adm);
            const int before = have ? __builtin_popcountll((bal >> (rl * kc)) & ((1ull << r) - 1ull)) : 0;
            walk(adm && before < w, src_q, tok_q, pw);
        }
        // ---- 2. the banks one constraint short of t: every word of the missing set, forced
        for (int j = 0; j < C; ++j) {
            if (!((t >> j) & 1)) continue;
            const int s = t ^ (1 << j), np_s = lane_get(pc_all, s);
            if (np_s == 0) continue;
            const int word = __shfl(cw, fi < w ? j * Wc + fk : 0, 64);
            const bool ok = fi < np_s && word >= 0;
            const int src_q = ok ? s * w + fi : 0;
            const float pw = ok ? ca.probs[(row0 + src_q) * ca.ld + word] : 0.f;
            walk(ok, src_q, ok ? word : -1, pw);
        }
        if (lane < hn) {
            const long o = v * w + lane;
            a.p_score[o] = part.sc;
            a.p_logprob[o] = part.lp;
            a.p_len[o] = part.len;
            a.parent[o] = (int)row0 + part.par;
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
        // ---- 3. the copies (sources: any row of the image)
        for (int s = 0; s <= w; ++s) {   // finished captions, per pool slot
            const int len0 = lane_get(rec_len0, s);
            if (len0 < 0) continue;
            const int i = lane_get(rec_src, s), tk = lane_get(rec_tok, s);
            int32_t* dst = a.c_sent + (v * (w + 1) + s) * L;
            for (int p = lane; p <= len0 && p < L; p += 64) dst[p] = p < len0 ? cur[i * L + p] : tk;
        }
        int32_t* nxt = a.sent_next + v * w * L;
        for (int j = 0; j < hn; ++j) {
            const int len = lane_get(part.len, j), src = lane_get(part.par, j), tk = lane_get(part.tok, j);
            for (int p = lane; p < len && p < L; p += 64) nxt[j * L + p] = p < len - 1 ? cur[src * L + p] : tk;
        }
    }
}

}  // namespace vc

extern "C" int vc_beam_update_constrained(void* stream, int B, int C, int Wc, int w, int kc, int Lmax, int eos, double len_norm_f,
                                          const int32_t* cons, const float* top_p, const int32_t* top_i, const float* probs, long ld, int V,
                                          int32_t* pcount, int32_t* ccount, double* p_score, double* p_logprob, int32_t* p_len,
                                          const int32_t* sent_cur, int32_t* sent_next, double* c_score, double* c_logprob, int32_t* c_len,
                                          int32_t* c_slot, int32_t* c_free, int32_t* c_sent, int32_t* parent, int32_t* tok) {
    using namespace vc;
    VC_CHECK_ARG(B > 0 && Lmax > 1 && V > 0, "bad argument");
    VC_CHECK_ARG(C >= 0 && C <= 3, "constraints per image must be 0..3");
    VC_CHECK_ARG(C == 0 || (Wc >= 1 && Wc <= 4), "words per constraint must be 1..4");
    VC_CHECK_ARG(w >= 1 && w <= BEAM_MAX && (w << C) <= BEAM_MAX, "beams per state x states must be 1..16");
    const int nw = C == 0 ? 0 : C * Wc;
    VC_CHECK_ARG(kc >= w && kc <= w + nw && kc <= V, "candidates per row must be min(beams per state + constraint words, vocabulary) and at least the beams per state");
    VC_CHECK_ARG(ld >= V, "row stride of the probabilities below the vocabulary");
    VC_CHECK_ARG(((long)B << C) * w <= 0x7fffffffL / Lmax, "too many rows");
    const BeamArgs a = beam_args(B, w, kc, Lmax, eos, len_norm_f, top_p, top_i, pcount, ccount, p_score, p_logprob, p_len, sent_cur, sent_next,
                                 c_score, c_logprob, c_len, c_slot, c_free, c_sent, parent, tok);
    VC_CHECK_ARG((C == 0 || (cons && probs)) && top_p && top_i && beam_state_given(a), "null pointer");
    ConsArgs ca;
    ca.C = C; ca.Wc = C == 0 ? 1 : Wc; ca.V = V; ca.ld = ld; ca.cons = cons; ca.probs = probs;
    hipLaunchKernelGGL(beam_update_constrained_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a, ca);
    VC_LAUNCH_CHECK();
    return 0;
}
