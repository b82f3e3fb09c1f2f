// Retrieval sweep kernels (replicated exemplar DB resident in HBM).
//
//  rg_discourse_scores_batched / rg_discourse_select_fused : the per-DB-entry categorical + prominence score of
//      rag/discourse_retrieval.py:86-222 for every query relation of a batch, in float64 with the reference's
//      operation order (sense +2, connective +4, speaker +3, mean of 4/(1+2|dp|) over the entry's
//      relations of that sense), plus the index of the relation whose bounds are returned
//      (`top_rel_idx`).  One thread per DB entry over integer-coded CSR metadata: pure HBM
//      streaming (<= ~40 B per entry).
//  rg_text_diag_sim_many : the tie-break similarity of rag/utils.py:86-132,
//      mean(diag(q[Lq,768] . db[Ld,768]^T)) = mean over i < min(Lq,Ld) of q[i].db[i], for a list
//      of (DB entry, query) pairs; fp32 products accumulated in fp64, one workgroup per pair, 16 B
//      per lane coalesced reads of the entry's token features (the reference computes the full
//      Lq x Ld matrix and takes its diagonal).
//  rg_rank_survivors_batch / rg_discourse_search_batch : a batch's whole search in one call -- (sweep,) survivor pack and ONE
//      read-back, the ranking on the host (rg_retrieval_host.h), ONE launch for every tie tier of every clip, ONE read-back.
//  rg_prosody_scores_batched : the prosody method's sweep (this project's own scoring), all queries of a batch in one launch; a
//      workgroup stages a tile of entries' words in LDS once and loops over the queries, an entry's words spread over 16 lanes.
//  rg_motion_scores_batched : the motion method's sweep (this project's own: exemplars by a motion example) -- squared fp32
//      distances between an example's VAE posterior means and every window position of every entry's; a workgroup stages one
//      entry's weighted parts in LDS once and loops over the queries, 16 lanes per query.
#include <climits>

#include "rg_common.h"
#include "rg_reduce.h"
#include "rg_retrieval_host.h"

namespace {

__device__ __forceinline__ void discourse_score_value(
    const int e, const int* __restrict__ spk, const int* __restrict__ rel_off, const int* __restrict__ rel_sense,
    const int* __restrict__ rel_conn, const double* __restrict__ rel_prom, int q_sense, int q_conn,
    int q_spk, double q_prom, double& score_ret, int& top_ret) {
  const int r0 = rel_off[e], r1 = rel_off[e + 1];
  double score = 0.0;
  int top = -1;
  int first = -1, conn_hit = -1;
  for (int r = r0; r < r1; ++r) {
    if (rel_sense[r] == q_sense) {
      if (first < 0) first = r;
      if (conn_hit < 0 && q_conn >= 0 && rel_conn[r] == q_conn) conn_hit = r;
    }
  }
  if (first >= 0) {
    score += 2.0;
    top = first;
    bool chosen = false;
    if (conn_hit >= 0) {
      score += 4.0;
      top = conn_hit;
      chosen = true;
    }
    if (spk[e] == q_spk) score += 3.0;
    double sum = 0.0, best = 0.0;
    int cnt = 0, best_r = -1;
    if (q_prom == q_prom) {  // query prominence known (not NaN)
      for (int r = first; r < r1; ++r) {
        if (rel_sense[r] != q_sense) continue;
        const double p = rel_prom[r];
        if (p != p) continue;
        const double diff = fabs(p - q_prom);
        sum += 4.0 / (1.0 + 2.0 * diff);
        if (best_r < 0 || diff < best) {  // first minimum = stable sort of the reference
          best = diff;
          best_r = r;
        }
        ++cnt;
      }
    }
    if (cnt > 0) {
      score += sum / (double)cnt;
      if (top != best_r && !chosen) top = best_r;
    }
    top -= r0;
  }
  score_ret = score;
  top_ret = top;
}

__device__ __forceinline__ void discourse_score_entry(
    const int e, const int* __restrict__ spk, const int* __restrict__ rel_off, const int* __restrict__ rel_sense,
    const int* __restrict__ rel_conn, const double* __restrict__ rel_prom, int q_sense, int q_conn,
    int q_spk, double q_prom, double* __restrict__ score_out, int* __restrict__ top_out) {
  double sc;
  int tp;
  discourse_score_value(e, spk, rel_off, rel_sense, rel_conn, rel_prom, q_sense, q_conn, q_spk, q_prom, sc, tp);
  score_out[e] = sc;
  top_out[e] = tp;
}

// all queries of a batch in one launch: blockIdx.y = query; params[q] = (sense, connective, speaker, prominence) as
// doubles (the integer codes are exact), outputs [n_queries][n_entries]
__global__ void __launch_bounds__(256) discourse_scores_batched_kernel(
    const int* __restrict__ spk, const int* __restrict__ rel_off, const int* __restrict__ rel_sense,
    const int* __restrict__ rel_conn, const double* __restrict__ rel_prom, int n_entries,
    const double* __restrict__ params, double* __restrict__ score_out, int* __restrict__ top_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  const double* qp = params + 4 * blockIdx.y;
  const size_t o = (size_t)blockIdx.y * n_entries;
  discourse_score_entry(e, spk, rel_off, rel_sense, rel_conn, rel_prom, (int)qp[0], (int)qp[1], (int)qp[2], qp[3],
                        score_out + o, top_out + o);
}

// rag/gesture_type_retrieval.py:41-117 for one query label (type, word): per DB entry, over its non-beat labels of
// the query type: +2 type present, +2 same speaker, +5 exact word (top = first label with that word) or
// +3/(1+2*max similarity) (top = first label of maximal similarity); word codes index the similarity vector the
// host computed for this query word (get_word_similarity_score against every DB word), float64 like the
// reference's Python floats.  top_out = index within the entry's non-beat labels, -1 if the type is absent.
__global__ void __launch_bounds__(256) gesture_scores_kernel(const int* __restrict__ spk, const int* __restrict__ lab_off,
                                                            const int* __restrict__ lab_type, const int* __restrict__ lab_word,
                                                            const double* __restrict__ lab_prom,
                                                            const double* __restrict__ word_sim, int n_entries, int q_type,
                                                            int q_word, int q_spk, double spk_bonus, double q_prom,
                                                            int sim_f32, double* __restrict__ score_out,
                                                            int* __restrict__ top_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  const int r0 = lab_off[e], r1 = lab_off[e + 1];
  int exact = -1, best = -1;
  double best_sim = 0.0;
  bool any = false;
  for (int r = r0; r < r1; ++r) {
    if (lab_type[r] != q_type) continue;
    any = true;
    const int w = lab_word[r];
    if (exact < 0 && q_word >= 0 && w == q_word) exact = r;
    const double sv = word_sim[w];
    if (best < 0 || sv > best_sim) {   // np.argmax: first maximum
      best = r;
      best_sim = sv;
    }
  }
  double score = 0.0;
  int top = -1;
  if (any) {
    bool f32 = false;
    score += 2.0;
    if (spk[e] == q_spk) score += spk_bonus;
    if (exact >= 0) {
      score += 5.0;
      top = exact - r0;
    } else {
      // a similarity model that returns numpy float32 (gensim) makes the reference's score float32 from here on
      // under NumPy >= 2 (NEP 50: python scalar (+|*|/) np.float32 -> float32); python floats, and float32 scalars
      // under the reference's pinned NumPy < 1.24 (scalar-scalar promotion), keep it float64
      if (sim_f32) {
        const float s = (float)best_sim;
        score = (double)((float)score + 3.0f / (1.0f + 2.0f * s));
        f32 = true;
      } else {
        score += 3.0 / (1.0 + 2.0 * best_sim);
      }
      top = best - r0;
    }
    // llm method only (rag/llm_retrieval.py:385-417): mean of 4/(1+2|prominence difference|) over the labels of
    // the query type with a known prominence; the label of smallest difference (first minimum) is reported
    if (lab_prom != nullptr && q_prom == q_prom) {
      double sum = 0.0, bestd = 0.0;
      int cnt = 0, best_r = -1;
      for (int r = r0; r < r1; ++r) {
        if (lab_type[r] != q_type) continue;
        const double p = lab_prom[r];
        if (p != p) continue;
        const double diff = fabs(p - q_prom);
        sum += 4.0 / (1.0 + 2.0 * diff);
        if (best_r < 0 || diff < bestd) {
          bestd = diff;
          best_r = r;
        }
        ++cnt;
      }
      if (cnt > 0) {
        const double ps = sum / (double)cnt;
        score = f32 ? (double)((float)score + (float)ps) : score + ps;
        top = best_r - r0;
      }
    }
  }
  score_out[e] = score;
  top_out[e] = top;
}

// The prosody method (this project's own scoring: the reference names the method and raises, raggesture.py:426-431): per
// query word (prominence p_q, duration dur_q, speaker spk_q, similarity row sim_q[V]) and DB entry, over the entry's words j
// with a finite prominence, all in float64 and in this association:
//   s_j   = (4 / (1 + 2 |prom_j - p_q|) + 2 sim_q[code_j]) + 1 / (1 + 4 |dur_j - dur_q|)
//   score = max_j s_j (lowest j among equals) + (spk == spk_q ? 3 : 0),  top = that j;  no such word: score 0, top -1.
// Every product is by a power of two (exact), so contraction into FMA cannot change a bit; the divisions are correctly rounded.
// Layout: a workgroup owns PS_TILE = 16 consecutive entries.  It stages their words (code, prominence, duration: 20 B each)
// in LDS once -- the first PS_CAP words of the tile; a tile with more (16 entries of more than 64 words on average) reads the
// rest from global memory, same values -- and then loops over ALL queries, so the word table leaves HBM once per launch.
// PS_GROUP = 16 adjacent lanes own one entry: lane l takes words l, l + 16, ... and keeps its first maximum, and
// group_argmax_f64 (greater score, then lower word index: a total order) merges the lanes, so the result does not depend on
// how the words were dealt out.  The time goes into the similarity gather (a dependent L2 read per word and query) and two
// float64 divisions per (word, query), not into HBM: a group takes PS_QU = 4 queries per pass over its words, so four
// gathers are in flight per lane and a word is read from LDS once per four queries; 20 KB of LDS leave room for seven
// workgroups per compute unit to hide the rest.
constexpr int PS_TILE = 16, PS_CAP = 1024, PS_GROUP = 16, PS_QU = 4;
static_assert(PS_TILE * PS_GROUP == 256, "one group of lanes per entry of the tile");

__global__ void __launch_bounds__(256) prosody_scores_batched_kernel(
    const int* __restrict__ spk, const int* __restrict__ word_off, const int* __restrict__ word_code,
    const double* __restrict__ word_prom, const double* __restrict__ word_dur, int n_entries, const double* __restrict__ sim,
    int n_vocab, const double* __restrict__ params, int n_queries, double* __restrict__ score_out, int* __restrict__ top_out) {
  __shared__ double s_prom[PS_CAP], s_dur[PS_CAP];
  __shared__ int s_code[PS_CAP], s_off[PS_TILE + 1], s_spk[PS_TILE];
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * PS_TILE;
  const int ne = n_entries - e0 < PS_TILE ? n_entries - e0 : PS_TILE;
  if (tid <= ne) s_off[tid] = word_off[e0 + tid];
  if (tid < ne) s_spk[tid] = spk[e0 + tid];
  __syncthreads();
  const int w0 = s_off[0];
  const int nw = s_off[ne] - w0;
  const int staged = nw < PS_CAP ? nw : PS_CAP;
  for (int i = tid; i < staged; i += 256) {
    s_code[i] = word_code[w0 + i];
    s_prom[i] = word_prom[w0 + i];
    s_dur[i] = word_dur[w0 + i];
  }
  __syncthreads();
  const int g = tid / PS_GROUP, l = tid % PS_GROUP;
  if (g >= ne) return;            // (whole groups leave: the butterfly below stays inside a group's 16 lanes; no barrier follows)
  const double inf = __builtin_huge_val();
  const int a = s_off[g] - w0, b = s_off[g + 1] - w0;
  const int e_spk = s_spk[g];
  for (int q0 = 0; q0 < n_queries; q0 += PS_QU) {
    double p_q[PS_QU], dur_q[PS_QU], best[PS_QU];
    const double* sim_q[PS_QU];
    int top[PS_QU];
#pragma unroll
    for (int u = 0; u < PS_QU; ++u) {
      const int q = q0 + u < n_queries ? q0 + u : n_queries - 1;      // (a short last pass repeats the last query)
      p_q[u] = params[3 * q], dur_q[u] = params[3 * q + 1];
      sim_q[u] = sim + (size_t)q * n_vocab;
      best[u] = -inf, top[u] = INT_MAX;
    }
    for (int j = a + l; j < b; j += PS_GROUP) {
      int c;
      double p, d;
      if (j < PS_CAP) {
        c = s_code[j], p = s_prom[j], d = s_dur[j];
      } else {
        c = word_code[w0 + j], p = word_prom[w0 + j], d = word_dur[w0 + j];
      }
      if (!(fabs(p) < inf)) continue;                                    // unknown prominence
      const bool known = (unsigned)c < (unsigned)n_vocab;                // (a code outside the vocabulary reads nothing)
      double sv[PS_QU];
#pragma unroll
      for (int u = 0; u < PS_QU; ++u) sv[u] = known ? sim_q[u][c] : 0.0;
#pragma unroll
      for (int u = 0; u < PS_QU; ++u) {
        const double s = (4.0 / (1.0 + 2.0 * fabs(p - p_q[u])) + 2.0 * sv[u]) + 1.0 / (1.0 + 4.0 * fabs(d - dur_q[u]));
        if (s > best[u]) {            // j ascends: the lane keeps its first maximum; a NaN never enters
          best[u] = s;
          top[u] = j - a;
        }
      }
    }
    double my_best = -inf;
    int my_top = INT_MAX;
#pragma unroll
    for (int u = 0; u < PS_QU; ++u) {
      group_argmax_f64<PS_GROUP>(best[u], top[u]);
      if (l == u) my_best = best[u], my_top = top[u];
    }
    if (l < PS_QU && q0 + l < n_queries) {       // lane u of the group stores query q0 + u
      const int q = q0 + l;
      const size_t o = (size_t)q * n_entries + e0 + g;
      const bool any = my_top != INT_MAX;
      score_out[o] = any ? my_best + (e_spk == (int)params[3 * q + 2] ? 3.0 : 0.0) : 0.0;
      top_out[o] = any ? my_top : -1;
    }
  }
}

// The motion method (this project's own: the reference has no counterpart): exemplars by a motion example.  Per query q (n_q
// chunks of posterior means qlat[q] [4][n_q][D], part weights w, speaker, bonus) and DB entry e (lat[e] [4][L][D]), over the
// offsets o = 0 .. L - n_q:
//   S_p(o) = sum_{c < n_q} sum_{k < D} (lat[e][p][o + c][k] - qlat[q][p][c][k])^2       fp32: one subtraction, one multiply-add
//   d(o)   = sum_{p, w_p > 0} (double)w_p * (double)S_p(o)                              fp64, parts in order, nothing contracted
//   o*     = the offset of the smallest d (the lowest among equals)
//   score  = 1 / (1 + d(o*) / (n_q D sum_p w_p)) + (spk[e] == speaker ? bonus : 0);  top = o*
// The difference form keeps every term non-negative: the error of S_p is relative and a copied example scores exactly 1.
// Layout: a workgroup owns ONE entry.  It stages the rows of the parts that any query weighs (part_mask, from the host check) in
// LDS once -- 20 KB per part at L = 10, D = 512 -- and then loops over ALL queries, so the table leaves HBM once per launch
// whatever the number of queries.  MS_GROUP = 16 adjacent lanes own one query of a pass of 16: lane l takes the float4 columns
// l, l + 16, ... of every row (a group reads 256 contiguous bytes of LDS per instruction: no bank conflict; the four groups of a
// wave that read the same row share the address).  For each column block the lane holds the query's n_q chunk values in
// registers, reads each table row ONCE and adds it into the accumulators of every offset it belongs to (row j pairs with chunk c
// at offset j - c), so a row is read L times per part and query, not n_q (L - n_q + 1) times.  The order of the additions into
// S_p(o) is: column blocks ascending, rows ascending, the four values of a float4 in order, then a xor butterfly over the 16
// lanes -- a function of the query and the entry alone, so a query's row does not depend on what else is in the launch.
constexpr int MS_GROUP = 16, MS_QPASS = 256 / MS_GROUP, MS_L = RG_MOTION_MAX_L, MS_P = RG_MOTION_PARTS;

template <int WIDTH>
__device__ __forceinline__ float group_sum_f32(float v) {
#pragma unroll
  for (int m = WIDTH >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ float sq_acc4(float acc, const float4 a, const float4 b) {
  const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z, w = a.w - b.w;
  acc = fmaf(x, x, acc);
  acc = fmaf(y, y, acc);
  acc = fmaf(z, z, acc);
  return fmaf(w, w, acc);
}

// A lane's share of S_p(o) for all offsets of one part: column blocks l, l + 16, ... ascending, rows ascending; row j is chunk c
// of the span at offset j - c.  NQ chunks against a window of MS_L rows, everything unrolled; motion_part_sums_any is the same
// order of additions for a shorter window (L < MS_L), with the bounds as predicates.
template <int NQ>
__device__ __forceinline__ void motion_part_sums(const float4* __restrict__ qp, const float4* lp, int D4, int l, float (&S)[MS_L]) {
  constexpr int NO = MS_L - NQ + 1;
  for (int i = l; i < D4; i += MS_GROUP) {
    float4 qv[NQ];
#pragma unroll
    for (int c = 0; c < NQ; ++c) qv[c] = qp[c * D4 + i];
#pragma unroll
    for (int j = 0; j < MS_L; ++j) {
      const float4 x = lp[j * D4 + i];
#pragma unroll
      for (int c = 0; c < NQ; ++c)
        if (j - c >= 0 && j - c < NO) S[j - c] = sq_acc4(S[j - c], x, qv[c]);
    }
  }
}

__device__ __forceinline__ void motion_part_sums_any(const float4* __restrict__ qp, const float4* lp, int D4, int l, int L, int nq,
                                                     float (&S)[MS_L]) {
  const int no = L - nq + 1;
  for (int i = l; i < D4; i += MS_GROUP) {
    float4 qv[MS_L];
#pragma unroll
    for (int c = 0; c < MS_L; ++c)
      if (c < nq) qv[c] = qp[c * D4 + i];
#pragma unroll
    for (int j = 0; j < MS_L; ++j) {
      if (j < L) {
        const float4 x = lp[j * D4 + i];
#pragma unroll
        for (int c = 0; c <= j; ++c)
          if (c < nq && j - c < no) S[j - c] = sq_acc4(S[j - c], x, qv[c]);
      }
    }
  }
}

// S_p(o) of one part for all offsets, every lane of the group holding the sums; zeros for a part without weight (not read)
__device__ __forceinline__ void motion_part(bool weighted, const float4* __restrict__ qp, const float4* lp, int D4, int l, int L, int nq,
                                            float (&S)[MS_L]) {
#pragma unroll
  for (int o = 0; o < MS_L; ++o) S[o] = 0.0f;
  if (!weighted) return;
  if (L == MS_L) {                   // the model's window: offsets and chunk pairs are compile-time per n_q (no predicates)
    switch (nq) {
      case 1: motion_part_sums<1>(qp, lp, D4, l, S); break;
      case 2: motion_part_sums<2>(qp, lp, D4, l, S); break;
      case 3: motion_part_sums<3>(qp, lp, D4, l, S); break;
      case 4: motion_part_sums<4>(qp, lp, D4, l, S); break;
      case 5: motion_part_sums<5>(qp, lp, D4, l, S); break;
      case 6: motion_part_sums<6>(qp, lp, D4, l, S); break;
      case 7: motion_part_sums<7>(qp, lp, D4, l, S); break;
      case 8: motion_part_sums<8>(qp, lp, D4, l, S); break;
      case 9: motion_part_sums<9>(qp, lp, D4, l, S); break;
      default: motion_part_sums<10>(qp, lp, D4, l, S); break;
    }
  } else {
    motion_part_sums_any(qp, lp, D4, l, L, nq, S);
  }
#pragma unroll
  for (int o = 0; o < MS_L; ++o) S[o] = group_sum_f32<MS_GROUP>(S[o]);
}

__global__ void __launch_bounds__(256) motion_scores_batched_kernel(
    const float* __restrict__ lat, int n_entries, int L, int D, const int* __restrict__ spk, const float* __restrict__ qlat,
    const int* __restrict__ q_off, int n_chunks, const double* __restrict__ params, int n_queries, unsigned part_mask,
    double* __restrict__ score_out, int* __restrict__ top_out, float* __restrict__ sp_out) {
  extern __shared__ __attribute__((aligned(16))) float s_lat[];      // [parts staged][L][D]
  const int tid = threadIdx.x;
  const int e = blockIdx.x;                                          // (the grid is n_entries workgroups)
  const int D4 = D >> 2, row4 = L * D4;                              // float4 per chunk row, per part
  int slot_of[MS_P];
  {
    int slot = 0;
#pragma unroll
    for (int p = 0; p < MS_P; ++p) {
      slot_of[p] = slot;
      if (!((part_mask >> p) & 1u)) continue;
      const float4* src = reinterpret_cast<const float4*>(lat + ((size_t)e * MS_P + p) * (size_t)L * D);
      float4* dst = reinterpret_cast<float4*>(s_lat) + (size_t)slot * row4;
      for (int i = tid; i < row4; i += 256) dst[i] = src[i];
      ++slot;
    }
  }
  __syncthreads();
  const int g = tid / MS_GROUP, l = tid % MS_GROUP;
  const int e_spk = spk[e];
  for (int q = g; q < n_queries; q += MS_QPASS) {          // (whole groups leave: the butterflies stay inside a group; no barrier follows)
    const int c0 = q_off[q];
    const int nq = q_off[q + 1] - c0;
    const double* par = params + (size_t)q * RG_MOTION_PARAMS;
    const size_t o_out = (size_t)q * n_entries + e;
    if (nq < 1 || nq > L || c0 < 0 || c0 + nq > n_chunks) {          // device offsets that are not the checked host copy: nothing is read
      if (l == 0) {
        score_out[o_out] = __builtin_nan("");
        top_out[o_out] = -1;
      }
      continue;
    }
    const int no = L - nq + 1;
    const double w0 = par[0], w1 = par[1], w2 = par[2], w3 = par[3];
    const float4* qb = reinterpret_cast<const float4*>(qlat + (size_t)c0 * MS_P * D);
    const float4* lb = reinterpret_cast<const float4*>(s_lat);
    float S0[MS_L], S1[MS_L], S2[MS_L], S3[MS_L];      // (four arrays, four calls: every index a constant, all in registers)
    motion_part(w0 > 0.0 && (part_mask & 1u), qb, lb + (size_t)slot_of[0] * row4, D4, l, L, nq, S0);
    motion_part(w1 > 0.0 && (part_mask & 2u), qb + (size_t)nq * D4, lb + (size_t)slot_of[1] * row4, D4, l, L, nq, S1);
    motion_part(w2 > 0.0 && (part_mask & 4u), qb + (size_t)2 * nq * D4, lb + (size_t)slot_of[2] * row4, D4, l, L, nq, S2);
    motion_part(w3 > 0.0 && (part_mask & 8u), qb + (size_t)3 * nq * D4, lb + (size_t)slot_of[3] * row4, D4, l, L, nq, S3);
    {
#pragma clang fp contract(off)
      const double wsum = (((0.0 + w0) + w1) + w2) + w3;
      double best = 0.0;
      int top = 0;
      float sp0 = 0.0f, sp1 = 0.0f, sp2 = 0.0f, sp3 = 0.0f;
#pragma unroll
      for (int o = 0; o < MS_L; ++o) {
        double d = 0.0;
        if (w0 > 0.0) d += w0 * (double)S0[o];
        if (w1 > 0.0) d += w1 * (double)S1[o];
        if (w2 > 0.0) d += w2 * (double)S2[o];
        if (w3 > 0.0) d += w3 * (double)S3[o];
        if (o == 0 || (o < no && d < best)) {                        // ascending o, strictly smaller: the lowest offset among equals
          best = d;
          top = o;
          sp0 = S0[o], sp1 = S1[o], sp2 = S2[o], sp3 = S3[o];
        }
      }
      if (l == 0) {
        const double dn = best / ((double)(nq * D) * wsum);
        double sc = 1.0 / (1.0 + dn);
        if (e_spk == (int)par[4]) sc += par[5];
        score_out[o_out] = sc;
        top_out[o_out] = top;
        if (sp_out != nullptr) *reinterpret_cast<float4*>(sp_out + o_out * MS_P) = make_float4(sp0, sp1, sp2, sp3);
      }
    }
  }
}

// One workgroup's tie-break similarity of query q [Lq, dim] to DB entry c -> *out (a fixed loop and reduction tree: a pair's
// bits do not depend on where in a launch, or in which launch, it is computed)
__device__ __forceinline__ void text_diag_sim_one(const float* __restrict__ q, int Lq, const float* __restrict__ feats,
                                                  const int64_t* __restrict__ feat_off, const int c, int dim,
                                                  double* __restrict__ out, double* red) {
  const int64_t o0 = feat_off[c];
  const int Ld = (int)(feat_off[c + 1] - o0);
  const int n = Lq < Ld ? Lq : Ld;
  const int d4 = dim >> 2;
  const float4* qa = reinterpret_cast<const float4*>(q);
  const float4* fa = reinterpret_cast<const float4*>(feats + o0 * dim);
  double acc = 0.0;
  for (int i = threadIdx.x; i < n * d4; i += 256) {
    const float4 a = qa[i], b = fa[i];
    acc += (double)(a.x * b.x) + (double)(a.y * b.y) + (double)(a.z * b.z) + (double)(a.w * b.w);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *out = n > 0 ? ((red[0] + red[1]) + (red[2] + red[3])) / (double)n : 0.0;
}

// Every tie tier of every clip of a batch in one launch: blockIdx.x = pair (DB entry, query index); the query table holds
// each query's feature pointer and length.  Table and pairs are one uploaded block (the host checks every index).
struct SimQuery {
  const float* q;
  int Lq, pad;
};
struct SimPair {
  int entry, query;
};
__global__ void __launch_bounds__(256) text_diag_sim_many_kernel(const SimQuery* __restrict__ queries,
                                                                const SimPair* __restrict__ pairs,
                                                                const float* __restrict__ feats,
                                                                const int64_t* __restrict__ feat_off, int dim,
                                                                double* __restrict__ out) {
  __shared__ double red[4];
  const SimPair p = pairs[blockIdx.x];
  const SimQuery sq = queries[p.query];
  text_diag_sim_one(sq.q, sq.Lq, feats, feat_off, p.entry, dim, out + blockIdx.x, red);
}

// ---- survivor pack: the sweep's [Q][cap] lists -> one contiguous block -------------------------------------------------------
// counts[q] = min(cursor[q], cap) for every query, then the queries' survivors back to back as 16-byte rows (query q's rows
// start at the sum of the counts before it): what the host reads back in ONE copy instead of a cursor read and three strided
// slices.  If the rows do not fit rows_cap the kernel writes the counts alone; the host then grows the block and packs again.
struct alignas(16) PackRow {
  double score;
  int idx, top;
};
constexpr int PACK_BX = 4;   // workgroups per query

__global__ void __launch_bounds__(256) survivor_pack_kernel(const int* __restrict__ cursor, const int* __restrict__ idx,
                                                           const int* __restrict__ top, const double* __restrict__ score,
                                                           int n_queries, int cap, long long rows_cap,
                                                           int* __restrict__ counts_out, PackRow* __restrict__ rows_out) {
  __shared__ long long red[2][4];
  const int q = blockIdx.y;
  long long before = 0, total = 0;
  for (int j = threadIdx.x; j < n_queries; j += 256) {
    int c = cursor[j];
    c = c < cap ? c : cap;
    total += c;
    if (j < q) before += c;
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    before += __shfl_xor(before, off);
    total += __shfl_xor(total, off);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = before;
    red[1][threadIdx.x >> 6] = total;
  }
  __syncthreads();
  before = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  total = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  int cnt = cursor[q];
  cnt = cnt < cap ? cnt : cap;
  if (blockIdx.x == 0 && threadIdx.x == 0) counts_out[q] = cnt;
  if (total > rows_cap) return;                       // (uniform: the whole launch writes counts only)
  const size_t o = (size_t)q * cap;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += PACK_BX * 256) {   // before + i < total <= rows_cap
    PackRow r;
    r.score = score[o + i];
    r.idx = idx[o + i];
    r.top = top[o + i];
    rows_out[before + i] = r;
  }
}

// ---- candidate selection on the device --------------------------------------------------------
// The reference sorts all N scores and walks the ranking until it has 10 entries, so only entries
// whose score reaches the 10th largest one (with multiplicity) can ever be visited -- including
// EVERY entry tied at that score (they are ordered by the text-similarity tie-break).  Instead of
// copying N scores to the host, find that threshold on the device and compact the survivors:
//   topk_local : each workgroup extracts the 10 largest scores of its slice (10 rounds of a
//                block-wide max that consumes one instance per round: multiplicity is preserved);
//   topk_merge : one workgroup repeats that over the per-block lists -> threshold;
//   compact    : entries with score >= threshold and score > 0 are appended (atomic cursor;
//                the host re-sorts the few survivors by index, which restores the stable order).
// Scores are >= 0, comparisons only: the selection is exact.
constexpr int SEL_K = 10;
constexpr int SEL_IPT = 4;   // items per thread held in registers

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}

// The 10 largest values (with multiplicity) of the 256 x SEL_IPT items a workgroup holds in registers; tops[] is uniform
// across the block on return.  Per wave: 10 rounds of "largest remaining value" on wave shuffles alone (the owner of a
// round's maximum -- the lowest lane that holds it -- consumes ONE instance); the four waves' lists meet in LDS and wave 0
// repeats the rounds over those 40 values.  One barrier pair per call (round 3 took two per round plus an atomic: the ten
// rounds of a slice cost more than its whole sweep).
__device__ __forceinline__ void wave_top_rounds(double (&v)[SEL_IPT], double (&tops)[SEL_K]) {
  const int lane = threadIdx.x & 63;
  for (int r = 0; r < SEL_K; ++r) {
    double m = v[0];
#pragma unroll
    for (int i = 1; i < SEL_IPT; ++i) m = v[i] > m ? v[i] : m;
    const double wm = wave_max_f64(m);
    const unsigned long long holders = __ballot(m == wm);
    if (lane == __ffsll((long long)holders) - 1) {   // consume ONE instance of the maximum
      bool done = false;
#pragma unroll
      for (int i = 0; i < SEL_IPT; ++i)
        if (!done && v[i] == wm) {
          v[i] = -1.0;
          done = true;
        }
    }
    tops[r] = wm;
  }
}

__device__ __forceinline__ void block_top_rounds(double (&v)[SEL_IPT], double* red, double (&tops)[SEL_K]) {
  __shared__ double lists[4 * SEL_K + SEL_K];
  (void)red;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  wave_top_rounds(v, tops);
  if (lane < SEL_K) {
    double t = -1.0;
    for (int r = 0; r < SEL_K; ++r) t = (lane == r) ? tops[r] : t;
    lists[wave * SEL_K + lane] = t;
  }
  __syncthreads();
  if (wave == 0) {
    double w[SEL_IPT];
#pragma unroll
    for (int i = 0; i < SEL_IPT; ++i) w[i] = -1.0;
    if (lane < 4 * SEL_K) w[0] = lists[lane];
    double t2[SEL_K];
    wave_top_rounds(w, t2);
    if (lane < SEL_K) {
      double t = -1.0;
      for (int r = 0; r < SEL_K; ++r) t = (lane == r) ? t2[r] : t;
      lists[4 * SEL_K + lane] = t;
    }
  }
  __syncthreads();
  for (int r = 0; r < SEL_K; ++r) tops[r] = lists[4 * SEL_K + r];
  __syncthreads();                                   // (the lists are rewritten by the caller's next pass)
}

// blockIdx.y = query of a batched selection (strides in elements; 0 for a single query)
__global__ void __launch_bounds__(256) topk_local_kernel(const double* __restrict__ score, int n,
                                                        double* __restrict__ block_tops, size_t score_stride,
                                                        size_t ws_stride) {
  __shared__ double red[4];
  score += blockIdx.y * score_stride;
  block_tops += blockIdx.y * ws_stride;
  const int per_block = 256 * SEL_IPT;
  double v[SEL_IPT], tops[SEL_K];
#pragma unroll
  for (int i = 0; i < SEL_IPT; ++i) {
    const int e = blockIdx.x * per_block + i * 256 + threadIdx.x;
    v[i] = e < n ? score[e] : -1.0;
  }
  block_top_rounds(v, red, tops);
  if (threadIdx.x == 0)
    for (int r = 0; r < SEL_K; ++r) block_tops[blockIdx.x * SEL_K + r] = tops[r];
}

__global__ void __launch_bounds__(256) topk_merge_kernel(const double* __restrict__ block_tops, int n_lists,
                                                        int n_entries, double* __restrict__ threshold,
                                                        int* __restrict__ cursor, size_t ws_stride) {
  __shared__ double red[4];
  block_tops += blockIdx.y * ws_stride;
  threshold += blockIdx.y * ws_stride;
  cursor += blockIdx.y;
  // the 10th largest score lies among the per-block top-10 lists; fold them 1024 at a time
  double carry[SEL_K];
  for (int r = 0; r < SEL_K; ++r) carry[r] = -1.0;
  const int total = n_lists * SEL_K;
  for (int base = 0; base < total; base += 256 * SEL_IPT - SEL_K) {
    double v[SEL_IPT], tops[SEL_K];
#pragma unroll
    for (int i = 0; i < SEL_IPT; ++i) {
      const int j = i * 256 + threadIdx.x;          // slots [0, SEL_K) carry the running top-10
      double x = -1.0;
      if (j >= SEL_K && base + j - SEL_K < total) x = block_tops[base + j - SEL_K];
      v[i] = x;
    }
    if (threadIdx.x < SEL_K) {
      double c = -1.0;
      for (int r = 0; r < SEL_K; ++r) c = ((int)threadIdx.x == r) ? carry[r] : c;
      v[0] = c;
    }
    block_top_rounds(v, red, tops);
    for (int r = 0; r < SEL_K; ++r) carry[r] = tops[r];   // tops[] is uniform across the block
  }
  if (threadIdx.x == 0) {
    // fewer than 10 entries in total, or a 10th largest of 0: keep every positive score
    double t = carry[SEL_K - 1];
    if (n_entries <= 64 || t < 0.0) t = 0.0;
    *threshold = t;
    *cursor = 0;
  }
}

__global__ void __launch_bounds__(256) compact_kernel(const double* __restrict__ score, const int* __restrict__ top,
                                                     int n, const double* __restrict__ threshold,
                                                     int* __restrict__ cursor, int cap, int* __restrict__ out_idx,
                                                     int* __restrict__ out_top, double* __restrict__ out_score,
                                                     size_t score_stride, size_t ws_stride) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  score += blockIdx.y * score_stride;
  top += blockIdx.y * score_stride;
  threshold += blockIdx.y * ws_stride;
  cursor += blockIdx.y;
  out_idx += (size_t)blockIdx.y * cap;
  out_top += (size_t)blockIdx.y * cap;
  out_score += (size_t)blockIdx.y * cap;
  const double s = score[e];
  if (s >= *threshold && s > 0.0) {
    const int pos = atomicAdd(cursor, 1);
    if (pos < cap) {
      out_idx[pos] = e;
      out_top[pos] = top[e];
      out_score[pos] = s;
    }
  }
}


// ---- sweep + selection fused (round 4): the scores never go to memory ---------------------------------------------------
// The batched sweep above writes a float64 score and an int32 relation index per (query, entry) -- 12 B x Q x N, 19 MB for
// the 48 query relations of a guided batch over 32 768 entries -- which three selection launches then read back twice.
// Only the 10th largest score of every query (the threshold) and the few entries that reach it are ever used.  Two launches:
//   sweep_tops    : grid (entry slices of 1024, queries): every thread scores its 4 entries in registers, the workgroup
//                   extracts the slice's 10 largest scores (block_top_rounds) -> block_tops[query][slice][10];
//                   the (0, query) workgroup also zeroes the query's cursor;
//   sweep_compact : same grid: every workgroup first folds the query's per-slice lists into the threshold (n_slices x 10
//                   values: one block_top_rounds pass per 1014 of them), then scores its 4 entries AGAIN (the integer-coded
//                   CSR is 1.2 MB: it stays in L2) and appends the survivors.
// Same arithmetic, same comparisons: identical survivors (order arbitrary as before; the host sorts them by index).
__global__ void __launch_bounds__(256) sweep_tops_kernel(
    const int* __restrict__ spk, const int* __restrict__ rel_off, const int* __restrict__ rel_sense,
    const int* __restrict__ rel_conn, const double* __restrict__ rel_prom, int n_entries,
    const double* __restrict__ params, double* __restrict__ block_tops, int* __restrict__ cursor, size_t ws_stride) {
  __shared__ double red[4];
  const double* qp = params + 4 * blockIdx.y;
  const int q_sense = (int)qp[0], q_conn = (int)qp[1], q_spk = (int)qp[2];
  const double q_prom = qp[3];
  double v[SEL_IPT], tops[SEL_K];
#pragma unroll
  for (int i = 0; i < SEL_IPT; ++i) {
    const int e = blockIdx.x * (256 * SEL_IPT) + i * 256 + threadIdx.x;
    v[i] = -1.0;
    if (e < n_entries) {
      int tp;
      discourse_score_value(e, spk, rel_off, rel_sense, rel_conn, rel_prom, q_sense, q_conn, q_spk, q_prom, v[i], tp);
    }
  }
  block_top_rounds(v, red, tops);
  if (threadIdx.x == 0) {
    double* bt = block_tops + blockIdx.y * ws_stride + blockIdx.x * SEL_K;
    for (int r = 0; r < SEL_K; ++r) bt[r] = tops[r];
    if (blockIdx.x == 0) cursor[blockIdx.y] = 0;
  }
}

__global__ void __launch_bounds__(256) sweep_compact_kernel(
    const int* __restrict__ spk, const int* __restrict__ rel_off, const int* __restrict__ rel_sense,
    const int* __restrict__ rel_conn, const double* __restrict__ rel_prom, int n_entries,
    const double* __restrict__ params, const double* __restrict__ block_tops, int n_lists, int* __restrict__ cursor,
    int cap, int* __restrict__ out_idx, int* __restrict__ out_top, double* __restrict__ out_score, size_t ws_stride) {
  __shared__ double red[4];
  block_tops += blockIdx.y * ws_stride;
  // threshold = 10th largest of the query's per-slice lists (as topk_merge_kernel)
  double carry[SEL_K];
  for (int r = 0; r < SEL_K; ++r) carry[r] = -1.0;
  const int total = n_lists * SEL_K;
  for (int base = 0; base < total; base += 256 * SEL_IPT - SEL_K) {
    double v[SEL_IPT], tops[SEL_K];
#pragma unroll
    for (int i = 0; i < SEL_IPT; ++i) {
      const int j = i * 256 + threadIdx.x;
      double x = -1.0;
      if (j >= SEL_K && base + j - SEL_K < total) x = block_tops[base + j - SEL_K];
      v[i] = x;
    }
    if (threadIdx.x < SEL_K) {
      double c = -1.0;
      for (int r = 0; r < SEL_K; ++r) c = ((int)threadIdx.x == r) ? carry[r] : c;
      v[0] = c;
    }
    block_top_rounds(v, red, tops);
    for (int r = 0; r < SEL_K; ++r) carry[r] = tops[r];
  }
  double thr = carry[SEL_K - 1];
  if (n_entries <= 64 || thr < 0.0) thr = 0.0;
  const double* qp = params + 4 * blockIdx.y;
  const int q_sense = (int)qp[0], q_conn = (int)qp[1], q_spk = (int)qp[2];
  const double q_prom = qp[3];
  cursor += blockIdx.y;
  out_idx += (size_t)blockIdx.y * cap;
  out_top += (size_t)blockIdx.y * cap;
  out_score += (size_t)blockIdx.y * cap;
#pragma unroll
  for (int i = 0; i < SEL_IPT; ++i) {
    const int e = blockIdx.x * (256 * SEL_IPT) + i * 256 + threadIdx.x;
    if (e >= n_entries) continue;
    double sc;
    int tp;
    discourse_score_value(e, spk, rel_off, rel_sense, rel_conn, rel_prom, q_sense, q_conn, q_spk, q_prom, sc, tp);
    if (sc >= thr && sc > 0.0) {
      const int pos = atomicAdd(cursor, 1);
      if (pos < cap) {
        out_idx[pos] = e;
        out_top[pos] = tp;
        out_score[pos] = sc;
      }
    }
  }
}


// ------------------------------------------------------------------------------ fuzzy word similarity
// fuzzywuzzy 0.18 `fuzz.partial_ratio` (pure-python flavour: difflib.SequenceMatcher) of one query string against every
// word of the DB vocabulary, one thread per word -- the similarity `get_word_similarity_score` effectively returns
// (rag/utils.py:239-272: the embedding models are undefined, every call ends in `fuzz.partial_ratio(w1, w2) / 100`).
// Strings are code-point arrays.  difflib's matcher for sequences below its autojunk length, written out:
//   find_longest_match: longest common substring of a[alo:ahi], b[blo:bhi]; among equals the earliest in a, then in b
//   get_matching_blocks: LIFO queue of the pieces left and right of each match
//   ratio = 2 * matched / (len a + len b)
// partial_ratio: for every diagonal d = max(j - i, 0) of the outer blocks (the (la, lb, 0) sentinel included) the ratio
// of `shorter` against longer[d : d + la]; > .995 -> 100; else int(round(100 * max)) (round half to even, like Python).
constexpr int PR_MAX = 48;   // longest string handled on the device (longer: out = NaN, the host computes it)

struct PrQuery {
  int len;
  int c[PR_MAX];
};

__device__ int pr_longest(const int* a, const int* b, int alo, int ahi, int blo, int bhi, int& bi, int& bj) {
  unsigned char prev[PR_MAX], cur[PR_MAX];
  for (int j = blo; j < bhi; ++j) prev[j] = 0;
  int best = 0;
  bi = alo;
  bj = blo;
  for (int i = alo; i < ahi; ++i) {
    const int ai = a[i];
    for (int j = blo; j < bhi; ++j) {
      int k = 0;
      if (b[j] == ai) {
        k = (j > blo ? prev[j - 1] : 0) + 1;
        if (k > best) {
          best = k;
          bi = i - k + 1;
          bj = j - k + 1;
        }
      }
      cur[j] = (unsigned char)k;
    }
    for (int j = blo; j < bhi; ++j) prev[j] = cur[j];
  }
  return best;
}

// matched characters of SequenceMatcher(None, a, b); diag (optional): bit d set for every block diagonal max(j - i, 0)
__device__ int pr_matches(const int* a, int la, const int* b, int lb, unsigned long long* diag) {
  short st[PR_MAX + 2][4];
  int sp = 0, total = 0;
  st[0][0] = 0; st[0][1] = (short)la; st[0][2] = 0; st[0][3] = (short)lb;
  sp = 1;
  while (sp > 0) {
    --sp;
    const int alo = st[sp][0], ahi = st[sp][1], blo = st[sp][2], bhi = st[sp][3];
    int i, j;
    const int k = pr_longest(a, b, alo, ahi, blo, bhi, i, j);
    if (k) {
      total += k;
      if (diag) *diag |= 1ull << (j - i > 0 ? j - i : 0);
      if (alo < i && blo < j) {
        st[sp][0] = (short)alo; st[sp][1] = (short)i; st[sp][2] = (short)blo; st[sp][3] = (short)j;
        ++sp;
      }
      if (i + k < ahi && j + k < bhi) {
        st[sp][0] = (short)(i + k); st[sp][1] = (short)ahi; st[sp][2] = (short)(j + k); st[sp][3] = (short)bhi;
        ++sp;
      }
    }
  }
  return total;
}

__global__ void __launch_bounds__(64) partial_ratio_kernel(const int* __restrict__ vocab, const int* __restrict__ vlen,
                                                           int n_words, int stride, const PrQuery q,
                                                           double* __restrict__ out) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n_words) return;
  const int l1 = vlen[v], l2 = q.len;
  if (l1 > PR_MAX || l2 > PR_MAX) {
    out[v] = __longlong_as_double(0x7ff8000000000000ll);   // NaN: too long for the device form
    return;
  }
  int s1[PR_MAX], s2[PR_MAX];
  for (int i = 0; i < l1; ++i) s1[i] = vocab[(size_t)v * stride + i];
  for (int i = 0; i < l2; ++i) s2[i] = q.c[i];
  bool same = l1 == l2;
  for (int i = 0; same && i < l1; ++i) same = s1[i] == s2[i];
  if (same) { out[v] = 1.0; return; }             // check_for_equivalence (also two empty strings)
  if (l1 == 0 || l2 == 0) { out[v] = 0.0; return; }
  const int* a = l1 <= l2 ? s1 : s2;               // shorter (ties: the first argument = the DB word)
  const int* b = l1 <= l2 ? s2 : s1;
  const int la = l1 <= l2 ? l1 : l2, lb = l1 <= l2 ? l2 : l1;
  unsigned long long diag = 1ull << (lb - la);     // the (la, lb, 0) sentinel block
  pr_matches(a, la, b, lb, &diag);
  double best = 0.0;
  bool hit = false;
  for (int d = 0; d <= lb && !hit; ++d) {
    if (!((diag >> d) & 1ull)) continue;
    const int ls = (d + la <= lb) ? la : lb - d;   // longer[d : d + la] is cut at the end of the string
    const int m = pr_matches(a, la, b + d, ls, nullptr);
    const double r = (la + ls) ? 2.0 * (double)m / (double)(la + ls) : 1.0;
    if (r > .995) hit = true;
    best = r > best ? r : best;
  }
  out[v] = hit ? 1.0 : rint(100.0 * best) / 100.0;
}
}  // namespace

static int select_launch(rg_handle* h, const double* score, const int* top, int n_entries, int n_queries,
                         double* workspace, int* cursor, int cap, int* out_idx, int* out_top, double* out_score,
                         void* stream) {
  const int nb = (n_entries + 256 * SEL_IPT - 1) / (256 * SEL_IPT);
  const size_t ws_stride = (size_t)nb * SEL_K + 1, sc_stride = (size_t)n_entries;
  hipStream_t s = rg_stream(stream);
  // workspace per query: [nb * 10] per-block tops, then the threshold
  hipLaunchKernelGGL(topk_local_kernel, dim3(nb, n_queries), dim3(256), 0, s, score, n_entries, workspace, sc_stride,
                     ws_stride);
  hipLaunchKernelGGL(topk_merge_kernel, dim3(1, n_queries), dim3(256), 0, s, workspace, nb, n_entries,
                     workspace + nb * SEL_K, cursor, ws_stride);
  hipLaunchKernelGGL(compact_kernel, dim3((n_entries + 255) / 256, n_queries), dim3(256), 0, s, score, top, n_entries,
                     workspace + nb * SEL_K, cursor, cap, out_idx, out_top, out_score, sc_stride, ws_stride);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_select_top_scores(rg_handle* h, const double* score, const int* top, int n_entries,
                                    double* workspace, int* cursor, int cap, int* out_idx, int* out_top,
                                    double* out_score, void* stream) {
  RG_REQUIRE(h, score && top && workspace && cursor && out_idx && out_top && out_score, "null pointer");
  RG_REQUIRE(h, n_entries > 0 && cap > 0, "bad shape");
  return select_launch(h, score, top, n_entries, 1, workspace, cursor, cap, out_idx, out_top, out_score, stream);
}

extern "C" int rg_select_top_scores_batched(rg_handle* h, const double* score, const int* top, int n_entries,
                                            int n_queries, double* workspace, int* cursor, int cap, int* out_idx,
                                            int* out_top, double* out_score, void* stream) {
  RG_REQUIRE(h, score && top && workspace && cursor && out_idx && out_top && out_score, "null pointer");
  RG_REQUIRE(h, n_entries > 0 && cap > 0 && n_queries > 0 && n_queries <= 65535, "bad shape");
  return select_launch(h, score, top, n_entries, n_queries, workspace, cursor, cap, out_idx, out_top, out_score, stream);
}

extern "C" int rg_discourse_select_fused(rg_handle* h, const int* spk, const int* rel_off, const int* rel_sense,
                                        const int* rel_conn, const double* rel_prom, int n_entries, const double* params,
                                        int n_queries, double* workspace, int* cursor, int cap, int* out_idx, int* out_top,
                                        double* out_score, void* stream) {
  RG_REQUIRE(h, spk && rel_off && rel_sense && rel_conn && rel_prom && params, "null pointer");
  RG_REQUIRE(h, workspace && cursor && out_idx && out_top && out_score, "null pointer");
  RG_REQUIRE(h, n_entries > 0 && cap > 0 && n_queries > 0 && n_queries <= 65535, "bad shape");
  const int nb = (n_entries + 256 * SEL_IPT - 1) / (256 * SEL_IPT);
  const size_t ws_stride = (size_t)nb * SEL_K + 1;
  hipStream_t s = rg_stream(stream);
  hipLaunchKernelGGL(sweep_tops_kernel, dim3(nb, n_queries), dim3(256), 0, s, spk, rel_off, rel_sense, rel_conn, rel_prom,
                     n_entries, params, workspace, cursor, ws_stride);
  hipLaunchKernelGGL(sweep_compact_kernel, dim3(nb, n_queries), dim3(256), 0, s, spk, rel_off, rel_sense, rel_conn, rel_prom,
                     n_entries, params, workspace, nb, cursor, cap, out_idx, out_top, out_score, ws_stride);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_select_workspace_doubles(int n_entries) {
  return (n_entries + 256 * SEL_IPT - 1) / (256 * SEL_IPT) * SEL_K + 1;
}

extern "C" int rg_discourse_scores_batched(rg_handle* h, const int* spk, const int* rel_off, const int* rel_sense,
                                           const int* rel_conn, const double* rel_prom, int n_entries,
                                           const double* params, int n_queries, double* score_out, int* top_out,
                                           void* stream) {
  RG_REQUIRE(h, spk && rel_off && rel_sense && rel_conn && rel_prom && params && score_out && top_out, "null pointer");
  RG_REQUIRE(h, n_entries > 0 && n_queries > 0 && n_queries <= 65535, "bad shape");
  hipLaunchKernelGGL(discourse_scores_batched_kernel, dim3((n_entries + 255) / 256, n_queries), dim3(256), 0,
                     rg_stream(stream), spk, rel_off, rel_sense, rel_conn, rel_prom, n_entries, params, score_out, top_out);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

// ---- the batched search: buffers the handle owns ---------------------------------------------------------------------------
// A device buffer with a page-locked host twin, grown on demand (a growth frees the old pair: hipFree waits for the device).
struct rg_twin_buf {
  void* dev = nullptr;
  void* host = nullptr;
  size_t bytes = 0;
  bool reserve(size_t want, bool with_host = true) {
    if (want <= bytes) return true;
    release();
    if (hipMalloc(&dev, want) != hipSuccess) { dev = nullptr; return false; }
    if (with_host && hipHostMalloc(&host, want, hipHostMallocDefault) != hipSuccess) { host = nullptr; release(); return false; }
    bytes = want;
    return true;
  }
  void release() {
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = nullptr;
    bytes = 0;
  }
};

// Survivors of one guided batch of the benchmark's 32 768-entry database (16 clips, 48 query relations): 1 492 rows, 266 in
// the largest query (NOTEBOOK 28); the block starts at 4 096 rows (64 KiB) and grows when a batch does not fit.
constexpr int PACK_ROWS_INITIAL = 4096;

struct rg_retrieval_state {
  rg_twin_buf sweep;      // device only: params, selection workspace, cursor and the [Q][cap] survivor lists
  rg_twin_buf pack;       // counts [pack_q] (padded to 16 bytes), then pack_rows rows
  rg_twin_buf upload;     // staged host -> device block: sweep parameters, or query table + pairs
  rg_twin_buf sims;       // similarities of the pairs (rg_discourse_search_batch)
  int pack_rows = PACK_ROWS_INITIAL, pack_q = 0;
  hipEvent_t upload_used = nullptr;   // recorded behind the last consumer of `upload`
  bool upload_pending = false;
  ~rg_retrieval_state() {
    sweep.release(); pack.release(); upload.release(); sims.release();
    if (upload_used) (void)hipEventDestroy(upload_used);
  }
};

void rg_retrieval_release(rg_handle* h) {
  delete h->retr;
  h->retr = nullptr;
}

static rg_retrieval_state* retrieval_state(rg_handle* h) {
  if (!h->retr) h->retr = new rg_retrieval_state();
  return h->retr;
}

#define RG_HIP(h, call, what)                                                            \
  do {                                                                                   \
    hipError_t e__ = (call);                                                             \
    if (e__ != hipSuccess) {                                                             \
      (h)->err = std::string(__func__) + ": " + (what) + ": " + hipGetErrorString(e__);  \
      return RG_ERR_HIP;                                                                 \
    }                                                                                    \
  } while (0)

static size_t pack_header_bytes(int n_queries) { return ((size_t)n_queries * sizeof(int) + 15) / 16 * 16; }

// The staging block for the next upload, `bytes` large: waits until whatever read the previous one has run.
static int upload_stage(rg_handle* h, rg_retrieval_state* st, size_t bytes) {
  if (st->upload_pending) {
    RG_HIP(h, hipEventSynchronize(st->upload_used), "waiting for the previous upload's consumer");
    st->upload_pending = false;
  }
  if (!st->upload_used) RG_HIP(h, hipEventCreateWithFlags(&st->upload_used, hipEventDisableTiming), "event");
  if (!st->upload.reserve(bytes < 4096 ? 4096 : bytes * 2)) {
    h->err = std::string(__func__) + ": cannot allocate the upload block";
    return RG_ERR_HIP;
  }
  return RG_OK;
}

// One launch for n_pairs (entry, query) pairs; table and pairs go up in one copy from page-locked memory.
static int sims_many_launch(rg_handle* h, const void* const* q_feat_host, const int* q_len_host, int n_queries,
                            const int* pair_entry_host, const int* pair_query_host, int n_pairs, const float* feats,
                            const int64_t* feat_off, int n_entries, int dim, double* out, void* stream) {
  for (int p = 0; p < n_pairs; ++p) {
    const int e = pair_entry_host[p], q = pair_query_host[p];
    RG_REQUIRE(h, e >= 0 && e < n_entries && q >= 0 && q < n_queries, "pair out of range");
    RG_REQUIRE(h, q_feat_host[q] != nullptr && q_len_host[q] > 0, "a pair's query has no features");
    RG_REQUIRE(h, (reinterpret_cast<uintptr_t>(q_feat_host[q]) & 15) == 0, "query features must be 16-byte aligned");
  }
  rg_retrieval_state* st = retrieval_state(h);
  const size_t tab = (size_t)n_queries * sizeof(SimQuery), bytes = tab + (size_t)n_pairs * sizeof(SimPair);
  const int rc = upload_stage(h, st, bytes);
  if (rc != RG_OK) return rc;
  SimQuery* tq = static_cast<SimQuery*>(st->upload.host);
  for (int q = 0; q < n_queries; ++q) tq[q] = SimQuery{static_cast<const float*>(q_feat_host[q]), q_len_host[q], 0};
  SimPair* tp = reinterpret_cast<SimPair*>(static_cast<char*>(st->upload.host) + tab);
  for (int p = 0; p < n_pairs; ++p) tp[p] = SimPair{pair_entry_host[p], pair_query_host[p]};
  hipStream_t s = rg_stream(stream);
  RG_HIP(h, hipMemcpyAsync(st->upload.dev, st->upload.host, bytes, hipMemcpyHostToDevice, s), "upload");
  hipLaunchKernelGGL(text_diag_sim_many_kernel, dim3(n_pairs), dim3(256), 0, s, static_cast<const SimQuery*>(st->upload.dev),
                     reinterpret_cast<const SimPair*>(static_cast<const char*>(st->upload.dev) + tab), feats, feat_off, dim, out);
  RG_CHECK_LAUNCH(h);
  RG_HIP(h, hipEventRecord(st->upload_used, s), "event record");
  st->upload_pending = true;
  return RG_OK;
}

extern "C" int rg_text_diag_sim_many(rg_handle* h, const void* const* q_feat_host, const int* q_len_host, int n_queries,
                                     const int* pair_entry_host, const int* pair_query_host, int n_pairs, const float* feats,
                                     const int64_t* feat_off, int n_entries, int dim, double* out, void* stream) {
  RG_REQUIRE(h, q_feat_host && q_len_host && pair_entry_host && pair_query_host && feats && feat_off && out, "null pointer");
  RG_REQUIRE(h, n_queries > 0 && n_pairs > 0 && n_entries > 0 && dim > 0 && dim % 4 == 0, "bad shape");
  return sims_many_launch(h, q_feat_host, q_len_host, n_queries, pair_entry_host, pair_query_host, n_pairs, feats, feat_off,
                          n_entries, dim, out, stream);
}

extern "C" int rg_retrieval_pack_rows(rg_handle* h, int rows) {
  if (!h) return 0;
  rg_retrieval_state* st = retrieval_state(h);
  if (rows > 0 && rows != st->pack_rows) {
    (void)hipDeviceSynchronize();
    st->pack.release();
    st->pack_rows = rows;
    st->pack_q = 0;
  }
  return st->pack_rows;
}

// Steps 2-7 of the search (include/rg_gesture.h rg_discourse_search_batch) over the device survivor lists of any sweep:
// d_cursor [Q], d_idx / d_top / d_score [Q][cap].  The callers have checked the arguments.
static int rank_survivors(rg_handle* h, const int* d_cursor, const int* d_idx, const int* d_top, const double* d_score,
                          int Q, int cap, const float* feats, const int64_t* feat_off, int n_entries, int dim,
                          const void* const* q_feat_host, const int* q_len_host, int* n_ranked_host, int* entry_host,
                          int* top_host, void* stream) {
  rg_retrieval_state* st = retrieval_state(h);
  hipStream_t s = rg_stream(stream);
  int rc = RG_OK;
  // ---- 2./3. pack, one fixed-size read-back, synchronise; a batch that does not fit grows the block and packs again
  const int* counts = nullptr;
  const PackRow* rows = nullptr;
  for (int attempt = 0;; ++attempt) {
    if (Q > st->pack_q) {
      st->pack.release();
      st->pack_q = (Q + 63) / 64 * 64;
    }
    const size_t head = pack_header_bytes(st->pack_q), block = head + (size_t)st->pack_rows * sizeof(PackRow);
    if (!st->pack.reserve(block)) {
      h->err = std::string(__func__) + ": cannot allocate the survivor block";
      return RG_ERR_HIP;
    }
    hipLaunchKernelGGL(survivor_pack_kernel, dim3(PACK_BX, Q), dim3(256), 0, s, d_cursor, d_idx, d_top, d_score, Q, cap,
                       (long long)st->pack_rows, static_cast<int*>(st->pack.dev),
                       reinterpret_cast<PackRow*>(static_cast<char*>(st->pack.dev) + head));
    RG_CHECK_LAUNCH(h);
    RG_HIP(h, hipMemcpyAsync(st->pack.host, st->pack.dev, block, hipMemcpyDeviceToHost, s), "survivor read-back");
    RG_HIP(h, hipStreamSynchronize(s), "synchronise");
    counts = static_cast<const int*>(st->pack.host);
    rows = reinterpret_cast<const PackRow*>(static_cast<const char*>(st->pack.host) + head);
    long long total = 0;
    for (int q = 0; q < Q; ++q) {
      RG_REQUIRE(h, counts[q] >= 0 && counts[q] <= cap, "survivor count out of range");
      total += counts[q];
    }
    if (total <= st->pack_rows) break;
    RG_REQUIRE(h, attempt == 0 && total <= 0x7fffffffll / 2, "the survivor block did not fit after it was grown");
    const long long grown = std::max(2ll * st->pack_rows, (total + 1023) / 1024 * 1024);
    st->pack.release();
    st->pack_rows = (int)grown;
  }
  // ---- 4. rank: the leading score tiers of every query; the members of the multi-member tiers are the pairs
  std::vector<rg_rank_cut> cuts(Q);
  std::vector<int> pair_entry, pair_query, sidx, stop;
  std::vector<double> sscore;
  size_t row0 = 0;
  for (int q = 0; q < Q; ++q) {
    const int c = counts[q];
    sidx.resize(c); stop.resize(c); sscore.resize(c);
    for (int i = 0; i < c; ++i) {
      const PackRow& r = rows[row0 + i];
      RG_REQUIRE(h, r.idx >= 0 && r.idx < n_entries, "survivor entry out of range");
      sidx[i] = r.idx; stop[i] = r.top; sscore[i] = r.score;
    }
    row0 += c;
    rg_rank_cut_tiers(sidx.data(), stop.data(), sscore.data(), c, cuts[q]);
    for (const auto& t : cuts[q].tiers)
      if (t.second > 1)
        for (int k = 0; k < t.second; ++k) {
          pair_entry.push_back(cuts[q].entry[t.first + k]);
          pair_query.push_back(q);
        }
  }
  // ---- 5./6. one launch for every tie tier, read-back, synchronise
  const int n_pairs = (int)pair_entry.size();
  if (n_pairs > 0) {
    if (!st->sims.reserve((size_t)n_pairs * 8 < 65536 ? 65536 : (size_t)n_pairs * 16)) {
      h->err = std::string(__func__) + ": cannot allocate the similarity buffer";
      return RG_ERR_HIP;
    }
    rc = sims_many_launch(h, q_feat_host, q_len_host, Q, pair_entry.data(), pair_query.data(), n_pairs, feats, feat_off,
                          n_entries, dim, static_cast<double*>(st->sims.dev), stream);
    if (rc != RG_OK) return rc;
    RG_HIP(h, hipMemcpyAsync(st->sims.host, st->sims.dev, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, s), "similarity read-back");
    RG_HIP(h, hipStreamSynchronize(s), "synchronise");
    st->upload_pending = false;
  }
  // ---- 7. tie-break walk
  const double* sims = static_cast<const double*>(st->sims.host);
  size_t s0 = 0;
  for (int q = 0; q < Q; ++q) {
    n_ranked_host[q] = rg_rank_walk(cuts[q], sims + s0, entry_host + (size_t)q * RG_RANK_MAX, top_host + (size_t)q * RG_RANK_MAX);
    s0 += cuts[q].multi_members();
  }
  return RG_OK;
}

extern "C" int rg_rank_survivors_batch(rg_handle* h, const int* cursor, const int* idx, const int* top, const double* score,
                                      int n_queries, int cap, const float* feats, const int64_t* feat_off, int n_entries,
                                      int dim, const void* const* q_feat_host, const int* q_len_host, int* n_ranked_host,
                                      int* entry_host, int* top_host, void* stream) {
  RG_REQUIRE(h, cursor && idx && top && score && feats && feat_off, "null pointer");
  RG_REQUIRE(h, q_feat_host && q_len_host && n_ranked_host && entry_host && top_host, "null pointer");
  RG_REQUIRE(h, n_entries > 0 && cap > 0 && n_queries > 0 && n_queries <= 65535 && dim > 0 && dim % 4 == 0, "bad shape");
  return rank_survivors(h, cursor, idx, top, score, n_queries, cap, feats, feat_off, n_entries, dim, q_feat_host, q_len_host,
                        n_ranked_host, entry_host, top_host, stream);
}

extern "C" int rg_discourse_search_batch(rg_handle* h, const int* spk, const int* rel_off, const int* rel_sense,
                                        const int* rel_conn, const double* rel_prom, int n_entries, const float* feats,
                                        const int64_t* feat_off, int dim, const double* params_host, int n_queries,
                                        const void* const* q_feat_host, const int* q_len_host, int* n_ranked_host,
                                        int* entry_host, int* top_host, void* stream) {
  RG_REQUIRE(h, spk && rel_off && rel_sense && rel_conn && rel_prom && feats && feat_off, "null pointer");
  RG_REQUIRE(h, params_host && q_feat_host && q_len_host && n_ranked_host && entry_host && top_host, "null pointer");
  RG_REQUIRE(h, n_entries > 0 && n_queries > 0 && n_queries <= 65535 && dim > 0 && dim % 4 == 0, "bad shape");
  rg_retrieval_state* st = retrieval_state(h);
  hipStream_t s = rg_stream(stream);
  const int Q = n_queries, cap = n_entries;
  // ---- 1. sweep: parameters up, two launches
  const size_t ws_doubles = (size_t)rg_select_workspace_doubles(n_entries);
  const size_t o_params = 0, o_ws = o_params + (size_t)Q * 4 * 8, o_score = o_ws + (size_t)Q * ws_doubles * 8,
               o_idx = o_score + (size_t)Q * cap * 8, o_top = o_idx + (size_t)Q * cap * 4, o_cursor = o_top + (size_t)Q * cap * 4,
               sweep_bytes = o_cursor + (size_t)Q * 4;
  if (!st->sweep.reserve(sweep_bytes, false)) {
    h->err = std::string(__func__) + ": cannot allocate the sweep buffers";
    return RG_ERR_HIP;
  }
  char* sw = static_cast<char*>(st->sweep.dev);
  double* d_params = reinterpret_cast<double*>(sw + o_params);
  double* d_ws = reinterpret_cast<double*>(sw + o_ws);
  double* d_score = reinterpret_cast<double*>(sw + o_score);
  int* d_idx = reinterpret_cast<int*>(sw + o_idx);
  int* d_top = reinterpret_cast<int*>(sw + o_top);
  int* d_cursor = reinterpret_cast<int*>(sw + o_cursor);
  int rc = upload_stage(h, st, (size_t)Q * 4 * 8);
  if (rc != RG_OK) return rc;
  std::copy(params_host, params_host + (size_t)Q * 4, static_cast<double*>(st->upload.host));
  RG_HIP(h, hipMemcpyAsync(d_params, st->upload.host, (size_t)Q * 4 * 8, hipMemcpyHostToDevice, s), "parameter upload");
  rc = rg_discourse_select_fused(h, spk, rel_off, rel_sense, rel_conn, rel_prom, n_entries, d_params, Q, d_ws, d_cursor, cap,
                                 d_idx, d_top, d_score, stream);
  if (rc != RG_OK) return rc;
  // ---- 2.-7. pack, read-back, ranking, tie-break similarities, read-back, walk
  return rank_survivors(h, d_cursor, d_idx, d_top, d_score, Q, cap, feats, feat_off, n_entries, dim, q_feat_host, q_len_host,
                        n_ranked_host, entry_host, top_host, stream);
}

extern "C" int rg_gesture_scores(rg_handle* h, const int* spk, const int* lab_off, const int* lab_type, const int* lab_word,
                                 const double* lab_prom, const double* word_sim, int n_entries, int q_type, int q_word,
                                 int q_spk, double spk_bonus, double q_prom, int sim_f32, double* score_out, int* top_out,
                                 void* stream) {
  RG_REQUIRE(h, spk && lab_off && lab_type && lab_word && word_sim && score_out && top_out, "null pointer");
  RG_REQUIRE(h, n_entries > 0, "empty database");
  hipLaunchKernelGGL(gesture_scores_kernel, dim3((n_entries + 255) / 256), dim3(256), 0, rg_stream(stream), spk, lab_off,
                     lab_type, lab_word, lab_prom, word_sim, n_entries, q_type, q_word, q_spk, spk_bonus, q_prom, sim_f32,
                     score_out, top_out);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_prosody_scores_batched(rg_handle* h, const int* spk, const int* word_off, const int* word_off_host,
                                         const int* word_code, const double* word_prom, const double* word_dur, int n_entries,
                                         int n_words, const double* sim, int n_vocab, const double* params, int n_queries,
                                         double* score_out, int* top_out, void* stream) {
  RG_REQUIRE(h, spk && word_off && word_off_host && word_code && word_prom && word_dur && sim && params && score_out && top_out,
             "null pointer");
  RG_REQUIRE(h, n_entries > 0 && n_words >= 0 && n_vocab >= 1 && n_queries >= 1, "bad shape");
  RG_REQUIRE(h, word_off_host[0] == 0, "offsets must start at 0 and not decrease");
  for (int e = 0; e < n_entries; ++e)
    RG_REQUIRE(h, word_off_host[e + 1] >= word_off_host[e], "offsets must start at 0 and not decrease");
  RG_REQUIRE(h, word_off_host[n_entries] == n_words, "word_off must end at n_words");
  hipLaunchKernelGGL(prosody_scores_batched_kernel, dim3((n_entries + PS_TILE - 1) / PS_TILE), dim3(256), 0, rg_stream(stream),
                     spk, word_off, word_code, word_prom, word_dur, n_entries, sim, n_vocab, params, n_queries, score_out,
                     top_out);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_motion_scores_batched(rg_handle* h, const float* lat, int n_entries, int L, int D, const int* spk,
                                        const float* qlat, const int* q_off, const int* q_off_host, const double* params,
                                        const double* params_host, int n_queries, double* score_out, int* top_out,
                                        float* sp_out, void* stream) {
  RG_REQUIRE(h, lat && spk && qlat && q_off && q_off_host && params && params_host && score_out && top_out, "null pointer");
  RG_REQUIRE(h, n_entries > 0, "empty database");
  RG_REQUIRE(h, ((uintptr_t)lat | (uintptr_t)qlat | (uintptr_t)sp_out) % 16 == 0, "lat, qlat and sp_out must be 16-byte aligned");
  unsigned mask = 0;
  const char* bad = rg_motion_check_queries(q_off_host, params_host, n_queries, L, D, &mask);
  RG_REQUIRE(h, bad == nullptr, bad);
  int parts = 0;
  for (int p = 0; p < RG_MOTION_PARTS; ++p) parts += (mask >> p) & 1u;
  const size_t lds = (size_t)parts * L * D * sizeof(float);
  RG_REQUIRE(h, lds <= 160u * 1024u, "the weighted parts of one entry must fit the LDS (parts * L * D * 4 <= 160 KiB)");
  static rg_attr_once once;
  RG_RESERVE_LDS(h, once, motion_scores_batched_kernel, 160 * 1024);
  hipLaunchKernelGGL(motion_scores_batched_kernel, dim3(n_entries), dim3(256), lds, rg_stream(stream), lat, n_entries, L, D, spk,
                     qlat, q_off, q_off_host[n_queries], params, n_queries, mask, score_out, top_out, sp_out);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_partial_ratio(rg_handle* h, const int* vocab, const int* vocab_len, int n_words, int stride,
                                const int* query_host, int query_len, double* out, void* stream) {
  RG_REQUIRE(h, vocab && vocab_len && out && (query_host || query_len == 0), "null pointer");
  RG_REQUIRE(h, n_words > 0 && stride >= 1 && query_len >= 0, "bad shape");
  PrQuery q;
  q.len = query_len;
  for (int i = 0; i < PR_MAX; ++i) q.c[i] = (i < query_len && query_len <= PR_MAX) ? query_host[i] : 0;
  hipLaunchKernelGGL(partial_ratio_kernel, dim3((n_words + 63) / 64), dim3(64), 0, rg_stream(stream), vocab, vocab_len,
                     n_words, stride, q, out);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_partial_ratio_max_len(void) { return PR_MAX; }
