// Host side of the batched exemplar search (csrc/rg_retrieval.hip rg_rank_survivors_batch / rg_discourse_search_batch): the
// ranking of one query's survivors.  Plain C++, no HIP: tests/test_retrieval_rank_host_cpu.py compiles it into a program of its
// own and checks it against the oracle's ranking_walk.
//
// This is the product's one statement of the reference's ranking walk (rag/discourse_retrieval.py:224-300, the same walk in
// gesture_type_retrieval.py and llm_retrieval.py):
//   survivors in ascending entry order; a stable sort by descending score; the leading tiers of bit-equal score while fewer
//   than RG_RANK_MAX entries are held, and only scores > 0; a multi-member tier reordered by a stable sort on descending
//   tie-break similarity (a similarity that is not a number goes behind every number); the first RG_RANK_MAX.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <numeric>
#include <utility>
#include <vector>

constexpr int RG_RANK_MAX = 10;   // entries the reference's ranking walk holds when it stops

// The leading score tiers of one query relation: entry / top hold the tiers' members back to back, in ranking order before
// any tie-break; tiers = (first member, members) of every tier.
struct rg_rank_cut {
  std::vector<int> entry, top;
  std::vector<std::pair<int, int>> tiers;
  int multi_members() const {       // members of the multi-member tiers = similarities rg_rank_walk reads
    int n = 0;
    for (const auto& t : tiers) n += t.second > 1 ? t.second : 0;
    return n;
  }
};

// Survivors (idx, top, score)[n] of one query in any order (the device appends them through an atomic cursor) -> the cut.
inline void rg_rank_cut_tiers(const int* idx, const int* top, const double* score, int n, rg_rank_cut& out) {
  out.entry.clear();
  out.top.clear();
  out.tiers.clear();
  std::vector<int> o(n > 0 ? n : 0);
  std::iota(o.begin(), o.end(), 0);
  std::sort(o.begin(), o.end(), [&](int a, int b) { return idx[a] < idx[b]; });                   // entries are distinct
  std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return score[a] > score[b]; });        // descending score, stable
  int i = 0, held = 0;
  while (i < n && held < RG_RANK_MAX) {
    const double sc = score[o[i]];
    if (!(sc > 0)) break;
    int j = i;
    while (j < n && score[o[j]] == sc) ++j;
    out.tiers.emplace_back((int)out.entry.size(), j - i);
    for (int k = i; k < j; ++k) {
      out.entry.push_back(idx[o[k]]);
      out.top.push_back(top[o[k]]);
    }
    held += j - i;
    i = j;
  }
}

// The ranking walk: sims = the tie-break similarities of the cut's multi-member tiers, members in the cut's order, tiers back
// to back (multi_members() values).  Writes at most RG_RANK_MAX (entry, top) pairs and returns their number.
inline int rg_rank_walk(const rg_rank_cut& cut, const double* sims, int* entry_out, int* top_out) {
  int n = 0, s0 = 0;
  std::vector<int> o;
  for (const auto& t : cut.tiers) {
    const int first = t.first, len = t.second;
    o.resize(len);
    std::iota(o.begin(), o.end(), 0);
    if (len > 1) {
      const double* s = sims + s0;
      // stable, ascending in -s, NaN behind every number
      std::stable_sort(o.begin(), o.end(), [&](int a, int b) {
        const double x = -s[a], y = -s[b];
        return x < y || (std::isnan(y) && !std::isnan(x));
      });
      s0 += len;
    }
    for (int k = 0; k < len && n < RG_RANK_MAX; ++k, ++n) {
      entry_out[n] = cut.entry[first + o[k]];
      top_out[n] = cut.top[first + o[k]];
    }
    if (n >= RG_RANK_MAX) break;
  }
  return n;
}

// ---- the motion method's sweep (rg_motion_scores_batched): its argument checks, on the HOST copies, before anything is launched.
constexpr int RG_MOTION_PARTS = 4;     // upper, hands, face, lower+trans: the model's part order
constexpr int RG_MOTION_MAX_L = 10;    // latent chunks of a window the kernel's unrolled offset loop covers
constexpr int RG_MOTION_PARAMS = 6;    // doubles per query: four part weights, speaker, bonus

// nullptr if the queries can be swept, else what is wrong with them.  q_off [n_queries + 1] in chunks; params
// [n_queries][RG_MOTION_PARAMS].  *part_mask gets the union of the parts any query weighs (what a workgroup stages).
inline const char* rg_motion_check_queries(const int* q_off, const double* params, int n_queries, int L, int D, unsigned* part_mask) {
  if (!q_off || !params || !part_mask) return "null pointer";
  if (n_queries < 1 || L < 1 || L > RG_MOTION_MAX_L || D < 4) return "bad shape (1 <= L <= 10, D >= 4, n_queries >= 1)";
  if (D % 4 != 0) return "D must be a multiple of 4";
  if (q_off[0] != 0) return "offsets must start at 0 and not decrease";
  unsigned mask = 0;
  for (int q = 0; q < n_queries; ++q) {
    if (q_off[q + 1] < q_off[q]) return "offsets must start at 0 and not decrease";
    const int nq = q_off[q + 1] - q_off[q];
    if (nq < 1 || nq > L) return "every query holds 1 ... L chunks (n_q out of range)";
    if (q_off[q + 1] > INT_MAX / (RG_MOTION_PARTS * D)) return "too many query chunks";
    const double* w = params + (size_t)q * RG_MOTION_PARAMS;
    bool any = false;
    for (int p = 0; p < RG_MOTION_PARTS; ++p) {
      if (!std::isfinite(w[p]) || w[p] < 0.0) return "weights must be finite and non-negative";
      if (w[p] > 0.0) {
        any = true;
        mask |= 1u << p;
      }
    }
    if (!any) return "weights must not all be zero";
    if (!std::isfinite(w[5])) return "the speaker bonus must be finite";
  }
  *part_mask = mask;
  return nullptr;
}
