// Word timings from a CTC model's character emissions, and word vectors laid onto motion frames (rag-gesture_amd/align.py,
// features.WindowFeatures(frame_words=True)):
//   rg_ctc_log_softmax : one wave per emission row, lane = class (V <= 64): the row maximum and the sum of expf(x - max) by an
//                        xor butterfly over the 64 lanes (a fixed order, every lane ends with the same bits), logp = (x - max) -
//                        logf(sum), and the lowest class index among the maxima (greedy decoding)
//   rg_ctc_align       : one workgroup per item of a ragged batch -- the Viterbi alignment of the item's emission rows against its
//                        blank-extended token sequence.  A thread owns 16 consecutive states in registers and one uint32 of 2-bit
//                        back-pointer codes per frame; per frame it hands its last two values to its right neighbour through a
//                        two-row LDS ping-pong (one barrier per frame) and reads the frame's emission row, staged in LDS one frame
//                        ahead.  One thread walks the back-pointers, then all threads find each token's first and last frame
//   rg_word_frames     : one workgroup per output frame -- the last word of the frame's window whose span covers it, the serial
//                        fp32 mean of that word's token rows (mogen/datasets/beatx_dataset.py:865-869, :1155-1156)
#include <math.h>

#include "rg_common.h"

namespace {

constexpr int WAVE = 64;
constexpr int LSM_THREADS = 256;                       // four rows per workgroup
constexpr int PER = RG_CTC_STATES_PER_THREAD;          // states (and 2-bit codes of one back-pointer word) per thread
constexpr int MAX_THREADS = RG_CTC_MAX_STATES / PER;   // 256
static_assert(PER == 16, "a thread's codes of one frame fill one uint32");
static_assert(RG_CTC_MAX_VOCAB == WAVE, "lane = class");
static_assert(MAX_THREADS % WAVE == 0 && MAX_THREADS <= 1024, "whole waves, one workgroup");

__global__ void __launch_bounds__(LSM_THREADS) ctc_log_softmax_kernel(const float* __restrict__ logits, int64_t rows, int V,
                                                                      float* __restrict__ logp, int* __restrict__ best) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * (LSM_THREADS / WAVE) + (threadIdx.x >> 6);
  if (row >= rows) return;                             // (the whole wave)
  const bool live = lane < V;
  const float x = live ? logits[row * V + lane] : -INFINITY;
  float mx = x;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
  const float d = x - mx;
  float sum = live ? expf(d) : 0.0f;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  if (live) logp[row * V + lane] = d - logf(sum);
  const unsigned long long at_max = __ballot(live && x == mx);
  if (lane == 0) best[row] = at_max ? __ffsll(at_max) - 1 : 0;
}

// max over the candidates in the order (stay, one back, two back), a strict > to replace; -> the 2-bit code
__device__ __forceinline__ unsigned pick(float stay, float one, float two, bool skip_ok, float& best) {
  unsigned code = 0;
  best = stay;
  if (one > best) best = one, code = 1;
  if (skip_ok && two > best) best = two, code = 2;
  return code;
}

__global__ void __launch_bounds__(MAX_THREADS) ctc_align_kernel(const float* __restrict__ logp, int V, const int64_t* __restrict__ frame_off,
                                                               const int* __restrict__ tokens, const int64_t* __restrict__ tok_off, int blank,
                                                               unsigned* __restrict__ backptr, const int64_t* __restrict__ backptr_off,
                                                               int* __restrict__ path, int* __restrict__ tok_first, int* __restrict__ tok_last,
                                                               float* __restrict__ score, int* __restrict__ status) {
  __shared__ float erow[2][RG_CTC_MAX_VOCAB];          // the emission rows of this frame and the next
  __shared__ float edge[2][2 * MAX_THREADS];           // every thread's last two values of the previous frame
  __shared__ float fin[2];                             // a[T - 1][S - 2], a[T - 1][S - 1]
  __shared__ int feasible;
  const int item = blockIdx.x, tid = threadIdx.x;
  const int64_t f0 = frame_off[item], k0 = tok_off[item];
  const int T = (int)(frame_off[item + 1] - f0), L = (int)(tok_off[item + 1] - k0);
  const int S = 2 * L + 1, W = (S + PER - 1) / PER;
  const int* y = tokens + k0;
  const float* E = logp + f0 * V;
  unsigned* bp = backptr + backptr_off[item];
  const int s0 = tid * PER;

  // the labels of this thread's states (blank beyond S: never read into a state below S) and where two back is a candidate
  int lab[PER];
  unsigned skip = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int s = s0 + k;
    lab[k] = blank;
    if ((s & 1) && s < S) {
      const int c = y[s >> 1];
      bad |= c < 0 || c >= V || c == blank;
      lab[k] = bad ? blank : c;
      if (s >= 3 && c != y[(s >> 1) - 1]) skip |= 1u << k;
    }
  }
  if (__syncthreads_or(bad)) {                         // a token outside the vocabulary or equal to blank: nothing is aligned
    for (int t = tid; t < T; t += blockDim.x) path[f0 + t] = 0;
    for (int j = tid; j < L; j += blockDim.x) tok_first[k0 + j] = tok_last[k0 + j] = -1;
    if (tid == 0) score[item] = -INFINITY, status[item] = 2;
    return;
  }

  if (tid < V) erow[0][tid] = E[tid];
  float ahead = (tid < V && T > 1) ? E[V + tid] : 0.0f;          // row t + 1, loaded a frame early
  __syncthreads();
  float a[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) a[k] = (s0 + k < 2 && s0 + k < S) ? erow[0][lab[k]] : -INFINITY;

  for (int t = 1; t < T; ++t) {
    const int pp = t & 1;
    edge[pp][2 * tid] = a[PER - 2];
    edge[pp][2 * tid + 1] = a[PER - 1];
    if (tid < V) {
      erow[pp][tid] = ahead;
      if (t + 1 < T) ahead = E[(int64_t)(t + 1) * V + tid];
    }
    __syncthreads();
    const float left2 = tid ? edge[pp][2 * tid - 2] : -INFINITY, left1 = tid ? edge[pp][2 * tid - 1] : -INFINITY;
    const float* e = erow[pp];
    unsigned word = 0;
#pragma unroll
    for (int k = PER - 1; k >= 0; --k) {               // descending: a[k - 1], a[k - 2] are still the previous frame's
      const float one = k >= 1 ? a[k - 1] : left1, two = k >= 2 ? a[k - 2] : (k == 1 ? left1 : left2);
      float best;
      const unsigned code = pick(a[k], one, two, (skip >> k) & 1u, best);
      const bool in = s0 + k < S;
      a[k] = in ? e[lab[k]] + best : -INFINITY;
      word |= (in ? code : 0u) << (2 * k);
    }
    if (tid < W) bp[(int64_t)t * W + tid] = word;
  }

#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (s0 + k == S - 1) fin[1] = a[k];
    if (s0 + k == S - 2) fin[0] = a[k];
  }
  __syncthreads();                                     // (also: every thread's back-pointer words are visible to thread 0)
  if (tid == 0) {
    int s = S - 1;
    float end = fin[1];
    if (S > 1 && fin[0] > end) end = fin[0], s = S - 2;
    const bool ok = end > -INFINITY;
    score[item] = end;
    status[item] = ok ? 0 : 1;
    feasible = ok;
    if (ok) {
      for (int t = T - 1; t >= 0; --t) {
        path[f0 + t] = s;
        if (t) s -= (int)((bp[(int64_t)t * W + s / PER] >> (2 * (s % PER))) & 3u);
      }
    }
  }
  __syncthreads();
  if (!feasible) {
    for (int t = tid; t < T; t += blockDim.x) path[f0 + t] = 0;
    for (int j = tid; j < L; j += blockDim.x) tok_first[k0 + j] = tok_last[k0 + j] = -1;
    return;
  }
  // a feasible path is monotone and visits every token state in one run of frames
  for (int t = tid; t < T; t += blockDim.x) {
    const int s = path[f0 + t];
    if (s & 1) {
      if (t == 0 || path[f0 + t - 1] != s) tok_first[k0 + (s >> 1)] = t;
      if (t == T - 1 || path[f0 + t + 1] != s) tok_last[k0 + (s >> 1)] = t;
    }
  }
}

constexpr int WF_THREADS = 256;

__global__ void __launch_bounds__(WF_THREADS) word_frames_kernel(const float* __restrict__ hidden, const int* __restrict__ tok_row_off,
                                                                const int* __restrict__ start_frame, const int* __restrict__ end_frame,
                                                                const int* __restrict__ word_off, const int64_t* __restrict__ frame_off,
                                                                int n_windows, int D, float* __restrict__ out) {
  const int64_t row = blockIdx.x;
  int lo = 0, hi = n_windows;                          // the last window with frame_off[b] <= row (empty windows own no row)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (frame_off[mid] <= row) lo = mid; else hi = mid;
  }
  const int f = (int)(row - frame_off[lo]);
  int w = word_off[lo + 1] - 1;
  while (w >= word_off[lo] && !(start_frame[w] <= f && f < end_frame[w])) --w;      // later words overwrite earlier ones
  float* o = out + row * D;
  if (w < word_off[lo]) {
    for (int c = threadIdx.x; c < D; c += WF_THREADS) o[c] = 0.0f;
    return;
  }
  const int r0 = tok_row_off[w], r1 = tok_row_off[w + 1];
  const float n = (float)(r1 - r0);
  for (int c = threadIdx.x; c < D; c += WF_THREADS) {
    float s = 0.0f;
    for (int r = r0; r < r1; ++r) s += hidden[(int64_t)r * D + c];
    o[c] = s / n;
  }
}

// the offsets of a ragged batch: start at 0, do not decrease
bool ctc_offsets_ok(const int64_t* off, int n) {
  if (off[0] != 0) return false;
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}

}  // namespace

extern "C" int rg_ctc_log_softmax(rg_handle* h, const float* logits, int64_t rows, int V, float* logp, int* best, void* stream) {
  RG_REQUIRE(h, logits && logp && best, "null pointer");
  RG_REQUIRE(h, V >= 2 && V <= RG_CTC_MAX_VOCAB, "need 2 to 64 classes");
  RG_REQUIRE(h, rows >= 1 && rows < ((int64_t)1 << 31), "need 1 to 2^31 - 1 rows");
  const int64_t blocks = (rows + LSM_THREADS / WAVE - 1) / (LSM_THREADS / WAVE);
  hipLaunchKernelGGL(ctc_log_softmax_kernel, dim3((unsigned)blocks), dim3(LSM_THREADS), 0, rg_stream(stream), logits, rows, V, logp, best);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_ctc_align(rg_handle* h, const float* logp, int V, const int64_t* frame_off, const int64_t* frame_off_host,
                            const int* tokens, const int64_t* tok_off, const int64_t* tok_off_host, int n_items, int blank,
                            unsigned* backptr, const int64_t* backptr_off, const int64_t* backptr_off_host, int* path, int* tok_first,
                            int* tok_last, float* score, int* status, void* stream) {
  RG_REQUIRE(h, logp && frame_off && frame_off_host && tokens && tok_off && tok_off_host && backptr && backptr_off && backptr_off_host &&
                    path && tok_first && tok_last && score && status, "null pointer");
  RG_REQUIRE(h, V >= 2 && V <= RG_CTC_MAX_VOCAB, "need 2 to 64 classes");
  RG_REQUIRE(h, blank >= 0 && blank < V, "blank must be a class");
  RG_REQUIRE(h, n_items >= 1, "need at least one item");
  RG_REQUIRE(h, ctc_offsets_ok(frame_off_host, n_items) && ctc_offsets_ok(tok_off_host, n_items) && ctc_offsets_ok(backptr_off_host, n_items),
             "offsets must start at 0 and not decrease");
  RG_REQUIRE(h, frame_off_host[n_items] < ((int64_t)1 << 31) / V, "too many emission rows in one call");
  int max_states = 0;
  for (int i = 0; i < n_items; ++i) {
    const int64_t T = frame_off_host[i + 1] - frame_off_host[i], L = tok_off_host[i + 1] - tok_off_host[i];
    RG_REQUIRE(h, T >= 1 && L >= 1, "an item needs at least one emission row and one token");
    RG_REQUIRE(h, 2 * L + 1 <= RG_CTC_MAX_STATES, "an item has more than RG_CTC_MAX_STATES states (2 tokens + 1)");
    const int64_t W = (2 * L + 1 + PER - 1) / PER;
    RG_REQUIRE(h, backptr_off_host[i + 1] - backptr_off_host[i] >= T * W, "an item's back-pointer scratch is smaller than frames x ceil(states / 16) words");
    if (2 * L + 1 > max_states) max_states = (int)(2 * L + 1);
  }
  const int threads = ((max_states + PER - 1) / PER + WAVE - 1) / WAVE * WAVE;      // whole waves; <= MAX_THREADS by the cap above
  hipLaunchKernelGGL(ctc_align_kernel, dim3(n_items), dim3(threads), 0, rg_stream(stream), logp, V, frame_off, tokens, tok_off, blank, backptr,
                     backptr_off, path, tok_first, tok_last, score, status);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_word_frames(rg_handle* h, const float* hidden, const int* tok_row_off, const int* start_frame, const int* end_frame,
                              const int* word_off, const int* word_off_host, const int64_t* frame_off, const int64_t* frame_off_host,
                              int n_windows, int D, float* out, void* stream) {
  RG_REQUIRE(h, hidden && tok_row_off && start_frame && end_frame && word_off && word_off_host && frame_off && frame_off_host && out, "null pointer");
  RG_REQUIRE(h, n_windows >= 1 && D >= 1, "need at least one window and one column");
  RG_REQUIRE(h, ctc_offsets_ok(frame_off_host, n_windows), "offsets must start at 0 and not decrease");
  RG_REQUIRE(h, word_off_host[0] == 0, "offsets must start at 0 and not decrease");
  for (int b = 0; b < n_windows; ++b) RG_REQUIRE(h, word_off_host[b + 1] >= word_off_host[b], "offsets must start at 0 and not decrease");
  const int64_t rows = frame_off_host[n_windows];
  RG_REQUIRE(h, rows < ((int64_t)1 << 31), "too many frames in one call");
  if (rows == 0) return RG_OK;
  hipLaunchKernelGGL(word_frames_kernel, dim3((unsigned)rows), dim3(WF_THREADS), 0, rg_stream(stream), hidden, tok_row_off, start_frame, end_frame,
                     word_off, frame_off, n_windows, D, out);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
