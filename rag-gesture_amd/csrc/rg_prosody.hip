// Word prosodic prominence from 16 kHz audio and word timings (rag-gesture_amd/prosody.py; the arithmetic is stated in
// include/rg_gesture.h and DESIGN section 15), four launches for a ragged batch of recordings:
//   rg_prosody_frames : one workgroup per 10 ms frame -- the 1024-sample window staged in LDS, log energy by a fixed-order block sum,
//                       the normalised cross-correlation of 229 lags (thread = lag: x[i] is an LDS broadcast, x[i + L] consecutive
//                       across the lanes), the biased argmax by a wave butterfly and a fixed order over the waves, a parabola
//   rg_prosody_signal : one workgroup per recording -- voicing, the gaps of f0 and of the word-duration track filled linearly between
//                       knots (a thread owns a contiguous share of the frames and learns the knots around it from its neighbours'
//                       first / last knot in LDS), the three tracks z-normalised with fp64 moments, their weighted sum
//   rg_prosody_cwt    : one workgroup per 256 frames of one recording -- the sum with its halo and the ten scales' taps in LDS, a
//                       serial ascending sum per scale and frame
//   rg_prosody_words  : one workgroup per recording -- lines of maximum amplitude climbed from every local maximum (minimum) of the
//                       finest scale, then one wave per word: the strongest line that starts inside it / behind its middle
#include <math.h>

#include "rg_common.h"
#include "rg_reduce.h"

namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int NWAVES = THREADS / WAVE;
constexpr int HOP = RG_PROSODY_HOP, WIN = RG_PROSODY_WIN, LAG_MIN = RG_PROSODY_LAG_MIN, LAG_MAX = RG_PROSODY_LAG_MAX;
constexpr int NPROD = WIN - LAG_MAX - 1;                // 757 products per lag
constexpr int LAG_LO = LAG_MIN - 1, NLAGS = LAG_MAX + 1 - LAG_LO + 1;      // 39 .. 267: 229 lags
constexpr int SCALES = RG_PROSODY_SCALES, TILE = RG_PROSODY_TILE, HALO = RG_PROSODY_HALO, TAPS = RG_PROSODY_TAPS;
static_assert(NLAGS <= THREADS && NPROD + LAG_MAX + 1 <= WIN, "a thread per lag; every product inside the window");
static_assert(WIN == 4 * THREADS && TILE == THREADS && SCALES == 10, "launch shapes");

__constant__ const int RADIUS[SCALES] = {10, 15, 20, 29, 40, 57, 80, 114, 160, 227};     // ceil(5 s_j)
__constant__ const int REACH[SCALES] = {2, 3, 4, 6, 8, 12, 16, 23, 32, 46};              // ceil(s_j)

// the last item with off[item] <= at (items without rows own none)
__device__ __forceinline__ int owner(const int64_t* __restrict__ off, int n, int64_t at) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= at) lo = mid; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------------------------ frames
__global__ void __launch_bounds__(THREADS) prosody_frames_kernel(const float* __restrict__ samples, const int64_t* __restrict__ sample_off,
                                                                 const int64_t* __restrict__ frame_off, int n_rec, float* __restrict__ energy,
                                                                 float* __restrict__ nccf, int* __restrict__ lag, float* __restrict__ logf0) {
  __shared__ float x[WIN];
  __shared__ float r[THREADS];
  __shared__ float red[NWAVES];
  __shared__ float best_s[NWAVES];
  __shared__ int best_l[NWAVES];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int rec = owner(frame_off, n_rec, row);
  const int64_t t = row - frame_off[rec], s0 = sample_off[rec], n = sample_off[rec + 1] - s0;
  const int64_t first = t * HOP - WIN / 2;
  float e = 0.0f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = tid + q * THREADS;
    const int64_t s = first + k;
    const float v = (s >= 0 && s < n) ? samples[s0 + s] : 0.0f;
    x[k] = v;
    e = fmaf(v, v, e);
  }
  e = block_sum(e, red);                               // (its barriers also publish x)
  if (tid == 0) energy[row] = logf(e / (float)WIN + 1e-10f);

  const int L = LAG_LO + tid;
  float rl = 0.0f;
  if (tid < NLAGS) {
    float xx = 0.0f, xy = 0.0f, yy = 0.0f;
    for (int i = 0; i < NPROD; ++i) {
      const float a = x[i], b = x[i + L];
      xx = fmaf(a, a, xx);
      xy = fmaf(a, b, xy);
      yy = fmaf(b, b, yy);
    }
    rl = xy / sqrtf(xx * yy + 1e-20f);
  }
  r[tid] = rl;
  const bool cand = tid < NLAGS && L >= LAG_MIN && L <= LAG_MAX;
  float s = cand ? rl - 0.05f * (float)L / (float)LAG_MAX : -INFINITY;
  int bl = cand ? L : 0x7fffffff;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float os = __shfl_xor(s, m);
    const int ol = __shfl_xor(bl, m);
    if (os > s || (os == s && ol < bl)) s = os, bl = ol;
  }
  if (lane == 0) best_s[wave] = s, best_l[wave] = bl;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NWAVES; ++w)
      if (best_s[w] > s || (best_s[w] == s && best_l[w] < bl)) s = best_s[w], bl = best_l[w];
    // (a NaN sample makes every comparison false: the lag stays a candidate of wave 0 or the sentinel, clamped here)
    bl = bl < LAG_MIN ? LAG_MIN : (bl > LAG_MAX ? LAG_MAX : bl);
    const float rm = r[bl - LAG_LO - 1], r0 = r[bl - LAG_LO], rp = r[bl - LAG_LO + 1];
    const float d = rm - 2.0f * r0 + rp;
    float delta = d == 0.0f ? 0.0f : 0.5f * (rm - rp) / d;
    delta = fminf(fmaxf(delta, -0.5f), 0.5f);
    nccf[row] = r0;
    lag[row] = bl;
    logf0[row] = logf(16000.0f / ((float)bl + delta));
  }
}

// ------------------------------------------------------------------------------------------------------------------ signal
// v holds a value at every knot (knot[t] != 0) of the T frames; every other frame is filled: linear between the nearest knots,
// flat outside, 0 without knots.  Thread tid owns frames [lo, hi).  first_k / last_k: LDS, one entry per thread.  -> any knot at all
__device__ bool fill_between_knots(float* v, const int* knot, int T, int lo, int hi, int* first_k, int* last_k) {
  const int tid = threadIdx.x;
  int f = -1, l = -1;
  for (int t = lo; t < hi; ++t)
    if (knot[t]) {
      if (f < 0) f = t;
      l = t;
    }
  __syncthreads();                                     // (the arrays may still be read from an earlier call)
  first_k[tid] = f;
  last_k[tid] = l;
  __syncthreads();
  int prev = -1, next_out = -1;
  for (int j = tid - 1; j >= 0 && prev < 0; --j) prev = last_k[j];
  for (int j = tid + 1; j < THREADS && next_out < 0; ++j) next_out = first_k[j];
  int any = f >= 0 || prev >= 0 || next_out >= 0;
  any = __syncthreads_or(any);
  int t = lo;
  while (t < hi) {
    if (knot[t]) {
      prev = t++;
      continue;
    }
    int e = t;                                         // the run of frames without a knot [t, e) inside this share
    while (e < hi && !knot[e]) ++e;
    const int next = e < hi ? e : next_out;
    const float va = prev >= 0 ? v[prev] : 0.0f, vb = next >= 0 ? v[next] : 0.0f;
    for (int u = t; u < e; ++u) {
      float out = 0.0f;
      if (prev >= 0 && next >= 0) out = va + (vb - va) * ((float)(u - prev) / (float)(next - prev));
      else if (prev >= 0) out = va;
      else if (next >= 0) out = vb;
      v[u] = out;
    }
    t = e;
  }
  __syncthreads();
  return any != 0;
}

// z-normalise v[0 .. T) into z: fp64 mean and population variance in a fixed order
__device__ void znorm(const float* v, float* z, int T, int lo, int hi, double* red) {
  double s = 0.0;
  for (int t = lo; t < hi; ++t) s += (double)v[t];
  const double mean = block_sum(s, red) / (double)T;
  double q = 0.0;
  for (int t = lo; t < hi; ++t) {
    const double d = (double)v[t] - mean;
    q += d * d;
  }
  const double sd = sqrt(block_sum(q, red) / (double)T);
  const double den = sd > 1e-6 ? sd : 1e-6;
  for (int t = lo; t < hi; ++t) z[t] = (float)(((double)v[t] - mean) / den);
}

__global__ void __launch_bounds__(THREADS) prosody_signal_kernel(
    const float* __restrict__ energy, const float* __restrict__ nccf, const float* __restrict__ logf0, const int64_t* __restrict__ frame_off,
    const int64_t* __restrict__ word_off, const int* __restrict__ start_frame, const int* __restrict__ end_frame,
    const float* __restrict__ word_start, const float* __restrict__ word_end, float w_f0, float w_en, float w_dur, int* __restrict__ voiced,
    float* __restrict__ f0, float* __restrict__ f0z, float* __restrict__ ez, float* __restrict__ dz, float* __restrict__ c,
    int* __restrict__ knot, int* __restrict__ status) {
  __shared__ int first_k[THREADS], last_k[THREADS];
  __shared__ double red[NWAVES];
  __shared__ float wmax[NWAVES];
  const int rec = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int64_t fo = frame_off[rec];
  const int T = (int)(frame_off[rec + 1] - fo);
  if (T <= 0) {
    if (tid == 0) status[rec] = 1;
    return;
  }
  const int share = (T + THREADS - 1) / THREADS;
  const int lo = min(tid * share, T), hi = min(lo + share, T);
  const float* en = energy + fo;
  const float* nc = nccf + fo;
  const float* lf = logf0 + fo;
  int* vo = voiced + fo;
  int* kn = knot + fo;
  float *F0 = f0 + fo, *F0Z = f0z + fo, *EZ = ez + fo, *DZ = dz + fo, *C = c + fo;

  float mx = -INFINITY;
  for (int t = lo; t < hi; ++t) mx = fmaxf(mx, en[t]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  const float emax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  const float floor_e = emax - 11.5f;

  // voicing; f0 holds logf0 at the voiced frames; EZ holds the clamped energy until it is normalised in place
  for (int t = lo; t < hi; ++t) {
    const float e = en[t];
    const int v = (nc[t] >= 0.5f && e >= floor_e) ? 1 : 0;
    vo[t] = v;
    F0[t] = v ? lf[t] : 0.0f;
    EZ[t] = fmaxf(e, floor_e);
    kn[t] = 0;
    DZ[t] = 0.0f;
  }
  __syncthreads();
  const bool any_voiced = fill_between_knots(F0, vo, T, lo, hi, first_k, last_k);
  if (tid == 0) status[rec] = any_voiced ? 0 : 1;

  // the words' duration knots (distinct frames: the words' frame ranges are disjoint)
  const int64_t w0 = word_off[rec], w1 = word_off[rec + 1];
  for (int64_t w = w0 + tid; w < w1; w += THREADS) {
    const int a = max(start_frame[w], 0), b = min(end_frame[w], T);
    if (a < b) {
      const int mid = (a + b - 1) / 2;
      DZ[mid] = logf(fmaxf(word_end[w] - word_start[w], 0.01f));
      kn[mid] = 1;
    }
  }
  __syncthreads();
  fill_between_knots(DZ, kn, T, lo, hi, first_k, last_k);

  znorm(F0, F0Z, T, lo, hi, red);
  znorm(EZ, EZ, T, lo, hi, red);
  znorm(DZ, DZ, T, lo, hi, red);
  for (int t = lo; t < hi; ++t) C[t] = fmaf(w_dur, DZ[t], fmaf(w_en, EZ[t], w_f0 * F0Z[t]));
}

// ------------------------------------------------------------------------------------------------------------------ cwt
__global__ void __launch_bounds__(THREADS) prosody_cwt_kernel(const float* __restrict__ c, const int64_t* __restrict__ frame_off,
                                                              const int64_t* __restrict__ tile_off, int n_rec, const float* __restrict__ taps,
                                                              int64_t total_frames, float* __restrict__ W) {
  __shared__ float cs[TILE + 2 * HALO];
  __shared__ float psi[TAPS];
  const int tid = threadIdx.x;
  const int rec = owner(tile_off, n_rec, (int64_t)blockIdx.x);
  const int64_t fo = frame_off[rec];
  const int T = (int)(frame_off[rec + 1] - fo);
  const int t0 = (int)((int64_t)blockIdx.x - tile_off[rec]) * TILE;
  for (int k = tid; k < TILE + 2 * HALO; k += THREADS) {
    const int t = t0 - HALO + k;
    cs[k] = (t >= 0 && t < T) ? c[fo + t] : 0.0f;
  }
  for (int k = tid; k < TAPS; k += THREADS) psi[k] = taps[k];
  __syncthreads();
  const int t = t0 + tid;
  if (t >= T) return;
  int base = 0;
#pragma unroll 1
  for (int j = 0; j < SCALES; ++j) {
    const int R = RADIUS[j];
    const float* x = cs + HALO + tid - R;
    const float* p = psi + base;
    float s = 0.0f;
    for (int k = 0; k <= 2 * R; ++k) s = fmaf(x[k], p[k], s);
    W[(int64_t)j * total_frames + fo + t] = s;
    base += 2 * R + 1;
  }
}

// ------------------------------------------------------------------------------------------------------------------ words
// the local-maximum test of sign * w at q
__device__ __forceinline__ bool line_point(const float* __restrict__ w, int T, int q, float sign) {
  const float v = sign * w[q];
  const float l = q > 0 ? sign * w[q - 1] : -INFINITY, r = q + 1 < T ? sign * w[q + 1] : -INFINITY;
  return v > 0.0f && v > l && v >= r;
}

// the strength of the line of sign * W that starts at p, 0 when none does
__device__ float line_strength(const float* __restrict__ W, int64_t stride, int T, int p, float sign) {
  if (!line_point(W, T, p, sign)) return 0.0f;
  float strength = sign * W[p];
  int pos = p;
  for (int j = 1; j < SCALES; ++j) {
    const float* w = W + (int64_t)j * stride;
    const int reach = REACH[j];
    int found = -1;
    for (int d = 0; d <= reach && found < 0; ++d) {
      const int a = pos - d, b = pos + d;
      if (a >= 0 && a < T && line_point(w, T, a, sign)) found = a;
      else if (d > 0 && b < T && line_point(w, T, b, sign)) found = b;
    }
    if (found < 0) break;
    strength += sign * w[found];
    pos = found;
  }
  return strength;
}

// the largest v[t] > 0 over [a, b) and the lowest frame that holds it, by the lanes of one wave; (0, -1) without one
__device__ __forceinline__ void wave_best(const float* v, int a, int b, int lane, float& best, int& at) {
  best = 0.0f;
  at = -1;
  for (int t = a + lane; t < b; t += WAVE) {
    const float x = v[t];
    if (x > best) best = x, at = t;                    // ascending t: the lowest frame among equals stays
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ob = __shfl_xor(best, m);
    const int oa = __shfl_xor(at, m);
    if (ob > best || (ob == best && oa >= 0 && (at < 0 || oa < at))) best = ob, at = oa;
  }
}

__global__ void __launch_bounds__(THREADS) prosody_words_kernel(const float* __restrict__ W, const int64_t* __restrict__ frame_off,
                                                                const int64_t* __restrict__ word_off, const int* __restrict__ start_frame,
                                                                const int* __restrict__ end_frame, int64_t total_frames,
                                                                float* __restrict__ peak_strength, float* __restrict__ valley_strength,
                                                                float* __restrict__ prominence, float* __restrict__ boundary,
                                                                int* __restrict__ prom_frame, int* __restrict__ bnd_frame) {
  const int rec = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int64_t fo = frame_off[rec];
  const int T = (int)(frame_off[rec + 1] - fo);
  const float* Wr = W + fo;
  float* pk = peak_strength + fo;
  float* vl = valley_strength + fo;
  for (int t = tid; t < T; t += THREADS) {
    pk[t] = line_strength(Wr, total_frames, T, t, 1.0f);
    vl[t] = line_strength(Wr, total_frames, T, t, -1.0f);
  }
  __syncthreads();                                     // (the strengths of every frame are visible to the workgroup)
  const int64_t w0 = word_off[rec], w1 = word_off[rec + 1];
  for (int64_t w = w0 + wave; w < w1; w += NWAVES) {
    const int a = max(start_frame[w], 0), b = min(end_frame[w], T);
    float best = 0.0f, bbest = 0.0f;
    int at = -1, bat = -1;
    if (a < b) {
      wave_best(pk, a, b, lane, best, at);
      int stop = T;                                    // the middle of the next word that has frames
      for (int64_t v = w + 1; v < w1; ++v) {
        const int a2 = max(start_frame[v], 0), b2 = min(end_frame[v], T);
        if (a2 < b2) {
          stop = (a2 + b2 - 1) / 2;
          break;
        }
      }
      wave_best(vl, (a + b - 1) / 2, stop, lane, bbest, bat);
    }
    if (lane == 0) {
      prominence[w] = best;
      prom_frame[w] = at;
      boundary[w] = bbest;
      bnd_frame[w] = bat;
    }
  }
}

// the offsets of a ragged batch: start at 0, do not decrease
bool offsets_ok(const int64_t* off, int n) {
  if (off[0] != 0) return false;
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}

// every recording's words lie inside its frames, in order, without overlap
bool words_ok(const int64_t* frame_off, const int64_t* word_off, const int* start, const int* end, int n) {
  for (int i = 0; i < n; ++i) {
    const int64_t T = frame_off[i + 1] - frame_off[i];
    int prev = 0;
    for (int64_t w = word_off[i]; w < word_off[i + 1]; ++w) {
      if (start[w] < prev || end[w] < start[w] || end[w] > T) return false;
      prev = end[w];
    }
  }
  return true;
}

}  // namespace

extern "C" int rg_prosody_frames(rg_handle* h, const float* samples, const int64_t* sample_off, const int64_t* sample_off_host,
                                 const int64_t* frame_off, const int64_t* frame_off_host, int n_rec, float* energy, float* nccf, int* lag,
                                 float* logf0, void* stream) {
  RG_REQUIRE(h, samples && sample_off && sample_off_host && frame_off && frame_off_host && energy && nccf && lag && logf0, "null pointer");
  RG_REQUIRE(h, n_rec >= 1, "need at least one recording");
  RG_REQUIRE(h, offsets_ok(sample_off_host, n_rec) && offsets_ok(frame_off_host, n_rec), "offsets must start at 0 and not decrease");
  for (int i = 0; i < n_rec; ++i)
    RG_REQUIRE(h, frame_off_host[i + 1] - frame_off_host[i] == 1 + (sample_off_host[i + 1] - sample_off_host[i]) / HOP,
               "a recording of n samples has 1 + n / 160 frames");
  RG_REQUIRE(h, frame_off_host[n_rec] < ((int64_t)1 << 31), "too many frames in one call");
  hipLaunchKernelGGL(prosody_frames_kernel, dim3((unsigned)frame_off_host[n_rec]), dim3(THREADS), 0, rg_stream(stream), samples, sample_off,
                     frame_off, n_rec, energy, nccf, lag, logf0);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_prosody_signal(rg_handle* h, const float* energy, const float* nccf, const float* logf0, const int64_t* frame_off,
                                 const int64_t* frame_off_host, const int64_t* word_off, const int64_t* word_off_host, const int* start_frame,
                                 const int* end_frame, const int* start_frame_host, const int* end_frame_host, const float* word_start,
                                 const float* word_end, int n_rec, float w_f0, float w_en, float w_dur, int* voiced, float* f0, float* f0z,
                                 float* ez, float* dz, float* c, int* knot, int* status, void* stream) {
  RG_REQUIRE(h, energy && nccf && logf0 && frame_off && frame_off_host && word_off && word_off_host && start_frame && end_frame &&
                    start_frame_host && end_frame_host && word_start && word_end && voiced && f0 && f0z && ez && dz && c && knot && status,
             "null pointer");
  RG_REQUIRE(h, n_rec >= 1, "need at least one recording");
  RG_REQUIRE(h, offsets_ok(frame_off_host, n_rec) && offsets_ok(word_off_host, n_rec), "offsets must start at 0 and not decrease");
  RG_REQUIRE(h, frame_off_host[n_rec] < ((int64_t)1 << 31), "too many frames in one call");
  RG_REQUIRE(h, words_ok(frame_off_host, word_off_host, start_frame_host, end_frame_host, n_rec),
             "a recording's word frames must lie inside it, in order and without overlap");
  hipLaunchKernelGGL(prosody_signal_kernel, dim3(n_rec), dim3(THREADS), 0, rg_stream(stream), energy, nccf, logf0, frame_off, word_off,
                     start_frame, end_frame, word_start, word_end, w_f0, w_en, w_dur, voiced, f0, f0z, ez, dz, c, knot, status);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_prosody_cwt(rg_handle* h, const float* c, const int64_t* frame_off, const int64_t* frame_off_host, const int64_t* tile_off,
                              const int64_t* tile_off_host, int n_rec, const float* taps, float* W, void* stream) {
  RG_REQUIRE(h, c && frame_off && frame_off_host && tile_off && tile_off_host && taps && W, "null pointer");
  RG_REQUIRE(h, n_rec >= 1, "need at least one recording");
  RG_REQUIRE(h, offsets_ok(frame_off_host, n_rec) && offsets_ok(tile_off_host, n_rec), "offsets must start at 0 and not decrease");
  for (int i = 0; i < n_rec; ++i)
    RG_REQUIRE(h, tile_off_host[i + 1] - tile_off_host[i] == (frame_off_host[i + 1] - frame_off_host[i] + TILE - 1) / TILE,
               "a recording of T frames has ceil(T / 256) tiles");
  const int64_t total = frame_off_host[n_rec], tiles = tile_off_host[n_rec];
  RG_REQUIRE(h, total < ((int64_t)1 << 31), "too many frames in one call");
  if (tiles == 0) return RG_OK;
  hipLaunchKernelGGL(prosody_cwt_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, rg_stream(stream), c, frame_off, tile_off, n_rec, taps, total, W);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_prosody_words(rg_handle* h, const float* W, const int64_t* frame_off, const int64_t* frame_off_host, const int64_t* word_off,
                                const int64_t* word_off_host, const int* start_frame, const int* end_frame, const int* start_frame_host,
                                const int* end_frame_host, int n_rec, float* peak_strength, float* valley_strength, float* prominence,
                                float* boundary, int* prom_frame, int* bnd_frame, void* stream) {
  RG_REQUIRE(h, W && frame_off && frame_off_host && word_off && word_off_host && start_frame && end_frame && start_frame_host &&
                    end_frame_host && peak_strength && valley_strength && prominence && boundary && prom_frame && bnd_frame, "null pointer");
  RG_REQUIRE(h, n_rec >= 1, "need at least one recording");
  RG_REQUIRE(h, offsets_ok(frame_off_host, n_rec) && offsets_ok(word_off_host, n_rec), "offsets must start at 0 and not decrease");
  RG_REQUIRE(h, frame_off_host[n_rec] < ((int64_t)1 << 31), "too many frames in one call");
  RG_REQUIRE(h, words_ok(frame_off_host, word_off_host, start_frame_host, end_frame_host, n_rec),
             "a recording's word frames must lie inside it, in order and without overlap");
  hipLaunchKernelGGL(prosody_words_kernel, dim3(n_rec), dim3(THREADS), 0, rg_stream(stream), W, frame_off, word_off, start_frame, end_frame,
                     frame_off_host[n_rec], peak_strength, valley_strength, prominence, boundary, prom_frame, bnd_frame);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
