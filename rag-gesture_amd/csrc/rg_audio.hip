// Audio onset detection for beat alignment (mogen/models/utils/metric.py:64-76 alignment.load_audio): the defaults of
// librosa.onset.onset_detect(y, sr=16000, hop_length=512) restated, over a ragged batch of clips (concatenated samples and
// int64 offsets), in two launches:
//   rg_onset_mel_db : one workgroup per frame -- 2048 windowed samples (zero beyond the clip), a 2048-point complex fp32 FFT in
//                     LDS, |X|^2 over 1025 bins, 128 mel filter sums, 10 log10(max(1e-10, .)); the clip's maximum by one atomic max
//                     per workgroup on the order-preserving integer image of the float
//   rg_onset_pick   : one workgroup per clip -- the -80 dB clamp against the clip's own maximum, the spectral flux, its 3-frame
//                     shift, min / max normalisation, the 7-frame mean, the threshold and an ordered compaction
// and what comes in front of them for recorded audio of any rate, channel count and sample format:
//   rg_resample_poly: one workgroup per 1024 consecutive outputs of a clip -- the input span of the tile decoded, downmixed and
//                     staged in LDS (zero outside the clip, by index), then per output one serial fp32 sum over the taps of its
//                     phase's row of the polyphase table
#include <float.h>

#include "rg_common.h"

namespace {

constexpr int N_FFT = RG_ONSET_N_FFT;
constexpr int HOP = RG_ONSET_HOP;
constexpr int N_BINS = N_FFT / 2 + 1;
constexpr int N_MELS = RG_ONSET_MELS;
constexpr int MEL_STRIDE = RG_ONSET_MEL_STRIDE;
constexpr int THREADS = 256;
constexpr int LDS_N = N_FFT + N_FFT / 32;      // one pad dword per 32: see lds_at

// LDS index of FFT element a.  Real and imaginary parts live in two float arrays (4-byte accesses, 32 banks).  A radix-4 pass
// whose outputs lie p apart writes lane i's element to 4 (i - i % p) + i % p + r p: for p = 1 that is a stride of 4 dwords, a
// 4-way bank conflict over a 32-lane half.  One pad dword per 32 elements moves every eighth lane one bank on: the p = 1 pass
// becomes conflict-free, the p = 4 pass 2-way, and the reads (consecutive lanes, consecutive elements) stay conflict-free.
__device__ __forceinline__ int lds_at(int a) { return a + (a >> 5); }

__device__ __forceinline__ void cmul(float& re, float& im, const float2 w) {
  const float r = re * w.x - im * w.y;
  im = re * w.y + im * w.x;
  re = r;
}

// One Stockham pass of radix R over the 2048 elements in re / im, in place: every thread first reads the inputs of its
// butterflies (element i + r N/R of butterfly i), the workgroup meets, then it writes the outputs (element j + r p, where
// k = i mod p, j = R (i - k) + k and p is the product of the radices before this pass).  Input r is turned by
// exp(-2 pi i r k / (p R)) = tw[r k N / (p R)]: the table is exp(-2 pi i m / N), computed in float64 and rounded once.
template <int R>
__device__ __forceinline__ void fft_pass(float* re, float* im, const float2* __restrict__ tw, int p, int tid) {
  constexpr int T = N_FFT / R, PER = T / THREADS;
  float ur[PER][R], ui[PER][R];
#pragma unroll
  for (int q = 0; q < PER; ++q)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int a = lds_at(tid + q * THREADS + r * T);
      ur[q][r] = re[a];
      ui[q][r] = im[a];
    }
  __syncthreads();
  const int step = N_FFT / (p * R);
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int i = tid + q * THREADS, k = i & (p - 1), j = (i - k) * R + k;
#pragma unroll
    for (int r = 1; r < R; ++r) cmul(ur[q][r], ui[q][r], tw[r * k * step]);
    if (R == 4) {
      const float ar = ur[q][0] + ur[q][2], ai = ui[q][0] + ui[q][2], br = ur[q][0] - ur[q][2], bi = ui[q][0] - ui[q][2];
      const float cr = ur[q][1] + ur[q][3], ci = ui[q][1] + ui[q][3], dr = ur[q][1] - ur[q][3], di = ui[q][1] - ui[q][3];
      ur[q][0] = ar + cr, ui[q][0] = ai + ci;
      ur[q][1] = br + di, ui[q][1] = bi - dr;                 // b - i d
      ur[q][2] = ar - cr, ui[q][2] = ai - ci;
      ur[q][3] = br - di, ui[q][3] = bi + dr;                 // b + i d
    } else {
      const float ar = ur[q][0] + ur[q][1], ai = ui[q][0] + ui[q][1];
      ur[q][1] = ur[q][0] - ur[q][1], ui[q][1] = ui[q][0] - ui[q][1];
      ur[q][0] = ar, ui[q][0] = ai;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int a = lds_at(j + r * p);
      re[a] = ur[q][r];
      im[a] = ui[q][r];
    }
  }
  __syncthreads();
}

// order-preserving image of a float in an unsigned integer: a < b  <=>  image(a) < image(b) (no NaN reaches it)
__device__ __forceinline__ unsigned ordered_image(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// the clip of frame f: off[c] <= f < off[c + 1] (clips without frames do not exist: every clip has at least one)
__device__ __forceinline__ int clip_of(const int64_t* __restrict__ off, int n_clips, int64_t f) {
  int lo = 0, hi = n_clips;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(THREADS) onset_mel_db_kernel(rg_onset_mel_args a) {
  __shared__ float re[LDS_N], im[LDS_N];            // 2 x 8.25 KB
  __shared__ float power[N_BINS + 3];
  __shared__ float wave_max[THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x;
  const int c = clip_of(a.frame_off, a.n_clips, f);
  const int64_t s0 = a.sample_off[c], len = a.sample_off[c + 1] - s0;
  const int64_t first = (f - a.frame_off[c]) * HOP - N_FFT / 2;      // sample of window position 0 (centred frames)
  const float* y = a.samples + s0;
#pragma unroll
  for (int q = 0; q < N_FFT / THREADS; ++q) {
    const int k = tid + q * THREADS;
    const int64_t s = first + k;
    const float v = (s >= 0 && s < len) ? y[s] * a.window[k] : 0.0f;
    re[lds_at(k)] = v;
    im[lds_at(k)] = 0.0f;
  }
  __syncthreads();
  const float2* tw = reinterpret_cast<const float2*>(a.twiddle);
  fft_pass<4>(re, im, tw, 1, tid);
  fft_pass<4>(re, im, tw, 4, tid);
  fft_pass<4>(re, im, tw, 16, tid);
  fft_pass<4>(re, im, tw, 64, tid);
  fft_pass<4>(re, im, tw, 256, tid);
  fft_pass<2>(re, im, tw, 1024, tid);
  for (int b = tid; b < N_BINS; b += THREADS) {
    const float xr = re[lds_at(b)], xi = im[lds_at(b)];
    power[b] = xr * xr + xi * xi;
  }
  __syncthreads();
  // 16 lanes per filter: the filter's contiguous bins in strides of 16, then a butterfly over the 16 lanes
  const int sub = tid & 15, group = tid >> 4;
  float best = -FLT_MAX;
  for (int m = group; m < N_MELS; m += THREADS / 16) {
    const int start = a.mel_start[m], n = min(a.mel_len[m], MEL_STRIDE);
    const float* w = a.mel_weight + m * MEL_STRIDE;
    float s = 0.0f;
    for (int j = sub; j < n; j += 16)
      if (start + j >= 0 && start + j < N_BINS) s = fmaf(w[j], power[start + j], s);
#pragma unroll
    for (int x = 8; x >= 1; x >>= 1) s += __shfl_xor(s, x);
    const float db = 10.0f * log10f(fmaxf(1e-10f, s));
    if (sub == 0) a.db[f * N_MELS + m] = db;
    best = fmaxf(best, db);
  }
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) best = fmaxf(best, __shfl_xor(best, x));
  if ((tid & 63) == 0) wave_max[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < THREADS / 64; ++w) best = fmaxf(best, wave_max[w]);
    atomicMax(a.clip_max + c, ordered_image(best));
  }
}

__device__ __forceinline__ float block_min_max(float v, bool want_max, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float o = __shfl_xor(v, m);
    v = want_max ? fmaxf(v, o) : fminf(v, o);
  }
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < THREADS / 64; ++w) r = want_max ? fmaxf(r, red[w]) : fminf(r, red[w]);
  return r;
}

__global__ void __launch_bounds__(THREADS) onset_pick_kernel(rg_onset_pick_args a) {
  __shared__ float red[THREADS / 64];
  __shared__ int wave_count[THREADS / 64];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t f0 = a.frame_off[c];
  const int64_t n = a.frame_off[c + 1] - f0;
  float* db = a.db + f0 * N_MELS;
  float* x = a.x + f0;
  float* avg = a.avg + f0;
  int* out = a.onset_frames + f0;

  // power_to_db(top_db=80): nothing lies more than 80 dB under this clip's maximum
  const float floor_db = ordered_value(a.clip_max[c]) - a.top_db;
  for (int64_t i = tid; i < n * N_MELS; i += THREADS) db[i] = fmaxf(db[i], floor_db);
  __syncthreads();

  // env[t] = mean over the bands of max(0, dB[t - 2] - dB[t - 3]), zero in the first three frames: one wave per frame, a lane
  // takes bands lane and lane + 64, the lanes add up by a butterfly (a fixed order)
  float lo = FLT_MAX, hi = -FLT_MAX;
  for (int64_t t = wave; t < n; t += THREADS / 64) {
    float e = 0.0f;
    if (t >= 3) {
      const float* cur = db + (t - 2) * N_MELS;
      const float* prev = cur - N_MELS;
      e = fmaxf(0.0f, cur[lane] - prev[lane]) + fmaxf(0.0f, cur[lane + 64] - prev[lane + 64]);
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) e += __shfl_xor(e, m);
      e *= 1.0f / N_MELS;
    }
    if (lane == 0) x[t] = e;
    lo = fminf(lo, e), hi = fmaxf(hi, e);
  }
  lo = block_min_max(lo, false, red);
  hi = block_min_max(hi, true, red);      // (its barriers also make the envelope visible to the whole workgroup)
  const bool silent = !(hi > 0.0f);        // the envelope is >= 0: all zero -> no onsets, x = avg = 0

  const float inv_den = silent ? 0.0f : 1.0f / ((hi - lo) + FLT_MIN);
  for (int64_t t = tid; t < n; t += THREADS) x[t] = silent ? 0.0f : (x[t] - lo) * inv_den;
  __syncthreads();

  // avg[t] = mean(x[max(t - 3, 0) : min(t + 4, n)]); onset when x > 0 and x >= avg + delta; kept in frame order: the flags of
  // 256 frames at a time, a wave's earlier flags by ballot, the earlier waves' and the earlier rounds' counts added in front
  int base = 0;
  for (int64_t t0 = 0; t0 < n; t0 += THREADS) {
    const int64_t t = t0 + tid;
    bool flag = false;
    if (t < n) {
      const int64_t b = t - a.pre_avg > 0 ? t - a.pre_avg : 0, e = t + a.post_avg < n ? t + a.post_avg : n;
      float s = 0.0f;
      for (int64_t i = b; i < e; ++i) s += x[i];
      const float m = silent ? 0.0f : s / (float)(e - b);
      avg[t] = m;
      flag = !silent && x[t] > 0.0f && x[t] >= m + a.delta;
    }
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int before = base, all = base;
    for (int w = 0; w < THREADS / 64; ++w) {
      if (w < wave) before += wave_count[w];
      all += wave_count[w];
    }
    if (flag) out[before + __popcll(mask & ((1ull << lane) - 1ull))] = (int)t;
    base = all;
    __syncthreads();
  }
  if (tid == 0) a.onset_count[c] = base;
}

// the offsets of a ragged batch: start at 0, do not decrease
bool offsets_ok(const int64_t* off, int n) {
  if (off[0] != 0) return false;
  for (int c = 0; c < n; ++c)
    if (off[c + 1] < off[c]) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------- rg_resample_poly
constexpr int RS_TILE = RG_RESAMPLE_TILE;
constexpr int RS_PER = RS_TILE / THREADS;            // outputs per thread
constexpr int RS_LDS_MAX = 64 * 1024;
static_assert(RS_TILE % THREADS == 0, "a tile is a whole number of outputs per thread");

// input samples a tile of RS_TILE outputs can reach: k_hi of its last output less k_hi of its first is at most
// (RS_TILE - 1) down / up + 1, and the first output reaches taps - 1 samples further back
inline int64_t resample_span(int up, int down, int taps) { return (int64_t)(RS_TILE - 1) * down / up + 1 + taps; }

// frame `frame` of the interleaved source, decoded and downmixed: the channels added up in channel order, one multiply
__device__ __forceinline__ float resample_frame(const void* __restrict__ src, int fmt, int channels, float inv_channels, int64_t frame) {
  const int64_t s = frame * channels;
  float sum = 0.0f;
  if (fmt == RG_RESAMPLE_PCM16) {
    const int16_t* v = static_cast<const int16_t*>(src) + s;
    for (int ch = 0; ch < channels; ++ch) sum += (float)v[ch] * (1.0f / 32768.0f);
  } else if (fmt == RG_RESAMPLE_PCM24) {
    const unsigned char* v = static_cast<const unsigned char*>(src) + 3 * s;
    for (int ch = 0; ch < channels; ++ch) {
      const unsigned u = (unsigned)v[3 * ch] | ((unsigned)v[3 * ch + 1] << 8) | ((unsigned)v[3 * ch + 2] << 16);
      sum += (float)((int)(u << 8) >> 8) * (1.0f / 8388608.0f);
    }
  } else if (fmt == RG_RESAMPLE_PCM32) {
    const int32_t* v = static_cast<const int32_t*>(src) + s;
    for (int ch = 0; ch < channels; ++ch) sum += (float)v[ch] * (1.0f / 2147483648.0f);
  } else {
    const float* v = static_cast<const float*>(src) + s;
    for (int ch = 0; ch < channels; ++ch) sum += v[ch];
  }
  return sum * inv_channels;
}

// Block b works on clip c = the last one with out_off[c] / RS_TILE + c <= b, tile b - (out_off[c] / RS_TILE + c) of it: that
// count grows by at least ceil(n_out / RS_TILE) from a clip to the next, so every tile of every clip has a block, a tile never
// spans two clips, and at most one block per clip finds nothing to do.  (grid = out_off[n_clips] / RS_TILE + n_clips)
template <bool LDS_COEFF>
__global__ void __launch_bounds__(THREADS) resample_poly_kernel(const void* __restrict__ src, int fmt, int channels, float inv_channels,
                                                                const int64_t* __restrict__ src_off, const int64_t* __restrict__ out_off,
                                                                int n_clips, int up, int down, int half_len, int taps,
                                                                const float* __restrict__ coeff, float* __restrict__ out) {
  extern __shared__ float rs_lds[];                 // the tile's input span, then (LDS_COEFF) the table
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  int lo = 0, hi = n_clips;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (out_off[mid] / RS_TILE + mid <= b) lo = mid; else hi = mid;
  }
  const int c = lo;
  const int64_t o0 = out_off[c], n_out = out_off[c + 1] - o0;
  const int64_t m0 = (b - (o0 / RS_TILE + c)) * RS_TILE;
  if (m0 >= n_out) return;                          // (the whole workgroup)
  const int64_t s0 = src_off[c], n = src_off[c + 1] - s0;
  const int cnt = (int)(n_out - m0 < RS_TILE ? n_out - m0 : RS_TILE);
  const int64_t kb = (m0 * down + half_len) / up - (taps - 1);                           // the first sample of the span
  const int span = (int)(((m0 + cnt - 1) * down + half_len) / up - kb) + 1;               // <= resample_span
  float* x = rs_lds;
  for (int i = tid; i < span; i += THREADS) {
    const int64_t k = kb + i;
    x[i] = (k >= 0 && k < n) ? resample_frame(src, fmt, channels, inv_channels, s0 + k) : 0.0f;
  }
  const float* cf = coeff;
  if (LDS_COEFF) {
    float* cl = rs_lds + ((int64_t)(RS_TILE - 1) * down / up + 1 + taps);
    for (int i = tid; i < up * taps; i += THREADS) cl[i] = coeff[i];
    cf = cl;
  }
  __syncthreads();
  if (!coeff) {                                     // up = down = taps = 1: the samples themselves
    for (int i = tid; i < cnt; i += THREADS) out[o0 + m0 + i] = x[i];
    return;
  }
  int base[RS_PER], row[RS_PER];
  float acc[RS_PER];
#pragma unroll
  for (int q = 0; q < RS_PER; ++q) {
    const int i = tid + q * THREADS;
    const int64_t cc = (m0 + (i < cnt ? i : 0)) * down + half_len;
    base[q] = (int)(cc / up - kb);                  // x[base - j] is sample k_hi - j
    row[q] = (int)(cc % up) * taps;
    acc[q] = 0.0f;
  }
  for (int j = 0; j < taps; ++j)
#pragma unroll
    for (int q = 0; q < RS_PER; ++q) acc[q] = fmaf(cf[row[q] + j], x[base[q] - j], acc[q]);
#pragma unroll
  for (int q = 0; q < RS_PER; ++q) {
    const int i = tid + q * THREADS;
    if (i < cnt) out[o0 + m0 + i] = acc[q];
  }
}

}  // namespace

extern "C" int rg_onset_mel_db(rg_handle* h, const rg_onset_mel_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_onset_mel_args& a = *args_host;
  RG_REQUIRE(h, a.samples && a.sample_off && a.sample_off_host && a.frame_off && a.frame_off_host && a.window && a.twiddle &&
                    a.mel_start && a.mel_len && a.mel_start_host && a.mel_len_host && a.mel_weight && a.db && a.clip_max,
             "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1, "need at least one clip");
  RG_REQUIRE(h, offsets_ok(a.sample_off_host, a.n_clips) && offsets_ok(a.frame_off_host, a.n_clips), "offsets must start at 0 and not decrease");
  for (int c = 0; c < a.n_clips; ++c)
    RG_REQUIRE(h, a.frame_off_host[c + 1] - a.frame_off_host[c] == 1 + (a.sample_off_host[c + 1] - a.sample_off_host[c]) / HOP,
               "a clip of n samples has 1 + n / 512 frames");
  for (int m = 0; m < N_MELS; ++m)
    RG_REQUIRE(h, a.mel_start_host[m] >= 0 && a.mel_len_host[m] >= 0 && a.mel_len_host[m] <= MEL_STRIDE &&
                      a.mel_start_host[m] + a.mel_len_host[m] <= N_BINS, "a mel filter leaves the 1025 bins or is longer than its row");
  const int64_t frames = a.frame_off_host[a.n_clips];
  RG_REQUIRE(h, frames < (int64_t)1 << 31, "too many frames in one call");
  hipError_t e = hipMemsetAsync(a.clip_max, 0, sizeof(unsigned) * a.n_clips, rg_stream(stream));   // below every image
  RG_REQUIRE(h, e == hipSuccess, hipGetErrorString(e));
  hipLaunchKernelGGL(onset_mel_db_kernel, dim3((unsigned)frames), dim3(THREADS), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_onset_pick(rg_handle* h, const rg_onset_pick_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_onset_pick_args& a = *args_host;
  RG_REQUIRE(h, a.db && a.clip_max && a.frame_off && a.frame_off_host && a.x && a.avg && a.onset_frames && a.onset_count, "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1, "need at least one clip");
  RG_REQUIRE(h, offsets_ok(a.frame_off_host, a.n_clips), "offsets must start at 0 and not decrease");
  RG_REQUIRE(h, a.frame_off_host[a.n_clips] < (int64_t)1 << 31, "too many frames in one call");
  RG_REQUIRE(h, a.pre_avg >= 0 && a.post_avg >= 1 && a.top_db > 0.0f && a.delta == a.delta, "need pre_avg >= 0, post_avg >= 1, top_db > 0 and a delta that is a number");
  hipLaunchKernelGGL(onset_pick_kernel, dim3(a.n_clips), dim3(THREADS), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_resample_poly(rg_handle* h, const void* src, int fmt, int channels, const int64_t* src_off, const int64_t* src_off_host,
                                const int64_t* out_off, const int64_t* out_off_host, int n_clips, int up, int down, int half_len, int taps,
                                const float* coeff, float* out, void* stream) {
  RG_REQUIRE(h, src && src_off && src_off_host && out_off && out_off_host && out, "null pointer");
  RG_REQUIRE(h, fmt == RG_RESAMPLE_PCM16 || fmt == RG_RESAMPLE_PCM24 || fmt == RG_RESAMPLE_PCM32 || fmt == RG_RESAMPLE_F32, "unknown sample format");
  RG_REQUIRE(h, channels >= 1 && channels <= RG_RESAMPLE_MAX_CHANNELS, "need 1 to 8 channels");
  RG_REQUIRE(h, n_clips >= 1, "need at least one clip");
  RG_REQUIRE(h, up >= 1 && down >= 1 && taps >= 1 && half_len >= 0, "need up, down, taps > 0 and half_len >= 0");
  RG_REQUIRE(h, (int64_t)taps == 2 * (int64_t)half_len / up + 1, "taps must be 2 half_len / up + 1");
  RG_REQUIRE(h, coeff || (up == 1 && down == 1 && half_len == 0), "no table: only a copy (up = down = 1, half_len = 0) goes without");
  RG_REQUIRE(h, offsets_ok(src_off_host, n_clips) && offsets_ok(out_off_host, n_clips), "offsets must start at 0 and not decrease");
  for (int c = 0; c < n_clips; ++c) {
    const int64_t n = src_off_host[c + 1] - src_off_host[c];
    RG_REQUIRE(h, n < ((int64_t)1 << 62) / up / down, "a clip is too long");
    RG_REQUIRE(h, out_off_host[c + 1] - out_off_host[c] == (n * up + down - 1) / down, "a clip of n frames has ceil(n up / down) outputs");
  }
  const bool lds_coeff = coeff && up <= 2;
  const int64_t lds = (resample_span(up, down, taps) + (lds_coeff ? (int64_t)up * taps : 0)) * (int64_t)sizeof(float);
  RG_REQUIRE(h, lds <= RS_LDS_MAX, "a tile's input span does not fit in 64 KB of LDS (down / up or the filter is too long)");
  const int64_t blocks = out_off_host[n_clips] / RS_TILE + n_clips;
  RG_REQUIRE(h, blocks < (int64_t)1 << 31, "too many outputs in one call");
  const float inv_channels = 1.0f / (float)channels;
  if (lds_coeff)
    hipLaunchKernelGGL(resample_poly_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), (size_t)lds, rg_stream(stream), src, fmt, channels,
                       inv_channels, src_off, out_off, n_clips, up, down, half_len, taps, coeff, out);
  else
    hipLaunchKernelGGL(resample_poly_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), (size_t)lds, rg_stream(stream), src, fmt, channels,
                       inv_channels, src_off, out_off, n_clips, up, down, half_len, taps, coeff, out);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
