// FGD evaluation (tools/evaluate.py:255-275, :436): the EMAGE skeleton-convolution encoder and the latent moments.
//   rg_fgd_encoder_layer : one SkeletonResidual layer of VAESKConv.map2latent (eval_models/skeleton.py:551-590) over a ragged
//                          batch of clips, one workgroup per clip
//   rg_latent_moments    : column mean + covariance of the latents in fp64 (metric.py:253-258)
#include "rg_reduce.h"

namespace {

constexpr int FGD_THREADS = 256;
constexpr int FGD_TT = 16;                       // output frames per time tile
constexpr int FGD_MAX_CIN = 480;                 // staged tile: (2 * FGD_TT + 2) rows x c_in floats <= 64 KiB
constexpr int FGD_MAX_GROUPS = 64;

// grid = n_clips, 256 threads.  Phases (each clip's data lives in r / s / y between them; the workgroup barrier orders them):
//  1. per time tile: stage input rows 2*t0-1 .. 2*t0+2*nt (zeros outside the clip) in LDS, then every (channel, frame) of the
//     tile: r = bias + sum over kept inputs and the 4 taps, s = bias + sum over kept inputs of the centre-right tap
//  2. GroupNorm statistics, one wave per group: fp64 sum -> mean, then fp64 sum of squared deviations -> biased variance
//  3. y = (r - mean) * rstd * gamma + beta + s, in place in r
//  4. out = tanh(pool(y)) (or tanh(y))
__global__ void __launch_bounds__(FGD_THREADS) fgd_layer_kernel(rg_fgd_layer_args a) {
  extern __shared__ float sx[];
  __shared__ float s_mean[FGD_MAX_GROUPS], s_rstd[FGD_MAX_GROUPS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cin = a.c_in, cout = a.c_out, cpool = a.c_pool;
  const int r0 = a.clip_off[blockIdx.x] >> a.layer, r1 = a.clip_off[blockIdx.x + 1] >> a.layer;
  const int T = r1 - r0, To = T >> 1, o0 = r0 >> 1;
  const float* __restrict__ x = a.x + (size_t)r0 * cin;
  float* __restrict__ R = a.r + (size_t)o0 * cout;
  float* __restrict__ S = a.s + (size_t)o0 * cout;
  float* __restrict__ Y = a.y + (size_t)o0 * cpool;
  const float4* __restrict__ wres = reinterpret_cast<const float4*>(a.w_res);

  for (int t0 = 0; t0 < To; t0 += FGD_TT) {
    const int nt = min(FGD_TT, To - t0), rows = 2 * nt + 2;
    __syncthreads();                                         // (the previous tile's readers are done)
    for (int i = tid; i < rows * cin; i += FGD_THREADS) {
      const int rr = i / cin, ch = i - rr * cin, tin = 2 * t0 - 1 + rr;
      sx[i] = (tin >= 0 && tin < T) ? x[(size_t)tin * cin + ch] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < cout * FGD_TT; i += FGD_THREADS) {
      const int o = i / FGD_TT, tl = i - o * FGD_TT;       // 16 lanes share an output channel: uniform weight loads
      if (tl >= nt) continue;
      const float* s0 = sx + 2 * tl * cin;
      float acc = 0.0f, sc = 0.0f;
      const int p1 = a.row_ptr[o + 1];
      for (int p = a.row_ptr[o]; p < p1; ++p) {
        const int ch = a.col[p];
        const float4 w = wres[p];
        const float x1 = s0[cin + ch];
        acc = fmaf(w.x, s0[ch], acc);
        acc = fmaf(w.y, x1, acc);
        acc = fmaf(w.z, s0[2 * cin + ch], acc);
        acc = fmaf(w.w, s0[3 * cin + ch], acc);
        sc = fmaf(a.w_sc[p], x1, sc);
      }
      R[(size_t)(t0 + tl) * cout + o] = acc + a.b_res[o];
      S[(size_t)(t0 + tl) * cout + o] = sc + a.b_sc[o];
    }
  }
  __syncthreads();

  const int cg = cout / a.groups, n = cg * To;
  for (int g = wave; g < a.groups; g += FGD_THREADS / 64) {
    double sum = 0.0;
    for (int i = lane; i < n; i += 64) {
      const int t = i / cg, ch = g * cg + (i - t * cg);
      sum += (double)R[(size_t)t * cout + ch];
    }
    const double mean = wave_sum_f64(sum) / n;
    double m2 = 0.0;
    for (int i = lane; i < n; i += 64) {
      const int t = i / cg, ch = g * cg + (i - t * cg);
      const double d = (double)R[(size_t)t * cout + ch] - mean;
      m2 = fma(d, d, m2);
    }
    const double var = wave_sum_f64(m2) / n;
    if (lane == 0) {
      s_mean[g] = (float)mean;
      s_rstd[g] = (float)(1.0 / sqrt(var + (double)a.eps));
    }
  }
  __syncthreads();

  for (int i = tid; i < To * cout; i += FGD_THREADS) {
    const int o = i % cout, g = o / cg;
    R[i] = (R[i] - s_mean[g]) * (s_rstd[g] * a.gamma[o]) + a.beta[o] + S[i];
  }
  __syncthreads();

  for (int i = tid; i < To * cpool; i += FGD_THREADS) {
    const int t = i / cpool, p = i - t * cpool;
    float v;
    if (a.pool_src) {
      v = 0.0f;
      for (int k = 0; k < a.pool_k; ++k) {
        const int src = a.pool_src[p * a.pool_k + k];
        if (src >= 0 && src < cout) v = fmaf(a.pool_w[p * a.pool_k + k], R[(size_t)t * cout + src], v);
      }
    } else {
      v = R[(size_t)t * cout + p];
    }
    Y[(size_t)t * cpool + p] = tanhf(v);
  }
}

// mean: grid = ceil(dim / 64), 256 threads = 64 columns x 4 row phases; fp64, fixed order
__global__ void __launch_bounds__(256) moments_mean_kernel(const float* __restrict__ lat, int n, int dim, double* __restrict__ mean) {
  __shared__ double part[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  double s = 0.0;
  if (c < dim)
    for (int r = ph; r < n; r += 4) s += (double)lat[(size_t)r * dim + c];
  part[ph][threadIdx.x & 63] = s;
  __syncthreads();
  if (ph == 0 && c < dim) mean[c] = (((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x]) / n;
}

// covariance: grid = (ceil(dim/32), ceil(dim/32)), 256 threads, each a 2 x 2 block of a 32 x 32 tile; rows in chunks of 32
// staged centred (fp64) in LDS.  cov[i][j] and cov[j][i] see the same products in the same order: exactly symmetric.
constexpr int MT = 32;
__global__ void __launch_bounds__(256) moments_cov_kernel(const float* __restrict__ lat, int n, int dim,
                                                          const double* __restrict__ mean, double* __restrict__ cov) {
  __shared__ double sa[MT][MT + 1], sb[MT][MT + 1];
  const int i0 = blockIdx.y * MT, j0 = blockIdx.x * MT;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int r0 = 0; r0 < n; r0 += MT) {
    __syncthreads();
    for (int e = threadIdx.x; e < MT * MT; e += 256) {
      const int rr = e / MT, cc = e % MT, r = r0 + rr;
      const int ci = i0 + cc, cj = j0 + cc;
      sa[rr][cc] = (r < n && ci < dim) ? (double)lat[(size_t)r * dim + ci] - mean[ci] : 0.0;
      sb[rr][cc] = (r < n && cj < dim) ? (double)lat[(size_t)r * dim + cj] - mean[cj] : 0.0;
    }
    __syncthreads();
    const int m = min(MT, n - r0);
    for (int rr = 0; rr < m; ++rr) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = fma(sa[rr][ty + 16 * u], sb[rr][tx + 16 * v], acc[u][v]);
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < dim && j < dim) cov[(size_t)i * dim + j] = acc[u][v] / (n - 1);
    }
}

}  // namespace

extern "C" int rg_fgd_encoder_layer(rg_handle* h, const rg_fgd_layer_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_fgd_layer_args& a = *args_host;
  RG_REQUIRE(h, a.x && a.y && a.r && a.s && a.clip_off && a.clip_off_host && a.row_ptr && a.col && a.w_res && a.w_sc &&
                    a.b_res && a.b_sc && a.gamma && a.beta, "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1 && a.layer >= 0 && a.layer <= 3, "bad clip count or layer");
  RG_REQUIRE(h, a.c_in >= 1 && a.c_in <= FGD_MAX_CIN && a.c_out >= 1 && a.c_pool >= 1, "bad channel counts");
  RG_REQUIRE(h, a.groups >= 1 && a.groups <= FGD_MAX_GROUPS && a.c_out % a.groups == 0, "c_out must be a multiple of groups <= 64");
  RG_REQUIRE(h, a.eps >= 0.0f, "negative eps");
  if (a.pool_src) RG_REQUIRE(h, a.pool_w && a.pool_k >= 1 && a.pool_k <= 16, "bad pool");
  else RG_REQUIRE(h, a.c_pool == a.c_out, "without a pool c_pool must equal c_out");
  RG_REQUIRE(h, a.clip_off_host[0] == 0, "clip_off must start at 0");
  for (int c = 0; c < a.n_clips; ++c) {
    const int len = a.clip_off_host[c + 1] - a.clip_off_host[c];
    RG_REQUIRE(h, len >= 16 && len % 16 == 0, "every clip must be a positive multiple of 16 frames");
  }
  const size_t lds = (size_t)(2 * FGD_TT + 2) * a.c_in * sizeof(float);
  hipLaunchKernelGGL(fgd_layer_kernel, dim3(a.n_clips), dim3(FGD_THREADS), lds, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_latent_moments(rg_handle* h, const float* lat, int n, int dim, double* mean, double* cov, void* stream) {
  RG_REQUIRE(h, lat && mean && cov, "null pointer");
  RG_REQUIRE(h, n >= 2 && dim >= 1 && dim <= 4096, "need n >= 2 rows and 1 <= dim <= 4096");
  hipLaunchKernelGGL(moments_mean_kernel, dim3((dim + 63) / 64), dim3(256), 0, rg_stream(stream), lat, n, dim, mean);
  RG_CHECK_LAUNCH(h);
  const int nt = (dim + MT - 1) / MT;
  hipLaunchKernelGGL(moments_cov_kernel, dim3(nt, nt), dim3(256), 0, rg_stream(stream), lat, n, dim, mean, cov);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
