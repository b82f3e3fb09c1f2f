// Conditioning feature extraction per window (tools/longform_synthesis.py:64-94): the small kernels the
// wav2vec2-base and BERT-base forwards need besides rg_gemm / rg_mha_bf16 / rg_layernorm_res -- all HBM-bound byte movers.
//   rg_embed_sum3          BERT embeddings: word[id] + position[i] + token_type[0]
//   rg_time_groupnorm_gelu wav2vec2 feature extractor layer 0: GroupNorm(512 groups = per channel, over time) -> GELU -> bf16
//   rg_im2col_grouped      wav2vec2 positional convolution (k = 128, 16 groups, padding 64): per-group patch matrix, bf16
// and their forms for many windows per launch (Wav2Vec2Features.batch / BertFeatures.batch):
//   rg_wave_normalize, rg_time_groupnorm_gelu_batched, rg_im2col_grouped_batched, rg_embed_sum3_ragged
#include "rg_common.h"

namespace {

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

__global__ void __launch_bounds__(256) embed_sum3_kernel(const int64_t* __restrict__ ids, const float* __restrict__ word,
                                                        const float* __restrict__ pos, const float* __restrict__ type0,
                                                        float* __restrict__ out, int L, int dim) {
  const int64_t total = (int64_t)L * dim;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i / dim), c = (int)(i % dim);
    out[i] = word[(size_t)ids[t] * dim + c] + type0[c] + pos[(size_t)t * dim + c];   // HF order: inputs + token_type, + position
  }
}

// column sums of x [T][C] (or of (x - mean)^2 when mean != null) into acc[C]; thread -> column, block -> 64 rows
__global__ void __launch_bounds__(256) col_reduce_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                        float* __restrict__ acc, int T, int C, float inv_t) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const int t0 = blockIdx.x * 64, t1 = min(T, t0 + 64);
  const float m = mean ? mean[c] * inv_t : 0.f;
  float s = 0.f;
  for (int t = t0; t < t1; ++t) {
    const float d = x[(size_t)t * C + c] - m;
    s += mean ? d * d : d;
  }
  atomicAdd(acc + c, s);
}

__global__ void __launch_bounds__(256) groupnorm_gelu_kernel(const float* __restrict__ x, const float* __restrict__ sum,
                                                            const float* __restrict__ sq, const float* __restrict__ g,
                                                            const float* __restrict__ b, unsigned short* __restrict__ out,
                                                            float* __restrict__ out32, int64_t total, int C, float inv_t,
                                                            float eps) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const float mean = sum[c] * inv_t;
    const float rstd = 1.0f / sqrtf(sq[c] * inv_t + eps);
    const float v = gelu_erf((x[i] - mean) * rstd * g[c] + b[c]);
    if (out) out[i] = __builtin_bit_cast(unsigned short, (__bf16)v);
    if (out32) out32[i] = v;
  }
}

// out[g][t][k * Cg + ci] = xpad[t + k][g * Cg + ci], xpad = x padded with `pad` zero rows in front (and behind)
__global__ void __launch_bounds__(256) im2col_grouped_kernel(const float* __restrict__ x, unsigned short* __restrict__ out,
                                                            int T, int C, int groups, int ksize, int pad) {
  const int Cg = C / groups;
  const int64_t row_len = (int64_t)ksize * Cg, total = (int64_t)groups * T * row_len;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ci = (int)(i % Cg);
    const int k = (int)((i / Cg) % ksize);
    const int t = (int)((i / row_len) % T);
    const int g = (int)(i / (row_len * T));
    const int ts = t + k - pad;
    const float v = (ts >= 0 && ts < T) ? x[(size_t)ts * C + g * Cg + ci] : 0.f;
    out[i] = __builtin_bit_cast(unsigned short, (__bf16)v);
  }
}

// ------------------------------------------------------------------------------ many windows per launch
// sum over the workgroup's 1024 threads in a fixed order (xor tree inside a wave, then the 16 wave sums one after the other)
__device__ __forceinline__ float block_sum_1024(float v, float* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  __syncthreads();                                   // red may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) s += red[w];
  return s;
}

// one workgroup per window: mean about the first sample (a constant window has mean == its value and variance 0 exactly),
// biased variance about the mean, then the normalised samples and the zero padding
__global__ void __launch_bounds__(1024) wave_normalize_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out,
                                                             int n, int n_pad, int normalize) {
  __shared__ float red[16];
  const float* xb = x + (size_t)blockIdx.x * ldx;
  float* ob = out + (size_t)blockIdx.x * n_pad;
  float mean = 0.f, den = 1.f;
  if (normalize) {
    const float x0 = xb[0];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) s += xb[i] - x0;
    mean = x0 + block_sum_1024(s, red) / (float)n;
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) {
      const float d = xb[i] - mean;
      q = fmaf(d, d, q);
    }
    den = sqrtf(block_sum_1024(q, red) / (float)n + 1e-7f);
  }
  for (int i = threadIdx.x; i < n_pad; i += 1024) ob[i] = i < n ? (xb[i] - mean) / den : 0.f;
}

// per (window, channel) sums over the rows t < T of x [B][T_pad][C] (of (x - mean)^2 when mean != null) into acc[b][C]:
// grid (ceil(C / 32), B), 1024 threads = 32 channels (one 128-byte line per row) x 32 row phases; every thread adds its rows in
// order (eight running sums, combined in a fixed tree), the 32 phases are added in order: no atomics, the same bits every run
__global__ void __launch_bounds__(1024) col_reduce_batched_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                 float* __restrict__ acc, int T, int T_pad, int C, float inv_t) {
  __shared__ float red[32][33];
  const int cl = threadIdx.x & 31, ph = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, b = blockIdx.y;
  const bool ok = c < C;
  const float* xb = x + (size_t)b * T_pad * C + (ok ? c : 0);
  const float m = (mean && ok) ? mean[(size_t)b * C + c] * inv_t : 0.f;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    for (int t = ph; t < T; t += 32 * 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (t + 32 * j < T) {
          const float d = xb[(size_t)(t + 32 * j) * C] - m;
          a[j] += mean ? d * d : d;
        }
      }
    }
  }
  red[ph][cl] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (ph == 0 && ok) {
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < 32; ++p) s += red[p][cl];
    acc[(size_t)b * C + c] = s;
  }
}

// four channels per thread (C % 4 == 0); rows t >= T of a window come out as zero
__global__ void __launch_bounds__(256) groupnorm_gelu_batched_kernel(const float* __restrict__ x, const float* __restrict__ sum,
                                                                    const float* __restrict__ sq, const float* __restrict__ g,
                                                                    const float* __restrict__ b, unsigned short* __restrict__ out,
                                                                    float* __restrict__ out32, int64_t total4, int T, int T_pad,
                                                                    int C, float inv_t, float eps) {
  const int C4 = C / 4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const int64_t row = i / C4;
    const int t = (int)(row % T_pad), w = (int)(row / T_pad);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (t < T) {
      const float4 xv = *reinterpret_cast<const float4*>(x + i * 4);
      const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float mean = sum[(size_t)w * C + c + e] * inv_t;
        const float rstd = 1.0f / sqrtf(sq[(size_t)w * C + c + e] * inv_t + eps);
        v[e] = gelu_erf((xs[e] - mean) * rstd * g[c + e] + b[c + e]);
      }
    }
    if (out) {
      ushort4 o;
      o.x = __builtin_bit_cast(unsigned short, (__bf16)v[0]);
      o.y = __builtin_bit_cast(unsigned short, (__bf16)v[1]);
      o.z = __builtin_bit_cast(unsigned short, (__bf16)v[2]);
      o.w = __builtin_bit_cast(unsigned short, (__bf16)v[3]);
      *reinterpret_cast<ushort4*>(out + i * 4) = o;
    }
    if (out32) *reinterpret_cast<float4*>(out32 + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// out[g][w * T + t][k * Cg + ci] = x[w * T + t + k - pad][g * Cg + ci] inside the window's own rows, else zero; four ci per thread
__global__ void __launch_bounds__(256) im2col_grouped_batched_kernel(const float* __restrict__ x, unsigned short* __restrict__ out,
                                                                    int B, int T, int C, int groups, int ksize, int pad) {
  const int Cg = C / groups, Cg4 = Cg / 4;
  const int64_t row4 = (int64_t)ksize * Cg4, rows = (int64_t)B * T, total4 = (int64_t)groups * rows * row4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int ci = (int)(i % Cg4) * 4;
    const int k = (int)((i / Cg4) % ksize);
    const int64_t r = (i / row4) % rows;
    const int g = (int)(i / (row4 * rows));
    const int t = (int)(r % T), ts = t + k - pad;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ts >= 0 && ts < T) v = *reinterpret_cast<const float4*>(x + (size_t)(r - t + ts) * C + g * Cg + ci);
    ushort4 o;
    o.x = __builtin_bit_cast(unsigned short, (__bf16)v.x);
    o.y = __builtin_bit_cast(unsigned short, (__bf16)v.y);
    o.z = __builtin_bit_cast(unsigned short, (__bf16)v.z);
    o.w = __builtin_bit_cast(unsigned short, (__bf16)v.w);
    *reinterpret_cast<ushort4*>(out + i * 4) = o;
  }
}

// token rows of all sequences concatenated; the row's sequence by bisection of seq_off
__global__ void __launch_bounds__(256) embed_sum3_ragged_kernel(const int64_t* __restrict__ ids, const float* __restrict__ word,
                                                               const float* __restrict__ pos, const float* __restrict__ type0,
                                                               float* __restrict__ out, const int* __restrict__ seq_off,
                                                               int n_seq, int rows, int dim) {
  const int64_t total = (int64_t)rows * dim;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i / dim), c = (int)(i % dim);
    int lo = 0, hi = n_seq - 1;                      // the last s with seq_off[s] <= t
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (seq_off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    out[i] = word[(size_t)ids[t] * dim + c] + type0[c] + pos[(size_t)(t - seq_off[lo]) * dim + c];
  }
}

}  // namespace

extern "C" int rg_wave_normalize(rg_handle* h, const float* x, int64_t ldx, float* out, int B, int n, int n_pad, int normalize,
                                 void* stream) {
  RG_REQUIRE(h, x && out, "null pointer");
  RG_REQUIRE(h, B > 0 && n > 0 && n_pad >= n && ldx >= n, "bad shape (n <= n_pad, n <= ldx)");
  hipLaunchKernelGGL(wave_normalize_kernel, dim3(B), dim3(1024), 0, rg_stream(stream), x, ldx, out, n, n_pad, normalize);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_time_groupnorm_gelu_batched(rg_handle* h, const float* x, const float* gamma, const float* beta, void* out_bf16,
                                              float* out_f32, int B, int T, int T_pad, int C, float eps, float* workspace,
                                              void* stream) {
  RG_REQUIRE(h, x && gamma && beta && (out_bf16 || out_f32) && workspace, "null pointer");
  RG_REQUIRE(h, B > 0 && B <= 65535 && T > 0 && T_pad >= T && C > 0 && C % 4 == 0, "bad shape (T <= T_pad, C % 4 == 0, B <= 65535)");
  hipStream_t s = rg_stream(stream);
  const dim3 grid((C + 31) / 32, B);
  const float inv_t = 1.0f / (float)T;
  float* sum = workspace;
  float* sq = workspace + (size_t)B * C;
  hipLaunchKernelGGL(col_reduce_batched_kernel, grid, dim3(1024), 0, s, x, (const float*)nullptr, sum, T, T_pad, C, inv_t);
  hipLaunchKernelGGL(col_reduce_batched_kernel, grid, dim3(1024), 0, s, x, (const float*)sum, sq, T, T_pad, C, inv_t);
  const int64_t total4 = (int64_t)B * T_pad * (C / 4);
  hipLaunchKernelGGL(groupnorm_gelu_batched_kernel, dim3(rg_grid_1d(total4, 256)), dim3(256), 0, s, x, (const float*)sum,
                     (const float*)sq, gamma, beta, reinterpret_cast<unsigned short*>(out_bf16), out_f32, total4, T, T_pad, C, inv_t,
                     eps);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_im2col_grouped_batched(rg_handle* h, const float* x, void* out_bf16, int B, int T, int C, int groups, int ksize,
                                         int pad, void* stream) {
  RG_REQUIRE(h, x && out_bf16, "null pointer");
  RG_REQUIRE(h, B > 0 && T > 0 && C > 0 && groups > 0 && C % groups == 0 && (C / groups) % 4 == 0 && ksize > 0 && pad >= 0 &&
                    (int64_t)B * T <= INT32_MAX,
             "bad shape ((C / groups) % 4 == 0)");
  hipLaunchKernelGGL(im2col_grouped_batched_kernel, dim3(rg_grid_1d((int64_t)B * T * (C / 4) * ksize, 256)), dim3(256), 0,
                     rg_stream(stream), x, reinterpret_cast<unsigned short*>(out_bf16), B, T, C, groups, ksize, pad);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_embed_sum3_ragged(rg_handle* h, const int64_t* ids, const float* word, const float* pos, const float* type0,
                                    float* out, const int* seq_off, const int* seq_off_host, int n_seq, int dim, int max_pos,
                                    void* stream) {
  RG_REQUIRE(h, ids && word && pos && type0 && out && seq_off && seq_off_host, "null pointer");
  RG_REQUIRE(h, n_seq > 0 && dim > 0 && max_pos > 0, "bad shape");
  RG_REQUIRE(h, seq_off_host[0] == 0, "seq_off must start at 0");
  for (int s = 0; s < n_seq; ++s)
    RG_REQUIRE(h, seq_off_host[s + 1] >= seq_off_host[s] && seq_off_host[s + 1] - seq_off_host[s] <= max_pos,
               "seq_off must not decrease, and no sequence may be longer than max_pos");
  const int rows = seq_off_host[n_seq];
  RG_REQUIRE(h, rows > 0, "no token rows");
  hipLaunchKernelGGL(embed_sum3_ragged_kernel, dim3(rg_grid_1d((int64_t)rows * dim, 256)), dim3(256), 0, rg_stream(stream), ids,
                     word, pos, type0, out, seq_off, n_seq, rows, dim);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_embed_sum3(rg_handle* h, const int64_t* ids, const float* word, const float* pos, const float* type0,
                             float* out, int L, int dim, void* stream) {
  RG_REQUIRE(h, ids && word && pos && type0 && out, "null pointer");
  RG_REQUIRE(h, L > 0 && dim > 0, "bad shape");
  hipLaunchKernelGGL(embed_sum3_kernel, dim3(rg_grid_1d((int64_t)L * dim, 256)), dim3(256), 0, rg_stream(stream), ids, word, pos,
                     type0, out, L, dim);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_time_groupnorm_gelu(rg_handle* h, const float* x, const float* gamma, const float* beta, void* out_bf16,
                                      float* out_f32, int T, int C, float eps, float* workspace, void* stream) {
  RG_REQUIRE(h, x && gamma && beta && (out_bf16 || out_f32) && workspace, "null pointer");
  RG_REQUIRE(h, T > 0 && C > 0, "bad shape");
  hipStream_t s = rg_stream(stream);
  if (hipMemsetAsync(workspace, 0, sizeof(float) * 2 * C, s) != hipSuccess) return RG_ERR_HIP;
  const dim3 grid((T + 63) / 64, (C + 255) / 256);
  const float inv_t = 1.0f / (float)T;
  hipLaunchKernelGGL(col_reduce_kernel, grid, dim3(256), 0, s, x, (const float*)nullptr, workspace, T, C, inv_t);
  hipLaunchKernelGGL(col_reduce_kernel, grid, dim3(256), 0, s, x, (const float*)workspace, workspace + C, T, C, inv_t);
  hipLaunchKernelGGL(groupnorm_gelu_kernel, dim3(rg_grid_1d((int64_t)T * C, 256)), dim3(256), 0, s, x, workspace, workspace + C,
                     gamma, beta, reinterpret_cast<unsigned short*>(out_bf16), out_f32, (int64_t)T * C, C, inv_t, eps);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_im2col_grouped(rg_handle* h, const float* x, void* out_bf16, int T, int C, int groups, int ksize, int pad,
                                 void* stream) {
  RG_REQUIRE(h, x && out_bf16, "null pointer");
  RG_REQUIRE(h, T > 0 && C > 0 && groups > 0 && C % groups == 0 && ksize > 0 && pad >= 0, "bad shape");
  hipLaunchKernelGGL(im2col_grouped_kernel, dim3(rg_grid_1d((int64_t)T * C * ksize, 256)), dim3(256), 0, rg_stream(stream), x,
                     reinterpret_cast<unsigned short*>(out_bf16), T, C, groups, ksize, pad);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
