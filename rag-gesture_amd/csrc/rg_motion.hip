// SMPL-X joint metrics (tools/evaluate.py:286-464, tools/evaluate_mm.py:158-187): forward kinematics of the 55 joints and the
// per-clip statistics the reference computes on them.
//   rg_smplx_joints        : J_transformed of smplx.lbs.batch_rigid_transform for axis-angle poses, one wave per frame
//   rg_joint_clip_stats    : per clip, the L1div partial sum, the motion-beat flags and the masked MPJPE sum (metric.py)
//   rg_pair_distance_sums  : per group of rows, sum over pairs i < j of ||X_i - X_j||, pairs accumulated in fp64
//   rg_srgr_clip_sums      : per clip, the sem-weighted sum and the count of joint-frames within the SRGR threshold (metric.py)
#include "rg_reduce.h"
#include "rg_smplx.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int PD_TILE = 32;            // 32 x 32 row pairs per workgroup
constexpr int PD_CHUNK = 64;           // columns staged in LDS per step

// the forward kinematics of rg_smplx.h on the frame's pose row and its clip's rest joints; stores the joints.  (Frames past
// the end and lanes past the joints compute frame 0's / joint 0's values and write nothing.)
__global__ void __launch_bounds__(FK_THREADS) smplx_fk_kernel(rg_smplx_joints_args a, int total) {
  __shared__ float g[FK_THREADS / 64][NJ][12];     // per wave: the 3 x 4 global transform of every joint, row-major
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * (FK_THREADS / 64) + wave;
  const int jl = lane < NJ ? lane : 0, ff = f < total ? f : 0;
  const bool live = f < total && lane < NJ;
  const fk_tree tr = fk_tree_of(a.parents, lane);
  float J[3], t[3], R[9];
  fk_rest_joint(a.rest + (size_t)clip_of(a.clip_off, a.n_clips, ff) * NJ * 3, nullptr, nullptr, jl, J);
  fk_bone(J, tr.par, t);
  fk_rotation(a.poses + (size_t)ff * POSE_DIM + 3 * jl, a.pose_mean ? a.pose_mean + 3 * jl : nullptr, a.fold, R);
  fk_chain(g[wave], tr, live, lane, R, t);
  if (live) {
    const float* mine = g[wave][lane];
    float* o = a.joints + ((size_t)f * NJ + lane) * 3;
    o[0] = mine[3], o[1] = mine[7], o[2] = mine[11];
  }
}

// velocity norm of joint j at frame t of a clip of n >= 2 frames, over mmae (metric.py:97-109): forward difference at the first
// frame, central in the middle, backward at the last; fp32 differences over fp32 dt, fp32 norm, fp64 division by mmae[j]
__device__ __forceinline__ double joint_vel(const float* J, int n, int t, int j, float dt, float dt2, double mmae) {
  int t1 = t + 1, t0 = t - 1;
  float sc = dt2;
  if (t == 0) t0 = 0, sc = dt;
  if (t == n - 1) t1 = n - 1, sc = dt;
  const float* p1 = J + ((size_t)t1 * NJ + j) * 3;
  const float* p0 = J + ((size_t)t0 * NJ + j) * 3;
  const float dx = (p1[0] - p0[0]) / sc, dy = (p1[1] - p0[1]) / sc, dz = (p1[2] - p0[2]) / sc;
  return (double)sqrtf(dx * dx + dy * dy + dz * dz) / mmae;
}

// one workgroup per clip: (1) L1div partial, two-pass fp64; (2) beat flags; (3) masked MPJPE sum against the retrieval
__global__ void __launch_bounds__(ST_THREADS) joint_stats_kernel(rg_joint_stats_args a) {
  __shared__ double mean[POSE_DIM];
  __shared__ double red[ST_THREADS / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int r0 = a.clip_off[c], n = a.clip_off[c + 1] - r0;
  const float* J = a.joints + (size_t)r0 * POSE_DIM;

  if (tid < POSE_DIM) {
    double s = 0.0;
    for (int t = 0; t < n; ++t) s += (double)J[(size_t)t * POSE_DIM + tid];
    mean[tid] = s / n;
  }
  __syncthreads();
  double l1 = 0.0;
  for (int i = tid; i < n * POSE_DIM; i += ST_THREADS) l1 += fabs((double)J[i] - mean[i % POSE_DIM]);
  l1 = block_sum_f64(l1, red);
  if (tid == 0) a.l1_sum[c] = l1;

  if (a.beats) {
    // argrelextrema(vel[t_start:t_end], np.less, order, mode='clip') (metric.py:118): window index w is a minimum when it is
    // strictly below every neighbour within `order` inside the window (the clipped edges compare with themselves: never a
    // minimum).  metric.py:121-123 then keeps w when vel at frame w -- the window-relative index read as an absolute frame --
    // is above the threshold.  The flag is stored at frame t_start + w.
    const int ts = a.t_margin, L = n - 2 * a.t_margin;
    unsigned char* B = a.beats + (size_t)r0 * NJ;
    for (int i = tid; i < n * NJ; i += ST_THREADS) {
      const int t = i / NJ, j = i - t * NJ, w = t - ts;
      unsigned char flag = 0;
      if (w >= 1 && w <= L - 2) {
        const double mm = a.mmae[j];
        const double v = joint_vel(J, n, t, j, a.dt, a.dt2, mm);
        bool is_min = true;
        for (int k = 1; k <= a.order && is_min; ++k) {
          const int wp = min(w + k, L - 1), wm = max(w - k, 0);
          is_min = v < joint_vel(J, n, ts + wp, j, a.dt, a.dt2, mm) && v < joint_vel(J, n, ts + wm, j, a.dt, a.dt2, mm);
        }
        flag = is_min && joint_vel(J, n, w, j, a.dt, a.dt2, mm) > a.threshold;
      }
      B[i] = flag;
    }
  }

  if (a.mpjpe_sum) {
    const int q0 = a.retr_off[c];
    double e = 0.0;
    if (q0 >= 0) {
      const float* Q = a.retr_joints + (size_t)q0 * POSE_DIM;
      const float* P = a.retr_poses + (size_t)q0 * POSE_DIM;
      for (int i = tid; i < n * NJ; i += ST_THREADS) {
        const int j = i % NJ;
        const float* pp = P + (size_t)i * 3;
        if (!a.joint_mask[j] || (pp[0] == 0.f && pp[1] == 0.f && pp[2] == 0.f)) continue;
        const float* x = J + (size_t)i * 3;
        const float* y = Q + (size_t)i * 3;
        const float dx = (x[0] - J[0]) - (y[0] - Q[0]), dy = (x[1] - J[1]) - (y[1] - Q[1]), dz = (x[2] - J[2]) - (y[2] - Q[2]);
        e += sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
      }
    }
    e = block_sum_f64(e, red);
    if (tid == 0) a.mpjpe_sum[c] = e;
  }
}

// one workgroup per clip, threads stride over (frame, joint): metric.py:41-46 SRGR.run.  A success adds its frame's weight to
// the thread's fp64 sum; the thread sums meet in block_sum_f64's fixed order, so the bits depend on the clip alone.
__global__ void __launch_bounds__(ST_THREADS) srgr_kernel(rg_srgr_args a) {
  __shared__ double red[ST_THREADS / 64];
  __shared__ long long redc[ST_THREADS / 64];
  const int c = blockIdx.x, tid = threadIdx.x, nj = a.n_joints;
  const int r0 = a.clip_off[c], n = a.clip_off[c + 1] - r0;
  const float* P = a.pred + (size_t)r0 * nj * 3;
  const float* G = a.gt + (size_t)r0 * nj * 3;
  const float* W = a.weights + r0;
  const long long total = (long long)n * nj;
  double s = 0.0;
  long long k = 0;
  for (long long i = tid; i < total; i += ST_THREADS) {
    const float* x = P + i * 3;
    const float* y = G + i * 3;
    const float diff = (fabsf(x[0] - y[0]) + fabsf(x[1] - y[1])) + fabsf(x[2] - y[2]);
    if (diff < a.threshold) {
      s += (double)W[i / nj];
      ++k;
    }
  }
  s = block_sum_f64(s, red);
  k = block_sum_i64(k, redc);
  if (tid == 0) {
    a.wsum[c] = s;
    a.count[c] = k;
  }
}

// grid = (tiles, tiles, groups): tile (I, J), I <= J, of group g; 256 threads each own 2 x 2 pairs of the 32 x 32 tile.
// Columns stream through LDS in chunks of 64; differences in fp32, squares accumulated per pair in fp64.  The tile's sum
// (pairs i < j only, fixed order) goes to partial[(g * tiles + I) * tiles + J].
__global__ void __launch_bounds__(256) pair_dist_tile_kernel(rg_pair_dist_args a, int tiles) {
  __shared__ float sa[PD_TILE][PD_CHUNK + 1], sb[PD_TILE][PD_CHUNK + 1];
  __shared__ double red[4];
  const int I = blockIdx.y, Jt = blockIdx.x, g = blockIdx.z;
  const int g0 = a.group_off[g], ng = a.group_off[g + 1] - g0;
  const int nt = (ng + PD_TILE - 1) / PD_TILE;
  if (I > Jt || Jt >= nt) return;                  // (uniform per workgroup: no barrier is skipped by part of it)
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = I * PD_TILE, j0 = Jt * PD_TILE;
  const int D = a.dim;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int k0 = 0; k0 < D; k0 += PD_CHUNK) {
    const int kc = min(PD_CHUNK, D - k0);
    __syncthreads();
    for (int e = threadIdx.x; e < PD_TILE * PD_CHUNK; e += 256) {
      const int rr = e / PD_CHUNK, kk = e - rr * PD_CHUNK;
      const int ri = i0 + rr, rj = j0 + rr;
      sa[rr][kk] = (ri < ng && kk < kc) ? a.x[(size_t)(g0 + ri) * D + k0 + kk] : 0.f;
      sb[rr][kk] = (rj < ng && kk < kc) ? a.x[(size_t)(g0 + rj) * D + k0 + kk] : 0.f;
    }
    __syncthreads();
    for (int kk = 0; kk < kc; ++kk) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const double d = (double)(sa[ty + 16 * u][kk] - sb[tx + 16 * v][kk]);
          acc[u][v] = fma(d, d, acc[u][v]);
        }
    }
  }
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < j && j < ng) s += sqrt(acc[u][v]);
    }
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) a.partial[((size_t)g * tiles + I) * tiles + Jt] = s;
}

// one workgroup per group: the sum of its upper-triangle tile sums in a fixed order
__global__ void __launch_bounds__(256) pair_dist_reduce_kernel(rg_pair_dist_args a, int tiles) {
  __shared__ double red[4];
  const int g = blockIdx.x;
  const int ng = a.group_off[g + 1] - a.group_off[g], nt = (ng + PD_TILE - 1) / PD_TILE;
  double s = 0.0;
  for (int e = threadIdx.x; e < nt * nt; e += 256) {
    const int I = e / nt, Jt = e - I * nt;
    if (I <= Jt) s += a.partial[((size_t)g * tiles + I) * tiles + Jt];
  }
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) a.out[g] = s;
}

}  // namespace

extern "C" int rg_smplx_joints(rg_handle* h, const rg_smplx_joints_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_smplx_joints_args& a = *args_host;
  RG_REQUIRE(h, a.poses && a.rest && a.parents && a.parents_host && a.clip_off && a.clip_off_host && a.joints, "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1, "need at least one clip");
  const char* bad = bad_parents(a.parents_host);
  RG_REQUIRE(h, !bad, bad);
  bad = bad_clip_off(a.clip_off_host, a.n_clips);
  RG_REQUIRE(h, !bad, bad);
  const int total = a.clip_off_host[a.n_clips];
  if (total == 0) return RG_OK;
  const int fpb = FK_THREADS / 64;
  hipLaunchKernelGGL(smplx_fk_kernel, dim3((total + fpb - 1) / fpb), dim3(FK_THREADS), 0, rg_stream(stream), a, total);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_joint_clip_stats(rg_handle* h, const rg_joint_stats_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_joint_stats_args& a = *args_host;
  RG_REQUIRE(h, a.joints && a.clip_off && a.clip_off_host && a.l1_sum, "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1, "need at least one clip");
  RG_REQUIRE(h, a.clip_off_host[0] == 0, "clip_off must start at 0");
  for (int c = 0; c < a.n_clips; ++c) RG_REQUIRE(h, a.clip_off_host[c + 1] - a.clip_off_host[c] >= 2, "every clip needs >= 2 frames");
  if (a.beats) {
    RG_REQUIRE(h, a.mmae, "beats need mmae");
    RG_REQUIRE(h, a.t_margin >= 0 && a.order >= 1 && a.dt > 0.f && a.dt2 > 0.f, "bad beat parameters");
  }
  if (a.mpjpe_sum) RG_REQUIRE(h, a.retr_off && a.retr_joints && a.retr_poses && a.joint_mask, "MPJPE needs the retrieval buffers");
  hipLaunchKernelGGL(joint_stats_kernel, dim3(a.n_clips), dim3(ST_THREADS), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_pair_distance_sums(rg_handle* h, const rg_pair_dist_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_pair_dist_args& a = *args_host;
  RG_REQUIRE(h, a.x && a.group_off && a.group_off_host && a.partial && a.out, "null pointer");
  RG_REQUIRE(h, a.n_groups >= 1 && a.n_groups <= 65535 && a.dim >= 1, "need 1 <= n_groups <= 65535 and at least one column");
  RG_REQUIRE(h, a.group_off_host[0] == 0, "group_off must start at 0");
  int max_rows = 0;
  for (int g = 0; g < a.n_groups; ++g) {
    const int ng = a.group_off_host[g + 1] - a.group_off_host[g];
    RG_REQUIRE(h, ng >= 0, "group_off must not decrease");
    max_rows = max(max_rows, ng);
  }
  const int tiles = max(1, (max_rows + PD_TILE - 1) / PD_TILE);
  RG_REQUIRE(h, tiles <= 65535, "too many rows in one group");
  RG_REQUIRE(h, a.partial_len >= (int64_t)a.n_groups * tiles * tiles, "partial holds fewer than n_groups * tiles^2 doubles");
  hipLaunchKernelGGL(pair_dist_tile_kernel, dim3(tiles, tiles, a.n_groups), dim3(256), 0, rg_stream(stream), a, tiles);
  RG_CHECK_LAUNCH(h);
  hipLaunchKernelGGL(pair_dist_reduce_kernel, dim3(a.n_groups), dim3(256), 0, rg_stream(stream), a, tiles);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_srgr_clip_sums(rg_handle* h, const rg_srgr_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_srgr_args& a = *args_host;
  RG_REQUIRE(h, a.pred && a.gt && a.weights && a.clip_off && a.clip_off_host && a.wsum && a.count, "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1, "need at least one clip");
  RG_REQUIRE(h, a.n_joints >= 1 && a.threshold == a.threshold, "need n_joints >= 1 and a threshold that is a number");
  const char* bad = bad_clip_off(a.clip_off_host, a.n_clips);
  RG_REQUIRE(h, !bad, bad);
  hipLaunchKernelGGL(srgr_kernel, dim3(a.n_clips), dim3(ST_THREADS), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
