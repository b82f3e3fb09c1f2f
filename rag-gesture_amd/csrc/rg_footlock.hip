// Contact ankles locked by analytic leg IK (include/rg_gesture.h; this project's own: the reference has no
// counterpart).
//   rg_foot_lock_targets : per frame and ankle the offset d that takes the ankle to its run's anchor (the mean position over the
//                          run of flagged frames), blended to zero outside the runs; per clip RG_FOOT_LOCK_STATS numbers
//   rg_foot_lock_ik      : hip, knee and ankle rotations re-solved so that the ankle reaches p + d; everything else copied
// The targets walk a clip's frames in tiles of LOCK_THREADS, one workgroup per clip, first forward, then backward: a clip's
// result depends on that clip alone.  Arithmetic in fp64 on the fp32 inputs, every product and sum rounded on its own (no FMA
// contraction), as tests/foot_lock_ref.py restates it.  The IK runs the shared forward kinematics of rg_smplx.h in fp32 (the
// positions are the bits rg_smplx_joints_expr stores) and solves a leg per lane in fp64.  Both are latency-bound.
#include "rg_reduce.h"
#include "rg_smplx.h"
#include "rg_legik.h"

#pragma clang fp contract(off)

namespace {

constexpr int LOCK_THREADS = 256;
constexpr int LOCK_WAVES = LOCK_THREADS / 64;
constexpr int N_LEG = 2;
constexpr int N_FLAG = 4;                               // contact [F][4]: the ankles' flags are columns 0 and 1
constexpr int NO_RUN = 2147483647;

// ---------------------------------------------------------------------------------------------------------------- targets
// an element of a segmented sum: f set = the sum starts again here
struct seg3 {
  double x, y, z;
  int c, f;
};
__device__ __forceinline__ seg3 seg_join(const seg3& a, const seg3& b) {      // b behind a
  seg3 r = b;
  if (!b.f) r.x = a.x + b.x, r.y = a.y + b.y, r.z = a.z + b.z, r.c = a.c + b.c;
  r.f = a.f | b.f;
  return r;
}

// inclusive segmented sum over the workgroup in thread order, continued from `carry` (the earlier tiles): inside a wave by
// shuffles, across the waves in order through LDS.  Every thread calls this (two barriers, the first in front of the store).
__device__ __forceinline__ seg3 seg_scan(seg3 v, seg3& carry, seg3* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const seg3 o = {__shfl_up(v.x, d), __shfl_up(v.y, d), __shfl_up(v.z, d), __shfl_up(v.c, d), __shfl_up(v.f, d)};
    if (lane >= d) v = seg_join(o, v);
  }
  __syncthreads();
  if (lane == 63) tot[wave] = v;
  __syncthreads();
  seg3 pre = carry;
  for (int w = 0; w < LOCK_WAVES; ++w) {
    if (w == wave) v = seg_join(pre, v);
    pre = seg_join(pre, tot[w]);
  }
  carry = pre;
  return v;
}

// inclusive running maximum over the workgroup in thread order, continued from `carry`; the same structure
__device__ __forceinline__ int max_scan(int v, int& carry, int* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v = max(o, v);
  }
  __syncthreads();
  if (lane == 63) tot[wave] = v;
  __syncthreads();
  int pre = carry;
  for (int w = 0; w < LOCK_WAVES; ++w) {
    if (w == wave) v = max(pre, v);
    pre = max(pre, tot[w]);
  }
  carry = pre;
  return v;
}

// frame t of a clip of n frames is a member frame of ankle k: the flag of pair (t, t + 1) or of pair (t - 1, t) is set
__device__ __forceinline__ bool lock_member(const float* C, int t, int n, int k, double cthr) {
  if (t < 0 || t >= n) return false;
  return (t <= n - 2 && (double)C[(size_t)t * N_FLAG + k] >= cthr) || (t >= 1 && (double)C[(size_t)(t - 1) * N_FLAG + k] >= cthr);
}

__device__ __forceinline__ void ankle_load(const float* J, int t, int k, double p[3]) {
  const float* q = J + ((size_t)t * NJ + 7 + k) * 3;
  p[0] = (double)q[0], p[1] = (double)q[1], p[2] = (double)q[2];
}

__device__ __forceinline__ double blend_weight(int k, int blend) {
  const double w = 1.0 - (double)k / ((double)blend + 1.0);
  return w > 0.0 ? w : 0.0;
}

// One workgroup per clip.  Forward walk: a thread owns frame base + threadIdx.x; the segmented sum of the member frames'
// positions and their count give, at a run's last frame, the run's anchor; a member frame stores sum / count in its slot of
// `off`, any other frame the index of the last member frame before it (-1: none).  Backward walk: a thread owns frame
// base + 255 - threadIdx.x, so the same scans run from the clip's end: the anchor travels from a run's last frame to its
// others, and the first member frame behind a frame is a running maximum of -t.  Member frames store d = A - p first; behind a
// barrier the other frames read d of the run ends on either side (a run end in a tile not walked yet still holds its anchor:
// d is formed from it with the same subtraction) and store their blend.
__global__ void __launch_bounds__(LOCK_THREADS) foot_lock_targets_kernel(const float* joints, const float* contact, const int* clip_off,
                                                                         float cthr_, int blend, double* offsets, double* stats) {
  __shared__ seg3 tot[LOCK_WAVES];
  __shared__ int toti[LOCK_WAVES];
  __shared__ double red[LOCK_WAVES];
  const int cidx = blockIdx.x;
  const int r0 = clip_off[cidx], n = clip_off[cidx + 1] - r0;
  const float* J = joints + (size_t)r0 * POSE_DIM;
  const float* C = contact + (size_t)r0 * N_FLAG;
  double* off = offsets + (size_t)r0 * N_LEG * 3;
  const double cthr = cthr_;
  const int tiles = (n + LOCK_THREADS - 1) / LOCK_THREADS;

  {
    seg3 carry[N_LEG];
    int last[N_LEG];
#pragma unroll
    for (int k = 0; k < N_LEG; ++k) carry[k] = {0.0, 0.0, 0.0, 0, 0}, last[k] = -1;
    for (int tile = 0; tile < tiles; ++tile) {
      const int t = tile * LOCK_THREADS + threadIdx.x;
#pragma unroll
      for (int k = 0; k < N_LEG; ++k) {
        const bool m = lock_member(C, t, n, k, cthr);
        double p[3] = {0.0, 0.0, 0.0};
        if (m) ankle_load(J, t, k, p);
        seg3 v = {p[0], p[1], p[2], m ? 1 : 0, m ? 0 : 1};
        v = seg_scan(v, carry[k], tot);
        const int e = max_scan(m ? t : -1, last[k], toti);
        if (t < n) {
          double* o = off + ((size_t)t * N_LEG + k) * 3;
          if (m) {
            const double cnt = (double)v.c;
            o[0] = v.x / cnt, o[1] = v.y / cnt, o[2] = v.z / cnt;
          } else {
            o[0] = (double)e, o[1] = 0.0, o[2] = 0.0;
          }
        }
      }
    }
  }
  __syncthreads();                                     // (the forward walk's stores are read by other threads below)

  double n_member = 0.0, n_runs = 0.0, n_moved = 0.0, sum_d = 0.0, max_d = 0.0;
  seg3 carry[N_LEG];
  int next[N_LEG];
#pragma unroll
  for (int k = 0; k < N_LEG; ++k) carry[k] = {0.0, 0.0, 0.0, 0, 0}, next[k] = -NO_RUN;
  for (int tile = tiles - 1; tile >= 0; --tile) {
    const int base = tile * LOCK_THREADS;
    const int t = base + (LOCK_THREADS - 1 - (int)threadIdx.x);
    bool member[N_LEG];
    int prev_end[N_LEG], next_start[N_LEG];
#pragma unroll
    for (int k = 0; k < N_LEG; ++k) {
      const bool m = lock_member(C, t, n, k, cthr);
      const bool is_end = m && !lock_member(C, t + 1, n, k, cthr);
      double* o = off + ((size_t)t * N_LEG + k) * 3;
      double own[3] = {0.0, 0.0, 0.0};
      if (t < n) own[0] = o[0], own[1] = o[1], own[2] = o[2];
      seg3 v = {is_end ? own[0] : 0.0, is_end ? own[1] : 0.0, is_end ? own[2] : 0.0, 0, is_end ? 1 : 0};
      v = seg_scan(v, carry[k], tot);                  // a member frame: its run's anchor
      const int ns = max_scan(m ? -t : -NO_RUN, next[k], toti);
      member[k] = m;
      prev_end[k] = m ? -1 : (int)own[0];
      next_start[k] = ns == -NO_RUN ? -1 : -ns;
      if (m) {
        double p[3];
        ankle_load(J, t, k, p);
        const double dx = v.x - p[0], dy = v.y - p[1], dz = v.z - p[2];
        o[0] = dx, o[1] = dy, o[2] = dz;
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        n_member += 1.0;
        if (!lock_member(C, t - 1, n, k, cthr)) n_runs += 1.0;
        if (dx != 0.0 || dy != 0.0 || dz != 0.0) n_moved += 1.0;
        sum_d += len;
        max_d = fmax(max_d, len);
      }
    }
    __syncthreads();                                   // (this tile's member frames hold their d)
    if (t < n) {
#pragma unroll
      for (int k = 0; k < N_LEG; ++k) {
        if (member[k]) continue;
        double d1[3] = {0.0, 0.0, 0.0}, d2[3] = {0.0, 0.0, 0.0}, w1 = 0.0, w2 = 0.0;
        const int e = prev_end[k], s = next_start[k];
        if (e >= 0) w1 = blend_weight(t - e, blend);
        if (s >= 0) w2 = blend_weight(s - t, blend);
        if (w1 > 0.0) {
          const double* q = off + ((size_t)e * N_LEG + k) * 3;
          d1[0] = q[0], d1[1] = q[1], d1[2] = q[2];
          if (e < base) {                              // still the anchor of the run that ends at e
            double p[3];
            ankle_load(J, e, k, p);
            d1[0] -= p[0], d1[1] -= p[1], d1[2] -= p[2];
          }
        }
        if (w2 > 0.0) {
          const double* q = off + ((size_t)s * N_LEG + k) * 3;
          d2[0] = q[0], d2[1] = q[1], d2[2] = q[2];
        }
        const double den = fmax(1.0, w1 + w2);
        double* o = off + ((size_t)t * N_LEG + k) * 3;
        bool moved = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double d = (w1 * d1[i] + w2 * d2[i]) / den;
          o[i] = d;
          moved = moved || d != 0.0;
        }
        if (moved) n_moved += 1.0;
      }
    }
  }
  // the counts are exact in any order; the sum of |d|: a thread's frames from the clip's end, the lanes by xor butterfly, the
  // waves 0 to 3
  n_member = block_sum_f64(n_member, red);
  n_runs = block_sum_f64(n_runs, red);
  n_moved = block_sum_f64(n_moved, red);
  sum_d = block_sum_f64(sum_d, red);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) max_d = fmax(max_d, __shfl_xor(max_d, s));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = max_d;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < LOCK_WAVES; ++w) max_d = fmax(max_d, red[w]);
    double* o = stats + (size_t)cidx * RG_FOOT_LOCK_STATS;
    o[0] = n_member, o[1] = n_runs, o[2] = n_moved, o[3] = sum_d, o[4] = max_d;
  }
}

// --------------------------------------------------------------------------------------------------------------------- IK
__device__ __forceinline__ m3 world_rotation(const float* G) {
  return {{(double)G[0], (double)G[1], (double)G[2], (double)G[4], (double)G[5], (double)G[6], (double)G[8], (double)G[9], (double)G[10]}};
}

// the two-bone solve of one leg (rg_legik.h): g the frame's global transforms, tr the frame's translation, d the ankle's
// offset -> the nine new channels (hip, knee, ankle; pose_mean taken off) and |T - a| / (l1 + l2)
__device__ __forceinline__ double leg_channels(const float (*g)[12], const int* parents, const float* pose_mean, const float tr[3], int k,
                                               const double d[3], double stretch, float out[9]) {
  const int hip = 1 + k, knee = 4 + k, ankle = 7 + k;
  const auto pos = [&](int j) -> v3 { return {(double)(g[j][3] + tr[0]), (double)(g[j][7] + tr[1]), (double)(g[j][11] + tr[2])}; };
  const v3 c = pos(ankle);
  double aa[9];
  const double reach = leg_solve(world_rotation(g[parents[hip]]), world_rotation(g[hip]), world_rotation(g[knee]), world_rotation(g[ankle]),
                                 pos(hip), pos(knee), c, {c.x + d[0], c.y + d[1], c.z + d[2]}, stretch, aa);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int ch = 3 * (hip + 3 * i) + q;
      out[3 * i + q] = (float)(pose_mean ? aa[3 * i + q] - (double)pose_mean[ch] : aa[3 * i + q]);
    }
  return reach;
}

// one wave per frame, one lane per joint for the forward kinematics of rg_smplx.h and for the copy of the frame's channels;
// lanes 0 and 1 then solve the left and the right leg.  A lane reads its channels before anything is stored, so poses_out may
// be poses.  (Frames past the end compute frame 0's values and write nothing.)
__global__ void __launch_bounds__(FK_THREADS) foot_lock_ik_kernel(const float* poses, const float* transl, const float* rest,
                                                                  const float* pose_mean, const int* parents, const int* clip_off,
                                                                  int n_clips, const double* offsets, float stretch_, float* poses_out,
                                                                  float* reach, int total) {
  __shared__ float g[FK_THREADS / 64][NJ][12];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * (FK_THREADS / 64) + wave;
  const int jl = lane < NJ ? lane : 0, ff = f < total ? f : 0;
  const bool live = f < total && lane < NJ;
  const fk_tree tr = fk_tree_of(parents, lane);
  const int c = clip_of(clip_off, n_clips, ff);
  const float* src = poses + (size_t)ff * POSE_DIM + 3 * jl;
  const float pv[3] = {src[0], src[1], src[2]};
  double d[N_LEG][3];
  bool need[N_LEG];
#pragma unroll
  for (int k = 0; k < N_LEG; ++k) {
    const double* q = offsets + ((size_t)ff * N_LEG + k) * 3;
    d[k][0] = q[0], d[k][1] = q[1], d[k][2] = q[2];
    need[k] = d[k][0] != 0.0 || d[k][1] != 0.0 || d[k][2] != 0.0;
  }
  float J[3], t[3], R[9];
  fk_rest_joint(rest + (size_t)c * NJ * 3, nullptr, nullptr, jl, J);
  fk_bone(J, tr.par, t);
  fk_rotation(pv, pose_mean ? pose_mean + 3 * jl : nullptr, 0, R);
  fk_chain(g[wave], tr, live, lane, R, t);
  if (!live) return;
  const int leg = (lane == 1 || lane == 4 || lane == 7) ? 0 : (lane == 2 || lane == 5 || lane == 8) ? 1 : -1;
  if (leg < 0 || !need[leg]) {
    float* o = poses_out + (size_t)f * POSE_DIM + 3 * lane;
    o[0] = pv[0], o[1] = pv[1], o[2] = pv[2];
  }
  if (lane < N_LEG) {
    float r = 0.f;
    if (need[lane]) {
      const float trn[3] = {transl[(size_t)f * 3], transl[(size_t)f * 3 + 1], transl[(size_t)f * 3 + 2]};
      float out[9];
      r = (float)leg_channels(g[wave], parents, pose_mean, trn, lane, d[lane], (double)stretch_, out);
      float* o = poses_out + (size_t)f * POSE_DIM;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int q = 0; q < 3; ++q) o[3 * (1 + lane + 3 * i) + q] = out[3 * i + q];
    }
    reach[(size_t)f * N_LEG + lane] = r;
  }
}

// the legs the solve assumes: hip, knee, ankle = (1, 4, 7) and (2, 5, 8) hang on each other
const char* bad_legs(const int* parents) {
  for (int k = 0; k < N_LEG; ++k)
    if (parents[4 + k] != 1 + k || parents[7 + k] != 4 + k) return "the legs must be the chains 1-4-7 and 2-5-8 (parents[4], [5], [7], [8])";
  return nullptr;
}

}  // namespace

extern "C" int rg_foot_lock_targets(rg_handle* h, const float* joints, const float* contact, const int* clip_off,
                                    const int* clip_off_host, int n_clips, float contact_thr, int blend, double* offsets,
                                    double* stats, void* stream) {
  RG_REQUIRE(h, joints && contact && clip_off && clip_off_host && offsets && stats, "null pointer");
  RG_REQUIRE(h, n_clips >= 1, "need at least one clip");
  const char* bad = bad_foot_clips(clip_off_host, n_clips);
  RG_REQUIRE(h, !bad, bad);
  RG_REQUIRE(h, contact_thr == contact_thr, "the threshold contact_thr must be a number");
  RG_REQUIRE(h, blend >= 0, "blend must not be negative");
  hipLaunchKernelGGL(foot_lock_targets_kernel, dim3(n_clips), dim3(LOCK_THREADS), 0, rg_stream(stream), joints, contact, clip_off,
                     contact_thr, blend, offsets, stats);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_foot_lock_ik(rg_handle* h, const float* poses, const float* transl, const float* rest, const float* pose_mean,
                               const int* parents, const int* parents_host, const int* clip_off, const int* clip_off_host,
                               int n_clips, const double* offsets, float stretch, float* poses_out, float* reach, void* stream) {
  RG_REQUIRE(h, poses && transl && rest && parents && parents_host && clip_off && clip_off_host && offsets && poses_out && reach,
             "null pointer");
  RG_REQUIRE(h, n_clips >= 1, "need at least one clip");
  const char* bad = bad_foot_clips(clip_off_host, n_clips);
  RG_REQUIRE(h, !bad, bad);
  bad = bad_parents(parents_host);
  RG_REQUIRE(h, !bad, bad);
  bad = bad_legs(parents_host);
  RG_REQUIRE(h, !bad, bad);
  RG_REQUIRE(h, stretch > 0.f && stretch <= 1.f, "stretch must lie in (0, 1]");
  const int total = clip_off_host[n_clips];
  const int fpb = FK_THREADS / 64;
  hipLaunchKernelGGL(foot_lock_ik_kernel, dim3((total + fpb - 1) / fpb), dim3(FK_THREADS), 0, rg_stream(stream), poses, transl, rest,
                     pose_mean, parents, clip_off, n_clips, offsets, stretch, poses_out, reach, total);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
