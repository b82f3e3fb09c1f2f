// Raw SMPL-X recordings -> model inputs (mogen/datasets/beatx_dataset.py, motion side).
//   rg_smplx_joints_expr : the 55 posed joints with expression and translation (:373-415, :206-272), one wave per frame
//   rg_clip_prepare      : strided motion / trans / facial, the four body-part gathers and the foot contacts (:354-440)
//   rg_joint_speed_sums  : per clip and joint, the sum over frames of the velocity norm (:272-288 calculate_mean_velocity)
// Several recordings share a launch as concatenated rows; clip c reads raw rows raw_off[c] + t * stride (include/rg_gesture.h).
#include "rg_common.h"

namespace {

constexpr int NJ = 55;                 // SMPL-X joints
constexpr int POSE_DIM = NJ * 3;
constexpr int NEXPR = 100;
constexpr int FK_THREADS = 256;        // 4 waves = 4 frames
constexpr int PREP_THREADS = 256;
constexpr int SP_THREADS = 256;
constexpr int N_UPPER = 39, N_LOWER = 27, N_HANDS = 90, N_FACE = 3;
constexpr int N_PART_COLS = N_UPPER + N_LOWER + N_HANDS + N_FACE;            // 159
constexpr int N_CONTACT = 4;
constexpr int ROW_OUT = POSE_DIM + 3 + NEXPR + N_PART_COLS + N_CONTACT;      // 431 values written per frame
constexpr float RG_PI = 3.14159265358979323846f;

// the clip of output frame f: clip_off[lo] <= f < clip_off[lo + 1] (an empty clip is never chosen)
__device__ __forceinline__ int clip_of(const int* clip_off, int n_clips, int f) {
  int lo = 0, hi = n_clips;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (clip_off[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// one wave per output frame, one lane per joint (the arithmetic of smplx_fk_kernel in rg_motion.hip and of
// mesh_transforms_kernel in rg_mesh.hip): J_j = rest[j] + j_expr[j] . psi, R_j = batch_rodrigues(fold(pose_j) + pose_mean_j)
// with its +1e-8 inside the norm, the chain G_j = G_parent(j) . [R_j | J_j - J_parent(j)] level by level through LDS, then
// joint = G_j[:3, 3] + transl.
__global__ void __launch_bounds__(FK_THREADS) joints_expr_kernel(rg_smplx_joints_expr_args a, int total) {
  __shared__ float g[FK_THREADS / 64][NJ][12];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * (FK_THREADS / 64) + wave;
  const int jl = lane < NJ ? lane : 0;
  const bool live = f < total && lane < NJ;
  int depth = 0, par = -1;
  if (lane < NJ) {
    par = a.parents[lane];
    for (int p = par; p >= 0 && depth < NJ; p = a.parents[p]) ++depth;
  }
  int max_depth = depth;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) max_depth = max(max_depth, __shfl_xor(max_depth, m));   // the same in every wave

  const int ff = f < total ? f : 0;                  // (frames past the end compute frame 0's values and write nothing)
  const int c = clip_of(a.clip_off, a.n_clips, ff);
  const size_t r = (size_t)a.raw_off[c] + (size_t)(ff - a.clip_off[c]) * (size_t)a.stride;
  const float* psi = a.exprs ? a.exprs + r * NEXPR : nullptr;
  float J[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    float s = a.rest[((size_t)c * NJ + jl) * 3 + d];
    if (psi) {
      const float* e = a.j_expr + ((size_t)jl * 3 + d) * NEXPR;
      for (int k = 0; k < NEXPR; ++k) s = fmaf(e[k], psi[k], s);
    }
    J[d] = s;
  }
  const int pj = par >= 0 ? par : 0;
  float t[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float jp = __shfl(J[d], pj);
    t[d] = par >= 0 ? J[d] - jp : J[d];
  }

  float R[9];
  {
    const float* pv = a.poses + r * POSE_DIM + 3 * jl;
    float vx = pv[0], vy = pv[1], vz = pv[2];
    if (a.fold) {                                    // aa -> 6D -> aa (evaluate.py:261-280): angle into [0, pi]
      const float th = sqrtf(vx * vx + vy * vy + vz * vz);
      if (th > 0.f) {
        const float ph = fmodf(th, 2.f * RG_PI);
        const float s = (ph > RG_PI ? ph - 2.f * RG_PI : ph) / th;
        vx *= s, vy *= s, vz *= s;
      }
    }
    if (a.pose_mean) vx += a.pose_mean[3 * jl], vy += a.pose_mean[3 * jl + 1], vz += a.pose_mean[3 * jl + 2];
    const float ex = vx + 1e-8f, ey = vy + 1e-8f, ez = vz + 1e-8f;
    const float ang = sqrtf(ex * ex + ey * ey + ez * ez);
    const float rx = vx / ang, ry = vy / ang, rz = vz / ang;
    const float cs = cosf(ang), sn = sinf(ang), oc = 1.f - cs;
    // K = [[0, -rz, ry], [rz, 0, -rx], [-ry, rx, 0]];  R = I + sin K + (1 - cos) K^2
    const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float kk = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
        R[3 * i + j] = (i == j ? 1.f : 0.f) + sn * K[3 * i + j] + oc * kk;
      }
  }
  float* mine = g[wave][jl];
  for (int level = 0; level <= max_depth; ++level) {
    if (live && depth == level) {
      float out[12];
      if (par < 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          out[4 * i] = R[3 * i], out[4 * i + 1] = R[3 * i + 1], out[4 * i + 2] = R[3 * i + 2], out[4 * i + 3] = t[i];
        }
      } else {
        const float* P = g[wave][par];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j)
            out[4 * i + j] = fmaf(P[4 * i + 2], R[6 + j], fmaf(P[4 * i + 1], R[3 + j], P[4 * i] * R[j]));
          out[4 * i + 3] = fmaf(P[4 * i + 2], t[2], fmaf(P[4 * i + 1], t[1], fmaf(P[4 * i], t[0], P[4 * i + 3])));
        }
      }
#pragma unroll
      for (int k = 0; k < 12; ++k) mine[k] = out[k];
    }
    __syncthreads();
  }
  if (live) {
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (a.transl) tx = a.transl[r * 3], ty = a.transl[r * 3 + 1], tz = a.transl[r * 3 + 2];
    float* o = a.joints + ((size_t)f * NJ + lane) * 3;
    o[0] = mine[3] + tx, o[1] = mine[7] + ty, o[2] = mine[11] + tz;
  }
}

// one workgroup per output frame; its threads stride over the 431 values the frame gets: copies of the raw row, the part
// gathers, and the four contact flags from the joints of this frame and the clip's next one
__global__ void __launch_bounds__(PREP_THREADS) clip_prepare_kernel(rg_clip_prepare_args a) {
  const int f = blockIdx.x;
  const int c = clip_of(a.clip_off, a.n_clips, f);
  const int t = f - a.clip_off[c], n = a.clip_off[c + 1] - a.clip_off[c];
  const size_t r = (size_t)a.raw_off[c] + (size_t)t * (size_t)a.stride;
  const float* pose = a.poses + r * POSE_DIM;
  for (int i = threadIdx.x; i < ROW_OUT; i += PREP_THREADS) {
    if (i < POSE_DIM) {
      a.motion[(size_t)f * POSE_DIM + i] = pose[i];
    } else if (i < POSE_DIM + 3) {
      const int k = i - POSE_DIM;
      a.trans_out[(size_t)f * 3 + k] = a.trans[r * 3 + k];
    } else if (i < POSE_DIM + 3 + NEXPR) {
      const int k = i - (POSE_DIM + 3);
      a.facial[(size_t)f * NEXPR + k] = a.exprs[r * NEXPR + k];
    } else if (i < POSE_DIM + 3 + NEXPR + N_PART_COLS) {
      const int k = i - (POSE_DIM + 3 + NEXPR);
      const float v = pose[a.part_cols[k]];
      if (k < N_UPPER) a.upper[(size_t)f * N_UPPER + k] = v;
      else if (k < N_UPPER + N_LOWER) a.lower[(size_t)f * N_LOWER + (k - N_UPPER)] = v;
      else if (k < N_UPPER + N_LOWER + N_HANDS) a.hands[(size_t)f * N_HANDS + (k - N_UPPER - N_LOWER)] = v;
      else a.face[(size_t)f * N_FACE + (k - N_UPPER - N_LOWER - N_HANDS)] = v;
    } else {
      const int q = i - (POSE_DIM + 3 + NEXPR + N_PART_COLS);
      const int j = q < 2 ? 7 + q : 8 + q;           // joints 7, 8, 10, 11 (beatx_dataset.py:396)
      float flag = 1.f;                              // feetv[last] = 0 < threshold (:417-420)
      if (t + 1 < n) {
        const float* p0 = a.joints + ((size_t)f * NJ + j) * 3;
        const float* p1 = p0 + POSE_DIM;
        const float dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
        const float feetv = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        flag = feetv < a.threshold ? 1.f : 0.f;
      }
      a.contact[(size_t)f * N_CONTACT + q] = flag;
    }
  }
}

// one workgroup per clip: lane = joint, the four waves take frames w, w + 4, ...; a lane's fp64 sum runs over its frames in
// order, the four wave sums meet in the order ((0 + 1) + 2) + 3
__global__ void __launch_bounds__(SP_THREADS) joint_speed_kernel(rg_joint_speed_args a) {
  __shared__ double part[SP_THREADS / 64][NJ];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = a.clip_off[c], n = a.clip_off[c + 1] - r0;
  const float* J = a.joints + (size_t)r0 * POSE_DIM;
  const float dt = a.dt, dt2 = 2.f * a.dt;
  if (lane < NJ) {
    double s = 0.0;
    for (int t = wave; t < n; t += SP_THREADS / 64) {
      int t1 = t + 1, t0 = t - 1;
      float sc = dt2;
      if (t == 0) t0 = 0, sc = dt;
      if (t == n - 1) t1 = n - 1, sc = dt;
      const float* p1 = J + ((size_t)t1 * NJ + lane) * 3;
      const float* p0 = J + ((size_t)t0 * NJ + lane) * 3;
      const float dx = (p1[0] - p0[0]) / sc, dy = (p1[1] - p0[1]) / sc, dz = (p1[2] - p0[2]) / sc;
      s += (double)sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    }
    part[wave][lane] = s;
  }
  __syncthreads();
  if (threadIdx.x < NJ)
    a.sums[(size_t)c * NJ + threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// clip_off / raw_off as include/rg_gesture.h states them; nullptr when they hold, else what is wrong
const char* check_tables(const int* clip_off, const int* raw_off, int n_clips, int raw_rows, int stride) {
  if (n_clips < 1) return "need at least one clip";
  if (stride < 1) return "stride must be at least 1";
  if (raw_rows < 0) return "raw_rows must not be negative";
  if (clip_off[0] != 0 || raw_off[0] != 0) return "clip_off and raw_off must start at 0";
  for (int c = 0; c < n_clips; ++c) {
    const long long n = (long long)clip_off[c + 1] - clip_off[c], m = (long long)raw_off[c + 1] - raw_off[c];
    if (n < 0 || m < 0) return "clip_off and raw_off must not decrease";
    if (n > 0 && m < (n - 1) * stride + 1) return "a clip owns fewer raw rows than (frames - 1) * stride + 1";
  }
  if (raw_off[n_clips] > raw_rows) return "raw_off ends beyond raw_rows";
  if (clip_off[n_clips] >= 2147483647 / POSE_DIM) return "too many frames in one call";   // (as SMPLXJoints.joints)
  return nullptr;
}

}  // namespace

extern "C" int rg_smplx_joints_expr(rg_handle* h, const rg_smplx_joints_expr_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_smplx_joints_expr_args& a = *args_host;
  RG_REQUIRE(h, a.poses && a.rest && a.parents && a.parents_host && a.clip_off && a.clip_off_host && a.raw_off && a.raw_off_host &&
                    a.joints, "null pointer");
  RG_REQUIRE(h, !a.exprs || a.j_expr, "expressions need j_expr");
  RG_REQUIRE(h, a.parents_host[0] < 0, "joint 0 must be the root (parent < 0)");
  for (int j = 1; j < NJ; ++j) RG_REQUIRE(h, a.parents_host[j] >= 0 && a.parents_host[j] < j, "parents[j] must lie in [0, j)");
  const char* bad = check_tables(a.clip_off_host, a.raw_off_host, a.n_clips, a.raw_rows, a.stride);
  RG_REQUIRE(h, !bad, bad);
  const int total = a.clip_off_host[a.n_clips];
  if (total == 0) return RG_OK;
  const int fpb = FK_THREADS / 64;
  hipLaunchKernelGGL(joints_expr_kernel, dim3((total + fpb - 1) / fpb), dim3(FK_THREADS), 0, rg_stream(stream), a, total);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_clip_prepare(rg_handle* h, const rg_clip_prepare_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_clip_prepare_args& a = *args_host;
  RG_REQUIRE(h, a.poses && a.trans && a.exprs && a.joints && a.part_cols && a.part_cols_host && a.clip_off && a.clip_off_host &&
                    a.raw_off && a.raw_off_host, "null pointer");
  RG_REQUIRE(h, a.motion && a.trans_out && a.facial && a.upper && a.lower && a.hands && a.face && a.contact, "null output pointer");
  RG_REQUIRE(h, a.threshold == a.threshold, "the contact threshold must be a number");
  for (int k = 0; k < N_PART_COLS; ++k)
    RG_REQUIRE(h, a.part_cols_host[k] >= 0 && a.part_cols_host[k] < POSE_DIM, "part_cols must lie in [0, 165)");
  const char* bad = check_tables(a.clip_off_host, a.raw_off_host, a.n_clips, a.raw_rows, a.stride);
  RG_REQUIRE(h, !bad, bad);
  const int total = a.clip_off_host[a.n_clips];
  if (total == 0) return RG_OK;
  hipLaunchKernelGGL(clip_prepare_kernel, dim3(total), dim3(PREP_THREADS), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_joint_speed_sums(rg_handle* h, const rg_joint_speed_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_joint_speed_args& a = *args_host;
  RG_REQUIRE(h, a.joints && a.clip_off && a.clip_off_host && a.sums, "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1, "need at least one clip");
  RG_REQUIRE(h, a.dt > 0.f, "dt must be positive");
  RG_REQUIRE(h, a.clip_off_host[0] == 0, "clip_off must start at 0");
  for (int c = 0; c < a.n_clips; ++c) RG_REQUIRE(h, a.clip_off_host[c + 1] - a.clip_off_host[c] >= 2, "every clip needs >= 2 frames");
  hipLaunchKernelGGL(joint_speed_kernel, dim3(a.n_clips), dim3(SP_THREADS), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
