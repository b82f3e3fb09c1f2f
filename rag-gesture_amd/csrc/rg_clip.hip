// Raw SMPL-X recordings -> model inputs (mogen/datasets/beatx_dataset.py, motion side).
//   rg_smplx_joints_expr : the 55 posed joints with expression and translation (:373-415, :206-272), one wave per frame
//   rg_clip_prepare      : strided motion / trans / facial, the four body-part gathers and the foot contacts (:354-440)
//   rg_joint_speed_sums  : per clip and joint, the sum over frames of the velocity norm (:272-288 calculate_mean_velocity)
// Several recordings share a launch as concatenated rows; clip c reads raw rows raw_off[c] + t * stride (include/rg_gesture.h).
#include "rg_smplx.h"

namespace {

constexpr int PREP_THREADS = 256;
constexpr int SP_THREADS = 256;
constexpr int N_UPPER = 39, N_LOWER = 27, N_HANDS = 90, N_FACE = 3;
constexpr int N_PART_COLS = N_UPPER + N_LOWER + N_HANDS + N_FACE;            // 159
constexpr int N_CONTACT = 4;
constexpr int ROW_OUT = POSE_DIM + 3 + NEXPR + N_PART_COLS + N_CONTACT;      // 431 values written per frame

// the forward kinematics of rg_smplx.h on raw row r of output frame f, the rest joints moved by the row's expression; stores
// joint = G_j[:3, 3] + transl.  (Frames past the end compute frame 0's values and write nothing.)
__global__ void __launch_bounds__(FK_THREADS) joints_expr_kernel(rg_smplx_joints_expr_args a, int total) {
  __shared__ float g[FK_THREADS / 64][NJ][12];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * (FK_THREADS / 64) + wave;
  const int jl = lane < NJ ? lane : 0, ff = f < total ? f : 0;
  const bool live = f < total && lane < NJ;
  const fk_tree tr = fk_tree_of(a.parents, lane);
  const int c = clip_of(a.clip_off, a.n_clips, ff);
  const size_t r = (size_t)a.raw_off[c] + (size_t)(ff - a.clip_off[c]) * (size_t)a.stride;
  float J[3], t[3], R[9];
  fk_rest_joint(a.rest + (size_t)c * NJ * 3, a.j_expr, a.exprs ? a.exprs + r * NEXPR : nullptr, jl, J);
  fk_bone(J, tr.par, t);
  fk_rotation(a.poses + r * POSE_DIM + 3 * jl, a.pose_mean ? a.pose_mean + 3 * jl : nullptr, a.fold, R);
  fk_chain(g[wave], tr, live, lane, R, t);
  if (live) {
    const float* mine = g[wave][lane];
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
  const char* bad = bad_parents(a.parents_host);
  RG_REQUIRE(h, !bad, bad);
  bad = check_tables(a.clip_off_host, a.raw_off_host, a.n_clips, a.raw_rows, a.stride);
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
