// The SMPL-X forward kinematics that rg_motion.hip (smplx_fk_kernel), rg_clip.hip (joints_expr_kernel) and rg_mesh.hip
// (mesh_transforms_kernel) run: one wave per frame, one lane per joint.  A lane builds its local transform
// [R_j | J_j - J_parent(j)], R_j = batch_rodrigues(fold(pose_j) + pose_mean_j) with its +1e-8 inside the norm (lbs.py), then
// the chain G_j = G_parent(j) . [R_j | J_j - J_parent(j)] is walked level by level of the tree depth through LDS.  A kernel
// keeps its own index arithmetic and its own epilogue; the arithmetic in between is stated here once, so the three cannot
// drift apart (tests/test_smplx_fk_gpu.py compares their joints bit for bit).  Also the host-side checks of the tables these
// entry points share.  Not for rg_common.h: that header is part of every unit.
#pragma once
#include "rg_common.h"

namespace {

constexpr int NJ = 55;                 // SMPL-X joints
constexpr int POSE_DIM = NJ * 3;
constexpr int NEXPR = 100;             // expression coefficients
constexpr int FK_THREADS = 256;        // 4 waves = 4 frames
constexpr float RG_PI = 3.14159265358979323846f;

// the clip of frame f: clip_off[lo] <= f < clip_off[lo + 1] (an empty clip is never chosen)
__device__ __forceinline__ int clip_of(const int* clip_off, int n_clips, int f) {
  int lo = 0, hi = n_clips;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (clip_off[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// a lane's place in the tree: its parent (-1: the root, and the lanes past the joints), its depth, and the deepest level
struct fk_tree {
  int par, depth, max_depth;
};
__device__ __forceinline__ fk_tree fk_tree_of(const int* parents, int lane) {
  fk_tree tr = {-1, 0, 0};
  if (lane < NJ) {
    tr.par = parents[lane];
    for (int p = tr.par; p >= 0 && tr.depth < NJ; p = parents[p]) ++tr.depth;
  }
  tr.max_depth = tr.depth;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) tr.max_depth = max(tr.max_depth, __shfl_xor(tr.max_depth, m));   // the same in every wave
  return tr;
}

// the rest joint J_j = rest[j] (+ j_expr[j] . psi when the frame has expression coefficients), rest = the clip's [55][3]
__device__ __forceinline__ void fk_rest_joint(const float* rest, const float* j_expr, const float* psi, int j, float J[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    float s = rest[j * 3 + d];
    if (psi) {
      const float* e = j_expr + ((size_t)j * 3 + d) * NEXPR;
      for (int k = 0; k < NEXPR; ++k) s = fmaf(e[k], psi[k], s);
    }
    J[d] = s;
  }
}

// the bone t = J - J_parent (the root: J), the parent's J from its lane: every lane of the wave calls this
__device__ __forceinline__ void fk_bone(const float J[3], int par, float t[3]) {
  const int pj = par >= 0 ? par : 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float jp = __shfl(J[d], pj);
    t[d] = par >= 0 ? J[d] - jp : J[d];
  }
}

// R = batch_rodrigues(fold(pv) + pose_mean): pv the joint's axis-angle, pose_mean its three values or nullptr
__device__ __forceinline__ void fk_rotation(const float* pv, const float* pose_mean, int fold, float R[9]) {
  float vx = pv[0], vy = pv[1], vz = pv[2];
  if (fold) {                                        // aa -> matrix -> 6D -> matrix -> aa (evaluate.py:261-280): angle into [0, pi]
    const float th = sqrtf(vx * vx + vy * vy + vz * vz);
    if (th > 0.f) {
      const float ph = fmodf(th, 2.f * RG_PI);
      const float s = (ph > RG_PI ? ph - 2.f * RG_PI : ph) / th;
      vx *= s, vy *= s, vz *= s;
    }
  }
  if (pose_mean) vx += pose_mean[0], vy += pose_mean[1], vz += pose_mean[2];   // SMPLX.forward: full_pose += pose_mean
  const float ex = vx + 1e-8f, ey = vy + 1e-8f, ez = vz + 1e-8f;
  const float ang = sqrtf(ex * ex + ey * ey + ez * ez);
  const float rx = vx / ang, ry = vy / ang, rz = vz / ang;
  const float c = cosf(ang), s = sinf(ang), oc = 1.f - c;
  // K = [[0, -rz, ry], [rz, 0, -rx], [-ry, rx, 0]];  R = I + sin K + (1 - cos) K^2
  const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float kk = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
      R[3 * i + j] = (i == j ? 1.f : 0.f) + s * K[3 * i + j] + oc * kk;
    }
}

// the chain walk through the wave's block g[55][12] (the row-major 3 x 4 global transform of every joint): level by level a
// live lane stores G_j = G_parent . [R | t] in g[lane]; every thread of the workgroup calls this (it holds the barriers)
__device__ __forceinline__ void fk_chain(float (*g)[12], const fk_tree& tr, bool live, int lane, const float R[9], const float t[3]) {
  for (int level = 0; level <= tr.max_depth; ++level) {
    if (live && tr.depth == level) {
      float out[12];
      if (tr.par < 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          out[4 * i] = R[3 * i], out[4 * i + 1] = R[3 * i + 1], out[4 * i + 2] = R[3 * i + 2], out[4 * i + 3] = t[i];
        }
      } else {
        const float* P = g[tr.par];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j)
            out[4 * i + j] = fmaf(P[4 * i + 2], R[6 + j], fmaf(P[4 * i + 1], R[3 + j], P[4 * i] * R[j]));
          out[4 * i + 3] = fmaf(P[4 * i + 2], t[2], fmaf(P[4 * i + 1], t[1], fmaf(P[4 * i], t[0], P[4 * i + 3])));
        }
      }
#pragma unroll
      for (int k = 0; k < 12; ++k) g[lane][k] = out[k];
    }
    __syncthreads();
  }
}

// the kinematic tree on the host: nullptr when joint 0 is the root and every other joint follows its parent, else what is wrong
inline const char* bad_parents(const int* parents) {
  if (parents[0] >= 0) return "joint 0 must be the root (parent < 0)";
  for (int j = 1; j < NJ; ++j)
    if (parents[j] < 0 || parents[j] >= j) return "parents[j] must lie in [0, j)";
  return nullptr;
}

// a clip_off table of n_clips + 1 entries on the host: nullptr when it starts at 0 and does not decrease, else what is wrong
inline const char* bad_clip_off(const int* clip_off, int n_clips) {
  if (clip_off[0] != 0) return "clip_off must start at 0";
  for (int c = 0; c < n_clips; ++c)
    if (clip_off[c + 1] < clip_off[c]) return "clip_off must not decrease";
  return nullptr;
}

// what the foot entry points (rg_foot.hip, rg_footlock.hip) refuse about their clip table; nullptr when it holds
inline const char* bad_foot_clips(const int* clip_off, int n_clips) {
  const char* bad = bad_clip_off(clip_off, n_clips);
  if (bad) return bad;
  for (int c = 0; c < n_clips; ++c)
    if (clip_off[c + 1] == clip_off[c]) return "an empty clip (every clip needs at least one frame)";
  if (clip_off[n_clips] >= 2147483647 / POSE_DIM) return "too many frames in one call";   // (as SMPLXJoints.joints)
  return nullptr;
}

}  // namespace
