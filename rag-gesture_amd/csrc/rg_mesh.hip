// SMPL-X mesh vertices (smplx.lbs with expression and pose blend shapes) and the face metrics of tools/evaluate.py:328-367.
//   rg_mesh_transforms  : per row (frame) the coefficient row [psi | active pose features] and the skinning transforms
//                         A_j = [R_g | t_g - R_g J_j] of the 55 joints, one wave per row
//   rg_mesh_blend_skin  : coeff . basis on fp32-input MFMA (exact fp32), + the clip's base, then linear blend skinning from
//                         per-vertex sparse weight lists; out: raw rows, vertices, or per frame pair the face sums
//   rg_mesh_face_sums   : per clip, the fixed-order sum of the face partials (l2: every frame, lvel: frames 1..n-1)
#include "rg_reduce.h"
#include "rg_smplx.h"

namespace {

constexpr int MT = 64;                   // rows per tile (face mode: 32 frame pairs)
constexpr int VT = 64;                   // vertices per tile
constexpr int NT = 3 * VT;               // columns per tile
constexpr int KC = 16;                   // K per LDS stage
constexpr int BS_THREADS = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the forward kinematics of rg_smplx.h on row r, the rest joints j_clip moved by the row's expression; stores the row's
// coefficients [psi | R_j - I of the active joints], A_j = [R_g | t_g - R_g J_j] and optionally the joints.  (Rows past the
// end compute row 0's values and write nothing.)
__global__ void __launch_bounds__(FK_THREADS) mesh_transforms_kernel(rg_mesh_transforms_args a, int total) {
  __shared__ float g[FK_THREADS / 64][NJ][12];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * (FK_THREADS / 64) + wave;
  const int jl = lane < NJ ? lane : 0, rr = r < total ? r : 0;
  const bool live = r < total && lane < NJ;
  const fk_tree tr = fk_tree_of(a.parents, lane);
  const float* psi = a.exprs ? a.exprs + (size_t)rr * NEXPR : nullptr;
  float J[3], t[3], R[9];
  fk_rest_joint(a.j_clip + (size_t)clip_of(a.clip_off, a.n_clips, rr) * NJ * 3, a.j_expr, psi, jl, J);
  fk_bone(J, tr.par, t);
  fk_rotation(a.poses + (size_t)rr * POSE_DIM + 3 * jl, a.pose_mean ? a.pose_mean + 3 * jl : nullptr, a.fold, R);
  fk_chain(g[wave], tr, live, lane, R, t);
  if (r >= total) return;
  float* crow = a.coeff + (size_t)r * a.k_pad;
  for (int k = lane; k < NEXPR; k += 64) crow[k] = psi ? psi[k] : 0.f;
  if (!live) return;
  const float* mine = g[wave][lane];
  const int col = a.pf_col[lane];
  if (col >= 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) crow[col + i] = R[i] - ((i == 0 || i == 4 || i == 8) ? 1.f : 0.f);
  }
  float* A = a.A + ((size_t)r * NJ + lane) * 12;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    A[4 * i] = mine[4 * i], A[4 * i + 1] = mine[4 * i + 1], A[4 * i + 2] = mine[4 * i + 2];
    A[4 * i + 3] = mine[4 * i + 3] - fmaf(mine[4 * i + 2], J[2], fmaf(mine[4 * i + 1], J[1], mine[4 * i] * J[0]));
  }
  if (a.joints) {
    float* o = a.joints + ((size_t)r * NJ + lane) * 3;
    o[0] = mine[3], o[1] = mine[7], o[2] = mine[11];
  }
}

// T = sum_q w_q A_{j_q} over the vertex's nonzero weights (list order), vertex = T . [p; 1]
__device__ __forceinline__ void skin_vertex(const float* __restrict__ Arow, const int* __restrict__ sj, const float* __restrict__ sw,
                                            int n, float px, float py, float pz, float o[3]) {
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = 0.f;
  for (int q = 0; q < n; ++q) {
    const float w = sw[q];
    const float4* m = reinterpret_cast<const float4*>(Arow + 12 * sj[q]);
    const float4 m0 = m[0], m1 = m[1], m2 = m[2];
    T[0] = fmaf(w, m0.x, T[0]), T[1] = fmaf(w, m0.y, T[1]), T[2] = fmaf(w, m0.z, T[2]), T[3] = fmaf(w, m0.w, T[3]);
    T[4] = fmaf(w, m1.x, T[4]), T[5] = fmaf(w, m1.y, T[5]), T[6] = fmaf(w, m1.z, T[6]), T[7] = fmaf(w, m1.w, T[7]);
    T[8] = fmaf(w, m2.x, T[8]), T[9] = fmaf(w, m2.y, T[9]), T[10] = fmaf(w, m2.z, T[10]), T[11] = fmaf(w, m2.w, T[11]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = fmaf(T[4 * i + 2], pz, fmaf(T[4 * i + 1], py, fmaf(T[4 * i], px, T[4 * i + 3])));
}

// grid = (row tiles, groups).  A workgroup takes row tile blockIdx.x and the vertex tiles blockIdx.y, + gridDim.y, ... in
// order.  Per vertex tile: the [64 x 192] block of coeff . basis on v_mfma_f32_32x32x2_f32 (each wave 32 rows x 96 columns,
// K staged through LDS 16 at a time; an element is a k-ordered fp32 fma chain from 0 whatever the other rows of the tile), the
// block through LDS, + base, then per (row, vertex) one thread: RAW stores the row, VERTICES skins and stores the vertex,
// FACE skins both rows of a frame pair and sums (rec - tar)^2 and |rec - tar| over the tile's vertices in fp64 (lane order,
// then tile order).
__global__ void __launch_bounds__(BS_THREADS) mesh_blend_skin_kernel(rg_mesh_blend_args a, int n_vt) {
  constexpr int AS = KC + 1;                           // padded row of the staged coefficient tile
  constexpr int OS = NT + 1;                           // padded row of the result tile
  constexpr int SMEM = (MT * AS + KC * NT) > MT * OS ? (MT * AS + KC * NT) : MT * OS;
  __shared__ float smem[SMEM];
  __shared__ int row_base[MT];
  __shared__ double fsum[MT / 2][2];
  float* As = smem;
  float* Bs = smem + MT * AS;
  float* Out = smem;                                   // (aliases As / Bs: used after the K loop only)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * MT;
  const int m0 = 32 * (wave & 1), n0 = 96 * (wave >> 1);

  if (tid < MT) {
    int b = 0;
    const int r = min(r0 + tid, a.rows - 1);
    if (a.base_per_clip) b = clip_of(a.clip_off, a.n_clips, r);
    row_base[tid] = b;
  }
  if (tid < MT / 2) fsum[tid][0] = fsum[tid][1] = 0.0;

  for (int vt = blockIdx.y; vt < n_vt; vt += gridDim.y) {
    const int c0 = vt * NT;
    f32x16 acc[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[s][i] = 0.f;
    for (int k0 = 0; k0 < a.k_pad; k0 += KC) {
      __syncthreads();
      {
        const int r = tid >> 2, q = tid & 3;
        const float4 v = *reinterpret_cast<const float4*>(a.coeff + (size_t)(r0 + r) * a.k_pad + k0 + 4 * q);
        float* d = As + r * AS + 4 * q;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
      }
#pragma unroll
      for (int e = tid; e < KC * NT / 4; e += BS_THREADS) {
        const int k = e / (NT / 4), q = e - k * (NT / 4);
        *reinterpret_cast<float4*>(Bs + k * NT + 4 * q) =
            *reinterpret_cast<const float4*>(a.basis + (size_t)(k0 + k) * a.d_pad + c0 + 4 * q);
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < KC; kk += 2) {
        const int k = kk + (lane >> 5);
        const float av = As[(m0 + (lane & 31)) * AS + k];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const float bv = Bs[k * NT + n0 + 32 * s + (lane & 31)];
          acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[s], 0, 0, 0);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        Out[row * OS + n0 + 32 * s + (lane & 31)] = acc[s][i];
      }
    __syncthreads();

    if (a.mode == RG_MESH_RAW) {
      for (int e = tid; e < MT * NT; e += BS_THREADS) {
        const int r = e / NT, j = e - r * NT;
        if (r0 + r < a.rows)
          a.out[(size_t)(r0 + r) * a.d_pad + c0 + j] = Out[r * OS + j] + a.base[(size_t)row_base[r] * a.d_pad + c0 + j];
      }
      continue;
    }
    const int v = vt * VT + lane;
    const bool vlive = v < a.n_verts;
    const int nnz = vlive ? a.skin_n[v] : 0;
    const int* sj = a.skin_j + (size_t)(vlive ? v : 0) * a.max_nnz;
    const float* sw = a.skin_w + (size_t)(vlive ? v : 0) * a.max_nnz;
    if (a.mode == RG_MESH_VERTICES) {
      for (int r = wave; r < MT; r += 4) {
        const int row = r0 + r;
        if (row >= a.rows || !vlive) continue;
        const float* bp = a.base + (size_t)row_base[r] * a.d_pad + c0 + 3 * lane;
        const float* op = Out + r * OS + 3 * lane;
        float o[3];
        skin_vertex(a.A + (size_t)row * NJ * 12, sj, sw, nnz, op[0] + bp[0], op[1] + bp[1], op[2] + bp[2], o);
        float* dst = a.out + ((size_t)row * a.n_verts + v) * 3;
        const float* tr = a.transl ? a.transl + (size_t)row * 3 : nullptr;
        dst[0] = tr ? o[0] + tr[0] : o[0], dst[1] = tr ? o[1] + tr[1] : o[1], dst[2] = tr ? o[2] + tr[2] : o[2];
      }
    } else {                                           // RG_MESH_FACE: rows 2p (prediction) and 2p + 1 (ground truth)
      for (int p = wave; p < MT / 2; p += 4) {
        const int row = r0 + 2 * p;
        double s2 = 0.0, s1 = 0.0;
        if (row < a.rows && vlive) {
          const float* bp = a.base + (size_t)row_base[2 * p] * a.d_pad + c0 + 3 * lane;
          const float* op = Out + 2 * p * OS + 3 * lane;
          float rec[3], tar[3];
          skin_vertex(a.A + (size_t)row * NJ * 12, sj, sw, nnz, op[0] + bp[0], op[1] + bp[1], op[2] + bp[2], rec);
          op += OS;
          skin_vertex(a.A + (size_t)(row + 1) * NJ * 12, sj, sw, nnz, op[0] + bp[0], op[1] + bp[1], op[2] + bp[2], tar);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double d = (double)(rec[c] - tar[c]);
            s2 = fma(d, d, s2);
            s1 += fabs(d);
          }
        }
        s2 = wave_sum_f64(s2);
        s1 = wave_sum_f64(s1);
        if (lane == 0) fsum[p][0] += s2, fsum[p][1] += s1;
      }
    }
  }
  if (a.mode == RG_MESH_FACE) {
    __syncthreads();
    if (tid < MT / 2 && r0 + 2 * tid < a.rows) {
      double* d = a.partial + ((size_t)(r0 / 2 + tid) * gridDim.y + blockIdx.y) * 2;
      d[0] = fsum[tid][0], d[1] = fsum[tid][1];
    }
  }
}

// one workgroup per clip: l2 = sum over its frame pairs and groups of partial[.][.][0], lvel the same of [1] without frame 0
__global__ void __launch_bounds__(256) mesh_face_sums_kernel(rg_mesh_face_sums_args a) {
  __shared__ double red[4];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = a.pair_off[c], n = a.pair_off[c + 1] - p0;
  double s2 = 0.0, s1 = 0.0;
  for (int t = tid; t < n; t += 256) {
    const double* q = a.partial + (size_t)(p0 + t) * a.n_groups * 2;
    for (int g = 0; g < a.n_groups; ++g) {
      s2 += q[2 * g];
      if (t > 0) s1 += q[2 * g + 1];
    }
  }
  double out[2] = {s2, s1};
#pragma unroll
  for (int i = 0; i < 2; ++i) {                  // (block_sum_f64 starts from 0.0 and loops over blockDim.x / 64: other code)
    const double v = wave_sum_f64(out[i]);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    out[i] = ((red[0] + red[1]) + red[2]) + red[3];
  }
  if (tid == 0) a.sums[2 * c] = out[0], a.sums[2 * c + 1] = out[1];
}

}  // namespace

extern "C" int rg_mesh_transforms(rg_handle* h, const rg_mesh_transforms_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_mesh_transforms_args& a = *args_host;
  RG_REQUIRE(h, a.poses && a.j_clip && a.j_expr && a.parents && a.parents_host && a.clip_off && a.clip_off_host && a.pf_col &&
                a.pf_col_host && a.coeff && a.A, "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1, "need at least one clip");
  const char* bad = bad_parents(a.parents_host);
  RG_REQUIRE(h, !bad, bad);
  RG_REQUIRE(h, a.k_pad >= NEXPR && a.k_pad % KC == 0, "k_pad must be a multiple of 16 and hold the 100 expression columns");
  RG_REQUIRE(h, a.pf_col_host[0] < 0, "the root has no pose-feature columns");
  for (int j = 1; j < NJ; ++j)
    RG_REQUIRE(h, a.pf_col_host[j] < 0 || (a.pf_col_host[j] >= NEXPR && a.pf_col_host[j] + 9 <= a.k_pad), "pf_col out of range");
  bad = bad_clip_off(a.clip_off_host, a.n_clips);
  RG_REQUIRE(h, !bad, bad);
  const int total = a.clip_off_host[a.n_clips];
  if (total == 0) return RG_OK;
  const int rpb = FK_THREADS / 64;
  hipLaunchKernelGGL(mesh_transforms_kernel, dim3((total + rpb - 1) / rpb), dim3(FK_THREADS), 0, rg_stream(stream), a, total);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_mesh_blend_skin(rg_handle* h, const rg_mesh_blend_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_mesh_blend_args& a = *args_host;
  RG_REQUIRE(h, a.coeff && a.basis && a.base, "null pointer");
  RG_REQUIRE(h, a.mode == RG_MESH_RAW || a.mode == RG_MESH_VERTICES || a.mode == RG_MESH_FACE, "unknown mode");
  RG_REQUIRE(h, a.rows >= 1 && a.k_pad >= KC && a.k_pad % KC == 0, "need rows >= 1 and k_pad a positive multiple of 16");
  RG_REQUIRE(h, a.coeff_rows >= (a.rows + MT - 1) / MT * MT, "coeff must hold rows rounded up to a multiple of 64");
  RG_REQUIRE(h, a.n_verts >= 1 && a.d_pad == (a.n_verts + VT - 1) / VT * NT, "d_pad must be 3 * n_verts rounded up to 192");
  if (a.base_per_clip) {
    RG_REQUIRE(h, a.clip_off && a.clip_off_host && a.n_clips >= 1, "a base per clip needs clip_off");
    RG_REQUIRE(h, a.clip_off_host[0] == 0 && a.clip_off_host[a.n_clips] == a.rows, "clip_off must run from 0 to rows");
    for (int c = 0; c < a.n_clips; ++c) RG_REQUIRE(h, a.clip_off_host[c + 1] >= a.clip_off_host[c], "clip_off must not decrease");
  }
  const int n_vt = a.d_pad / NT;
  int groups = n_vt < 65535 ? n_vt : 65535;
  if (a.mode == RG_MESH_RAW) {
    RG_REQUIRE(h, a.out, "RAW needs out");
  } else {
    RG_REQUIRE(h, a.A && a.skin_n && a.skin_j && a.skin_w, "skinning needs A and the weight lists");
    RG_REQUIRE(h, a.max_nnz >= 1 && a.max_nnz <= NJ, "max_nnz must lie in [1, 55]");
    if (a.mode == RG_MESH_VERTICES) {
      RG_REQUIRE(h, a.out, "VERTICES needs out");
    } else {
      RG_REQUIRE(h, a.partial && a.rows % 2 == 0 && a.n_groups >= 1 && a.n_groups <= n_vt,
                 "FACE needs partial, even rows and 1 <= n_groups <= vertex tiles");
      RG_REQUIRE(h, a.partial_len >= (int64_t)(a.rows / 2) * a.n_groups * 2, "partial holds fewer than rows / 2 * n_groups * 2 doubles");
      RG_REQUIRE(h, a.base_per_clip, "FACE needs a base per clip");
      for (int c = 0; c <= a.n_clips; ++c) RG_REQUIRE(h, a.clip_off_host[c] % 2 == 0, "FACE clips must hold frame pairs");
      groups = a.n_groups;
    }
  }
  const int tiles = (a.rows + MT - 1) / MT;
  hipLaunchKernelGGL(mesh_blend_skin_kernel, dim3(tiles, groups), dim3(BS_THREADS), 0, rg_stream(stream), a, n_vt);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_mesh_face_sums(rg_handle* h, const rg_mesh_face_sums_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_mesh_face_sums_args& a = *args_host;
  RG_REQUIRE(h, a.partial && a.pair_off && a.pair_off_host && a.sums, "null pointer");
  RG_REQUIRE(h, a.n_clips >= 1 && a.n_groups >= 1, "need at least one clip and one group");
  RG_REQUIRE(h, a.pair_off_host[0] == 0, "pair_off must start at 0");
  for (int c = 0; c < a.n_clips; ++c) RG_REQUIRE(h, a.pair_off_host[c + 1] >= a.pair_off_host[c], "pair_off must not decrease");
  hipLaunchKernelGGL(mesh_face_sums_kernel, dim3(a.n_clips), dim3(256), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
