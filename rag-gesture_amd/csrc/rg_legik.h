// The two-bone leg solve of the foot lock (rg_footlock.hip; include/rg_gesture.h) in fp64: plain C++ with no
// device call in it, so that the kernel's lanes and a host program run the same source -- tests/test_foot_lock_cpu.py compiles it
// with the host compiler and walks every branch (the straight leg, the target on the hip-ankle line, the log map next to zero and
// next to pi) against the numpy restatement, which poses stored as fp32 cannot reach on the device.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RG_LEGIK_FN __host__ __device__ __forceinline__
#else
#define RG_LEGIK_FN inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace {

struct v3 {
  double x, y, z;
};
struct m3 {
  double m[9];                                         // row-major
};
RG_LEGIK_FN v3 vsub(v3 a, v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
RG_LEGIK_FN v3 vcross(v3 a, v3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
RG_LEGIK_FN double vdot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RG_LEGIK_FN double vlen(v3 a) { return sqrt(vdot(a, a)); }
RG_LEGIK_FN double vangle(v3 a, v3 b) { return atan2(vlen(vcross(a, b)), vdot(a, b)); }
RG_LEGIK_FN double clamp1(double x) { return fmin(1.0, fmax(-1.0, x)); }

// R = cos I + (1 - cos) n n^T + sin [n]x for a unit axis n
RG_LEGIK_FN m3 rot(v3 n, double th) {
  const double c = cos(th), s = sin(th), oc = 1.0 - c;
  return {{c + oc * n.x * n.x, oc * n.x * n.y - s * n.z, oc * n.x * n.z + s * n.y,
           oc * n.y * n.x + s * n.z, c + oc * n.y * n.y, oc * n.y * n.z - s * n.x,
           oc * n.z * n.x - s * n.y, oc * n.z * n.y + s * n.x, c + oc * n.z * n.z}};
}
RG_LEGIK_FN m3 identity3() { return {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}}; }
RG_LEGIK_FN m3 mmul(const m3& a, const m3& b) {
  m3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.m[3 * i + j] = (a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j]) + a.m[3 * i + 2] * b.m[6 + j];
  return r;
}
RG_LEGIK_FN m3 mtmul(const m3& a, const m3& b) {                               // a^T b
  m3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.m[3 * i + j] = (a.m[i] * b.m[j] + a.m[3 + i] * b.m[3 + j]) + a.m[6 + i] * b.m[6 + j];
  return r;
}

// the axis-angle of a rotation matrix, angle in [0, pi]: r = (R32 - R23, R13 - R31, R21 - R12) = 2 sin(angle) axis and
// trace - 1 = 2 cos(angle).  |r| < 1e-9: the small angle r / 2, or next to pi the axis from the diagonal of (R + I) / 2, its
// signs from the row of its greatest entry
RG_LEGIK_FN void log_map(const m3& R, double out[3]) {
  const double rx = R.m[7] - R.m[5], ry = R.m[2] - R.m[6], rz = R.m[3] - R.m[1];
  const double s2 = sqrt((rx * rx + ry * ry) + rz * rz), c2 = ((R.m[0] + R.m[4]) + R.m[8]) - 1.0;
  if (s2 >= 1e-9) {
    const double k = atan2(s2, c2) / s2;
    out[0] = k * rx, out[1] = k * ry, out[2] = k * rz;
  } else if (c2 > 0.0) {
    out[0] = 0.5 * rx, out[1] = 0.5 * ry, out[2] = 0.5 * rz;
  } else {
    double ax[3];
    int big = 0;
    for (int i = 0; i < 3; ++i) {
      ax[i] = sqrt(fmax(0.0, 0.5 * (R.m[4 * i] + 1.0)));
      if (ax[i] > ax[big]) big = i;
    }
    for (int i = 0; i < 3; ++i)
      if (i != big && R.m[3 * big + i] + R.m[3 * i + big] < 0.0) ax[i] = -ax[i];
    const double pi = 3.14159265358979323846;
    out[0] = pi * ax[0], out[1] = pi * ax[1], out[2] = pi * ax[2];
  }
}

// world rotations of the hip's parent, hip, knee and ankle, positions a, b, c of hip, knee and ankle, the ankle's target T ->
// the new local axis-angles of hip, knee and ankle in aa[9] (pose_mean not taken off) and |T - a| / (l1 + l2).
// A straight leg bends about the hip's own x axis by a POSITIVE angle: the thigh turns backwards and the shank forwards (for a
// leg hanging along -y with z forward), the reverse of a natural knee; the choice is the definition's, and only a leg that is
// straight to 1e-5 takes it.
RG_LEGIK_FN double leg_solve(const m3& Wp, const m3& Wh, const m3& Wk, const m3& Wa, v3 a, v3 b, v3 c, v3 T, double stretch,
                             double aa[9]) {
  const v3 ab = vsub(b, a), ac = vsub(c, a), aT = vsub(T, a), ba = vsub(a, b), bc = vsub(c, b);
  const double l1 = vlen(ab), l2 = vlen(bc), want = vlen(aT);
  const double dist = fmin(fmax(want, fabs(l1 - l2) * (1.0 + 1e-3) + 1e-9), stretch * (l1 + l2));
  const double A0 = vangle(ac, ab), K0 = vangle(ba, bc);
  const double A1 = acos(clamp1(((l1 * l1 + dist * dist) - l2 * l2) / ((2.0 * l1) * dist)));
  const double K1 = acos(clamp1(((l1 * l1 + l2 * l2) - dist * dist) / ((2.0 * l1) * l2)));
  v3 n0 = vcross(ac, ab);
  double len = vlen(n0);
  if (len < 1e-5 * (vlen(ac) * l1)) {                  // a straight leg
    n0 = {Wh.m[0], Wh.m[3], Wh.m[6]};
    len = vlen(n0);
  }
  n0 = {n0.x / len, n0.y / len, n0.z / len};
  const m3 B0 = rot(n0, A1 - A0), B1 = rot(n0, K1 - K0);
  v3 n1 = vcross(ac, aT);
  const double len1 = vlen(n1);
  m3 S = identity3();
  if (len1 > 0.0 && len1 >= 1e-12 * (vlen(ac) * want)) {
    n1 = {n1.x / len1, n1.y / len1, n1.z / len1};
    S = rot(n1, vangle(ac, aT));
  }
  const m3 SB0 = mmul(S, B0);
  const m3 Wh2 = mmul(SB0, Wh), Wk2 = mmul(mmul(SB0, B1), Wk);
  log_map(mtmul(Wp, Wh2), aa);
  log_map(mtmul(Wh2, Wk2), aa + 3);
  log_map(mtmul(Wk2, Wa), aa + 6);
  return want / (l1 + l2);
}

}  // namespace
