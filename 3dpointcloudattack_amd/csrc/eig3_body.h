// The closed-form solve both normal estimators share (normal.hip: GeoA3's estimate_normal; siadv.hip: SI-Adv's PCA
// normals): the unit eigenvector of the SMALLEST eigenvalue of a symmetric 3 x 3 matrix, in double.
#pragma once
#include "pc3d_common.h"

namespace pc3d {

// A = [[c00 c01 c02] [c01 c11 c12] [c02 c12 c22]]. Eigenvalues from the trigonometric solution of the characteristic
// cubic (Smith 1961), the eigenvector as the largest cross product of two rows of A - lambda_min I. (nx, ny, nz) is
// left at (0, 0, 1) when the deviator of A is zero (A a multiple of I) or every cross product vanishes. The sign of the
// result is whatever the cross product gives: callers fix it by their own rule.
__device__ __forceinline__ void eig3_smallest_vec(double c00, double c01, double c02, double c11, double c12, double c22,
                                                  double& nx, double& ny, double& nz) {
  nx = 0.0, ny = 0.0, nz = 1.0;
  const double q = (c00 + c11 + c22) / 3.0;
  const double p1 = c01 * c01 + c02 * c02 + c12 * c12;
  const double d0 = c00 - q, d1 = c11 - q, d2 = c22 - q;
  const double p2 = d0 * d0 + d1 * d1 + d2 * d2 + 2.0 * p1;
  if (p2 > 0.0) {
    const double p = sqrt(p2 / 6.0), ip = 1.0 / p;
    const double b00 = d0 * ip, b11 = d1 * ip, b22 = d2 * ip, b01 = c01 * ip, b02 = c02 * ip, b12 = c12 * ip;
    double r = 0.5 * (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02));
    r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    const double phi = acos(r) / 3.0;
    const double lmin = q + 2.0 * p * cos(phi + 2.0943951023931953);   // + 2 pi / 3
    // eigenvector: the largest cross product of two rows of A - lmin I
    const double r0x = c00 - lmin, r0y = c01, r0z = c02;
    const double r1x = c01, r1y = c11 - lmin, r1z = c12;
    const double r2x = c02, r2y = c12, r2z = c22 - lmin;
    const double ax = r0y * r1z - r0z * r1y, ay = r0z * r1x - r0x * r1z, az = r0x * r1y - r0y * r1x;
    const double bx = r0y * r2z - r0z * r2y, by = r0z * r2x - r0x * r2z, bz = r0x * r2y - r0y * r2x;
    const double cx = r1y * r2z - r1z * r2y, cy = r1z * r2x - r1x * r2z, cz = r1x * r2y - r1y * r2x;
    const double na = ax * ax + ay * ay + az * az, nbn = bx * bx + by * by + bz * bz, nc = cx * cx + cy * cy + cz * cz;
    double vx = ax, vy = ay, vz = az, nn = na;
    if (nbn > nn) vx = bx, vy = by, vz = bz, nn = nbn;
    if (nc > nn) vx = cx, vy = cy, vz = cz, nn = nc;
    if (nn > 0.0) {
      const double inv = 1.0 / sqrt(nn);
      nx = vx * inv, ny = vy * inv, nz = vz * inv;
    }
  }
}

}  // namespace pc3d
