// The rotation the angle-holding tasks share (swingup.hip, reacher.hip; `_rot` of pql_amd/envs/swingup.py is the definition).
#pragma once

#pragma clang fp contract(off)

// (c, s) rotated by the angle d, |d| <= 0.5: cos d and sin d to degree 4 / 5, then m = 1.5 - 0.5 |.|^2 pulls the result back
// to the unit circle.  No transcendental function, no division, no square root; the operation order is the one of `_rot`.
__device__ __forceinline__ void task_rot(float& c, float& s, float d) {
  const float d2 = d * d;
  const float cd = 1.0f - d2 * (0.5f - d2 * 0.041666668f);
  const float sd = d * (1.0f - d2 * (0.16666667f - d2 * 0.008333334f));
  const float cn = c * cd - s * sd;
  const float sn = s * cd + c * sd;
  const float m = 1.5f - 0.5f * (cn * cn + sn * sn);
  c = cn * m;
  s = sn * m;
}
