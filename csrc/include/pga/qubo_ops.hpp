// qubo_ops.hpp — one-flip local search semantics of the QUBO objective
// (LS_ONE_FLIP), shared by the gfx950 kernel (csrc/kernels/qubo_ls.hip) and
// the CPU reference (csrc/cpu/cpu_qubo.cpp).  Integer arithmetic end to end:
// the two agree bit for bit with no tolerance anywhere.
//
// q[i][j] = qubo_coef(Q[i][j]), x the row's bits, f(x) = sum_ij q[i][j] x_i x_j.
//   g_p     = sum_j (q[p][j] + q[j][p]) x_j      (j = p included; Q need not be symmetric)
//   delta_p = (1 - 2 x_p) g_p + q[p][p]          the change of f when bit p flips
//   gain_p  = s * delta_p,  s = +1 if obj_f0 > 0, -1 if obj_f0 < 0
// One move: the largest gain over p in [0, L), ties to the smallest p (the
// maximum of one_flip_key); a gain > 0 flips the bit, after which every g_j
// changes by (1 - 2 x_p_old) (q[j][p] + q[p][j]); otherwise the row is
// one-flip optimal.  A row that moved is scored obj_f0 * (float)(int32_t) f
// with f = (sum_p x_p g_p) / 2 exactly in integers -- the value MODE_EVAL gives.
// |g_p| <= 256 * 1024 and |f| <= 128 * 1024^2: everything fits int32.
#pragma once

#include "pga/core.hpp"

namespace pga {

// s; 0 when obj_f0 is 0 or NaN (the stage then throws)
PGA_HD int32_t one_flip_sign(float obj_f0) { return obj_f0 > 0.f ? 1 : (obj_f0 < 0.f ? -1 : 0); }
PGA_HD int32_t one_flip_delta(int32_t x_p, int32_t g_p, int32_t q_pp) { return (1 - 2 * x_p) * g_p + q_pp; }
// a candidate's key (0: no candidate): larger gain first, then the smaller position
PGA_HD unsigned long long one_flip_key(int32_t gain, uint32_t p) {
  return gain > 0 ? (((unsigned long long)(uint32_t)gain << 32) | (0xFFFFFFFFu - p)) : 0ull;
}
PGA_HD uint32_t one_flip_pos(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }
PGA_HD float one_flip_score(float obj_f0, int32_t twice_f) { return obj_f0 * (float)(int32_t)(twice_f / 2); }

}  // namespace pga
