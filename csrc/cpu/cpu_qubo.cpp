// cpu_qubo.cpp — CPU reference of the one-flip local search stage of the QUBO
// objective (LS_ONE_FLIP); mirrors csrc/kernels/qubo_ls.hip.  It follows the
// definitions of qubo_ops.hpp literally, one individual at a time, in exact
// integer arithmetic, so rows and scores are bit-identical to the GPU.  No
// length limit of its own.
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "pga/cpu.hpp"
#include "pga/qubo_ops.hpp"

namespace pga {
namespace cpu {

void qubo_local_search(const LsArgs& a) {
  const int32_t s = one_flip_sign(a.obj_f0);
  if (s == 0) throw std::invalid_argument("one-flip local search: the QUBO score factor (obj_f0) must be non-zero");
  const uint32_t L = a.L;
  // w[p][j] = q[p][j] + q[j][p] (symmetric), d[p] = q[p][p]
  std::vector<int16_t> w((size_t)L * L);
  std::vector<int32_t> d(L);
  for (uint32_t p = 0; p < L; ++p) {
    d[p] = qubo_coef(a.obj_data[(size_t)p * L + p]);
    for (uint32_t j = 0; j < L; ++j)
      w[(size_t)p * L + j] = (int16_t)(qubo_coef(a.obj_data[(size_t)p * L + j]) + qubo_coef(a.obj_data[(size_t)j * L + p]));
  }
  uint32_t* rows = (uint32_t*)a.rows;
  parallel_for(a.S, 16, [&](uint64_t n_begin, uint64_t n_end, unsigned) {
    std::vector<int32_t> g(L);
    for (uint64_t n = n_begin; n < n_end; ++n) {
      if (!ls_selected(a, n)) continue;
      uint32_t* r = rows + n * a.row_words;
      const auto bit = [&](uint32_t p) -> int32_t { return (int32_t)((r[p / 32] >> (p % 32)) & 1u); };
      std::fill(g.begin(), g.end(), 0);
      for (uint32_t j = 0; j < L; ++j) {
        if (!bit(j)) continue;
        const int16_t* wj = &w[(size_t)j * L];  // w is symmetric: row j is column j
        for (uint32_t p = 0; p < L; ++p) g[p] += wj[p];
      }
      bool moved = false;
      for (uint32_t m = 0; m < a.moves; ++m) {
        unsigned long long best = 0;
        for (uint32_t p = 0; p < L; ++p) {
          const unsigned long long k = one_flip_key(s * one_flip_delta(bit(p), g[p], d[p]), p);
          best = k > best ? k : best;
        }
        if (best == 0) break;  // one-flip optimal
        const uint32_t p = one_flip_pos(best);
        const int32_t sg = 1 - 2 * bit(p);
        r[p / 32] ^= 1u << (p % 32);
        const int16_t* wp = &w[(size_t)p * L];
        for (uint32_t j = 0; j < L; ++j) g[j] += sg * wp[j];
        moved = true;
      }
      if (!moved) continue;
      int32_t f2 = 0;
      for (uint32_t p = 0; p < L; ++p) f2 += bit(p) ? g[p] : 0;
      a.scores[n] = one_flip_score(a.obj_f0, f2);
    }
  });
}

}  // namespace cpu
}  // namespace pga
