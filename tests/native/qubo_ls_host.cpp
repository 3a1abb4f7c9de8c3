// qubo_ls_host.cpp — stand-alone host check of cpu::qubo_local_search (the CPU
// mirror of the one-flip local search stage), meant to be built with
// AddressSanitizer + UndefinedBehaviorSanitizer; no GPU, no python:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Icsrc/include tests/native/qubo_ls_host.cpp csrc/cpu/cpu_qubo.cpp csrc/cpu/parallel.cpp \
//       -lpthread -o build/qubo_ls_host && build/qubo_ls_host
//
// The case: L = 65 (two 32-bit words and one bit; a 128-bit row), asymmetric
// Q in [-128, 127], 64 rows, minimise, moves in {1, 3, 4 L}, every row
// selected and a share of 0.3.  Each result is compared with a literal
// re-computation that rebuilds every gain from the matrix at every move.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pga/cpu.hpp"
#include "pga/qubo_ops.hpp"

using namespace pga;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main() {
  const uint32_t L = 65, row_words = 4, S = 64;
  uint32_t seed = 12345u;
  std::vector<float> Q((size_t)L * L);
  for (float& v : Q) v = (float)((int)(lcg(seed) >> 24) - 128);
  std::vector<int> q((size_t)L * L);
  for (size_t i = 0; i < q.size(); ++i) q[i] = qubo_coef(Q[i]);
  std::vector<uint32_t> rows0((size_t)S * row_words, 0u);
  for (uint32_t n = 0; n < S; ++n)
    for (uint32_t p = 0; p < L; ++p)
      if (lcg(seed) >> 31) rows0[(size_t)n * row_words + p / 32] |= 1u << (p % 32);
  const float f0 = -1.f;
  int bad = 0;
  for (uint32_t moves : {1u, 3u, 4u * L})
    for (float prob : {1.f, 0.3f}) {
      std::vector<uint32_t> rows = rows0;
      std::vector<float> scores(S, 12345.f);
      LsArgs a;
      std::memset(&a, 0, sizeof(a));
      a.rows = rows.data();
      a.scores = scores.data();
      a.S = S;
      a.L = L;
      a.row_words = row_words;
      a.chunks = 1;
      a.key.k0 = 7;
      a.key.gen = 3;
      a.objective = OBJ_QUBO;
      a.obj_data = Q.data();
      a.obj_f0 = f0;
      a.kind = LS_ONE_FLIP;
      a.moves = moves;
      a.always = prob >= 1.f ? 1u : 0u;
      a.thresh = (uint32_t)((double)prob * 4294967296.0 >= 4294967295.0 ? 4294967295.0 : (double)prob * 4294967296.0);
      cpu::qubo_local_search(a);

      for (uint32_t n = 0; n < S; ++n) {
        std::vector<int> x(L);
        for (uint32_t p = 0; p < L; ++p) x[p] = (rows0[(size_t)n * row_words + p / 32] >> (p % 32)) & 1u;
        const auto f = [&]() {
          long long v = 0;
          for (uint32_t i = 0; i < L; ++i)
            for (uint32_t j = 0; j < L; ++j) v += (long long)q[(size_t)i * L + j] * x[i] * x[j];
          return v;
        };
        bool moved = false;
        if (ls_selected(a, n))
          for (uint32_t m = 0; m < moves; ++m) {
            const long long base = f();
            long long bg = 0;
            int bp = -1;
            for (uint32_t p = 0; p < L; ++p) {  // the first maximum of s * (f(x ^ e_p) - f(x))
              x[p] ^= 1;
              const long long g = -(f() - base);
              x[p] ^= 1;
              if (g > bg) bg = g, bp = (int)p;
            }
            if (bp < 0) break;
            x[bp] ^= 1;
            moved = true;
          }
        for (uint32_t w = 0; w < row_words; ++w) {
          uint32_t want = 0;
          for (uint32_t p = 32 * w; p < 32 * w + 32 && p < L; ++p) want |= (uint32_t)x[p] << (p % 32);
          if (rows[(size_t)n * row_words + w] != want) ++bad;
        }
        const float ws = moved ? f0 * (float)(int32_t)f() : 12345.f;
        if (scores[n] != ws) ++bad;
      }
    }
  std::printf("qubo_ls_host: %s (%d mismatches)\n", bad ? "FAILED" : "ok", bad);
  return bad ? 1 : 0;
}
