// perm_ls.hip — 2-opt local search stage of the PERMUTATION encoding on gfx950
// (Island::local_search; the semantics are perm_ops.hpp two_opt_*, the CPU
// mirror is cpu_perm.cpp perm_local_search).
//
// One 64-lane wave owns one tour (waves stride over the population).  The
// tour lives in LDS as u16 beside the f32 lengths of its own edges, so a
// candidate pair (i, j) costs two distance lookups: d(t[i], t[j]) and
// d(t[i+1], t[j+1]).  The distance source is a template parameter:
//   SRC_L2     the f32 matrix through L2
//   SRC_TRI16  GenArgs::obj_aux kind 1: the u16 lower triangle, staged in LDS
//   SRC_TRI32  kind 3: the f32 lower triangle, staged in LDS
//   SRC_EUC    city coordinates staged in LDS (OBJ_TSP_EUC)
// The triangle variants run 16-wave blocks so that 16 tours share the one
// table of a CU, as perm.hip's TBL variants do.  Every source holds the
// matrix's own values, so all four give identical moves and scores.
//
// Per move: for each wave-uniform i the lanes stride over j (ascending) and
// keep their first best gain (strict >, so a lane's best is its first in
// (i, j) order); one u64 butterfly max of two_opt_key picks the pair; the
// lanes reverse t[i+1 .. j] and the edge lengths between (a symmetric d keeps
// them), and lane 0 stores the two new edges.  Only wave-level
// synchronisation inside the move loop: the waves of a block stop after
// different move counts.  A wave whose individual is not selected costs its
// one Philox draw.  (Four slots of j per step, with the next i's uniform
// reads issued one i ahead, measured 2 % faster at TSP-256 -- inside the
// run-to-run spread -- so the plain loop stays: the pair loop is bound by
// VALU issue, ~50 instructions per 64 pairs, docs/ARCHITECTURE.md.)
//
// A row that moved is written back with the score MODE_EVAL would give it:
// lane q < GS sums the edges of chunks q, q + GS, ... in order, then the
// GS-lane butterfly (perm.hip stage 4, cpu_perm.cpp).
#include <hip/hip_runtime.h>

#include <string>

#include "pga/device.hpp"
#include "pga/ops.hpp"
#include "pga/perm_ops.hpp"

namespace pga {
namespace {

using namespace dev;

enum : int { SRC_L2 = 0, SRC_TRI16 = 1, SRC_TRI32 = 3, SRC_EUC = 4 };

// per-wave LDS: the tour (lp u16) and its edge lengths (lp f32)
__host__ __device__ inline size_t ls_wave_bytes(uint32_t chunks) { return 8ull * chunks * (2 + 4); }
__host__ __device__ inline size_t ls_lds_bytes(uint32_t chunks, uint32_t L, int src, uint32_t aux_bytes, uint32_t nw) {
  const size_t coords = src == SRC_EUC ? (8ull * L + 15) / 16 * 16 : 0;
  const size_t table = (src == SRC_TRI16 || src == SRC_TRI32) ? aux_bytes : 0;
  return coords + table + (size_t)nw * ls_wave_bytes(chunks);
}

template <int SRC, bool OPEN>
__global__ __launch_bounds__(SRC == SRC_TRI16 || SRC == SRC_TRI32 ? 1024 : kBlock) void perm_ls_kernel(LsArgs a) {
  const uint32_t L = a.L, nch = a.chunks, lp = 8 * nch;
  const uint32_t BLK = blockDim.x, NW = BLK >> 6, wv = threadIdx.x >> 6, lane = lane_id();
  // shared sources first (16-byte aligned sizes), then the waves' arrays
  char* base = (char*)pga_dyn_lds;
  const float* coords = (const float*)base;
  const uint16_t* tab16 = (const uint16_t*)base;
  const float* tab32 = (const float*)base;
  const size_t shared_bytes = ls_lds_bytes(nch, L, SRC, a.obj_aux_bytes, 0);
  uint16_t* t = (uint16_t*)(base + shared_bytes + (size_t)wv * ls_wave_bytes(nch));
  float* el = (float*)(t + lp);

  if (SRC == SRC_EUC)
    for (uint32_t i = threadIdx.x; i < 2 * L; i += BLK) ((float*)base)[i] = a.obj_data[i];
  if (SRC == SRC_TRI16 || SRC == SRC_TRI32)
    for (uint32_t i = threadIdx.x; i < a.obj_aux_bytes / 16; i += BLK) ((uint4*)base)[i] = ((const uint4*)a.obj_aux)[i];
  __syncthreads();  // the only block barrier: the waves are on their own from here

  // d(u, w); the min(): a forged row can never index out of bounds (perm.hip stage 4)
  const auto dist = [&](uint32_t u, uint32_t w) -> float {
    u = min(u, L - 1);
    w = min(w, L - 1);
    if constexpr (SRC == SRC_EUC) {
      const float2 pu = ((const float2*)coords)[u], pw = ((const float2*)coords)[w];
      const float dx = pu.x - pw.x, dy = pu.y - pw.y;
      return sqrtf(fmaf(dx, dx, dy * dy));
    } else if constexpr (SRC == SRC_TRI16 || SRC == SRC_TRI32) {
      const uint32_t hi = max(u, w), lo = min(u, w);
      const uint32_t ix = ((hi * (hi + 1u)) >> 1) + lo;  // (hi, lo <= hi) at hi (hi + 1) / 2 + lo
      return SRC == SRC_TRI16 ? (float)tab16[ix] : tab32[ix];
    } else {
      return a.obj_data[u * L + w];
    }
  };

  const uint64_t rs = a.row_words >> 2;
  uint4* rows = (uint4*)a.rows;
  const uint32_t GS = group_size(nch);
  const uint64_t TW = (uint64_t)gridDim.x * NW;
  for (uint64_t n = (uint64_t)blockIdx.x * NW + wv; n < a.S; n += TW) {  // wave-uniform
    if (!ls_selected(a, n)) continue;
    for (uint32_t c = lane; c < nch; c += 64) *(uint4*)(t + 8 * c) = rows[n * rs + c];
    wave_lds_sync();
    for (uint32_t p = lane; p < L; p += 64)
      el[p] = (OPEN && p == L - 1) ? 0.f : dist(t[p], t[p + 1 == L ? 0 : p + 1]);
    wave_lds_sync();

    bool moved = false;
    for (uint32_t m = 0; m < a.moves && L >= 3; ++m) {
      float bg = 0.f;  // a NaN gain never passes the strict >
      uint32_t bp = 0;
      for (uint32_t i = 0; i + 2 < L; ++i) {
        const uint32_t ta = t[i], tb = t[i + 1];  // wave-uniform reads
        const float dab = el[i];
        const uint32_t jmax = two_opt_jmax(i, L, OPEN);
        for (uint32_t j = i + 2 + lane; j <= jmax; j += 64) {
          const bool closing = OPEN && j == L - 1;
          const uint32_t tc = t[j], te = t[j + 1 == L ? 0 : j + 1];
          const float dce = el[j];  // 0 in the open path's closing position
          const float dac = dist(ta, tc), dbe = closing ? 0.f : dist(tb, te);
          const float g = two_opt_gain(dab, dce, dac, dbe);
          if (g > bg) {
            bg = g;
            bp = i * L + j;
          }
        }
      }
      unsigned long long key = two_opt_key(bg, bp);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = shfl_xor_u64(key, o);
        key = w > key ? w : key;
      }
      if (key == 0ull) break;  // 2-optimal (wave-uniform)
      const uint32_t pr = two_opt_pair(key), i = pr / L, j = pr - i * L;
      // the two new edges (every lane: the same values), read before the reversal
      const float nac = dist(t[i], t[j]);
      const float nbe = (OPEN && j == L - 1) ? 0.f : dist(t[i + 1], t[j + 1 == L ? 0 : j + 1]);
      wave_lds_sync();
      for (uint32_t k = lane; k < (j - i) / 2; k += 64) {  // t[i+1 .. j]
        const uint16_t x = t[i + 1 + k];
        t[i + 1 + k] = t[j - k];
        t[j - k] = x;
      }
      for (uint32_t k = lane; k < (j - i - 1) / 2; k += 64) {  // the edges between: el[i+1 .. j-1]
        const float x = el[i + 1 + k];
        el[i + 1 + k] = el[j - 1 - k];
        el[j - 1 - k] = x;
      }
      if (lane == 0) {
        el[i] = nac;
        el[j] = nbe;
      }
      wave_lds_sync();
      moved = true;
    }
    if (!moved) continue;

    for (uint32_t c = lane; c < nch; c += 64) rows[n * rs + c] = *(const uint4*)(t + 8 * c);
    float len = 0.f;
    const uint32_t last = OPEN ? L - 1 : L;
    if (lane < GS)
      for (uint32_t c = lane; c < nch; c += GS)
        for (uint32_t e = 0; e < 8; ++e) {
          const uint32_t p = 8 * c + e;
          if (p >= last) break;
          len += el[p];
        }
    for (uint32_t o = GS >> 1; o > 0; o >>= 1) len += __shfl_xor(len, (int)o, 64);
    if (lane == 0) a.scores[n] = -len;
    wave_lds_sync();  // the next tour overwrites t / el
  }
}

template <int SRC, bool OPEN>
void go(const LsArgs& a, hipStream_t s) {
  auto k = perm_ls_kernel<SRC, OPEN>;
  const size_t avail = allow_dynamic_lds((const void*)k);
  constexpr bool TBL = SRC == SRC_TRI16 || SRC == SRC_TRI32;
  // the largest block whose waves' arrays fit beside the shared source
  uint32_t blk = 0;
  for (uint32_t b : {TBL ? 1024u : (uint32_t)kBlock, TBL ? 512u : 128u, TBL ? 256u : 64u})
    if (ls_lds_bytes(a.chunks, a.L, SRC, a.obj_aux_bytes, b / 64) <= avail) {
      blk = b;
      break;
    }
  if (blk == 0) {
    if constexpr (TBL) return go<SRC_L2, OPEN>(a, s);  // no room beside the table: the matrix through L2
    throw std::invalid_argument("local search: the tour does not fit the LDS of this device");
  }
  const size_t lds = ls_lds_bytes(a.chunks, a.L, SRC, a.obj_aux_bytes, blk / 64);
  const uint32_t nw = blk / 64;
  uint64_t cap = (uint64_t)device_cu_count() * occupancy_blocks((const void*)k, (int)blk, lds);
  if (cap < 1) cap = 1;
  if (cap > kMaxGrid) cap = kMaxGrid;
  const uint64_t need = (a.S + nw - 1) / nw;
  hipLaunchKernelGGL(k, (uint32_t)(need < cap ? need : cap), blk, lds, s, a);
}

template <bool OPEN>
void go_src(const LsArgs& a, hipStream_t s) {
  if (a.obj_aux && a.obj_aux_bytes % 16 == 0) {
    if (a.obj_aux_kind == 1) return go<SRC_TRI16, OPEN>(a, s);
    if (a.obj_aux_kind == 3) return go<SRC_TRI32, OPEN>(a, s);
  }
  go<SRC_L2, OPEN>(a, s);
}

}  // namespace

void perm_ls_launch(const LsArgs& a, hipStream_t s) {
  if (a.L > kPermMaxL)
    throw std::invalid_argument("local search: genome too long for the LDS-resident tour (" + std::to_string(a.L) +
                                " cities; at most " + std::to_string(kPermMaxL) + " on the GPU)");
  switch (a.objective) {
    case OBJ_TSP: go_src<false>(a, s); break;
    case OBJ_TSP_OPEN: go_src<true>(a, s); break;
    case OBJ_TSP_EUC: go<SRC_EUC, false>(a, s); break;
    default: throw std::invalid_argument("local search needs a TSP objective");
  }
  PGA_HIP_CHECK(hipGetLastError());
}

}  // namespace pga
