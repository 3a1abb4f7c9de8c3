// perm_ls.hip — 2-opt and Or-opt local search stages of the PERMUTATION
// encoding on gfx950 (Island::local_search, by LsArgs::kind; the semantics are
// perm_ops.hpp two_opt_* / or_opt_*, the CPU mirror is cpu_perm.cpp
// perm_local_search).  Both kernels share one frame; 2-opt first, the Or-opt
// scan and move are described at perm_oropt_kernel.
//
// One 64-lane wave owns one tour (waves stride over the population).  The
// tour lives in LDS as u16 beside the f32 lengths of its own edges, so a
// candidate pair (i, j) costs two distance lookups: d(t[i], t[j]) and
// d(t[i+1], t[j+1]).  The distance source is a template parameter:
//   SRC_L2     the f32 matrix through L2
//   SRC_TRI16  GenArgs::obj_aux kind 1: the u16 lower triangle, staged in LDS
//   SRC_FULL16 kind 2: the full u16 matrix of an asymmetric integer instance,
//              staged in LDS (Or-opt only: 2-opt refuses such a matrix)
//   SRC_TRI32  kind 3: the f32 lower triangle, staged in LDS
//   SRC_EUC    city coordinates staged in LDS (OBJ_TSP_EUC)
// The table variants run 16-wave blocks so that 16 tours share the one
// table of a CU, as perm.hip's TBL variants do.  Every source holds the
// matrix's own values, so all give identical moves and scores.
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

enum : int { SRC_L2 = 0, SRC_TRI16 = 1, SRC_FULL16 = 2, SRC_TRI32 = 3, SRC_EUC = 4 };
constexpr bool src_table(int src) { return src == SRC_TRI16 || src == SRC_FULL16 || src == SRC_TRI32; }

// per-wave LDS: the tour (lp u16) and its edge lengths (lp f32)
__host__ __device__ inline size_t ls_wave_bytes(uint32_t chunks) { return 8ull * chunks * (2 + 4); }
__host__ __device__ inline size_t ls_lds_bytes(uint32_t chunks, uint32_t L, int src, uint32_t aux_bytes, uint32_t nw) {
  const size_t coords = src == SRC_EUC ? (8ull * L + 15) / 16 * 16 : 0;
  const size_t table = src_table(src) ? aux_bytes : 0;
  return coords + table + (size_t)nw * ls_wave_bytes(chunks);
}

// d(u, w) of one source; the min(): a forged row can never index out of bounds
// (perm.hip stage 4)
template <int SRC>
struct Dist {
  const void* lds;   // the staged coordinates or table
  const float* mat;  // the f32 matrix (SRC_L2)
  uint32_t L;
  __device__ __forceinline__ float operator()(uint32_t u, uint32_t w) const {
    u = min(u, L - 1);
    w = min(w, L - 1);
    if constexpr (SRC == SRC_EUC) {
      const float2 pu = ((const float2*)lds)[u], pw = ((const float2*)lds)[w];
      const float dx = pu.x - pw.x, dy = pu.y - pw.y;
      return sqrtf(fmaf(dx, dx, dy * dy));
    } else if constexpr (SRC == SRC_TRI16 || SRC == SRC_TRI32) {
      const uint32_t hi = max(u, w), lo = min(u, w);
      const uint32_t ix = ((hi * (hi + 1u)) >> 1) + lo;  // (hi, lo <= hi) at hi (hi + 1) / 2 + lo
      return SRC == SRC_TRI16 ? (float)((const uint16_t*)lds)[ix] : ((const float*)lds)[ix];
    } else if constexpr (SRC == SRC_FULL16) {
      return (float)((const uint16_t*)lds)[u * L + w];
    } else {
      return mat[u * L + w];
    }
  }
};

// The frame of both kernels: the block stages the shared source (its only
// block barrier: the waves are on their own afterwards), every wave gets its
// own tour and edge-length arrays behind it.
template <int SRC>
__device__ __forceinline__ Dist<SRC> ls_stage(const LsArgs& a, uint16_t*& t, float*& el) {
  const uint32_t BLK = blockDim.x, wv = threadIdx.x >> 6;
  // shared sources first (16-byte aligned sizes), then the waves' arrays
  char* base = (char*)pga_dyn_lds;
  const size_t shared_bytes = ls_lds_bytes(a.chunks, a.L, SRC, a.obj_aux_bytes, 0);
  t = (uint16_t*)(base + shared_bytes + (size_t)wv * ls_wave_bytes(a.chunks));
  el = (float*)(t + 8 * a.chunks);
  if (SRC == SRC_EUC)
    for (uint32_t i = threadIdx.x; i < 2 * a.L; i += BLK) ((float*)base)[i] = a.obj_data[i];
  if (src_table(SRC))
    for (uint32_t i = threadIdx.x; i < a.obj_aux_bytes / 16; i += BLK) ((uint4*)base)[i] = ((const uint4*)a.obj_aux)[i];
  __syncthreads();
  return Dist<SRC>{base, a.obj_data, a.L};
}

// row n into t, its edge lengths into el
template <bool OPEN, class D>
__device__ __forceinline__ void ls_load(const LsArgs& a, uint64_t n, const D& dist, uint16_t* t, float* el) {
  const uint32_t L = a.L, lane = lane_id();
  const uint4* rows = (const uint4*)a.rows;
  for (uint32_t c = lane; c < a.chunks; c += 64) *(uint4*)(t + 8 * c) = rows[n * (a.row_words >> 2) + c];
  wave_lds_sync();
  for (uint32_t p = lane; p < L; p += 64)
    el[p] = (OPEN && p == L - 1) ? 0.f : dist(t[p], t[p + 1 == L ? 0 : p + 1]);
  wave_lds_sync();
}

// A row that moved goes back with the score MODE_EVAL would give it: lane
// q < GS sums the edges of chunks q, q + GS, ... in order, then the GS-lane
// butterfly (perm.hip stage 4, cpu_perm.cpp).
template <bool OPEN>
__device__ __forceinline__ void ls_store(const LsArgs& a, uint64_t n, const uint16_t* t, const float* el) {
  const uint32_t L = a.L, nch = a.chunks, lane = lane_id(), GS = group_size(nch);
  uint4* rows = (uint4*)a.rows;
  for (uint32_t c = lane; c < nch; c += 64) rows[n * (a.row_words >> 2) + c] = *(const uint4*)(t + 8 * c);
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

__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long key) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = shfl_xor_u64(key, o);
    key = w > key ? w : key;
  }
  return key;
}

template <int SRC, bool OPEN>
__global__ __launch_bounds__(src_table(SRC) ? 1024 : kBlock) void perm_ls_kernel(LsArgs a) {
  const uint32_t L = a.L, NW = blockDim.x >> 6, wv = threadIdx.x >> 6, lane = lane_id();
  uint16_t* t;
  float* el;
  const Dist<SRC> dist = ls_stage<SRC>(a, t, el);
  const uint64_t TW = (uint64_t)gridDim.x * NW;
  for (uint64_t n = (uint64_t)blockIdx.x * NW + wv; n < a.S; n += TW) {  // wave-uniform
    if (!ls_selected(a, n)) continue;
    ls_load<OPEN>(a, n, dist, t, el);

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
      const unsigned long long key = wave_max_key(two_opt_key(bg, bp));
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
    if (moved) ls_store<OPEN>(a, n, t, el);
  }
}

// Or-opt (perm_ops.hpp or_opt_*) in the same frame.  For each wave-uniform p
// the lanes stride over the insertion edge q (ascending); six lookups,
// d(c, t[p..p+2]) and d(t[p..p+2], e), serve the five (s, r) candidates of a
// (p, q), taken in that order with a strict >, so a lane's best is its first
// in (p, q, s, r) order and the u64 butterfly max of or_opt_key picks the
// contract's winner.  The move shifts the stretch between the segment and its
// new place by s <= 3 inside LDS in 64-wide steps, from the end that never
// overwrites an unread entry, each step's reads before its writes; then every
// edge the move made gets a fresh d().
template <int SRC, bool OPEN>
__global__ __launch_bounds__(src_table(SRC) ? 1024 : kBlock) void perm_oropt_kernel(LsArgs a) {
  const uint32_t L = a.L, NW = blockDim.x >> 6, wv = threadIdx.x >> 6, lane = lane_id();
  uint16_t* t;
  float* el;
  const Dist<SRC> dist = ls_stage<SRC>(a, t, el);
  const uint64_t TW = (uint64_t)gridDim.x * NW;
  for (uint64_t n = (uint64_t)blockIdx.x * NW + wv; n < a.S; n += TW) {  // wave-uniform
    if (!ls_selected(a, n)) continue;
    ls_load<OPEN>(a, n, dist, t, el);

    bool moved = false;
    for (uint32_t m = 0; m < a.moves && L >= 3; ++m) {
      float bg = 0.f;  // a NaN gain never passes the strict >
      uint32_t bc = 0;
      for (uint32_t p = 0; p < L; ++p) {
        // wave-uniform: the segment's cities and edges (past the array's end:
        // clamped reads that no valid candidate uses), d(a, b) per length
        const uint32_t pm = p ? p - 1 : L - 1, smax = or_opt_smax(p, L);
        const uint32_t p1 = min(p + 1, L - 1), p2 = min(p + 2, L - 1);
        const uint32_t ta = t[pm], x0 = t[p], x1 = t[p1], x2 = t[p2];
        const float elp = el[pm], e0 = el[p], e1 = el[p1], e2 = el[p2];
        float dab[3];
#pragma unroll
        for (uint32_t s = 1; s <= 3; ++s) {
          const uint32_t pe = p + s;
          dab[s - 1] = (OPEN && (p == 0 || pe == L)) ? 0.f : dist(ta, t[pe >= L ? pe - L : pe]);
        }
        const float rev2 = dist(x1, x0), fwd3 = e0 + e1, rev3 = rev2 + dist(x2, x1);
        for (uint32_t q = lane; q < L; q += 64) {
          if (q == pm || q == p) continue;
          const uint32_t sq = q < p ? smax : min(smax, q - p);  // or_opt_q_ok: s <= q - p behind p
          const bool closing = OPEN && q == L - 1;
          const uint32_t c = t[q], e = t[q + 1 == L ? 0 : q + 1];
          const float elq = el[q];
          const float c0 = dist(c, x0), c1 = dist(c, x1), c2 = dist(c, x2);
          const float o0 = closing ? 0.f : dist(x0, e), o1 = closing ? 0.f : dist(x1, e), o2 = closing ? 0.f : dist(x2, e);
          const uint32_t cand = or_opt_cand(p, q, 1, 0, L);  // + 2 (s - 1) + r
          const auto take = [&](float g, uint32_t k) {
            if (g > bg) {
              bg = g;
              bc = k;
            }
          };
          if (sq >= 1) take(or_opt_gain(or_opt_removed(elp, e0, elq), dab[0], c0, o0), cand);
          if (sq >= 2) {
            const float rm = or_opt_removed(elp, e1, elq);
            take(or_opt_gain(rm, dab[1], c0, o1), cand + 2);
            take(or_opt_gain_rev(rm, e0, dab[1], c1, o0, rev2), cand + 3);
          }
          if (sq >= 3) {
            const float rm = or_opt_removed(elp, e2, elq);
            take(or_opt_gain(rm, dab[2], c0, o2), cand + 4);
            take(or_opt_gain_rev(rm, fwd3, dab[2], c2, o0, rev3), cand + 5);
          }
        }
      }
      const unsigned long long key = wave_max_key(or_opt_key(bg, bc));
      if (key == 0ull) break;  // Or-optimal (wave-uniform)
      uint32_t p, q, s, r;
      or_opt_decode(or_opt_key_cand(key), L, p, q, s, r);
      const uint32_t x0 = t[p], x1 = t[min(p + 1, L - 1)], x2 = t[min(p + 2, L - 1)];  // the segment, every lane
      wave_lds_sync();
      uint32_t at, ab;  // the segment's new first position, the position of the edge a -> b
      if (q > p) {      // t[p+s .. q] moves down by s, el[p+s .. q-1] with it: from the bottom
        const uint32_t cnt = q + 1 - (p + s);
        for (uint32_t k = lane; k - lane < cnt; k += 64) {
          const uint32_t src = p + s + k;
          const uint16_t tv = k < cnt ? t[src] : (uint16_t)0;
          const float ev = k + 1 < cnt ? el[src] : 0.f;
          wave_lds_sync();
          if (k < cnt) t[src - s] = tv;
          if (k + 1 < cnt) el[src - s] = ev;
          wave_lds_sync();
        }
        at = q + 1 - s;
        ab = p ? p - 1 : L - 1;
      } else {  // t[q+1 .. p-1] moves up by s, el[q+1 .. p-2] with it: from the top
        const uint32_t cnt = p - 1 - q;
        for (uint32_t k = lane; k - lane < cnt; k += 64) {
          const uint32_t src = p - 1 - k;  // (used for k < cnt only)
          const uint16_t tv = k < cnt ? t[src] : (uint16_t)0;
          const float ev = k + 1 < cnt ? el[src - 1] : 0.f;
          wave_lds_sync();
          if (k < cnt) t[src + s] = tv;
          if (k + 1 < cnt) el[src - 1 + s] = ev;
          wave_lds_sync();
        }
        at = q + 1;
        ab = p - 1 + s;
      }
      if (lane < s) {
        const uint32_t i = r ? s - 1 - lane : lane;
        t[at + lane] = (uint16_t)(i == 0 ? x0 : i == 1 ? x1 : x2);
      }
      wave_lds_sync();
      // the edges into, inside and out of the segment (positions at-1 .. at+s-1) and a -> b
      if (lane <= s + 1) {
        const uint32_t k = lane <= s ? at - 1 + lane : ab;
        el[k] = (OPEN && k == L - 1) ? 0.f : dist(t[k], t[k + 1 == L ? 0 : k + 1]);
      }
      wave_lds_sync();
      moved = true;
    }
    if (moved) ls_store<OPEN>(a, n, t, el);
  }
}

// ORO: the Or-opt kernel, else 2-opt
template <int SRC, bool OPEN, bool ORO>
void go(const LsArgs& a, hipStream_t s) {
  void (*k)(LsArgs);
  if constexpr (ORO) k = perm_oropt_kernel<SRC, OPEN>;
  else k = perm_ls_kernel<SRC, OPEN>;
  const size_t avail = allow_dynamic_lds((const void*)k);
  constexpr bool TBL = src_table(SRC);
  // the largest block whose waves' arrays fit beside the shared source
  uint32_t blk = 0;
  for (uint32_t b : {TBL ? 1024u : (uint32_t)kBlock, TBL ? 512u : 128u, TBL ? 256u : 64u})
    if (ls_lds_bytes(a.chunks, a.L, SRC, a.obj_aux_bytes, b / 64) <= avail) {
      blk = b;
      break;
    }
  if (blk == 0) {
    if constexpr (TBL) return go<SRC_L2, OPEN, ORO>(a, s);  // no room beside the table: the matrix through L2
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

template <bool OPEN, bool ORO>
void go_src(const LsArgs& a, hipStream_t s) {
  if (a.obj_aux && a.obj_aux_bytes % 16 == 0) {
    if (a.obj_aux_kind == 1) return go<SRC_TRI16, OPEN, ORO>(a, s);
    if (a.obj_aux_kind == 3) return go<SRC_TRI32, OPEN, ORO>(a, s);
    // the full u16 matrix of an asymmetric integer instance: Or-opt only (2-opt never sees one)
    if constexpr (ORO)
      if (a.obj_aux_kind == 2 && a.obj_aux_bytes >= 2ull * a.L * a.L) return go<SRC_FULL16, OPEN, ORO>(a, s);
  }
  go<SRC_L2, OPEN, ORO>(a, s);
}

template <bool ORO>
void go_objective(const LsArgs& a, hipStream_t s) {
  switch (a.objective) {
    case OBJ_TSP: go_src<false, ORO>(a, s); break;
    case OBJ_TSP_OPEN: go_src<true, ORO>(a, s); break;
    case OBJ_TSP_EUC: go<SRC_EUC, false, ORO>(a, s); break;
    default: throw std::invalid_argument("local search needs a TSP objective");
  }
}

}  // namespace

void perm_ls_launch(const LsArgs& a, hipStream_t s) {
  if (a.L > kPermMaxL)
    throw std::invalid_argument("local search: genome too long for the LDS-resident tour (" + std::to_string(a.L) +
                                " cities; at most " + std::to_string(kPermMaxL) + " on the GPU)");
  if (a.kind == LS_OR_OPT) go_objective<true>(a, s);
  else go_objective<false>(a, s);
  PGA_HIP_CHECK(hipGetLastError());
}

}  // namespace pga
