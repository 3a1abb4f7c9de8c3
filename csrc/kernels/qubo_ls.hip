// qubo_ls.hip — one-flip local search stage of the QUBO objective on gfx950
// (Island::local_search with BINARY / OBJ_QUBO; the semantics are
// qubo_ops.hpp, the CPU mirror is cpu_qubo.cpp qubo_local_search).
//
// One 64-lane wave per block; waves never synchronise with one another.  A
// wave walks the population in runs of 64 R individuals (R = 1 when everyone
// is selected, up to 4 for small shares, so that a share of 5 % still fills
// most of a tile): lane l draws the selection tests of individuals base + l,
// base + 64 + l, ..., one ballot each gives the run's selected set, and a run
// with nobody selected costs those Philox draws and nothing else.  The
// selected individuals are taken 16 at a time (a tile):
//
//   1. the tile's bit rows are staged in LDS and expanded to int8 A fragments
//      for all of K (as qubo.hip does; the same operand convention);
//   2. g = X (Q + Q^T) comes from the int8 matrix cores: per 16-column n-tile,
//      v_mfma_i32_16x16x64_i8 with the Q^T block and then the Q block as B
//      operands into ONE i32 accumulator (B fragments are 16-byte loads from
//      the two packed matrices, which stay L2-resident; a tile's loads are
//      issued together, one n-tile ahead of their MFMAs), stored to the wave's
//      g tile in LDS: [16][Lp + 4] i32 (the + 4 spreads the four row groups of
//      the C layout over the 32 banks of a ds_write_b32);
//   3. the tile's individuals then move four at a time, each on its own group
//      of 16 lanes that stride over the positions four at a time (one
//      ds_read_b128 of g per lane and step).  Per move: a u64 butterfly max of
//      one_flip_key over the group (ties to the smallest position by
//      construction), the group's first lane flips the bit in LDS, every lane
//      reads its 4 bytes of row p of Q and of Q^T, updates its own g entries
//      and rescans them for the next move -- O(Lp) per move, wave-level
//      synchronisation only, every individual stops after its own move count
//      (a move is a dependent chain -- butterfly, bit, two L2 row reads, g --
//      so four chains per wave run in the time of one);
//   4. a row that moved is written back with obj_f0 * (float)(int32) f,
//      f = (sum_p x_p g_p) / 2 exactly in i32 -- never from the stored float.
//
// No workspace in global memory.  Positions >= L never win (their matrix
// rows and columns are zero and the scan masks them), so the only data-
// dependent index, the flipped position, is < L whatever bits a forged row
// sets beyond L; those bits meet zero coefficients.
#include <hip/hip_runtime.h>

#include "pga/device.hpp"
#include "pga/ops.hpp"
#include "pga/qubo_ops.hpp"

namespace pga {
namespace {

using namespace dev;
typedef int v4i __attribute__((ext_vector_type(4)));

// 16 bits -> 16 int8 {0,1}: byte j of the 16-byte result = bit j (qubo.hip)
__device__ __forceinline__ v4i expand16(uint32_t h) {
  v4i r;
  r[0] = (int)(((h & 0xFu) * 0x00204081u) & 0x01010101u);
  r[1] = (int)((((h >> 4) & 0xFu) * 0x00204081u) & 0x01010101u);
  r[2] = (int)((((h >> 8) & 0xFu) * 0x00204081u) & 0x01010101u);
  r[3] = (int)((((h >> 12) & 0xFu) * 0x00204081u) & 0x01010101u);
  return r;
}
// signed byte e of a word
__device__ __forceinline__ int32_t sbyte(uint32_t w, int e) { return (int32_t)(int8_t)(w >> (8 * e)); }

constexpr uint32_t kTile = 16;  // individuals per MFMA tile
__host__ __device__ constexpr uint32_t ls_grow(uint32_t Lp) { return Lp + 4u; }       // g row stride (i32)
__host__ __device__ constexpr uint32_t ls_brow(uint32_t Lp) { return Lp / 8u + 8u; }  // bit row stride (bytes)
__host__ __device__ constexpr size_t ls_lds_bytes(uint32_t Lp) {
  return (size_t)kTile * ls_grow(Lp) * 4u + (size_t)kTile * ls_brow(Lp) + Lp + kTile * 4u;
}

constexpr uint32_t kMaxRun = 4;  // a wave's run: up to 4 x 64 individuals

// max of a packed key / sum over an aligned group of 16 lanes (every lane of the wave calls)
__device__ __forceinline__ unsigned long long max16(unsigned long long v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const unsigned long long w = shfl_xor_u64(v, o);
    v = w > v ? w : v;
  }
  return v;
}

template <int KS>
__global__ __launch_bounds__(64) void qubo_ls_kernel(LsArgs a, uint32_t R) {
  constexpr uint32_t Lp = 64u * KS;       // padded genome bits
  constexpr uint32_t GROW = ls_grow(Lp), BROW = ls_brow(Lp);
  constexpr uint32_t WPR = Lp / 32u;      // 32-bit words per staged row
  constexpr uint32_t NQ = Lp / 4u;        // 4-position steps per row
  int32_t* gl = (int32_t*)pga_dyn_lds;                        // [16][GROW]
  unsigned char* bits = pga_dyn_lds + kTile * GROW * 4u;      // [16][BROW]
  unsigned char* diag = bits + kTile * BROW;                  // [Lp] q[p][p]
  uint32_t* sel = (uint32_t*)(diag + Lp);                     // [16] the tile's individuals

  const uint32_t lane = lane_id(), col = lane & 15u, g = lane >> 4;
  const uint32_t L = a.L, rw = a.row_words;
  const uint32_t wb = WPR < rw ? WPR : rw;  // row words that hold positions < Lp
  const int32_t sgn = one_flip_sign(a.obj_f0);
  uint32_t* rows = (uint32_t*)a.rows;
  const int8_t* __restrict__ qt = a.qubo_qt;
  const int8_t* __restrict__ qn = a.qubo_qn;

  for (uint32_t p = lane; p < Lp; p += 64) diag[p] = (unsigned char)qn[(size_t)p * Lp + p];
  wave_lds_sync();

  // gains of the lane's positions q, q + 16, ... of the row (gc, bc): the lane's best key
  const auto scan = [&](const int32_t* gc, const unsigned char* bc) -> unsigned long long {
    unsigned long long key = 0ull;
#pragma unroll 4
    for (uint32_t q = col; q < NQ; q += 16) {
      const v4i gv = *(const v4i*)(gc + 4u * q);
      const uint32_t xb = *(const uint32_t*)(bc + 4u * (q >> 3)) >> (4u * (q & 7u));
      const uint32_t dg = *(const uint32_t*)(diag + 4u * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t p = 4u * q + (uint32_t)e;
        const int32_t gain = sgn * one_flip_delta((int32_t)((xb >> e) & 1u), gv[e], sbyte(dg, e));
        const unsigned long long k = p < L ? one_flip_key(gain, p) : 0ull;
        key = k > key ? k : key;
      }
    }
    return key;
  };

  const uint64_t run = 64ull * R;
  for (uint64_t base = (uint64_t)blockIdx.x * run; base < a.S; base += (uint64_t)gridDim.x * run) {
    // the run's selected individuals, numbered in index order
    uint32_t rk[kMaxRun], cnt = 0;
    bool pk[kMaxRun];
#pragma unroll
    for (uint32_t k = 0; k < kMaxRun; ++k) {
      bool pick = false;
      if (k < R) {  // wave-uniform
        const uint64_t me = base + 64u * k + lane;
        pick = me < a.S && ls_selected(a, me);
      }
      const unsigned long long mask = __ballot(pick);
      pk[k] = pick;
      rk[k] = cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      cnt += (uint32_t)__popcll(mask);
    }
    if (cnt == 0) continue;  // nobody selected: the draws and nothing else

    for (uint32_t r0 = 0; r0 < cnt; r0 += kTile) {  // tiles of the run's selected individuals
      const uint32_t m = cnt - r0 < kTile ? cnt - r0 : kTile;
      wave_lds_sync();  // the previous tile is done with sel / bits / gl
#pragma unroll
      for (uint32_t k = 0; k < kMaxRun; ++k)
        if (pk[k] && rk[k] >= r0 && rk[k] < r0 + kTile) sel[rk[k] - r0] = (uint32_t)(base + 64u * k + lane);
      wave_lds_sync();
      for (uint32_t i = lane; i < kTile * WPR; i += 64) {
        const uint32_t c = i / WPR, w = i % WPR;
        const uint32_t v = (c < m && w < rw) ? rows[(uint64_t)sel[c] * rw + w] : 0u;
        *(uint32_t*)(bits + c * BROW + 4u * w) = v;
      }
      wave_lds_sync();

      // ---- g = X (Q + Q^T) on the matrix cores ----
      {
        v4i A[KS];
        const unsigned char* br = bits + col * BROW;
#pragma unroll
        for (int s = 0; s < KS; ++s) A[s] = expand16(*(const uint16_t*)(br + 8u * s + 2u * g));
        // B fragments of n-tile nt: column n of Q (sum_k x_k q[k][n]) from qt,
        // row n of Q (sum_k x_k q[n][k]) from qn.  All 2 KS loads of a tile are
        // issued together, one tile ahead of the MFMAs that use them: with
        // one or two waves per SIMD nothing else hides their L2 latency
        const auto load_b = [&](v4i (&B)[2 * KS], uint32_t nt) {
          const size_t off = (size_t)(16u * nt + col) * Lp + 16u * g;
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            B[2 * s] = *(const v4i*)(qt + off + 64u * s);
            B[2 * s + 1] = *(const v4i*)(qn + off + 64u * s);
          }
        };
        v4i Bc[2 * KS], Bn[2 * KS];
        load_b(Bc, 0);
#pragma unroll 2
        for (uint32_t nt = 0; nt < Lp / 16u; ++nt) {
          if (nt + 1 < Lp / 16u) load_b(Bn, nt + 1);
          v4i acc = v4i{0, 0, 0, 0};
#pragma unroll
          for (int s = 0; s < 2 * KS; ++s) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[s / 2], Bc[s], acc, 0, 0, 0);
#pragma unroll
          for (int s = 0; s < 2 * KS; ++s) Bc[s] = Bn[s];
          // C layout: acc[i] = tile row 4 g + i, column 16 nt + col
#pragma unroll
          for (int i = 0; i < 4; ++i) gl[(4u * g + (uint32_t)i) * GROW + 16u * nt + col] = acc[i];
        }
      }
      wave_lds_sync();

      // ---- moves: four individuals at a time, lane group g (16 lanes) owns individual c0 + g.
      // Branches on valid / alive / moved are group-uniform; everything that
      // shuffles or synchronises runs in wave-uniform control flow ----
      for (uint32_t c0 = 0; c0 < m; c0 += 4) {
        const bool valid = c0 + g < m;
        const uint32_t c = valid ? c0 + g : c0;  // (an idle group addresses a live row and never writes)
        int32_t* gc = gl + c * GROW;
        unsigned char* bc = bits + c * BROW;
        unsigned long long key = max16(valid ? scan(gc, bc) : 0ull);
        bool moved = false;
        for (uint32_t mv = 0; mv < a.moves; ++mv) {
          const bool alive = key != 0ull;  // 0: one-flip optimal (or idle)
          if (__ballot(alive) == 0ull) break;
          uint32_t p = one_flip_pos(key);
          p = p < L ? p : L - 1u;  // (alive: always; positions >= L are never candidates)
          uint32_t* word = (uint32_t*)(bc + 4u * (p >> 5));
          const uint32_t old = *word;
          const int32_t sg = 1 - 2 * (int32_t)((old >> (p & 31u)) & 1u);
          wave_lds_sync();
          if (alive && col == 0) *word = old ^ (1u << (p & 31u));
          wave_lds_sync();
          unsigned long long nk = 0ull;
          if (alive) {
            const size_t ro = (size_t)p * Lp;
#pragma unroll 4
            for (uint32_t q = col; q < NQ; q += 16) {  // the lane's own g entries
              const uint32_t r1 = *(const uint32_t*)(qn + ro + 4u * q);  // q[p][j]
              const uint32_t r2 = *(const uint32_t*)(qt + ro + 4u * q);  // q[j][p]
              v4i gv = *(const v4i*)(gc + 4u * q);
#pragma unroll
              for (int e = 0; e < 4; ++e) gv[e] += sg * (sbyte(r1, e) + sbyte(r2, e));
              *(v4i*)(gc + 4u * q) = gv;
            }
            nk = scan(gc, bc);  // reads back the lane's own entries only
            moved = true;
          }
          key = max16(nk);
        }

        int32_t f2 = 0;  // 2 f = sum_p x_p g_p
        if (moved)
          for (uint32_t q = col; q < NQ; q += 16) {
            const v4i gv = *(const v4i*)(gc + 4u * q);
            const uint32_t xb = *(const uint32_t*)(bc + 4u * (q >> 3)) >> (4u * (q & 7u));
#pragma unroll
            for (int e = 0; e < 4; ++e) f2 += ((xb >> e) & 1u) ? gv[e] : 0;
          }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) f2 += __shfl_xor(f2, o, 64);
        if (moved) {
          const uint64_t n = sel[c];
          for (uint32_t w = col; w < wb; w += 16) rows[n * rw + w] = *(const uint32_t*)(bc + 4u * w);
          if (col == 0) a.scores[n] = one_flip_score(a.obj_f0, f2);
        }
      }
    }
  }
}

template <int KS>
void go(const LsArgs& a, hipStream_t s) {
  auto k = qubo_ls_kernel<KS>;
  constexpr size_t lds = ls_lds_bytes(64u * KS);
  if (allow_dynamic_lds((const void*)k) < lds)
    throw std::invalid_argument("one-flip local search: the g tile does not fit the LDS of this device");
  // the run a wave draws at once: long enough that a share `prob` fills a 16-individual tile
  uint32_t R = 1;
  if (!a.always) {
    const double sel64 = 64.0 * (double)a.thresh / 4294967296.0;  // selected per 64 individuals
    R = sel64 * kMaxRun <= kTile ? kMaxRun : (uint32_t)((kTile + sel64 - 1e-9) / sel64);
    R = R < 1 ? 1 : (R > kMaxRun ? kMaxRun : R);
  }
  uint64_t cap = (uint64_t)device_cu_count() * occupancy_blocks((const void*)k, 64, lds);
  if (cap < 1) cap = 1;
  if (cap > kMaxGrid) cap = kMaxGrid;
  const uint64_t need = (a.S + 64ull * R - 1) / (64ull * R);
  hipLaunchKernelGGL(k, (uint32_t)(need < cap ? need : cap), 64, lds, s, a, R);
}

}  // namespace

void qubo_ls_launch(const LsArgs& a, hipStream_t s) {
  if (one_flip_sign(a.obj_f0) == 0)
    throw std::invalid_argument("one-flip local search: the QUBO score factor (obj_f0) must be non-zero");
  if (!a.qubo_qt || !a.qubo_qn) throw std::invalid_argument("one-flip local search: the packed QUBO matrices are not built");
  if (a.moves == 0) return;
  switch (qubo_padded_length(a.L)) {
    case 64: go<1>(a, s); break;
    case 128: go<2>(a, s); break;
    case 256: go<4>(a, s); break;
    case 512: go<8>(a, s); break;
    case 1024: go<16>(a, s); break;
    default: throw std::invalid_argument("QUBO objective supports genomes of at most 1024 bits");
  }
  PGA_HIP_CHECK(hipGetLastError());
}

}  // namespace pga
