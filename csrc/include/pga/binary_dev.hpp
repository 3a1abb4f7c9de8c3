// binary_dev.hpp — the BINARY encoding's device code (bit-packed rows, see
// csrc/kernels/binary.hip for the design): objective accumulators, the
// knapsack matrix-core evaluation, the sparse bit-flip samplers, the generic
// kernel and the hot two-phase generation kernel binary_gen_tp.  Included by
// binary.hip (the built-in objectives and the launchers) and by jitgen.hip
// (binary_gen_tp with a hipRTC-compiled user objective linked in, OBJ_JIT).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pga/device.hpp"
#include "pga/ops.hpp"
#include "pga/tp.hpp"

// The user objective of a fused JIT generation kernel (jitgen.hip): defined in
// the user's bitcode, LTO-linked with the kernel's bitcode and inlined
// (jit.cpp).  Never referenced by the built-in kernels.
// The row pointer is an LDS (address space 3) pointer: the child's row as the
// step just staged it next to its global store (see kJitStageSteps).
typedef __attribute__((address_space(3))) const unsigned int* pga_lds_words;
extern "C" __device__ float pga_user_objective(pga_lds_words words, unsigned int nbits, const float* data);

namespace pga {
// jitgen.hip instantiates the generation kernel with external linkage (a named
// namespace), so the kernel keeps a predictable symbol in the bitcode the JIT
// links against; everywhere else the device code stays TU-local
#ifdef PGA_JIT_GEN
namespace jitgen {
#else
namespace {
#endif

using namespace dev;


// per-lane objective accumulator over the chunks a lane owns
template <int OBJ>
struct BinObj {
  uint32_t u = 0;                 // ONEMAX / TRAP counts
  uint32_t first0 = 0xFFFFFFFFu;  // LEADING_ONES: first zero bit position
  float v = 0.f, w = 0.f;         // KNAPSACK

  __device__ __forceinline__ void add(const GenArgs& a, uint4 x, uint32_t c) {
    const uint32_t wd[4] = {x.x, x.y, x.z, x.w};
    if (OBJ == OBJ_ONEMAX) {
      u += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
    } else if (OBJ == OBJ_KNAPSACK) {
      const float* val = a.obj_data;
      const float* wt = a.obj_data + a.L;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t bits = wd[j];
        const uint32_t base = c * 128u + 32u * j;
        while (bits) {
          uint32_t b = __ffs(bits) - 1;
          bits &= bits - 1;
          v += val[base + b];
          w += wt[base + b];
        }
      }
    } else if (OBJ == OBJ_TRAP) {
      const uint32_t k = (uint32_t)a.obj_i;
      const uint32_t km = k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t base = c * 128u + 32u * j;
        for (uint32_t i = 0; i < 32u; i += k) {
          if (base + i + k > a.L) break;
          uint32_t ones = __popc((wd[j] >> i) & km);
          u += ones == k ? k : (k - 1 - ones);
        }
      }
    } else if (OBJ == OBJ_LEADING_ONES) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t inv = ~wd[j];
        if (inv != 0u) {
          uint32_t p = c * 128u + 32u * j + (__ffs(inv) - 1);
          first0 = p < first0 ? p : first0;
          break;
        }
      }
    }
  }

  template <int GS>
  __device__ __forceinline__ float finish(const GenArgs& a) {
    if (OBJ == OBJ_ONEMAX || OBJ == OBJ_TRAP) return (float)group_sum_u<GS>(u);
    if (OBJ == OBJ_KNAPSACK) {
      float vv = group_sum<GS>(v), ww = group_sum<GS>(w);
      return ww <= a.obj_f0 ? vv : a.obj_f0 - ww;
    }
    if (OBJ == OBJ_LEADING_ONES) {
      uint32_t m = group_min_u<GS>(first0);
      return (float)(m < a.L ? m : a.L);
    }
    return 0.f;
  }
};

__device__ __forceinline__ uint4 u4(u32x4 v) { return make_uint4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ uint4 and4(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }
__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ uint4 mix4(uint4 a, uint4 b, uint4 m) {  // a where m, else b
  return make_uint4((a.x & m.x) | (b.x & ~m.x), (a.y & m.y) | (b.y & ~m.y), (a.z & m.z) | (b.z & ~m.z),
                    (a.w & m.w) | (b.w & ~m.w));
}
__device__ __forceinline__ uint4 range_keep_a(uint32_t c, uint32_t lo, uint32_t hi) {  // 1 = bit from A
  const uint32_t b0 = c * 128u;
  return make_uint4(~range_mask32(b0, lo, hi), ~range_mask32(b0 + 32, lo, hi), ~range_mask32(b0 + 64, lo, hi),
                    ~range_mask32(b0 + 96, lo, hi));
}
__device__ __forceinline__ uint4 bit4(uint32_t b) {  // one bit of a 128-bit chunk
  const uint32_t m = 1u << (b & 31u), j = b >> 5;
  return make_uint4(j == 0 ? m : 0u, j == 1 ? m : 0u, j == 2 ? m : 0u, j == 3 ? m : 0u);
}
__device__ __forceinline__ uint32_t chunk_len(uint32_t L, uint32_t c) {
  const uint32_t b = c * 128u;
  return L - b >= 128u ? 128u : L - b;
}

// ---------------------------------------------------------------------------
// 0/1 knapsack on the matrix cores (the hot kernel's evaluation when the
// instance is integer-exact, see build_knap_table).
//
// score needs V = bits . values and W = bits . weights per child.  A wave's
// step holds its NG children as 64 16-byte chunks (lane = g*GS + q), staged
// in its LDS scratch as 16 "virtual rows" of 512 bits: virtual row m = the
// chunks of lanes 4m..4m+3 = part r = m % R (R = GS/4) of child m / R.  One
// v_mfma_i32_16x16x64_i8 per 64-bit slice s (8 slices):
//   A[m][k] = bit k of virtual row m (expanded to int8 0/1),
//   B[k][c] = digit d of quantity qty (values | weights) of the gene bit k of
//             part r stands for, column c = (2r + qty) * D + d,
// with balanced base-256 digits in [-128, 127] (D <= 4), so C[m][c] is an
// exact partial dot product in i32 and only the columns of row m's own part
// are used:  V = sum_r sum_d C[gR + r][2rD + d] 256^d  (W: qty = 1).
// The element order inside a slice (element j of lane group h <-> bit 16h + j
// of the slice's 64) is the same for A and B, so the hardware's internal k
// permutation cannot matter; the integer result equals the CPU backend's
// float sum bit for bit (every partial sum is an integer below 2^24).
// Reference: test2/test.cu:28-36 (the knapsack objective); SURVEY.md C10.
// ---------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
constexpr int kObjKnapMfma = 1000;  // launcher-only objective id: OBJ_KNAPSACK via knap_mfma
constexpr uint32_t kKnapSlices = 8;  // 512-bit virtual row / 64-bit MFMA k-step
constexpr uint32_t kKnapMaxCols = 16;

__device__ __forceinline__ v4i expand16(uint32_t h) {  // 16 bits -> 16 int8 {0,1}
  v4i r;
  r[0] = (int)(__umul24(h & 0xFu, 0x00204081u) & 0x01010101u);
  r[1] = (int)(__umul24((h >> 4) & 0xFu, 0x00204081u) & 0x01010101u);
  r[2] = (int)(__umul24((h >> 8) & 0xFu, 0x00204081u) & 0x01010101u);
  r[3] = (int)(__umul24((h >> 12) & 0xFu, 0x00204081u) & 0x01010101u);
  return r;
}

// chunk slot of lane 4m + h in the wave scratch: virtual row m, lane group h,
// XOR-swizzled so that both the lane-order store and the (h, n) fragment
// read touch 8 distinct 16-byte bank groups per 8 lanes
__device__ __forceinline__ uint32_t knap_slot(uint32_t m, uint32_t h) { return 4u * m + (h ^ ((m >> 1) & 3u)); }
constexpr uint32_t kKnapCStride = 20;  // ints per C column in the scratch (padded against bank conflicts)
constexpr uint32_t kKnapScratch = 16 * kKnapCStride / 4;  // uint4 per wave (>= 64 chunk slots)

// every lane of the wave calls this with its chunk `v` (zero if it holds
// none); returns the score of the lane's child.  scr: the wave's scratch
// (kKnapScratch uint4); tab: the digit table in LDS, [s][h][16 columns] x
// 16 B, columns >= knap_cols zero.
template <int GS>
__device__ __forceinline__ float knap_mfma(const GenArgs& a, uint4 v, uint32_t lane, uint32_t q, uint4* scr,
                                           const uint4* tab) {
  constexpr uint32_t R = GS / 4;
  const uint32_t D = a.knap_dig, NC = a.knap_cols;
  scr[knap_slot(lane >> 2, lane & 3u)] = v;
  wave_lds_sync();
  const uint32_t h = lane >> 4, n = lane & 15u;
  const uint4 x = scr[knap_slot(n, h)];  // A: virtual row n, lane group h's 128 bits
  const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
  const uint4* tb = tab + h * kKnapMaxCols + n;
  v4i acc = {0, 0, 0, 0};
#pragma unroll
  for (uint32_t s = 0; s < kKnapSlices; ++s) {
    const uint4 t = tb[s * 4u * kKnapMaxCols];
    const uint32_t bits = (s & 1u) ? (xs[s >> 1] >> 16) : (xs[s >> 1] & 0xFFFFu);
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(expand16(bits), v4i{(int)t.x, (int)t.y, (int)t.z, (int)t.w}, acc,
                                                0, 0, 0);
  }
  wave_lds_sync();
  int* cl = (int*)scr;  // C, column-major: [column n][row 4h + i], stride kKnapCStride
  *(v4i*)(cl + n * kKnapCStride + 4u * h) = acc;
  wave_lds_sync();
  const uint32_t g = lane / GS;
  uint32_t V = 0, W = 0;  // mod 2^32: exact, the true sums are below 2^24
  for (uint32_t e = q; e < NC; e += GS) {
    const uint32_t r = e / (2u * D), d = e % D;
    const uint32_t c = (uint32_t)cl[e * kKnapCStride + g * R + r] << (8u * d);
    if ((e / D) & 1u) W += c;
    else V += c;
  }
  const float vv = (float)(int)group_sum_u<GS>(V), ww = (float)(int)group_sum_u<GS>(W);
  return ww <= a.obj_f0 ? vv : a.obj_f0 - ww;
}

// Sparse bit-flip sampler, group-cooperative form: continue the sequence of
// mutation words at j with n distinct positions already flipped in fm (this
// lane's chunk q), until K distinct positions are flipped.  A candidate is a
// repeat iff its owner lane already has the bit: one ballot per candidate.
template <int GS, bool NH = false>
__device__ __forceinline__ uint4 sparse_continue(const GenArgs& a, uint64_t child, uint32_t K, uint32_t n, uint32_t j,
                                              uint4 fm, uint32_t q, uint32_t gbase) {
  u32x4 blk = draw<NH>(a.key, ST_BMUT, child, j >> 2);
  while (n < K) {  // group-uniform
    if ((j & 3u) == 0u) blk = draw<NH>(a.key, ST_BMUT, child, j >> 2);
    const uint32_t p = word_to_index(sel4(blk, j & 3u), a.L);
    ++j;
    const uint32_t b = p & 127u;
    const bool own = (p >> 7) == q;
    const uint32_t wd = sel4(u32x4{fm.x, fm.y, fm.z, fm.w}, b >> 5);
    unsigned long long bal = __ballot(own && ((wd >> (b & 31u)) & 1u));
    if (GS < 64) bal = (bal >> gbase) & ((1ull << GS) - 1ull);
    if (bal == 0ull) {
      if (own) fm = xor4(fm, bit4(b));
      ++n;
    }
  }
  return fm;
}

// Sparse bit-flip sampler, sequential form (the definition, cpu_ops.cpp
// sparse_positions): the first kk distinct word_to_index(mutation word j, L),
// packed as 16-bit positions (0xFFFF = none; positions are < kSparseMaxL);
// jn = the next unused word.
template <bool NH>
__device__ __forceinline__ uint4 sparse_seq(const RngKey& key, uint64_t child, uint32_t kk, uint32_t L, uint32_t& jn) {
  uint32_t w0 = 0xFFFFFFFFu, w1 = 0xFFFFFFFFu, w2 = 0xFFFFFFFFu, w3 = 0xFFFFFFFFu;
  uint32_t n = 0, j = 0;
  u32x4 blk{0, 0, 0, 0};
  while (n < kk) {
    if ((j & 3u) == 0u) blk = draw<NH>(key, ST_BMUT, child, j >> 2);
    const uint32_t p = word_to_index(sel4(blk, j & 3u), L);
    ++j;
    const bool seen = (w0 & 0xFFFFu) == p || (w0 >> 16) == p || (w1 & 0xFFFFu) == p || (w1 >> 16) == p ||
                      (w2 & 0xFFFFu) == p || (w2 >> 16) == p || (w3 & 0xFFFFu) == p || (w3 >> 16) == p;
    if (!seen) {
      const uint32_t sh = (n & 1u) * 16u, keep = ~(0xFFFFu << sh), v = p << sh, wi = n >> 1;
      w0 = wi == 0u ? (w0 & keep) | v : w0;
      w1 = wi == 1u ? (w1 & keep) | v : w1;
      w2 = wi == 2u ? (w2 & keep) | v : w2;
      w3 = wi == 3u ? (w3 & keep) | v : w3;
      ++n;
    }
  }
  jn = j;
  return make_uint4(w0, w1, w2, w3);
}

// ---------------------------------------------------------------------------
// Generic kernel: every mode, every operator, any genome length.
// ---------------------------------------------------------------------------
template <int GS, int OBJ, int MODE>
__global__ __launch_bounds__(kBlock) void binary_kernel(GenArgs a, unsigned long long* best_parts) {
  resolve_gen(a);
  __shared__ unsigned long long lds_red[kBlock / 64];
  __shared__ uint32_t lds_elite;
  __shared__ uint32_t lds_thr[kMutCap];

  const uint32_t lane = lane_id();
  const uint32_t q = lane & (GS - 1);
  const uint32_t gbase = lane & ~(uint32_t)(GS - 1);
  constexpr uint32_t GPB = kBlock / GS;
  const uint32_t g_in_block = threadIdx.x / GS;
  const uint64_t rs = a.row_words >> 2;  // row stride in uint4
  const uint4* cur = (const uint4*)a.cur;
  uint4* nxt = (uint4*)a.next;
  const uint32_t nchunks = a.chunks;
  const uint32_t L = a.L;
  constexpr bool MUTATES = MODE == MODE_GEN || MODE == MODE_MUTATE;
  constexpr bool EVALS = OBJ != OBJ_NONE && (MODE == MODE_GEN || MODE == MODE_INIT || MODE == MODE_EVAL);
  const bool bitflip = MUTATES && a.mutation == MUT_BIT_FLIP && a.mut_rate > 0.f;
  const bool sparse = bitflip && a.mut_sparse;
  const bool reset_one = MUTATES && a.mutation == MUT_RESET_ONE;

  if (MODE == MODE_GEN && a.n_elite > 0 && a.elite_idx == nullptr && blockIdx.x == 0) {
    unsigned long long b = block_reduce_parts(a.best_cur, a.n_best_cur, lds_red);
    if (threadIdx.x == 0) lds_elite = (uint32_t)best_index(b);
  }
  if (bitflip)
    for (uint32_t i = threadIdx.x; i < kMutCap; i += kBlock) lds_thr[i] = a.mut_thr[i];
  __syncthreads();

  unsigned long long my_best = 0;
  ScoreStats st;
  const uint64_t stride = (uint64_t)gridDim.x * GPB;
  for (uint64_t child = (uint64_t)blockIdx.x * GPB + g_in_block; child < a.S; child += stride) {
    float score = 0.f;
    {
      // elitism: child = copy of the elite row, re-evaluated like every child
      const bool elite = MODE == MODE_GEN && child < a.n_elite;
      uint32_t pa = 0, pb = 0;
      bool xo = false;
      uint32_t blo = 0, bhi = 0;  // ONE/TWO_POINT: bits [blo, bhi) come from parent B
      u32x4 misc{0, 0, 0, 0};
      if (MODE == MODE_GEN || MODE == MODE_CROSS || MODE == MODE_MUTATE) misc = bin_misc(a.key, child);
      if (elite) {
        pa = pb = a.elite_idx ? a.elite_idx[child] : lds_elite;
      } else if (MODE == MODE_GEN || MODE == MODE_CROSS) {
        st_select_parents(a, child, pa, pb);
        xo = a.crossover != XO_NONE && do_crossover(a, misc.x);
        if (a.crossover == XO_ONE_POINT) {
          blo = word_to_index(misc.y, L);
          bhi = L;
        } else if (a.crossover == XO_TWO_POINT) {
          uint32_t c1 = word_to_index(misc.y, L);
          uint32_t c2 = word_to_index(misc.z, L);
          blo = c1 < c2 ? c1 : c2;
          bhi = c1 < c2 ? c2 : c1;
        }
      }
      uint32_t rpos = 0xFFFFFFFFu;  // RESET_ONE: the one flipped bit
      if (reset_one && !elite && misc.w < a.mut_ind_thresh) rpos = word_to_index(bin_mut_word(a.key, child, 0), L);
      uint4 fm = make_uint4(0, 0, 0, 0);  // sparse bit-flip: flips of chunk q (L <= 8192: one chunk per lane)
      if (sparse && !elite) fm = sparse_continue<GS>(a, child, binom_count(misc.w, lds_thr), 0, 0, fm, q, gbase);

      BinObj<OBJ> acc;
      for (uint32_t c0 = 0; c0 < nchunks; c0 += GS) {  // group-uniform segment loop
        const uint32_t c = c0 + q;
        if (c >= nchunks) continue;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (MODE == MODE_INIT) {
          v = u4(draw(a.key, ST_INIT, child, c));
        } else if (MODE == MODE_EVAL || MODE == MODE_MUTATE) {
          v = cur[child * rs + c];
        } else {
          const uint4 A = cur[(uint64_t)pa * rs + c];
          if (xo) {
            const uint4 B = cur[(uint64_t)pb * rs + c];
            const uint4 m = a.crossover == XO_UNIFORM ? u4(draw(a.key, ST_XO, child, c)) : range_keep_a(c, blo, bhi);
            v = mix4(A, B, m);
          } else {
            v = A;
          }
        }
        if (c == nchunks - 1) v = and4(v, u4(a.last_mask));
        if (bitflip && !sparse && !elite) {
          v = xor4(v, u4(chunk_flip_mask(a, child, c, chunk_len(L, c), bin_chunk_mut_word(a.key, child, c), lds_thr)));
        } else if (sparse) {
          v = xor4(v, fm);
        } else if (reset_one && (rpos >> 7) == c) {
          v = xor4(v, bit4(rpos & 127u));
        }
        if (MODE != MODE_EVAL) nxt[child * rs + c] = v;
        if (EVALS) acc.add(a, v, c);
      }
      if (EVALS) score = acc.template finish<GS>(a);
    }
    if (EVALS && q == 0) {
      a.score_next[child] = score;
      if (a.key_next) a.key_next[child] = (uint16_t)score;
      const unsigned long long pb = pack_best(score, child);
      my_best = pb > my_best ? pb : my_best;
      st.add(score);
    }
  }
  if (EVALS && best_parts) {
    unsigned long long b = block_max_u64(my_best, lds_red);
    if (threadIdx.x == 0) best_parts[blockIdx.x] = b;
    if (a.stats_parts) block_stats_store(st, a.stats_parts);
  }
}

// ---------------------------------------------------------------------------
// The hot generation kernel: transposed tournaments.
//
// A wave breeds NG = 64/GS children per STEP (group g: child bs + i*NG + g).
// Steps come in BATCHES of GS steps = 64 children, and the per-child work
// that does not touch the genome runs transposed, one lane per child of a
// whole batch.  A block owns a contiguous share of the population
// (tp_block_range), in ROUNDS of at most tp_par_cap children, each in two
// phases:
//   TOURNAMENTS  SEGMENTS of up to kSegBatches batches pulled from an LDS
//                counter, one per wave at a time: one Philox block = the 4
//                contestants of a child, all 4 x kSegBatches key loads in
//                flight together, compare -> (parent A, parent B) of every
//                child of the segment in LDS, then the segment's ready flag
//                (linear ranking: two rank picks, two rank-order loads)
//   BREED        UNITS of U <= 64 children pulled from a second counter once
//                no segment is left (a unit waits for its segment's flag):
//                RESOLVE the misc block (crossover test, cut points,
//                mutation count K) and the sparse bit-flip positions (one
//                more block, first K distinct by a pairwise check) -> a
//                32-byte child RECORD in the wave's LDS ring (2 batches);
//                per step: XO mask Philox (one block per chunk), mix, flips,
//                popcount, group butterfly, stores.
//                Two loop forms (BREED below): the rotating three-set loop
//                with per-step score / key stores, and for the exact-key
//                objectives at GS 4 / 8 and full units the UNIT loop: GS
//                straight-line steps over four register sets, static
//                cursors, the scores transposed to one child per lane and
//                ONE epilogue per unit, and a wait for the next step's rows
//                before each step's arithmetic (-2.4 us at the headline).
//                TAIL (the GS 8 unit loop on the 16-wave launch): the last
//                GenArgs::tp_tail units of a round are owned by no wave.  The
//                wave that draws such a unit's ticket RESOLVEs it into
//                block-shared records behind the histogram bins and sets the
//                unit's flag; waves without an owned unit left pull the tail's
//                STEPS (NG children each) from a third counter, with the
//                rotating loop's three register sets, the same wait and the
//                per-step epilogue, and a wave leaves its last owned unit
//                with its first two tail steps' rows already in flight.  The
//                waves of a block then end within a step of each other
//                instead of within a unit (last-barrier wait 9.5 K -> 2.2 K
//                cycles; profiles/tail_steps.md).  125 VGPRs, 104 SGPRs,
//                scratch 0.
// Why two phases: the EA (L2 -> fabric) traffic is the bound (PMC: ~530 MB
// per generation at 1M x 1024 bits, ~5.7 TB/s).  Tournament keys are a 2 MB
// array read at random; interleaved with the row gathers, ~1/4 of the key
// reads missed the XCD's 4 MB L2 (a 128-B line each, ~1/4 of all EA bytes).
// At kernel start every wave is in its tournament phase, so the L2 holds
// little but key lines and the key reads cost ~2 MB of fabric per XCD.
// A child costs 3/64 of a Philox per lane for its child-level words, and
// mutation is a short loop over the record's positions instead of a
// divergent geometric search in every chunk.
// Why a counter: equal static shares per wave left the CU's youngest waves
// breeding alone for the last ~20 us (oldest-first issue, tp.hpp); pulled
// batches end every wave of a CU within about one batch of each other.
// ---------------------------------------------------------------------------

#ifdef PGA_TP_TIMING
// experiment builds only (tools/variants.sh): per-wave clocks of the two
// phases, wall-clock start / end, the XCD the wave ran on, and its waits at
// the FIRST round's first barrier (launch skew inside the block: on the
// critical path), at the later rounds' first barriers (they follow the
// previous round's last barrier at once) and at the rounds' last barriers (the
// block's tail: not on the critical path)
constexpr uint32_t kTpClkWords = 14;
__device__ unsigned long long pga_tp_clk[kMaxGrid * 4][kTpClkWords];
#endif

// kTpMaxElite (elites the fast kernel routes through its records),
// kSegBatches and the work units: tp.hpp

__device__ __forceinline__ uint32_t pos16(uint4 r1, uint32_t k) {  // k-th packed 16-bit position
  const uint32_t w = sel4(u32x4{r1.x, r1.y, r1.z, r1.w}, k >> 1);
  return (k & 1u) ? (w >> 16) : (w & 0xFFFFu);
}

template <int GS, int OBJ, bool FULL, bool DENSE>
__device__ __forceinline__ void binary_gen_tp_body(GenArgs a, unsigned long long* best_parts) {
  resolve_gen(a);
  const uint32_t NW = blockDim.x >> 6;  // 4 or 16 waves (tp_dyn_lds of the launch)
  constexpr uint32_t NG = 64 / GS;      // children per wave per step
  constexpr uint32_t PD = tp_prefetch_depth(GS);  // steps of parent rows in flight (tp.hpp)
  constexpr bool EVALS = OBJ != OBJ_NONE;
  // integer objectives tournament on their exact u16 keys (L2-resident)
  constexpr bool KEY = OBJ == OBJ_ONEMAX || OBJ == OBJ_LEADING_ONES || OBJ == OBJ_TRAP;
  // dynamic LDS: per wave 2 batches x 64 records x 32 B, then the round's
  // (parent A, parent B) of every child
  uint4(*lds_rec)[2][64][2] = (uint4(*)[2][64][2])pga_dyn_lds;
  uint2* lds_par = (uint2*)(pga_dyn_lds + NW * 4096u);
  __shared__ uint32_t lds_thr[kMutCap];
  __shared__ uint32_t lds_el[kTpMaxElite];  // elite sources
  __shared__ unsigned long long lds_red[kTpMaxWaves];
  __shared__ uint32_t lds_next;   // the round's next unbred unit
  __shared__ uint32_t lds_tnext;  // the round's next tournament segment
  __shared__ uint32_t lds_ready[kTpMaxSegs];  // per segment: its parents are in LDS
  // tail steps (TAIL below; the unit loop on the 16-wave launch only): the
  // round's next tail step, and per tail unit: its records are in LDS
  __shared__ uint32_t lds_tstep;
  __shared__ uint32_t lds_tready[kTpMaxTail];
  constexpr bool KMF = OBJ == kObjKnapMfma;
  __shared__ uint4 lds_kscr[KMF ? kTpMaxWaves : 1][kKnapScratch];      // knapsack: per-wave chunk / C scratch
  __shared__ uint4 lds_ktab[KMF ? kKnapSlices * 4 * kKnapMaxCols : 1];  // knapsack: digit table
  // JIT (a linked user objective): each step also stages its children's rows
  // in the wave's LDS slice (64 lanes x 16 B), and every kJitStageSteps steps
  // one lane per staged child runs the objective on its LDS row.  Reading the
  // rows back from global memory instead (round 3/4: once per unit) has to
  // wait for every load issued before it -- the parent rows in flight PD steps
  // ahead -- since vector memory counters retire in order: a drained pipeline
  // per unit (110.8 vs 89.8 us/gen); LDS reads wait on their own counter.
  constexpr bool JIT = OBJ == kObjJit;
  // fused key histogram (GenArgs::key_hist): an LDS histogram of the keys the
  // block writes, after the round's parents in dynamic LDS (the launcher adds
  // hist_bins words), flushed with one global atomic per non-empty bin
  constexpr bool HISTK = KEY && !JIT;
  // the breed loop unrolled per 64-child unit with the per-unit epilogue
  // (BREED below): the exact-key objectives at the group sizes whose unit (GS
  // steps, four register sets at PD = 2) unrolls into the instruction cache --
  // 16 steps are ~68 KB of code, and a partly unrolled unit measured slower
  constexpr bool UNITF = HISTK && PD == 2 && (GS == 4 || GS == 8);
  // the unit loop's TAIL steps (BREED below), at GS 8 only: at GS 4 (steps of 16
  // children, 4 per unit) they measured 0.3 us SLOWER at OneMax-512
  // (profiles/tail_steps_ab.txt), so those kernels compile without them
  constexpr bool TAILF = UNITF && GS == 8;

  const uint32_t lane = lane_id(), wid = threadIdx.x >> 6;
  const uint32_t q = lane & (GS - 1), gbase = lane & ~(uint32_t)(GS - 1), g = lane / GS;
  const uint4* cur = (const uint4*)a.cur;
  uint4* nxt = (uint4*)a.next;
  const uint32_t L = a.L, S = (uint32_t)a.S;
  // FULL: chunks == GS, every lane owns a chunk
  const bool have = FULL || q < a.chunks, last = q == a.chunks - 1;
  const uint32_t qq = have ? q : 0u;
  const uint32_t clen = have ? chunk_len(L, q) : 0u;
  const bool xo_on = a.crossover != XO_NONE;
  const bool range = a.crossover != XO_UNIFORM;  // ONE/TWO_POINT, or NONE (empty range)
  // DENSE: per-chunk geometric bit-flips; otherwise the record carries the
  // flip positions (sparse bit-flip, RESET_ONE, or none)
  const bool bitflip = a.mutation == MUT_BIT_FLIP && a.mut_rate > 0.f;
  const bool sparse = !DENSE && bitflip;
  const bool reset_one = !DENSE && a.mutation == MUT_RESET_ONE;
  const uint4 lmask = u4(a.last_mask);
  // Every row / score byte offset fits 32 bits (the launcher checks (S + pad)
  // rows < 4 GiB): uniform base + 32-bit lane offset, one VGPR per address
  const uint32_t rb = a.row_words * 4u;
#define ELEM(T, base, i) (*(T*)((char*)(base) + (uint32_t)(i) * (uint32_t)sizeof(T)))
#define ROW(base, row, ch) (*(uint4*)((char*)(base) + ((uint32_t)(row) * rb + (uint32_t)(ch) * 16u)))

  // this block's children [bbegin, bend) (tp.hpp)
  const uint32_t U = tp_unit(a, NG);  // children per breed unit (tp.hpp)
  const uint32_t nst = U / NG;        // steps of a unit
  uint32_t bbegin, bend;
  tp_block_range(S, U, bbegin, bend, a.tp_skew);
  const uint32_t pcap = tp_par_cap(NW);
  // JIT staging after the parents: kJitStageSteps KB per wave (jit.cpp adds it to the launch's LDS)
  uint4* lds_stage = (uint4*)(pga_dyn_lds + NW * 4096u + pcap * 8u) + wid * (kJitStageSteps * 64u);
  (void)lds_stage;
  uint32_t* lds_hist = (uint32_t*)(pga_dyn_lds + NW * 4096u + pcap * 8u);  // (never with the JIT staging)
  const bool hist = HISTK && (a.key_hist != nullptr || a.rank_counts != nullptr);  // block-uniform
  const uint32_t hmax = a.hist_bins - 1u;

  // The elite sources of children [0, n_elite) (n_elite <= kTpMaxElite, for
  // the block that holds any of them) and the mutation table are loaded by
  // wave 0 AFTER the round's first barrier and published by a flag that only
  // RESOLVE waits on: the tournaments never need them, and the barrier no
  // longer waits for their global round trips (nor block 0 for the reduction
  // of every block's best partial)
  __shared__ uint32_t lds_pro;  // 1: lds_el / lds_thr are loaded
  bool pro_ok = false;          // wave-uniform: this wave has seen lds_pro set
  if (KMF)
    for (uint32_t i = threadIdx.x; i < kKnapSlices * 4 * kKnapMaxCols; i += blockDim.x)
      lds_ktab[i] = ((const uint4*)a.knap_tab)[i];
  if (threadIdx.x == 0) lds_next = lds_tnext = lds_pro = 0;
  if (threadIdx.x < kTpMaxSegs) lds_ready[threadIdx.x] = 0;
  if constexpr (TAILF) {
    if (threadIdx.x == 0) lds_tstep = 0;
    if (threadIdx.x < kTpMaxTail) lds_tready[threadIdx.x] = 0;
  }
  if (hist) {
    for (uint32_t i = threadIdx.x; i < a.hist_bins; i += blockDim.x) lds_hist[i] = 0;
    if (a.hist_zero)  // a later generation's histogram starts from zero
      for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.hist_zero_words; i += gridDim.x * blockDim.x)
        a.hist_zero[i] = 0;
  }

  unsigned long long my_best = 0;
  ScoreStats st;
  uint4(*rec)[64][2] = lds_rec[wid];
  static_assert(sizeof(lds_rec[0]) >= kSegBatches * 64 * sizeof(uint4), "contestant staging");
#ifdef PGA_TP_TIMING
  const unsigned long long clk0 = clock64(), rt0 = wall_clock64();
  unsigned long long clk_t = 0, clk_b = 0, n_bred = 0, clk_spin = 0, clk_sync0 = 0, clk_syncn = 0, clk_sync1 = 0;
  unsigned long long clk_tail = 0, n_tail = 0, clk_tflag = 0;  // the tail loop: cycles, steps bred, waits on unit flags
#endif
  for (uint32_t rbeg = bbegin; rbeg < bend; rbeg += pcap) {  // block-uniform rounds
    const uint32_t rend = rbeg + pcap < bend ? rbeg + pcap : bend;  // the round's children
    const uint32_t nu = (rend - rbeg + U - 1) / U;                  // its units: U children each
    const uint32_t nseg = (rend - rbeg + kSegBatches * 64 - 1) / (kSegBatches * 64);  // its tournament segments
#ifdef PGA_TP_TIMING
    const unsigned long long clkS = clock64();
#endif
    __syncthreads();  // tables / counters visible; the previous round's records and parents released
#ifdef PGA_TP_TIMING
    const unsigned long long clkA = clock64();
    if (rbeg == bbegin) clk_sync0 += clkA - clkS;
    else clk_syncn += clkA - clkS;
#endif
    if (rbeg == bbegin && wid == 0) {  // wave-uniform: the prologue loads (lds_pro)
      uint32_t plane = lane;  // (the unit loop's kernels: opaque, as at the kernel's end)
      if constexpr (TAILF) asm volatile("" : "+v"(plane));
      if (a.n_elite > 0 && bbegin < a.n_elite) {
        if (a.elite_idx) {
          for (uint32_t i = plane; i < a.n_elite; i += 64) lds_el[i] = a.elite_idx[i];
        } else {
          const unsigned long long b = wave_reduce_parts(a.best_cur, a.n_best_cur);
          if (lane == 0) lds_el[0] = (uint32_t)best_index(b);
        }
      }
      if (bitflip)
        for (uint32_t i = plane; i < kMutCap; i += 64) lds_thr[i] = a.mut_thr[i];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      tp_flag_set(&lds_pro);
    }

    // TOURNAMENTS of the round, one segment of <= kSegBatches batches at a
    // time per wave, segments pulled from a counter: all key loads of a
    // segment in flight at once; the contestants wait in the wave's record
    // ring (free until it breeds).  A wave breeds as soon as no segment is
    // left; a unit's RESOLVE waits for its segment's flag (no block barrier)
    for (;;) {
      const uint32_t sg = tp_ticket(&lds_tnext, lane);
      if (sg >= nseg) break;
      const uint32_t begin = rbeg + sg * kSegBatches * 64u;
      const uint32_t end = begin + kSegBatches * 64u < rend ? begin + kSegBatches * 64u : rend;
      uint2* par = lds_par + sg * kSegBatches * 64u;
      // the contestants wait in the wave's record ring (4 x 64 x 16 B = its
      // 4 KiB, free until it breeds); every key load of the segment in flight
      // at once (tp.hpp, the one definition shared with real_gen_tp)
      tp_select_segment<KEY ? TP_KEY16 : TP_F32>(a, begin, end, lane, &rec[0][0][0], par);
      // publish: the segment's parents (this wave's LDS stores, in order)
      // before its flag
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      tp_flag_set(&lds_ready[sg]);
    }
    // several blocks per CU (the 4-wave grid): a barrier parks the waiting
    // waves (a flag spin would take issue slots from the other blocks' waves:
    // REAL at S = 100K, 36 -> 55 us/gen); one block per CU: the flags alone
    if (NW < kTpMaxWaves) __syncthreads();
#ifdef PGA_TP_TIMING
    const unsigned long long clkB = clock64();
    clk_t += clkB - clkA;
#endif

#ifdef PGA_TP_TIMING
#define PGA_TP_SPIN0 const unsigned long long sp0_ = clock64();
#define PGA_TP_SPIN1 clk_spin += clock64() - sp0_;
#else
#define PGA_TP_SPIN0
#define PGA_TP_SPIN1
#endif
    // RESOLVE: parents, crossover plan and flip positions of the round's unit
    // BI -> the records of ring slot SL (lanes past the unit: unused copies)
#define PGA_TP_RESOLVE_TO(US, UE, DST)                                                                         \
  {                                                                                                             \
    if (!pro_ok) { /* the prologue loads of wave 0 (once per wave) */                                          \
      while (__hip_atomic_load(&lds_pro, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u)                 \
        __builtin_amdgcn_s_sleep(1);                                                                            \
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");                                                    \
      pro_ok = true;                                                                                            \
    }                                                                                                           \
    const uint32_t tc = (US) + lane;                                                                            \
    const uint32_t cc = tc < (UE) ? tc : (UE) - 1;                                                              \
    /* its segment is done (wave-uniform spin, rare) */                                                         \
    const uint32_t sg_ = ((US) - rbeg) / (kSegBatches * 64u);                                                   \
    PGA_TP_SPIN0                                                                                                \
    while (__hip_atomic_load(&lds_ready[sg_], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u)            \
      __builtin_amdgcn_s_sleep(1);                                                                              \
    PGA_TP_SPIN1                                                                                                \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");                                                      \
    const uint2 pp = lds_par[cc - rbeg]; /* parents from the round's tournaments */                             \
    uint32_t pa = pp.x, pb = pp.y;                                                                              \
    const u32x4 misc = bin_misc<true>(a.key, cc);                                                               \
    const bool elite = tc < a.n_elite;                                                                          \
    const bool xo = !elite && xo_on && do_crossover(a, misc.x);                                                 \
    if (elite) pa = lds_el[tc];                                                                                 \
    pb = xo ? pb : pa;                                                                                          \
    uint32_t lo = 0, hi = 0;                                                                                    \
    if (range && xo) {                                                                                          \
      const uint32_t x1 = word_to_index(misc.y, L);                                                             \
      if (a.crossover == XO_ONE_POINT) {                                                                        \
        lo = x1;                                                                                                \
        hi = L;                                                                                                 \
      } else {                                                                                                  \
        const uint32_t x2 = word_to_index(misc.z, L);                                                           \
        lo = x1 < x2 ? x1 : x2;                                                                                 \
        hi = x1 < x2 ? x2 : x1;                                                                                 \
      }                                                                                                         \
    }                                                                                                           \
    uint32_t K = 0, jn = 0;                                                                                     \
    uint4 P = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);                                   \
    if (reset_one && !elite && misc.w < a.mut_ind_thresh) {                                                     \
      K = 1;                                                                                                    \
      P.x = word_to_index(bin_mut_word<true>(a.key, cc, 0), L) | 0xFFFF0000u;                                   \
    }                                                                                                           \
    if (sparse && !elite) {                                                                                     \
      K = binom_count(misc.w, lds_thr);                                                                         \
      if (K > 0u) {                                                                                             \
        const uint32_t kk = K < kRecPos ? K : kRecPos;                                                          \
        const u32x4 m0 = draw<true>(a.key, ST_BMUT, cc, 0);                                                     \
        const uint32_t c0 = word_to_index(m0.x, L), c1 = word_to_index(m0.y, L);                                \
        const uint32_t c2 = word_to_index(m0.z, L), c3 = word_to_index(m0.w, L);                                \
        /* common case: the first kk <= 4 candidates are distinct, hence the positions */                      \
        const bool slow = kk > 4u || (kk > 1u && c0 == c1) || (kk > 2u && (c2 == c0 || c2 == c1)) ||            \
                          (kk > 3u && (c3 == c0 || c3 == c1 || c3 == c2));                                      \
        P = make_uint4(c0 | (c1 << 16), c2 | (c3 << 16), 0xFFFFFFFFu, 0xFFFFFFFFu);                             \
        jn = kk;                                                                                                \
        if (slow) P = sparse_seq<true>(a.key, cc, kk, L, jn);                                                   \
      }                                                                                                         \
    }                                                                                                           \
    const uint32_t meta = (K > 255u ? 255u : K) | ((jn > 0xFFFFu ? 0xFFFFu : jn) << 8) | (elite ? 1u << 31 : 0u); \
    uint4(*r)[2] = (DST);                                                                                       \
    r[lane][0] = make_uint4(pa, pb, lo | (hi << 16), meta);                                                     \
    r[lane][1] = P;                                                                                             \
  }
#define PGA_TP_RESOLVE(US, UE, SL) PGA_TP_RESOLVE_TO(US, UE, rec[(SL)])

    // BREED: the round's units in ticket order from the block's counter, as
    // two cursors over the wave's sequence of steps: the LOAD cursor issues
    // the parent-row loads of the step PD steps ahead of the BREED cursor
    // (PD register sets in flight: the row gathers are latency-bound, so the
    // bytes in flight per wave set the throughput) and RESOLVEs a unit into
    // the other ring slot when it enters it (a full unit has U / NG >= PD
    // steps, so the breed cursor has left that slot by then).  Every vector
    // memory operation is unconditional (s_waitcnt vmcnt retires in order and
    // hipcc assumes the fewest outstanding loads over all paths, so a
    // conditionally issued load would make the next wait drain it): an
    // exhausted load cursor re-reads the breed cursor's rows.
    // NEXT unit [US, UE) of this wave (US = kNoUnit: none), from the block's
    // LDS counter.  Tickets [nown, nu) are the round's TAIL units (below): the
    // wave that draws one owes its RESOLVE (tpend) and owns none of its steps
    constexpr uint32_t kNoUnit = 0xFFFFFFFFu;
    // TAIL: the last tcap units of a round (nu - nown of them, ntst steps in
    // all; none: nown = nu) are bred step by step by whichever wave is free;
    // their records are block-shared, 2 KB per unit after the histogram bins
    // (the launcher sizes the launch for tp_tail units).  Worked out here, not
    // at the kernel's start: nothing of it is live across the tournaments
    const uint32_t tcap = TAILF && U == 64u && NW == kTpMaxWaves ? (a.tp_tail < kTpMaxTail ? a.tp_tail : kTpMaxTail) : 0u;
    const uint32_t nown = nu - (tcap < nu ? tcap : nu), ntst = (nu - nown) * (uint32_t)GS;
    const uint32_t toff = tp_tail_off(NW * 4096u + pcap * 8u + (hist ? 4u * a.hist_bins : 0u));
    uint4(*trec)[64][2] = (uint4(*)[64][2])(pga_dyn_lds + toff);
    (void)trec;
    uint32_t tpend = kNoUnit;  // the tail unit this wave drew and has not resolved yet
    (void)tpend;
#define PGA_TP_NEXT(US, UE)                                                                                 \
  {                                                                                                         \
    US = kNoUnit;                                                                                           \
    const uint32_t tk_ = tp_ticket(&lds_next, lane);                                                        \
    if (tk_ < nown) {                                                                                       \
      US = rbeg + tk_ * U;                                                                                  \
      UE = US + U < rend ? US + U : rend;                                                                   \
    } else if (TAILF && tk_ < nu) {                                                                         \
      tpend = tk_ - nown;                                                                                   \
    }                                                                                                       \
  }

    // TAIL (the GS 8 unit loop on the 16-wave launch, GenArgs::tp_tail > 0).  The
    // unit counter levels the block's waves only to within one unit (~28 K
    // cycles of a wave's ~114 K breed cycles at the headline), and a wave that
    // is done idles until the block's last barrier.  So the last ntst / GS
    // units of the round, in ticket order, are owned by no wave: whoever draws
    // such a unit's ticket RESOLVEs it into the block-shared records trec and
    // publishes lds_tready[unit] (fence, then flag, like a segment's flag), and
    // a wave without an owned unit left pulls the tail's STEPS one by one from
    // a third counter (step ticket t: unit t / GS, step t % GS), loads the
    // step's parent rows PD steps ahead as everywhere, breeds with the same
    // arithmetic and takes the per-step epilogue.  The RNG is keyed per child,
    // best is a max, the histogram is atomic adds and the statistics are
    // exact integer sums (the unit loop's bound), so who breeds a step does
    // not show in any output.
    // Progress.  A wave waits for lds_tready[u] only after it has seen u's
    // unit ticket drawn (lds_next counts past it), drawing tickets itself
    // until then and resolving each tail unit it draws BEFORE it waits for
    // anything (TSERVE).  The flag of u is thus always owed by a wave that has
    // drawn u's ticket and that, between the draw and the flag, runs nothing
    // but RESOLVE, whose own waits (lds_pro, the segment flags) are on waves in
    // their tournament phase, which wait on nothing.  No wave waits on a tail
    // flag before its own pending unit is published, so there is no cycle.
    // No wave resolves the tail alone either: the waves of the unit loop draw
    // one ticket per unit they enter, which hands the first tail units to up
    // to 16 different waves, and a wave in the tail loop draws at most one
    // more ticket per step it pulls while any is left.  Every spin sleeps.
    // The round's last barrier releases trec, lds_tstep and the flags.
#define PGA_TP_TPULL(TQ) TQ = tp_ticket(&lds_tstep, lane);
    // resolve the pending tail unit; draw until NEEDT unit tickets are drawn
    // (0: none needed), and one more if EAGER and any is left
#define PGA_TP_TSERVE(NEEDT, EAGER)                                                                         \
  {                                                                                                         \
    bool eg_ = (EAGER);                                                                                     \
    for (;;) {                                                                                              \
      if (tpend != kNoUnit) {                                                                               \
        const uint32_t ts_ = rbeg + (nown + tpend) * 64u;                                                   \
        const uint32_t te_ = ts_ + 64u < rend ? ts_ + 64u : rend;                                           \
        PGA_TP_RESOLVE_TO(ts_, te_, trec[tpend])                                                            \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");                                              \
        tp_flag_set(&lds_tready[tpend]);                                                                    \
        tpend = kNoUnit;                                                                                    \
      }                                                                                                     \
      const uint32_t d_ = __builtin_amdgcn_readfirstlane(__hip_atomic_load(                                 \
                              &lds_next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >> 6;             \
      if (d_ >= (NEEDT) && !(eg_ && d_ < nu)) break;                                                        \
      eg_ = false;                                                                                          \
      const uint32_t tk_ = tp_ticket(&lds_next, lane);                                                      \
      if (tk_ >= nown && tk_ < nu) tpend = tk_ - nown;                                                      \
    }                                                                                                       \
  }
    // unit tickets that must be drawn before step ticket TQ can be waited for
#define PGA_TP_TNEED(TQ) ((TQ) < ntst ? nown + (TQ) / (uint32_t)GS + 1u : 0u)
    // wait for the records of step ticket TQ's unit (wave-uniform spin)
#define PGA_TP_TWAIT(TQ)                                                                                    \
  if ((TQ) < ntst) {                                                                                        \
    PGA_TP_TSPIN0                                                                                           \
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&lds_tready[(TQ) / (uint32_t)GS], __ATOMIC_RELAXED, \
                                                             __HIP_MEMORY_SCOPE_WORKGROUP)) == 0u)          \
      __builtin_amdgcn_s_sleep(1);                                                                          \
    PGA_TP_TSPIN1                                                                                           \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");                                                  \
  }
#ifdef PGA_TP_TIMING
#define PGA_TP_TSPIN0 const unsigned long long tsp0_ = clock64();
#define PGA_TP_TSPIN1 clk_tflag += clock64() - tsp0_;
#else
#define PGA_TP_TSPIN0
#define PGA_TP_TSPIN1
#endif

    uint32_t ns, ne = 0;  // the wave's next unit (prefetched ticket)
    PGA_TP_NEXT(ns, ne)
    const bool own = ns != kNoUnit;  // the wave drew an owned unit
    const bool tailm = TAILF && U == 64u && ntst > 0u;  // the round has tail steps
    if (own || tailm) {
      // breed cursor: ring slot, step and its unit [bs, be).  Every unit
      // takes its full nst = U / NG steps, a partial one (only ever at S)
      // too: its children past S write the padding rows, and a unit never
      // holds fewer steps than the PD the load cursor runs ahead
      uint32_t slot = 0, i = 0, bs = ns, be = ne;
      if (own) {
        PGA_TP_NEXT(ns, ne)
        PGA_TP_RESOLVE(bs, be, 0u)
      }
      // load cursor of the rotating loop; lpend: at the end of its unit with
      // unit ns next; lmore = false: past the wave's last step
      uint32_t lslot = 0, li = 0, lbs = bs, lbe = be;
      bool lpend = false, lmore = true, done = false;

      // LOAD the parent rows of the load cursor's step into (YA, YB) and
      // advance it
#define PGA_TP_LOAD(YA, YB)                                                                                 \
  {                                                                                                         \
    if (lpend) { /* entering the next unit */                                                               \
      PGA_TP_RESOLVE(ns, ne, lslot ^ 1u)                                                                    \
      lslot ^= 1u;                                                                                          \
      li = 0;                                                                                               \
      lbs = ns;                                                                                             \
      lbe = ne;                                                                                             \
      lpend = false;                                                                                        \
      PGA_TP_NEXT(ns, ne)                                                                                   \
    }                                                                                                       \
    const uint4 r = rec[lmore ? lslot : slot][(lmore ? li : i) * NG + g][0];                                \
    YA = ROW(cur, r.x, qq);                                                                                 \
    YB = ROW(cur, r.y, qq);                                                                                 \
    if (lmore && ++li == nst) {                                                                             \
      lpend = ns != kNoUnit;                                                                                \
      lmore = lpend;                                                                                        \
    }                                                                                                       \
  }

      // BREED step I of the breed cursor's unit from the parent rows (XA, XB):
      // child c = bs + I * NG + g, its row v stored, its score sc (uniform
      // over the group's lanes; JIT: evaluated later).  Children past S, at
      // the population's end only, write the padding rows.  R: the unit's
      // records (the wave's ring slot, or a tail unit's shared ones).  Shared
      // by the loop forms; c, v and sc stay in the enclosing scope.
#define PGA_TP_BREED(XA, XB, I, R)                                                                          \
    const uint32_t c = bs + (I) * NG + g;                                                                   \
    const uint4 r0 = (R)[(I) * NG + g][0];                                                                  \
    const uint32_t meta = r0.w;                                                                             \
    const uint4 m = range ? range_keep_a(q, r0.z & 0xFFFFu, r0.z >> 16) : u4(draw<true>(a.key, ST_XO, c, q)); \
    uint4 v = mix4(XA, XB, m);                                                                              \
    if (last) v = and4(v, lmask);                                                                           \
    uint4 fm = make_uint4(0, 0, 0, 0);                                                                      \
    if (DENSE) {                                                                                            \
      if (bitflip && !(meta >> 31)) /* elites are not mutated */                                           \
        fm = u4(chunk_flip_mask(a, c, q, clen, bin_chunk_mut_word<true>(a.key, c, q), lds_thr));            \
    } else {                                                                                                \
      const uint32_t K = meta & 0xFFu;                                                                      \
      if (K > 0u) {                                                                                         \
        const uint4 r1 = (R)[(I) * NG + g][1];                                                              \
        const uint32_t kk = K < kRecPos ? K : kRecPos;                                                      \
        /* the first 4 unrolled (a loop here costs ~20 VGPRs of the whole kernel) */                       \
        _Pragma("unroll") for (uint32_t k = 0; k < 4; ++k) {                                               \
          const uint32_t p = pos16(r1, k);                                                                  \
          if (k < kk && (p >> 7) == q) fm = xor4(fm, bit4(p & 127u));                                       \
        }                                                                                                   \
        if (kk > 4u)                                                                                        \
          for (uint32_t k = 4; k < kk; ++k) {                                                               \
            const uint32_t p = pos16(r1, k);                                                                \
            if ((p >> 7) == q) fm = xor4(fm, bit4(p & 127u));                                              \
          }                                                                                                 \
        if (K > kRecPos) fm = sparse_continue<GS, true>(a, c, K, kRecPos, (meta >> 8) & 0xFFFFu, fm, q, gbase); \
      }                                                                                                     \
    }                                                                                                       \
    v = xor4(v, fm);                                                                                        \
    float sc;                                                                                               \
    if constexpr (KMF) {                                                                                    \
      sc = knap_mfma<GS>(a, have ? v : make_uint4(0, 0, 0, 0), lane, q, lds_kscr[wid], lds_ktab);            \
    } else if constexpr (JIT) {                                                                             \
      sc = 0.f; /* evaluated after the unit */                                                              \
    } else {                                                                                                \
      BinObj<OBJ> acc;                                                                                      \
      if (have) acc.add(a, v, q);                                                                           \
      sc = acc.template finish<GS>(a);                                                                      \
    }                                                                                                       \
    if (have) ROW(nxt, c, q) = v;

      // the per-STEP epilogue of child c: every lane of the group stores the
      // same score
#define PGA_TP_STEP_SCORE                                                                                   \
    if (EVALS && !JIT) {                                                                                    \
      ELEM(float, a.score_next, c) = sc;                                                                    \
      if (KEY) ELEM(uint16_t, a.key_next, c) = (uint16_t)sc;                                                \
      if (hist && q == 0u && c < S) {                                                                       \
        const uint32_t kb = (uint16_t)sc;                                                                   \
        __hip_atomic_fetch_add(&lds_hist[kb < hmax ? kb : hmax], 1u, __ATOMIC_RELAXED,                      \
                               __HIP_MEMORY_SCOPE_WORKGROUP);                                               \
      }                                                                                                     \
      const unsigned long long pk = c < S ? pack_best(sc, c) : 0ull;                                        \
      my_best = pk > my_best ? pk : my_best;                                                                \
      st.add_if(q == 0u && c < S, sc);                                                                      \
    }

      // one STEP of the rotating loop: load PD steps ahead into (YA, YB), breed
      // the breed cursor's step i from (XA, XB), advance the breed cursor
#define PGA_TP_STEP(XA, XB, YA, YB)                                                                         \
  {                                                                                                         \
    PGA_TP_LOAD(YA, YB)                                                                                     \
    PGA_TP_BREED(XA, XB, i, rec[slot])                                                                      \
    if constexpr (JIT) {                                                                                    \
      lds_stage[(i % kJitStageSteps) * 64u + lane] = v;                                                     \
      if (i % kJitStageSteps == kJitStageSteps - 1u || i + 1u == nst) PGA_TP_JIT_EVAL                       \
    }                                                                                                       \
    PGA_TP_STEP_SCORE                                                                                       \
    if (++i == nst) {                                                                                       \
      PGA_TP_COUNT                                                                                          \
      if (lbs == bs) { /* the load cursor never left this unit: it was the wave's last */                   \
        done = true;                                                                                        \
      } else {                                                                                              \
        slot ^= 1u;                                                                                         \
        i = 0;                                                                                              \
        bs = lbs;                                                                                           \
        be = lbe;                                                                                           \
      }                                                                                                     \
    }                                                                                                       \
  }

      // JIT: the staged steps s0..i of the unit, child j = lane (step s0 + j / NG,
      // group j % NG); the wavefront fences keep the compiler from moving LDS
      // accesses across (one wave's LDS operations execute in order)
#define PGA_TP_JIT_EVAL                                                                                     \
  {                                                                                                         \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                  \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                                                  \
    const uint32_t s0 = i - i % kJitStageSteps, ns = i - s0 + 1u;                                           \
    const uint32_t cj = bs + s0 * NG + lane;                                                                \
    if (lane < ns * NG && cj < be) {                                                                        \
      const uint32_t js = lane / NG, jg = lane % NG;                                                        \
      const float sj = pga_user_objective((pga_lds_words)(lds_stage + js * 64u + jg * GS), L, a.obj_data);  \
      ELEM(float, a.score_next, cj) = sj;                                                                   \
      my_best = pack_best(sj, cj) > my_best ? pack_best(sj, cj) : my_best;                                  \
      st.add(sj);                                                                                           \
    }                                                                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                  \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                                                  \
  }
#ifdef PGA_TP_TIMING
#define PGA_TP_COUNT n_bred += be - bs;
#define PGA_TP_TCOUNT n_bred += NG, n_tail += 1;
#else
#define PGA_TP_COUNT
#define PGA_TP_TCOUNT
#endif

      // one step I of the UNIT loop (full units: GS steps, the load cursor a
      // static PD steps ahead; the exact-key objectives only, UNITF): the loads
      // of step I + PD into (YA, YB) -- from step GS - PD on in the wave's next
      // unit, RESOLVEd into the other ring slot there, once; a wave without
      // one loads its first PD TAIL steps' rows there instead, so that it goes
      // over to the tail loop with its loads in flight, or, with no tail step
      // left either, re-reads its own step's rows -- then breed step I from (XA, XB)
      // and move the group's score to lane I * NG + group (one ds_bpermute and
      // a select); nothing but the row is stored per step.
      // Before the arithmetic the step waits until the rows of step I + 1
      // (NA, NB) have landed too (an empty asm reads them): while a wave
      // computes, one pair of row loads is in flight, not two.  The fabric is
      // the bound, and holding the second pair back measured 2.4 us per
      // generation faster at the headline (docs/ARCHITECTURE.md, section 4).
#define PGA_TP_USTEP(I, XA, XB, YA, YB, NA, NB)                                                             \
  {                                                                                                         \
    const uint32_t ul_ = (I) + PD;                                                                          \
    if (ul_ == (uint32_t)GS) { /* wave-uniform; no vector memory operation inside */                        \
      hn = ns != kNoUnit;                                                                                   \
      if (hn) {                                                                                             \
        PGA_TP_RESOLVE(ns, ne, slot ^ 1u)                                                                   \
        nbs = ns;                                                                                           \
        nbe = ne;                                                                                           \
        PGA_TP_NEXT(ns, ne)                                                                                 \
      }                                                                                                     \
      /* TAIL, at most twice per wave and round (unlikely: laid out outside the unit's straight line): */  \
      /* a tail unit the ticket above drew, or, without a next unit, the hand-over: the first PD tail  */  \
      /* steps take the load cursor's place                                                            */  \
      if (__builtin_expect(tailm && (!hn || tpend != kNoUnit), 0)) {                                        \
        if (!hn) {                                                                                          \
          PGA_TP_TPULL(tq0)                                                                                 \
          PGA_TP_TPULL(tq1)                                                                                 \
        }                                                                                                   \
        const uint32_t tqm_ = tq1 < ntst ? tq1 : tq0;                                                       \
        PGA_TP_TSERVE(hn ? 0u : PGA_TP_TNEED(tqm_), false)                                                  \
        if (!hn) {                                                                                          \
          PGA_TP_TWAIT(tq0)                                                                                 \
          PGA_TP_TWAIT(tq1)                                                                                 \
          /* where the two steps' records start in LDS (uniform), so that the loads below take a select */ \
          /* and the unit stays one straight line                                                        */ \
          uo0 = tq0 < ntst ? toff + tq0 / (uint32_t)GS * kTpTailUnitBytes + tq0 % (uint32_t)GS * (NG * 32u) : kNoUnit; \
          uo1 = tq1 < ntst ? toff + tq1 / (uint32_t)GS * kTpTailUnitBytes + tq1 % (uint32_t)GS * (NG * 32u) : kNoUnit; \
        }                                                                                                   \
      }                                                                                                     \
    }                                                                                                       \
    const bool un_ = ul_ >= (uint32_t)GS;                                                                   \
    const uint4* up_ = &rec[un_ && hn ? slot ^ 1u : slot][(un_ ? (hn ? ul_ - GS : (I)) : ul_) * NG + g][0]; \
    if (un_) { /* (compile time) the hand-over: a tail step's records */                                    \
      const uint32_t uo_ = ul_ == (uint32_t)GS ? uo0 : uo1;                                                 \
      up_ = uo_ != kNoUnit ? (const uint4*)(pga_dyn_lds + (uo_ + g * 32u)) : up_;                           \
    }                                                                                                       \
    const uint4 ur_ = *up_;                                                                                 \
    YA = ROW(cur, ur_.x, qq);                                                                               \
    YB = ROW(cur, ur_.y, qq);                                                                               \
    {                                                                                                       \
      const uint32_t w_ = NA.x | NB.x;                                                                      \
      asm volatile("" ::"v"(w_));                                                                           \
    }                                                                                                       \
    PGA_TP_BREED(XA, XB, I, rec[slot])                                                                      \
    const float t_ = __shfl(sc, (int)usrc, 64);                                                             \
    usc = lane / NG == (I) ? t_ : usc;                                                                      \
  }

      uint4 A0, B0, A1, B1, A2, B2, A3, B3;  // PD + 1 register sets, rotated statically (the unit loop: 4)
      (void)A2; (void)B2; (void)A3; (void)B3;
      if (UNITF && U == 64u) {  // full units of GS steps (wave-uniform)
        // the unit's scores, one child per lane (child bs + lane), gathered
        // step by step from lane usrc, a lane of group lane % NG
        float usc = 0.f;
        const uint32_t usrc = (lane % NG) * GS + lane / NG;
        // hn: the wave has a next unit [nbs, nbe), known once the load cursor
        // has left the current one
        bool hn = false;
        uint32_t nbs = 0, nbe = 0;
        // TAIL: the step tickets whose rows the register sets hold (>= ntst: none)
        uint32_t tq0 = kNoUnit, tq1 = kNoUnit, tq2 = kNoUnit;
        uint32_t uo0 = kNoUnit, uo1 = kNoUnit;  // the hand-over: LDS offsets of the records of tq0, tq1
        if (tailm) {
          // the tail unit a first ticket drew; a wave that owns no unit at all
          // starts with the tail's next PD steps.  (Its two pairs of row loads
          // below are the one place where a vector memory operation of this
          // kernel sits under a condition: once per wave and round, before the
          // loop and with nothing in flight that a merged wait could drain.)
          if (!own) {
            PGA_TP_TPULL(tq0)
            PGA_TP_TPULL(tq1)
          }
          const uint32_t tqm_ = tq1 < ntst ? tq1 : tq0;
          PGA_TP_TSERVE(PGA_TP_TNEED(tqm_), false)
          PGA_TP_TWAIT(tq0)
          PGA_TP_TWAIT(tq1)
          if (tq0 < ntst) {
            const uint32_t t1_ = tq1 < ntst ? tq1 : tq0;
            const uint4 r = trec[tq0 / (uint32_t)GS][(tq0 % (uint32_t)GS) * NG + g][0];
            A0 = ROW(cur, r.x, qq);
            B0 = ROW(cur, r.y, qq);
            const uint4 r1 = trec[t1_ / (uint32_t)GS][(t1_ % (uint32_t)GS) * NG + g][0];
            A1 = ROW(cur, r1.x, qq);
            B1 = ROW(cur, r1.y, qq);
          }
        }
        if (own) {
          {
            const uint4 r = rec[0][g][0];
            A0 = ROW(cur, r.x, qq);
            B0 = ROW(cur, r.y, qq);
          }
          {
            const uint4 r = rec[0][NG + g][0];
            A1 = ROW(cur, r.x, qq);
            B1 = ROW(cur, r.y, qq);
          }
          for (;;) {
#pragma unroll
            for (uint32_t u = 0; u < (uint32_t)GS; u += 4u) {  // one rotation of the four register sets
              PGA_TP_USTEP(u, A0, B0, A2, B2, A1, B1)
              PGA_TP_USTEP(u + 1u, A1, B1, A3, B3, A2, B2)
              PGA_TP_USTEP(u + 2u, A2, B2, A0, B0, A3, B3)
              PGA_TP_USTEP(u + 3u, A3, B3, A1, B1, A0, B0)
            }
            // The unit's epilogue, once per child: lane j holds the score of
            // child bs + j.  Statistics: every lane now adds one child per unit
            // where lane q == 0 of a group added GS.  The scores are
            // non-negative integers (exact keys, <= 65535), so every per-lane,
            // per-wave and per-block partial sum is bounded by the block's
            // total; while that is below 2^24 all of them are exact in f32 and
            // the block's {min, sum} equals the rotating loop's bit for bit.
            // Above it (a block share x mean score >= 2^24: from S ~ 8 M at
            // L = 1024 on 256 CUs) the rotating loop's sum already depends on
            // which wave pulled which unit, i.e. it differs from run to run;
            // the launcher's users that need exact sums check the same bound
            // (roulette_fused_launch).
            {
              const uint32_t c = bs + lane;
              ELEM(float, a.score_next, c) = usc;
              ELEM(uint16_t, a.key_next, c) = (uint16_t)usc;
              if (hist && c < S) {
                const uint32_t kb = (uint16_t)usc;
                __hip_atomic_fetch_add(&lds_hist[kb < hmax ? kb : hmax], 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
              }
              const unsigned long long pk = c < S ? pack_best(usc, c) : 0ull;
              my_best = pk > my_best ? pk : my_best;
              st.add_if(c < S, usc);
            }
            PGA_TP_COUNT
            if (!hn) break;  // the load cursor never left this unit: it was the wave's last
            slot ^= 1u;
            bs = nbs;
            be = nbe;
          }
        }  // if (own)
        // one step of the TAIL loop: pull the step PD ahead (ticket TY) and load
        // its rows into (YA, YB) -- none left: re-read the breed cursor's --,
        // wait for the next step's rows (NA, NB) as the unit loop does, breed
        // the step of ticket TX from (XA, XB) with the per-step epilogue
#define PGA_TP_TSTEP(XA, XB, YA, YB, NA, NB, TX, TY)                                                        \
  {                                                                                                         \
    PGA_TP_TPULL(TY)                                                                                        \
    PGA_TP_TSERVE(PGA_TP_TNEED(TY), TY < ntst)                                                              \
    PGA_TP_TWAIT(TY)                                                                                        \
    {                                                                                                       \
      const uint32_t tl_ = TY < ntst ? TY : TX;                                                             \
      const uint4 tr_ = trec[tl_ / (uint32_t)GS][(tl_ % (uint32_t)GS) * NG + g][0];                         \
      YA = ROW(cur, tr_.x, qq);                                                                             \
      YB = ROW(cur, tr_.y, qq);                                                                             \
    }                                                                                                       \
    {                                                                                                       \
      const uint32_t w_ = NA.x | NB.x;                                                                      \
      asm volatile("" ::"v"(w_));                                                                           \
    }                                                                                                       \
    {                                                                                                       \
      const uint32_t tu_ = TX / (uint32_t)GS, ti_ = TX % (uint32_t)GS;                                      \
      const uint32_t bs = rbeg + (nown + tu_) * 64u;                                                        \
      PGA_TP_BREED(XA, XB, ti_, trec[tu_])                                                                  \
      PGA_TP_STEP_SCORE                                                                                     \
    }                                                                                                       \
    PGA_TP_TCOUNT                                                                                           \
  }
        if (tailm) {
#ifdef PGA_TP_TIMING
          const unsigned long long clkT = clock64();
#endif
          for (;;) {
            if (tq0 >= ntst) break;
            PGA_TP_TSTEP(A0, B0, A2, B2, A1, B1, tq0, tq2)
            if (tq1 >= ntst) break;
            PGA_TP_TSTEP(A1, B1, A0, B0, A2, B2, tq1, tq0)
            if (tq2 >= ntst) break;
            PGA_TP_TSTEP(A2, B2, A1, B1, A0, B0, tq2, tq1)
          }
#ifdef PGA_TP_TIMING
          clk_tail += clock64() - clkT;
#endif
        }
#undef PGA_TP_TSTEP
      } else if constexpr (PD == 1) {
        PGA_TP_LOAD(A0, B0)
        for (;;) {
          PGA_TP_STEP(A0, B0, A1, B1)
          if (done) break;
          PGA_TP_STEP(A1, B1, A0, B0)
          if (done) break;
        }
      } else if constexpr (PD == 2) {
        PGA_TP_LOAD(A0, B0)
        PGA_TP_LOAD(A1, B1)
        for (;;) {
          PGA_TP_STEP(A0, B0, A2, B2)
          if (done) break;
          PGA_TP_STEP(A1, B1, A0, B0)
          if (done) break;
          PGA_TP_STEP(A2, B2, A1, B1)
          if (done) break;
        }
      } else {
        PGA_TP_LOAD(A0, B0)
        PGA_TP_LOAD(A1, B1)
        PGA_TP_LOAD(A2, B2)
        for (;;) {
          PGA_TP_STEP(A0, B0, A3, B3)
          if (done) break;
          PGA_TP_STEP(A1, B1, A0, B0)
          if (done) break;
          PGA_TP_STEP(A2, B2, A1, B1)
          if (done) break;
          PGA_TP_STEP(A3, B3, A2, B2)
          if (done) break;
        }
      }
#undef PGA_TP_USTEP
#undef PGA_TP_STEP
#undef PGA_TP_STEP_SCORE
#undef PGA_TP_BREED
#undef PGA_TP_LOAD
#undef PGA_TP_NEXT
#undef PGA_TP_JIT_EVAL
#undef PGA_TP_COUNT
#undef PGA_TP_TCOUNT
    }
#undef PGA_TP_TPULL
#undef PGA_TP_TSERVE
#undef PGA_TP_TNEED
#undef PGA_TP_TWAIT
#undef PGA_TP_TSPIN0
#undef PGA_TP_TSPIN1
#undef PGA_TP_RESOLVE
#undef PGA_TP_RESOLVE_TO
#undef PGA_TP_SPIN0
#undef PGA_TP_SPIN1
#ifdef PGA_TP_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this round's stores issued and done
    const unsigned long long clkE = clock64();
    clk_b += clkE - clkB;
#endif
    __syncthreads();  // every wave out of the round's counters before they are reset
#ifdef PGA_TP_TIMING
    clk_sync1 += clock64() - clkE;
#endif
    if (threadIdx.x == 0) lds_next = lds_tnext = 0;
    if (threadIdx.x < kTpMaxSegs) lds_ready[threadIdx.x] = 0;
    if constexpr (TAILF) {
      if (threadIdx.x == 0) lds_tstep = 0;
      if (threadIdx.x < kTpMaxTail) lds_tready[threadIdx.x] = 0;
    }
  }
#undef ROW
#undef ELEM
#ifdef PGA_TP_TIMING
  if (lane == 0 && blockIdx.x * NW + wid < kMaxGrid * 4) {
    const uint32_t wv = blockIdx.x * NW + wid;
    pga_tp_clk[wv][0] = clk_t;
    pga_tp_clk[wv][1] = clk_b;
    pga_tp_clk[wv][2] = clock64() - clk0;
    pga_tp_clk[wv][3] = n_bred;
    pga_tp_clk[wv][4] = rt0;
    pga_tp_clk[wv][5] = wall_clock64();
    pga_tp_clk[wv][6] = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // HW_REG_XCC_ID[3:0]
    pga_tp_clk[wv][7] = clk_spin;  // cycles a breeding wave waited for a segment's flag
    pga_tp_clk[wv][8] = clk_sync0;   // ... at the first round's first barrier
    pga_tp_clk[wv][9] = clk_sync1;   // ... at the rounds' last barriers
    pga_tp_clk[wv][10] = clk_syncn;  // ... at the later rounds' first barriers
    pga_tp_clk[wv][11] = clk_tail;   // cycles in the tail loop
    pga_tp_clk[wv][12] = n_tail;     // tail steps the wave bred
    pga_tp_clk[wv][13] = clk_tflag;  // cycles it waited for tail units' flags
  }
#endif
  // (the unit loop's kernels: an opaque thread id, so that this loop's bounds
  // are worked out here and not shared with the zeroing loop at the kernel's
  // start, in registers across everything between)
  uint32_t ftid = threadIdx.x;
  if constexpr (TAILF) asm volatile("" : "+v"(ftid));
  if (hist)  // every wave passed the last round's barrier: the block's counts are complete
    for (uint32_t i = ftid; i < a.hist_bins; i += blockDim.x) {
      const uint32_t v = lds_hist[i];
      if (a.key_hist && v) __hip_atomic_fetch_add(&a.key_hist[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.rank_counts) a.rank_counts[i * gridDim.x + blockIdx.x] = v;  // this block's sort tile
    }
  if (EVALS && best_parts) {  // block-uniform
    unsigned long long bb = block_max_u64_n(my_best, lds_red, NW);
    if (threadIdx.x == 0) best_parts[blockIdx.x] = bb;
    if (a.stats_parts) block_stats_store_n(st, a.stats_parts, NW);
  }
}

// 16-wave blocks (one per CU) for the headline launch and 4-wave blocks for
// small populations; 128 VGPRs either way (the breed phase measured alike at
// 4 and 5 waves per SIMD: the fabric is the bound)
template <int GS, int OBJ, bool FULL, bool DENSE>
__global__ __launch_bounds__(kTpMaxWaves * 64) void binary_gen_tp(GenArgs a, unsigned long long* best_parts) {
  binary_gen_tp_body<GS, OBJ, FULL, DENSE>(a, best_parts);
}

// ---------------------------------------------------------------------------
// Batched islands: up to kMaxBatch same-shape islands of one device in ONE
// launch, island = blockIdx.y (its GenArgs and best partials from the kernel
// argument block), blockIdx.x / gridDim.x the island's own grid.  Many small
// islands on separate streams are launch-bound and share the process's 4
// hardware queues; one launch fills the device with all of them.  The
// reference's islands are at most MAX_POPULATIONS = 10 per solver
// (include/pga.h:44), run serially (src/pga.cu:272-276).
// ---------------------------------------------------------------------------
constexpr uint32_t kMaxBatch = 10;
struct GenBatch {
  GenArgs a[kMaxBatch];
  unsigned long long* parts[kMaxBatch];
};

template <int GS, int OBJ, bool FULL, bool DENSE>
__global__ __launch_bounds__(kTpMaxWaves * 64) void binary_gen_tp_batch(GenBatch b) {
  binary_gen_tp_body<GS, OBJ, FULL, DENSE>(b.a[blockIdx.y], b.parts[blockIdx.y]);
}

}  // namespace (jitgen / anonymous)
}  // namespace pga
