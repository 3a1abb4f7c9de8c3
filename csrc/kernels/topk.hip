// topk.hip — exact top-k / bottom-k selection (radix select, value-histogram
// and ticketed selects with the row moves fused in), row gather / scatter and
// the stripe migration kernels: elitism > 1, Island.topk and island migration.
//
// Implements the reference's stubbed top-N / migration entry points
// (src/pga.cu:238-248, :368-374) on the device.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <stdexcept>

#include "pga/device.hpp"
#include "pga/ops.hpp"

namespace pga {

namespace {
using namespace dev;

// ---------------- radix-select top-k ----------------
struct TopkState {
  uint32_t prefix, mask, remaining, pad;
  uint32_t hist[256];
};

__device__ __forceinline__ uint32_t topk_key(float s, bool largest) {
  uint32_t k = score_key(s);
  return largest ? k : ~k;
}

// Keys of the selection: 32-bit orderable f32 keys, or (integer objectives)
// the population's u16 tournament keys — two radix passes instead of four.
// u16 keys are clamped to vmax (= R - 1 of a value-histogram selection) in
// every pass, exactly as the histogram bins them: a key above the objective's
// range (a checkpoint's or an unvalidated migrant's score) can then neither
// make the passes disagree nor write past k indices.
template <int BITS>
struct TopkKeys {
  const float* s;
  const uint16_t* k16;
  bool largest;
  uint32_t vmax = 0xFFFFu;
  __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
    if (BITS == 16) {
      const uint32_t v = min((uint32_t)k16[i], vmax);
      return largest ? v : 0xFFFFu - v;
    }
    return topk_key(s[i], largest);
  }
};

__global__ __launch_bounds__(kBlock) void topk_init_kernel(TopkState* st, uint32_t k) {
  if (threadIdx.x == 0) {
    st->prefix = 0;
    st->mask = 0;
    st->remaining = k;
  }
  st->hist[threadIdx.x] = 0;
}

// One count per active lane into the LDS histogram h.  Scores cluster (a
// converging population shares its high digits), so when every active lane of
// the wave agrees on one bin the wave adds its count with one atomic; else
// plain per-lane LDS atomics.  Every lane of the wave calls it (ballots).
__device__ __forceinline__ void wave_hist_add(uint32_t* h, bool act, uint32_t bin) {
  const unsigned long long active = __ballot(act);
  if (active) {
    const int leader = __ffsll((long long)active) - 1;
    const uint32_t b = (uint32_t)__shfl((int)bin, leader, 64);
    const unsigned long long same = __ballot(act && bin == b);
    if (same == active) {
      if ((int)lane_id() == leader) atomicAdd(&h[b], (uint32_t)__popcll(same));
    } else if (act) {
      atomicAdd(&h[bin], 1u);
    }
  }
}

// 8-bit digit histogram of the keys that match the prefix found so far
template <int BITS>
__global__ __launch_bounds__(kBlock) void topk_hist_kernel(TopkKeys<BITS> keys, uint64_t S, uint32_t shift,
                                                           TopkState* st) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t prefix = st->prefix, mask = st->mask;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < S; base += stride) {  // wave-uniform trip count
    const uint64_t i = base + threadIdx.x;
    uint32_t bin = 0;
    bool act = false;
    if (i < S) {
      const uint32_t key = keys(i);
      act = (key & mask) == prefix;
      bin = (key >> shift) & 255u;
    }
    wave_hist_add(h, act, bin);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

// pick the digit: the largest d whose suffix count reaches `remaining`
// (block-parallel suffix sums over the 256 bins; one thread per bin)
__global__ __launch_bounds__(kBlock) void topk_digit_kernel(TopkState* st, uint32_t shift) {
  __shared__ uint32_t suf[kBlock];
  const uint32_t t = threadIdx.x;
  const uint32_t c = st->hist[255 - t];  // reversed: suf[t] = sum of bins >= 255 - t
  const uint32_t rem = st->remaining;
  suf[t] = c;
  __syncthreads();
  for (uint32_t o = 1; o < kBlock; o <<= 1) {
    const uint32_t v = t >= o ? suf[t - o] : 0u;
    __syncthreads();
    suf[t] += v;
    __syncthreads();
  }
  // first t (largest digit 255 - t) whose inclusive suffix reaches rem
  const bool hit = suf[t] >= rem && (t == 0 || suf[t - 1] < rem);
  const bool last = t == kBlock - 1 && suf[t] < rem;  // cannot happen for k <= S; keep digit 0
  if (hit || last) {
    const uint32_t d = 255 - t;
    st->remaining = rem - (t ? suf[t - 1] : 0u);
    st->prefix |= d << shift;
    st->mask |= 255u << shift;
  }
  __syncthreads();
  st->hist[t] = 0;
}

// ordered compaction: contiguous range per block
template <int BITS>
__global__ __launch_bounds__(kBlock) void topk_count_kernel(TopkKeys<BITS> keys, uint64_t S, uint64_t per_block,
                                                            const TopkState* st, uint32_t* cnt) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t T = st->prefix;
  const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
  const uint64_t b1 = b0 + per_block < S ? b0 + per_block : S;
  uint32_t gt = 0, eq = 0;
  for (uint64_t i = b0 + threadIdx.x; i < b1; i += kBlock) {
    uint32_t key = keys(i);
    gt += key > T;
    eq += key == T;
  }
  auto add = [](uint32_t a, uint32_t b) { return a + b; };
  gt = block_reduce(gt, lds, add);
  eq = block_reduce(eq, lds, add);
  if (threadIdx.x == 0) {
    cnt[2 * blockIdx.x] = gt;
    cnt[2 * blockIdx.x + 1] = eq;
  }
}

// exclusive scan of the per-block (gt, eq) counts, n <= 4 * kBlock, one block
__global__ __launch_bounds__(kBlock) void topk_offsets_kernel(uint32_t* cnt, uint32_t n) {
  __shared__ uint32_t lds[kBlock / 64];
  uint32_t g[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0};
  uint32_t sg = 0, se = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t i = 4 * threadIdx.x + j;
    if (i < n) {
      g[j] = cnt[2 * i];
      e[j] = cnt[2 * i + 1];
    }
    sg += g[j];
    se += e[j];
  }
  uint32_t tg, te;
  uint32_t og = block_excl_scan_u(sg, lds, tg);
  __syncthreads();
  uint32_t oe = block_excl_scan_u(se, lds, te);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t i = 4 * threadIdx.x + j;
    if (i < n) {
      cnt[2 * i] = og;
      cnt[2 * i + 1] = oe;
    }
    og += g[j];
    oe += e[j];
  }
  if (threadIdx.x == 0) cnt[2 * n] = tg;  // total strictly greater
}

template <int BITS>
__global__ __launch_bounds__(kBlock) void topk_write_kernel(TopkKeys<BITS> keys, uint64_t S, uint64_t per_block,
                                                            const TopkState* st, const uint32_t* cnt, uint32_t nblocks,
                                                            uint32_t* keys_out, uint32_t* idx_out) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t T = st->prefix;
  const uint32_t need_eq = st->remaining;
  const uint32_t gt_total = cnt[2 * nblocks];
  uint32_t gpos = cnt[2 * blockIdx.x], epos = cnt[2 * blockIdx.x + 1];
  const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
  const uint64_t b1 = b0 + per_block < S ? b0 + per_block : S;
  for (uint64_t t0 = b0; t0 < b1; t0 += kBlock) {
    uint64_t i = t0 + threadIdx.x;
    uint32_t key = i < b1 ? keys(i) : 0u;
    uint32_t isg = (i < b1 && key > T) ? 1u : 0u;
    uint32_t ise = (i < b1 && key == T) ? 1u : 0u;
    uint32_t tg, te;
    uint32_t rg = block_excl_scan_u(isg, lds, tg);
    __syncthreads();
    uint32_t re = block_excl_scan_u(ise, lds, te);
    if (isg && gpos + rg < gt_total) {
      if (keys_out) keys_out[gpos + rg] = key;
      idx_out[gpos + rg] = (uint32_t)i;
    }
    if (ise && epos + re < need_eq) {
      if (keys_out) keys_out[gt_total + epos + re] = key;
      idx_out[gt_total + epos + re] = (uint32_t)i;
    }
    gpos += tg;
    epos += te;
    __syncthreads();
  }
}

// ---------------- selection order in one ticketed select ----------------
// The threshold bin of an R-bin histogram G counted from the top — the bin
// where the count of keys in higher bins first reaches k — and the k left for
// it.  R is a multiple of kBlock, at most 8 bins per thread (the f32 digit
// histograms); block-wide, every thread returns the same, and the barrier
// that publishes sh[0..1] is the last thing it does.
__device__ __forceinline__ void topk_threshold(const uint32_t* G, uint32_t R, uint32_t k, uint32_t* lds, uint32_t* sh,
                                               uint32_t& T, uint32_t& rem) {
  const uint32_t per = R / kBlock;  // 8 or 4
  uint32_t c[8], mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) {
    c[j] = j < per ? G[R - 1 - threadIdx.x * per - j] : 0u;
    mine += c[j];
  }
  uint32_t tot;
  const uint32_t before = block_excl_scan_u(mine, lds, tot);
  if (before < k && before + mine >= k) {  // the one thread holding the threshold
    uint32_t acc = before;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      if (j < per && acc < k && acc + c[j] >= k) {
        sh[0] = R - 1 - threadIdx.x * per - j;
        sh[1] = k - acc;
      }
      acc += c[j];
    }
  }
  if (threadIdx.x == 0 && tot < k) {  // k > S cannot happen (the launcher checks); keep bin 0
    sh[0] = 0;
    sh[1] = k;
  }
  __syncthreads();
  T = sh[0];
  rem = sh[1];
}

// selections per block listed in LDS for the cooperative row move (a
// migration's k / blocks is ~41 at the headline; more go row by row).  Small:
// with ~9 KB of LDS the selections fit beside a generation kernel's block
// (120 KB), so one on the transport stream runs concurrently with it.
constexpr uint32_t kTopkMoveSlots = 1024;

// What the fused selection does with the i-th selected individual at output
// position pos (besides idx_out[pos] = i when idx_out is set):
//   GATHER   out rows[pos] = population row i, out scores[pos] = score i (emigrants)
//   SCATTER  population row i = in rows[pos], score i and its u16 key =
//            in scores[pos] (immigrants replace the selected victims)
// so an island-migration epoch needs no separate gather / scatter kernels.
__device__ __forceinline__ void topk_emit(const TopkMove& mv, uint32_t* idx_out, uint32_t pos, uint64_t i) {
  if (idx_out) idx_out[pos] = (uint32_t)i;
  if (mv.mode == TopkMove::GATHER) {
    for (uint32_t c = 0; c < mv.rw16; ++c) mv.dst_rows[(uint64_t)pos * mv.rw16 + c] = mv.src_rows[i * mv.rw16 + c];
    mv.dst_scores[pos] = mv.src_scores[i];
  } else if (mv.mode == TopkMove::SCATTER) {
    for (uint32_t c = 0; c < mv.rw16; ++c) mv.dst_rows[i * mv.rw16 + c] = mv.src_rows[(uint64_t)pos * mv.rw16 + c];
    const float v = mv.src_scores[pos];
    mv.dst_scores[i] = v;
    if (mv.dst_keys) mv.dst_keys[i] = score_to_key16(v);
  }
}

// The select, after its histogram(s): threshold, count, block offsets and the
// ordered write in one launch.  Each block takes a ticket b (its position in
// dispatch order) and owns the b-th contiguous range; each thread owns a
// contiguous sub-range of whole 16-key chunks, so one block scan of the
// per-thread (gt, eq) counts orders the block.  The block publishes its
// aggregate (flag | gt | eq) and then reads the aggregates of ALL its
// predecessors in parallel (one word per thread, no look-back chain): a
// predecessor by ticket is already dispatched and publishes without waiting
// on anyone, so every wait ends.  The words carry all the data, so relaxed
// agent-scope atomics suffice.  A block derives its threshold from the
// histogram before it publishes, and the last ticket has seen every other
// block's word: every read of the histogram is done by then, so it may
// re-zero what the blocks read (last_ticket()) for the next selection.  The
// histogram kernels zero the words and the tickets before every selection.
// Same result as count -> offsets -> write (topk_run): the keys beyond the
// threshold T in population order, then the first need_eq ties.
//
// With a row move, the block's selections are listed in LDS first (slot: gt
// ones in scan order, then the taken ties) and copied by the whole block
// afterwards, 16 bytes per lane, rows contiguous: one thread per row was 3x
// slower than the separate gather / scatter kernels.  SCATTER with best_parts
// also writes the block's new packed best: the best survivor (Keys::keep /
// Keys::block_best) or the best immigrant placed here.
//
// Keys: load(c0, end, kv) -> the 16 keys of [c0, c0 + 16) clipped to end in
// order space (larger = selected first) and the mask of the valid ones;
// keep(key, i) -> survivor i's contribution to the block's best;
// block_best(kb, mv) -> the packed best of the block's max contribution.
constexpr uint64_t kLbAgg = 1ull << 62, kLbMask31 = 0x7FFFFFFFull;

template <class Keys, class LastTicket>
__device__ __forceinline__ void topk_select_body(const Keys& keys, uint64_t S, uint64_t per_block, uint32_t k,
                                                 uint32_t T, uint32_t need_eq, uint32_t b, uint64_t* status,
                                                 uint32_t nblocks, uint32_t* idx_out, const TopkMove mv,
                                                 uint32_t* lds, LastTicket last_ticket) {
  __shared__ uint32_t sel_pos[kTopkMoveSlots], sel_src[kTopkMoveSlots];  // row moves: output position, source
  const uint32_t gt_total = k - need_eq;                                   // every key above T
  const uint64_t pt = ((per_block + kBlock - 1) / kBlock + 15) / 16 * 16;  // keys per thread, whole 16-key chunks
  const uint64_t blo = (uint64_t)b * per_block;
  const uint64_t bhi = blo + per_block < S ? blo + per_block : S;
  const uint64_t t0 = blo + threadIdx.x * pt;
  const uint64_t t1 = t0 + pt < bhi ? t0 + pt : bhi;
  uint32_t gt = 0, eq = 0;
  for (uint64_t c0 = t0; c0 < t1; c0 += 16) {
    uint32_t kv[16];
    const uint32_t m = keys.load(c0, t1, kv);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      gt += ((m >> e) & 1u) && kv[e] > T;
      eq += ((m >> e) & 1u) && kv[e] == T;
    }
  }
  uint32_t bg, be;
  uint32_t og = block_excl_scan_u(gt, lds, bg);
  __syncthreads();
  uint32_t oe = block_excl_scan_u(eq, lds, be);
  if (threadIdx.x == 0)
    __hip_atomic_store(&status[b], kLbAgg | ((uint64_t)bg << 31) | (uint64_t)be, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  // block prefix = sum of the predecessors' aggregates, read in parallel
  uint32_t pg = 0, pe = 0;
  for (uint32_t j = threadIdx.x; j < b; j += kBlock) {
    uint64_t w = 0;
    for (uint32_t spins = 0; spins < (1u << 26); ++spins) {  // bound: never hang the device
      w = __hip_atomic_load(&status[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (w) break;
    }
    pg += (uint32_t)((w >> 31) & kLbMask31);
    pe += (uint32_t)(w & kLbMask31);
  }
  auto add = [](uint32_t x, uint32_t y) { return x + y; };
  pg = block_reduce(pg, lds, add);
  pe = block_reduce(pe, lds, add);
  if (b == nblocks - 1) last_ticket();
  uint32_t gpos = pg + og, epos = pe + oe;
  const bool move = mv.mode != TopkMove::NONE;
  const bool bests = mv.mode == TopkMove::SCATTER && mv.best_parts != nullptr;
  unsigned long long keep_best = 0, imm_best = 0;
  uint32_t lg = og, le = bg + oe;
  for (uint64_t c0 = t0; c0 < t1; c0 += 16) {
    uint32_t kv[16];
    const uint32_t m = keys.load(c0, t1, kv);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (!((m >> e) & 1u)) continue;
      uint32_t pos = 0xFFFFFFFFu, slot = 0;
      if (kv[e] > T && gpos < gt_total) {
        pos = gpos++;
        slot = lg++;
      }
      if (kv[e] == T) {
        if (epos < need_eq) {
          pos = gt_total + epos;
          slot = le;
        }
        ++epos;
        ++le;
      }
      if (bests) {
        if (pos == 0xFFFFFFFFu) {
          const unsigned long long kb = keys.keep(kv[e], c0 + e);
          keep_best = kb > keep_best ? kb : keep_best;
        } else {
          const unsigned long long ib = pack_best(mv.src_scores[pos], c0 + e);
          imm_best = ib > imm_best ? ib : imm_best;
        }
      }
      if (pos == 0xFFFFFFFFu) continue;
      if (idx_out) idx_out[pos] = (uint32_t)(c0 + e);
      if (move && slot < kTopkMoveSlots) {
        sel_pos[slot] = pos;
        sel_src[slot] = (uint32_t)(c0 + e - blo);
      } else if (move) {
        topk_emit(mv, nullptr, pos, c0 + e);  // beyond the LDS list (huge blocks): per thread
      }
    }
  }
  if (bests) {  // block-uniform: the block's new packed best
    __shared__ unsigned long long red[kBlock / 64];
    const unsigned long long kb = block_max_u64(keep_best, red);
    const unsigned long long ib = block_max_u64(imm_best, red);
    if (threadIdx.x == 0) {
      const unsigned long long sb = keys.block_best(kb, mv);
      mv.best_parts[b] = sb > ib ? sb : ib;
    }
  }
  if (!move) return;
  // slots [0, bg): keys above T (those with a global rank < gt_total were
  // taken), [bg, bg + be): ties, of which those with a tie rank < need_eq
  __syncthreads();
  const uint32_t taken_eq = pe >= need_eq ? 0u : min(be, need_eq - pe);
  const uint32_t n_gt = pg >= gt_total ? 0u : min(bg, gt_total - pg);
  const uint32_t nsel = min(bg + taken_eq, kTopkMoveSlots);
  const uint32_t rw16 = mv.rw16;
  for (uint32_t t = threadIdx.x; t < nsel * rw16; t += kBlock) {
    const uint32_t r = t / rw16, c = t % rw16;
    if (r >= n_gt && r < bg) continue;  // gt slots beyond gt_total were never filled
    const uint64_t i = blo + sel_src[r];
    const uint64_t pos = sel_pos[r];
    if (mv.mode == TopkMove::GATHER) {
      mv.dst_rows[pos * rw16 + c] = mv.src_rows[i * rw16 + c];
      if (c == 0) mv.dst_scores[pos] = mv.src_scores[i];
    } else {
      mv.dst_rows[i * rw16 + c] = mv.src_rows[pos * rw16 + c];
      if (c == 0) {
        const float v = mv.src_scores[pos];
        mv.dst_scores[i] = v;
        if (mv.dst_keys) mv.dst_keys[i] = score_to_key16(v);
      }
    }
  }
}

// ---- integer objectives: the u16 keys take at most R = L + 1 values, so one
// LDS histogram of R bins replaces the radix passes ----
// 16 consecutive u16 keys [c0, c0+16) clipped to `end`: two dwordx4 loads
// issued together when the chunk is whole and aligned (c0 % 8 == 0), else
// per-key loads; bit e of the result marks key e valid
__device__ __forceinline__ uint32_t load_keys16(const uint16_t* k16, uint64_t c0, uint64_t end, uint32_t (&kv)[16]) {
  if (c0 + 16 <= end && (c0 & 7) == 0) {
    const uint4 a = *(const uint4*)(k16 + c0), b = *(const uint4*)(k16 + c0 + 8);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      kv[2 * e] = w[e] & 0xFFFFu;
      kv[2 * e + 1] = w[e] >> 16;
    }
    return 0xFFFFu;
  }
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const bool ok = c0 + e < end;
    kv[e] = ok ? k16[c0 + e] : 0u;
    m |= ok ? (1u << e) : 0u;
  }
  return m;
}

// bin = key for the largest, R - 1 - key for the smallest; also zeroes the
// aggregate words and the ticket counters of the topk16_select_kernel that follows
__global__ __launch_bounds__(kBlock) void topk16_hist_kernel(const uint16_t* k16, uint64_t S, uint32_t R, bool largest,
                                                             uint32_t* G, uint64_t* status, uint32_t n_status) {
  uint32_t* hr = (uint32_t*)pga_dyn_lds;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_status; i += gridDim.x * kBlock) status[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < 2) ((uint32_t*)(status + n_status))[threadIdx.x] = 0;
  for (uint32_t i = threadIdx.x; i < R; i += kBlock) hr[i] = 0;
  __syncthreads();
  // 16 keys per thread per pass (coalesced 32-byte chunks)
  for (uint64_t c0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 16; c0 < S;
       c0 += (uint64_t)gridDim.x * kBlock * 16) {
    uint32_t kv[16];
    const uint32_t m = load_keys16(k16, c0, S, kv);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const uint32_t v = min(kv[e], R - 1);
      if ((m >> e) & 1u) atomicAdd(&hr[largest ? v : R - 1 - v], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < R; i += kBlock)
    if (hr[i]) atomicAdd(&G[i], hr[i]);
}

// the u16 keys in TopkKeys<16> order space: clamped to vmax = R - 1 as the
// histogram bins them, flipped for the smallest
struct SelectKeys16 {
  const uint16_t* k16;
  uint32_t vmax, flip;
  __device__ __forceinline__ uint32_t load(uint64_t c0, uint64_t end, uint32_t (&kv)[16]) const {
    const uint32_t m = load_keys16(k16, c0, end, kv);
#pragma unroll
    for (int e = 0; e < 16; ++e) kv[e] = min(kv[e], vmax) ^ flip;
    return m;
  }
  // (clamped key, ~index): the pack_best order, as key == score for the integer objectives
  __device__ __forceinline__ unsigned long long keep(uint32_t key, uint64_t i) const {
    return ((unsigned long long)(key ^ flip) << 32) | (0xFFFFFFFFull - (uint32_t)i);
  }
  // the best survivor's own score (a survivor's score is not written by this launch)
  __device__ __forceinline__ unsigned long long block_best(unsigned long long kb, const TopkMove& mv) const {
    if (!kb) return 0;
    const uint64_t i = 0xFFFFFFFFull - (uint32_t)kb;
    return pack_best(mv.dst_scores[i], i);
  }
};

// G in bin space (topk16_hist_kernel) unless fused: then G is a value-order
// histogram read only (the generation kernel's fused histogram, GenArgs::
// key_hist), bin b at G[R - 1 - b] for the smallest, and nothing re-zeroes it
__global__ __launch_bounds__(kBlock) void topk16_select_kernel(const uint16_t* k16, uint64_t S, uint64_t per_block,
                                                               uint32_t R, bool largest, uint32_t k, uint32_t* G,
                                                               uint64_t* status, uint32_t* ctr, uint32_t nblocks,
                                                               uint32_t* idx_out, TopkMove mv, bool fused) {
  __shared__ uint32_t lds[kBlock / 64], sh[2], sh_b;
  if (threadIdx.x == 0) sh_b = atomicAdd(&ctr[0], 1u);
  // threshold bin, as topk_threshold, for a run-time R of up to 32 bins per
  // thread that need not fill the block: thread t owns bins
  // [R-1 - (t+1)*per + 1, R-1 - t*per] from the top and the one holding the
  // threshold re-reads them.  (A helper shared with the f32 digits, its bins
  // kept in 32 unrolled registers, made a OneMax migration epoch 2 us slower:
  // profiles/topk_refactor_ab.md.)
  const uint32_t per = (R + kBlock - 1) / kBlock;
  const bool rev = fused && !largest;
  uint32_t mine = 0;
  for (uint32_t j = 0; j < per; ++j) {
    const int64_t b = (int64_t)R - 1 - (int64_t)threadIdx.x * per - j;
    if (b >= 0) mine += G[rev ? R - 1 - b : b];
  }
  uint32_t tot;
  const uint32_t before = block_excl_scan_u(mine, lds, tot);
  if (before < k && before + mine >= k) {
    uint32_t acc = before;
    for (uint32_t j = 0; j < per; ++j) {
      const int64_t b = (int64_t)R - 1 - (int64_t)threadIdx.x * per - j;
      if (b < 0) break;
      const uint32_t c = G[rev ? R - 1 - b : b];
      if (acc + c >= k) {
        sh[0] = (uint32_t)b;
        sh[1] = k - acc;
        break;
      }
      acc += c;
    }
  }
  if (threadIdx.x == 0 && tot < k) {  // k > S cannot happen (the launcher checks); keep bin 0
    sh[0] = 0;
    sh[1] = k;
  }
  __syncthreads();  // (also publishes sh_b)
  const uint32_t T = largest ? sh[0] : sh[0] + 0x10000u - R;  // bin -> key in order space
  const uint32_t need_eq = sh[1];
  topk_select_body(SelectKeys16{k16, R - 1, largest ? 0u : 0xFFFFu}, S, per_block, k, T, need_eq, sh_b, status,
                   nblocks, idx_out, mv, lds, [=] {
                     if (!fused)
                       for (uint32_t i = threadIdx.x; i < R; i += kBlock) G[i] = 0;
                   });
}

// ---- f32 scores: the exact top-k in selection order from three radix
// digits of the 32-bit orderable keys (11 / 11 / 10 bits) and one ticketed
// select: 4 launches per selection (the 8-bit radix path above takes 11, and
// the gather / scatter / best passes after it 3 more).  Each histogram
// kernel's blocks re-derive the previous digit's threshold from its global
// histogram themselves (block 0 also records it for the next launch), so no
// single-block digit kernels sit between the passes; the select kernel
// derives the last digit and runs the shared body. ----
constexpr uint32_t kT32R1 = 2048, kT32R2 = 2048, kT32R3 = 1024;  // digit bins: key >> 21, (key >> 10) & 2047, key & 1023
constexpr uint32_t kT32State = kT32R1 + kT32R2 + kT32R3;         // G word offset of {T1, k2, T2, k3}
static_assert(kT32State + 4 <= kTopkMaxRange, "f32 selection histograms fit the value-histogram region");

// 16 keys of [c0, c0 + 16) clipped to end (float4 loads when whole and aligned)
__device__ __forceinline__ uint32_t load_keys32(const float* s, uint64_t c0, uint64_t end, bool largest,
                                                uint32_t (&kv)[16]) {
  if (c0 + 16 <= end && (c0 & 3) == 0) {
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *(const float4*)(s + c0 + 4 * j);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      kv[4 * j] = topk_key(v[j].x, largest);
      kv[4 * j + 1] = topk_key(v[j].y, largest);
      kv[4 * j + 2] = topk_key(v[j].z, largest);
      kv[4 * j + 3] = topk_key(v[j].w, largest);
    }
    return 0xFFFFu;
  }
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const bool ok = c0 + e < end;
    kv[e] = ok ? topk_key(s[c0 + e], largest) : 0u;
    m |= ok ? (1u << e) : 0u;
  }
  return m;
}

// histogram of digit `level` (1, 2, 3) over the keys whose higher digits
// match the thresholds found so far; level 1 also zeroes the select's status
// words and tickets
__global__ __launch_bounds__(kBlock) void topk32_hist_kernel(const float* scores, uint64_t S, uint64_t per_block,
                                                             bool largest, uint32_t k, uint32_t level, uint32_t* G,
                                                             uint64_t* status, uint32_t n_status) {
  __shared__ uint32_t h[kT32R1];
  __shared__ uint32_t lds[kBlock / 64], sh[2];
  const uint32_t R = level == 3 ? kT32R3 : kT32R1;
  for (uint32_t i = threadIdx.x; i < R; i += kBlock) h[i] = 0;
  uint32_t pfx = 0, pmask = 0, shift = 21, dmask = kT32R1 - 1;
  if (level == 1) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_status; i += gridDim.x * kBlock) status[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 2) ((uint32_t*)(status + n_status))[threadIdx.x] = 0;
  } else {
    uint32_t* st = G + kT32State;
    uint32_t T1, k2;
    if (level == 2) {
      topk_threshold(G, kT32R1, k, lds, sh, T1, k2);
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[0] = T1;
        st[1] = k2;
      }
      pfx = T1 << 21;
      pmask = 0xFFE00000u;
      shift = 10;
    } else {
      T1 = st[0];
      k2 = st[1];
      uint32_t T2, k3;
      topk_threshold(G + kT32R1, kT32R2, k2, lds, sh, T2, k3);
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[2] = T2;
        st[3] = k3;
      }
      pfx = (T1 << 21) | (T2 << 10);
      pmask = 0xFFFFFC00u;
      shift = 0;
      dmask = kT32R3 - 1;
    }
  }
  __syncthreads();
  const uint64_t pt = ((per_block + kBlock - 1) / kBlock + 15) / 16 * 16;
  const uint64_t blo = (uint64_t)blockIdx.x * per_block;
  const uint64_t bhi = blo + per_block < S ? blo + per_block : S;
  const uint64_t t0 = blo + threadIdx.x * pt, t1 = t0 + pt < bhi ? t0 + pt : bhi;
  // trip count uniform across the wave (per-thread ranges of equal length):
  // the ballots of wave_hist_add need every lane in every iteration
  for (uint64_t c0 = blo + threadIdx.x * pt, n = 0; n < pt; c0 += 16, n += 16) {
    uint32_t kv[16];
    const uint32_t m = c0 < t1 ? load_keys32(scores, c0, t1, largest, kv) : 0u;
#pragma unroll
    for (int e = 0; e < 16; ++e)
      wave_hist_add(h, ((m >> e) & 1u) && (kv[e] & pmask) == pfx, (kv[e] >> shift) & dmask);
  }
  __syncthreads();
  uint32_t* Gl = G + (level == 1 ? 0u : (level == 2 ? kT32R1 : kT32R1 + kT32R2));
  for (uint32_t i = threadIdx.x; i < R; i += kBlock)
    if (h[i]) atomicAdd(&Gl[i], h[i]);
}

// the orderable keys of the f32 scores, flipped for the smallest (flip = 0 or
// ~0, as SelectKeys16: a mask, not a select on `largest` per key, keeps the
// kernel's scalar registers below the unshared kernel's)
struct SelectKeys32 {
  const float* s;
  uint32_t flip;
  __device__ __forceinline__ uint32_t load(uint64_t c0, uint64_t end, uint32_t (&kv)[16]) const {
    const uint32_t m = load_keys32(s, c0, end, true, kv);
#pragma unroll
    for (int e = 0; e < 16; ++e) kv[e] ^= flip;
    return m;
  }
  // a survivor's own score, exactly, from the key
  __device__ __forceinline__ unsigned long long keep(uint32_t key, uint64_t i) const {
    return pack_best(key_score(key ^ flip), i);
  }
  __device__ __forceinline__ unsigned long long block_best(unsigned long long kb, const TopkMove&) const { return kb; }
};

// threshold key T from the three digits, then the shared select
__global__ __launch_bounds__(kBlock) void topk32_select_kernel(const float* scores, uint64_t S, uint64_t per_block,
                                                               bool largest, uint32_t k, uint32_t* G,
                                                               uint64_t* status, uint32_t* ctr, uint32_t nblocks,
                                                               uint32_t* idx_out, TopkMove mv) {
  __shared__ uint32_t lds[kBlock / 64], sh[2], sh_b;
  if (threadIdx.x == 0) sh_b = atomicAdd(&ctr[0], 1u);
  const uint32_t* st = G + kT32State;
  const uint32_t T1 = st[0], T2 = st[2], k3 = st[3];
  uint32_t T3, need_eq;
  topk_threshold(G + kT32R1 + kT32R2, kT32R3, k3, lds, sh, T3, need_eq);  // (its barrier publishes sh_b)
  const uint32_t b = sh_b;
  // G1 / G2 are read by no block of this launch: zeroed here for the next
  // selection (a slice per block); G3 and the state by the last ticket
  for (uint32_t i = b * kBlock + threadIdx.x; i < kT32R1 + kT32R2; i += nblocks * kBlock) G[i] = 0;
  topk_select_body(SelectKeys32{scores, largest ? 0u : ~0u}, S, per_block, k, (T1 << 21) | (T2 << 10) | T3, need_eq, b, status,
                   nblocks, idx_out, mv, lds, [=] {
                     for (uint32_t i = threadIdx.x; i < kT32R3 + 4; i += kBlock) G[kT32R1 + kT32R2 + i] = 0;
                   });
}

// ---------------- row gather / scatter by index ----------------
__global__ __launch_bounds__(kBlock) void gather_rows_kernel(const uint4* rows, const float* scores, uint32_t rw16,
                                                             const uint32_t* idx, uint32_t n, uint4* out,
                                                             float* out_scores) {
  const uint64_t total = (uint64_t)n * rw16;
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (uint64_t)gridDim.x * kBlock) {
    uint64_t r = t / rw16, c = t % rw16;
    uint64_t src = idx[r];
    out[t] = rows[src * rw16 + c];
    if (c == 0 && scores && out_scores) out_scores[r] = scores[src];
  }
}

__global__ __launch_bounds__(kBlock) void scatter_rows_kernel(uint4* rows, float* scores, uint32_t rw16,
                                                              const uint32_t* idx, uint32_t n, const uint4* in,
                                                              const float* in_scores) {
  const uint64_t total = (uint64_t)n * rw16;
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (uint64_t)gridDim.x * kBlock) {
    uint64_t r = t / rw16, c = t % rw16;
    uint64_t dst = idx[r];
    rows[dst * rw16 + c] = in[t];
    if (c == 0 && scores && in_scores) scores[dst] = in_scores[r];
  }
}

// ---- MIG_STRIPE migration: one wave per stripe (grid-stride over stripes) ----
// 16 lanes per stripe (4 stripes per wave): at 1% of 1M the k = 10486 stripes
// of ~100 individuals are 2622 waves, all resident at once, each lane loading
// its ~7 scores in one burst
constexpr uint32_t kStripeLanes = 16;
constexpr uint32_t kStripeCache = 8;  // scores per lane kept in registers (stripes <= 128)

__global__ __launch_bounds__(kBlock) void stripe_emigrate_kernel(const float* __restrict__ scores,
                                                                 const uint4* __restrict__ rows, uint32_t rw16,
                                                                 uint64_t S, uint32_t k, uint4* __restrict__ out,
                                                                 float* __restrict__ out_scores) {
  const uint32_t sl = threadIdx.x & (kStripeLanes - 1);
  const uint32_t ng = gridDim.x * (kBlock / kStripeLanes);
  for (uint32_t i = (blockIdx.x * kBlock + threadIdx.x) / kStripeLanes; i < k; i += ng) {  // group-uniform
    const uint64_t lo = (uint64_t)i * S / k, hi = (uint64_t)(i + 1) * S / k;
    unsigned long long b = 0;
    for (uint64_t j = lo + sl; j < hi; j += kStripeLanes) {
      const unsigned long long p = pack_best(scores[j], j);
      b = p > b ? p : b;
    }
#pragma unroll
    for (int o = kStripeLanes / 2; o > 0; o >>= 1) {
      const unsigned long long x = shfl_xor_u64(b, o);
      b = x > b ? x : b;
    }
    const uint64_t src = best_index(b);
    for (uint32_t c = sl; c < rw16; c += kStripeLanes) out[(uint64_t)i * rw16 + c] = rows[src * rw16 + c];
    if (sl == 0) out_scores[i] = best_score(b);
  }
}

__global__ __launch_bounds__(kBlock) void stripe_immigrate_kernel(float* __restrict__ scores, uint16_t* keys,
                                                                  uint4* __restrict__ rows, uint32_t rw16, uint64_t S,
                                                                  uint32_t k, const uint4* __restrict__ in,
                                                                  const float* __restrict__ in_scores,
                                                                  unsigned long long* best_parts, float* stats_parts) {
  __shared__ unsigned long long lds_red[kBlock / 64];
  const uint32_t sl = threadIdx.x & (kStripeLanes - 1);
  const uint32_t ng = gridDim.x * (kBlock / kStripeLanes);
  unsigned long long my_best = 0;
  ScoreStats st;
  for (uint32_t i = (blockIdx.x * kBlock + threadIdx.x) / kStripeLanes; i < k; i += ng) {  // group-uniform
    const uint64_t lo = (uint64_t)i * S / k, hi = (uint64_t)(i + 1) * S / k;
    const bool cached = hi - lo <= (uint64_t)kStripeLanes * kStripeCache;  // group-uniform
    // the immigrant (independent of the victim: issued with the score loads)
    const float sin = in_scores[i];
    const uint4 r0 = sl < rw16 ? in[(uint64_t)i * rw16 + sl] : make_uint4(0, 0, 0, 0);
    float v[kStripeCache];
    unsigned long long w = ~0ull;  // min of (score key << 32 | index): the worst, lowest index
#pragma unroll
    for (uint32_t t = 0; t < kStripeCache; ++t) {
      const uint64_t j = lo + sl + (uint64_t)t * kStripeLanes;
      v[t] = (cached && j < hi) ? scores[j] : 0.f;
      const unsigned long long p = ((unsigned long long)score_key(v[t]) << 32) | j;
      w = (cached && j < hi && p < w) ? p : w;
    }
    if (!cached)
      for (uint64_t j = lo + sl; j < hi; j += kStripeLanes) {
        const unsigned long long p = ((unsigned long long)score_key(scores[j]) << 32) | j;
        w = p < w ? p : w;
      }
#pragma unroll
    for (int o = kStripeLanes / 2; o > 0; o >>= 1) {
      const unsigned long long x = shfl_xor_u64(w, o);
      w = x < w ? x : w;
    }
    const uint64_t dst = (uint32_t)w;
    if (sl < rw16) rows[dst * rw16 + sl] = r0;
    for (uint32_t c = sl + kStripeLanes; c < rw16; c += kStripeLanes) rows[dst * rw16 + c] = in[(uint64_t)i * rw16 + c];
    if (sl == 0) {
      scores[dst] = sin;
      if (keys) keys[dst] = score_to_key16(sin);
    }
    // the stripe after the replacement: best partial and statistics
    if (cached) {
#pragma unroll
      for (uint32_t t = 0; t < kStripeCache; ++t) {
        const uint64_t j = lo + sl + (uint64_t)t * kStripeLanes;
        if (j < hi) {
          const float x = j == dst ? sin : v[t];
          const unsigned long long p = pack_best(x, j);
          my_best = p > my_best ? p : my_best;
          st.add(x);
        }
      }
    } else {
      for (uint64_t j = lo + sl; j < hi; j += kStripeLanes) {
        const float x = j == dst ? sin : scores[j];
        const unsigned long long p = pack_best(x, j);
        my_best = p > my_best ? p : my_best;
        st.add(x);
      }
    }
  }
  const unsigned long long b = block_max_u64(my_best, lds_red);
  if (threadIdx.x == 0) best_parts[blockIdx.x] = b;
  if (stats_parts) block_stats_store(st, stats_parts);
}

// The selection workspace: byte offsets of its regions, in this order,
//   state | status / count words | 3 k-arrays | radix-sort workspace (sorted
//   mode) | histogram words
// The histogram region (the u16 value histogram, or the f32 digit histograms
// and their state) is zero on allocation (Island::ensure_topk_ws clears the
// whole workspace) and every selection leaves it zeroed.
struct TopkLayout {
  size_t state, status, keys, keys_sorted, idx, sort, hist, bytes;
  static TopkLayout of(uint32_t k) {
    size_t p = 0;
    auto take = [&p](size_t n) {
      const size_t at = p;
      p += (n + 255) & ~(size_t)255;
      return at;
    };
    TopkLayout l;
    l.state = take(sizeof(TopkState));
    l.status = take(sizeof(uint32_t) * kTopkStatusWords);
    l.keys = take(4ull * k);
    l.keys_sorted = take(4ull * k);
    l.idx = take(4ull * k);
    l.sort = take(radix_sort_workspace_bytes(k));
    l.hist = take(4ull * kTopkMaxRange);
    l.bytes = p;
    return l;
  }
};

template <int BITS>
void topk_run(TopkKeys<BITS> keys, uint64_t S, uint32_t k, bool sorted, uint32_t* idx_out, void* ws, hipStream_t s) {
  const TopkLayout l = TopkLayout::of(k);
  char* p = (char*)ws;
  TopkState* st = (TopkState*)(p + l.state);
  uint32_t* cnt = (uint32_t*)(p + l.status);

  const uint32_t grid = launch_grid(S, kBlock * 4);
  hipLaunchKernelGGL(topk_init_kernel, 1, kBlock, 0, s, st, k);
  for (int d = 0; d < BITS / 8; ++d) {
    const uint32_t shift = BITS - 8 - 8 * d;
    hipLaunchKernelGGL(topk_hist_kernel<BITS>, grid, kBlock, 0, s, keys, S, shift, st);
    hipLaunchKernelGGL(topk_digit_kernel, 1, kBlock, 0, s, st, shift);
  }
  const uint32_t cgrid = grid > 1024 ? 1024 : grid;
  const uint64_t per_block = (S + cgrid - 1) / cgrid;
  hipLaunchKernelGGL(topk_count_kernel<BITS>, cgrid, kBlock, 0, s, keys, S, per_block, st, cnt);
  hipLaunchKernelGGL(topk_offsets_kernel, 1, kBlock, 0, s, cnt, cgrid);
  if (!sorted) {
    // selection order: every key above the threshold by index, then the
    // threshold ties by index — what the CPU backend's unsorted mode returns
    hipLaunchKernelGGL(topk_write_kernel<BITS>, cgrid, kBlock, 0, s, keys, S, per_block, st, cnt, cgrid,
                       (uint32_t*)nullptr, idx_out);
    PGA_HIP_CHECK(hipGetLastError());
    return;
  }
  uint32_t* keys_buf = (uint32_t*)(p + l.keys);
  uint32_t* idx = (uint32_t*)(p + l.idx);
  hipLaunchKernelGGL(topk_write_kernel<BITS>, cgrid, kBlock, 0, s, keys, S, per_block, st, cnt, cgrid, keys_buf, idx);
  PGA_HIP_CHECK(hipGetLastError());
  // stable descending sort (sort.hip) keeps equal keys in ascending index order
  radix_sort_pairs(keys_buf, idx, k, BITS, true, (uint32_t*)(p + l.keys_sorted), idx_out, p + l.sort, s);
}

// keys per thread of the selection-order kernels (their grid: S / (256 kpt)
// blocks, at most 1024); PGA_TOPK_KPT overrides (16, 32, 64 or 128)
uint32_t topk_kpt() {
  static const uint32_t v = [] {
    const char* e = std::getenv("PGA_TOPK_KPT");
    const uint32_t x = e ? (uint32_t)std::strtoul(e, nullptr, 10) : 16u;
    return (x == 16 || x == 32 || x == 64 || x == 128) ? x : 16u;
  }();
  return v;
}

bool value_histogram_range(uint32_t key_range) { return key_range >= 2 && key_range <= kTopkMaxRange; }

}  // namespace

size_t topk_workspace_bytes(uint64_t S, uint32_t k) {
  (void)S;
  return TopkLayout::of(k).bytes;
}

bool topk_move_supported(const uint16_t* keys16, uint32_t key_range, uint64_t S) {
  // u16 keys: the value-histogram select; f32 scores: the 3-digit radix select
  return (!keys16 || value_histogram_range(key_range)) && S < (1ull << 31);
}

uint32_t topk_launch(const float* scores, const uint16_t* keys16, uint32_t key_range, uint64_t S, uint32_t k,
                     bool largest, bool sorted, uint32_t* idx_out, void* ws, hipStream_t s, const TopkMove* mv,
                     const TopkFused* fused) {
  if (k == 0) return 0;
  if (k > S) throw std::runtime_error("topk: k > S");
  if (mv && (sorted || !topk_move_supported(keys16, key_range, S)))
    throw std::invalid_argument("topk: fused row moves need the u16-key selection-order path");
  if (!sorted && topk_move_supported(keys16, key_range, S)) {
    // selection order below 2^31 individuals: histogram(s) + the ticketed select
    const TopkLayout l = TopkLayout::of(k);
    uint64_t* status = (uint64_t*)((char*)ws + l.status);  // cgrid aggregate words, then 2 ticket counters
    uint32_t* G = (uint32_t*)((char*)ws + l.hist);          // zero on allocation and after every use
    const uint32_t grid = launch_grid(S, kBlock * topk_kpt());
    const uint32_t cgrid = grid > 1024 ? 1024 : grid;
    const uint64_t per_block = ((S + cgrid - 1) / cgrid + 15) / 16 * 16;  // whole 16-key chunks for every thread
    const TopkMove move = mv ? *mv : TopkMove{};
    if (!keys16) {
      // f32 scores: 3 radix digits (topk32_*)
      for (uint32_t level = 1; level <= 3; ++level)
        hipLaunchKernelGGL(topk32_hist_kernel, cgrid, kBlock, 0, s, scores, S, per_block, largest, k, level, G, status,
                           cgrid);
      hipLaunchKernelGGL(topk32_select_kernel, cgrid, kBlock, 0, s, scores, S, per_block, largest, k, G, status,
                         (uint32_t*)(status + cgrid), cgrid, idx_out, move);
    } else if (fused && fused->hist && fused->status) {
      // integer objective with the generation kernel's histogram of these
      // keys, its status words zeroed by that kernel: the select alone (one
      // pass over the keys)
      uint64_t* fst = (uint64_t*)fused->status;
      hipLaunchKernelGGL(topk16_select_kernel, cgrid, kBlock, 0, s, keys16, S, per_block, key_range, largest, k,
                         const_cast<uint32_t*>(fused->hist), fst, (uint32_t*)(fst + cgrid), cgrid, idx_out, move, true);
    } else {
      // integer objective: histogram over the key_range key values
      hipLaunchKernelGGL(topk16_hist_kernel, grid, kBlock, 4 * key_range, s, keys16, S, key_range, largest, G, status,
                         cgrid);
      hipLaunchKernelGGL(topk16_select_kernel, cgrid, kBlock, 0, s, keys16, S, per_block, key_range, largest, k, G,
                         status, (uint32_t*)(status + cgrid), cgrid, idx_out, move, false);
    }
    PGA_HIP_CHECK(hipGetLastError());
    return move.mode == TopkMove::SCATTER && move.best_parts ? cgrid : 0u;
  }
  // sorted, or 2^31 individuals and more: the 8-bit radix select.  In
  // selection order the u16 keys are clamped to the objective's range, as the
  // value histogram bins them.
  if (keys16) {
    TopkKeys<16> keys{scores, keys16, largest};
    if (!sorted && value_histogram_range(key_range)) keys.vmax = key_range - 1;
    topk_run<16>(keys, S, k, sorted, idx_out, ws, s);
  } else {
    topk_run<32>(TopkKeys<32>{scores, keys16, largest}, S, k, sorted, idx_out, ws, s);
  }
  return 0;
}

void gather_rows_launch(const void* rows, const float* scores, uint32_t row_words, const uint32_t* idx, uint32_t n,
                        void* out_rows, float* out_scores, hipStream_t s) {
  if (n == 0) return;
  const uint32_t rw16 = row_words / 4;
  uint32_t grid = launch_grid((uint64_t)n * rw16, kBlock);
  hipLaunchKernelGGL(gather_rows_kernel, grid, kBlock, 0, s, (const uint4*)rows, scores, rw16, idx, n,
                     (uint4*)out_rows, out_scores);
  PGA_HIP_CHECK(hipGetLastError());
}

void scatter_rows_launch(void* rows, float* scores, uint32_t row_words, const uint32_t* idx, uint32_t n,
                         const void* in_rows, const float* in_scores, hipStream_t s) {
  if (n == 0) return;
  const uint32_t rw16 = row_words / 4;
  uint32_t grid = launch_grid((uint64_t)n * rw16, kBlock);
  hipLaunchKernelGGL(scatter_rows_kernel, grid, kBlock, 0, s, (uint4*)rows, scores, rw16, idx, n,
                     (const uint4*)in_rows, in_scores);
  PGA_HIP_CHECK(hipGetLastError());
}

void stripe_emigrate_launch(const float* scores, const void* rows, uint32_t row_words, uint64_t S, uint32_t k,
                            void* out_rows, float* out_scores, hipStream_t s) {
  if (k == 0) return;
  if (k > S) throw std::invalid_argument("stripe migration: k exceeds the population");
  uint64_t grid = ((uint64_t)k + kBlock / kStripeLanes - 1) / (kBlock / kStripeLanes);
  if (grid > kMaxGrid) grid = kMaxGrid;
  hipLaunchKernelGGL(stripe_emigrate_kernel, (uint32_t)grid, kBlock, 0, s, scores, (const uint4*)rows, row_words / 4,
                     S, k, (uint4*)out_rows, out_scores);
  PGA_HIP_CHECK(hipGetLastError());
}

uint32_t stripe_immigrate_launch(float* scores, uint16_t* keys, void* rows, uint32_t row_words, uint64_t S, uint32_t k,
                                 const void* in_rows, const float* in_scores, unsigned long long* best_parts,
                                 float* stats_parts, hipStream_t s) {
  if (k == 0 || k > S) throw std::invalid_argument("stripe migration: k must be in [1, S]");
  uint64_t grid = ((uint64_t)k + kBlock / kStripeLanes - 1) / (kBlock / kStripeLanes);
  if (grid > kMaxGrid) grid = kMaxGrid;
  hipLaunchKernelGGL(stripe_immigrate_kernel, (uint32_t)grid, kBlock, 0, s, scores, keys, (uint4*)rows, row_words / 4,
                     S, k, (const uint4*)in_rows, in_scores, best_parts, stats_parts);
  PGA_HIP_CHECK(hipGetLastError());
  return (uint32_t)grid;
}

}  // namespace pga
