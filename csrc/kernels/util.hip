// util.hip — launch geometry and occupancy helpers, population-wide best /
// statistics reductions, tournament-key conversion and roulette prefix sums.
// (Top-k selection, row gather / scatter and migration: topk.hip.)
//
// Replaces the reference's host-side argmax over a D2H copy of every score
// (pga_get_best, src/pga.cu:218-236) on the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

#include "pga/device.hpp"
#include "pga/ops.hpp"
#include "pga/tp.hpp"

namespace pga {

int device_cu_count() {
  static int counts[64] = {0};
  int dev = 0;
  PGA_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) dev = 0;
  if (counts[dev] == 0) {
    int n = 0;
    PGA_HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    counts[dev] = n > 0 ? n : 256;
  }
  return counts[dev];
}

uint32_t launch_grid(uint64_t S, uint32_t per_block) {
  uint64_t need = (S + per_block - 1) / per_block;
  uint64_t cap = (uint64_t)device_cu_count() * 8;
  if (cap > kMaxGrid) cap = kMaxGrid;
  uint64_t g = need < cap ? need : cap;
  return (uint32_t)(g == 0 ? 1 : g);
}

uint32_t occupancy_blocks(const void* kernel, int block, size_t dyn_lds) {
  static std::mutex mu;
  static std::map<std::tuple<const void*, int, int, size_t>, int> cache;
  int dev = 0;
  PGA_HIP_CHECK(hipGetDevice(&dev));
  const auto key = std::make_tuple(kernel, dev, block, dyn_lds);
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return (uint32_t)it->second;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, dyn_lds) != hipSuccess || n <= 0) n = 1;
  cache[key] = n;
  return (uint32_t)n;
}

bool force_generic_kernels() {
  static const bool v = [] {
    const char* e = getenv("PGA_FORCE_GENERIC");
    return e && e[0] == '1';
  }();
  return v;
}

size_t allow_dynamic_lds(const void* kernel) {
  // once per (kernel, device): the attribute is per device, so a process that
  // drives a second GPU raises it there too
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> raised;
  int dev = 0;
  PGA_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  auto it = raised.find({kernel, dev});
  if (it != raised.end()) return it->second;
  hipFuncAttributes at;
  PGA_HIP_CHECK(hipFuncGetAttributes(&at, kernel));
  const size_t avail = 160 * 1024 - at.sharedSizeBytes;
  PGA_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)avail));
  raised[{kernel, dev}] = avail;
  return avail;
}

TpGeom tp_geometry(uint64_t S, uint32_t islands, const void* kernel, uint32_t ng, uint32_t pseg) {
  (void)allow_dynamic_lds(kernel);  // the 16-wave launch's dynamic LDS is above the default limit
  return tp_geometry_occ(S, islands, occupancy_blocks(kernel, 256, dev::tp_dyn_lds(4, pseg)), ng, pseg);
}

uint32_t tp_dyn_lds_bytes(uint32_t nw, uint32_t pseg) { return dev::tp_dyn_lds(nw, pseg); }
uint32_t tp_jit_stage_bytes(uint32_t nw) { return dev::tp_jit_stage_lds(nw); }

uint32_t tp_skew_units(const TpGeom& t, uint64_t S) {
  // PGA_TP_SKEW = units each odd block of a pair hands to its even
  // neighbour (one 16-wave block per CU only: there block b runs on XCD b % 8;
  // at most a quarter of a block's units)
  static const uint32_t d = [] {
    // default 2 of the 64 units of the headline's blocks: interleaved A/B
    // (round 4) 0 / 2 / 4 / 6 -> 90.7 / 90.2 / 92.7 / 95.4 us per generation
    const char* e = std::getenv("PGA_TP_SKEW");
    return e ? (uint32_t)std::strtoul(e, nullptr, 10) : 2u;
  }();
  if (d == 0 || t.block != dev::kTpMaxWaves * 64 || t.grid < 2) return 0;
  const uint64_t per = (S + t.grid - 1) / t.grid, units = (per + t.unit - 1) / t.unit;
  return d * 4 < units ? d : 0u;
}

uint32_t tp_tail_units(const TpGeom& t, uint32_t gs, uint32_t used, size_t avail) {
  // PGA_TP_TAIL = the last units of a 16-wave block's round that are bred
  // step by step by whichever wave is free (binary_dev.hpp, TAIL); 0: none
  static const uint32_t d = [] {
    const char* e = std::getenv("PGA_TP_TAIL");
    return e ? (uint32_t)std::strtoul(e, nullptr, 10) : kTpTailDefault;
  }();
  // the unit loop's launches at GS 8 only (binary_dev.hpp TAILF): 64-child units of 8 steps on the 16-wave block
  if (d == 0 || t.block != dev::kTpMaxWaves * 64 || t.unit != 64 || gs != 8) return 0;
  uint32_t n = d < dev::kTpMaxTail ? d : dev::kTpMaxTail;
  const size_t off = dev::tp_tail_off(used);
  if (off >= avail) return 0;
  const size_t fit = (avail - off) / dev::kTpTailUnitBytes;  // what the CU's LDS leaves: fewer tail units, not a failed launch
  return n < fit ? n : (uint32_t)fit;
}

TpGeom tp_geometry_occ(uint64_t S, uint32_t islands, uint32_t occ4, uint32_t ng, uint32_t pseg) {
  if (islands == 0) islands = 1;
  if (ng == 0 || ng > 64) ng = 64;
  const uint32_t cus = (uint32_t)device_cu_count();
  const uint32_t share = cus / islands > 0 ? cus / islands : 1;
  // one 16-wave block per CU when every wave breeds at least one 64-child unit
  if ((S + 63) / 64 >= (uint64_t)dev::kTpMaxWaves * share)
    return {share, dev::kTpMaxWaves * 64, dev::tp_dyn_lds(dev::kTpMaxWaves, pseg), 64};
  // else 4-wave blocks on the occupancy grid, with units small enough that
  // every resident wave gets one (each unit costs U / ng dependent steps)
  uint64_t cap = (uint64_t)cus * (occ4 > 0 ? occ4 : 1) / islands;
  if (cap < 1) cap = 1;
  if (cap > kMaxGrid) cap = kMaxGrid;
  const uint64_t per_wave = (S + 4 * cap - 1) / (4 * cap);
  uint32_t u = ng * dev::tp_prefetch_depth(64 / ng);  // a unit holds >= PD steps
  static const uint32_t umax = [] {  // PGA_TP_UMAX: largest unit of this grid (sweeps)
    const char* e = std::getenv("PGA_TP_UMAX");
    return e ? (uint32_t)std::strtoul(e, nullptr, 10) : 64u;
  }();
  while (u < 64 && u < per_wave && 2 * u <= umax) u *= 2;
  const uint64_t need = (S + 4ull * u - 1) / (4ull * u);
  const uint64_t g = need < cap ? need : cap;
  return {(uint32_t)(g == 0 ? 1 : g), 256u, dev::tp_dyn_lds(4, pseg), u};
}

uint32_t launch_grid_occ(uint64_t S, uint32_t per_block, const void* kernel) {
  uint64_t need = (S + per_block - 1) / per_block;
  uint64_t cap = (uint64_t)device_cu_count() * occupancy_blocks(kernel, dev::kBlock);
  if (cap > kMaxGrid) cap = kMaxGrid;
  uint64_t g = need < cap ? need : cap;
  return (uint32_t)(g == 0 ? 1 : g);
}

void build_mut_table(float p, uint32_t L, uint32_t* out, float* inv_log2_1mp) {
  const double q = 1.0 - (double)p;
  double t = 1.0;
  for (uint32_t m = 1; m <= L; ++m) {
    t *= q;
    double v = std::floor(t * 4294967296.0);
    out[m - 1] = v >= 4294967295.0 ? 0xFFFFFFFFu : (v <= 0.0 ? 0u : (uint32_t)v);
  }
  if (p <= 0.f) *inv_log2_1mp = 0.f;
  else if (p >= 1.f) *inv_log2_1mp = 0.f;
  else *inv_log2_1mp = (float)(1.0 / std::log2(q));
}

void build_binom_table(float p, uint32_t L, uint32_t* out) {
  // out[k] = floor(P(K <= k) * 2^32), K ~ Binomial(L, p); 0xFFFFFFFF once the
  // remaining tail is below 2^-32 (ends the table, see binom_count)
  const long double pp = p, qq = 1.0L - pp;
  long double pmf = expl((long double)L * log1pl(-pp)), cdf = 0.0L;
  for (uint32_t k = 0; k < kMutCap; ++k) {
    cdf += pmf;
    const long double v = floorl(cdf * 4294967296.0L);
    out[k] = v >= 4294967295.0L ? 0xFFFFFFFFu : (uint32_t)v;
    pmf = k < L ? pmf * (long double)(L - k) / (long double)(k + 1) * pp / qq : 0.0L;
  }
  out[kMutCap - 1] = 0xFFFFFFFFu;
}

namespace {
using namespace dev;

__global__ __launch_bounds__(kBlock) void reduce_best_kernel(const unsigned long long* parts, uint32_t n,
                                                             unsigned long long* out) {
  __shared__ unsigned long long lds[kBlock / 64];
  unsigned long long b = block_reduce_parts(parts, n, lds);
  if (threadIdx.x == 0) out[0] = b;
}

// per-block best partials of a score array; with `keys` also refreshes the
// u16 tournament keys in the same pass (integer objectives)
__global__ __launch_bounds__(kBlock) void best_of_scores_kernel(const float* scores, uint64_t S,
                                                                unsigned long long* parts, uint16_t* keys) {
  __shared__ unsigned long long lds[kBlock / 64];
  unsigned long long b = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < S; i += (uint64_t)gridDim.x * kBlock) {
    const float v = scores[i];
    unsigned long long p = pack_best(v, i);
    b = p > b ? p : b;
    if (keys) keys[i] = score_to_key16(v);
  }
  b = block_max_u64(b, lds);
  if (threadIdx.x == 0) parts[blockIdx.x] = b;
}

struct FMin { __device__ float operator()(float a, float b) const { return fminf(a, b); } };
struct FMax { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct FAdd { __device__ float operator()(float a, float b) const { return a + b; } };

// stage 1: per-block {min, max, sum}
__global__ __launch_bounds__(kBlock) void stats_part_kernel(const float* s, uint64_t S, float* parts) {
  __shared__ float lds[kBlock / 64];
  float mn = INFINITY, mx = -INFINITY, sm = 0.f;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < S; i += (uint64_t)gridDim.x * kBlock) {
    float v = s[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    sm += v;
  }
  mn = block_reduce(mn, lds, FMin());
  mx = block_reduce(mx, lds, FMax());
  sm = block_reduce(sm, lds, FAdd());
  if (threadIdx.x == 0) {
    parts[3 * blockIdx.x + 0] = mn;
    parts[3 * blockIdx.x + 1] = mx;
    parts[3 * blockIdx.x + 2] = sm;
  }
}

__global__ __launch_bounds__(kBlock) void stats_final_kernel(const float* parts, uint32_t n, uint64_t S,
                                                             float* out) {
  __shared__ float lds[kBlock / 64];
  float mn = INFINITY, mx = -INFINITY, sm = 0.f;
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
    mn = fminf(mn, parts[3 * i]);
    mx = fmaxf(mx, parts[3 * i + 1]);
    sm += parts[3 * i + 2];
  }
  mn = block_reduce(mn, lds, FMin());
  mx = block_reduce(mx, lds, FMax());
  sm = block_reduce(sm, lds, FAdd());
  if (threadIdx.x == 0) {
    out[0] = mn;
    out[1] = mx;
    out[2] = sm;
    out[3] = (float)S;
  }
}

// roulette: contiguous range per block, weights = max(s - min, 0)
__device__ __forceinline__ float block_excl_scan(float v, float* lds, float& total) {
  // inclusive wave scan
  const uint32_t lane = lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    float t = __shfl_up(v, o, 64);
    if (lane >= (uint32_t)o) v += t;
  }
  __syncthreads();
  if (lane == 63) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float off = 0.f;
  total = 0.f;
  for (int i = 0; i < kBlock / 64; ++i) {
    if (i < (int)(threadIdx.x >> 6)) off += lds[i];
    total += lds[i];
  }
  return off + v;  // inclusive
}

// Roulette in three launches: PART (per-block weight sums), FINAL (each block
// reduces the sums before it for its carry, scans its range into cumfit; the
// last block publishes the guide scale), GUIDE (bucket -> first individual).
// The score minimum comes from the generation kernel's fused {min, sum}
// partials when it stored them (PART reduces them in every block and block 0
// publishes it), else from score_stats_launch beforehand.
__device__ __forceinline__ float parts_min(const float* parts, uint32_t n, float* lds) {
  float mn = INFINITY;
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) mn = fminf(mn, parts[2 * i]);
  return block_reduce(mn, lds, FMin());
}

__global__ __launch_bounds__(kBlock) void prefix_part_kernel(const float* s, uint64_t S, uint64_t per_block,
                                                             const float* parts, uint32_t nparts, float* stats,
                                                             float* block_sums) {
  __shared__ float lds[kBlock / 64];
  float mn;
  if (parts) {
    mn = parts_min(parts, nparts, lds);
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[0] = mn;
  } else {
    mn = stats[0];
  }
  const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
  const uint64_t b1 = b0 + per_block < S ? b0 + per_block : S;
  float sm = 0.f;
  for (uint64_t i = b0 + threadIdx.x; i < b1; i += kBlock) sm += fmaxf(s[i] - mn, 0.f);
  sm = block_reduce(sm, lds, FAdd());
  if (threadIdx.x == 0) block_sums[blockIdx.x] = sm;
}

__global__ __launch_bounds__(kBlock) void prefix_final_kernel(const float* s, uint64_t S, uint64_t per_block,
                                                              const float* stats, const float* block_sums,
                                                              float* cumfit, float* meta) {
  __shared__ float lds[kBlock / 64];
  const float mn = stats[0];
  // carry = the sums of the blocks before this one, in a fixed order
  float pre = 0.f;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kBlock) pre += block_sums[j];
  float carry = block_reduce(pre, lds, FAdd());
  const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
  const uint64_t b1 = b0 + per_block < S ? b0 + per_block : S;
  for (uint64_t t0 = b0; t0 < b1; t0 += kBlock) {
    uint64_t i = t0 + threadIdx.x;
    float v = i < b1 ? fmaxf(s[i] - mn, 0.f) : 0.f;
    float total;
    float inc = block_excl_scan(v, lds, total);
    if (i < b1) cumfit[i] = carry + inc;
    if (i == S - 1) meta[0] = carry + inc > 0.f ? (float)S / (carry + inc) : 0.f;  // guide scale (roulette_bucket)
    carry += total;
    __syncthreads();
  }
}

// Integer objectives: the same two passes with u64 weight sums, so cumfit[i]
// is the exact prefix rounded once to f32 — what roulette_fused_kernel and the
// CPU backend's f64 prefix give, at any population size.
template <int BLK>
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
  for (uint32_t w = 0; w < BLK / 64; ++w) t += lds[w];
  return t;
}

__global__ __launch_bounds__(kBlock) void prefix_part_int_kernel(const float* s, uint64_t S, uint64_t per_block,
                                                                 const float* parts, uint32_t nparts, float* stats,
                                                                 unsigned long long* block_sums) {
  __shared__ float lds[kBlock / 64];
  __shared__ unsigned long long lds64[kBlock / 64];
  float mn;
  if (parts) {
    mn = parts_min(parts, nparts, lds);
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[0] = mn;
  } else {
    mn = stats[0];
  }
  const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
  const uint64_t b1 = b0 + per_block < S ? b0 + per_block : S;
  unsigned long long sm = 0;
  for (uint64_t i = b0 + threadIdx.x; i < b1; i += kBlock) sm += (unsigned long long)fmaxf(s[i] - mn, 0.f);
  sm = block_sum_u64<kBlock>(sm, lds64);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = sm;
}

__global__ __launch_bounds__(kBlock) void prefix_final_int_kernel(const float* s, uint64_t S, uint64_t per_block,
                                                                  const float* stats,
                                                                  const unsigned long long* block_sums, float* cumfit,
                                                                  float* meta) {
  __shared__ unsigned long long lds64[kBlock / 64];
  const float mn = stats[0];
  unsigned long long pre = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kBlock) pre += block_sums[j];
  unsigned long long carry = block_sum_u64<kBlock>(pre, lds64);
  const uint32_t lane = lane_id(), wid = threadIdx.x >> 6;
  const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
  const uint64_t b1 = b0 + per_block < S ? b0 + per_block : S;
  for (uint64_t t0 = b0; t0 < b1; t0 += kBlock) {
    const uint64_t i = t0 + threadIdx.x;
    const unsigned long long v = i < b1 ? (unsigned long long)fmaxf(s[i] - mn, 0.f) : 0ull;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(inc, o, 64);
      if (lane >= (uint32_t)o) inc += y;
    }
    __syncthreads();
    if (lane == 63) lds64[wid] = inc;
    __syncthreads();
    unsigned long long off = 0, total = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
      off += w < wid ? lds64[w] : 0ull;
      total += lds64[w];
    }
    const float c = __ull2float_rn(carry + off + inc);
    if (i < b1) cumfit[i] = c;
    if (i == S - 1) meta[0] = c > 0.f ? (float)S / c : 0.f;  // guide scale (roulette_bucket)
    carry += total;
  }
}

// guide[b] = i for every bucket b in (bucket(cumfit[i-1]), bucket(cumfit[i])].
// Spans of 32 buckets or more (one individual holding >= 32/S of the total
// weight) are queued in LDS and filled by the whole block, so no thread loops
// over a heavy individual's buckets.
// cov: kGuideCovered, or 0 (no covered flags: S >= 2^31)
__global__ __launch_bounds__(kBlock) void roulette_guide_kernel(const float* c, uint64_t S, const float* meta,
                                                                 uint32_t* guide, uint32_t cov) {
  __shared__ uint4 spans[kBlock];
  __shared__ uint32_t nsp;
  const float scale = meta[0];
  const uint32_t B = (uint32_t)S;
  for (uint64_t t0 = (uint64_t)blockIdx.x * kBlock; t0 < S; t0 += (uint64_t)gridDim.x * kBlock) {  // block-uniform
    if (threadIdx.x == 0) nsp = 0;
    __syncthreads();
    const uint64_t i = t0 + threadIdx.x;
    if (i < S) {
      const float ci = c[i];
      const uint32_t hi = roulette_bucket(ci, scale, B);
      const uint32_t lo = i ? roulette_bucket(c[i - 1], scale, B) + 1u : 0u;
      if (hi >= lo) {
        if (hi - lo < 32u) {
          for (uint32_t b = lo; b <= hi; ++b) guide[b] = (uint32_t)i | (b < hi ? cov : 0u);
        } else {
          spans[atomicAdd(&nsp, 1u)] = make_uint4(lo, hi, (uint32_t)i, 0u);
        }
      }
    }
    __syncthreads();
    const uint32_t n = nsp;
    for (uint32_t k = 0; k < n; ++k) {
      const uint4 sp = spans[k];
      for (uint32_t b = sp.x + threadIdx.x; b <= sp.y; b += kBlock) guide[b] = sp.z | (b < sp.y ? cov : 0u);
    }
    __syncthreads();
  }
}

// Roulette in ONE launch for an integer objective (roulette_fused_launch):
// block j of this grid takes the children block j of the generation kernel
// wrote (tp_share over the same grid), whose {min, sum} partials are exact
// integers in f32.  Every block reduces all partials itself: the minimum, the
// weight total sum_i - n_i * min of every partial, the total and the sum of
// the partials before it (its carry), in u64 — so the three-launch chain
// (partials pass, carry + scan, guide) becomes one, and the prefix sums are
// exact (cumfit[i] = the integer prefix rounded once; the guide scale is
// S / cumfit[S - 1] as in prefix_final_kernel).  The block then scans its
// range (kRoulPer consecutive individuals per thread, loaded and stored
// coalesced through LDS) and fills the guide
// buckets of its individuals as roulette_guide_kernel does.
constexpr uint32_t kRoulThreads = 1024, kRoulPer = 8, kRoulSpans = 1024;

__global__ __launch_bounds__(kRoulThreads) void roulette_fused_kernel(const float* __restrict__ s, uint64_t S,
                                                                      const float* __restrict__ parts, uint32_t unit,
                                                                      uint32_t skew, float* __restrict__ cumfit,
                                                                      uint32_t* __restrict__ guide, float* meta,
                                                                      uint32_t cov) {
  __shared__ unsigned long long red[kRoulThreads / 64];
  __shared__ float fred[kRoulThreads / 64];
  __shared__ uint32_t wsum[kRoulThreads / 64];
  __shared__ uint4 spans[kRoulSpans];
  __shared__ uint32_t nsp;
  __shared__ __align__(16) uint32_t xch[kRoulThreads * kRoulPer];  // a chunk's weights, then its cumfit values
  const uint32_t t = threadIdx.x, lane = lane_id(), wid = t >> 6, np = gridDim.x;
  const uint32_t Su = (uint32_t)S;
  uint32_t bb, be;
  tp_share(Su, unit, blockIdx.x, bb, be, skew);
  // the first chunk's scores, loaded before the partials are reduced (the two
  // global round trips overlap; a share of up to kRoulThreads * kRoulPer, the
  // usual case, is this one chunk)
  float sv0[kRoulPer];
#pragma unroll
  for (uint32_t k = 0; k < kRoulPer; ++k) {
    const uint32_t i = bb + k * kRoulThreads + t;
    sv0[k] = s[i < be ? i : (be > 0u ? be - 1u : 0u)];  // unconditional load
  }
  float mn = __builtin_inff();
  for (uint32_t i = t; i < np; i += kRoulThreads) mn = fminf(mn, parts[2 * i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if (lane == 0) fred[wid] = mn;
  __syncthreads();
  mn = fred[0];
  for (uint32_t w = 1; w < kRoulThreads / 64; ++w) mn = fminf(mn, fred[w]);
  const unsigned long long mnu = (unsigned long long)mn;  // an integer objective's scores are >= 0
  unsigned long long below = 0, tot = 0;
  for (uint32_t i = t; i < np; i += kRoulThreads) {
    uint32_t b0, b1;
    tp_share(Su, unit, i, b0, b1, skew);
    const unsigned long long w = b1 > b0 ? (unsigned long long)parts[2 * i + 1] - (unsigned long long)(b1 - b0) * mnu : 0ull;
    tot += w;
    below += i < blockIdx.x ? w : 0ull;
  }
  tot = block_sum_u64<kRoulThreads>(tot, red);
  below = block_sum_u64<kRoulThreads>(below, red);
  const float total = __ull2float_rn(tot);
  const float scale = tot > 0ull ? (float)S / total : 0.f;
  if (blockIdx.x == 0 && t == 0) meta[0] = scale;
  unsigned long long carry = below;
  for (uint32_t c0 = bb; c0 < be; c0 += kRoulThreads * kRoulPer) {  // block-uniform
    // coalesced loads, transposed through LDS: thread t scans the kRoulPer
    // consecutive weights [t P, t P + P) of the chunk
#pragma unroll
    for (uint32_t k = 0; k < kRoulPer; ++k) {
      const uint32_t i = c0 + k * kRoulThreads + t;
      const float v = i < be ? (c0 == bb ? sv0[k] : s[i]) : mn;
      xch[k * kRoulThreads + t] = (uint32_t)fmaxf(v - mn, 0.f);
    }
    if (t == 0) nsp = 0;
    __syncthreads();
    uint32_t w[kRoulPer], ts = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRoulPer; j += 4) {
      const uint4 q = *(const uint4*)&xch[t * kRoulPer + j];
      w[j] = q.x;
      w[j + 1] = q.y;
      w[j + 2] = q.z;
      w[j + 3] = q.w;
    }
#pragma unroll
    for (uint32_t j = 0; j < kRoulPer; ++j) ts += w[j];
    uint32_t incl = ts;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();  // (every thread has read its weights: xch is reused for the prefix sums)
    uint32_t off = incl - ts, ctot = 0;
    for (uint32_t q = 0; q < kRoulThreads / 64; ++q) {
      off += q < wid ? wsum[q] : 0u;
      ctot += wsum[q];
    }
    unsigned long long run = carry + off;  // the exact prefix before the thread's first individual
    float c[kRoulPer];
#pragma unroll
    for (uint32_t j = 0; j < kRoulPer; ++j) {
      run += w[j];
      c[j] = __ull2float_rn(run);
    }
#pragma unroll
    for (uint32_t j = 0; j < kRoulPer; j += 4)
      *(float4*)&xch[t * kRoulPer + j] = make_float4(c[j], c[j + 1], c[j + 2], c[j + 3]);
    __syncthreads();
    // coalesced stores; the guide buckets of individual i, as roulette_guide_kernel
    const float prev0 = __ull2float_rn(carry);  // = cumfit[c0 - 1]
#pragma unroll
    for (uint32_t k = 0; k < kRoulPer; ++k) {
      const uint32_t e = k * kRoulThreads + t, i = c0 + e;
      if (i < be) {
        const float ci = __builtin_bit_cast(float, xch[e]);
        const float prev = e ? __builtin_bit_cast(float, xch[e - 1]) : prev0;
        cumfit[i] = ci;
        const uint32_t hi = roulette_bucket(ci, scale, Su);
        const uint32_t lo = i ? roulette_bucket(prev, scale, Su) + 1u : 0u;
        if (hi >= lo) {
          const uint32_t q = hi - lo < 32u ? kRoulSpans : atomicAdd(&nsp, 1u);
          if (q < kRoulSpans) spans[q] = make_uint4(lo, hi, i, 0u);
          else
            for (uint32_t b = lo; b <= hi; ++b) guide[b] = i | (b < hi ? cov : 0u);  // short span (or a full queue)
        }
      }
    }
    __syncthreads();
    const uint32_t n = nsp < kRoulSpans ? nsp : kRoulSpans;
    for (uint32_t q = 0; q < n; ++q) {
      const uint4 sp = spans[q];
      for (uint32_t b = sp.x + t; b <= sp.y; b += kRoulThreads) guide[b] = sp.z | (b < sp.y ? cov : 0u);
    }
    __syncthreads();  // (nsp, wsum and xch are reused by the next chunk)
    carry += ctot;
  }
}

__global__ __launch_bounds__(kBlock) void scores_to_keys_kernel(const float* s, uint64_t S, uint16_t* k) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < S; i += (uint64_t)gridDim.x * kBlock)
    k[i] = score_to_key16(s[i]);
}

__global__ __launch_bounds__(kBlock) void scores_to_qkeys_kernel(const float* s, uint64_t S, const float* mm,
                                                                  uint16_t* k) {
  float lo, scale;
  qkey_params(mm[0], mm[1], lo, scale);
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < S; i += (uint64_t)gridDim.x * kBlock)
    k[i] = (uint16_t)qkey(s[i], lo, scale);
}

__global__ void advance_counter_kernel(uint32_t* c, uint32_t d) {
  if (threadIdx.x == 0) *c += d;
}

}  // namespace

void advance_counter_launch(uint32_t* counter, uint32_t delta, hipStream_t s) {
  hipLaunchKernelGGL(advance_counter_kernel, 1, 64, 0, s, counter, delta);
  PGA_HIP_CHECK(hipGetLastError());
}

void reduce_best_launch(const unsigned long long* parts, uint32_t n, unsigned long long* out, hipStream_t s) {
  hipLaunchKernelGGL(reduce_best_kernel, 1, kBlock, 0, s, parts, n, out);
  PGA_HIP_CHECK(hipGetLastError());
}

uint32_t best_of_scores_launch(const float* scores, uint64_t S, unsigned long long* parts, hipStream_t s,
                               uint16_t* keys) {
  uint32_t grid = launch_grid(S, kBlock * 4);
  hipLaunchKernelGGL(best_of_scores_kernel, grid, kBlock, 0, s, scores, S, parts, keys);
  PGA_HIP_CHECK(hipGetLastError());
  return grid;
}

void scores_to_keys_launch(const float* scores, uint64_t S, uint16_t* keys, hipStream_t s) {
  uint32_t grid = launch_grid(S, kBlock * 4);
  hipLaunchKernelGGL(scores_to_keys_kernel, grid, kBlock, 0, s, scores, S, keys);
  PGA_HIP_CHECK(hipGetLastError());
}

void scores_to_qkeys_launch(const float* scores, uint64_t S, const float* mm, uint16_t* keys, hipStream_t s) {
  uint32_t grid = launch_grid(S, kBlock * 4);
  hipLaunchKernelGGL(scores_to_qkeys_kernel, grid, kBlock, 0, s, scores, S, mm, keys);
  PGA_HIP_CHECK(hipGetLastError());
}

// {min, max, sum, count} of a generation from the fused partials its kernel
// stored: {min, sum} pairs (GenArgs::stats_parts) and packed bests (the max)
__global__ __launch_bounds__(kBlock) void stats_from_parts_kernel(const float* parts, const unsigned long long* best,
                                                                 uint32_t n, uint64_t S, float* out) {
  __shared__ float lds[kBlock / 64];
  __shared__ unsigned long long lds_b[kBlock / 64];
  float mn = INFINITY, sm = 0.f;
  unsigned long long b = 0;
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
    mn = fminf(mn, parts[2 * i]);
    sm += parts[2 * i + 1];
    b = best[i] > b ? best[i] : b;
  }
  mn = block_reduce(mn, lds, FMin());
  sm = block_reduce(sm, lds, FAdd());
  b = block_max_u64(b, lds_b);
  if (threadIdx.x == 0) {
    out[0] = mn;
    out[1] = best_score(b);
    out[2] = sm;
    out[3] = (float)S;
  }
}

void stats_from_parts_launch(const float* parts, const unsigned long long* best, uint32_t n, uint64_t S, float* out,
                             hipStream_t s) {
  hipLaunchKernelGGL(stats_from_parts_kernel, 1, kBlock, 0, s, parts, best, n, S, out);
  PGA_HIP_CHECK(hipGetLastError());
}

void score_stats_launch(const float* scores, uint64_t S, float* stats, hipStream_t s) {
  // stats buffer layout: [0..4) result, [4..) 3*grid partials
  uint32_t grid = launch_grid(S, kBlock * 4);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(stats_part_kernel, grid, kBlock, 0, s, scores, S, stats + 4);
  hipLaunchKernelGGL(stats_final_kernel, 1, kBlock, 0, s, stats + 4, grid, S, stats);
  PGA_HIP_CHECK(hipGetLastError());
}

size_t roulette_workspace_floats(uint64_t S) {
  // stats | stats partials | block sums | scale, pad | u64 block sums (integer objectives)
  (void)S;
  return kRoulScale + 4 + 2 * 1024;
}

void roulette_prefix_launch(const float* scores, uint64_t S, const float* parts, uint32_t nparts, float* cumfit,
                            float* ws, hipStream_t s, bool integer) {
  // ws layout: [0..4) stats, [4 .. 4+3*1024) stats partials, then block sums, then [kRoulScale] the guide scale
  if (!parts) score_stats_launch(scores, S, ws, s);
  uint32_t grid = launch_grid(S, kBlock * 4);
  if (grid > 1024) grid = 1024;
  const uint64_t per_block = (S + grid - 1) / grid;
  float* block_sums = ws + 4 + 3 * 1024;
  if (integer) {
    unsigned long long* sums64 = (unsigned long long*)(ws + kRoulScale + 4);
    hipLaunchKernelGGL(prefix_part_int_kernel, grid, kBlock, 0, s, scores, S, per_block, parts, nparts, ws, sums64);
    hipLaunchKernelGGL(prefix_final_int_kernel, grid, kBlock, 0, s, scores, S, per_block, ws,
                       (const unsigned long long*)sums64, cumfit, ws + kRoulScale);
  } else {
    hipLaunchKernelGGL(prefix_part_kernel, grid, kBlock, 0, s, scores, S, per_block, parts, nparts, ws, block_sums);
    hipLaunchKernelGGL(prefix_final_kernel, grid, kBlock, 0, s, scores, S, per_block, ws, block_sums, cumfit,
                       ws + kRoulScale);
  }
  PGA_HIP_CHECK(hipGetLastError());
}

// the guide's covered flag (tp.hpp reads it only while S < 2^31)
static uint32_t guide_cover_flag(uint64_t S) { return S <= kGuideIndexMask ? kGuideCovered : 0u; }

bool roulette_fused_launch(const float* scores, uint64_t S, const float* parts, const TpPartition& part,
                           uint32_t max_score, float* cumfit, uint32_t* guide, float* ws, hipStream_t s) {
  if (!parts || part.grid == 0 || part.unit == 0 || S == 0 || S > 0xFFFFFFFFull) return false;
  // the largest share (tp_share: ceil(S / grid) in whole units, plus the skew)
  // times the largest score stays below 2^24, so every f32 partial sum is exact
  const uint64_t per = ((S + part.grid - 1) / part.grid + part.unit - 1) / part.unit * part.unit;
  const uint64_t share = per + (uint64_t)part.skew * part.unit;
  if (share * (uint64_t)max_score >= (1ull << 24)) return false;
  // a chunk's u32 weight sum: kRoulThreads * kRoulPer * max_score < 2^32
  if ((uint64_t)kRoulThreads * kRoulPer * max_score >= (1ull << 32)) return false;
  hipLaunchKernelGGL(roulette_fused_kernel, part.grid, kRoulThreads, 0, s, scores, S, parts, part.unit, part.skew, cumfit,
                     guide, ws + kRoulScale, guide_cover_flag(S));
  PGA_HIP_CHECK(hipGetLastError());
  return true;
}

void roulette_guide_launch(const float* cumfit, uint64_t S, uint32_t* guide, float* ws, hipStream_t s) {
  const uint32_t grid = launch_grid(S, kBlock);
  hipLaunchKernelGGL(roulette_guide_kernel, grid, kBlock, 0, s, cumfit, S, (const float*)(ws + kRoulScale), guide,
                     guide_cover_flag(S));
  PGA_HIP_CHECK(hipGetLastError());
}

}  // namespace pga
