// island.cpp — native GA runtime (see island.hpp).
#include "pga/island.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "pga/cpu.hpp"
#include "pga/ops.hpp"
#include "pga/perm_ops.hpp"
#include "pga/qubo_ops.hpp"
#include "pga/trace.hpp"

namespace pga {

void row_geometry(int32_t encoding, uint32_t L, uint32_t* row_words, uint32_t* chunks) {
  uint32_t c = 0;
  switch (encoding) {
    case ENC_BINARY: c = (L + 127) / 128; break;
    case ENC_REAL: c = (L + 3) / 4; break;
    case ENC_PERMUTATION: c = (L + 7) / 8; break;
    default: throw std::invalid_argument("unknown encoding");
  }
  if (c == 0) c = 1;
  *chunks = c;
  *row_words = 4 * c;
}

namespace {
bool per_individual_mutation(int32_t m) { return m == MUT_RESET_ONE || m == MUT_SWAP || m == MUT_INVERSION; }
uint32_t prob_thresh(float p) {
  double v = std::floor((double)p * 4294967296.0);
  return v >= 4294967295.0 ? 0xFFFFFFFFu : (v <= 0 ? 0u : (uint32_t)v);
}
// A/B knobs: NAME=0 turns a path off (each read once, where it is used)
bool env_off(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '0';
}
bool roul_fused_off() {  // PGA_ROUL_FUSED=0: the three-launch roulette prefix
  static const bool off = env_off("PGA_ROUL_FUSED");
  return off;
}
const char kJitNotTwoOpt[] = "2-opt local search needs a built-in TSP objective, not a JIT objective";
const char kJitNotOrOpt[] = "Or-opt local search needs a built-in TSP objective, not a JIT objective";
const char kJitNotOneFlip[] = "one-flip local search needs the built-in QUBO objective, not a JIT objective";
}  // namespace

Buffer::Buffer(size_t n, bool device) : bytes(n), device_(device) {
  if (n == 0) return;
  if (device) {
    PGA_HIP_CHECK(hipMalloc(&ptr, n));
  } else {
    ptr = std::aligned_alloc(64, (n + 63) & ~(size_t)63);
    if (!ptr) throw std::bad_alloc();
    std::memset(ptr, 0, n);
  }
}

Buffer::~Buffer() {
  if (!ptr) return;
  if (device_) (void)hipFree(ptr);
  else std::free(ptr);
}

bool Island::reserve(Buffer& b, size_t bytes, bool sync) {
  if (b.bytes >= bytes) return false;
  if (sync) synchronize();
  return b.reserve(bytes, on_gpu());
}

Island::Island(const Config& cfg, int device) : cfg_(cfg), device_(device) {
  if (cfg_.S == 0) throw std::invalid_argument("population size must be > 0");
  if (cfg_.S >= (1ull << 32)) throw std::invalid_argument("population size must be < 2^32");
  if (cfg_.L == 0) throw std::invalid_argument("genome length must be > 0");
  if (cfg_.encoding == ENC_PERMUTATION && cfg_.L > 65536) throw std::invalid_argument("permutation length > 65536");
  if (cfg_.island >= 65536) throw std::invalid_argument("island id must be < 65536");
  row_geometry(cfg_.encoding, cfg_.L, &row_words_, &chunks_);
  if (on_gpu()) PGA_HIP_CHECK(hipSetDevice(device_));
  const uint64_t Sp = cfg_.S + kRowPad;  // padded (ops.hpp kRowPad)
  const size_t rb = 4ull * row_words_ * Sp;
  for (int i = 0; i < 2; ++i) {
    reserve(rows_[i], rb);
    reserve(scores_[i], 4ull * Sp);
    reserve(best_[i], 8ull * kMaxGrid);
    if (on_gpu()) reserve(stats_parts_[i], 8ull * kMaxGrid);
    reserve(keys_[i], 2ull * Sp);
  }
  reserve(out_best_, 64);
  reserve(stats_, 4ull * (4 + 3 * 1024));
  aux_on_ = std::getenv("PGA_TSP_NO_LDS") == nullptr;  // verification: the f32 L2 matrix path
  if (cfg_.encoding == ENC_BINARY) {
    const uint32_t rem = cfg_.L - 128 * (chunks_ - 1);
    uint32_t m[4];
    for (uint32_t j = 0; j < 4; ++j) m[j] = range_mask32(32 * j, 0, rem);
    last_mask_ = u32x4{m[0], m[1], m[2], m[3]};
  } else {
    last_mask_ = u32x4{~0u, ~0u, ~0u, ~0u};
  }
  set_operators(cfg_);
  if (const char* e = std::getenv("PGA_GRAPH")) set_graph_generations((uint32_t)std::strtoul(e, nullptr, 10));
}

Island::~Island() {
  // the graph exec and the capture stream go before the buffers (the members) do
  drop_graph();
  if (cap_stream_) (void)hipStreamDestroy(cap_stream_);
}

void* Island::scratch(size_t bytes) {
  reserve(scratch_, bytes, /*sync=*/scratch_.ptr != nullptr);
  return scratch_.ptr;
}

// ------------------------------------------------- per-parity record ---
void Island::scores_written(int p, const Derived& made) {
  d_[p] = made;
  if (made.rank_cnt) d_[p ^ 1].rank_cnt = false;  // one workspace
  if (made.fhist >= 0) {
    const int z = (made.fhist + 1) % 3;
    fhist_clean_[made.fhist] = true;  // zeroed (bins and status) by the launch before this one
    fhist_clean_[z] = true;           // zeroed by this launch
    if (d_[p ^ 1].fhist == z) d_[p ^ 1].fhist = -1;
    ++fhist_rot_;
  }
}

bool Island::take_rank_counts() {
  const bool ready = d_[cur_].rank_cnt && !capturing_;
  d_[0].rank_cnt = d_[1].rank_cnt = false;  // the sort scans them in place
  return ready;
}

void Island::drop_key_counts() {
  d_[0].fhist = d_[1].fhist = -1;
  d_[0].rank_cnt = d_[1].rank_cnt = false;
}

void Island::set_n_best(uint32_t n) {
  d_[cur_].n_best = n;
  d_[cur_].stats = false;
  d_[cur_].part = TpPartition{0, 0, 0};
}

void Island::copy_to_host(void* dst, const void* src, size_t bytes) {
  if (on_gpu()) {
    PGA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    PGA_HIP_CHECK(hipStreamSynchronize(stream));
  } else {
    std::memcpy(dst, src, bytes);
  }
}

void Island::copy_to_device(void* dst, const void* src, size_t bytes) {
  if (on_gpu()) {
    PGA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    PGA_HIP_CHECK(hipStreamSynchronize(stream));
  } else {
    std::memcpy(dst, src, bytes);
  }
}

void Island::synchronize() {
  if (on_gpu()) PGA_HIP_CHECK(hipStreamSynchronize(stream));
}

void Island::rebuild_mut_table() {
  const bool per_ind = per_individual_mutation(cfg_.mutation);
  mut_rate_eff_ = cfg_.mut_rate >= 0.f ? cfg_.mut_rate : (per_ind ? 0.01f : 1.f / (float)cfg_.L);
  if (mut_rate_eff_ > 1.f) mut_rate_eff_ = 1.f;
  std::vector<uint32_t> thr(kMutCap);
  build_mut_table(per_ind ? 0.f : mut_rate_eff_, kMutCap, thr.data(), &mut_inv_);
  // sparse samplers (K ~ Binomial(L, p), then K distinct positions): BINARY
  // bit-flip and REAL per-gene mutation at the usual ~1/L rates
  const bool per_gene = (cfg_.encoding == ENC_BINARY && cfg_.mutation == MUT_BIT_FLIP) ||
                        (cfg_.encoding == ENC_REAL && (cfg_.mutation == MUT_GAUSSIAN || cfg_.mutation == MUT_UNIFORM));
  mut_sparse_ = per_gene && bin_sparse_mutation(cfg_.L, mut_rate_eff_);
  if (mut_sparse_) build_binom_table(mut_rate_eff_, cfg_.L, thr.data());
  reserve(mut_thr_, 4ull * kMutCap);
  synchronize();
  copy_to_device(mut_thr_.ptr, thr.data(), 4ull * kMutCap);
}

void Island::set_operators(const Config& c) {
  config_changed();
  if (c.S != cfg_.S || c.L != cfg_.L || c.encoding != cfg_.encoding)
    throw std::invalid_argument("set_operators cannot change S, L or encoding");
  if (c.selection == SEL_TOURNAMENT && (c.tour_k < 1 || c.tour_k > 64))
    throw std::invalid_argument("tournament size must be in [1, 64]");
  if (c.n_elite > c.S) throw std::invalid_argument("elitism count exceeds population");
  if (c.selection < SEL_TOURNAMENT || c.selection > SEL_RANK) throw std::invalid_argument("unknown selection");
  if (c.selection == SEL_RANK && !(c.rank_pressure >= 1.f && c.rank_pressure <= 2.f))
    throw std::invalid_argument("rank pressure must be in [1, 2]");
  if (c.local_search != LS_NONE && c.local_search != LS_TWO_OPT && c.local_search != LS_ONE_FLIP &&
      c.local_search != LS_OR_OPT)
    throw std::invalid_argument("unknown local search");
  if (c.local_search == LS_ONE_FLIP && (c.encoding != ENC_BINARY || c.objective != OBJ_QUBO))
    throw std::invalid_argument("one-flip local search needs the BINARY encoding with the built-in QUBO objective");
  if (c.local_search == LS_TWO_OPT) {
    if (c.encoding != ENC_PERMUTATION) throw std::invalid_argument("2-opt local search needs the PERMUTATION encoding");
    if (c.objective != OBJ_TSP && c.objective != OBJ_TSP_OPEN && c.objective != OBJ_TSP_EUC)
      throw std::invalid_argument("2-opt local search needs a built-in TSP objective");
  }
  if (c.local_search == LS_OR_OPT) {
    if (c.encoding != ENC_PERMUTATION) throw std::invalid_argument("Or-opt local search needs the PERMUTATION encoding");
    if (c.objective != OBJ_TSP && c.objective != OBJ_TSP_OPEN && c.objective != OBJ_TSP_EUC)
      throw std::invalid_argument("Or-opt local search needs a built-in TSP objective");
  }
  const float old_rate = cfg_.mut_rate;
  const int32_t old_mut = cfg_.mutation;
  cfg_ = c;
  if (!mut_thr_.ptr || old_rate != c.mut_rate || old_mut != c.mutation) rebuild_mut_table();
  fhist_on_ = fhist_user_ || cfg_.n_elite > 1;  // elitism > 1 selects top-k every generation
  if (cfg_.n_elite > 1) reserve(elite_idx_, 4ull * cfg_.n_elite);
  if (cfg_.selection == SEL_ROULETTE) {
    reserve(cumfit_, 4ull * (cfg_.S + 4));  // + 4: the GEN kernels' 16-byte window loads (tp.hpp)
    if (on_gpu()) {
      reserve(cum_ws_, 4ull * roulette_workspace_floats(cfg_.S));
      reserve(roul_guide_, 4ull * (cfg_.S + 1));  // guide[0..S]: roulette_bucket's range
    }
  }
  if (cfg_.selection == SEL_RANK) {
    reserve(rank_order_, 4ull * cfg_.S);
    if (on_gpu()) reserve(rank_ws_, rank_order_workspace_bytes(cfg_.S));
  }
}

void Island::set_user_operators(void* xo, void* mut) {
  config_changed();
  if ((xo || mut) && !on_gpu()) throw std::invalid_argument("device function pointers need the GPU backend");
  if ((xo || mut) && cfg_.encoding != ENC_REAL)
    throw std::invalid_argument("user crossover/mutate callbacks need the REAL (float gene) encoding");
  user_xo_fn_ = xo;
  user_mut_fn_ = mut;
  if (xo || mut) reserve(compat_rand_, 4ull * cfg_.S * cfg_.L);
}

void Island::set_objective_data(const float* host, size_t n, int which) {
  config_changed();
  if (which < 0 || which > 1) throw std::invalid_argument("objective data slot must be 0 or 1");
  synchronize();
  obj_data_[which] = Buffer();  // a fresh buffer every time, the old one freed first
  obj_data_[which] = Buffer(4ull * (n ? n : 1), on_gpu());
  if (n) copy_to_device(obj_data_[which].ptr, host, 4ull * n);
  obj_len_[which] = n;
  if (which == 0) obj_host0_.assign(host, host + n);
  ++obj_version_;
}

void Island::prepare_knapsack() {
  if (cfg_.objective != OBJ_KNAPSACK || cfg_.encoding != ENC_BINARY || !on_gpu() || knap_version_ == obj_version_) return;
  knap_version_ = obj_version_;
  knap_dig_ = knap_cols_ = 0;
  std::vector<uint8_t> tab;
  if (obj_host0_.size() >= 2ull * cfg_.L &&
      build_knap_table(obj_host0_.data(), obj_host0_.data() + cfg_.L, cfg_.L, chunks_, tab, knap_dig_, knap_cols_)) {
    reserve(knap_tab_, tab.size());
    copy_to_device(knap_tab_.ptr, tab.data(), tab.size());
  }
}

void Island::prepare_tsp_matrix() {
  if ((cfg_.objective != OBJ_TSP && cfg_.objective != OBJ_TSP_OPEN) || cfg_.encoding != ENC_PERMUTATION || !on_gpu() ||
      aux_version_ == obj_version_)
    return;
  // the matrix for the LDS-resident tour evaluation (perm.hip perm_gen_fast
  // TBL, which reads it): an integer matrix (entries in [0, 65535]) as u16
  // -- when symmetric the row-major lower triangle with the diagonal, entry
  // (i, j <= i) at i (i + 1) / 2 + j (kind 1), else the full matrix (kind
  // 2); any other symmetric matrix as the f32 lower triangle in the same
  // layout (kind 3); an asymmetric float matrix stays in L2 (kind 0)
  aux_version_ = obj_version_;
  aux_kind_ = aux_bytes_ = 0;
  const uint32_t L = cfg_.L;
  const float* d = obj_host0_.data();
  // (only what can fit one CU's LDS: 160 KiB)
  const size_t tri = (size_t)L * (L + 1) / 2, lds = 160 * 1024;
  const bool have = obj_host0_.size() >= (size_t)L * L && L >= 2 && 2 * tri <= lds;
  bool ints = have;
  for (size_t i = 0; ints && i < (size_t)L * L; ++i) ints = d[i] >= 0.f && d[i] <= 65535.f && d[i] == std::floor(d[i]);
  const bool sym = have && matrix_symmetric();
  std::vector<uint8_t> t;
  auto put = [&t](const auto v) {
    const size_t o = t.size();
    t.resize(o + sizeof(v));
    std::memcpy(t.data() + o, &v, sizeof(v));
  };
  if (ints && sym) {
    for (uint32_t i = 0; i < L; ++i)  // rows of the lower triangle with the diagonal: (i, j <= i) at i (i + 1) / 2 + j
      for (uint32_t j = 0; j <= i; ++j) put((uint16_t)d[(size_t)i * L + j]);
    aux_kind_ = 1;
  } else if (ints && 2ull * L * L <= lds) {
    for (size_t i = 0; i < (size_t)L * L; ++i) put((uint16_t)d[i]);
    aux_kind_ = 2;
  } else if (sym && !ints && 4 * tri <= lds) {
    for (uint32_t i = 0; i < L; ++i)
      for (uint32_t j = 0; j <= i; ++j) put(d[(size_t)i * L + j]);
    aux_kind_ = 3;
  }
  if (aux_kind_) {
    t.resize((t.size() + 15) / 16 * 16, 0);  // whole 16-byte stores
    reserve(obj_aux_, t.size());
    copy_to_device(obj_aux_.ptr, t.data(), t.size());
    aux_bytes_ = (uint32_t)t.size();
  }
}

void Island::prepare_qubo() {
  if (cfg_.objective != OBJ_QUBO) return;
  if (cfg_.encoding != ENC_BINARY) throw std::invalid_argument("the QUBO objective needs the BINARY encoding");
  if (obj_len_[0] < (size_t)cfg_.L * cfg_.L) throw std::invalid_argument("QUBO: objective data must hold the L x L matrix Q");
  if (!on_gpu() || qubo_version_ == obj_version_) return;
  const uint32_t lp = qubo_padded_length(cfg_.L);
  if (lp > kQuboMaxBits) throw std::invalid_argument("QUBO objective supports genomes of at most 1024 bits");
  reserve(qubo_qt_, (size_t)lp * lp);
  reserve(qubo_qn_, (size_t)lp * lp);
  qubo_pack_launch(obj_data_[0].as<const float>(), cfg_.L, qubo_qt_.as<int8_t>(), stream, qubo_qn_.as<int8_t>());
  qubo_version_ = obj_version_;
}

RngKey Island::key() const {
  return RngKey{(uint32_t)cfg_.seed, (uint32_t)(cfg_.seed >> 32) ^ (epoch_ * 0x9E3779B9u), gen_, cfg_.island};
}

LsArgs Island::ls_args(int kind, uint32_t moves, float prob) const {
  if (!(prob == prob)) throw std::invalid_argument("local search probability is NaN");
  LsArgs a;
  std::memset(&a, 0, sizeof(a));
  a.rows = rows_[cur_].ptr;
  a.scores = scores_at(cur_);
  a.S = cfg_.S;
  a.L = cfg_.L;
  a.row_words = row_words_;
  a.chunks = chunks_;
  a.key = key();
  a.objective = cfg_.objective;
  a.obj_data = obj_data_[0].as<const float>();
  a.kind = kind;
  a.moves = moves;
  a.always = prob >= 1.f ? 1u : 0u;
  a.thresh = prob_thresh(prob);
  return a;
}

bool Island::matrix_symmetric() {
  if (sym_version_ != obj_version_) {
    sym_version_ = obj_version_;
    const uint32_t L = cfg_.L;
    const float* d = obj_host0_.data();
    bool sym = obj_host0_.size() >= (size_t)L * L;
    for (uint32_t i = 0; sym && i < L; ++i)
      for (uint32_t j = 0; sym && j < i; ++j)
        sym = std::memcmp(&d[(size_t)i * L + j], &d[(size_t)j * L + i], sizeof(float)) == 0;
    sym_ok_ = sym;
  }
  return sym_ok_;
}

void Island::local_search(uint32_t moves, float prob) {
  // the configured kind; without one, the stage of the population: one-flip
  // for BINARY with the QUBO objective, 2-opt otherwise
  int kind = cfg_.local_search;
  if (kind == LS_NONE) kind = (cfg_.encoding == ENC_BINARY && cfg_.objective == OBJ_QUBO) ? LS_ONE_FLIP : LS_TWO_OPT;
  local_search(moves, prob, kind);
}

void Island::local_search(uint32_t moves, float prob, int kind) {
  TraceRange tr("pga.local_search");
  if (kind != LS_TWO_OPT && kind != LS_ONE_FLIP && kind != LS_OR_OPT) throw std::invalid_argument("unknown local search");
  if (kind == LS_ONE_FLIP) {
    if (cfg_.encoding != ENC_BINARY || cfg_.objective != OBJ_QUBO)
      throw std::invalid_argument("one-flip local search needs the BINARY encoding with the built-in QUBO objective");
    one_flip_search(moves, prob);
    return;
  }
  const bool oro = kind == LS_OR_OPT;
  const std::string name = oro ? "Or-opt" : "2-opt";
  if (cfg_.encoding != ENC_PERMUTATION)
    throw std::invalid_argument(name + " local search needs the PERMUTATION encoding (one-flip: BINARY with the QUBO objective)");
  if (jit_) throw std::invalid_argument(oro ? kJitNotOrOpt : kJitNotTwoOpt);
  const bool euc = cfg_.objective == OBJ_TSP_EUC;
  if (!euc && cfg_.objective != OBJ_TSP && cfg_.objective != OBJ_TSP_OPEN)
    throw std::invalid_argument(name + " local search needs a built-in TSP objective");
  if (obj_len_[0] < (euc ? 2ull * cfg_.L : (size_t)cfg_.L * cfg_.L))
    throw std::invalid_argument(name + " local search: the objective data is not set");
  // Or-opt turns no edge outside its own segment round: any matrix will do
  if (!oro && !euc && !matrix_symmetric())
    throw std::invalid_argument("2-opt local search needs a symmetric distance matrix");
  LsArgs a = ls_args(kind, moves, prob);
  prepare_objective();
  if (!euc && aux_kind_ && aux_on_) {
    a.obj_aux = obj_aux_.ptr;
    a.obj_aux_kind = aux_kind_;
    a.obj_aux_bytes = aux_bytes_;
  }
  if (on_gpu()) perm_ls_launch(a, stream);
  else cpu::perm_local_search(a);
  // rows and scores changed in place: the partials, the fused statistics and
  // every key derived from the scores follow, as after evaluate()
  rebest();
}

void Island::one_flip_search(uint32_t moves, float prob) {
  if (jit_) throw std::invalid_argument(kJitNotOneFlip);
  if (one_flip_sign(cfg_.obj_f0) == 0)
    throw std::invalid_argument("one-flip local search: the QUBO score factor (obj_f0) must be non-zero");
  LsArgs a = ls_args(LS_ONE_FLIP, moves, prob);
  prepare_objective();  // (throws when the matrix is not set) both packed matrices on the GPU
  a.qubo_qt = qubo_qt_.as<const int8_t>();
  a.qubo_qn = qubo_qn_.as<const int8_t>();
  a.obj_f0 = cfg_.obj_f0;
  if (on_gpu()) qubo_ls_launch(a, stream);
  else cpu::qubo_local_search(a);
  rebest();  // as after the 2-opt stage
}

GenArgs Island::make_args(int mode) {
  prepare_objective();
  GenArgs a;
  std::memset(&a, 0, sizeof(a));
  a.qubo_qt = qubo_qt_.as<const int8_t>();
  if (aux_kind_ && aux_on_ && (cfg_.objective == OBJ_TSP || cfg_.objective == OBJ_TSP_OPEN)) {
    a.obj_aux = obj_aux_.ptr;
    a.obj_aux_kind = aux_kind_;
    a.obj_aux_bytes = aux_bytes_;
  }
  if (cfg_.objective == OBJ_KNAPSACK && knap_cols_ > 0) {
    a.knap_tab = knap_tab_.ptr;
    a.knap_dig = knap_dig_;
    a.knap_cols = knap_cols_;
  }
  // INIT and EVAL write the current parity in place, every other mode the next one
  const int nx = cur_ ^ 1, out = (mode == MODE_INIT || mode == MODE_EVAL) ? cur_ : nx;
  a.cur = rows_[mode == MODE_MUTATE ? nx : cur_].ptr;
  a.next = rows_[out].ptr;
  a.score_cur = scores_at(cur_);
  a.score_next = scores_at(out);
  a.S = cfg_.S;
  a.L = cfg_.L;
  a.row_words = row_words_;
  a.chunks = chunks_;
  a.encoding = (uint32_t)cfg_.encoding;
  a.key = key();
  a.selection = cfg_.selection;
  a.tour_k = cfg_.tour_k;
  a.cumfit = cumfit_.as<const float>();
  a.roul_guide = roul_guide_.as<const uint32_t>();
  a.roul_scale = cum_ws_.ptr ? cum_ws_.as<const float>() + kRoulScale : nullptr;
  a.rank_order = rank_order_.as<const uint32_t>();
  a.rank_thresh = rank_thresh_of(cfg_.rank_pressure);
  a.crossover = cfg_.crossover;
  a.xo_always = cfg_.xo_prob >= 1.f ? 1u : 0u;
  a.xo_thresh_hi = prob_thresh(cfg_.xo_prob);
  a.blend_alpha = cfg_.blend_alpha;
  a.mutation = cfg_.mutation;
  a.mut_rate = mut_rate_eff_;
  a.mut_ind_thresh = per_individual_mutation(cfg_.mutation) ? prob_thresh(mut_rate_eff_) : 0u;
  a.mut_thr = mut_thr_.as<const uint32_t>();
  a.mut_inv_log2_1mp = mut_inv_;
  a.mut_sparse = mut_sparse_ ? 1u : 0u;
  a.sigma = cfg_.sigma;
  a.lo = cfg_.lo;
  a.hi = cfg_.hi;
  a.objective = cfg_.objective;
  a.obj_i = cfg_.obj_i;
  a.obj_f0 = cfg_.obj_f0;
  a.obj_f1 = cfg_.obj_f1;
  a.obj_data = obj_data_[0].as<const float>();
  a.obj_data2 = obj_data_[1].as<const float>();
  a.user_fn = user_fn_;
  a.user_xo_fn = user_xo_fn_;
  a.user_mut_fn = user_mut_fn_;
  a.compat_rand = compat_rand_.as<float>();
  a.n_elite = cfg_.n_elite;
  a.elite_idx = cfg_.n_elite > 1 ? elite_idx_.as<const uint32_t>() : nullptr;
  a.best_cur = best_at(cur_);
  a.n_best_cur = d_[cur_].n_best;
  a.last_mask = last_mask_;
  if (capturing_) {
    a.gen_dev = gen_dev_.as<const uint32_t>();
    a.gen_off = gen_ - capture_base_;
  }
  if (fused_stats()) a.stats_parts = stats_at(out);
  if (integer_objective(cfg_.objective, cfg_.L)) {
    a.key_cur = keys_at(cur_);
    a.key_next = keys_at(out);
  } else if (mode == MODE_GEN && real_qk() && d_[cur_].qk && qk_ws_.ptr) {
    a.key_cur = keys_at(cur_);
    a.key_next = keys_at(nx);
    a.qk = qk_ws_.as<const float>();
  }
  return a;
}

LaunchReport Island::launch(int mode, const GenArgs& a, unsigned long long* parts) {
  if (mode != MODE_GEN && a.cur == rows_[cur_].ptr) drop_key_counts();  // staged / init / eval
  if (on_gpu()) return encoding_launch(mode, a, parts, stream);
  LaunchReport r;
  r.grid = cpu::encoding_run(mode, a, parts);
  return r;
}

void Island::initialize() {
  TraceRange tr("pga.initialize");
  evaluate_current(MODE_INIT);
  if (cfg_.objective == OBJ_NONE && !jit_) rebest();
}

void Island::evaluate() {
  TraceRange tr("pga.evaluate");
  evaluate_current(MODE_EVAL);
}

void Island::evaluate_current(int mode) {
  Derived made;
  if (mode == MODE_INIT || !jit_) {
    GenArgs a = make_args(mode);
    made.n_best = launch(mode, a, best_at(cur_)).grid;
    made.stats = a.stats_parts != nullptr;
  }
  if (jit_) made = Derived{jit_eval(rows_[cur_].ptr, scores_at(cur_), cfg_.S, best_at(cur_))};
  scores_written(cur_, made);
}

void Island::rebest() {
  Derived made;
  if (on_gpu()) {
    made.n_best = best_of_scores_launch(scores_at(cur_), cfg_.S, best_at(cur_), stream, int_keys_at(cur_));
  } else {
    best_at(cur_)[0] = cpu::best_of_scores(scores_at(cur_), cfg_.S);
    made.n_best = 1;
  }
  scores_written(cur_, made);
}

bool Island::real_qk() const {
  // quantized tournament keys feed only the two-phase kernel (real_gen_tp),
  // which small populations do not take: there they would cost a launch
  return on_gpu() && cfg_.encoding == ENC_REAL && cfg_.objective != OBJ_NONE && cfg_.objective != OBJ_USER_FNPTR &&
         !jit_ &&
         cfg_.S * batch_n_ >= real_tp_min_population();
}

void Island::prepare_generation() {
  const float* sc = scores_at(cur_);
  const Derived& now = d_[cur_];
  if (real_qk()) {
    // the current generation's score range (fused partials when its kernel
    // stored them), and its quantized keys if anything rewrote the scores
    if (reserve(qk_ws_, 4ull * (4 + 3 * 1024))) qk_age_ = 0;
    // The quantization range only has to be the same for every key of a
    // generation: keys are monotonic in the score and equal keys fall back to
    // the exact f32 compare, so any range gives the same tournaments.  It is
    // refreshed every few generations (a stale range only costs more
    // ties), not every generation: small populations are launch-bound.
    // Every 8 generations (32 below 2^18 children, where the ~5 us refresh
    // launch is a larger share of a short generation: reference E1).
    const uint32_t refresh = cfg_.S * batch_n_ < (1ull << 18) ? 32u : 8u;
    if (qk_age_++ % refresh == 0) {
      if (now.stats) stats_from_parts_launch(stats_at(cur_), best_at(cur_), now.n_best, cfg_.S, qk_ws_.as<float>(), stream);
      else score_stats_launch(sc, cfg_.S, qk_ws_.as<float>(), stream);
    }
    if (!now.qk) {
      scores_to_qkeys_launch(sc, cfg_.S, qk_ws_.as<const float>(), keys_at(cur_), stream);
      keys_requantized();
    }
  }
  if (cfg_.selection == SEL_ROULETTE) {
    const bool fused = on_gpu() && now.stats && stats_at(cur_);  // min from the GEN kernel's partials
    // integer objectives after a two-phase GEN launch: one exact launch
    // (the partials give every block its carry)
    const bool one = fused && now.part.grid && integer_objective(cfg_.objective, cfg_.L) &&
                     cfg_.objective != OBJ_KNAPSACK && !roul_fused_off() &&
                     roulette_fused_launch(sc, cfg_.S, stats_at(cur_), now.part, cfg_.L, cumfit_.as<float>(),
                                           roul_guide_.as<uint32_t>(), cum_ws_.as<float>(), stream);
    if (one) {
    } else if (on_gpu()) {
      roulette_prefix_launch(sc, cfg_.S, fused ? stats_at(cur_) : nullptr, now.n_best, cumfit_.as<float>(),
                             cum_ws_.as<float>(), stream, integer_objective(cfg_.objective, cfg_.L));
      roulette_guide_launch(cumfit_.as<const float>(), cfg_.S, roul_guide_.as<uint32_t>(), cum_ws_.as<float>(), stream);
    } else {
      cpu::roulette_prefix(sc, cfg_.S, cumfit_.as<float>());
    }
  }
  if (cfg_.selection == SEL_RANK) {
    uint32_t* order = rank_order_.as<uint32_t>();
    if (on_gpu() && int_keys_at(cur_)) {
      // with the tile counts of these keys, when the GEN kernel that wrote them stored them
      rank_order16_launch(keys_at(cur_), cfg_.S, cfg_.L + 1, order, rank_ws_.ptr, stream, take_rank_counts());
    }
    else if (on_gpu()) rank_order_launch(sc, cfg_.S, order, rank_ws_.ptr, stream);
    else cpu::rank_order(sc, cfg_.S, order);
  }
  if (cfg_.n_elite > 1) topk(cfg_.n_elite, true, elite_idx_.as<uint32_t>(), /*sorted=*/false);
}

void Island::run(uint32_t n) {
  TraceRange tr("pga.run");
  if (cfg_.local_search != LS_NONE) {  // a stage follows every generation: plain launches only
    if (jit_)
      throw std::invalid_argument(cfg_.local_search == LS_ONE_FLIP ? kJitNotOneFlip
                                  : cfg_.local_search == LS_OR_OPT ? kJitNotOrOpt
                                                                   : kJitNotTwoOpt);
    run_plain(n);
    return;
  }
  if (run_tiny(n)) return;
  if (on_gpu() && graph_g_ > 0 && !graph_broken_ && !hist_on_ && n >= graph_g_ + 2) {
    const bool fresh = gexec_ && g_cur_ == cur_ && g_epoch_ == epoch_ && g_version_ == version_ &&
                       g_nbest_ == d_[cur_].n_best && g_len_ == graph_g_;
    if (!fresh) {
      // two plain generations first: the best-partials count of this parity
      // then equals the GEN kernel's grid, which is what every replay leaves
      run_plain(2);
      n -= 2;
    }
    const uint32_t reps = n / graph_g_;
    drop_key_counts();  // replays produce no fused histogram (nor rank counts; their sorts overwrite the workspace)
    if (run_graph(reps, fresh)) n -= reps * graph_g_;
  }
  run_plain(n);
}

bool Island::run_tiny(uint32_t n) {
  // REAL populations that fit one block: all n generations in one launch
  // (real_launch_multi); nothing to prepare between generations, so the
  // launch is exactly n run_plain generations
  if (!on_gpu() || n < 2 || cfg_.encoding != ENC_REAL || jit_ || hist_on_ || capturing_ || real_qk()) return false;
  if (cfg_.n_elite > 1 || (cfg_.selection != SEL_TOURNAMENT && cfg_.selection != SEL_RANDOM)) return false;
  GenArgs a = make_args(MODE_GEN);
  const int nx = cur_ ^ 1;
  unsigned long long* const parts[2] = {best_at(nx), best_at(cur_)};
  float* const st[2] = {a.stats_parts, a.stats_parts ? stats_at(cur_) : nullptr};
  if (!real_launch_multi(a, parts, st, n, stream)) return false;
  TraceRange tg("pga.generations_tiny", 2);
  // the kernel keeps the population in LDS between generations: only the
  // last generation's buffers (the new current parity) are written
  for (uint32_t i = 0; i < n; ++i) swap();
  // the previous parity's rows / scores / partials were never written (its
  // generations lived in LDS): no valid partials there until a kernel writes them
  Derived made{1};
  made.stats = a.stats_parts != nullptr;
  scores_written(cur_, made);
  scores_written(cur_ ^ 1, Derived{});
  return true;
}

void Island::run_plain(uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    TraceRange tg("pga.generation", 2);
    prepare_generation();
    GenArgs a = make_args(MODE_GEN);
    if (!jit_ || !fused_jit_generation(a)) {  // (else: the objective linked into the generation kernel)
      const int nx = cur_ ^ 1, w = (int)(fhist_rot_ % 3);
      const bool fh = fhist_ready_for(a);
      if (fh) {  // this generation may also write the value histogram of its keys (GenArgs::key_hist)
        a.key_hist = fhist_[w].as<uint32_t>();
        a.hist_zero = fhist_[(w + 1) % 3].as<uint32_t>();
        a.hist_bins = cfg_.L + 1;
        a.hist_zero_words = fused_hist_words(cfg_.L + 1);
      }
      a.rank_counts = rank_counts_for_gen();
      if (a.rank_counts) a.hist_bins = cfg_.L + 1;
      const LaunchReport rep = launch(MODE_GEN, a, best_at(nx));
      tp_tail_ = rep.part.tail;
      route_ = rep.route;
      Derived made{rep.grid};
      made.stats = a.stats_parts != nullptr;
      // (the roulette prefix's carries, roulette_fused_launch)
      if (made.stats && rep.part.grid == rep.grid) made.part = rep.part;
      made.qk = a.qk != nullptr;  // every REAL GEN kernel writes the keys it is given
      // the histogram and the rank counts only when the launcher reports that its
      // kernel took them (binary_gs.hip go_tp), not on the conditions predicted above
      if (fh && rep.hist) made.fhist = w;
      made.rank_cnt = a.rank_counts && rep.rank_counts;
      if (jit_) made = Derived{jit_eval(rows_[nx].ptr, scores_at(nx), cfg_.S, best_at(nx))};
      scores_written(nx, made);
    }
    swap();
    if (cfg_.local_search != LS_NONE) local_search(cfg_.ls_moves, cfg_.ls_prob);
    if (hist_on_ && !hist_manual_ && !capturing_) append_history();
  }
}

bool Island::run_batched(const std::vector<Island*>& isls, uint32_t n, hipStream_t s) {
  const size_t N = isls.size();
  if (N < 2 || !isls[0]) return false;
  const Island* i0 = isls[0];
  const bool bin = i0->cfg_.encoding == ENC_BINARY, real = i0->cfg_.encoding == ENC_REAL;
  const bool perm = i0->cfg_.encoding == ENC_PERMUTATION;
  if ((!bin && !real && !perm) || N > (bin ? binary_max_batch() : real ? real_max_batch() : perm_max_batch()))
    return false;
  for (const Island* i : isls) {
    if (!i || !i->on_gpu() || i->device_ != i0->device_ || i->cfg_.encoding != i0->cfg_.encoding || i->jit_ ||
        i->user_fn_ || i->user_xo_fn_ || i->user_mut_fn_ || i->hist_on_ || i->cfg_.local_search != LS_NONE || i->cfg_.S != i0->cfg_.S || i->cfg_.L != i0->cfg_.L)
      return false;
    for (const Island* j : isls)
      if (j != i && j->rows_[0].ptr == i->rows_[0].ptr) return false;  // the same island twice
  }
  {  // the batched kernels' conditions from the configuration alone, before
     // any launch (an island that cannot qualify pays no extra prepare pass)
    const Config& c = i0->cfg_;
    const bool sel_ok = (c.selection == SEL_TOURNAMENT && c.tour_k == 2) || c.selection == SEL_RANDOM ||
                        c.selection == SEL_RANK || c.selection == SEL_ROULETTE;
    const bool o32 = (c.S + kRowPad) * (uint64_t)i0->row_words_ * 4u <= 0xFFFFFFFFull;
    if (perm) {  // perm_gen_fast: every selection; the TSP objectives, one chunk per lane
      if (c.objective != OBJ_TSP && c.objective != OBJ_TSP_OPEN && c.objective != OBJ_TSP_EUC) return false;
      if (i0->chunks_ > 64 || force_generic_kernels()) return false;
      for (const Island* i : isls)
        if (i->cfg_.objective != c.objective) return false;
    } else if (!sel_ok || !o32 || i0->chunks_ > 64 || c.n_elite > 64 || force_generic_kernels()) {
      return false;
    } else if (bin) {
      if (c.objective != OBJ_ONEMAX && c.objective != OBJ_LEADING_ONES && c.objective != OBJ_TRAP) return false;
      for (const Island* i : isls)
        if (!integer_objective(i->cfg_.objective, i->cfg_.L) || !i->keys_[0].ptr || i->cfg_.objective != c.objective)
          return false;
    } else {
      const bool obj_ok = c.objective == OBJ_SPHERE || c.objective == OBJ_RASTRIGIN || c.objective == OBJ_ROSENBROCK ||
                          c.objective == OBJ_ACKLEY || c.objective == OBJ_GRIEWANK || c.objective == OBJ_SCHWEFEL ||
                          c.objective == OBJ_LINEAR || c.objective == OBJ_KNAPSACK_REAL;
      if (!obj_ok || (c.obj_i & 2) || c.S * N < real_tp_min_population()) return false;
      for (const Island* i : isls)
        if (i->cfg_.objective != c.objective || i->cfg_.obj_i != c.obj_i) return false;
    }
  }
  TraceRange tr("pga.run_batched");
  // REAL: the batch takes the two-phase kernel, which tournaments on the
  // quantized keys, so every island keeps them for the batch's population
  for (Island* I : isls) I->batch_n_ = (uint32_t)N;
  struct Reset {
    const std::vector<Island*>& v;
    ~Reset() {
      for (Island* I : v) I->batch_n_ = 1;
    }
  } reset{isls};
  std::vector<GenArgs> args(N);
  std::vector<unsigned long long*> parts(N);
  for (uint32_t g = 0; g < n; ++g) {
    for (size_t k = 0; k < N; ++k) {
      Island& I = *isls[k];
      I.stream = s;
      I.prepare_generation();
      args[k] = I.make_args(MODE_GEN);
      parts[k] = I.best_at(I.cur_ ^ 1);
    }
    LaunchReport rep;  // (REAL and PERMUTATION report their grid alone)
    if (bin) rep = binary_launch_batch(args.data(), parts.data(), (uint32_t)N, s);
    else rep.grid = real ? real_launch_batch(args.data(), parts.data(), (uint32_t)N, s)
                         : perm_launch_batch(args.data(), parts.data(), (uint32_t)N, s, &rep.route);
    if (rep.grid == 0) {
      if (g == 0) return false;  // not eligible (decided on the first generation's arguments)
      throw std::logic_error("batched islands stopped qualifying mid-run");
    }
    for (size_t k = 0; k < N; ++k) {
      Island& I = *isls[k];
      // no fused histogram, rank counts or roulette partition from the batched launch
      Derived made{rep.grid};
      made.stats = args[k].stats_parts != nullptr;
      made.qk = real && args[k].qk != nullptr;  // the REAL kernel writes the keys it is given
      I.scores_written(I.cur_ ^ 1, made);
      I.tp_tail_ = rep.part.tail;
      I.route_ = rep.route;
      I.swap();
    }
  }
  return true;
}

uint32_t Island::run_until(uint32_t n, float target, uint32_t check_every) {
  TraceRange tr("pga.run_until");
  if (check_every == 0) check_every = 10;
  uint32_t done = 0;
  while (done < n) {
    const uint32_t k = std::min(check_every, n - done);
    run(k);
    done += k;
    if (best_score() >= target) break;  // one sync per check
  }
  return done;
}

bool Island::fused_stats() const {
  // JIT objectives and the QUBO evaluation pass store best partials only
  return on_gpu() && !jit_ && cfg_.objective != OBJ_QUBO && cfg_.objective != OBJ_NONE;
}

void Island::set_stats_history(bool on) {
  hist_on_ = on;
  if (!on) return;  // off keeps the rows so far
  hist_n_ = 0;
  hist_host_.clear();
}

void Island::append_history() {
  if (!on_gpu()) {
    float r[4];
    cpu::score_stats(scores_at(cur_), cfg_.S, r);
    hist_host_.insert(hist_host_.end(), r, r + 4);
    ++hist_n_;
    return;
  }
  if (hist_.bytes < 16ull * (hist_n_ + 1)) {  // grow (rare): keep the rows so far
    const uint64_t cap = std::max<uint64_t>(1024, 2 * (hist_n_ + 1));
    Buffer nb(16ull * cap, true);
    if (hist_n_) PGA_HIP_CHECK(hipMemcpyAsync(nb.ptr, hist_.ptr, 16ull * hist_n_, hipMemcpyDeviceToDevice, stream));
    synchronize();
    hist_ = std::move(nb);  // (nb frees the old rows)
  }
  float* row = hist_.as<float>() + 4 * hist_n_;
  if (d_[cur_].stats) {
    stats_from_parts_launch(stats_at(cur_), best_at(cur_), d_[cur_].n_best, cfg_.S, row, stream);
  } else {
    score_stats_launch(scores_at(cur_), cfg_.S, stats_.as<float>(), stream);
    PGA_HIP_CHECK(hipMemcpyAsync(row, stats_.ptr, 16, hipMemcpyDeviceToDevice, stream));
  }
  ++hist_n_;
}

std::vector<float> Island::history() {
  if (!on_gpu()) return hist_host_;
  std::vector<float> out(4 * hist_n_);
  if (hist_n_) copy_to_host(out.data(), hist_.ptr, 16ull * hist_n_);
  return out;
}

void Island::crossover_stage() {
  TraceRange tr("pga.crossover");
  prepare_generation();
  GenArgs a = make_args(MODE_CROSS);
  launch(MODE_CROSS, a, nullptr);
}

void Island::mutate_stage() {
  TraceRange tr("pga.mutate");
  GenArgs a = make_args(MODE_MUTATE);
  launch(MODE_MUTATE, a, nullptr);
}

void Island::swap() {
  cur_ ^= 1;
  ++gen_;
}

unsigned long long Island::best_packed() {
  unsigned long long r = 0;
  if (on_gpu()) {
    reduce_best_launch(best_at(cur_), d_[cur_].n_best, out_best_.as<unsigned long long>(), stream);
    copy_to_host(&r, out_best_.ptr, 8);
  } else {
    r = cpu::reduce_best(best_at(cur_), d_[cur_].n_best);
  }
  return r;
}

void Island::stats(float out[4]) {
  const float* sc = scores_at(cur_);
  if (on_gpu() && d_[cur_].stats) {  // fused partials of the kernel that scored this generation
    stats_from_parts_launch(stats_at(cur_), best_at(cur_), d_[cur_].n_best, cfg_.S, stats_.as<float>(), stream);
    copy_to_host(out, stats_.ptr, 16);
  } else if (on_gpu()) {
    score_stats_launch(sc, cfg_.S, stats_.as<float>(), stream);
    copy_to_host(out, stats_.ptr, 16);
  } else {
    cpu::score_stats(sc, cfg_.S, out);
  }
}

void Island::ensure_topk_ws(uint32_t k) {
  const size_t need = topk_workspace_bytes(cfg_.S, k);
  if (reserve(topk_ws_, need, /*sync=*/true))
    PGA_HIP_CHECK(hipMemsetAsync(topk_ws_.ptr, 0, need, stream));  // the value histogram must start zeroed
}

void Island::topk(uint32_t k, bool largest, uint32_t* idx_out, bool sorted) {
  TraceRange tr(largest ? "pga.topk" : "pga.bottomk");
  if (k > cfg_.S) throw std::invalid_argument("k exceeds population size");
  const float* sc = scores_at(cur_);
  if (on_gpu()) {
    ensure_topk_ws(k);
    const uint16_t* k16 = int_keys_at(cur_);
    TopkFused f;
    topk_launch(sc, k16, cfg_.L + 1, cfg_.S, k, largest, sorted, idx_out, topk_ws_.ptr, stream, nullptr,
                sorted || !k16 ? nullptr : fused_select(f));
  } else {
    cpu::topk(sc, cfg_.S, k, largest, idx_out, sorted);
  }
}

std::vector<uint32_t> Island::topk_host(uint32_t k, bool largest) {
  std::vector<uint32_t> out(k);
  if (k == 0) return out;
  if (on_gpu()) {
    uint32_t* d = (uint32_t*)scratch(4ull * k);
    topk(k, largest, d);
    copy_to_host(out.data(), d, 4ull * k);
  } else {
    topk(k, largest, out.data());
  }
  return out;
}

std::vector<uint32_t> Island::row_host(uint64_t i) {
  if (i >= cfg_.S) throw std::out_of_range("individual index out of range");
  std::vector<uint32_t> out(row_words_);
  copy_to_host(out.data(), (const uint32_t*)rows_[cur_].ptr + i * row_words_, 4ull * row_words_);
  return out;
}

bool Island::qkeys_host(int which, std::vector<uint16_t>& keys, float range[2]) {
  const int p = (which & 1) ^ cur_;
  if (!real_qk() || !d_[p].qk || !qk_ws_.ptr || !keys_[p].ptr) return false;
  keys.resize(cfg_.S);
  copy_to_host(keys.data(), keys_[p].ptr, 2ull * cfg_.S);
  copy_to_host(range, qk_ws_.ptr, 8);
  return true;
}

void Island::gather(const uint32_t* idx, uint32_t n, void* out_rows, float* out_scores) {
  TraceRange tr("pga.migrate.gather");
  if (on_gpu())
    gather_rows_launch(rows_[cur_].ptr, scores_at(cur_), row_words_, idx, n, out_rows, out_scores, stream);
  else
    cpu::gather_rows(rows_[cur_].ptr, scores_at(cur_), row_words_, idx, n, out_rows, out_scores);
}

void Island::scatter(const uint32_t* idx, uint32_t n, const void* in_rows, const float* in_scores) {
  TraceRange tr("pga.migrate.scatter");
  if (on_gpu())
    scatter_rows_launch(rows_[cur_].ptr, scores_at(cur_), row_words_, idx, n, in_rows, in_scores, stream);
  else
    cpu::scatter_rows(rows_[cur_].ptr, scores_at(cur_), row_words_, idx, n, in_rows, in_scores);
  rebest();  // best partials and tournament keys follow the new scores
}

void Island::set_migration_policy(int p) {
  if (p != MIG_TOPK && p != MIG_STRIPE) throw std::invalid_argument("migration policy must be MIG_TOPK or MIG_STRIPE");
  mig_policy_ = p;
}

void Island::emigrate(uint32_t k, void* out_rows, float* out_scores) {
  TraceRange tr("pga.migrate.emigrate");
  if (k == 0) return;
  if (k > cfg_.S) throw std::invalid_argument("k exceeds population size");
  if (mig_policy_ == MIG_STRIPE) {
    if (on_gpu())
      stripe_emigrate_launch(scores_at(cur_), rows_[cur_].ptr, row_words_, cfg_.S, k, out_rows, out_scores, stream);
    else
      cpu::stripe_emigrate(scores_at(cur_), rows_[cur_].ptr, row_words_, cfg_.S, k, out_rows, out_scores);
    return;
  }
  const uint16_t* k16 = int_keys_at(cur_);
  if (on_gpu() && topk_move_supported(k16, cfg_.L + 1, cfg_.S)) {
    ensure_topk_ws(k);
    TopkMove mv;
    mv.mode = TopkMove::GATHER;
    mv.rw16 = row_words_ / 4;
    mv.src_rows = rows_[cur_].as<const uint4>();
    mv.src_scores = scores_at(cur_);
    mv.dst_rows = (uint4*)out_rows;
    mv.dst_scores = out_scores;
    TopkFused f;
    topk_launch(scores_at(cur_), k16, cfg_.L + 1, cfg_.S, k, true, false, nullptr, topk_ws_.ptr, stream, &mv,
                fused_select(f));
    return;
  }
  uint32_t* idx = (uint32_t*)scratch(4ull * k);
  topk(k, true, idx, false);
  gather(idx, k, out_rows, out_scores);
}

void Island::immigrate(uint32_t k, const void* in_rows, const float* in_scores) {
  TraceRange tr("pga.migrate.immigrate");
  if (k == 0) return;
  if (k > cfg_.S) throw std::invalid_argument("k exceeds population size");
  uint16_t* k16 = int_keys_at(cur_);
  if (mig_policy_ == MIG_STRIPE) {
    if (on_gpu()) {
      // victims, their keys, and the island's best partials + statistics in one pass
      float* sp = fused_stats() ? stats_at(cur_) : nullptr;
      Derived made{stripe_immigrate_launch(scores_at(cur_), k16, rows_[cur_].ptr, row_words_, cfg_.S, k, in_rows,
                                           in_scores, best_at(cur_), sp, stream)};
      made.stats = sp != nullptr;
      scores_written(cur_, made);
    } else {
      cpu::stripe_immigrate(scores_at(cur_), rows_[cur_].ptr, row_words_, cfg_.S, k, in_rows, in_scores);
      rebest();
    }
    return;
  }
  if (on_gpu() && topk_move_supported(k16, cfg_.L + 1, cfg_.S)) {
    ensure_topk_ws(k);
    TopkMove mv;
    mv.mode = TopkMove::SCATTER;
    mv.rw16 = row_words_ / 4;
    mv.src_rows = (const uint4*)in_rows;
    mv.src_scores = in_scores;
    mv.dst_rows = rows_[cur_].as<uint4>();
    mv.dst_scores = scores_at(cur_);
    mv.dst_keys = k16;
    mv.best_parts = best_at(cur_);  // the new per-block bests, from the selection itself
    TopkFused f;  // the victims' selection reads the histogram of the keys as they are before it
    const uint32_t nb = topk_launch(scores_at(cur_), k16, cfg_.L + 1, cfg_.S, k, false, false, nullptr, topk_ws_.ptr,
                                    stream, &mv, fused_select(f));
    // the victims' keys were written with their rows; the best partials came
    // with the selection (else one pass over the scores)
    scores_written(cur_, Derived{nb ? nb : best_of_scores_launch(scores_at(cur_), cfg_.S, best_at(cur_), stream, nullptr)});
    return;
  }
  uint32_t* idx = (uint32_t*)scratch(4ull * k);
  topk(k, false, idx, false);
  scatter(idx, k, in_rows, in_scores);
}

void Island::set_fused_histogram(bool on) {
  fhist_user_ = on;
  fhist_on_ = on || cfg_.n_elite > 1;
}

uint32_t* Island::rank_counts_for_gen() const {
  // the launcher (binary_gs.hip go_tp) takes them only at the sort's tile geometry
  if (cfg_.selection != SEL_RANK || !on_gpu() || capturing_ || jit_ || cfg_.encoding != ENC_BINARY) return nullptr;
  if (!integer_objective(cfg_.objective, cfg_.L) || cfg_.objective == OBJ_KNAPSACK || !keys_[0].ptr) return nullptr;
  if (cfg_.L + 1 > kHistMaxBins || !rank_ws_.ptr) return nullptr;
  static const bool off = env_off("PGA_RANK_FUSED");  // the sort counts its keys itself
  if (off) return nullptr;
  return rank_order16_counts(rank_ws_.ptr, cfg_.S, cfg_.L + 1);
}

bool Island::fhist_ready_for(const GenArgs& a) {
  // the conditions under which binary_gen_tp runs with u16 keys (binary_gs.hip
  // launch_mode), so the launch really produces the histogram
  if (!fhist_on_ || !on_gpu() || capturing_ || jit_ || cfg_.encoding != ENC_BINARY) return false;
  if (!integer_objective(cfg_.objective, cfg_.L) || cfg_.L + 1 > kHistMaxBins || a.key_cur == nullptr) return false;
  if (cfg_.objective == OBJ_KNAPSACK) return false;
  uint32_t gs = 0;
  bool full = false, dense = false;
  if (!binary_tp_plan(a, gs, full, dense)) return false;
  for (Buffer& b : fhist_)  // allocated zeroed on first use
    if (reserve(b, 4ull * fused_hist_words(cfg_.L + 1))) PGA_HIP_CHECK(hipMemsetAsync(b.ptr, 0, b.bytes, stream));
  return true;
}

const TopkFused* Island::fused_select(TopkFused& f) {
  const int b = on_gpu() ? d_[cur_].fhist : -1;
  if (b < 0) return nullptr;
  f.hist = fhist_[b].as<const uint32_t>();
  f.status = fhist_[b].as<uint32_t>() + (cfg_.L + 1 + 3) / 4 * 4;
  if (!fhist_clean_[b])  // a selection on this population already used its status words
    PGA_HIP_CHECK(hipMemsetAsync(f.status, 0, 4ull * kTopkStatusWords, stream));
  fhist_clean_[b] = false;
  return &f;
}

bool Island::evaluate_rows(void* rows, float* scores, uint32_t n) {
  if (cfg_.objective == OBJ_NONE && !jit_) return false;
  if (n == 0) return true;
  TraceRange tr("pga.migrate.evaluate");
  reserve(ev_parts_, 8ull * kMaxGrid);
  if (jit_) {
    jit_eval(rows, scores, n, ev_parts_.as<unsigned long long>());
    return true;
  }
  GenArgs a = make_args(MODE_EVAL);
  a.cur = rows;
  a.next = rows;
  a.score_cur = scores;
  a.score_next = scores;
  a.S = n;
  a.key_cur = nullptr;
  a.key_next = nullptr;
  a.stats_parts = nullptr;  // the island's own statistics are not these rows'
  a.n_elite = 0;
  a.elite_idx = nullptr;
  launch(MODE_EVAL, a, ev_parts_.as<unsigned long long>());
  return true;
}

// ----------------------------------------------------------------- JIT ---
void Island::set_jit_objective(std::shared_ptr<JitKernel> k) {
  if (k) {
    if (!on_gpu()) throw std::invalid_argument("JIT objectives need the GPU backend");
    if (cfg_.objective != OBJ_NONE) throw std::invalid_argument("a JIT objective needs objective OBJ_NONE");
    if (k->encoding != cfg_.encoding) throw std::invalid_argument("JIT objective compiled for another encoding");
    k->function(device_);  // load the module now: errors surface here, not mid-run
  }
  jit_ = std::move(k);
  jit_fused_off_ = false;
  config_changed();
}

bool Island::fused_jit_generation(GenArgs& a) {
  if (!on_gpu() || (cfg_.encoding != ENC_BINARY && cfg_.encoding != ENC_REAL) || jit_fused_off_) return false;
  uint32_t gs = 0;
  bool full = false, dense = false;
  if (cfg_.encoding == ENC_REAL ? !real_tp_plan(a, gs) : !binary_tp_plan(a, gs, full, dense)) return false;
  // no compile / module load inside a graph capture: there only a variant
  // loaded by an earlier plain generation is used
  hipFunction_t f = jit_->gen_function(device_, gs, full, dense, cfg_.L, !capturing_);
  if (!f) {
    if (!capturing_) jit_fused_off_ = true;  // fall back to generation + evaluation pass (fused_error() says why)
    return false;
  }
  TraceRange tr("pga.jit_generation", 2);
  const int nx = cur_ ^ 1;
  a.stats_parts = stats_at(nx);  // the fused kernel stores {min, sum} partials like the built-ins
  Derived made{jit_->gen_launch(f, &a, sizeof(a), cfg_.S, best_at(nx), kMaxGrid, stream)};
  made.stats = a.stats_parts != nullptr;
  scores_written(nx, made);
  ++jit_fused_gens_;
  return true;
}

uint32_t Island::jit_eval(const void* rows, float* scores, uint64_t n, unsigned long long* parts) {
  TraceRange tr("pga.jit_eval", 2);
  return jit_->eval(device_, rows, row_words_, n, cfg_.L, obj_data_[0].as<const float>(), scores, parts, kMaxGrid, stream);
}

// ------------------------------------------------------------ hipGraph ---
void Island::set_graph_generations(uint32_t g) {
  if (g % 2) ++g;  // even: the graph must end on the parity it started from
  graph_g_ = g;
  drop_graph();
}

void Island::drop_graph() {
  if (gexec_) (void)hipGraphExecDestroy(gexec_);
  gexec_ = nullptr;
  g_cur_ = -1;
}

bool Island::capture_graph() {
  drop_graph();
  reserve(gen_dev_, 64);
  if (!cap_stream_) PGA_HIP_CHECK(hipStreamCreateWithFlags(&cap_stream_, hipStreamNonBlocking));
  // workspaces that a stage would otherwise (re)allocate synchronously
  if (cfg_.n_elite > 1) {
    ensure_topk_ws(cfg_.n_elite);
  }
  const int cur0 = cur_;
  const uint32_t gen0 = gen_, nb0 = d_[cur_].n_best;
  hipStream_t user = stream;
  stream = cap_stream_;
  capturing_ = true;
  capture_base_ = gen_;
  hipGraph_t graph = nullptr;
  bool ok = hipStreamBeginCapture(cap_stream_, hipStreamCaptureModeThreadLocal) == hipSuccess;
  if (ok) {
    try {
      run_plain(graph_g_);
      advance_counter_launch(gen_dev_.as<uint32_t>(), graph_g_, cap_stream_);
    } catch (...) {
      ok = false;
    }
    ok = (hipStreamEndCapture(cap_stream_, &graph) == hipSuccess) && ok && graph;
  }
  capturing_ = false;
  stream = user;
  gen_ = gen0;  // the captured launches ran nothing: restore the host view
  if (cur_ != cur0) cur_ = cur0;
  if (ok) ok = hipGraphInstantiate(&gexec_, graph, nullptr, nullptr, 0) == hipSuccess;
  if (graph) (void)hipGraphDestroy(graph);
  if (!ok) {
    (void)hipGetLastError();
    gexec_ = nullptr;
    graph_broken_ = true;  // fall back to plain launches for good
    return false;
  }
  g_cur_ = cur0;
  g_epoch_ = epoch_;
  g_version_ = version_;
  g_nbest_ = nb0;
  g_len_ = graph_g_;
  return true;
}

bool Island::run_graph(uint32_t reps, bool fresh) {
  if (!fresh && !capture_graph()) return false;
  PGA_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)gen_dev_.ptr, (int)gen_, 1, stream));
  for (uint32_t r = 0; r < reps; ++r) PGA_HIP_CHECK(hipGraphLaunch(gexec_, stream));
  gen_ += reps * graph_g_;
  graph_replays_ += reps;
  return true;
}

// ------------------------------------------------------------ checkpoint ---
namespace {
struct CkptHeader {
  char magic[8];  // "PGACKPT1"
  uint32_t version, encoding, L, row_words;
  uint64_t S;
  uint32_t gen, epoch, island, pad;
  uint64_t seed;
};
}  // namespace

void Island::save(const std::string& path) {
  TraceRange tr("pga.checkpoint.save");
  CkptHeader h;
  std::memset(&h, 0, sizeof(h));
  std::memcpy(h.magic, "PGACKPT1", 8);
  h.version = 1;
  h.encoding = (uint32_t)cfg_.encoding;
  h.L = cfg_.L;
  h.row_words = row_words_;
  h.S = cfg_.S;
  h.gen = gen_;
  h.epoch = epoch_;
  h.island = cfg_.island;
  h.seed = cfg_.seed;
  std::vector<char> rows(4ull * row_words_ * cfg_.S);
  std::vector<float> sc(cfg_.S);
  copy_to_host(rows.data(), rows_[cur_].ptr, rows.size());
  copy_to_host(sc.data(), scores_[cur_].ptr, 4ull * cfg_.S);
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open checkpoint for writing: " + path);
  bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1 && std::fwrite(rows.data(), 1, rows.size(), f) == rows.size() &&
            std::fwrite(sc.data(), 4, cfg_.S, f) == cfg_.S;
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) throw std::runtime_error("short write to checkpoint: " + path);
}

void Island::load(const std::string& path) {
  TraceRange tr("pga.checkpoint.load");
  config_changed();
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open checkpoint: " + path);
  CkptHeader h;
  if (std::fread(&h, sizeof(h), 1, f) != 1 || std::memcmp(h.magic, "PGACKPT1", 8) != 0) {
    std::fclose(f);
    throw std::runtime_error("not a pga checkpoint: " + path);
  }
  if (h.S != cfg_.S || h.L != cfg_.L || h.encoding != (uint32_t)cfg_.encoding || h.row_words != row_words_) {
    std::fclose(f);
    throw std::runtime_error("checkpoint geometry does not match this population");
  }
  std::vector<char> rows(4ull * row_words_ * cfg_.S);
  std::vector<float> sc(cfg_.S);
  bool ok = std::fread(rows.data(), 1, rows.size(), f) == rows.size() && std::fread(sc.data(), 4, cfg_.S, f) == cfg_.S;
  std::fclose(f);
  if (!ok) throw std::runtime_error("truncated checkpoint: " + path);
  copy_to_device(rows_[cur_].ptr, rows.data(), rows.size());
  copy_to_device(scores_[cur_].ptr, sc.data(), 4ull * cfg_.S);
  gen_ = h.gen;
  epoch_ = h.epoch;
  cfg_.seed = h.seed;
  cfg_.island = h.island;
  rebest();
}

}  // namespace pga
