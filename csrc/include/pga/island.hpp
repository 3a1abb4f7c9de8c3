// island.hpp — the native GA runtime: one population (an "island") resident on
// one device (or on the host for the CPU reference backend).
//
// An Island owns its memory (double-buffered rows + scores, per-block best
// partials, mutation tables, objective data, top-k/roulette workspaces) and
// enqueues every stage on ONE stream without host synchronisation, so a run
// of n generations is n back-to-back fused kernel launches.  It is the
// engine behind both the reference-compatible C API (csrc/capi/pga.cpp,
// include/pga.h) and the torch bindings (csrc/python/bindings.cpp).
//
// Reference counterparts: struct population / struct pga (src/pga.cu:37-56),
// __fill_population (:107-118), pga_run (:376-391), pga_get_best (:218-236).
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "pga/core.hpp"
#include "pga/jit.hpp"
#include "pga/ops.hpp"

namespace pga {
struct TopkFused;  // ops.hpp
}

namespace pga {

struct Config {
  int32_t encoding = ENC_BINARY;
  uint64_t S = 0;
  uint32_t L = 0;
  int32_t selection = SEL_TOURNAMENT;
  uint32_t tour_k = 2;
  int32_t crossover = XO_UNIFORM;
  float xo_prob = 1.f;
  float blend_alpha = 0.5f;
  int32_t mutation = MUT_BIT_FLIP;
  float mut_rate = -1.f;  // < 0: 1/L per gene (BIT_FLIP/GAUSSIAN/UNIFORM), 0.01 per individual (RESET_ONE...)
  float sigma = 0.1f;
  float rank_pressure = 1.5f;  // SEL_RANK: expected copies of the best individual, in [1, 2]
  float lo = 0.f, hi = 1.f;
  int32_t objective = OBJ_ONEMAX;
  int32_t obj_i = 0;
  float obj_f0 = 0.f, obj_f1 = 0.f;
  uint32_t n_elite = 0;
  uint64_t seed = 0;
  uint32_t island = 0;
  // local search stage after every generation of run() / run_until()
  // (Island::local_search): LS_NONE, LS_TWO_OPT or LS_ONE_FLIP, moves per selected
  // individual, share of the population selected
  int32_t local_search = LS_NONE;
  uint32_t ls_moves = 1;
  float ls_prob = 1.f;
};

// words per row and gene chunks for an encoding
void row_geometry(int32_t encoding, uint32_t L, uint32_t* row_words, uint32_t* chunks);

// Owning, move-only memory: hipMalloc on the device, or 64-byte aligned and
// zeroed on the host, chosen when it is allocated.  The destructor frees it and
// swallows errors.
struct Buffer {
  void* ptr = nullptr;
  size_t bytes = 0;

  Buffer() = default;
  Buffer(size_t n, bool device);
  Buffer(Buffer&& o) noexcept : ptr(o.ptr), bytes(o.bytes), device_(o.device_) { o.ptr = nullptr, o.bytes = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    std::swap(ptr, o.ptr), std::swap(bytes, o.bytes), std::swap(device_, o.device_);  // o frees the old memory
    return *this;
  }
  ~Buffer();
  // grow-only: a fresh allocation of n bytes (the contents are not kept) when
  // fewer are held; true when it reallocated
  bool reserve(size_t n, bool device) {
    if (bytes >= n) return false;
    *this = Buffer(n, device);
    return true;
  }
  template <typename T>
  T* as() const { return (T*)ptr; }

 private:
  bool device_ = false;
};

class Island {
 public:
  // device >= 0: GPU ordinal; device < 0: CPU reference backend
  Island(const Config& cfg, int device);
  ~Island();
  Island(const Island&) = delete;
  Island& operator=(const Island&) = delete;

  const Config& config() const { return cfg_; }
  bool on_gpu() const { return device_ >= 0; }
  int device() const { return device_; }
  uint32_t row_words() const { return row_words_; }
  uint32_t chunks() const { return chunks_; }
  uint32_t generation() const { return gen_; }
  void set_generation(uint32_t g) { gen_ = g; }
  uint32_t epoch() const { return epoch_; }
  void bump_epoch() { ++epoch_; }

  hipStream_t stream = nullptr;

  // ---- configuration (may be changed between generations) ----
  void set_operators(const Config& c);  // selection/crossover/mutation/objective scalars
  void set_objective_data(const float* host, size_t n, int which);  // which = 0 or 1
  void set_user_fn(void* f) {
    user_fn_ = f;
    config_changed();
  }
  // reference-ABI crossover_f / mutate_f device pointers (nullptr = built-in)
  void set_user_operators(void* xo, void* mut);
  // hipRTC-compiled objective (jit.hpp); needs objective OBJ_NONE and the GPU.
  // Its data pointer is objective data slot 0.  nullptr detaches.
  void set_jit_objective(std::shared_ptr<JitKernel> k);
  bool has_jit() const { return (bool)jit_; }
  // generations whose JIT objective ran inside the generation kernel (fused),
  // and why fusion is off when it is ("" while it works or was never tried)
  uint64_t jit_fused_generations() const { return jit_fused_gens_; }
  std::string jit_fused_error() const { return jit_ ? jit_->fused_error() : std::string(); }

  // ---- stages ----
  void initialize();          // random population + evaluation (generation 0)
  void evaluate();            // scores(cur) <- objective(rows(cur))
  void run(uint32_t n);       // n fused generations
  // n generations of several islands of one device as ONE launch per
  // generation (binary_launch_batch: BINARY, same shape / operators, built-in
  // integer objective); every island's stream is set to s.  Returns false
  // (nothing run) when the islands do not qualify: run them one by one.
  static bool run_batched(const std::vector<Island*>& isls, uint32_t n, hipStream_t s);
  // up to n generations, stopping once the best score reaches `target`; the
  // best is read (one stream sync) every `check_every` generations (0: 10).
  // Returns the generations run.
  uint32_t run_until(uint32_t n, float target, uint32_t check_every);
  void crossover_stage();     // next <- crossover(select(cur))  (no mutation / evaluation)
  void mutate_stage();        // mutate next in place
  void swap();                // cur <-> next, generation++
  void rebest();              // recompute best partials (and tournament keys) of cur from its scores
  // 2-opt local search on the current population, in place (perm_ops.hpp
  // two_opt_*): up to `moves` best-improvement moves on every individual n
  // with prob >= 1 or draw(key, ST_LS, n, 0).x < prob * 2^32, key.gen = the
  // current generation counter -- so two calls in one generation select the
  // same individuals.  Rows that moved get the score evaluate() would give
  // them; every other row and score is untouched.  Best partials are current
  // afterwards; the generation counter does not advance.  PERMUTATION with a
  // TSP objective (matrix objectives: a symmetric matrix), no JIT objective.
  // BINARY with OBJ_QUBO runs the one-flip stage instead (qubo_ops.hpp): up to
  // `moves` best-improvement single-bit flips, the same selection rule.
  // With Config::local_search = LS_OR_OPT the PERMUTATION stage is Or-opt
  // (perm_ops.hpp or_opt_*): segments of 1 to 3 cities move, in either
  // orientation; any matrix, symmetric or not.  The second form names the
  // kind for this one stage, whatever the configuration says.
  void local_search(uint32_t moves, float prob);
  void local_search(uint32_t moves, float prob, int kind);

  // ---- queries (synchronise the stream) ----
  unsigned long long best_packed();
  float best_score() { return pga::best_score(best_packed()); }
  uint64_t best_index() { return pga::best_index(best_packed()); }
  void stats(float out4[4]);  // min, max, sum, count of current scores
  // Per-generation statistics history: when on, every generation appends its
  // {min, max, sum, count} row on the device (from the generation kernel's
  // fused partials, no pass over the scores); history() copies the rows out.
  // Turning it on clears the history and disables hipGraph replay.
  void set_stats_history(bool on);
  // manual history: generations append no row themselves; the caller appends
  // one per generation with record_history_row() once the scores are final
  // (an objective evaluated outside the island, e.g. GeneticAlgorithm's
  // torch_objective)
  void set_history_manual(bool on) { hist_manual_ = on; }
  void record_history_row() {
    if (hist_on_) append_history();
  }
  bool stats_history() const { return hist_on_; }
  std::vector<float> history();
  std::vector<uint32_t> topk_host(uint32_t k, bool largest);
  std::vector<uint32_t> row_host(uint64_t i);
  // read-only view of the REAL quantized tournament keys (tests): host copies
  // of the u16 keys of parity `which` (the convention of rows(which)) and of
  // the range {min, max} they were last refreshed to.  false when this island
  // keeps no such keys or those of that parity are not valid.  Launches
  // nothing and changes no state (the refresh age included).
  bool qkeys_host(int which, std::vector<uint16_t>& keys, float range[2]);
  // read-only record of the kernel the last PERMUTATION generation took on
  // the GPU (tests; ops.hpp PermRoute): kernel PERM_K_NONE before the first
  // generation, on the CPU backend and for the other encodings
  const PermRoute& route() const { return route_; }

  // ---- device-side building blocks (no sync) ----
  // idx_out: device (or host for CPU) memory.  sorted: best first (ties by
  // index); unsorted: selection order, cheaper (migration, elitism)
  void topk(uint32_t k, bool largest, uint32_t* idx_out, bool sorted = true);
  void gather(const uint32_t* idx, uint32_t n, void* out_rows, float* out_scores);
  void scatter(const uint32_t* idx, uint32_t n, const void* in_rows, const float* in_scores);
  // Island migration, stream-ordered: emigrate = the top-k rows + scores
  // (selection order) into out buffers; immigrate = the k given rows replace
  // the bottom-k (then best partials follow).  On the GPU, integer objectives
  // do each in ONE selection kernel with the row moves fused in; otherwise
  // topk + gather / scatter.  `idx_scratch` (k words, device) may be null.
  void emigrate(uint32_t k, void* out_rows, float* out_scores);
  // MIG_TOPK (default: the reference's "top pct%") or MIG_STRIPE, see core.hpp MigrationPolicy
  void set_migration_policy(int p);
  int migration_policy() const { return mig_policy_; }
  void immigrate(uint32_t k, const void* in_rows, const float* in_scores);
  // score n external rows (e.g. received migrants) with this island's
  // objective, in place; false when the objective is not native (OBJ_NONE)
  bool evaluate_rows(void* rows, float* scores, uint32_t n);
  // Fused key histogram (GenArgs::key_hist): when on, the BINARY generation
  // kernel of an integer objective also produces the value histogram of the
  // keys it writes, and the exact top-k / bottom-k selections of that
  // population (migration, elitism > 1, unsorted top-k) skip their histogram
  // pass over the keys.  On by default with elitism > 1; island models turn it
  // on for migration.  Results are identical either way.
  void set_fused_histogram(bool on);
  bool fused_histogram() const { return fhist_on_; }
  // a fused histogram of the current population is available (tests, benches)
  bool fused_histogram_ready() const { return d_[cur_].fhist >= 0; }

  // raw buffers (cur = current generation)
  void* rows(int which) { return rows_[which ^ cur_].ptr; }
  float* scores(int which) { return scores_at(which ^ cur_); }
  unsigned long long* best_parts() { return best_at(cur_); }
  uint32_t n_best() const { return d_[cur_].n_best; }
  void set_n_best(uint32_t n);
  size_t row_bytes() const { return 4ull * row_words_; }

  // scratch buffers for callers (migration staging)
  void* scratch(size_t bytes);

  // hipGraph replay: run() records G generations once per (parity, epoch,
  // configuration) and replays the graph; 0 disables.  Default: PGA_GRAPH
  // env (generations per graph), else 0.  Bit-identical to plain launches.
  // Off by default because it measured no gain on MI355X: even the smallest
  // populations (S=100) are bound by the kernel's own dependent memory chain
  // (~4.8 us/gen with or without the graph), not by host launch cost
  // (profiles/README.md).
  void set_graph_generations(uint32_t g);
  uint32_t graph_generations() const { return graph_g_; }
  uint64_t graph_replays() const { return graph_replays_; }
  // BINARY knapsack: int8 digits per value of the matrix-core evaluation
  // (0: the instance is not integer-exact and runs the scalar evaluation)
  uint32_t knapsack_digits() const { return knap_dig_; }
  // tail units of the last generation launch (binary_gen_tp's TAIL steps,
  // ops.hpp TpPartition::tail): 0 when the launch had none
  uint32_t tp_tail() const { return tp_tail_; }

  // checkpoint: header + current rows + scores
  void save(const std::string& path);
  void load(const std::string& path);

  void synchronize();
  void copy_to_host(void* dst, const void* src, size_t bytes);
  void copy_to_device(void* dst, const void* src, size_t bytes);

 private:
  // What is known about the population of parity p beyond rows_[p] and
  // scores_[p]: by-products of the kernel that last wrote scores_[p].  Only
  // the transitions below write it; scores_written() replaces the whole record
  // of p by what that kernel delivered (`made`, everything else: nothing).
  //
  //   event (parity)               n_best  stats  part  qk   fhist   rank_cnt
  //   scores_written(p, made):
  //     initialize, evaluate       grid    (a)    -     -    -       -
  //     jit_eval, rebest           grid    -      -     -    -       -
  //     immigrate: stripe, GPU     grid    (a)    -     -    -       -
  //                fused bottom-k  grid    -      -     -    -       -
  //     run_plain (next)           grid    (a)    (b)   (c)  (d)     (e)
  //     fused_jit_generation       grid    yes    -     -    -       -
  //     run_batched (next)         grid    (a)    -     (c)  -       -
  //     run_tiny: current / other  1 / 0   (a)/-  -     -    -       -
  //   keys_requantized (cur)       .       .      .     yes  .       .
  //   take_rank_counts (both)      .       .      .     .    .       -
  //   drop_key_counts (both)       .       .      .     .    -       -
  //   config_changed               = drop_key_counts, ++version_
  //   set_n_best(n) (cur)          n       -      -     .    .       .
  //   ("-": dropped, ".": kept)
  //   (a) the kernel was given stats_parts_[p] (fused_stats())
  //   (b) the report's partition, when (a) and its grid is the best-partials
  //       count (the roulette prefix's carries)
  //   (c) the REAL GEN kernel was given, and so wrote, quantized keys
  //   (d) only on the launcher's report that its kernel took GenArgs::key_hist,
  //       not on fhist_ready_for's prediction: fhist_[fhist_rot_ % 3].  It and
  //       the next buffer z, which the launch zeroed, become clean, the other
  //       parity loses a claim on z, the rotation advances.
  //   (e) on the launcher's report; rank_ws_ is ONE buffer, so the other
  //       parity loses its claim
  // drop_key_counts also precedes a staged / init / eval launch() on the
  // current rows and a graph replay (which produce neither).  qk_age_,
  // fhist_clean_ / fhist_rot_ and the graph freshness (g_*) are not in here.
  struct Derived {
    uint32_t n_best = 0;        // valid entries of best_[p]
    bool stats = false;         // stats_parts_[p] ({min, sum} per block) belongs to them
    TpPartition part{0, 0, 0};  // the binary_gen_tp launch that stored stats_parts_[p] (grid 0: another kernel)
    bool qk = false;            // keys_[p] holds the quantized keys of scores_[p] (REAL, see qk_ws_)
    int fhist = -1;             // the fhist_ buffer with the histogram of its keys (-1: none)
    bool rank_cnt = false;      // rank_ws_ holds the tile counts of its keys
  } d_[2];
  void scores_written(int p, const Derived& made);  // a kernel rewrote scores_[p]
  void keys_requantized() { d_[cur_].qk = true; }   // prepare_generation() re-keyed the current scores
  bool take_rank_counts();  // the current keys' tile counts are there; the sort that asks consumes them
  void drop_key_counts();   // the launches that follow produce no histogram and no rank counts
  void config_changed() { ++version_, drop_key_counts(); }
  uint32_t tp_tail_ = 0;  // tail units of the last GEN launch (its report), not a fact about a parity

  float* scores_at(int p) const { return scores_[p].as<float>(); }
  unsigned long long* best_at(int p) const { return best_[p].as<unsigned long long>(); }
  uint16_t* keys_at(int p) const { return keys_[p].as<uint16_t>(); }
  float* stats_at(int p) const { return stats_parts_[p].as<float>(); }
  // the integer objectives' exact u16 keys of parity p (nullptr: f32 scores)
  uint16_t* int_keys_at(int p) const { return integer_objective(cfg_.objective, cfg_.L) ? keys_at(p) : nullptr; }

  RngKey key() const;
  GenArgs make_args(int mode);
  LsArgs ls_args(int kind, uint32_t moves, float prob) const;
  LaunchReport launch(int mode, const GenArgs& a, unsigned long long* parts);
  PermRoute route_;  // of the last MODE_GEN launch (route())
  void evaluate_current(int mode);  // initialize() / evaluate(): MODE_INIT / MODE_EVAL on the current parity
  void prepare_generation();  // elitism indices, roulette prefix
  // grow-only b.reserve() on this island's backend; sync: the stream may
  // still use the memory it frees
  bool reserve(Buffer& b, size_t bytes, bool sync = false);
  void rebuild_mut_table();
  void ensure_topk_ws(uint32_t k);

  Config cfg_;
  int device_;
  uint32_t row_words_ = 0, chunks_ = 0;
  int cur_ = 0;
  uint32_t gen_ = 0, epoch_ = 0;
  Buffer rows_[2], scores_[2], best_[2], keys_[2];
  Buffer mut_thr_, obj_data_[2], elite_idx_, cumfit_, cum_ws_, topk_ws_, stats_, out_best_, scratch_;
  Buffer rank_order_, rank_ws_;
  Buffer roul_guide_;  // roulette guide table (GPU), S + 1 entries
  // REAL on the GPU: quantized u16 tournament keys in keys_[p] (qkey), valid
  // when d_[p].qk: written by the GEN kernel that bred parity p, or by
  // prepare_generation() after anything else rewrote its scores.  qk_ws_ =
  // {min, max, sum, count} (+ score_stats workspace) of the scores of the
  // generation of the last refresh (every 8 or 32 generations, qk_age_), NOT
  // of the current one: the range the GEN kernel quantizes the next
  // generation's keys over, and prepare_generation() a re-keyed current one.
  // All keys of ONE parity share a range; the two parities' ranges differ
  // across a refresh (only keys of one parity are ever compared).
  bool real_qk() const;
  Buffer qk_ws_;
  Buffer qubo_qt_;               // QUBO: int8 Q^T packed from objective data slot 0 (GPU)
  Buffer qubo_qn_;               // QUBO: int8 Q in the same padding (one-flip local search, GPU)
  uint32_t obj_version_ = 0, qubo_version_ = ~0u;
  // derived objective data, each rebuilt once per data version
  void prepare_objective() {
    prepare_knapsack();
    prepare_tsp_matrix();
    prepare_qubo();
  }
  void prepare_knapsack();    // BINARY knapsack: the matrix-core digit table
  void prepare_tsp_matrix();  // PERMUTATION TSP: the LDS-resident matrix
  void prepare_qubo();        // QUBO: the packed int8 matrices (throws when Q is not set)
  // slot 0 as an L x L matrix is bitwise symmetric (checked once per data version, both backends)
  bool matrix_symmetric();
  void one_flip_search(uint32_t moves, float prob);  // local_search() of BINARY / OBJ_QUBO
  uint32_t sym_version_ = ~0u;
  bool sym_ok_ = false;
  size_t obj_len_[2] = {0, 0};
  std::vector<float> obj_host0_;  // host copy of objective data slot 0 (derived tables)
  Buffer knap_tab_;               // BINARY knapsack: matrix-core digit table (GPU, integer instances)
  uint32_t knap_version_ = ~0u, knap_dig_ = 0, knap_cols_ = 0;
  // fused statistics partials per parity ({min, sum} per block of the kernel
  // that wrote best_[p]), current when d_[p].stats
  Buffer stats_parts_[2];
  bool fused_stats() const;  // the evaluating kernels of this configuration store them
  void append_history();
  Buffer hist_;
  std::vector<float> hist_host_;  // CPU backend
  uint64_t hist_n_ = 0;
  bool hist_on_ = false, hist_manual_ = false;
  int mig_policy_ = MIG_TOPK;
  float mut_inv_ = 0.f;
  bool mut_sparse_ = false;  // BINARY bit-flip uses the sparse (Binomial) sampler
  float mut_rate_eff_ = 0.f;
  void* user_fn_ = nullptr;
  void* user_xo_fn_ = nullptr;
  void* user_mut_fn_ = nullptr;
  Buffer compat_rand_, ev_parts_;
  std::shared_ptr<JitKernel> jit_;
  // JIT evaluation of `n` rows at `rows` -> scores, block bests -> parts; returns the grid
  uint32_t jit_eval(const void* rows, float* scores, uint64_t n, unsigned long long* parts);
  bool fused_jit_generation(GenArgs& a);
  uint32_t qk_age_ = 0;  // REAL quantized keys: generations since the range was refreshed
  bool jit_fused_off_ = false;
  uint64_t jit_fused_gens_ = 0;
  u32x4 last_mask_{0, 0, 0, 0};

  // graph replay state
  void run_plain(uint32_t n);
  bool run_tiny(uint32_t n);
  bool run_graph(uint32_t reps, bool fresh);
  bool capture_graph();
  void drop_graph();
  // fused key histograms: three buffers of fused_hist_words(L + 1) words
  // rotated by the generations that produce one (each zeroes the next);
  // d_[p].fhist = the buffer with the histogram of parity p's population
  Buffer fhist_[3];
  bool fhist_clean_[3] = {true, true, true};  // its selection status words are still zero
  uint32_t fhist_rot_ = 0;
  bool fhist_on_ = false, fhist_user_ = false;
  bool fhist_ready_for(const GenArgs& a);  // this GEN launch produces the histogram (allocates the buffers)
  // rank selection of an integer objective: the GEN kernel also stores the
  // next rank sort's tile counts into rank_ws_ (GenArgs::rank_counts) for the
  // parity it writes (d_[p].rank_cnt), consumed by the next
  // prepare_generation's sort
  uint32_t* rank_counts_for_gen() const;
  const TopkFused* fused_select(TopkFused& f);    // the current population's histogram for a select
  uint32_t graph_g_ = 0, version_ = 0;
  bool graph_broken_ = false, capturing_ = false;
  uint32_t capture_base_ = 0;
  Buffer gen_dev_;
  Buffer obj_aux_;        // derived objective table (TSP: the integer matrix as u16, GenArgs::obj_aux)
  uint32_t aux_kind_ = 0, aux_bytes_ = 0, aux_version_ = ~0u;
  bool aux_on_ = true;    // PGA_TSP_NO_LDS unset at construction
  uint32_t batch_n_ = 1;  // islands of the batch this one runs in (run_batched), else 1
  hipStream_t cap_stream_ = nullptr;
  hipGraphExec_t gexec_ = nullptr;
  int g_cur_ = -1;
  uint32_t g_epoch_ = 0, g_version_ = 0, g_nbest_ = 0, g_len_ = 0;
  uint64_t graph_replays_ = 0;
};

}  // namespace pga
