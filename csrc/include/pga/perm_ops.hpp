// perm_ops.hpp — PERMUTATION encoding semantics shared by the gfx950 kernel
// (csrc/kernels/perm.hip) and the CPU reference (csrc/cpu/cpu_perm.cpp).
// Genes are u16 city ids; a chunk is 8 genes (16 bytes).  Every operator is a
// deterministic function of the parents and the child's random words, so the
// GPU and CPU produce identical children.
#pragma once

#include "pga/core.hpp"

namespace pga {

// longest genome of the 4-individuals-per-block kernels (their LDS arrays);
// longer ones run one individual per 64-lane block (perm.hip go_long), and so
// do the few below it whose arrays no longer fit beside Euclidean coordinates
constexpr uint32_t kPermMaxL = 4096;

// child-word layout extension for permutations
//   W_CUT1, W_CUT2  segment [lo, hi) of parent A (PMX / OX)
//   W_MUTIND        per-individual mutation test
//   W_MUTPOS, W_SEL + sel_words   the two mutation positions
PGA_HD void perm_segment(uint32_t w1, uint32_t w2, uint32_t L, uint32_t& lo, uint32_t& hi) {
  uint32_t a = word_to_index(w1, L), b = word_to_index(w2, L + 1);  // hi may be L
  if (a > b) { uint32_t t = a; a = b; b = t; }
  lo = a;
  hi = b;
}

// Fisher-Yates (Durstenfeld) with j_i = index(word_i, i + 1), i = L-1 .. 1,
// word_i = register i%4 of ST_INIT block i/4
PGA_HD uint32_t perm_init_word(const RngKey& key, uint64_t child, uint32_t i) {
  return sel4(draw(key, ST_INIT, child, i / 4u), i % 4u);
}

PGA_HD void perm_mut_positions(uint32_t w1, uint32_t w2, uint32_t L, uint32_t& i, uint32_t& j) {
  i = word_to_index(w1, L);
  j = word_to_index(w2, L);
  if (i > j) { uint32_t t = i; i = j; j = t; }
}

// ------------------------------------------------ 2-opt local search ---
// One move on the tour t[0..L): over every pair (i, j), 0 <= i, i + 2 <= j < L
// (closed tours: not (0, L - 1)), with a = t[i], b = t[i+1], c = t[j],
// e = t[(j+1) % L],
//   gain = (d(a,b) + d(c,e)) - (d(a,c) + d(b,e))      in f32, this association
// d = the value the evaluation sums (the matrix entry, or tsp_euc_dist).  An
// open path is a closed tour whose closing edge has length 0: for j = L - 1,
// d(c,e) = d(b,e) = 0.  The pair with the largest gain wins, ties to the
// smallest i, then the smallest j: the maximum of two_opt_key.  A gain > 0
// reverses t[i+1 .. j]; otherwise (NaN included) the tour is 2-optimal.
// fl(x) > fl(y) implies x > y, so every move shortens the true tour and the
// search ends without an epsilon.  d must be symmetric bit for bit (the
// reversed edges keep their lengths).
PGA_HD float two_opt_gain(float dab, float dce, float dac, float dbe) { return (dab + dce) - (dac + dbe); }
// a candidate's key (0: no candidate); pairs are numbered i * L + j < 2^32
PGA_HD unsigned long long two_opt_key(float gain, uint32_t pair) {
  return gain > 0.f ? (((unsigned long long)score_key(gain) << 32) | (0xFFFFFFFFu - pair)) : 0ull;
}
PGA_HD uint32_t two_opt_pair(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }
// last j paired with i (the closed tour's pair (0, L - 1) shares the city t[0])
PGA_HD uint32_t two_opt_jmax(uint32_t i, uint32_t L, bool open) { return (i == 0 && !open) ? L - 2 : L - 1; }
// ------------------------------------------------ Or-opt local search ---
// One move on the tour t[0..L), el[k] = d(t[k], t[(k+1) % L]) (open path:
// el[L-1] = 0, as for 2-opt): a candidate (p, s, q, r) takes the segment
// t[p .. p+s), s in {1, 2, 3}, p + s <= L, s <= L - 2 (it never wraps), out of
// the tour and puts it back between c = t[q] and e = t[(q+1) % L], reversed
// when r = 1 (s >= 2 only).  q runs over [0, L) without the segment's own
// positions and the edge in front of it, (p - 1 + L) % L.  With a = t[p-1],
// x = t[p], y = t[p+s-1], b = t[(p+s) % L], in f32 with this association:
//   removed = (el[p-1] + el[p+s-1]) + el[q]
//   r = 0:  gain = removed - ((d(a,b) + d(c,x)) + d(y,e))
//   r = 1:  gain = (removed + If) - (((d(a,b) + d(c,y)) + d(x,e)) + Ir)
// If = the segment's own edges forwards, el[p] (+ el[p+1]), Ir = backwards,
// d(t[p+1], t[p]) (+ d(t[p+2], t[p+1])).  No edge outside a reversed segment
// changes direction, so d need not be symmetric.  Every new edge that lands on
// an open path's closing position (array index L-1 -> 0 of the new array)
// counts 0: d(a,b) when p = 0 or p + s = L, and the last term of `added` when
// q = L - 1.  The largest gain wins, ties to the smallest (p, q, s, r): the
// maximum of or_opt_key.  A gain > 0 applies the move -- the segment leaves
// the array and goes in directly behind the city that was t[q], for q = L - 1
// at the array's end -- otherwise (NaN included) the tour is Or-optimal.
PGA_HD float or_opt_removed(float el_prev, float el_end, float el_q) { return (el_prev + el_end) + el_q; }
PGA_HD float or_opt_gain(float removed, float dab, float dcx, float dye) { return removed - ((dab + dcx) + dye); }
PGA_HD float or_opt_gain_rev(float removed, float fwd, float dab, float dcy, float dxe, float rev) {
  return (removed + fwd) - (((dab + dcy) + dxe) + rev);
}
// longest segment starting at p
PGA_HD uint32_t or_opt_smax(uint32_t p, uint32_t L) {
  const uint32_t m = L - p < 3u ? L - p : 3u;
  return L < 3u ? 0u : (m < L - 2u ? m : L - 2u);
}
// q may take the segment (p, s): not in it, not the edge in front of it
PGA_HD bool or_opt_q_ok(uint32_t p, uint32_t s, uint32_t q, uint32_t L) {
  return (q < p || q >= p + s) && q != (p ? p - 1u : L - 1u);
}
// candidates are numbered in (p, q, s, r) order; the number stays under 2^32
// for L <= kPermMaxL (the GPU's limit; the CPU stage compares the fields)
PGA_HD uint32_t or_opt_cand(uint32_t p, uint32_t q, uint32_t s, uint32_t r, uint32_t L) {
  return ((p * L + q) * 3u + (s - 1u)) * 2u + r;
}
PGA_HD void or_opt_decode(uint32_t cand, uint32_t L, uint32_t& p, uint32_t& q, uint32_t& s, uint32_t& r) {
  r = cand & 1u;
  cand >>= 1;
  s = cand % 3u + 1u;
  cand /= 3u;
  p = cand / L;
  q = cand - p * L;
}
PGA_HD unsigned long long or_opt_key(float gain, uint32_t cand) { return two_opt_key(gain, cand); }
PGA_HD uint32_t or_opt_key_cand(unsigned long long key) { return two_opt_pair(key); }

// the Euclidean edge as every evaluation computes it
PGA_HD float tsp_euc_dist(const float* xy, uint32_t u, uint32_t w) {
  const float dx = xy[2 * u] - xy[2 * w], dy = xy[2 * u + 1] - xy[2 * w + 1];
  return __builtin_sqrtf(__builtin_fmaf(dx, dx, dy * dy));
}

}  // namespace pga
