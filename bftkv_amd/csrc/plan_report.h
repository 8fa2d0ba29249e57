// Launch sizing of the verify step (plain C++, no HIP: also built into a host test): the one place that turns a call's work into
// blocks, for everything run_pipeline launches behind the parse, in both phases and for every kind of call.
//
// A call enqueues its whole step before it knows what the step holds, so every grid covers `total` packets and exits on a
// device-side count: that is decide() with `enabled` false, and every grid of phase 1's modexp and inverses, which are in the
// queue before any word can arrive.  For a resident big call under a plan, k_scan_counts and k_plan<1> report through the pinned
// mailbox what the call really holds; the host waits for those words once the machine-filling modexp is in the queue
// (run_pipeline) and decide() turns them into the grids of everything that is enqueued after that wait:
//   - the walk's fill pass: only when some item overflowed its scratch row;
//   - the midstates of the hashes other than SHA-256 (payload and text mode): only when a signature names one;
//   - the 19 x 4 pass over values too long for the 29-bit form (WIDE_ONLY): only when the parse flagged one;
//   - phase 1's compare and DSA kernels: by the reported length of their work list;
//   - every phase-2 grid: by total - (sum of the reported lengths).  A record is queued at most once, so no list can grow
//     by more than that in phase 2.
// A word that did not arrive, or lengths that cannot be true (one above `total`, or their sum), count as absent, and what an
// absent word would have sized gets the grid it always had.  0 blocks means: not launched.
#ifndef BFTKV_PLAN_REPORT_H
#define BFTKV_PLAN_REPORT_H
#include <cstdint>

namespace plan_report {

// mailbox words this report adds or reads (uint32_t index into the pinned 64-byte mailbox of a context; words 0 .. 2 are the
// packet count, a staged call's sequence number and the chunk arena units)
constexpr int MAIL_PLAN_FLAGS = 3,      // k_plan<1>, first block: ARRIVED | FLAG_*
              MAIL_OVERFLOW = 4,        // k_scan_counts: items that overflowed their walk scratch row (written before the packet count)
              MAIL_LEN0 = 5;            // k_plan<1>, last block: ARRIVED | length of work list k after phase 1, k = 0..3
constexpr uint32_t ARRIVED = 0x80000000u;
constexpr uint32_t FLAG_OTHER_HASH = 1u;      // some signature uses a hash other than SHA-256
constexpr uint32_t FLAG_WIDE_VALUE = 2u;      // some RSA value is too long for the 29-bit form

// work lists, in the order of pk_count[0..3]
enum List { L_RSA2048 = 0, L_DSA = 1, L_RSA3072 = 2, L_RSA4096 = 3, N_LISTS = 4 };

// numbers (or packets) per block of each kernel family: the defaults are those of the default build, and run_pipeline sets every
// field from the kernels' own constants before it asks
struct Geometry {
  uint32_t modexp4 = 64;       // k_rsa_modexp, 4 lanes per number (MODEXP_BLOCK / MONT_TPI): the pass over long values
  uint32_t modexp8 = 32;       // ... 8 lanes (MODEXP_BLOCK / MONT_TPI_BIG): the 3072- and 4096-bit passes
  uint32_t modexp_main = 64;   // the main pass: modexp4, or modexp8 where a small staged call spreads its numbers over 8 lanes
  uint32_t compare = 64;       // k_rsa_compare (256 / CMP_LANES)
  uint32_t dsa_mul = 64;       // k_dsa_mul, k_dsa_inv: thread per signature, one wave
  uint32_t dsa_split = 256;    // k_dsa_split
  uint32_t dsa4 = 64;          // k_dsa_modexp<19, 4> (RSA_BLOCK / MONT_TPI)
  uint32_t dsa8 = 32;          // k_dsa_modexp<14, 8>
  uint32_t inv_tile = 4096;    // k_dsa_inv_batched
  uint32_t mid_items = 64;     // k_hash_mid_other / k_hash_mid_text: items per block
  uint32_t n_hashes = 7;       // grid.y of k_hash_mid_text; k_hash_mid_other: one less
};

struct Input {
  uint32_t total = 0;            // packets of the call
  uint32_t n_items = 0;
  bool enabled = true;           // false (BFTKV_PLAN_REPORT=0): ignore every word
  bool wide_form = true;         // the call has the pass over long values (the 29-bit form and WIDE_ONLY behind it); false (a build
                                 // of the 28-bit form, a main pass on 8 lanes): never launched
  bool overflow_arrived = false; uint32_t overflow_items = 0;     // MAIL_OVERFLOW (arrives with the packet count)
  uint32_t flags_word = 0;       // MAIL_PLAN_FLAGS as read (0: not arrived)
  uint32_t len_word[N_LISTS] = {0, 0, 0, 0};      // MAIL_LEN0.. as read (0: not arrived)
  // what the key table holds
  bool have_rsa3072 = false, have_rsa4096 = false, have_dsa2048 = false, have_dsa3072 = false;
  bool dsa_inv_batched = false, dsa_inv_single = false;     // which of the two inverse kernels run_pipeline enqueues (both: the device picks)
};

// per phase
struct PhaseGrids {
  uint32_t modexp = 0, modexp3072 = 0, modexp4096 = 0;      // k_rsa_modexp: the main pass, the 3072- and 4096-bit lists
  uint32_t wide = 0;                     // k_rsa_modexp<19, 4, 28, WIDE_ONLY>
  uint32_t dsa_inv_batched = 0, dsa_inv = 0;     // k_dsa_inv_batched, k_dsa_inv
  uint32_t compare[N_LISTS] = {0, 0, 0, 0};      // k_rsa_compare per RSA list ([L_DSA] stays 0)
  uint32_t dsa_mul = 0, dsa_split = 0, dsa_modexp4 = 0, dsa_modexp8 = 0;
};
struct Decision {
  bool flags_used = false, lengths_used = false, overflow_used = false;     // which words sized this call
  uint32_t phase2_bound = 0;             // packets phase 2 can still queue (total when the lengths are absent)
  uint32_t walk_fill = 0;                // k_walk<true>
  uint32_t mid_x = 0, mid_other = 0, mid_text = 0;      // k_hash_mid_other, k_hash_mid_text: grid.x, and grid.x * grid.y of each
  PhaseGrids p1, p2;
};

inline uint32_t blocks_for(uint64_t work, uint32_t per_block) { return (uint32_t)((work + per_block - 1) / per_block); }

// `queued`: what the phase's modexp and inverse passes can find in a list; `work`: the same per list for what runs behind them
inline void size_phase(PhaseGrids* g, const Input& in, const Geometry& geo, bool wide, uint64_t queued, const uint64_t work[N_LISTS]) {
  g->modexp = blocks_for(queued, geo.modexp_main);
  g->modexp3072 = in.have_rsa3072 ? blocks_for(queued, geo.modexp8) : 0u;
  g->modexp4096 = in.have_rsa4096 ? blocks_for(queued, geo.modexp8) : 0u;
  g->wide = wide ? blocks_for(work[L_RSA2048], geo.modexp4) : 0u;
  g->compare[L_RSA2048] = blocks_for(work[L_RSA2048], geo.compare);
  g->compare[L_DSA] = 0;
  g->compare[L_RSA3072] = in.have_rsa3072 ? blocks_for(work[L_RSA3072], geo.compare) : 0u;
  g->compare[L_RSA4096] = in.have_rsa4096 ? blocks_for(work[L_RSA4096], geo.compare) : 0u;
  const bool dsa = in.have_dsa2048 || in.have_dsa3072;
  g->dsa_inv_batched = dsa && in.dsa_inv_batched ? blocks_for(queued, geo.inv_tile) : 0u;
  g->dsa_inv = dsa && in.dsa_inv_single ? blocks_for(queued, geo.dsa_mul) : 0u;
  g->dsa_mul = dsa ? blocks_for(work[L_DSA], geo.dsa_mul) : 0u;
  g->dsa_split = in.have_dsa2048 && in.have_dsa3072 ? blocks_for(work[L_DSA], geo.dsa_split) : 0u;
  g->dsa_modexp4 = in.have_dsa2048 ? blocks_for(work[L_DSA], geo.dsa4) : 0u;
  g->dsa_modexp8 = in.have_dsa3072 ? blocks_for(work[L_DSA], geo.dsa8) : 0u;
}

// (`total` == 0: every grid over packets is 0, an empty call launches none of them)
inline Decision decide(const Input& in, const Geometry& geo = Geometry()) {
  Decision d;
  const uint64_t total = in.total;
  d.overflow_used = in.enabled && in.overflow_arrived && in.overflow_items <= in.n_items;
  d.flags_used = in.enabled && (in.flags_word & ARRIVED) != 0;
  uint64_t len[N_LISTS], sum = 0;
  bool have_len = in.enabled;
  for (int k = 0; k < N_LISTS; ++k) {
    have_len = have_len && (in.len_word[k] & ARRIVED) != 0;
    len[k] = in.len_word[k] & ~ARRIVED;
    have_len = have_len && len[k] <= total;
    sum += len[k];
  }
  have_len = have_len && sum <= total;
  // (lists the key table cannot feed must be empty: a length there says the words are not this call's)
  if (have_len && ((!in.have_rsa3072 && len[L_RSA3072]) || (!in.have_rsa4096 && len[L_RSA4096]) ||
                   (!in.have_dsa2048 && !in.have_dsa3072 && len[L_DSA]))) have_len = false;
  d.lengths_used = have_len;
  const bool other = d.flags_used ? (in.flags_word & FLAG_OTHER_HASH) != 0 : true;
  const bool wide = in.wide_form && (d.flags_used ? (in.flags_word & FLAG_WIDE_VALUE) != 0 : true);

  d.walk_fill = (d.overflow_used && in.overflow_items == 0) ? 0u : in.n_items;
  d.mid_x = blocks_for(in.n_items, geo.mid_items);
  d.mid_other = other ? d.mid_x * (geo.n_hashes - 1) : 0u;
  d.mid_text = other ? d.mid_x * geo.n_hashes : 0u;

  uint64_t w1[N_LISTS], w2[N_LISTS];
  d.phase2_bound = (uint32_t)(have_len ? total - sum : total);
  for (int k = 0; k < N_LISTS; ++k) { w1[k] = have_len ? len[k] : total; w2[k] = d.phase2_bound; }
  // phase 1's modexp and inverses are in the queue before the words can arrive: over `total`.  (Its wide pass is not: it is
  // enqueued behind the wait, over the list's length.)
  size_phase(&d.p1, in, geo, wide, total, w1);
  size_phase(&d.p2, in, geo, wide, d.phase2_bound, w2);
  return d;
}

// flat form for the diagnostics getter (bftkv_gpu_last_plan_report): blocks per launch, 0 = not launched, of what is enqueued
// behind the wait (phase 1's modexp and inverse grids, in the queue ahead of it, are always those over `total`: not reported)
enum Slot {
  S_WORDS = 0,            // bit 0 flags word used, bit 1 lengths used, bit 2 overflow word used, bit 3 the report was enabled
  S_PHASE2_BOUND,
  S_WALK_FILL, S_MID_OTHER, S_MID_TEXT,
  S_WIDE1, S_COMPARE1, S_COMPARE1_3072, S_COMPARE1_4096, S_DSA_MUL1, S_DSA_SPLIT1, S_DSA_MODEXP1_4, S_DSA_MODEXP1_8,
  S_MODEXP2, S_WIDE2, S_MODEXP2_3072, S_MODEXP2_4096, S_COMPARE2, S_COMPARE2_3072, S_COMPARE2_4096,
  S_DSA_INV2_BATCHED, S_DSA_INV2, S_DSA_MUL2, S_DSA_SPLIT2, S_DSA_MODEXP2_4, S_DSA_MODEXP2_8,
  S_TOTAL,                // packets of the call
  N_SLOTS
};
inline void flatten(const Decision& d, const Input& in, uint32_t out[N_SLOTS]) {
  out[S_WORDS] = (d.flags_used ? 1u : 0u) | (d.lengths_used ? 2u : 0u) | (d.overflow_used ? 4u : 0u) | (in.enabled ? 8u : 0u);
  out[S_PHASE2_BOUND] = d.phase2_bound;
  out[S_WALK_FILL] = d.walk_fill; out[S_MID_OTHER] = d.mid_other; out[S_MID_TEXT] = d.mid_text;
  out[S_WIDE1] = d.p1.wide; out[S_COMPARE1] = d.p1.compare[L_RSA2048]; out[S_COMPARE1_3072] = d.p1.compare[L_RSA3072];
  out[S_COMPARE1_4096] = d.p1.compare[L_RSA4096]; out[S_DSA_MUL1] = d.p1.dsa_mul; out[S_DSA_SPLIT1] = d.p1.dsa_split;
  out[S_DSA_MODEXP1_4] = d.p1.dsa_modexp4; out[S_DSA_MODEXP1_8] = d.p1.dsa_modexp8;
  out[S_MODEXP2] = d.p2.modexp; out[S_WIDE2] = d.p2.wide; out[S_MODEXP2_3072] = d.p2.modexp3072; out[S_MODEXP2_4096] = d.p2.modexp4096;
  out[S_COMPARE2] = d.p2.compare[L_RSA2048]; out[S_COMPARE2_3072] = d.p2.compare[L_RSA3072]; out[S_COMPARE2_4096] = d.p2.compare[L_RSA4096];
  out[S_DSA_INV2_BATCHED] = d.p2.dsa_inv_batched; out[S_DSA_INV2] = d.p2.dsa_inv; out[S_DSA_MUL2] = d.p2.dsa_mul; out[S_DSA_SPLIT2] = d.p2.dsa_split;
  out[S_DSA_MODEXP2_4] = d.p2.dsa_modexp4; out[S_DSA_MODEXP2_8] = d.p2.dsa_modexp8;
  out[S_TOTAL] = in.total;
}

}  // namespace plan_report
#endif
