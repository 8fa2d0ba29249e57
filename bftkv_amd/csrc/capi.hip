// C ABI of the bftkv MI355X verifier (include/bftkv_gpu.h) -- host side: context, key table,
// quorum descriptors, grow-only device arena, kernel pipeline.
#include "../../include/bftkv_gpu.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits.h>
#include <linux/futex.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <memory>
#include <functional>
#include <map>
#include <set>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>
#include <system_error>
#include <thread>
#include <tuple>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_bignum.h"
#include "host_sha256.h"
#include "kernels.hip"
#include "threshold_kernels.hip"
#include "ec_kernels.hip"
#include "dsa_verify_kernels.hip"
#include "rsa_verify_kernels.hip"
#include "window_chain.h"
#include "tpa_kernels.hip"
#include "rsa_psign_kernels.hip"
#include "tsig_share_kernels.hip"
#include "rsa_sign_kernels.hip"

using namespace bftkv;

namespace {

// results to the caller's arrays: memcpy's pointers must be valid even for n = 0, and an empty vector's data() may be null
inline void copy_out(void* dst, const void* src, size_t n) { if (n) memcpy(dst, src, n); }

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  // exactly `bytes` (the DSA table arena: GBs, sized by its own policy -- ensure()'s quarter on top would be tens of GB)
  hipError_t ensure_exact(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <typename T> T* as() const { return (T*)p; }
};

struct KeyEntry {
  uint64_t key_id = 0, entity_id = 0;
  uint8_t algo = 0, flags = 0;
  uint32_t bits = 0, e = 0, n0 = 0, qbits = 0, n0_29 = 0;
  std::vector<uint32_t> nl29, r2_29;    // <= 2048-bit RSA: n and (2^2088)^2 mod n as 72 limbs of 29 bits, with n0_29 = -n^-1 mod 2^29 (k_rsa_modexp<18,4,29>)
  std::vector<uint32_t> nl, r2, r2w, qw, dtab, qpow, qconst;    // r2w: R^2 mod n for the 80-limb form (<= 2048-bit RSA); qpow: 2^(28 j) mod q rows, qconst: mod-q Montgomery constants (DSA)
  std::string material;
  bool cert_only = false;
  int cert_group = -1;          // certificates: entries of one certificate share a group
  uint32_t entity_index = 0;   // filled by upload_key_table
  std::string cert_digest;     // certificates: identity of the certificate bytes
  uint64_t last_used = 0;      // certificates: the compound call (ctx->cert_clock) that last named this certificate
  bool dsa_unslotted = false;  // certificates: a DSA key that found no table slot at the last upload (its signatures are fenced)
};

struct QuorumHost {
  bool live = false;
  int n_qcs = 0;
  int32_t f[MAX_QC], mn[MAX_QC], thr[MAX_QC], suff[MAX_QC];
  std::vector<std::vector<uint64_t>> nodes;
  DevBuf member;          // [n_qcs][n_entities] bytes, keyed to the keyring generation below
  uint64_t keyring_gen = ~0ull;
  DevBuf ids;             // concatenated node ids
  uint32_t ids_off[MAX_QC + 1];
};

// A key set's own copy of the Montgomery rows of its moduli (n, R^2 mod n and -n^-1 per row; R_wide^2 mod n as well where the set's
// kernels read it), copied out of the context's cache, which may drop them: no call on the set uploads anything.
struct ModRows {
  DevBuf b[4];
  ModTab view() const { return ModTab{b[0].as<uint32_t>(), b[1].as<uint32_t>(), b[2].as<uint32_t>(), b[3].as<uint32_t>()}; }
  template <typename Set>                  // (the kind of the set that keeps the rows: it names the failure)
  int copy_from(bftkv_gpu_ctx* c, const ModTab& src, size_t n_rows, bool with_wide);
  void release() { for (DevBuf& x : b) x.release(); }
};

// The resident key sets.  Every kind has `live`, release(), its name in messages (`kind`) and the bytes of one signature under
// the set (sig_bytes); KeySets<Set> below keeps the handles of a kind.

// A resident ECDSA key set (ec_capi.inc): one fixed-base table per key, built on the device at registration
struct EcKeySet {
  static constexpr const char* kind = "ECDSA";
  bool live = false;
  int curve_id = -1;                       // index into kEcCurves
  uint32_t bits = 0, n_keys = 0, n_refused = 0;
  uint32_t w = 0, nwin = 0;                // window bits (the width of the context's G table when the set was made) and windows
  size_t key_words = 0;                    // fb_table_words of one key
  std::vector<uint8_t> curve;              // P || N || B || Gx || Gy
  DevBuf tab;                              // [n_keys][key_words]; the rows of a refused key are zero
  DevBuf refused;                          // [n_keys] bytes: 1 = elliptic.Unmarshal refuses the key
  ModRows mod;                             // N for k_modinv, with the wide row
  size_t sig_bytes() const { return 2 * (size_t)((bits + 7) / 8); }
  void release() { tab.release(); refused.release(); mod.release(); }
};

// A resident DSA key set (dsa_keyset_capi.inc): one fixed-base window table per distinct base, the groups' g first, then the keys' y
struct DsaKeySet {
  static constexpr const char* kind = "DSA";
  bool live = false;
  uint32_t n_keys = 0, n_groups = 0, pbytes = 0, qbytes = 0;
  uint32_t w = 0, windows = 0;             // window bits and ceil(max bits(q) / w)
  DevBuf tab;                              // [n_groups + n_keys][windows][2^w - 1][76], fully reduced Montgomery entries (R = 2^2128)
  ModRows modp, modq;                      // every p and q
  DevBuf q_be, key_group;                  // [n_groups][qbytes] bytes; [n_keys] clamped group indices
  DevBuf qc;                               // [n_groups] TsigMod<8>: every q in the eight-word form of tsig_share.h (bftkv_gpu_tdsa_share)
  uint64_t table_bytes() const { return (uint64_t)(n_groups + n_keys) * windows * ((1u << w) - 1u) * MONT_N * 4; }
  size_t sig_bytes() const { return 2 * (size_t)qbytes; }
  void release() { tab.release(); q_be.release(); key_group.release(); qc.release(); modp.release(); modq.release(); }
};

// A resident RSA key set (rsa_verify_capi.inc): the keys' Montgomery rows in both forms of k_rsav_verify.  An even modulus has
// zero rows and is counted in n_refused.
struct RsaKeySet {
  static constexpr const char* kind = "RSA";
  bool live = false;
  uint32_t n_keys = 0, n_refused = 0, nbytes = 0;
  DevBuf n29, r2_29, n80, r2_80;           // [n_keys][72] limbs of 29 bits (R = 2^2088); [n_keys][80] limbs of 28 bits (R = 2^2240)
  DevBuf meta;                             // [n_keys] uint4: -n^-1 mod 2^29, k = ceil(bits(n) / 8), e, 1 for an even n
  size_t sig_bytes() const { return nbytes; }
  void release() { n29.release(); r2_29.release(); n80.release(); r2_80.release(); meta.release(); }
};

// A resident RSA private key set (rsa_sign_capi.inc): per key the rows of p and q in the 10 x 4 form (R = 2^1120), dp and dq as bytes,
// qinv R mod p, and the verifier's rows of (n, e) for the check.  A refused key (n even; p or q even or below 3) has zero rows.
struct RsaSignerSet {
  static constexpr const char* kind = "RSA signer";
  bool live = false;
  uint32_t n_keys = 0, n_refused = 0, nbytes = 0, pbytes = 0;
  DevBuf mod, r2, r3, n0;                  // [n_keys][2][40] p | q, R^2 and R^3 mod each; [n_keys][2] -p^-1, -q^-1 mod 2^28        SECRET
  DevBuf d, qinv_r;                        // [n_keys][2][pbytes] dp | dq; [n_keys][40] qinv R mod p                              SECRET
  DevBuf refused;                          // [n_keys] bytes
  DevBuf n29, r2_29, meta;                 // the rows of an RsaKeySet's 18 x 4 form
  size_t sig_bytes() const { return nbytes; }
  void release();                          // overwrites the secret rows before it frees them
};

}  // namespace

using ctx_lock = std::lock_guard<std::recursive_mutex>;

struct bftkv_gpu_ctx {
  int device = 0;
  hipStream_t stream = nullptr;      // main stream: walk, parse, modexp, compare, tally
  hipStream_t stream_h = nullptr;    // hashing stream: runs beside the modexp
  hipStream_t stream_d = nullptr;    // DSA inverses (s^-1 mod q): latency-bound, runs beside both
  // One lock per context, RECURSIVE: the compound host entry points (certificate verification, Server.sign, ...) hold it
  // from entity resolution to the last pipeline call they make, so that no other thread can change the key table, the
  // certificate cache or the entity indices in between; the entry points they call re-acquire it.
  std::recursive_mutex mu;
  std::string err;

  // key table
  uint64_t keyring_gen = 0;
  uint32_t n_keys = 0, n_entities = 0;
  bool have_dsa_keys = false, have_rsa3072 = false, have_rsa4096 = false, have_ambiguous = false;
  std::vector<uint64_t> h_key_id, h_entity_id;      // per key slot / per entity
  std::vector<uint32_t> h_key_entity;
  std::vector<uint8_t> h_key_flags;
  std::vector<KeyEntry> ring, certs;   // processed rows: node keyring, then certificate-only entities
  uint32_t n_ring_entities = 0;
  std::map<std::string, bool> cert_valid;   // certificate bytes -> openpgp.ReadEntity would accept it
  DevBuf k_r2w;
  DevBuf k_n29, k_r2_29, k_n0_29;
  DevBuf k_id, k_entity, k_algo, k_flags, k_bits, k_e, k_n, k_r2, k_n0, k_q, k_qbits, k_dsatab, k_dsaslot, k_sorted_id, k_sorted_slot;
  // fixed-base DSA tables: built once per distinct key material, kept across key-table uploads
  DevBuf dsa_comb;
  uint32_t dsa_wbits = 8, dsa_wbits_pinned = 0;
  std::map<std::string, uint32_t> dsa_comb_slot;   // key material -> slot in dsa_comb
  std::set<std::string> dsa_cert_materials;        // ... those of certificate-only keys (bounded, recycled: sync_dsa_tables)
  uint64_t ring_epoch = 0, dsa_ring_epoch_seen = ~0ull;   // bftkv_gpu_keyring_set calls / the one the window width was chosen for
  uint32_t dsa_wbits_want = 0;
  uint32_t dsa_entry_limbs = DSA_N_SMALL;      // limbs of a table entry, arena-wide: DSA_N_BIG once the node keyring holds a DSA key with p beyond 2048 bits
  size_t dsa_budget_bytes = 0;                 // bftkv_gpu_set_dsa_table_budget: the arena never grows past this (0: the free-HBM policy)
  bool have_dsa3072 = false, have_dsa2048 = false;      // the key table holds a usable DSA key with p beyond / up to 2048 bits
  DevBuf dsa_idx;
  uint64_t cert_clock = 0;     // compound calls over request certificates (host_capi.inc cert_cache_gc)
  // Request certificates whose ReadEntity verdict is "valid" (cert_signature_core), by their bytes: a later request of the same
  // client is then ONE staged signature verification on a lane of the micro-batcher (batcher_capi.inc) instead of a compound call
  // on the root under its lock.  cert_fast_mu guards the map (a leaf lock; lookups share it).  A hit names the certificate's GROUP
  // and the epoch of that answer; the lane turns the group into an entity index through kt_group_ent, which -- like kt_cert_epoch
  // -- changes only under KtWrite (upload_key_table), i.e. never during a fork's device call: no lock on that side.  cert_epoch (under mu) counts the times the certificate rows
  // were dropped and the groups renumbered.
  struct CertFast { uint64_t issuer_id; int group; uint64_t epoch; };
  std::shared_mutex cert_fast_mu;
  std::unordered_map<std::string, CertFast> cert_fast;
  size_t cert_fast_bytes = 0;
  uint64_t cert_epoch = 0, kt_cert_epoch = 0;
  std::vector<uint32_t> kt_group_ent;
  KeyTableDev kt{};

  std::vector<QuorumHost> quorums;
  // root: the handles of bftkv_gpu_{ecdsa,dsa,rsa}_keyset_create and bftkv_gpu_rsa_signer_create, a space per kind; forks read them under KtRead, without a copy (KeySets)
  std::tuple<std::vector<EcKeySet>, std::vector<DsaKeySet>, std::vector<RsaKeySet>, std::vector<RsaSignerSet>> keysets;

  // per-call arena
  DevBuf txt_mid32, txt_mid64, txt_tail, txt_len;     // text-mode hashing state (TextDev)
  DevBuf forced_iss;      // per-item key ids of certificate checks (signature_verify_entities)
  DevBuf counts, base, total, item_flags, walk_scratch, cert_ent, sig_class, mid, mid64, hash_mask, recs, digests, r, xr, pk_list, pk_list3072, pk_list4096, r3072, r4096, pk_count, dsa_list, dsa_u, ids_tmp;
  DevBuf o_err, o_nver, o_verdict, o_fenced;
  DevBuf in_tbs, in_tbs_off, in_ss, in_ss_off;
  hipEvent_t seg_ev = nullptr;             // unsplit segmented call: the offsets are on the device (main stream -> hash stream)
  DevBuf in_prefix, in_prefix_off, in_shared, in_shared_off, in_seg;     // bftkv_gpu_collective_verify_segments: what crosses PCIe instead of whole payloads
  DevBuf st_tmp, item_tmp, bits_tmp, plan_cut;
  DevBuf chunk_arena, chunk_ctr;    // linearised partial-length signature bodies (parse_one) and their counters (k_walk / k_scan_counts)
  uint32_t multiexp_parts = 0;        // experiment knob (BFTKV_MULTIEXP_PARTS): quads per CalculateR operation, 0 = default policy
  uint32_t ec_split = 0;              // experiment knob (BFTKV_EC_SPLIT): ECDSA CalculateR lanes, 1 = per term, 2 = per operation, 0 = default policy
  uint32_t ec_window = 0;             // experiment knob (BFTKV_EC_WINDOW = 2..8): window bits of the fixed-base G tables, 0 = the default (4)
  DevBuf ec_fb_tab[4];                // ECDSA verification: the fixed-base table of G per recognised curve (ec_field.h fb_table_build), built at first use
  uint32_t ec_fb_w[4] = {};           // ... and its window width (0: not built)
  uint32_t multiexp_block = 0;        // experiment knob (BFTKV_MULTIEXP_BLOCK = 64): one-wave blocks for the 4-lane k_multiexp
  uint32_t multiexp_lanes = 0;        // experiment knob (BFTKV_MULTIEXP_LANES = 4 | 8): lanes per number in k_multiexp, 0 = by call size
  uint32_t rsav_lanes = 0;            // experiment knob (BFTKV_RSAV_LANES = 4 | 8): lanes per signature in k_rsav_verify, 0 = by call size
  uint32_t dsa_inv_mode = 0;          // experiment knob (BFTKV_DSA_INV = single | batched): 1 / 2, 0 = by batch shape
  bool psign_caller_order = false;    // experiment knob (BFTKV_PSIGN_ORDER = caller): k_psign_pow's chains as submitted, not longest first
  uint32_t n_cus = 256;               // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  uint32_t lagrange_x_bound = 0;      // bftkv_gpu_set_lagrange_x_bound: device-resident callers promise 0 <= x <= bound (0: no promise)
  bool early_exit = true;              // CollectiveSignature.Verify stops verifying where the reference stops reading (bftkv_gpu_set_early_exit)
  std::vector<DevBuf*> scratch_pool;   // threshold entry points' temporaries (threshold_capi.inc)
  std::unordered_map<std::string, std::vector<uint32_t>> modrow_cache;   // ... and the host-computed rows of ONE modulus (n, R^2, -n^-1, R_wide^2), by its bytes
  std::unordered_map<std::string, std::vector<uint32_t>> rsav_row_cache[2];   // RSA verification: n and R^2 mod n of ONE modulus by its bytes, [0] 72 limbs of 29 bits, [1] 80 of 28
  std::map<std::string, std::array<DevBuf, 4>> modtab_cache;   // Montgomery tables of the threshold entry points, by modulus bytes
  uint32_t* h_mail = nullptr;          // pinned + mapped: [0] packet count of the call in flight (k_scan_counts)
  uint32_t* d_mail = nullptr;
  uint32_t last_total = 0, last_rsa = 0, last_items = 0;
  bool last_total_on_dev = false;      // the last call was sized by an upper bound: its packet count is c->total[0] on the device
  bool have_plan_report = false;       // the last call was a resident big call under a plan: what it launched (bftkv_gpu_last_plan_report)
  uint32_t last_plan_report[plan_report::N_SLOTS] = {};
  hipEvent_t ev[10] = {};  // 0 start, 1 parsed, 2 modexp done (a big call sized by the plan's report: without its pass over long values), 3 compare + DSA done, 4 end, 5 hash start, 6 hash done, 7 DSA inverses done, 8 compare done,
                           // 9 modexp about to start (behind the turnstile)
  hipEvent_t ev_turn = nullptr;   // this context's ticket in the device's modexp turnstile (below)
  bool have_timing = false;
  void* rccl_comm = nullptr;   // ncclComm_t
  int n_ranks = 1, rank = 0;

  // Forked verifier contexts (bftkv_gpu_ctx_fork): own streams, arena, events and mailbox -- several device calls in flight at
  // once -- over the ROOT's resident key table, DSA tables and quorum descriptors.  A fork holds root->kt_rw SHARED for the
  // length of a device call; whatever changes the key table or the quorums (root only) holds it exclusively, i.e. waits until
  // the forks' calls in flight have drained and keeps new ones out.  A fork never takes the root's `mu`.
  bftkv_gpu_ctx* root = nullptr;            // null: this context is a root
  std::shared_mutex kt_rw;                  // root
  std::atomic<int> kt_writers{0};           // root: writers waiting or inside (forks stand back: pthread rwlocks prefer readers)
  std::atomic<int> n_forks{0};              // root: live forks (bftkv_gpu_destroy of the root refuses while > 0)
  uint64_t quorum_gen = 0;                  // root: bumped by quorum_create / quorum_destroy
  uint64_t seen_keyring_gen = ~0ull, seen_quorum_gen = ~0ull;   // fork: what its copies reflect
  size_t n_dsa_slots = 0;                   // fork: root->dsa_comb_slot.size() at the last refresh
  int kt_read_depth = 0;                    // fork: nesting of KtRead (under the fork's own lock)
  // staged small calls (the micro-batcher): one pinned staging buffer in, results written by the last kernel straight into
  // mapped host memory, completion = h_mail[1] reaching the call's sequence number
  DevBuf in_pack;
  uint8_t* h_out = nullptr; uint8_t* d_out = nullptr; size_t out_cap = 0;
  uint32_t out_seq = 0;
  // Pipelined host-buffer calls (bftkv_gpu_collective_verify on a big batch, see collective_verify_pipelined): the batch is cut
  // into pieces, each verified by a private worker context (own arena, streams, mailbox) over the ONE copy of the input this
  // context holds, while the pieces behind it are still crossing PCIe on stream_c.
  std::vector<bftkv_gpu_ctx*> hb_workers;   // private forks of the root (never handed out)
  hipStream_t stream_c = nullptr;           // host-to-device copies of the pieces, in order
  hipStream_t stream_c2 = nullptr;          // direct copies: a second helper thread and stream, so that the next range is already
                                            // in the runtime's hands when one completes (a pageable copy call returns when it is done)
  std::vector<hipEvent_t> hb_ev;            // [2k] signature streams of piece k on the device, [2k + 1] its payloads
  uint8_t* hb_out = nullptr; size_t hb_out_cap = 0;   // pinned: per-piece results land here, copied to the caller after the last sync
  // Unused dynamic LDS added to every 4-lane k_rsa_modexp launch of this context: 36.9 KB (18 x 4 at 2^29; 19 x 4: 38.9 KB) + pad > 53 KB leaves room for two blocks
  // per CU instead of three, i.e. 2 waves per SIMD and 192 of the 512 VGPRs free -- room in which the walk / parse / hash / tally
  // kernels of OTHER calls (or pieces) start at once instead of waiting for a round of modexp blocks to retire.
  uint32_t modexp_lds_pad = 0;
  uint32_t hb_pieces = 0;                   // bftkv_gpu_set_host_pipeline: 0 = by call size, 1 = never split, N = N pieces
  hipEvent_t hb_ev0 = nullptr;              // recorded on stream_c at the start of a pipelined call
  bool hb_tight = false;                    // tests: pieces sized by a bound real streams exceed (BFTKV_HOST_PIPELINE_TIGHT_BOUND)
  uint32_t hb_copy_mode = 0;                // 0: $BFTKV_HB_COPY or the pinned ring, 1: ring, 2: direct hipMemcpyAsync from the caller's memory
  void* hb_ring = nullptr;                  // HbRing: page-locked staging slots of the pipelined host-buffer path
  std::vector<float> hb_trace;              // last pipelined call: [pieces, ring?, copiers joined, copy stream drained, done, ...] + per piece
                                            // [ss enqueued, payload enqueued, piece picked up, payload hook, piece enqueued, piece drained] in us
  uint32_t hb_last_pieces = 0;              // > 0: the last verify call ran pipelined over that many workers (diagnostics read them)
  std::vector<uint32_t> hb_item0;           // first item of each piece of that call
  void* small_pin = nullptr;                // PinnedBuf[3] of bftkv_gpu_*_verify_small (batcher_capi.inc), created on first use
  uint32_t staged_spin_us = 50000;          // how long a staged call spins on its completion word before it blocks in the runtime (BFTKV_STAGED_SPIN_US)
};

void rccl_release(bftkv_gpu_ctx* c);
void release_small_pin(bftkv_gpu_ctx* c);
extern "C" int signature_verify_entities(bftkv_gpu_ctx* c, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off, const uint8_t* sig,
                                         const uint64_t* sig_off, const uint32_t* ent, uint8_t* err_out, const uint8_t* sig_class = nullptr,
                                         uint8_t* fenced_out = nullptr, const uint64_t* forced_issuer = nullptr);

namespace {

int fork_refresh(bftkv_gpu_ctx* c);

// Exclusive access to the key table / quorum descriptors / key sets (KeySets) of a root context (see bftkv_gpu_ctx::root).
struct KtWrite {
  bftkv_gpu_ctx* c;
  explicit KtWrite(bftkv_gpu_ctx* c_) : c(c_) { c->kt_writers.fetch_add(1); c->kt_rw.lock(); }
  ~KtWrite() { c->kt_rw.unlock(); c->kt_writers.fetch_sub(1); }
};
// Shared access for the length of one device call of a FORK (a no-op on a root: its calls and its writers are serialised by
// the context lock); brings the fork's copies of the key-table view and the quorum descriptors up to date first.
// Constructed with the fork's own lock held; nests (the entry points call one another).
struct KtRead {
  bftkv_gpu_ctx *c, *r;
  int rc = 0;
  explicit KtRead(bftkv_gpu_ctx* c_) : c(c_), r(c_->root) {
    if (!r || c->kt_read_depth++ > 0) return;
    while (r->kt_writers.load(std::memory_order_acquire) > 0) std::this_thread::yield();
    r->kt_rw.lock_shared();
    rc = fork_refresh(c);
  }
  ~KtRead() { if (r && --c->kt_read_depth == 0) r->kt_rw.unlock_shared(); }
};

// The modexp turnstile of a device.  A resident batch's k_rsa_modexp fills every SIMD for milliseconds; everything else of a
// call (walk, parse, plan; compare, tallies, exchange) is short and leaves most of the machine idle.  When several contexts have
// calls in flight, two such modexps launched side by side share the machine AND their heads and tails coincide -- the overlap
// that was wanted (one call's head and tail under the other's modexp) is lost as soon as the calls drift into step.  So the big
// modexps take turns: each waits (on its stream, not on the host) for the one before it, whichever context launched that.
// Calls too small to fill the machine (staged small calls, batches below TURNSTILE_MIN_PACKETS) do not queue here.
struct Turnstile { std::mutex mu; hipEvent_t last = nullptr; const void* owner = nullptr; };
Turnstile g_turnstile[16];
// host-buffer pipeline (collective_verify_pipelined)
constexpr uint64_t HB_PIPE_MIN_BYTES = 24ull << 20;      // below this a call is latency-, not PCIe-bound: one piece
constexpr uint32_t HB_PIPE_MAX_PIECES = 8;
std::mutex g_hb_mu[16];           // per device: pipelined host-buffer calls take turns (collective_verify_pipelined)
constexpr size_t HB_TR = 10;      // floats per piece in the timeline (bftkv_gpu_host_pipeline_trace)
// The caller's memory is pageable.  hipMemcpyAsync from it either pins the pages in place (the runtime caches such pins: fast
// for a buffer it has seen, ~17 GB/s for a fresh one, profiles/r04_h2d_rates_microbench.txt) and returns only when the copy is
// done.  The ring does not depend on that cache: helper threads memcpy chunk after chunk into page-locked slots (one thread
// moves ~30 GB/s, three outrun PCIe) and hand each slot to the DMA engine as a truly asynchronous copy; a slot is reused when
// the event behind its copy has fired.  Chunks are enqueued in plan order (a ticket), so the event recorded behind the last
// chunk of a range says the whole range -- and every range before it -- is on the device.
struct HbRing {
  static constexpr size_t SLOT = 16u << 20;     // (4 MB slots: ~45 GB/s, the per-copy cost shows; 16 MB: 54 of the 57 GB/s one copy reaches)
  static constexpr int NSLOT = 6;
  static constexpr int THREADS = 4;
  uint8_t* base = nullptr;
  hipEvent_t ev[NSLOT] = {};
  bool used[NSLOT] = {};
  ~HbRing() { if (base) (void)hipHostFree(base); for (auto e : ev) if (e) (void)hipEventDestroy(e); }
  hipError_t init() {
    if (base) return hipSuccess;
    hipError_t e = hipHostMalloc((void**)&base, SLOT * NSLOT, hipHostMallocDefault);
    if (e != hipSuccess) { base = nullptr; return e; }
    for (auto& x : ev) if ((e = hipEventCreateWithFlags(&x, hipEventDisableTiming)) != hipSuccess) return e;
    return hipSuccess;
  }
};


constexpr uint32_t TURNSTILE_MIN_PACKETS = 98304;     // two rounds of 768 resident blocks x 64 signatures

// live contexts: lets long-lived host objects (bftkv_quorum) notice that their context is gone
std::mutex g_live_mu;
std::vector<bftkv_gpu_ctx*> g_live;
bool ctx_is_live(bftkv_gpu_ctx* c) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  for (auto* p : g_live) if (p == c) return true;
  return false;
}

int fail(bftkv_gpu_ctx* c, int rc, const char* what, hipError_t e = hipSuccess) {
  char buf[512];
  if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else snprintf(buf, sizeof buf, "%s", what);
  c->err = buf;
  return rc;
}

#define HIPCHK(c, call)                                                    \
  do {                                                                     \
    hipError_t _e = (call);                                                \
    if (_e != hipSuccess) return fail((c), BFTKV_E_DEVICE, #call, _e);     \
  } while (0)

// The handles of one kind of resident key set (EcKeySet, DsaKeySet, RsaKeySet; a handle space per kind: handle 0 of one kind has
// nothing to do with handle 0 of another).  Sets live on the ROOT context like quorums: made and retired there under KtWrite (the
// forks' calls in flight drain first), read by the forks under KtRead without a copy.  Every entry below is called with c->mu held.
template <typename Set>
struct KeySets {
  // caller holds, on a fork, the root's key-table lock (KtRead) for as long as it uses the set
  static const Set* find(const bftkv_gpu_ctx* c, int h) {
    const std::vector<Set>& keysets = std::get<std::vector<Set>>((c->root ? c->root : c)->keysets);
    return h >= 0 && (size_t)h < keysets.size() && keysets[h].live ? &keysets[h] : nullptr;
  }
  static int bad_handle(bftkv_gpu_ctx* c) { return fail(c, BFTKV_E_INVALID, (std::string("bad ") + Set::kind + " key set handle").c_str()); }
  static int nomem(bftkv_gpu_ctx* c) {
    (void)hipGetLastError();
    return fail(c, BFTKV_E_NOMEM, (std::string(Set::kind) + " key set: device allocation failed").c_str());
  }
  // build(Set&) fills a new set on c->stream.  A failed build leaves nothing behind: whatever it queued on the set's buffers (copies,
  // memsets, table kernels) is drained, THEN they are freed.  A built set takes the lowest dead handle, or a new one.
  template <typename Build>
  static int create(bftkv_gpu_ctx* c, int* handle_out, Build&& build) {
    if (c->root) return fail(c, BFTKV_E_STATE, (std::string(Set::kind) + " key sets are created on the root context; its forks see them").c_str());
    HIPCHK(c, hipSetDevice(c->device));
    Set ks;
    if (const int rc = build(ks)) {
      (void)hipStreamSynchronize(c->stream);
      ks.release();
      return rc;
    }
    ks.live = true;
    std::vector<Set>& all = std::get<std::vector<Set>>(c->keysets);
    auto slot = std::find_if(all.begin(), all.end(), [](const Set& s) { return !s.live; });
    KtWrite kw(c);
    if (slot == all.end()) slot = all.emplace(all.end());
    *slot = std::move(ks);
    *handle_out = (int)(slot - all.begin());
    return 0;
  }
  static int retire(bftkv_gpu_ctx* c, int h) {
    if (c->root) return fail(c, BFTKV_E_STATE, (std::string(Set::kind) + " key sets are destroyed on the root context").c_str());
    if (!find(c, h)) return bad_handle(c);
    HIPCHK(c, hipSetDevice(c->device));
    KtWrite kw(c);
    HIPCHK(c, hipDeviceSynchronize());          // (_dev calls return before their kernels have run: nothing may still read the set)
    Set& ks = std::get<std::vector<Set>>(c->keysets)[h];
    ks.release();
    ks = Set();
    return 0;
  }
};
// bftkv_gpu_destroy
void keysets_release_all(bftkv_gpu_ctx* c) {
  std::apply([](auto&... of_kind) { (std::for_each(of_kind.begin(), of_kind.end(), [](auto& ks) { ks.release(); }), ...); }, c->keysets);
}

template <typename Set>
int ModRows::copy_from(bftkv_gpu_ctx* c, const ModTab& src, size_t n_rows, bool with_wide) {
  const void* from[4] = {src.n_limbs, src.r2_limbs, src.n0inv, src.r2w_limbs};
  const size_t len[4] = {n_rows * MONT_N * 4, n_rows * MONT_N * 4, n_rows * 4, n_rows * MONT_N_WIDE * 4};
  for (int k = 0; k < (with_wide ? 4 : 3); ++k) {
    // (the one-row form with the wide row keeps ensure()'s slack, the per-group form is exact: as each was before they met here)
    if ((with_wide ? b[k].ensure(len[k]) : b[k].ensure_exact(len[k])) != hipSuccess) return KeySets<Set>::nomem(c);
    HIPCHK(c, hipMemcpyAsync(b[k].p, from[k], len[k], hipMemcpyDeviceToDevice, c->stream));
  }
  return 0;
}

template <typename T>
int upload(bftkv_gpu_ctx* c, DevBuf& b, const std::vector<T>& v) {
  size_t bytes = v.size() * sizeof(T);
  HIPCHK(c, b.ensure(bytes ? bytes : 16));
  if (bytes) HIPCHK(c, hipMemcpyAsync(b.p, v.data(), bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}

int build_member(bftkv_gpu_ctx* c, QuorumHost& q) {
  if (q.keyring_gen == c->keyring_gen && q.member.p) return 0;
  std::vector<uint8_t> m((size_t)q.n_qcs * (c->n_entities ? c->n_entities : 1), 0);
  for (int qc = 0; qc < q.n_qcs; ++qc)
    for (uint32_t e = 0; e < c->n_entities; ++e)
      for (uint64_t id : q.nodes[qc])
        if (id == c->h_entity_id[e]) { m[(size_t)qc * c->n_entities + e] = 1; break; }
  int rc = upload(c, q.member, m);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  q.keyring_gen = c->keyring_gen;
  return 0;
}

QuorumDev quorum_dev(const bftkv_gpu_ctx* c, const QuorumHost& q) {
  QuorumDev d{};
  d.n_qcs = q.n_qcs;
  for (int i = 0; i < q.n_qcs; ++i) { d.f[i] = q.f[i]; d.min[i] = q.mn[i]; d.threshold[i] = q.thr[i]; d.suff[i] = q.suff[i]; }
  d.member = q.member.as<uint8_t>();
  d.n_entities = c->n_entities;
  return d;
}

// per-item fold of Signature.Verify semantics (crypto_pgp.go:319-330)
__global__ void k_sigverify_fold(const SigRec* __restrict__ recs, const uint32_t* __restrict__ base,
                                 const uint32_t* __restrict__ counts, const uint8_t* __restrict__ item_flags,
                                 uint32_t n_items, uint8_t* __restrict__ err_out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  uint32_t n_ok = 0;
  bool bad = false;
  for (uint32_t k = 0; k < counts[i]; ++k) {
    uint8_t st = recs[base[i] + k].status;
    if (st == ST_OK) ++n_ok;
    else if (st != ST_UNKNOWN_ISSUER) bad = true;
  }
  // a final call that only skips packets (unknown issuers / unknown packet types) runs into EOF
  // and returns ErrUnknownIssuer
  if (item_flags[i] & 1) bad = true;
  if (counts[i] && recs[base[i] + counts[i] - 1].status == ST_UNKNOWN_ISSUER) bad = true;
  err_out[i] = (!bad && n_ok >= 1) ? BFTKV_ERR_NONE : BFTKV_ERR_INVALID_SIGNATURE;
}

// quorum predicates over explicit node-id lists: one wave per list (wotqs.go:144-206)
__global__ void __launch_bounds__(256) k_tally_ids(const uint64_t* __restrict__ ids, const uint64_t* __restrict__ list_off,
                                                   uint32_t n_lists, const uint64_t* __restrict__ qc_ids,
                                                   const uint32_t* __restrict__ qc_off, QuorumDev q,
                                                   uint8_t* __restrict__ verdict) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  if (wave >= n_lists) return;
  uint32_t cq[MAX_QC];
#pragma unroll
  for (int c = 0; c < MAX_QC; ++c) cq[c] = 0;
  const uint64_t lo = list_off[wave], hi = list_off[wave + 1];
  for (uint64_t off = lo; off < hi; off += 64) {
    const bool in = off + lane < hi;
    const uint64_t id = in ? ids[off + lane] : 0;
#pragma unroll
    for (int c = 0; c < MAX_QC; ++c) {
      if (c < q.n_qcs) {
        bool mem = false;
        if (in)
          for (uint32_t k = qc_off[c]; k < qc_off[c + 1]; ++k)
            if (qc_ids[k] == id) { mem = true; break; }
        cq[c] += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mem));
      }
    }
  }
  if (lane == 0) {
    bool is_quorum = q.n_qcs > 0, is_thr = q.n_qcs > 0, is_suff = false, reject = true;
    for (int c = 0; c < q.n_qcs; ++c) {
      if (q.f[c] > 0 && (int32_t)cq[c] < q.min[c]) is_quorum = false;
      if (q.threshold[c] > 0 && (int32_t)cq[c] < q.threshold[c]) is_thr = false;
      if (q.suff[c] > 0 && (int32_t)cq[c] >= q.suff[c]) is_suff = true;
      if (q.f[c] == 0 || (int32_t)cq[c] <= q.f[c]) reject = false;
    }
    verdict[wave] = (is_quorum ? V_IS_QUORUM : 0) | (is_thr ? V_IS_THRESHOLD : 0) | (is_suff ? V_IS_SUFFICIENT : 0) |
                    (reject ? V_REJECT : 0);
  }
}

// What a caller asks of run_pipeline, by name.  A call is a combination of these, not one of N kinds; fields left alone: a
// resident call that verifies every packet of every item against the node keyring.
struct PipelineCall {
  uint32_t n_items = 0;
  const uint8_t* d_tbs = nullptr; const uint64_t* d_tbs_off = nullptr;      // the signed payloads and their [n_items + 1] offsets
  const uint8_t* d_ss = nullptr; const uint64_t* d_ss_off = nullptr;        // the signature streams, likewise
  uint64_t ss_len = 0;                        // bytes of d_ss (0: not known): sizes the walk's scratch row and a staged call's arena
  const uint32_t* d_cert_ent = nullptr;       // per item or null: the one entity whose keys may verify it (ParseArgs::cert_ent)
  const uint8_t* d_sig_class = nullptr;       // per item or null: the certificate check the item is (ParseArgs::sig_class)
  const uint64_t* d_forced_issuer = nullptr;  // per item or null, with d_sig_class: the key the caller holds (ParseArgs::forced_issuer)
  const uint32_t* d_msg_slot = nullptr;       // transport messages: per item the sender's slot and the hash its signature names
  const uint8_t* d_msg_hash = nullptr;        // (ParseArgs::msg_slot, msg_hash)
  // upload_tbs (host-buffer entry point): the signed payloads are still in host memory.  Only the hash stream reads them,
  // so their copy is issued on that stream AFTER the modexp has been launched and runs beside it; the signature stream
  // (which the walk, the parse and the modexp need) was copied before the call.
  const std::function<int(hipStream_t)>* upload_tbs = nullptr;
  // mid_prelaunched (pieces of a pipelined host-buffer call): the caller has already put k_sha256_mid for these items on the
  // hash stream -- when the payloads arrived, ahead of the signature streams -- so the chain of 134 dependent compressions per
  // payload is under way before the piece is picked up.
  bool mid_prelaunched = false;
  // ev_input (pipelined host-buffer calls): the signature streams and offsets of this call are still being copied by another
  // stream; the main stream waits for that event first (the hash stream joins the main stream's start, so it waits too).
  hipEvent_t ev_input = nullptr;
  // plan_q (CollectiveSignature.Verify with the early exit enabled): public-key work is queued in two phases by k_plan
  // instead of by the parse -- see kernels.hip "two-phase planning".
  const QuorumDev* plan_q = nullptr;
  // d_mid_in / d_tbs_prefix (the micro-batcher, whose callers absorb the whole blocks of their payload on their own threads):
  // SHA-256 midstates [n_items][8] and the byte counts behind them; d_tbs then holds only the < 64 bytes after each.  No
  // payload hashing on the device; a signature that asks for another hash stays ST_PENDING_HASH (the caller re-submits
  // such an item with its payload: k_fenced_out's rehash bit).
  const uint32_t* d_mid_in = nullptr; const uint64_t* d_tbs_prefix = nullptr;
  // staged_cap (staged small calls): the arena and the grids are sized for that many packet events up front and the
  // kernels read the real count from the device -- no host round trip in mid-pipeline; a call with more events turns
  // itself into an empty one (k_scan_counts) and is run again through the ordinary path by its caller.
  uint32_t staged_cap = 0;
};

constexpr uint32_t MAIL_EMPTY = 0xFFFFFFFFu;      // mailbox word 0 until the scan has written the packet count

// the buffers sized by the item count (before the packet count is known)
static int ensure_for_items(bftkv_gpu_ctx* c, const PipelineCall& call, uint32_t walk_cap, TextDev* txt) {
  const size_t n_items = call.n_items;
  HIPCHK(c, c->counts.ensure(sizeof(uint32_t) * (n_items + 1)));
  HIPCHK(c, c->base.ensure(sizeof(uint32_t) * (n_items + 1)));
  HIPCHK(c, c->total.ensure(16));
  HIPCHK(c, c->item_flags.ensure(n_items + 16));
  HIPCHK(c, c->walk_scratch.ensure(sizeof(WalkEnt) * walk_cap * n_items + 16));
  HIPCHK(c, c->mid.ensure(sizeof(uint32_t) * 8 * N_MID32 * n_items + 16));      // SHA-256 | SHA-224 | SHA-1 | MD5 | RIPEMD-160 midstates
  HIPCHK(c, c->mid64.ensure(sizeof(uint64_t) * 8 * 2 * n_items + 16));   // SHA-512 | SHA-384
  HIPCHK(c, c->hash_mask.ensure(sizeof(uint32_t) * n_items + 16));
  // partial-length signature packets are linearised into this arena by the parse; the walk reports how much the call needs
  // (mailbox word 2) and a staged call, which does not ask the host in mid-pipeline, lives with the minimum (beyond it: fenced)
  constexpr size_t CHUNK_ARENA_MIN = 64u << 10;
  if (!c->chunk_ctr.p) { HIPCHK(c, c->chunk_ctr.ensure(16)); HIPCHK(c, hipMemsetAsync(c->chunk_ctr.p, 0, 16, c->stream)); }
  HIPCHK(c, c->chunk_arena.ensure(CHUNK_ARENA_MIN + (call.staged_cap ? 2 * (size_t)call.ss_len : 0)));
  HIPCHK(c, c->pk_count.ensure(sizeof(uint32_t) * PK_COUNT_WORDS));
                                       // [0..3] work-list lengths, [4] some signature uses a hash other than SHA-256,
                                       // [5] some RSA value is too long for the 29-bit form (SIGF_WIDE_VALUE),
                                       // [8..11] lengths after phase 1 (phase 2's start), [12..15] zeros (phase 1's start),
                                       // [16..19] two uint64: clock stamps of k_rsa_modexp (bftkv_gpu_last_sclk_mhz),
                                       // [20..23] DSA class counts (k_dsa_split), [24] k_plan<1>'s ticket (PK_PLAN_TICKET)
  if (call.plan_q) HIPCHK(c, c->plan_cut.ensure(sizeof(uint32_t) * n_items + 16));
  *txt = TextDev{nullptr, nullptr, nullptr, nullptr};
  if (!call.d_mid_in) {      // (a midstate-only call cannot hash text-mode signatures: their items come back marked for the ordinary path)
    HIPCHK(c, c->txt_mid32.ensure(sizeof(uint32_t) * 8 * N_MID32 * n_items + 16));
    HIPCHK(c, c->txt_mid64.ensure(sizeof(uint64_t) * 8 * N_MID64 * n_items + 16));
    HIPCHK(c, c->txt_tail.ensure((size_t)128 * N_HASHES * n_items + 16));
    HIPCHK(c, c->txt_len.ensure(sizeof(uint64_t) * N_HASHES * n_items + 16));
    *txt = TextDev{c->txt_mid32.as<uint32_t>(), c->txt_mid64.as<uint64_t>(), c->txt_tail.as<uint8_t>(), c->txt_len.as<uint64_t>()};
  }
  return 0;
}

// ... and those sized by the packet count (`tr`: at least 1)
static int ensure_for_packets(bftkv_gpu_ctx* c, size_t tr) {
  HIPCHK(c, c->recs.ensure(sizeof(SigRec) * tr));
  HIPCHK(c, c->digests.ensure(sizeof(uint32_t) * 16 * tr));
  HIPCHK(c, c->r.ensure(sizeof(uint32_t) * EM_LOW_LIMBS * tr));   // low limbs of s^e mod n: k_rsa_modexp -> k_rsa_compare
  HIPCHK(c, c->xr.ensure(sizeof(uint32_t) * (c->have_rsa4096 ? MONT_NMAX : c->have_rsa3072 ? MONT_TPI_BIG * MONT_L3072 : 80) * tr));   // 80: the <10, 8> form
  HIPCHK(c, c->pk_list.ensure(sizeof(uint32_t) * tr));
  HIPCHK(c, c->pk_list3072.ensure(c->have_rsa3072 ? sizeof(uint32_t) * tr : 16));
  HIPCHK(c, c->pk_list4096.ensure(c->have_rsa4096 ? sizeof(uint32_t) * tr : 16));
  if (c->have_rsa3072) HIPCHK(c, c->r3072.ensure(sizeof(uint32_t) * EM_LOW_LIMBS * tr));
  if (c->have_rsa4096) HIPCHK(c, c->r4096.ensure(sizeof(uint32_t) * EM_LOW_LIMBS * tr));
  HIPCHK(c, c->dsa_list.ensure(sizeof(uint32_t) * tr));
  if (c->have_dsa_keys) HIPCHK(c, c->dsa_u.ensure(sizeof(uint32_t) * DSA_U_WORDS * tr));
  if (c->have_dsa3072 && c->have_dsa2048) HIPCHK(c, c->dsa_idx.ensure(sizeof(uint32_t) * 4 * tr + 16));      // k_dsa_split: two class lists per phase
  return 0;
}

// What the scan found, for a call that asks the host: from the mailbox, or read back when there is none or it stays empty.
struct PacketCount { uint32_t total, chunk_units, overflow_items; bool mailed; };
static int read_packet_count(bftkv_gpu_ctx* c, hipStream_t s, PacketCount* pk) {
  pk->total = MAIL_EMPTY;
  if (c->h_mail) {
    // spin on the mailbox (a few microseconds after the scan retires); give up after 20 ms and synchronise
    const auto t_spin = std::chrono::steady_clock::now();
    for (uint32_t it = 0;; ++it) {
      pk->total = __atomic_load_n(&c->h_mail[0], __ATOMIC_ACQUIRE);
      if (pk->total != MAIL_EMPTY) break;
      if ((it & 1023u) == 1023u && std::chrono::steady_clock::now() - t_spin > std::chrono::milliseconds(20)) break;
      __builtin_ia32_pause();
    }
  }
  pk->mailed = pk->total != MAIL_EMPTY;
  if (pk->mailed) {
    pk->chunk_units = c->h_mail[2];
    pk->overflow_items = c->h_mail[plan_report::MAIL_OVERFLOW];      // (written ahead of the packet count)
  } else {
    HIPCHK(c, hipMemcpyAsync(&pk->total, c->total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&pk->chunk_units, c->chunk_ctr.as<uint32_t>() + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  return 0;
}

// Wait a moment for k_plan<1>'s flags word (into rin->flags_word; 0: not there at the deadline).  By now the machine-filling
// modexp is in the queue, so a host that waits for that word delays nothing.
// lengths_too (a call sized by the report): also for the four list lengths, which the plan's LAST block sends -- under the same
// deadline.  What that costs: the flags word leaves with the plan's first block, the lengths with its last, so the calling thread
// spins for the plan's own duration more than it did, and beside a neighbour's modexp, where the plan is starved for block slots,
// usually to the deadline (cfg 2, three in flight: 0.57 ms per call, the lengths in time in 5 calls of 28; docs/history.md
// 2026-10-21).  Nothing tells the host sooner that the plan is complete: the lengths are that signal.  The hash stream's work
// needs the flags word alone: on_flags enqueues it the moment the word is read, or at the deadline without it.
template <class F>
static int wait_for_plan_words(bftkv_gpu_ctx* c, uint32_t total, bool lengths_too, plan_report::Input* rin, F&& on_flags) {
  const auto t_spin = std::chrono::steady_clock::now();
  bool hashed = false;
  int rc;
  for (uint32_t it = 0;; ++it) {
    const uint32_t v = __atomic_load_n(&c->h_mail[plan_report::MAIL_PLAN_FLAGS], __ATOMIC_ACQUIRE);
    if (v) {
      rin->flags_word = v;
      if (!lengths_too) break;
      if (!hashed) { if ((rc = on_flags())) return rc; hashed = true; }
      bool all = true;
      for (int k = 0; k < plan_report::N_LISTS; ++k) {
        rin->len_word[k] = __atomic_load_n(&c->h_mail[plan_report::MAIL_LEN0 + k], __ATOMIC_ACQUIRE);
        all = all && rin->len_word[k] != 0;
      }
      if (all) break;
    }
    // (the parse and the plan of a big batch take milliseconds themselves: ~0.1 ns per packet each, more beside a neighbour's modexp)
    if ((it & 255u) == 255u && std::chrono::steady_clock::now() - t_spin > std::chrono::microseconds(300) + std::chrono::nanoseconds((uint64_t)total / 2)) break;
    __builtin_ia32_pause();
  }
  return lengths_too && !hashed ? on_flags() : 0;
}

// Shared pipeline.  Main stream: walk -> parse -> RSA modexp -> compare.  Hash stream (forked after
// the parse): SHA-256 midstates -> per-signature digests; joined before the compare.  Leaves SigRec
// statuses final.
int run_pipeline(bftkv_gpu_ctx* c, const PipelineCall& call) {
  const uint32_t n_items = call.n_items, staged_cap = call.staged_cap;
  const uint8_t* const d_tbs = call.d_tbs; const uint64_t* const d_tbs_off = call.d_tbs_off;
  const uint8_t* const d_ss = call.d_ss; const uint64_t* const d_ss_off = call.d_ss_off;
  const uint32_t* const d_mid_in = call.d_mid_in;
  const QuorumDev* const plan_q = call.plan_q;
  // What this call is, in one place (`big` and what follows from it: below, once the packet count is known).
  // staged: sized up front for staged_cap packet events, it never asks the host for its packet count.
  const bool staged = staged_cap != 0;
  // A staged small call keeps its hashing on the main stream: its digest kernel is a few microseconds, two cross-stream joins
  // cost more than that, and a lane that occupies ONE hardware queue leaves the others to the other lanes (the runtime maps
  // streams onto 4 queues by default: three streams per lane made four lanes run one after the other).
  // (a capped call that waits for its input on an event is a PIECE of a pipelined host-buffer call: big, so it keeps the side
  // streams and the turnstile of a resident batch, and like a staged call it never asks the host for its packet count)
  const bool one_stream = staged && !call.ev_input;
  // hashes_payloads: the payloads are on the device (or on their way: upload_tbs); false: the caller sent midstates instead
  const bool hashes_payloads = !d_mid_in;
  // A staged call with few signatures (no SIMD would get a second wave either way) spreads every <= 2048-bit number over
  // eight lanes: 0.68x the instructions per wave, and such a call lasts as long as ONE wave's chain of 18 products.
  static const bool wide8_off = getenv("BFTKV_NO_WIDE8") != nullptr;
  const bool wide8 = staged && call.ss_len / 256 <= 8192 && !wide8_off;
  // BFTKV_PLAN_REPORT=0: the device's words are ignored, and a resident big call is enqueued as every other call is
  static const bool report_on = []{ const char* e = getenv("BFTKV_PLAN_REPORT"); return !(e && atoi(e) == 0); }();
  static const bool turnstile_off = getenv("BFTKV_NO_TURNSTILE") != nullptr;      // (read once: this is every big call's path)
  // s^-1 mod q: one extended GCD per run of signatures under one key (k_dsa_inv_batched) when the DSA work list gives every
  // key of the ring enough of them (64 on average, 4096 in all: a thread's 16 sorted entries then hold one or two runs), else
  // one per signature (k_dsa_inv).  The list length lives on the device, so both kernels are enqueued and one of them returns
  // at once.
  const size_t n_slots = c->root ? c->n_dsa_slots : c->dsa_comb_slot.size();
  const uint32_t inv_batch_min = c->dsa_inv_mode == 1 || n_slots > (c->dsa_inv_mode == 2 ? (size_t)INV_MAX_SLOTS : 256) ? 0xFFFFFFFFu
                                 : c->dsa_inv_mode == 2 ? 0u : (uint32_t)std::max<size_t>(4096, 64 * n_slots);

  hipStream_t s = c->stream, sh = one_stream ? c->stream : c->stream_h;
  auto rec = [&](int k, hipStream_t st) -> hipError_t { return one_stream ? hipSuccess : hipEventRecord(c->ev[k], st); };
  auto join = [&](hipStream_t st, int k) -> hipError_t { return one_stream ? hipSuccess : hipStreamWaitEvent(st, c->ev[k], 0); };
  if (!c->ev[0]) for (auto& e : c->ev) HIPCHK(c, hipEventCreate(&e));
  // walk scratch row: sized from the average stream length (a packet event needs >= 2 stream bytes, a signature ~100..300);
  // items with more events than the row holds take the sequential fill pass
  const uint32_t walk_cap = call.ss_len ? (uint32_t)std::min<uint64_t>(WALK_CAP_MAX, std::max<uint64_t>(WALK_CAP_MIN, call.ss_len / n_items / 48)) : 96u;
  TextDev txt;
  int rc;
  if ((rc = ensure_for_items(c, call, walk_cap, &txt))) return rc;
  if (call.ev_input) HIPCHK(c, hipStreamWaitEvent(s, call.ev_input, 0));
  HIPCHK(c, rec(0, s));
  // the payload midstates do not depend on the parse: start them right away on the hash stream
  HIPCHK(c, join(sh, 0));
  HIPCHK(c, rec(5, sh));
  if (!call.upload_tbs && hashes_payloads)
    hipLaunchKernelGGL(k_sha256_mid, dim3((n_items + MID_BLOCK - 1) / MID_BLOCK), dim3(MID_BLOCK), 0, sh, d_tbs, d_tbs_off, n_items, c->mid.as<uint32_t>());
  hipLaunchKernelGGL(k_walk<false>, dim3(n_items), dim3(64), 0, s, d_ss, d_ss_off, n_items, c->counts.as<uint32_t>(),
                     (const uint32_t*)nullptr, (SigRec*)nullptr, c->item_flags.as<uint8_t>(), c->walk_scratch.as<WalkEnt>(), walk_cap,
                     c->chunk_ctr.as<uint32_t>());
  if (c->h_mail && !staged) __atomic_store_n(&c->h_mail[0], MAIL_EMPTY, __ATOMIC_RELEASE);
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, c->counts.as<uint32_t>(), n_items, c->base.as<uint32_t>(),
                     c->total.as<uint32_t>(), staged ? (uint32_t*)nullptr : c->d_mail, c->pk_count.as<uint32_t>(), c->hash_mask.as<uint32_t>(),
                     staged_cap, c->chunk_ctr.as<uint32_t>(), staged ? (const uint8_t*)nullptr : c->item_flags.as<uint8_t>(), walk_cap);
  PacketCount pk{staged_cap, 0u, 0u, false};      // staged: the upper bound; the kernels read the count from c->total
  if (!staged && (rc = read_packet_count(c, s, &pk))) return rc;
  const uint32_t total = pk.total;
  const uint32_t* const n_recs_dev = staged ? c->total.as<uint32_t>() : nullptr;
  if (!staged && (size_t)pk.chunk_units * 16 > c->chunk_arena.cap) HIPCHK(c, c->chunk_arena.ensure((size_t)pk.chunk_units * 16));
  c->last_total = staged ? 0u : total;      // (per-packet diagnostics are not kept for staged calls)
  c->last_total_on_dev = staged && call.ev_input != nullptr;   // ... a piece's are: its count is read from the device when asked for
  c->last_items = n_items;
  c->hb_last_pieces = 0;
  if ((rc = ensure_for_packets(c, total ? total : 1))) return rc;
  // big: the call's modexp fills the machine, so it takes a turn at the turnstile (a piece is judged by its stream bytes)
  const bool big = staged ? (call.ev_input != nullptr && call.ss_len / 320 >= TURNSTILE_MIN_PACKETS) : total >= TURNSTILE_MIN_PACKETS;
  // waits_for_flags: a big call under a plan waits, once its modexp is queued, for the word that says whether any signature
  // named a hash other than SHA-256
  const bool waits_for_flags = total && hashes_payloads && plan_q && big && c->h_mail;
  // report_path: a resident big call under a plan sizes what it enqueues from here on by what the device reports
  // (plan_report.h): the scan's overflow count now, k_plan<1>'s words once the machine-filling modexp is in the queue; the
  // diagnostics getter describes such calls.  by_report: ... and the report is on.  Every other call is one with the report
  // disabled: grids over `total`, in the order below.
  const bool report_path = waits_for_flags && !staged && !call.upload_tbs;
  const bool by_report = report_path && report_on;
  // dsa: the call has a DSA side (inverses on their own stream, the table multiplications behind the digests)
  const bool dsa = total && c->have_dsa_keys;

  // The launch plan: every grid below comes from `dec` (0 blocks: not launched).
  plan_report::Input rin;
  rin.total = total; rin.n_items = n_items; rin.enabled = by_report;
  rin.overflow_arrived = pk.mailed; rin.overflow_items = pk.overflow_items;
  rin.wide_form = BFTKV_RSA_FORM == 29 && !wide8;
  rin.have_rsa3072 = c->have_rsa3072; rin.have_rsa4096 = c->have_rsa4096; rin.have_dsa2048 = c->have_dsa2048; rin.have_dsa3072 = c->have_dsa3072;
  rin.dsa_inv_batched = inv_batch_min != 0xFFFFFFFFu; rin.dsa_inv_single = inv_batch_min != 0u;
  plan_report::Geometry geo;      // (the kernels' own constants: a build with another block size sizes by that)
  geo.modexp4 = MODEXP_BLOCK / MONT_TPI; geo.modexp8 = MODEXP_BLOCK / MONT_TPI_BIG; geo.modexp_main = wide8 ? geo.modexp8 : geo.modexp4;
  geo.compare = 256 / CMP_LANES; geo.dsa_mul = 64; geo.dsa_split = 256; geo.dsa4 = QUADS_PER_BLOCK; geo.dsa8 = RSA_BLOCK / MONT_TPI_BIG;
  geo.inv_tile = INV_TILE; geo.mid_items = 64; geo.n_hashes = N_HASHES;
  plan_report::Decision dec = plan_report::decide(rin, geo);
  c->have_plan_report = false;
  // fill pass only for items whose event list overflowed the scratch (a no-op grid otherwise; not launched when the scan
  // reported that there are none)
  if (dec.walk_fill)
    hipLaunchKernelGGL(k_walk<true>, dim3(dec.walk_fill), dim3(64), 0, s, d_ss, d_ss_off, n_items, c->counts.as<uint32_t>(),
                       c->base.as<uint32_t>(), c->recs.as<SigRec>(), c->item_flags.as<uint8_t>(), (WalkEnt*)nullptr, walk_cap, (uint32_t*)nullptr);
  if (total) {
    ParseArgs pa;
    pa.sig_blob = d_ss; pa.sig_off = d_ss_off; pa.rec_base = c->base.as<uint32_t>(); pa.counts = c->counts.as<uint32_t>(); pa.n_items = n_items;
    pa.scratch = c->walk_scratch.as<WalkEnt>(); pa.walk_cap = walk_cap; pa.recs = c->recs.as<SigRec>(); pa.n_recs = total; pa.cert_ent = call.d_cert_ent;
    pa.pk_list = c->pk_list.as<uint32_t>(); pa.pk_list3072 = c->pk_list3072.as<uint32_t>(); pa.pk_list4096 = c->pk_list4096.as<uint32_t>();
    pa.pk_count = c->pk_count.as<uint32_t>(); pa.dsa_list = c->dsa_list.as<uint32_t>(); pa.item_hash_mask = c->hash_mask.as<uint32_t>();
    pa.sig_class = call.d_sig_class; pa.forced_issuer = call.d_forced_issuer; pa.msg_slot = call.d_msg_slot; pa.msg_hash = call.d_msg_hash;
    pa.item_flags = c->item_flags.as<uint8_t>();
    pa.defer_queue = plan_q ? 1u : 0u;
    pa.n_recs_dev = n_recs_dev;
    pa.chunk_arena = c->chunk_arena.as<uint8_t>(); pa.chunk_cap_units = (uint32_t)std::min<size_t>(c->chunk_arena.cap / 16, 0xFFFFFFF0u);
    pa.chunk_bump = c->chunk_ctr.as<uint32_t>() + 1;
    if (!staged && (uint64_t)total >= 128ull * n_items)     // very long items (n = 256 cliques: 171+ packets): block per item, no bisection
                                                 // (measured at 53 packets per item: 237 us item-major vs 210 us record-major)
      hipLaunchKernelGGL(k_parse_body_items, dim3(n_items), dim3(PARSE_ITEM_BLOCK), 0, s, pa, c->kt);
    else
      hipLaunchKernelGGL(k_parse_body, dim3((total + 255) / 256), dim3(256), 0, s, pa, c->kt);
  }
  uint32_t* const cnt_p = c->pk_count.as<uint32_t>();
  const uint32_t* const start0 = cnt_p + 12;        // phase 1 starts every work list at 0
  const uint32_t* const start1 = cnt_p + 8;         // phase 2: at the lengths after phase 1
  PlanArgs pl{};
  if (total && plan_q) {
    pl.recs = c->recs.as<SigRec>(); pl.rec_base = c->base.as<uint32_t>(); pl.counts = c->counts.as<uint32_t>(); pl.n_items = n_items;
    pl.pk_list = c->pk_list.as<uint32_t>(); pl.dsa_list = c->dsa_list.as<uint32_t>(); pl.pk_list3072 = c->pk_list3072.as<uint32_t>();
    pl.pk_list4096 = c->pk_list4096.as<uint32_t>(); pl.pk_count = cnt_p; pl.plan_cut = c->plan_cut.as<uint32_t>(); pl.verdict = nullptr;
    int min_suff = 0;
    for (int i = 0; i < plan_q->n_qcs; ++i) if (plan_q->suff[i] > 0 && (min_suff == 0 || plan_q->suff[i] < min_suff)) min_suff = plan_q->suff[i];
    pl.margin = 1u + (uint32_t)min_suff / 64u;
    pl.mail = c->d_mail ? c->d_mail + plan_report::MAIL_PLAN_FLAGS : nullptr;
    if (c->h_mail) {
      __atomic_store_n(&c->h_mail[plan_report::MAIL_PLAN_FLAGS], 0u, __ATOMIC_RELEASE);
      for (int k = 0; k < plan_report::N_LISTS; ++k) __atomic_store_n(&c->h_mail[plan_report::MAIL_LEN0 + k], 0u, __ATOMIC_RELEASE);
    }
    hipLaunchKernelGGL(k_plan<1>, dim3((n_items + PLAN_ITEMS - 1) / PLAN_ITEMS), dim3(PLAN_BLOCK), 0, s, pl, c->kt, *plan_q);
  }
  if (one_stream && dsa) HIPCHK(c, hipEventRecord(c->ev[1], s)); else HIPCHK(c, rec(1, s));
  auto launch_dsa_inv = [&](hipStream_t st, const uint32_t* start, const plan_report::PhaseGrids& pg) {
    if (pg.dsa_inv_batched)
      hipLaunchKernelGGL(k_dsa_inv_batched, dim3(pg.dsa_inv_batched), dim3(INV_BLOCK), 0, st, d_ss, c->recs.as<SigRec>(),
                         c->dsa_list.as<uint32_t>(), c->pk_count.as<uint32_t>(), start, c->kt, c->dsa_u.as<uint32_t>(), inv_batch_min);
    if (pg.dsa_inv)
      hipLaunchKernelGGL(k_dsa_inv, dim3(pg.dsa_inv), dim3(64), 0, st, d_ss, c->recs.as<SigRec>(), c->dsa_list.as<uint32_t>(),
                         c->pk_count.as<uint32_t>(), start, c->kt, c->dsa_u.as<uint32_t>(), inv_batch_min);
  };
  if (dsa) {
    HIPCHK(c, hipStreamWaitEvent(c->stream_d, c->ev[1], 0));
    launch_dsa_inv(c->stream_d, start0, dec.p1);
    HIPCHK(c, hipEventRecord(c->ev[7], c->stream_d));
  }
  auto hash_stream_work = [&]() -> int {
  // hash stream: digests need the parsed records
    HIPCHK(c, join(sh, 1));
    if (total) {
      // other hashes: a no-op grid unless some signature asked for them (not launched when the plan reported that none did)
      if (hashes_payloads && dec.mid_other) {
        hipLaunchKernelGGL(k_hash_mid_other, dim3(dec.mid_x, geo.n_hashes - 1), dim3(64), 0, sh, d_tbs, d_tbs_off, n_items,
                           c->hash_mask.as<uint32_t>(), c->mid.as<uint32_t>(), c->mid64.as<uint64_t>());
        hipLaunchKernelGGL(k_hash_mid_text, dim3(dec.mid_x, geo.n_hashes), dim3(64), 0, sh, d_tbs, d_tbs_off, n_items, c->hash_mask.as<uint32_t>(), txt);
      }
      hipLaunchKernelGGL(k_digest_sha256, dim3((total + 255) / 256), dim3(256), 0, sh, d_tbs, d_tbs_off, d_ss,
                         d_mid_in ? d_mid_in : c->mid.as<uint32_t>(), c->mid64.as<uint64_t>(), n_items, c->recs.as<SigRec>(), total,
                         c->digests.as<uint32_t>(), call.d_tbs_prefix, n_recs_dev);
    }
    HIPCHK(c, rec(6, sh));
    return 0;
  };
  // (by the report: behind the wait for the plan's words below -- this work waits for the plan on the device anyway)
  if (!call.upload_tbs && !by_report && (rc = hash_stream_work())) return rc;
  // main stream: modular exponentiations (status bytes are only written by the hash stream meanwhile)
  // the 19 x 4 form of 28 bits for the values too long for 72 limbs (262 .. 266 bytes; k_parse_body flags them and raises
  // cnt_p[5]): normally a grid of blocks that read one word and return
  auto launch_wide = [&](const uint32_t* start, uint32_t blocks) {
#if BFTKV_RSA_FORM == 29
    if (blocks)
      hipLaunchKernelGGL((k_rsa_modexp<MONT_L, MONT_TPI, MONT_W, true>), dim3(blocks), dim3(MODEXP_BLOCK), c->modexp_lds_pad, s, d_ss, c->recs.as<SigRec>(), c->pk_list.as<uint32_t>(),
                         cnt_p, start, c->kt, c->r.as<uint32_t>(), c->xr.as<uint32_t>(), (uint64_t*)nullptr, (const uint32_t*)(cnt_p + 5));
#else
    (void)start; (void)blocks;      // (never sized: Input::wide_form is false)
#endif
  };
  // wide_inline: the pass over the long values right behind the main pass, as every call has it but the one sized by the report
  auto launch_modexp = [&](const uint32_t* start, const plan_report::PhaseGrids& pg, bool wide_inline) {
    if (pg.modexp && wide8) {
      hipLaunchKernelGGL((k_rsa_modexp<10, MONT_TPI_BIG>), dim3(pg.modexp), dim3(MODEXP_BLOCK), 0, s, d_ss, c->recs.as<SigRec>(), c->pk_list.as<uint32_t>(),
                         cnt_p, start, c->kt, c->r.as<uint32_t>(), c->xr.as<uint32_t>(), (uint64_t*)(cnt_p + 16));
    } else if (pg.modexp) {
#if BFTKV_RSA_FORM == 29
      // 18 x 4 limbs of 29 bits (2 x 64 x 72 x 4 B of LDS per block)
      hipLaunchKernelGGL((k_rsa_modexp<RSA29_L, MONT_TPI, RSA29_W>), dim3(pg.modexp), dim3(MODEXP_BLOCK), c->modexp_lds_pad, s, d_ss, c->recs.as<SigRec>(), c->pk_list.as<uint32_t>(),
                         cnt_p, start, c->kt, c->r.as<uint32_t>(), c->xr.as<uint32_t>(), (uint64_t*)(cnt_p + 16), (const uint32_t*)(cnt_p + 5));
#else
      hipLaunchKernelGGL((k_rsa_modexp<MONT_L, MONT_TPI>), dim3(pg.modexp), dim3(MODEXP_BLOCK), c->modexp_lds_pad, s, d_ss, c->recs.as<SigRec>(), c->pk_list.as<uint32_t>(),
                         cnt_p, start, c->kt, c->r.as<uint32_t>(), c->xr.as<uint32_t>(), (uint64_t*)(cnt_p + 16));
#endif
    }
    if (wide_inline) launch_wide(start, pg.wide);
    // larger moduli: only when the keyring holds such keys (blocks beyond the queued count exit at once)
    if (pg.modexp3072)
      hipLaunchKernelGGL((k_rsa_modexp<MONT_L3072, MONT_TPI_BIG>), dim3(pg.modexp3072), dim3(MODEXP_BLOCK), 0, s, d_ss, c->recs.as<SigRec>(), c->pk_list3072.as<uint32_t>(),
                         cnt_p + 2, start + 2, c->kt, c->r3072.as<uint32_t>(), c->xr.as<uint32_t>(), (uint64_t*)nullptr);
    if (pg.modexp4096)
      hipLaunchKernelGGL((k_rsa_modexp<MONT_L4096, MONT_TPI_BIG>), dim3(pg.modexp4096), dim3(MODEXP_BLOCK), 0, s, d_ss, c->recs.as<SigRec>(), c->pk_list4096.as<uint32_t>(),
                         cnt_p + 3, start + 3, c->kt, c->r4096.as<uint32_t>(), c->xr.as<uint32_t>(), (uint64_t*)nullptr);
  };
  // a launch that fills the machine takes its turn behind the modexp of whichever context went last
  auto at_turnstile = [&](const std::function<void()>& launch, bool stamp) -> hipError_t {
    Turnstile& g = g_turnstile[(unsigned)c->device & 15u];
    std::lock_guard<std::mutex> tl(g.mu);
    hipError_t e = hipSuccess;
    if (g.last && g.owner != c && (e = hipStreamWaitEvent(s, g.last, 0)) != hipSuccess) return e;
    if (stamp && (e = rec(9, s)) != hipSuccess) return e;
    launch();
    if (!c->ev_turn && (e = hipEventCreateWithFlags(&c->ev_turn, hipEventDisableTiming)) != hipSuccess) return e;
    if ((e = hipEventRecord(c->ev_turn, s)) != hipSuccess) return e;
    g.last = c->ev_turn; g.owner = c;
    return hipSuccess;
  };
  // By the report, the pass over the long values waits for the flags word and goes apart from the main pass.  With the bit
  // read, it fills the machine as any modexp does and takes a turn at the turnstile of its own: this call's compare and phase 2
  // then stand behind the neighbour's modexp that went in between, and the call publishes a new turn.  With no flags word at the
  // deadline the grid is the one it always was, normally empty, and goes straight behind this call's modexp on the stream
  // WITHOUT a turn: the parent had it inside the main modexp's turn, so here a neighbour admitted after that turn may run
  // beside it.  (Either way it lies behind event 2: bftkv_gpu_last_timing's modexp figure does not include it.)
  auto launch_wide_apart = [&](const uint32_t* start, uint32_t blocks) -> hipError_t {
    if (blocks && !turnstile_off && dec.flags_used) return at_turnstile([&] { launch_wide(start, blocks); }, false);
    launch_wide(start, blocks);
    return hipSuccess;
  };
  if (big && !turnstile_off) {
    HIPCHK(c, at_turnstile([&] { launch_modexp(start0, dec.p1, !by_report); }, true));
  } else {
    HIPCHK(c, rec(9, s));
    launch_modexp(start0, dec.p1, !by_report);
  }
  HIPCHK(c, rec(2, s));
  if (call.upload_tbs) {
    if ((rc = (*call.upload_tbs)(sh))) return rc;
    if (!call.mid_prelaunched)
      hipLaunchKernelGGL(k_sha256_mid, dim3((n_items + MID_BLOCK - 1) / MID_BLOCK), dim3(MID_BLOCK), 0, sh, d_tbs, d_tbs_off, n_items, c->mid.as<uint32_t>());
    if ((rc = hash_stream_work())) return rc;
  }
  if (!by_report) HIPCHK(c, join(s, 6));
  if (waits_for_flags &&
      (rc = wait_for_plan_words(c, total, by_report, &rin, [&]() -> int {
         dec = plan_report::decide(rin, geo);      // (for the midstates of the other hashes: the flags are all they depend on)
         return hash_stream_work();
       }))) return rc;
  if (by_report) dec = plan_report::decide(rin, geo);      // (off the report no word changes a grid)
  if (report_path) {      // the getter flattens exactly the numbers the launches above and below read
    plan_report::flatten(dec, rin, c->last_plan_report);
    c->have_plan_report = true;
  }
  if (by_report) {
    HIPCHK(c, launch_wide_apart(start0, dec.p1.wide));
    HIPCHK(c, join(s, 6));
  }
  // digests of the hashes other than SHA-256: on the MAIN stream, after the modexp.  Normally there are none and the kernel
  // exits on a device-side flag; at its 203 VGPRs it cannot co-schedule beside k_rsa_modexp, and on the hash stream it sat
  // there until the modexp drained (1.7 ms per step in the trace) holding back the join.
  // ... and normally not even launched: the flags word says whether any signature named another hash.  (A profile of the
  // step used to show this no-op as the kernel that "ran" while a neighbour's modexp held the SIMDs.)
  const bool other_hashes = rin.flags_word ? (rin.flags_word & plan_report::FLAG_OTHER_HASH) != 0 : true;
  if (total && hashes_payloads && other_hashes)
    hipLaunchKernelGGL(k_digest_other, dim3(std::min<uint32_t>((total + 255) / 256, DIGEST_OTHER_MAX_BLOCKS)), dim3(256), 0, s,
                       d_tbs, d_tbs_off, d_ss, c->mid.as<uint32_t>(), c->mid64.as<uint64_t>(), n_items, c->recs.as<SigRec>(), total,
                       c->digests.as<uint32_t>(), c->pk_count.as<uint32_t>() + 4, txt, n_recs_dev);
  auto launch_compare = [&](const uint32_t* start, const plan_report::PhaseGrids& pg) {
    if (pg.compare[plan_report::L_RSA2048])
      hipLaunchKernelGGL(k_rsa_compare, dim3(pg.compare[plan_report::L_RSA2048]), dim3(256), 0, s, c->recs.as<SigRec>(), c->pk_list.as<uint32_t>(),
                         cnt_p, start, c->kt, c->r.as<uint32_t>(), c->digests.as<uint32_t>());
    if (pg.compare[plan_report::L_RSA3072])
      hipLaunchKernelGGL(k_rsa_compare, dim3(pg.compare[plan_report::L_RSA3072]), dim3(256), 0, s, c->recs.as<SigRec>(), c->pk_list3072.as<uint32_t>(),
                         cnt_p + 2, start + 2, c->kt, c->r3072.as<uint32_t>(), c->digests.as<uint32_t>());
    if (pg.compare[plan_report::L_RSA4096])
      hipLaunchKernelGGL(k_rsa_compare, dim3(pg.compare[plan_report::L_RSA4096]), dim3(256), 0, s, c->recs.as<SigRec>(), c->pk_list4096.as<uint32_t>(),
                         cnt_p + 3, start + 3, c->kt, c->r4096.as<uint32_t>(), c->digests.as<uint32_t>());
  };
  // DSA signatures (if any): u1 depends on the digest, so the table multiplications run after the join; the
  // inverses were started on their own stream right after the parse.  Grids cover every signature that can be in the list and
  // exit on the device-side count, so no host read-back sits between the kernels.
  auto launch_dsa = [&](const uint32_t* start, const plan_report::PhaseGrids& pg) {
    if (pg.dsa_mul)
      hipLaunchKernelGGL(k_dsa_mul, dim3(pg.dsa_mul), dim3(64), 0, s, c->recs.as<SigRec>(), c->dsa_list.as<uint32_t>(),
                         cnt_p, start, c->kt, c->digests.as<uint32_t>(), c->dsa_u.as<uint32_t>());
    // (the LDS-DMA form of this kernel measured the same and spilled: removed in round 5, profiles/r04_cfg3_ab_dsa_dma*.json)
    // a key table with DSA keys of both size classes: the list's positions sorted by class first (phase 1: counters [20], [21];
    // phase 2: [22], [23]), each instantiation over its own compact list; one class only: that instantiation over the list itself
    const uint32_t* idx_s = nullptr; const uint32_t* idx_b = nullptr; const uint32_t* cnt_cls = nullptr;
    if (c->have_dsa3072 && c->have_dsa2048) {
      uint32_t* cc = cnt_p + (start == start0 ? 20 : 22);
      uint32_t* is = c->dsa_idx.as<uint32_t>() + (start == start0 ? 0 : 2 * (size_t)total);
      if (pg.dsa_split)
        hipLaunchKernelGGL(k_dsa_split, dim3(pg.dsa_split), dim3(256), 0, s, c->recs.as<SigRec>(), c->dsa_list.as<uint32_t>(), cnt_p, start, c->kt,
                           is, is + total, cc);
      idx_s = is; idx_b = is + total; cnt_cls = cc;
    }
    if (pg.dsa_modexp4)
      hipLaunchKernelGGL((k_dsa_modexp<MONT_L, MONT_TPI>), dim3(pg.dsa_modexp4), dim3(RSA_BLOCK), 0, s,
                         c->recs.as<SigRec>(), c->dsa_list.as<uint32_t>(), cnt_p, start, c->kt, c->dsa_u.as<uint32_t>(), idx_s, cnt_cls);
    if (pg.dsa_modexp8)      // keys with p beyond 2048 bits: the 8-lane form
      hipLaunchKernelGGL((k_dsa_modexp<MONT_L3072, MONT_TPI_BIG>), dim3(pg.dsa_modexp8), dim3(RSA_BLOCK), 0, s,
                         c->recs.as<SigRec>(), c->dsa_list.as<uint32_t>(), cnt_p, start, c->kt, c->dsa_u.as<uint32_t>(), idx_b, cnt_cls ? cnt_cls + 1 : nullptr);
  };
  launch_compare(start0, dec.p1);
  HIPCHK(c, rec(8, s));
  if (dsa) {
    HIPCHK(c, hipStreamWaitEvent(s, c->ev[7], 0));
    launch_dsa(start0, dec.p1);
  }
  if (total && plan_q) {
    // phase 2: tally what phase 1 verified; whatever an item still lacks comes from its remaining packets.  No list can grow by
    // more than the packets phase 1 left unqueued (dec.phase2_bound; `total` without the plan's words)
    HIPCHK(c, c->o_nver.ensure(sizeof(uint32_t) * n_items));
    HIPCHK(c, c->o_verdict.ensure(n_items));
    hipLaunchKernelGGL(k_tally, dim3((n_items + 3) / 4), dim3(256), 0, s, c->recs.as<SigRec>(), c->base.as<uint32_t>(), c->counts.as<uint32_t>(),
                       n_items, c->kt, *plan_q, c->o_verdict.as<uint8_t>(), c->o_nver.as<uint32_t>(), (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_plan_snapshot, dim3(1), dim3(64), 0, s, cnt_p);
    pl.verdict = c->o_verdict.as<uint8_t>();
    hipLaunchKernelGGL(k_plan<2>, dim3((n_items + PLAN_ITEMS - 1) / PLAN_ITEMS), dim3(PLAN_BLOCK), 0, s, pl, c->kt, *plan_q);
    launch_dsa_inv(s, start1, dec.p2);
    launch_modexp(start1, dec.p2, !by_report);
    if (by_report) HIPCHK(c, launch_wide_apart(start1, dec.p2.wide));      // (behind a turn of its own, as in phase 1)
    launch_compare(start1, dec.p2);
    launch_dsa(start1, dec.p2);
  }
  // several keys under one key id: what the candidates behind the first do to the status of a record it did not verify
  // (never to a verdict: see the kernel)
  if (total && c->have_ambiguous && !call.d_msg_slot)
    hipLaunchKernelGGL(k_candidates, dim3((total + 63) / 64), dim3(64), 0, s, d_tbs, d_tbs_off, d_ss, d_mid_in ? d_mid_in : c->mid.as<uint32_t>(),
                       c->mid64.as<uint64_t>(), n_items, c->recs.as<SigRec>(), total, n_recs_dev, call.d_tbs_prefix, c->kt, call.d_cert_ent, call.d_sig_class, txt,
                       c->hash_mask.as<uint32_t>());
  HIPCHK(c, rec(3, s));
  HIPCHK(c, hipGetLastError());
  return 0;
}

// One processed key-table row (host copy, so that certificate entities can be appended later).
int make_key_entry(bftkv_gpu_ctx* c, const bftkv_gpu_pubkey& k, bool cert_only, KeyEntry* out) {
  KeyEntry& e = *out;
  e.key_id = k.key_id; e.entity_id = k.entity_id; e.algo = k.pk_algo; e.cert_only = cert_only;
  e.material.clear();
  e.material.push_back((char)k.pk_algo);
  e.material.push_back((char)k.usable_sign);
  auto app = [&](const uint8_t* p, uint32_t l) {
    uint32_t z = 0;
    while (z < l && p[z] == 0) ++z;
    if (l > z) e.material.append((const char*)p + z, l - z);
    e.material.push_back('|');
  };
  app(k.n, k.n_len); app(k.e, k.e_len); app(k.g, k.g_len); app(k.y, k.y_len);
  e.flags = 0;
  if (k.usable_sign) e.flags |= KEYF_USABLE_SIGN;
  if (k.pk_algo != PK_RSA_ENCRYPT_ONLY && k.pk_algo != PK_ELGAMAL) e.flags |= KEYF_CAN_SIGN;   // PublicKey.CanSign
  if (k.key_id == k.entity_id) e.flags |= KEYF_PRIMARY;
  if (cert_only) e.flags |= KEYF_CERT_ONLY;
  e.bits = (uint32_t)hostbn::bit_length(k.n, k.n_len);
  e.e = 0; e.n0 = 0; e.qbits = 0;
  e.r2w.clear(); e.nl29.clear(); e.r2_29.clear(); e.n0_29 = 0;
  e.nl.assign(MONT_NMAX, 0); e.r2.assign(MONT_NMAX, 0); e.qw.assign(8, 0); e.dtab.assign(2 * DSA_N_BIG, 0); e.qpow.clear(); e.qconst.clear();
  if (k.pk_algo == PK_RSA || k.pk_algo == PK_RSA_SIGN_ONLY) {
    if (hostbn::bit_length(k.e, k.e_len) > 32) return fail(c, BFTKV_E_UNSUPPORTED, "RSA public exponent wider than 32 bits");  // x/crypto refuses > 24 bits
    for (uint32_t j = 0; j < k.e_len; ++j) e.e = (e.e << 8) | k.e[j];
    // size class: limbs per number 76 / 112 / 152 for moduli up to 2048 / 3072 / 4096 bits (R = 2^(28 N) > 4n)
    const int nlimbs = e.bits <= 2048 ? MONT_N : (e.bits <= 3072 ? MONT_TPI_BIG * MONT_L3072 : MONT_TPI_BIG * MONT_L4096);
    if (e.bits > 4096) e.bits = 0xFFFFFFFFu;                       // status ST_UNSUPPORTED for this key
    else if (!hostbn::mont_setup(k.n, k.n_len, nlimbs, e.nl.data(), e.r2.data(), &e.n0)) e.bits = 0xFFFFFFFFu;   // even / zero modulus
    else if (e.bits <= 2048) {                                     // the 8-lane form of small calls: R = 2^2240
      std::vector<uint32_t> nl80(80);
      uint32_t n0b = 0;
      e.r2w.assign(80, 0);
      (void)hostbn::mont_setup(k.n, k.n_len, 80, nl80.data(), e.r2w.data(), &n0b);
      e.nl29.assign(RSA29_N, 0); e.r2_29.assign(RSA29_N, 0);              // the 4-lane form of big calls: 72 limbs of 29 bits
      (void)hostbn::mont_setup(k.n, k.n_len, RSA29_N, e.nl29.data(), e.r2_29.data(), &e.n0_29, RSA29_W);
    }
  } else if (k.pk_algo == PK_DSA) {
    // n = p, e = q.  Montgomery domain mod p; g and y in Montgomery form seed the fixed-base tables.
    // Size class of p: 76 limbs over 4 lanes (<= 2048 bits, R = 2^2128) or 112 limbs over 8 lanes (<= 3072 bits, R = 2^3136).
    e.qbits = (uint32_t)hostbn::bit_length(k.e, k.e_len);
    const int NLp = e.bits <= 2048 ? (int)DSA_N_SMALL : (int)DSA_N_BIG;
    const uint32_t cap_bits = e.bits <= 2048 ? 2048u : 3072u;
    const int nwords = (28 * NLp + 31) / 32 + 1;
    std::vector<uint32_t> p(nwords), g(nwords), y(nwords), q(nwords);
    hostbn::from_be(k.e, k.e_len, q.data(), nwords);
    bool ok = e.bits >= 2 && e.bits <= 3072 && e.qbits >= 32 && e.qbits <= 256 && (q[0] & 1u) &&
              hostbn::mont_setup(k.n, k.n_len, NLp, e.nl.data(), e.r2.data(), &e.n0);
    if (ok && (hostbn::bit_length(k.g, k.g_len) > cap_bits || hostbn::bit_length(k.y, k.y_len) > cap_bits)) ok = false;
    if (ok) {
      hostbn::from_be(k.n, k.n_len, p.data(), nwords);
      hostbn::from_be(k.g, k.g_len, g.data(), nwords);
      hostbn::from_be(k.y, k.y_len, y.data(), nwords);
      hostbn::reduce(g.data(), p.data(), nwords);
      hostbn::reduce(y.data(), p.data(), nwords);
      hostbn::to_mont_limbs(g.data(), p.data(), nwords, NLp, &e.dtab[0]);
      hostbn::to_mont_limbs(y.data(), p.data(), nwords, NLp, &e.dtab[DSA_N_BIG]);
      for (int j = 0; j < 8; ++j) e.qw[j] = q[j];
      // 2^(28 j) mod q, one row per limb of p, as radix-2^28 limbs (k_dsa_modexp folds v mod p to v mod q with them)
      e.qpow.assign((size_t)NLp * 10, 0);
      uint32_t x[9] = {1, 0, 0, 0, 0, 0, 0, 0, 0}, q9[9];
      for (int j = 0; j < 9; ++j) q9[j] = j < 8 ? q[j] : 0;
      for (int j = 0; j < NLp; ++j) {
        hostbn::to_limbs28(x, 9, &e.qpow[(size_t)j * 10], 10);
        for (int b = 0; b < MONT_W; ++b) hostbn::dbl_mod(x, q9, 9);
      }
      // mod-q Montgomery constants (u256_montmul): 2^512 mod q and -q^-1 mod 2^32
      e.qconst.assign(12, 0);
      uint32_t r2q[9] = {1, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int b = 0; b < 512; ++b) hostbn::dbl_mod(r2q, q9, 9);
      for (int j = 0; j < 8; ++j) e.qconst[j] = r2q[j];
      uint32_t inv = 1;
      for (int it = 0; it < 5; ++it) inv *= 2u - q[0] * inv;     // Newton: q^-1 mod 2^32
      e.qconst[8] = 0u - inv;
    } else {
      e.bits = 0xFFFFFFFFu;   // fenced key shapes (even p or q, q > 256 bits, p > 3072 bits): ST_UNSUPPORTED
    }
  }
  return 0;
}

// Fixed-base tables for the DSA rows of the table being uploaded.  A table depends only on (p, g, y), so it is
// keyed by the row's key material and survives re-uploads (certificate batches re-upload the table per request).
// Certificate-only DSA keys (they arrive inside unauthenticated requests) get a bounded number of table slots -- 8 at every
// width above 8 bits (14 bits: 189 MB and a build each), 1024 at the 5 MB width, fewer where a caller's budget leaves less room --
// recycled among themselves; a certificate key beyond that is marked unsupported for this upload (its signatures are fenced: the
// reference path decides).  The window width AND the entry size (76 limbs, or 112 once a key with p beyond 2048 bits is in the
// ring) follow the NODE keyring's DSA population alone and are re-evaluated only when that keyring changes, so neither a flood
// of certificates nor jitter in the free-memory reading can force the node keys' tables to be rebuilt: a certificate-only key with
// p beyond 2048 bits in an arena of 76-limb entries is fenced.  `bits_changed`: rows were marked.
int sync_dsa_tables(bftkv_gpu_ctx* c, const std::vector<const KeyEntry*>& rows, const std::vector<uint8_t>& algo,
                    std::vector<uint32_t>& bits, bool* bits_changed) {
  std::vector<uint32_t> slot(rows.size() ? rows.size() : 1, 0xFFFFFFFFu);
  *bits_changed = false;
  auto stride_bytes = [&](uint32_t w, uint32_t E) -> size_t { return (size_t)dsa_slot_stride(w, E) * sizeof(uint32_t); };
  size_t ring_dsa = 0;
  bool ring_big = false;
  for (size_t i = 0; i < rows.size(); ++i)
    if (algo[i] == PK_DSA && bits[i] != 0xFFFFFFFFu && !rows[i]->cert_only) { ++ring_dsa; ring_big = ring_big || bits[i] > 2048; }
  auto assign = [&](std::vector<uint32_t>& new_slots, std::vector<uint32_t>& new_rows) {
    new_slots.clear(); new_rows.clear();
    // certificate-only DSA keys share a bounded set of table slots, recycled by recency
    size_t cert_cap = c->dsa_wbits > 8 ? 8 : 1024;
    if (c->dsa_budget_bytes) {
      const size_t per = stride_bytes(c->dsa_wbits, c->dsa_entry_limbs), ring_need = per * ring_dsa;
      cert_cap = std::min(cert_cap, c->dsa_budget_bytes > ring_need ? (c->dsa_budget_bytes - ring_need) / per : 0);
    }
    for (size_t i = 0; i < rows.size(); ++i) {
      if (algo[i] != PK_DSA || bits[i] == 0xFFFFFFFFu) continue;
      if (bits[i] > 2048 && c->dsa_entry_limbs != DSA_N_BIG) {      // (only a certificate key can get here: the ring decides the entry size)
        bits[i] = 0xFFFFFFFFu; *bits_changed = true;
        const_cast<KeyEntry*>(rows[i])->dsa_unslotted = true;
        continue;
      }
      auto it = c->dsa_comb_slot.find(rows[i]->material);
      if (it == c->dsa_comb_slot.end()) {
        uint32_t id = (uint32_t)c->dsa_comb_slot.size();
        if (rows[i]->cert_only && c->dsa_cert_materials.size() >= cert_cap) {
          // recycle the slot of a certificate key this upload does not hold
          // ... a slot whose key is not in the table any more, or whose certificate the current compound call does not name
          std::string victim;
          if (rows[i]->last_used == c->cert_clock) {
            for (const std::string& m : c->dsa_cert_materials) {
              bool in_use = false;
              for (size_t j = 0; j < rows.size() && !in_use; ++j)
                in_use = algo[j] == PK_DSA && rows[j]->material == m && (!rows[j]->cert_only || rows[j]->last_used == c->cert_clock);
              if (!in_use) { victim = m; break; }
            }
          }
          if (victim.empty()) {
            bits[i] = 0xFFFFFFFFu; *bits_changed = true;
            const_cast<KeyEntry*>(rows[i])->dsa_unslotted = true;
            continue;
          }
          for (size_t j = 0; j < rows.size(); ++j)       // whoever held the slot is fenced from now on
            if (algo[j] == PK_DSA && rows[j]->material == victim) {
              bits[j] = 0xFFFFFFFFu; slot[j] = 0xFFFFFFFFu; *bits_changed = true;
              const_cast<KeyEntry*>(rows[j])->dsa_unslotted = true;
            }
          id = c->dsa_comb_slot[victim];
          c->dsa_comb_slot.erase(victim);
          c->dsa_cert_materials.erase(victim);
        }
        it = c->dsa_comb_slot.emplace(rows[i]->material, id).first;
        if (rows[i]->cert_only) c->dsa_cert_materials.insert(rows[i]->material);
        const_cast<KeyEntry*>(rows[i])->dsa_unslotted = false;
        new_slots.push_back(it->second); new_rows.push_back((uint32_t)i);
      } else if (!rows[i]->cert_only) c->dsa_cert_materials.erase(rows[i]->material);      // (a certificate key that joined the node keyring)
      slot[i] = it->second;
    }
  };
  // Window width by DSA population and free HBM -- HBM capacity traded for multiplications, GRADED (round 5: the policy used to
  // fall from 16 bits straight to 8 at 65 keys, 31 -> 63 products per signature).  2 * ceil(256 / w) - 1 products and
  // 2 * ceil(256 / w) * (2^w - 1) * 304 bytes per key (448 bytes per entry once the arena holds 3072-bit keys):
  //     w   18      16      15      14      13      12      10      8
  //   prod  29      31      35      37      39      43      51      63
  //   /key  2.39 GB 637 MB  358 MB  189 MB  100 MB  55 MB   16 MB   5 MB
  // Without a budget: the widest width whose tables for every key of the ring -- with the half again the buffer grows by -- fit
  // 45 % of the free HBM for 18 bits (as since round 3), a quarter for the others.  With a caller's budget
  // (bftkv_gpu_set_dsa_table_budget: a service that shares the GPU): the widest width whose tables for every key of the ring fit
  // the budget, and the arena is never allocated beyond it.  (17 bits has 16 windows like 16; 19 / 20 can be pinned, never
  // chosen.)  4 bits beyond 4096 keys.
  auto policy = [&](size_t n_keys, uint32_t E) -> uint32_t {
    if (c->dsa_wbits_pinned) return c->dsa_wbits_pinned;
    if (const char* e = getenv("BFTKV_DSA_WBITS")) {            // experiments: the width without touching the caller
      const uint32_t b = (uint32_t)atoi(e);
      if (b == 4 || (b >= 8 && b <= 20)) return b;
    }
    if (n_keys > 4096) return 4u;
    static const uint32_t widths[] = {18, 16, 15, 14, 13, 12, 10};
    if (c->dsa_budget_bytes) {
      for (uint32_t w : widths)
        if (std::max<size_t>(n_keys, 1) * stride_bytes(w, E) <= c->dsa_budget_bytes) return w;
      return std::max<size_t>(n_keys, 1) * stride_bytes(8, E) <= c->dsa_budget_bytes ? 8u : 4u;
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const size_t room = free_b + c->dsa_comb.cap;
      for (uint32_t w : widths) {
        const size_t need = (n_keys + 1) * stride_bytes(w, E) * 3 / 2;
        if (need < (w == 18 ? room / 100 * 45 : room / 4)) return w;
      }
    }
    return 8u;
  };
  uint32_t want_E = c->dsa_entry_limbs;
  if (c->dsa_ring_epoch_seen != c->ring_epoch || c->dsa_wbits_want == 0) {      // the node keyring changed (or first upload)
    want_E = ring_big ? DSA_N_BIG : DSA_N_SMALL;
    c->dsa_wbits_want = policy(ring_dsa, want_E);
    c->dsa_ring_epoch_seen = c->ring_epoch;
  }
  const uint32_t want_wbits = c->dsa_wbits_pinned ? c->dsa_wbits_pinned : c->dsa_wbits_want;
  std::vector<uint32_t> new_slots, new_rows;
  bool restart = false;
  if (want_wbits != c->dsa_wbits || want_E != c->dsa_entry_limbs) {       // width or entry size change: every table is rebuilt
    restart = true;
    c->dsa_comb_slot.clear();
    c->dsa_cert_materials.clear();
    c->dsa_wbits = want_wbits;
    c->dsa_entry_limbs = want_E;
  }
  assign(new_slots, new_rows);
  const size_t live = [&] { size_t n = 0; for (uint32_t v : slot) n += v != 0xFFFFFFFFu; return n; }();
  // tables of keys that left the keyring stay cached by key material (a key that comes back costs nothing) -- as long as they
  // are few and the wide layouts do not crowd the HBM: past 45 % of what is free (with the buffer's growth margin), or past the
  // caller's budget, they go
  bool crowded = false;
  if (!restart && c->dsa_comb_slot.size() > live) {
    const size_t held = c->dsa_comb_slot.size() * stride_bytes(c->dsa_wbits, c->dsa_entry_limbs);
    size_t free_b = 0, total_b = 0;
    if (c->dsa_budget_bytes) crowded = held > c->dsa_budget_bytes;
    else if (c->dsa_wbits >= 12 && hipMemGetInfo(&free_b, &total_b) == hipSuccess) crowded = held * 3 / 2 > (free_b + c->dsa_comb.cap) / 100 * 45;
  }
  if (!restart && (c->dsa_comb_slot.size() > 2 * live + 256 || crowded)) {   // mostly stale, or crowded: restart
    restart = true;
    c->dsa_comb_slot.clear();
    c->dsa_cert_materials.clear();
    for (size_t i = 0; i < rows.size(); ++i) slot[i] = 0xFFFFFFFFu;
    assign(new_slots, new_rows);
  }
  if (getenv("BFTKV_DEBUG_DSA")) {
    size_t n_cert_rows = 0, n_dsa = 0, n_fenced = 0;
    for (size_t i = 0; i < rows.size(); ++i) { n_cert_rows += rows[i]->cert_only; n_dsa += algo[i] == PK_DSA; n_fenced += algo[i] == PK_DSA && bits[i] == 0xFFFFFFFFu; }
    fprintf(stderr, "[dsa tables] rows %zu (cert %zu, dsa %zu, dsa without slot %zu) width %u want %u entry limbs %u slots %zu cert-slots %zu new %zu restart %d clock %llu budget %zu\n", rows.size(),
            n_cert_rows, n_dsa, n_fenced, c->dsa_wbits, want_wbits, c->dsa_entry_limbs, c->dsa_comb_slot.size(), c->dsa_cert_materials.size(), new_slots.size(), (int)restart,
            (unsigned long long)c->cert_clock, c->dsa_budget_bytes);
  }
  int rc;
  if ((rc = upload(c, c->k_dsaslot, slot))) return rc;
  c->kt.dsa_slot = c->k_dsaslot.as<uint32_t>();
  c->kt.dsa_wbits = c->dsa_wbits;
  c->kt.dsa_entry_limbs = c->dsa_entry_limbs;
  if (new_slots.empty()) return 0;
  const uint32_t E = c->dsa_entry_limbs;
  const size_t per_key = stride_bytes(c->dsa_wbits, E);
  const size_t need = per_key * c->dsa_comb_slot.size();
  // (a restart whose tables are much smaller than the arena -- a narrower width, a budget -- gives the memory back first)
  if (restart && (c->dsa_comb.cap > 2 * need + (64u << 20) || (c->dsa_budget_bytes && c->dsa_comb.cap > c->dsa_budget_bytes))) c->dsa_comb.release();
  if (need > c->dsa_comb.cap) {           // grow, keeping the tables already built
    DevBuf bigger;
    // room to grow by half -- but a pinned width beyond 18 bits (4.46 / 8.3 GB per key) only by two more keys, and never past a
    // caller's budget (the ring's own tables always fit it: the policy chose the width that way; a pinned width is the caller's word)
    size_t want = need + (c->dsa_wbits > 18 ? std::min(need / 2, 2 * per_key) : need / 2);
    if (c->dsa_budget_bytes) want = std::max(need, std::min(want, c->dsa_budget_bytes));
    if (restart) c->dsa_comb.release();      // (nothing to keep: the old tables go before the new ones are allocated)
    HIPCHK(c, bigger.ensure_exact(want));
    // every whole slot the old buffer holds (new and recycled slots are built below, in place)
    const size_t keep = restart ? 0 : std::min(need, (c->dsa_comb.cap / per_key) * per_key);
    if (keep && c->dsa_comb.p) HIPCHK(c, hipMemcpyAsync(bigger.p, c->dsa_comb.p, keep, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dsa_comb.release();
    c->dsa_comb = bigger;
  }
  c->kt.dsa_comb = c->dsa_comb.as<uint32_t>();
  for (size_t k = 0; k < new_slots.size(); ++k) {    // the slot's 2^(28 j) mod q rows and mod-q constants (host-computed, 3 - 4.5 KB)
    char* tail = (char*)c->dsa_comb.p + per_key * new_slots[k] + dsa_comb_limbs_per_key(c->dsa_wbits, E) * sizeof(uint32_t);
    const KeyEntry* ke = rows[new_rows[k]];
    HIPCHK(c, hipMemcpyAsync(tail, ke->qpow.data(), ke->qpow.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tail + dsa_qpow_words(E) * sizeof(uint32_t), ke->qconst.data(), ke->qconst.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  }
  // one build per size class of p: <19, 4> for p <= 2048 bits, <14, 8> beyond
  hipError_t e = hipSuccess;
  for (int big = 0; big < 2 && e == hipSuccess; ++big) {
    std::vector<uint32_t> cs, cr;
    for (size_t k = 0; k < new_slots.size(); ++k)
      if ((bits[new_rows[k]] > 2048) == (big == 1)) { cs.push_back(new_slots[k]); cr.push_back(new_rows[k]); }
    if (cs.empty()) continue;
    DevBuf d_slots, d_rows;
    if ((rc = upload(c, d_slots, cs)) || (rc = upload(c, d_rows, cr))) { d_slots.release(); d_rows.release(); return rc; }
    const uint32_t parts = c->dsa_wbits > 12 ? 1u << (c->dsa_wbits - 12u) : 1u;        // at most 4,096 entries per group
    const uint32_t n_groups = (uint32_t)cs.size() * 2u * dsa_nwin(c->dsa_wbits) * parts;
    if (big)
      hipLaunchKernelGGL((k_dsa_build_comb<MONT_L3072, MONT_TPI_BIG>), dim3((n_groups + RSA_BLOCK / MONT_TPI_BIG - 1) / (RSA_BLOCK / MONT_TPI_BIG)), dim3(RSA_BLOCK), 0, c->stream,
                         (uint32_t)cs.size(), d_slots.as<uint32_t>(), d_rows.as<uint32_t>(), c->kt, c->dsa_comb.as<uint32_t>(), parts);
    else
      hipLaunchKernelGGL((k_dsa_build_comb<MONT_L, MONT_TPI>), dim3((n_groups + QUADS_PER_BLOCK - 1) / QUADS_PER_BLOCK), dim3(RSA_BLOCK), 0, c->stream,
                         (uint32_t)cs.size(), d_slots.as<uint32_t>(), d_rows.as<uint32_t>(), c->kt, c->dsa_comb.as<uint32_t>(), parts);
    e = hipStreamSynchronize(c->stream);
    d_slots.release(); d_rows.release();
  }
  if (e != hipSuccess) return fail(c, BFTKV_E_DEVICE, "k_dsa_build_comb", e);
  return 0;
}

// Builds and uploads the device key table from c->ring (the node keyring, in getKeyring() order) followed by
// c->certs (entities that only exist inside request certificates, reachable through VerifyWithCertificate).
int upload_key_table(bftkv_gpu_ctx* c) {
  if (c->root) return fail(c, BFTKV_E_STATE, "a forked context cannot change the key table (use its root)");
  KtWrite kw(c);      // the forks' calls in flight drain first; new ones wait
  std::vector<uint64_t> key_id, entity_ids;
  std::vector<uint32_t> entity, bits, e32, nl, r2, r2w, n0, qw, qbits, dtab, nl29, r2_29, n0_29;
  std::vector<uint8_t> algo, flags;
  auto add29 = [&](const KeyEntry& e) {     // rows of the 29-bit tables: zero for keys that have none
    nl29.insert(nl29.end(), e.nl29.begin(), e.nl29.end()); nl29.resize(key_id.size() * RSA29_N, 0);
    r2_29.insert(r2_29.end(), e.r2_29.begin(), e.r2_29.end()); r2_29.resize(key_id.size() * RSA29_N, 0);
    n0_29.push_back(e.n0_29);
  };
  std::vector<const KeyEntry*> rows;
  auto add = [&](const KeyEntry& e, bool own_entity) {
    uint32_t ent = 0;
    if (own_entity) { ent = (uint32_t)entity_ids.size(); entity_ids.push_back(e.entity_id); }
    else {
      for (; ent < entity_ids.size(); ++ent) if (entity_ids[ent] == e.entity_id) break;
      if (ent == entity_ids.size()) entity_ids.push_back(e.entity_id);
    }
    key_id.push_back(e.key_id); entity.push_back(ent); algo.push_back(e.algo); flags.push_back(e.flags);
    bits.push_back(e.bits); e32.push_back(e.e); n0.push_back(e.n0); qbits.push_back(e.qbits);
    nl.insert(nl.end(), e.nl.begin(), e.nl.end()); r2.insert(r2.end(), e.r2.begin(), e.r2.end());
    r2w.insert(r2w.end(), e.r2w.begin(), e.r2w.end()); r2w.resize(key_id.size() * 80, 0);
    add29(e);
    qw.insert(qw.end(), e.qw.begin(), e.qw.end()); dtab.insert(dtab.end(), e.dtab.begin(), e.dtab.end());
    rows.push_back(&e);
    return ent;
  };
  for (auto& e : c->ring) add(e, false);
  c->n_ring_entities = (uint32_t)entity_ids.size();
  // certificate entities: one entity index per distinct certificate (cert_group), never merged with the keyring's
  int last_group = -1;
  uint32_t group_ent = 0;
  std::vector<uint32_t> group_ents;         // certificate group -> entity index (kt_group_ent)
  for (auto& e : c->certs) {
    if (e.cert_group != last_group) { group_ent = add(e, true); last_group = e.cert_group; }
    else {
      key_id.push_back(e.key_id); entity.push_back(group_ent); algo.push_back(e.algo); flags.push_back(e.flags);
      bits.push_back(e.bits); e32.push_back(e.e); n0.push_back(e.n0); qbits.push_back(e.qbits);
      nl.insert(nl.end(), e.nl.begin(), e.nl.end()); r2.insert(r2.end(), e.r2.begin(), e.r2.end());
      r2w.insert(r2w.end(), e.r2w.begin(), e.r2w.end()); r2w.resize(key_id.size() * 80, 0);
      add29(e);
      qw.insert(qw.end(), e.qw.begin(), e.qw.end()); dtab.insert(dtab.end(), e.dtab.begin(), e.dtab.end());
      rows.push_back(&e);
    }
    const_cast<KeyEntry&>(e).entity_index = group_ent;
    if (e.cert_group >= 0) {
      if (group_ents.size() <= (size_t)e.cert_group) group_ents.resize((size_t)e.cert_group + 1, 0xFFFFFFFEu);
      group_ents[(size_t)e.cert_group] = group_ent;
    }
  }
  // issuer lookup index: ids ascending, ties in table order (std::stable_sort over row numbers)
  std::vector<uint32_t> sorted_slot(key_id.size());
  for (size_t i = 0; i < sorted_slot.size(); ++i) sorted_slot[i] = (uint32_t)i;
  std::stable_sort(sorted_slot.begin(), sorted_slot.end(), [&](uint32_t a, uint32_t b) { return key_id[a] < key_id[b]; });
  std::vector<uint64_t> sorted_id(key_id.size());
  for (size_t i = 0; i < sorted_slot.size(); ++i) sorted_id[i] = key_id[sorted_slot[i]];
  int rc;
  if ((rc = upload(c, c->k_sorted_id, sorted_id)) || (rc = upload(c, c->k_sorted_slot, sorted_slot))) return rc;
  if ((rc = upload(c, c->k_id, key_id)) || (rc = upload(c, c->k_entity, entity)) || (rc = upload(c, c->k_algo, algo)) ||
      (rc = upload(c, c->k_flags, flags)) || (rc = upload(c, c->k_bits, bits)) || (rc = upload(c, c->k_e, e32)) ||
      (rc = upload(c, c->k_n, nl)) || (rc = upload(c, c->k_r2, r2)) || (rc = upload(c, c->k_n0, n0)) ||
      (rc = upload(c, c->k_q, qw)) || (rc = upload(c, c->k_qbits, qbits)) || (rc = upload(c, c->k_dsatab, dtab)) || (rc = upload(c, c->k_r2w, r2w)) ||
      (rc = upload(c, c->k_n29, nl29)) || (rc = upload(c, c->k_r2_29, r2_29)) || (rc = upload(c, c->k_n0_29, n0_29)))
    return rc;
  c->kt.r2_limbs80 = c->k_r2w.as<uint32_t>();
  c->kt.n_limbs29 = c->k_n29.as<uint32_t>(); c->kt.r2_limbs29 = c->k_r2_29.as<uint32_t>(); c->kt.n0inv29 = c->k_n0_29.as<uint32_t>();
  c->n_keys = (uint32_t)key_id.size();
  c->kt.n_keys = c->n_keys;
  c->kt.n_limbs = c->k_n.as<uint32_t>();
  c->kt.r2_limbs = c->k_r2.as<uint32_t>();          // k_dsa_build_comb reads n, R^2, n0inv and the table seeds
  c->kt.n0inv = c->k_n0.as<uint32_t>();
  c->kt.dsa_tab = c->k_dsatab.as<uint32_t>();
  bool bits_changed = false;
  if ((rc = sync_dsa_tables(c, rows, algo, bits, &bits_changed))) return rc;
  if (bits_changed && (rc = upload(c, c->k_bits, bits))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_dsa_keys = c->have_dsa3072 = c->have_dsa2048 = c->have_rsa3072 = c->have_rsa4096 = c->have_ambiguous = false;
  for (size_t i = 0; i < algo.size(); ++i) {
    if (flags[i] & KEYF_AMBIGUOUS) c->have_ambiguous = true;
    if (algo[i] == PK_DSA) c->have_dsa_keys = true;
    if (algo[i] == PK_DSA && bits[i] != 0xFFFFFFFFu && bits[i] > 2048) c->have_dsa3072 = true;
    if (algo[i] == PK_DSA && (bits[i] == 0xFFFFFFFFu || bits[i] <= 2048)) c->have_dsa2048 = true;
    if ((algo[i] == PK_RSA || algo[i] == PK_RSA_SIGN_ONLY) && bits[i] != 0xFFFFFFFFu) {
      if (bits[i] > 3072) c->have_rsa4096 = true; else if (bits[i] > 2048) c->have_rsa3072 = true;
    }
  }
  c->n_entities = (uint32_t)entity_ids.size();
  c->h_key_id = key_id;
  c->h_entity_id = entity_ids;
  c->h_key_entity = entity;
  c->h_key_flags = flags;
  c->kt.n_keys = c->n_keys;
  c->kt.key_id = c->k_id.as<uint64_t>();
  c->kt.sorted_id = c->k_sorted_id.as<uint64_t>();
  c->kt.sorted_slot = c->k_sorted_slot.as<uint32_t>();
  c->kt.entity = c->k_entity.as<uint32_t>();
  c->kt.pk_algo = c->k_algo.as<uint8_t>();
  c->kt.flags = c->k_flags.as<uint8_t>();
  c->kt.mod_bits = c->k_bits.as<uint32_t>();
  c->kt.rsa_e = c->k_e.as<uint32_t>();
  c->kt.n_limbs = c->k_n.as<uint32_t>();
  c->kt.r2_limbs = c->k_r2.as<uint32_t>();
  c->kt.n0inv = c->k_n0.as<uint32_t>();
  c->kt.q_words = c->k_q.as<uint32_t>();
  c->kt.q_bits = c->k_qbits.as<uint32_t>();
  c->kt.dsa_tab = c->k_dsatab.as<uint32_t>();
  c->kt.dsa_slot = c->k_dsaslot.as<uint32_t>();
  c->kt.dsa_comb = c->dsa_comb.as<uint32_t>();
  c->kt.dsa_wbits = c->dsa_wbits;
  c->kt.dsa_entry_limbs = c->dsa_entry_limbs;
  c->kt_group_ent = std::move(group_ents);
  c->kt_cert_epoch = c->cert_epoch;
  ++c->keyring_gen;
  return 0;
}

// A fork's view of its root (caller holds root->kt_rw shared): the key-table descriptor and the host-side id vectors by
// value, the quorum descriptors by value with the fork's own membership tables (built on demand, keyed to the generation).
int fork_refresh(bftkv_gpu_ctx* c) {
  bftkv_gpu_ctx* r = c->root;
  if (c->seen_keyring_gen != r->keyring_gen) {
    c->kt = r->kt;
    c->n_keys = r->n_keys; c->n_entities = r->n_entities; c->n_ring_entities = r->n_ring_entities;
    c->have_dsa_keys = r->have_dsa_keys; c->have_dsa3072 = r->have_dsa3072; c->have_dsa2048 = r->have_dsa2048; c->have_rsa3072 = r->have_rsa3072; c->have_rsa4096 = r->have_rsa4096; c->have_ambiguous = r->have_ambiguous;
    c->h_key_id = r->h_key_id; c->h_entity_id = r->h_entity_id; c->h_key_entity = r->h_key_entity; c->h_key_flags = r->h_key_flags;
    c->n_dsa_slots = r->dsa_comb_slot.size(); c->dsa_wbits = r->dsa_wbits; c->dsa_entry_limbs = r->dsa_entry_limbs;
    c->keyring_gen = r->keyring_gen;          // the fork's membership tables follow the root's generations
    c->seen_keyring_gen = r->keyring_gen;
  }
  c->early_exit = r->early_exit;
  if (c->seen_quorum_gen != r->quorum_gen) {
    for (auto& q : c->quorums) { q.member.release(); q.ids.release(); }
    c->quorums.clear();
    c->quorums.resize(r->quorums.size());
    for (size_t i = 0; i < r->quorums.size(); ++i) {
      const QuorumHost& s = r->quorums[i];
      QuorumHost& d = c->quorums[i];
      d.live = s.live; d.n_qcs = s.n_qcs; d.nodes = s.nodes;
      for (int k = 0; k < MAX_QC; ++k) { d.f[k] = s.f[k]; d.mn[k] = s.mn[k]; d.thr[k] = s.thr[k]; d.suff[k] = s.suff[k]; }
      d.keyring_gen = ~0ull;
    }
    c->seen_quorum_gen = r->quorum_gen;
  }
  return 0;
}

// offsets must start at 0 and be non-decreasing: they become device-side read ranges
int check_offsets(bftkv_gpu_ctx* c, const uint64_t* off, uint32_t n, const char* what) {
  if (off[0] != 0) return fail(c, BFTKV_E_INVALID, what);
  for (uint32_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return fail(c, BFTKV_E_INVALID, what);
  return 0;
}

int check_quorum(bftkv_gpu_ctx* c, int quorum) {
  if (quorum < 0 || (size_t)quorum >= c->quorums.size() || !c->quorums[quorum].live) return fail(c, BFTKV_E_INVALID, "bad quorum handle");
  return 0;
}

}  // namespace

extern "C" {

int bftkv_gpu_init(int device_ordinal, bftkv_gpu_ctx** out) {
  if (!out) return BFTKV_E_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return BFTKV_E_DEVICE;   // no GPU: fail loudly, no CPU fallback
  if (device_ordinal < 0 || device_ordinal >= n) return BFTKV_E_INVALID;
  if (hipSetDevice(device_ordinal) != hipSuccess) return BFTKV_E_DEVICE;
  bftkv_gpu_ctx* c = new bftkv_gpu_ctx();
  c->device = device_ordinal;
  if (hipHostMalloc((void**)&c->h_mail, 64, hipHostMallocMapped) == hipSuccess) {
    if (hipHostGetDevicePointer((void**)&c->d_mail, c->h_mail, 0) != hipSuccess) { (void)hipHostFree(c->h_mail); c->h_mail = nullptr; c->d_mail = nullptr; }
    else memset(c->h_mail, 0, 64);
  } else c->h_mail = nullptr;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream_h, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream_d, hipStreamNonBlocking) != hipSuccess) { delete c; return BFTKV_E_DEVICE; }
  { std::lock_guard<std::mutex> lk(g_live_mu); g_live.push_back(c); }
  if (const char* e = getenv("BFTKV_STAGED_SPIN_US")) c->staged_spin_us = (uint32_t)atoi(e);
  if (const char* e = getenv("BFTKV_MODEXP_LDS_PAD")) c->modexp_lds_pad = (uint32_t)atoi(e);
  if (const char* e = getenv("BFTKV_MULTIEXP_PARTS")) c->multiexp_parts = (uint32_t)atoi(e);
  if (const char* e = getenv("BFTKV_EC_SPLIT")) c->ec_split = (uint32_t)atoi(e);
  if (const char* e = getenv("BFTKV_EC_WINDOW")) c->ec_window = (uint32_t)atoi(e);
  if (const char* e = getenv("BFTKV_MULTIEXP_LANES")) c->multiexp_lanes = (uint32_t)atoi(e);
  if (const char* e = getenv("BFTKV_RSAV_LANES")) c->rsav_lanes = (uint32_t)atoi(e);
  if (const char* e = getenv("BFTKV_MULTIEXP_BLOCK")) c->multiexp_block = (uint32_t)atoi(e);
  if (const char* e = getenv("BFTKV_DSA_INV")) c->dsa_inv_mode = !strcmp(e, "batched") ? 2u : !strcmp(e, "single") ? 1u : 0u;
  if (const char* e = getenv("BFTKV_PSIGN_ORDER")) c->psign_caller_order = !strcmp(e, "caller");
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal) == hipSuccess && cus > 0) c->n_cus = (uint32_t)cus; }
  *out = c;
  return BFTKV_OK;
}

int bftkv_gpu_ctx_fork(bftkv_gpu_ctx* root, bftkv_gpu_ctx** out) {
  if (!root || !out) return BFTKV_E_INVALID;
  if (root->root) return fail(root, BFTKV_E_INVALID, "fork of a fork");
  bftkv_gpu_ctx* c = nullptr;
  int rc = bftkv_gpu_init(root->device, &c);
  if (rc) return rc;
  c->root = root;
  c->early_exit = root->early_exit;
  c->dsa_inv_mode = root->dsa_inv_mode;
  root->n_forks.fetch_add(1);
  *out = c;
  return 0;
}

void bftkv_gpu_destroy(bftkv_gpu_ctx* c) {
  if (!c) return;
  for (bftkv_gpu_ctx* w : c->hb_workers) bftkv_gpu_destroy(w);      // private forks of the root (host-buffer pipeline): they go first
  c->hb_workers.clear();
  if (!c->root && c->n_forks.load() > 0) {     // its forks read this context's key table: they go first
    fprintf(stderr, "bftkv_gpu_destroy: context still has %d forked context(s); not destroyed\n", c->n_forks.load());
    return;
  }
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (size_t i = 0; i < g_live.size(); ++i) if (g_live[i] == c) { g_live.erase(g_live.begin() + i); break; }
  }
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->stream_h);
  (void)hipStreamSynchronize(c->stream_d);
  for (DevBuf* b : {&c->k_id, &c->k_entity, &c->k_algo, &c->k_flags, &c->k_bits, &c->k_e, &c->k_n, &c->k_r2, &c->k_n0, &c->k_q, &c->k_qbits, &c->k_dsatab, &c->k_dsaslot, &c->dsa_comb, &c->k_sorted_id, &c->k_sorted_slot, &c->k_r2w, &c->k_n29, &c->k_r2_29, &c->k_n0_29,
                    &c->chunk_arena, &c->chunk_ctr, &c->counts, &c->base, &c->total, &c->item_flags, &c->walk_scratch, &c->cert_ent, &c->sig_class, &c->mid, &c->mid64, &c->hash_mask, &c->recs, &c->digests, &c->r, &c->xr,
                    &c->pk_list, &c->pk_list3072, &c->pk_list4096, &c->r3072, &c->r4096, &c->pk_count, &c->dsa_list, &c->dsa_u, &c->dsa_idx, &c->ids_tmp, &c->o_err, &c->o_nver, &c->o_verdict, &c->o_fenced, &c->in_tbs, &c->in_tbs_off,
                    &c->in_ss, &c->in_ss_off, &c->in_prefix, &c->in_prefix_off, &c->in_shared, &c->in_shared_off, &c->in_seg, &c->st_tmp, &c->item_tmp, &c->bits_tmp, &c->plan_cut, &c->txt_mid32, &c->txt_mid64, &c->txt_tail, &c->txt_len})
    b->release();
  for (auto& q : c->quorums) { q.member.release(); q.ids.release(); }
  keysets_release_all(c);
  c->in_pack.release();
  c->forced_iss.release();
  release_small_pin(c);
  if (c->h_out) (void)hipHostFree(c->h_out);
  if (c->root) c->root->n_forks.fetch_sub(1);
  for (DevBuf* b : c->scratch_pool) { b->release(); delete b; }
  for (auto& kv : c->modtab_cache) for (DevBuf& b : kv.second) b.release();
  for (DevBuf& b : c->ec_fb_tab) b.release();
  if (c->h_mail) (void)hipHostFree(c->h_mail);
  if (c->hb_out) (void)hipHostFree(c->hb_out);
  if (c->hb_ring) { if (c->stream_c) (void)hipStreamSynchronize(c->stream_c); delete (HbRing*)c->hb_ring; }
  for (hipEvent_t e : c->hb_ev) (void)hipEventDestroy(e);
  if (c->hb_ev0) (void)hipEventDestroy(c->hb_ev0);
  if (c->seg_ev) (void)hipEventDestroy(c->seg_ev);
  if (c->stream_c) { (void)hipStreamSynchronize(c->stream_c); (void)hipStreamDestroy(c->stream_c); }
  if (c->stream_c2) { (void)hipStreamSynchronize(c->stream_c2); (void)hipStreamDestroy(c->stream_c2); }
  rccl_release(c);
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  if (c->ev_turn) {
    Turnstile& g = g_turnstile[(unsigned)c->device & 15u];
    std::lock_guard<std::mutex> tl(g.mu);
    if (g.owner == c) { g.last = nullptr; g.owner = nullptr; }      // (the streams were synchronised above: nobody waits on it any more)
    (void)hipEventDestroy(c->ev_turn);
  }
  (void)hipStreamDestroy(c->stream);
  (void)hipStreamDestroy(c->stream_h);
  (void)hipStreamDestroy(c->stream_d);
  delete c;
}

const char* bftkv_gpu_last_error(const bftkv_gpu_ctx* c) { return c ? c->err.c_str() : "null context"; }

const char* bftkv_gpu_error_string(int e) {
  switch (e) {
    case BFTKV_ERR_NONE: return "";
    case BFTKV_ERR_INVALID_SIGNATURE: return "crypto: invalid signature";                          // crypto/crypto.go:20
    case BFTKV_ERR_INSUFFICIENT_SIGNATURES: return "crypto: insufficient number of signatures";    // crypto/crypto.go:19
    default: return "unknown";
  }
}

void* bftkv_gpu_stream(bftkv_gpu_ctx* c) { return c ? (void*)c->stream : nullptr; }

int bftkv_gpu_sync(bftkv_gpu_ctx* c) {
  if (!c) return BFTKV_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int bftkv_gpu_set_host_pipeline(bftkv_gpu_ctx* c, uint32_t pieces) {
  const uint32_t mode = (pieces >> 8) & 3u, tight = (pieces >> 10) & 1u;
  if (!c || (pieces & 0xFFu) > HB_PIPE_MAX_PIECES || mode > 2 || (pieces >> 11)) return BFTKV_E_INVALID;
  pieces &= 0xFFu;
  ctx_lock lk(c->mu);
  c->hb_pieces = pieces;
  c->hb_copy_mode = mode;
  c->hb_tight = tight != 0;
  return 0;
}

int bftkv_gpu_host_pipeline_trace(bftkv_gpu_ctx* c, float* out, uint32_t cap, uint32_t* n_out) {
  if (!c || !n_out) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  *n_out = (uint32_t)c->hb_trace.size();
  if (out) copy_out(out, c->hb_trace.data(), sizeof(float) * std::min<size_t>(cap, c->hb_trace.size()));
  return 0;
}

int bftkv_gpu_set_early_exit(bftkv_gpu_ctx* c, int on) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  if (c->root) return fail(c, BFTKV_E_STATE, "set on the root context; its forks follow");
  KtWrite kw(c);
  c->early_exit = on != 0;
  return 0;
}

int bftkv_gpu_set_hash_policy(bftkv_gpu_ctx* c, int hash_id, int state) {
  if (!c || (hash_id != HASH_MD5 && hash_id != HASH_RIPEMD160) || state < 0 || state > 2) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  if (c->root) return fail(c, BFTKV_E_STATE, "set on the root context; its forks follow");
  KtWrite kw(c);
  const int sh = hash_id == HASH_MD5 ? 0 : 2;
  c->kt.hash_policy = (c->kt.hash_policy & ~(3u << sh)) | ((uint32_t)state << sh);
  ++c->keyring_gen;       // the forks copy the key-table descriptor when the generation moves
  return 0;
}

// widths the tables can be built at: 4 and every width from 8 to 20 (windows may straddle words); 17, 19 and 20 are for callers
// that pin them (19: 4.46 GB per key and 27 table multiplications, 20: 8.3 GB and 25 -- never chosen by the policy)
static bool dsa_width_ok(uint32_t bits) { return bits == 4 || (bits >= 8 && bits <= 20); }

int bftkv_gpu_set_dsa_window_bits(bftkv_gpu_ctx* c, uint32_t bits) {
  if (!c || (bits != 0 && !dsa_width_ok(bits))) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  c->dsa_wbits_pinned = bits;
  return 0;
}

int bftkv_gpu_set_dsa_table_budget(bftkv_gpu_ctx* c, uint64_t bytes) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  if (c->root) return fail(c, BFTKV_E_STATE, "a forked context cannot change the key table (use its root)");
  c->dsa_budget_bytes = (size_t)bytes;
  c->dsa_wbits_want = 0;          // the next upload re-evaluates the width (sync_dsa_tables)
  return 0;
}

int bftkv_gpu_dsa_table_bytes(bftkv_gpu_ctx* c, uint64_t* bytes_out, uint32_t* entry_limbs_out) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  const bftkv_gpu_ctx* r = c->root ? c->root : c;
  if (bytes_out) *bytes_out = (uint64_t)r->dsa_comb.cap;
  if (entry_limbs_out) *entry_limbs_out = r->dsa_entry_limbs;
  return 0;
}

int bftkv_gpu_dsa_window_bits(bftkv_gpu_ctx* c, uint32_t* bits_out) {
  if (!c || !bits_out) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  const bftkv_gpu_ctx* r = c->root ? c->root : c;      // (a fork verifies over its root's tables)
  *bits_out = r->dsa_comb_slot.empty() ? 0u : r->dsa_wbits;
  return 0;
}

int bftkv_gpu_keyring_set(bftkv_gpu_ctx* c, const bftkv_gpu_pubkey* keys, uint32_t n_keys) {
  if (!c || (!keys && n_keys)) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  if (c->root) return fail(c, BFTKV_E_STATE, "a forked context cannot change the key table (use its root)");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<KeyEntry> ring;
  for (uint32_t i = 0; i < n_keys; ++i) {
    KeyEntry e;
    int rc = make_key_entry(c, keys[i], false, &e);
    if (rc) return rc;
    // identical material under one id (the node's own key sits in both rings) is one row; DIFFERENT material under one
    // 64-bit id stays in the table in keyring order (KeysByIdUsage returns every candidate; ids can be made to collide with
    // ~2^32 work, so this must not take the keyring down): lookups take the first usable row and fence the item
    bool dup = false;
    for (auto& o : ring) {
      if (o.key_id == e.key_id) {
        if (o.material == e.material) { dup = true; break; }
        o.flags |= KEYF_AMBIGUOUS; e.flags |= KEYF_AMBIGUOUS;
      }
    }
    if (!dup) ring.push_back(std::move(e));
  }
  c->ring = std::move(ring);
  c->certs.clear();
  c->cert_valid.clear();
  ++c->cert_epoch;
  { std::unique_lock<std::shared_mutex> fl(c->cert_fast_mu); c->cert_fast.clear(); c->cert_fast_bytes = 0; }
  ++c->ring_epoch;
  return upload_key_table(c);
}

int bftkv_gpu_quorum_create(bftkv_gpu_ctx* c, const bftkv_gpu_qc* qcs, uint32_t n_qcs, int* out) {
  if (!c || !out || (!qcs && n_qcs)) return BFTKV_E_INVALID;
  if (n_qcs > MAX_QC) return fail(c, BFTKV_E_UNSUPPORTED, "more than MAX_QC cliques in one quorum");
  ctx_lock lk(c->mu);
  if (c->root) return fail(c, BFTKV_E_STATE, "quorums are created on the root context; its forks see them");
  HIPCHK(c, hipSetDevice(c->device));
  QuorumHost q;
  q.live = true;
  q.n_qcs = (int)n_qcs;
  std::vector<uint64_t> all;
  q.ids_off[0] = 0;
  for (uint32_t i = 0; i < n_qcs; ++i) {
    q.f[i] = qcs[i].f; q.mn[i] = qcs[i].min; q.thr[i] = qcs[i].threshold; q.suff[i] = qcs[i].suff;
    q.nodes.emplace_back(qcs[i].node_ids, qcs[i].node_ids + qcs[i].n_nodes);
    all.insert(all.end(), qcs[i].node_ids, qcs[i].node_ids + qcs[i].n_nodes);
    q.ids_off[i + 1] = (uint32_t)all.size();
  }
  // device copy: ids followed by the offsets (as uint32)
  std::vector<uint64_t> blob = all;
  size_t ids_words = blob.size();
  blob.resize(ids_words + (MAX_QC + 2) / 2 + 1, 0);
  memcpy(&blob[ids_words], q.ids_off, sizeof(uint32_t) * (n_qcs + 1));
  int rc = upload(c, q.ids, blob);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  q.ids_off[MAX_QC] = (uint32_t)ids_words;   // remember where the offsets live
  int h = -1;
  for (size_t i = 0; i < c->quorums.size(); ++i) if (!c->quorums[i].live) { h = (int)i; break; }
  KtWrite kw(c);
  if (h < 0) { c->quorums.emplace_back(); h = (int)c->quorums.size() - 1; }
  c->quorums[h] = std::move(q);
  ++c->quorum_gen;
  *out = h;
  return 0;
}

int bftkv_gpu_quorum_destroy(bftkv_gpu_ctx* c, int quorum) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  if (c->root) return fail(c, BFTKV_E_STATE, "quorums are destroyed on the root context");
  int rc = check_quorum(c, quorum);
  if (rc) return rc;
  KtWrite kw(c);
  c->quorums[quorum].member.release();
  c->quorums[quorum].ids.release();
  c->quorums[quorum] = QuorumHost();
  ++c->quorum_gen;
  return 0;
}

// `call`: the batch and how it arrives, as the caller prepared it; the plan (call.plan_q) is set here
static int collective_verify_impl(bftkv_gpu_ctx* c, int quorum, PipelineCall call, uint8_t* err_out, uint32_t* nver_out,
                                  uint8_t* verdict_out, uint8_t* fenced_out) {
  // caller holds c->mu
  const uint32_t n_items = call.n_items;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = check_quorum(c, quorum);
  if (rc) return rc;
  if (n_items == 0) return 0;
  QuorumHost& q = c->quorums[quorum];
  if ((rc = build_member(c, q))) return rc;
  const QuorumDev qd = quorum_dev(c, q);
  call.plan_q = c->early_exit ? &qd : nullptr;
  if ((rc = run_pipeline(c, call))) return rc;
  HIPCHK(c, c->o_nver.ensure(sizeof(uint32_t) * n_items));
  HIPCHK(c, c->o_verdict.ensure(n_items));
  uint32_t* nv = nver_out ? nver_out : c->o_nver.as<uint32_t>();
  uint8_t* vd = verdict_out ? verdict_out : c->o_verdict.as<uint8_t>();
  hipLaunchKernelGGL(k_tally, dim3((n_items + 3) / 4), dim3(256), 0, c->stream, c->recs.as<SigRec>(), c->base.as<uint32_t>(),
                     c->counts.as<uint32_t>(), n_items, c->kt, quorum_dev(c, q), vd, nv, (uint32_t*)nullptr);
  if (err_out) {
    // err = IsSufficient ? nil : ErrInsufficientNumberOfSignatures
    hipLaunchKernelGGL(k_err_from_verdict, dim3((n_items + 255) / 256), dim3(256), 0, c->stream, vd, n_items, err_out);
  }
  if (fenced_out)
    hipLaunchKernelGGL(k_fenced_out, dim3((n_items + 255) / 256), dim3(256), 0, c->stream, c->item_flags.as<uint8_t>(),
                       c->hash_mask.as<uint32_t>(), n_items, fenced_out);
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  HIPCHK(c, hipGetLastError());
  c->have_timing = true;
  return 0;
}

int bftkv_gpu_collective_verify_dev(bftkv_gpu_ctx* c, int quorum, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off,
                                    const uint8_t* ss, const uint64_t* ss_off, uint64_t ss_len, uint8_t* err_out,
                                    uint32_t* nver_out, uint8_t* verdict_out, uint8_t* fenced_out) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  PipelineCall call;
  call.n_items = n_items; call.d_tbs = tbs; call.d_tbs_off = tbs_off; call.d_ss = ss; call.d_ss_off = ss_off; call.ss_len = ss_len;
  return collective_verify_impl(c, quorum, call, err_out, nver_out, verdict_out, fenced_out);
}

// A big batch handed over in HOST memory (what the cgo shim and every C caller do: crypto_pgp.go:485-500, the caller owns
// the slices).  Copy, then verify, costs the sum of both; here the batch is cut into pieces of about equal signature bytes and
// piece k is walked, parsed, exponentiated and tallied while pieces k+1.. are still crossing PCIe:
//   * ONE copy of the input in this context's in_* buffers; a helper thread issues the copies piece by piece (signature
//     streams, then payloads) on stream_c -- hipMemcpyAsync from pageable memory returns only when the runtime has staged or
//     pinned the source, so the thread that issues copies cannot be the one that enqueues kernels -- and records an event behind each;
//   * piece k runs on its own private worker context (a fork of the root: own arena, streams and mailbox, the resident key
//     table shared) over pointers INTO those buffers (offset arrays advanced to the piece's first item: offsets are absolute);
//     its main stream waits for the piece's signature event, its hash stream for the payload event (the upload_tbs hook of
//     run_pipeline, i.e. after the modexp has been enqueued); the machine-filling modexps of the pieces take turns at the device
//     turnstile like any other calls in flight;
//   * results leave through pinned memory (a D2H copy into pageable memory would block the enqueuing thread until the piece is
//     done) and reach the caller's arrays after the one synchronisation at the end.
// Items are independent, so the verdicts are those of the unsplit call by construction (test_host_buffer_pipeline_*).

struct HbPiece { uint32_t i0, i1; };

// fail closed: no byte of the caller's result arrays reads as "verified" beside a non-zero return code
static void fail_closed(uint32_t n_items, uint8_t* err_out, uint32_t* nver_out, uint8_t* verdict_out, uint8_t* fenced_out) {
  if (err_out) memset(err_out, BFTKV_ERR_INSUFFICIENT_SIGNATURES, n_items);
  if (verdict_out) memset(verdict_out, 0, n_items);
  if (nver_out) memset(nver_out, 0, sizeof(uint32_t) * (size_t)n_items);
  if (fenced_out) memset(fenced_out, 0, n_items);
}

// Segmented payloads (bftkv_gpu_collective_verify_segments): payload i = prefix[prefix_off[i] .. prefix_off[i+1]) || shared segment
// seg[i] (0xFFFFFFFF: none).  Only the prefixes and each distinct segment cross PCIe; k_expand_segments lays the payloads out in
// in_tbs exactly as the unsegmented call receives them, on the copy stream, behind the copy of the piece's prefixes.
struct HbSeg { const uint8_t* prefix; const uint64_t* prefix_off; const uint8_t* shared; const uint64_t* shared_off; uint32_t n_shared; const uint32_t* seg; };

// One contiguous range of the caller's buffers on its way to the device: `half` 0 = signature streams, 1 = payloads of piece k.
struct HbCopy { uint32_t piece; int half; const uint8_t* src; uint8_t* dst; uint64_t len; };

static uint32_t hb_forced_pieces(const bftkv_gpu_ctx* c) {
  static const int env = getenv("BFTKV_HB_PIECES") ? atoi(getenv("BFTKV_HB_PIECES")) : 0;
  return c->hb_pieces ? c->hb_pieces : (uint32_t)std::max(env, 0);     // bftkv_gpu_set_host_pipeline, else the environment
}

static uint32_t hb_pieces_for(const bftkv_gpu_ctx* c, uint64_t bytes, uint32_t n_items) {
  const uint32_t forced = hb_forced_pieces(c);
  if (forced == 1) return 1;
  if (forced > 1) return std::max<uint32_t>(1, std::min<uint32_t>(std::min(forced, HB_PIPE_MAX_PIECES), n_items));
  if (bytes < HB_PIPE_MIN_BYTES || n_items < 64) return 1;
  const uint32_t p = (uint32_t)std::min<uint64_t>(HB_PIPE_MAX_PIECES, std::max<uint64_t>(2, bytes / (40ull << 20)));
  return std::min<uint32_t>(p, n_items / 16);
}

static int collective_verify_pipelined(bftkv_gpu_ctx* c, int quorum, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off,
                                       const uint8_t* ss, const uint64_t* ss_off, uint8_t* err_out, uint32_t* nver_out,
                                       uint8_t* verdict_out, uint8_t* fenced_out, uint32_t n_pieces, const HbSeg* sg = nullptr) {
  // caller holds c->mu and, on a fork, the root's key-table lock (shared)
  // sg: `tbs` is null, tbs_off are the offsets of the EXPANDED payloads (computed by the caller from sg)
  // One pipelined call per device COPIES at a time: such a call is bound by the PCIe link, which concurrent callers would only
  // share (three at once: 7.2 ms per call against 5.2 alone, their 45 streams queueing on the runtime's four hardware queues).
  // The turn ends when this call's last byte is on its way (copiers joined): the next caller's first pieces cross the link
  // while this call's last piece is still being verified.
  std::unique_lock<std::mutex> link_turn(g_hb_mu[(unsigned)c->device & 15u]);
  const auto t_call = std::chrono::steady_clock::now();
  auto us_now = [&] { return (float)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_call).count() * 1e-3f; };
  bftkv_gpu_ctx* const root = c->root ? c->root : c;
  int rc = check_quorum(c, quorum);
  if (rc) return rc;
  const uint64_t tl = tbs_off[n_items], sl = ss_off[n_items];
  // Pieces of equal bytes (signature streams + payloads), cut at item boundaries.  A piece's walk / parse / modexp / tally take
  // about 0.72 of the time its bytes take to cross PCIe (2.9 ms of work per 226 MB against 4.0 ms of copy) plus ~0.2 ms of
  // launches and dependent small kernels, so a piece of >= ~40 MB is done before the next one has arrived and the call ends one
  // such piece behind the last byte; smaller pieces fall behind the copy (their fixed part does not shrink), larger ones leave
  // more work for the end.  (A small LAST piece was tried: the piece before it is then large and late -- worse.)
  // (Round 6 measured a cut at whole modexp ROUNDS instead -- 768 blocks of 64 signatures are resident at a time, and a piece of 1.79
  // rounds pays for 2 -- and lost: the kernel's time steps by thirds of a round (a CU holds 3 blocks), an estimate that lands a piece
  // just past a boundary costs more than the rule saves; docs/history.md.)
  std::vector<HbPiece> pc;
  {
    const uint64_t* const poff = sg ? sg->prefix_off : tbs_off;       // bytes that cross the link per item
    const uint64_t total = poff[n_items] + sl;
    uint32_t i = 0;
    for (uint32_t k = 0; k < n_pieces && i < n_items; ++k) {
      const uint64_t want = total / n_pieces * (k + 1);
      uint32_t lo = i + 1, hi = n_items;
      while (lo < hi) { const uint32_t m = lo + (hi - lo) / 2; if (poff[m] + ss_off[m] < want) lo = m + 1; else hi = m; }
      const uint32_t j = (k + 1 == n_pieces) ? n_items : lo;
      pc.push_back({i, j});
      i = j;
    }
  }
  const uint32_t P = (uint32_t)pc.size();
  while (c->hb_workers.size() < P) {
    bftkv_gpu_ctx* w = nullptr;
    if ((rc = bftkv_gpu_init(c->device, &w))) return fail(c, rc, "host-buffer pipeline: worker context");
    w->root = root; w->dsa_inv_mode = root->dsa_inv_mode;
    if (const char* e = getenv("BFTKV_HB_MODEXP_LDS_PAD")) w->modexp_lds_pad = (uint32_t)atoi(e);
    root->n_forks.fetch_add(1);
    c->hb_workers.push_back(w);
  }
  if (!c->stream_c) {
    // Its own hardware queue, if the runtime has one to give: the runtime maps all streams of a priority level onto a few
    // hardware queues (4 by default), and the markers behind this stream's copies -- which the ring waits on before it reuses a
    // slot -- would otherwise sit behind whatever long kernel another stream put into the same queue.
    int lo_p = 0, hi_p = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
    static const bool prio = !getenv("BFTKV_HB_COPY_NO_PRIORITY");
    if (!prio || hipStreamCreateWithPriority(&c->stream_c, hipStreamNonBlocking, hi_p) != hipSuccess) { c->stream_c = nullptr; HIPCHK(c, hipStreamCreateWithFlags(&c->stream_c, hipStreamNonBlocking)); }
    if (!prio || hipStreamCreateWithPriority(&c->stream_c2, hipStreamNonBlocking, hi_p) != hipSuccess) { c->stream_c2 = nullptr; HIPCHK(c, hipStreamCreateWithFlags(&c->stream_c2, hipStreamNonBlocking)); }
  }
  while (c->hb_ev.size() < 2 * (size_t)P + 1) { hipEvent_t e; HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->hb_ev.push_back(e); }
  HIPCHK(c, c->in_tbs.ensure(tl + 64));
  HIPCHK(c, c->in_ss.ensure(sl + 64));
  HIPCHK(c, c->in_tbs_off.ensure(sizeof(uint64_t) * (n_items + 1)));
  HIPCHK(c, c->in_ss_off.ensure(sizeof(uint64_t) * (n_items + 1)));
  const size_t o_err = 0, o_vd = (size_t)n_items, o_fn = 2 * (size_t)n_items, o_nv = (3 * (size_t)n_items + 15) & ~(size_t)15;
  const size_t off_bytes = sizeof(uint64_t) * ((size_t)n_items + 1);
  const size_t o_toff = (o_nv + sizeof(uint32_t) * (size_t)n_items + 15) & ~(size_t)15, o_soff = o_toff + off_bytes;
  const size_t o_tot = o_soff + off_bytes;                  // per piece: [packet events, overflow] (k_scan_counts)
  // segmented calls: prefix offsets, item -> segment map, segment offsets and (when small) the segments themselves, staged likewise
  const uint64_t seg_shl = sg && sg->n_shared ? sg->shared_off[sg->n_shared] : 0;
  const bool seg_stage_blob = sg && seg_shl <= (4u << 20);
  const size_t o_poff = (o_tot + 8 * (size_t)HB_PIPE_MAX_PIECES + 15) & ~(size_t)15;
  const size_t o_seg = o_poff + (sg ? off_bytes : 0);
  const size_t o_shoff = (o_seg + (sg ? sizeof(uint32_t) * (size_t)n_items : 0) + 15) & ~(size_t)15;
  const size_t o_shb = o_shoff + (sg ? sizeof(uint64_t) * ((size_t)sg->n_shared + 1) : 0);
  const size_t out_bytes = o_shb + (seg_stage_blob ? (size_t)seg_shl : 0) + 16;
  if (c->hb_out_cap < out_bytes) {
    if (c->hb_out) { (void)hipHostFree(c->hb_out); c->hb_out = nullptr; c->hb_out_cap = 0; }
    HIPCHK(c, hipHostMalloc((void**)&c->hb_out, out_bytes + out_bytes / 4, hipHostMallocDefault));
    c->hb_out_cap = out_bytes + out_bytes / 4;
  }
  if (!c->hb_ev0) HIPCHK(c, hipEventCreate(&c->hb_ev0));
  HIPCHK(c, hipEventRecord(c->hb_ev0, c->stream_c));      // origin of the device-side times of the timeline
  // the offsets of the whole batch first (a few hundred KB, through pinned memory: asynchronous), then the pieces
  memcpy(c->hb_out + o_toff, tbs_off, off_bytes);
  memcpy(c->hb_out + o_soff, ss_off, off_bytes);
  HIPCHK(c, hipMemcpyAsync(c->in_tbs_off.p, c->hb_out + o_toff, off_bytes, hipMemcpyHostToDevice, c->stream_c));
  HIPCHK(c, hipMemcpyAsync(c->in_ss_off.p, c->hb_out + o_soff, off_bytes, hipMemcpyHostToDevice, c->stream_c));
  if (sg) {      // the distinct segments, the prefix offsets and the item -> segment map go first (a few hundred KB)
    const uint64_t shl = sg->n_shared ? sg->shared_off[sg->n_shared] : 0;
    HIPCHK(c, c->in_prefix.ensure(sg->prefix_off[n_items] + 64));
    HIPCHK(c, c->in_prefix_off.ensure(off_bytes));
    HIPCHK(c, c->in_shared.ensure(shl + 64));
    HIPCHK(c, c->in_shared_off.ensure(sizeof(uint64_t) * ((size_t)sg->n_shared + 1)));
    HIPCHK(c, c->in_seg.ensure(sizeof(uint32_t) * (size_t)n_items));
    // (through the pinned buffer like the offsets above: four copies from pageable memory cost 0.4 ms before the first piece moved)
    memcpy(c->hb_out + o_poff, sg->prefix_off, off_bytes);
    memcpy(c->hb_out + o_seg, sg->seg, sizeof(uint32_t) * (size_t)n_items);
    HIPCHK(c, hipMemcpyAsync(c->in_prefix_off.p, c->hb_out + o_poff, off_bytes, hipMemcpyHostToDevice, c->stream_c));
    HIPCHK(c, hipMemcpyAsync(c->in_seg.p, c->hb_out + o_seg, sizeof(uint32_t) * (size_t)n_items, hipMemcpyHostToDevice, c->stream_c));
    if (sg->n_shared) {
      memcpy(c->hb_out + o_shoff, sg->shared_off, sizeof(uint64_t) * ((size_t)sg->n_shared + 1));
      HIPCHK(c, hipMemcpyAsync(c->in_shared_off.p, c->hb_out + o_shoff, sizeof(uint64_t) * ((size_t)sg->n_shared + 1), hipMemcpyHostToDevice, c->stream_c));
    }
    if (shl && seg_stage_blob) {
      memcpy(c->hb_out + o_shb, sg->shared, shl);
      HIPCHK(c, hipMemcpyAsync(c->in_shared.p, c->hb_out + o_shb, shl, hipMemcpyHostToDevice, c->stream_c));
    } else if (shl) HIPCHK(c, hipMemcpyAsync(c->in_shared.p, sg->shared, shl, hipMemcpyHostToDevice, c->stream_c));
  }
  // Segmented: a piece's payloads are laid out by k_expand_segments on the piece's own HASH stream, once that stream has waited for
  // the copy of the piece's prefixes (payload_ready below) -- right where they are consumed.  (On the copy stream, behind the
  // copy, it held the DMA engine back: a kernel squeezed in beside a machine-filling modexp takes 0.3 ms, and the next copy of
  // that stream waits for it -- 43 GB/s over the call instead of 51.)
  auto expand_piece = [&](uint32_t k, hipStream_t st) {
    if (!sg) return;
    const uint32_t nk = pc[k].i1 - pc[k].i0;
    if (nk) hipLaunchKernelGGL(k_expand_segments, dim3((nk + 3) / 4), dim3(256), 0, st, c->in_prefix.as<uint8_t>(), c->in_prefix_off.as<uint64_t>(),
                               c->in_shared.as<uint8_t>(), c->in_shared_off.as<uint64_t>(), c->in_seg.as<uint32_t>(), c->in_tbs_off.as<uint64_t>(),
                               pc[k].i0, nk, c->in_tbs.as<uint8_t>());
  };
  // copy plan: piece 0's signature streams first (its modexp can start), then for every piece the payloads BEFORE the signature
  // streams of the next one -- when a piece's streams have arrived, everything of it has, and nothing waits for a payload
  std::vector<HbCopy> plan;
  for (uint32_t k = 0; k < P; ++k) {
    const uint64_t s0 = ss_off[pc[k].i0], s1 = ss_off[pc[k].i1], t0 = tbs_off[pc[k].i0], t1 = tbs_off[pc[k].i1];
    const HbCopy cs{k, 0, ss + s0, c->in_ss.as<uint8_t>() + s0, s1 - s0};
    const HbCopy ct = sg ? HbCopy{k, 1, sg->prefix + sg->prefix_off[pc[k].i0], c->in_prefix.as<uint8_t>() + sg->prefix_off[pc[k].i0],
                                  sg->prefix_off[pc[k].i1] - sg->prefix_off[pc[k].i0]}
                         : HbCopy{k, 1, tbs + t0, c->in_tbs.as<uint8_t>() + t0, t1 - t0};
    if (k == 0) { plan.push_back(cs); plan.push_back(ct); } else { plan.push_back(ct); plan.push_back(cs); }
  }
  std::vector<std::atomic<int>> flag(2 * (size_t)P);      // 1: the range is enqueued and its event recorded, -1: the copy failed
  for (auto& f : flag) f.store(0);
  std::atomic<int> copy_err{(int)hipSuccess};
  static const bool ring_env = getenv("BFTKV_HB_COPY") && !strcmp(getenv("BFTKV_HB_COPY"), "ring");
  const bool use_ring = c->hb_copy_mode ? c->hb_copy_mode == 1 : ring_env;
  std::vector<float>& tr = c->hb_trace;
  tr.assign(8 + HB_TR * (size_t)P, 0.f);
  tr[0] = (float)P; tr[1] = use_ring ? 1.f : 0.f;
  std::vector<std::thread> copiers;
  bool spawn_failed = false;
  // (a thread the system refuses must end the call with an error, not the process: the copiers' loops are written so that the
  // ones that did start finish by themselves once `dead` is set)
  auto try_spawn = [&](std::vector<std::thread>& v, auto&& fn) {
    if (spawn_failed) return;
    try { v.emplace_back(std::forward<decltype(fn)>(fn)); } catch (const std::system_error&) { spawn_failed = true; }
  };
  std::atomic<uint64_t> ticket{0};          // ring: the next chunk that may be enqueued
  std::atomic<bool> dead{false};
  // chunks of the plan, numbered in order
  struct Chunk { uint32_t range; uint64_t off, len; bool last; };
  std::vector<Chunk> chunks;
  if (use_ring) {
    if (!c->hb_ring) c->hb_ring = new HbRing();
    HbRing& R = *(HbRing*)c->hb_ring;
    hipError_t e = R.init();
    if (e != hipSuccess) return fail(c, BFTKV_E_DEVICE, "host-buffer pipeline: pinned ring", e);
    for (uint32_t r = 0; r < plan.size(); ++r) {
      if (plan[r].len == 0) { chunks.push_back({r, 0, 0, true}); continue; }
      // chunk sizes ramp up from 2 MB: the DMA engine starts after 70 us of copying, not after a whole slot's 0.5 ms
      for (uint64_t o = 0; o < plan[r].len;) {
        const uint64_t want = std::min<uint64_t>(HbRing::SLOT, (2ull << 20) << std::min<size_t>(3, chunks.size() / HbRing::THREADS));
        const uint64_t len = std::min<uint64_t>(want, plan[r].len - o);
        chunks.push_back({r, o, len, o + len >= plan[r].len});
        o += len;
      }
    }
    const int nth = (int)std::min<size_t>(HbRing::THREADS, chunks.size());
    for (int t = 0; t < nth; ++t)
      try_spawn(copiers, [&, t, nth] {
        (void)hipSetDevice(c->device);
        HbRing& R = *(HbRing*)c->hb_ring;
        for (uint64_t i = (uint64_t)t; i < chunks.size(); i += (uint64_t)nth) {
          const Chunk& ch = chunks[i];
          const HbCopy& cp = plan[ch.range];
          const int slot = (int)(i % HbRing::NSLOT);
          hipError_t e = hipSuccess;
          // chunk i - NSLOT used this slot: it was enqueued long ago (tickets are in order); wait for its DMA
          if (!dead.load() && i >= (uint64_t)HbRing::NSLOT) {
            while (ticket.load(std::memory_order_acquire) <= i - HbRing::NSLOT && !dead.load()) __builtin_ia32_pause();
            e = hipEventSynchronize(R.ev[slot]);
          }
          if (e == hipSuccess && !dead.load() && ch.len) memcpy(R.base + (size_t)slot * HbRing::SLOT, cp.src + ch.off, ch.len);
          while (ticket.load(std::memory_order_acquire) != i && !dead.load()) { if ((i & 7) == 7) std::this_thread::yield(); else __builtin_ia32_pause(); }
          if (e == hipSuccess && !dead.load()) {
            if (ch.len) e = hipMemcpyAsync(cp.dst + ch.off, R.base + (size_t)slot * HbRing::SLOT, ch.len, hipMemcpyHostToDevice, c->stream_c);
            if (e == hipSuccess) e = hipEventRecord(R.ev[slot], c->stream_c);
            if (e == hipSuccess && ch.last) e = hipEventRecord(c->hb_ev[2 * cp.piece + cp.half], c->stream_c);
          }
          if (e != hipSuccess) { copy_err.store((int)e); dead.store(true); }
          if (ch.last) { flag[2 * cp.piece + cp.half].store(dead.load() ? -1 : 1, std::memory_order_release); tr[8 + HB_TR * cp.piece + cp.half] = us_now(); }
          if (!dead.load()) ticket.store(i + 1, std::memory_order_release);
        }
      });
  } else {
    // Two helper threads take the ranges of the plan alternately, each on its own stream: a copy from pageable memory returns
    // when it is done, so one thread alone leaves the link idle between two calls.  A range's event says that THIS range is on
    // the device (the offsets went first, on stream_c: the thread of stream_c2 waits for them once).
    // (Measured, profiles/r04_host_pipeline_*: two copiers drain the link 0.2 ms sooner, but a piece's payloads and signature streams
    // then arrive together, the midstates lose their head start and run beside the previous piece's modexp: 5.35 against 5.25 ms.
    // One is the default.)
    static const int n_copiers = getenv("BFTKV_HB_COPIERS") ? std::max(1, std::min(2, atoi(getenv("BFTKV_HB_COPIERS")))) : 1;
    if (n_copiers > 1) { HIPCHK(c, hipEventRecord(c->hb_ev[2 * (size_t)P], c->stream_c)); HIPCHK(c, hipStreamWaitEvent(c->stream_c2, c->hb_ev[2 * (size_t)P], 0)); }
    for (int t = 0; t < n_copiers; ++t)
      try_spawn(copiers, [&, t] {
        (void)hipSetDevice(c->device);
        hipStream_t st = t == 0 ? c->stream_c : c->stream_c2;
        for (size_t r = (size_t)t; r < plan.size(); r += (size_t)n_copiers) {
          const HbCopy& cp = plan[r];
          hipError_t e = hipSuccess;
          if (!dead.load()) {
            if (cp.len) e = hipMemcpyAsync(cp.dst, cp.src, cp.len, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipEventRecord(c->hb_ev[2 * cp.piece + cp.half], st);
            if (e != hipSuccess) { copy_err.store((int)e); dead.store(true); }
          }
          flag[2 * cp.piece + cp.half].store(dead.load() ? -1 : 1, std::memory_order_release);
          tr[8 + HB_TR * cp.piece + cp.half] = us_now();
        }
      });
  }
  if (spawn_failed) {
    dead.store(true);        // (the copiers that did start leave their ticket waits on it)
    for (auto& f : flag) f.store(-1, std::memory_order_release);
    for (auto& t : copiers) t.join();
    (void)hipStreamSynchronize(c->stream_c);
    return fail(c, BFTKV_E_NOMEM, "host-buffer pipeline: cannot start a copier thread");
  }
  auto wait_flag = [&](size_t i) -> int {
    for (uint32_t it = 0;; ++it) {
      const int v = flag[i].load(std::memory_order_acquire);
      if (v) return v;
      if ((it & 63u) == 63u) std::this_thread::yield(); else __builtin_ia32_pause();
    }
  };
  int first_rc = 0;
  uint32_t launched = 0;
  // Arenas sized by the bound cost ~700 bytes per packet event; a call of gigabytes whose bound would take a third of the free
  // HBM sizes its pieces by their real counts instead (each piece then asks the host once in mid-pipeline, as an unsplit call does).
  bool use_cap = true;
  if (sl > (1ull << 30)) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || (sl / 64 + 8ull * n_items) * 700ull > free_b / 3) use_cap = false;
  }
  // range arrived?  1 yes, 0 not yet, -1 the copy failed.  ARRIVED, not merely enqueued: a piece enqueued ahead of its input
  // parks a barrier at the head of its streams' hardware queues, and those queues are shared -- the streams of the pieces
  // before it, whose input is there, would wait behind it (measured: every piece then finishes at the very end).  So the
  // host paces the pieces by the copy events.
  auto arrived = [&](size_t i) -> int {
    const int v = flag[i].load(std::memory_order_acquire);
    if (v <= 0) return v;
    const hipError_t q = hipEventQuery(c->hb_ev[i]);
    return q == hipSuccess ? 1 : q == hipErrorNotReady ? 0 : -1;
  };
  // Payload midstates start when the payloads arrive (they travel AHEAD of their piece's signature streams, see the plan): a
  // payload's hash is one chain of dependent compressions, ~0.45 ms whatever the piece's size, and would otherwise begin only
  // when the piece is picked up and end after its modexp.
  // MEASURED AND SWITCHED OFF (profiles/r04_host_pipeline_*): the early kernel of piece k+1 needs 142 VGPRs and finds no room
  // beside the three modexp waves per SIMD of piece k; it then sits at the head of a hardware queue it shares with piece k's
  // hash stream, whose digests -- and with them the piece's compare and tally -- wait behind it: +0.5..0.9 ms per piece, 5.7
  // against 5.2 ms per call.  BFTKV_HB_EARLY_MIDS=1 turns it on (it pays together with BFTKV_HB_MODEXP_LDS_PAD, two modexp waves per SIMD).
  static const bool early_mids_env = getenv("BFTKV_HB_EARLY_MIDS") && atoi(getenv("BFTKV_HB_EARLY_MIDS")) != 0;
  const bool early_mids = early_mids_env && !sg;        // (segmented payloads exist only behind the piece's payload hook)
  uint32_t next_mid = early_mids ? 1 : P;
  auto launch_early_mids = [&]() -> int {
    while (next_mid < P) {
      const int a = arrived(2 * (size_t)next_mid + 1);
      if (a < 0) return -1;
      if (a == 0) return 0;
      bftkv_gpu_ctx* w = c->hb_workers[next_mid];
      const uint32_t n = pc[next_mid].i1 - pc[next_mid].i0;
      if (w->mid.ensure(sizeof(uint32_t) * 8 * N_MID32 * (size_t)n + 16) != hipSuccess) return -1;
      hipLaunchKernelGGL(k_sha256_mid, dim3((n + MID_BLOCK - 1) / MID_BLOCK), dim3(MID_BLOCK), 0, w->stream_h, c->in_tbs.as<uint8_t>(), c->in_tbs_off.as<uint64_t>() + pc[next_mid].i0, n,
                         w->mid.as<uint32_t>());
      tr[8 + HB_TR * next_mid + 3] = us_now();
      ++next_mid;
    }
    return 0;
  };
  for (uint32_t k = 0; k < P && !first_rc; ++k) {
    bftkv_gpu_ctx* w = c->hb_workers[k];
    const uint32_t nk = pc[k].i1 - pc[k].i0;
    for (uint32_t it = 0;; ++it) {
      int a = launch_early_mids();
      if (a >= 0) a = arrived(2 * (size_t)k);
      if (a < 0) { first_rc = fail(c, BFTKV_E_DEVICE, "host-buffer pipeline: copy of the signature streams", (hipError_t)copy_err.load()); break; }
      if (a > 0) break;
      if ((it & 31u) == 31u) std::this_thread::yield(); else __builtin_ia32_pause();
    }
    if (first_rc) break;
    if (early_mids && k > 0 && next_mid <= k) {      // (cannot happen with the plan's order: payloads of piece k travel before its signature streams)
      for (uint32_t it = 0; launch_early_mids() == 0 && next_mid <= k; ++it) { if ((it & 31u) == 31u) std::this_thread::yield(); else __builtin_ia32_pause(); }
      if (next_mid <= k) { first_rc = fail(c, BFTKV_E_DEVICE, "host-buffer pipeline: copy of the payloads", (hipError_t)copy_err.load()); break; }
    }
    tr[8 + HB_TR * k + 2] = us_now();
    ctx_lock wl(w->mu);
    if ((rc = fork_refresh(w))) { first_rc = rc; break; }     // (the caller's locks already keep the root's tables still)
    const std::function<int(hipStream_t)> payload_ready = [&, k](hipStream_t sh) -> int {
      if (early_mids && k > 0) return 0;       // arrived long ago, midstates under way
      tr[8 + HB_TR * k + 3] = us_now();
      if (wait_flag(2 * k + 1) < 0) return fail(w, BFTKV_E_DEVICE, "host-buffer pipeline: copy of the payloads", (hipError_t)copy_err.load());
      hipError_t q;      // arrived (only piece 0's payloads travel behind its signature streams: see the copy plan), for the same reason
      for (uint32_t it = 0; (q = hipEventQuery(c->hb_ev[2 * k + 1])) == hipErrorNotReady; ++it) { if ((it & 31u) == 31u) std::this_thread::yield(); else __builtin_ia32_pause(); }
      if (q != hipSuccess) return fail(w, BFTKV_E_DEVICE, "host-buffer pipeline: payload copy event", q);
      HIPCHK(w, hipStreamWaitEvent(sh, c->hb_ev[2 * k + 1], 0));
      expand_piece(k, sh);
      return 0;
    };
    hipError_t e;
    if ((e = w->o_err.ensure(nk)) != hipSuccess || (e = w->o_fenced.ensure(nk)) != hipSuccess) { first_rc = fail(c, BFTKV_E_DEVICE, "host-buffer pipeline: result buffers", e); break; }
    // The piece is sized by an upper bound on its packet events (one per 64 stream bytes: 4.5 of the path's 287-byte signature
    // packets) and reads the real count on the device, so that this thread never waits for the GPU in mid-pipeline: every piece
    // is enqueued as soon as its copies are, and runs when its events fire.  A stream of junk denser than that turns the piece
    // into an empty one (k_scan_counts); it is then run again below, sized by its real count.
    const uint64_t ssk = ss_off[pc[k].i1] - ss_off[pc[k].i0];
    const uint32_t cap = !use_cap ? 0u
                         : c->hb_tight ? (uint32_t)(ssk / 4096 + 1)       // (tests: a bound that real streams exceed, to exercise the second pass)
                                       : (uint32_t)std::min<uint64_t>(1u << 26, ssk / 64 + 8ull * nk + 4096);
    PipelineCall piece;
    piece.n_items = nk; piece.d_tbs = c->in_tbs.as<uint8_t>(); piece.d_tbs_off = c->in_tbs_off.as<uint64_t>() + pc[k].i0;
    piece.d_ss = c->in_ss.as<uint8_t>(); piece.d_ss_off = c->in_ss_off.as<uint64_t>() + pc[k].i0; piece.ss_len = ssk;
    piece.upload_tbs = &payload_ready; piece.ev_input = c->hb_ev[2 * k]; piece.staged_cap = cap; piece.mid_prelaunched = early_mids && k > 0;
    rc = collective_verify_impl(w, quorum, piece, w->o_err.as<uint8_t>(), nullptr, nullptr, fenced_out ? w->o_fenced.as<uint8_t>() : nullptr);
    ++launched;
    if (rc) { c->err = "host-buffer pipeline, piece " + std::to_string(k) + ": " + w->err; first_rc = rc; break; }
    const uint32_t i0 = pc[k].i0;
    if ((e = hipMemcpyAsync(c->hb_out + o_err + i0, w->o_err.p, nk, hipMemcpyDeviceToHost, w->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->hb_out + o_vd + i0, w->o_verdict.p, nk, hipMemcpyDeviceToHost, w->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->hb_out + o_nv + sizeof(uint32_t) * (size_t)i0, w->o_nver.p, sizeof(uint32_t) * (size_t)nk, hipMemcpyDeviceToHost, w->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->hb_out + o_tot + 8 * (size_t)k, w->total.p, 8, hipMemcpyDeviceToHost, w->stream)) != hipSuccess ||
        (fenced_out && (e = hipMemcpyAsync(c->hb_out + o_fn + i0, w->o_fenced.p, nk, hipMemcpyDeviceToHost, w->stream)) != hipSuccess))
      first_rc = fail(c, BFTKV_E_DEVICE, "host-buffer pipeline: results to the host", e);
    tr[8 + HB_TR * k + 4] = us_now();
  }
  if (first_rc) dead.store(true);
  for (auto& t : copiers) t.join();
  link_turn.unlock();
  tr[2] = us_now();
  // one synchronisation: every piece that was enqueued, and the copy stream (the caller's buffers must not be read after return)
  hipError_t se = hipStreamSynchronize(c->stream_c);
  { const hipError_t e2 = hipStreamSynchronize(c->stream_c2); if (se == hipSuccess) se = e2; }
  tr[3] = us_now();
  for (uint32_t k = 0; k < launched; ++k) {
    bftkv_gpu_ctx* w = c->hb_workers[k];
    for (hipStream_t st : {w->stream_h, w->stream_d, w->stream}) { const hipError_t e = hipStreamSynchronize(st); if (se == hipSuccess) se = e; }
    tr[8 + HB_TR * k + 5] = us_now();
  }
  if (!first_rc && se != hipSuccess) first_rc = fail(c, BFTKV_E_DEVICE, "host-buffer pipeline: synchronise", se);
  // pieces that outgrew their bound: once more, sized by their real count (the input is on the device by now)
  for (uint32_t k = 0; k < P && !first_rc; ++k) {
    bftkv_gpu_ctx* w = c->hb_workers[k];
    uint32_t tot[2];
    memcpy(tot, c->hb_out + o_tot + 8 * (size_t)k, 8);
    if (use_cap) { w->last_total = tot[0]; w->last_total_on_dev = false; }
    if (!use_cap || !tot[1]) continue;
    ctx_lock wl(w->mu);
    const uint32_t nk = pc[k].i1 - pc[k].i0, i0 = pc[k].i0;
    PipelineCall piece;      // (its input is on the device: a resident call)
    piece.n_items = nk; piece.d_tbs = c->in_tbs.as<uint8_t>(); piece.d_tbs_off = c->in_tbs_off.as<uint64_t>() + i0;
    piece.d_ss = c->in_ss.as<uint8_t>(); piece.d_ss_off = c->in_ss_off.as<uint64_t>() + i0; piece.ss_len = ss_off[pc[k].i1] - ss_off[i0];
    rc = collective_verify_impl(w, quorum, piece, w->o_err.as<uint8_t>(), nullptr, nullptr, fenced_out ? w->o_fenced.as<uint8_t>() : nullptr);
    hipError_t e = hipSuccess;
    if (rc) { c->err = "host-buffer pipeline, piece " + std::to_string(k) + " (second pass): " + w->err; first_rc = rc; break; }
    if ((e = hipMemcpyAsync(c->hb_out + o_err + i0, w->o_err.p, nk, hipMemcpyDeviceToHost, w->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->hb_out + o_vd + i0, w->o_verdict.p, nk, hipMemcpyDeviceToHost, w->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->hb_out + o_nv + sizeof(uint32_t) * (size_t)i0, w->o_nver.p, sizeof(uint32_t) * (size_t)nk, hipMemcpyDeviceToHost, w->stream)) != hipSuccess ||
        (fenced_out && (e = hipMemcpyAsync(c->hb_out + o_fn + i0, w->o_fenced.p, nk, hipMemcpyDeviceToHost, w->stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(w->stream)) != hipSuccess)
      first_rc = fail(c, BFTKV_E_DEVICE, "host-buffer pipeline: second pass of a piece", e);
    tr[6] += 1.f;
  }
  if (first_rc) { fail_closed(n_items, err_out, nver_out, verdict_out, fenced_out); return first_rc; }
  if (err_out) memcpy(err_out, c->hb_out + o_err, n_items);
  if (verdict_out) memcpy(verdict_out, c->hb_out + o_vd, n_items);
  if (fenced_out) memcpy(fenced_out, c->hb_out + o_fn, n_items);
  if (nver_out) memcpy(nver_out, c->hb_out + o_nv, sizeof(uint32_t) * (size_t)n_items);
  c->hb_last_pieces = P;
  c->hb_item0.assign(P, 0);
  uint32_t total = 0;
  for (uint32_t k = 0; k < P; ++k) { c->hb_item0[k] = pc[k].i0; total += c->hb_workers[k]->last_total; }
  c->last_total = total;
  c->last_items = n_items;
  c->have_timing = false;       // (per-phase events live in the workers; bftkv_gpu_last_timing describes unsplit calls)
  tr[4] = us_now();
  for (uint32_t k = 0; k < P; ++k) {
    tr[5] = std::max(tr[5], (float)(pc[k].i1 - pc[k].i0));
    // device side, from the worker's own events (run_pipeline): input there and pipeline started, modexp's turn, modexp done, piece done
    bftkv_gpu_ctx* w = c->hb_workers[k];
    const int evs[4] = {0, 9, 2, 4};
    for (int j = 0; j < 4; ++j) { float ms = 0; if (hipEventElapsedTime(&ms, c->hb_ev0, w->ev[evs[j]]) == hipSuccess) tr[8 + HB_TR * k + 6 + j] = ms * 1e3f; }
  }
  return 0;
}

static int collective_verify_host(bftkv_gpu_ctx* c, int quorum, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off,
                                  const uint8_t* ss, const uint64_t* ss_off, uint8_t* err_out, uint32_t* nver_out,
                                  uint8_t* verdict_out, uint8_t* fenced_out, const HbSeg* sg = nullptr) {
  if (!c || (n_items && (!ss_off || (!sg && !tbs_off)))) return BFTKV_E_INVALID;
  if (sg && n_items && (!sg->prefix_off || !sg->seg || (sg->n_shared && (!sg->shared_off || (!sg->shared && sg->shared_off[sg->n_shared]))))) return BFTKV_E_INVALID;
  if (n_items == 0) return 0;
  ctx_lock lk(c->mu);      // one lock for copy-in, pipeline and copy-out: callers may share a context
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  HIPCHK(c, hipSetDevice(c->device));
  int rco;
  std::vector<uint64_t> toff_seg;        // segmented: the offsets of the payloads as the device lays them out
  if (sg) {
    if ((rco = check_offsets(c, sg->prefix_off, n_items, "prefix_off not monotone from 0"))) return rco;
    if (sg->n_shared && (rco = check_offsets(c, sg->shared_off, sg->n_shared, "shared_off not monotone from 0"))) return rco;
    toff_seg.resize((size_t)n_items + 1);
    toff_seg[0] = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
      const uint32_t g = sg->seg[i];
      if (g != 0xFFFFFFFFu && g >= sg->n_shared) return fail(c, BFTKV_E_INVALID, "segment index beyond n_shared");
      toff_seg[i + 1] = toff_seg[i] + (sg->prefix_off[i + 1] - sg->prefix_off[i]) + (g == 0xFFFFFFFFu ? 0 : sg->shared_off[g + 1] - sg->shared_off[g]);
    }
    tbs_off = toff_seg.data();
  }
  if ((rco = check_offsets(c, tbs_off, n_items, "tbs_off not monotone from 0")) || (rco = check_offsets(c, ss_off, n_items, "ss_off not monotone from 0")))
    return rco;
  const uint64_t tl = tbs_off[n_items], sl = ss_off[n_items];
  const uint64_t link_bytes = (sg ? sg->prefix_off[n_items] : tl) + sl;       // what crosses PCIe decides whether the call is cut into pieces
  if (const uint32_t pieces = hb_pieces_for(c, link_bytes, n_items); pieces > 1)
    return collective_verify_pipelined(c, quorum, n_items, tbs, tbs_off, ss, ss_off, err_out, nver_out, verdict_out, fenced_out, pieces, sg);
  HIPCHK(c, c->in_tbs.ensure(tl + 64));
  HIPCHK(c, c->in_ss.ensure(sl + 64));
  HIPCHK(c, c->in_tbs_off.ensure(sizeof(uint64_t) * (n_items + 1)));
  HIPCHK(c, c->in_ss_off.ensure(sizeof(uint64_t) * (n_items + 1)));
  HIPCHK(c, c->o_err.ensure(n_items));
  HIPCHK(c, c->o_nver.ensure(sizeof(uint32_t) * n_items));
  HIPCHK(c, c->o_verdict.ensure(n_items));
  HIPCHK(c, c->o_fenced.ensure(n_items));
  // the signature streams and the offsets first: the walk, the parse and the modexp need nothing else
  if (sl) HIPCHK(c, hipMemcpyAsync(c->in_ss.p, ss, sl, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->in_tbs_off.p, tbs_off, sizeof(uint64_t) * (n_items + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->in_ss_off.p, ss_off, sizeof(uint64_t) * (n_items + 1), hipMemcpyHostToDevice, c->stream));
  // the signed payloads go over PCIe while the modexp runs (run_pipeline calls this once the modexp is launched)
  const std::function<int(hipStream_t)> upload_tbs = [&](hipStream_t sh) -> int {
    if (!sg) {
      if (tl) HIPCHK(c, hipMemcpyAsync(c->in_tbs.p, tbs, tl, hipMemcpyHostToDevice, sh));
      return 0;
    }
    // segmented: prefixes, the distinct segments and the map, then the payloads laid out on the device (in_tbs_off went ahead on the
    // main stream: this stream waits for it)
    const uint64_t pl = sg->prefix_off[n_items], shl = sg->n_shared ? sg->shared_off[sg->n_shared] : 0;
    const size_t off_bytes = sizeof(uint64_t) * ((size_t)n_items + 1);
    HIPCHK(c, c->in_prefix.ensure(pl + 64));
    HIPCHK(c, c->in_prefix_off.ensure(off_bytes));
    HIPCHK(c, c->in_shared.ensure(shl + 64));
    HIPCHK(c, c->in_shared_off.ensure(sizeof(uint64_t) * ((size_t)sg->n_shared + 1)));
    HIPCHK(c, c->in_seg.ensure(sizeof(uint32_t) * (size_t)n_items));
    if (pl) HIPCHK(c, hipMemcpyAsync(c->in_prefix.p, sg->prefix, pl, hipMemcpyHostToDevice, sh));
    HIPCHK(c, hipMemcpyAsync(c->in_prefix_off.p, sg->prefix_off, off_bytes, hipMemcpyHostToDevice, sh));
    if (shl) HIPCHK(c, hipMemcpyAsync(c->in_shared.p, sg->shared, shl, hipMemcpyHostToDevice, sh));
    if (sg->n_shared) HIPCHK(c, hipMemcpyAsync(c->in_shared_off.p, sg->shared_off, sizeof(uint64_t) * ((size_t)sg->n_shared + 1), hipMemcpyHostToDevice, sh));
    HIPCHK(c, hipMemcpyAsync(c->in_seg.p, sg->seg, sizeof(uint32_t) * (size_t)n_items, hipMemcpyHostToDevice, sh));
    if (!c->seg_ev) HIPCHK(c, hipEventCreateWithFlags(&c->seg_ev, hipEventDisableTiming));
    HIPCHK(c, hipStreamWaitEvent(sh, c->seg_ev, 0));
    hipLaunchKernelGGL(k_expand_segments, dim3((n_items + 3) / 4), dim3(256), 0, sh, c->in_prefix.as<uint8_t>(), c->in_prefix_off.as<uint64_t>(),
                       c->in_shared.as<uint8_t>(), c->in_shared_off.as<uint64_t>(), c->in_seg.as<uint32_t>(), c->in_tbs_off.as<uint64_t>(), 0u, n_items,
                       c->in_tbs.as<uint8_t>());
    return 0;
  };
  if (sg) {      // (the offsets are on the main stream: the hash stream's expansion kernel must see them)
    if (!c->seg_ev) HIPCHK(c, hipEventCreateWithFlags(&c->seg_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->seg_ev, c->stream));
  }
  PipelineCall call;
  call.n_items = n_items; call.d_tbs = c->in_tbs.as<uint8_t>(); call.d_tbs_off = c->in_tbs_off.as<uint64_t>();
  call.d_ss = c->in_ss.as<uint8_t>(); call.d_ss_off = c->in_ss_off.as<uint64_t>(); call.ss_len = sl; call.upload_tbs = &upload_tbs;
  int rc = collective_verify_impl(c, quorum, call, c->o_err.as<uint8_t>(), c->o_nver.as<uint32_t>(), c->o_verdict.as<uint8_t>(),
                                  fenced_out ? c->o_fenced.as<uint8_t>() : nullptr);
  if (rc) return rc;
  if (fenced_out) HIPCHK(c, hipMemcpyAsync(fenced_out, c->o_fenced.p, n_items, hipMemcpyDeviceToHost, c->stream));
  if (err_out) HIPCHK(c, hipMemcpyAsync(err_out, c->o_err.p, n_items, hipMemcpyDeviceToHost, c->stream));
  if (nver_out) HIPCHK(c, hipMemcpyAsync(nver_out, c->o_nver.p, sizeof(uint32_t) * n_items, hipMemcpyDeviceToHost, c->stream));
  if (verdict_out) HIPCHK(c, hipMemcpyAsync(verdict_out, c->o_verdict.p, n_items, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int bftkv_gpu_collective_verify(bftkv_gpu_ctx* c, int quorum, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off,
                                const uint8_t* ss, const uint64_t* ss_off, uint8_t* err_out, uint32_t* nver_out,
                                uint8_t* verdict_out, uint8_t* fenced_out) {
  const int rc = collective_verify_host(c, quorum, n_items, tbs, tbs_off, ss, ss_off, err_out, nver_out, verdict_out, fenced_out);
  if (rc && n_items) fail_closed(n_items, err_out, nver_out, verdict_out, fenced_out);      // on EVERY path
  return rc;
}

int bftkv_gpu_collective_verify_segments(bftkv_gpu_ctx* c, int quorum, uint32_t n_items, const uint8_t* prefix, const uint64_t* prefix_off,
                                         const uint8_t* shared, const uint64_t* shared_off, uint32_t n_shared, const uint32_t* seg_of_item,
                                         const uint8_t* ss, const uint64_t* ss_off, uint8_t* err_out, uint32_t* nver_out,
                                         uint8_t* verdict_out, uint8_t* fenced_out) {
  const HbSeg sg{prefix, prefix_off, shared, shared_off, n_shared, seg_of_item};
  const int rc = collective_verify_host(c, quorum, n_items, nullptr, nullptr, ss, ss_off, err_out, nver_out, verdict_out, fenced_out, &sg);
  if (rc && n_items) fail_closed(n_items, err_out, nver_out, verdict_out, fenced_out);
  return rc;
}

// Signature.Verify over a batch with the keyring of item i restricted to entity index ent[i] (0xFFFFFFFF: the node
// keyring).  Shared by bftkv_gpu_signature_verify and the Server.sign site of the host mirror.
int signature_verify_entities(bftkv_gpu_ctx* c, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off, const uint8_t* sig,
                              const uint64_t* sig_off, const uint32_t* ent, uint8_t* err_out, const uint8_t* sig_class, uint8_t* fenced_out,
                              const uint64_t* forced_issuer) {
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  HIPCHK(c, hipSetDevice(c->device));
  int rco;
  if ((rco = check_offsets(c, tbs_off, n_items, "tbs_off not monotone from 0")) || (rco = check_offsets(c, sig_off, n_items, "sig_off not monotone from 0")))
    return rco;
  const uint64_t tl = tbs_off[n_items], sl = sig_off[n_items];
  HIPCHK(c, c->in_tbs.ensure(tl + 64));
  HIPCHK(c, c->in_ss.ensure(sl + 64));
  HIPCHK(c, c->in_tbs_off.ensure(sizeof(uint64_t) * (n_items + 1)));
  HIPCHK(c, c->in_ss_off.ensure(sizeof(uint64_t) * (n_items + 1)));
  HIPCHK(c, c->o_err.ensure(n_items));
  if (tl) HIPCHK(c, hipMemcpyAsync(c->in_tbs.p, tbs, tl, hipMemcpyHostToDevice, c->stream));
  if (sl) HIPCHK(c, hipMemcpyAsync(c->in_ss.p, sig, sl, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->in_tbs_off.p, tbs_off, sizeof(uint64_t) * (n_items + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->in_ss_off.p, sig_off, sizeof(uint64_t) * (n_items + 1), hipMemcpyHostToDevice, c->stream));
  const uint32_t* d_cert = nullptr;
  if (ent) {
    HIPCHK(c, c->cert_ent.ensure(sizeof(uint32_t) * n_items));
    HIPCHK(c, hipMemcpyAsync(c->cert_ent.p, ent, sizeof(uint32_t) * n_items, hipMemcpyHostToDevice, c->stream));
    d_cert = c->cert_ent.as<uint32_t>();
  }
  const uint8_t* d_cls = nullptr;
  if (sig_class) {
    HIPCHK(c, c->sig_class.ensure(n_items + 16));
    HIPCHK(c, hipMemcpyAsync(c->sig_class.p, sig_class, n_items, hipMemcpyHostToDevice, c->stream));
    d_cls = c->sig_class.as<uint8_t>();
  }
  const uint64_t* d_forced = nullptr;
  if (forced_issuer && sig_class) {     // certificate checks: the key the caller holds for each check (ParseArgs::forced_issuer)
    HIPCHK(c, c->forced_iss.ensure(sizeof(uint64_t) * n_items + 16));
    HIPCHK(c, hipMemcpyAsync(c->forced_iss.p, forced_issuer, sizeof(uint64_t) * n_items, hipMemcpyHostToDevice, c->stream));
    d_forced = c->forced_iss.as<uint64_t>();
  }
  PipelineCall call;
  call.n_items = n_items; call.d_tbs = c->in_tbs.as<uint8_t>(); call.d_tbs_off = c->in_tbs_off.as<uint64_t>();
  call.d_ss = c->in_ss.as<uint8_t>(); call.d_ss_off = c->in_ss_off.as<uint64_t>(); call.ss_len = sl;
  call.d_cert_ent = d_cert; call.d_sig_class = d_cls; call.d_forced_issuer = d_forced;
  int rc = run_pipeline(c, call);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sigverify_fold, dim3((n_items + 255) / 256), dim3(256), 0, c->stream, c->recs.as<SigRec>(),
                     c->base.as<uint32_t>(), c->counts.as<uint32_t>(), c->item_flags.as<uint8_t>(), n_items, c->o_err.as<uint8_t>());
  if (fenced_out) {
    HIPCHK(c, c->o_fenced.ensure(n_items));
    hipLaunchKernelGGL(k_fenced_out, dim3((n_items + 255) / 256), dim3(256), 0, c->stream, c->item_flags.as<uint8_t>(),
                       c->hash_mask.as<uint32_t>(), n_items, c->o_fenced.as<uint8_t>());
    HIPCHK(c, hipMemcpyAsync(fenced_out, c->o_fenced.p, n_items, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  HIPCHK(c, hipMemcpyAsync(err_out, c->o_err.p, n_items, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  c->have_timing = true;
  return 0;
}

int bftkv_gpu_signature_verify(bftkv_gpu_ctx* c, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off,
                               const uint8_t* sig, const uint64_t* sig_off, const uint64_t* cert_key_id, uint8_t* err_out,
                               uint8_t* fenced_out) {
  if (!c || (n_items && (!tbs_off || !sig_off || !err_out))) return BFTKV_E_INVALID;
  if (n_items == 0) return 0;
  std::vector<uint32_t> ce;
  ctx_lock lk(c->mu);      // entity indices resolved here stay valid until the pipeline has consumed them
  KtRead kr(c);            // (shared locks nest: signature_verify_entities takes it again)
  if (kr.rc) return kr.rc;
  if (cert_key_id) {
    ce.resize(n_items);
    for (uint32_t i = 0; i < n_items; ++i) {
      uint32_t e = 0xFFFFFFFEu;   // an entity that is not in the table: nothing matches
      for (uint32_t k = 0; k < c->n_entities; ++k) if (c->h_entity_id[k] == cert_key_id[i]) { e = k; break; }
      ce[i] = e;
    }
  }
  int rc = signature_verify_entities(c, n_items, tbs, tbs_off, sig, sig_off, cert_key_id ? ce.data() : nullptr, err_out, nullptr, fenced_out);
  // a certificate whose entity the device table does not hold: the library cannot speak for the reference (which verifies
  // against the certificate it is handed) -- reported as fenced, never as a verdict
  if (!rc && fenced_out && cert_key_id)
    for (uint32_t i = 0; i < n_items; ++i) if (ce[i] == 0xFFFFFFFEu) fenced_out[i] = 1;
  return rc;
}

int bftkv_gpu_last_statuses(bftkv_gpu_ctx* c, uint8_t* st, uint32_t* item, uint32_t cap, uint32_t* n_out) {
  if (!c || !n_out) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  if (c->last_total_on_dev && !c->hb_last_pieces) {
    HIPCHK(c, hipMemcpy(&c->last_total, c->total.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    c->last_total_on_dev = false;
  }
  *n_out = c->last_total;
  if (c->hb_last_pieces) {      // the last call ran pipelined: the records live in the workers, piece after piece
    uint32_t done = 0;
    for (uint32_t k = 0; k < c->hb_last_pieces && st && done < cap; ++k) {
      uint32_t nk = 0;
      const int rc = bftkv_gpu_last_statuses(c->hb_workers[k], st + done, item ? item + done : nullptr, cap - done, &nk);
      if (rc) return fail(c, rc, c->hb_workers[k]->err.c_str());
      nk = std::min(nk, cap - done);
      if (item) for (uint32_t j = 0; j < nk; ++j) item[done + j] += c->hb_item0[k];
      done += nk;
    }
    return 0;
  }
  uint32_t n = c->last_total < cap ? c->last_total : cap;
  if (!n || !st) return 0;
  HIPCHK(c, c->st_tmp.ensure(n));
  HIPCHK(c, c->item_tmp.ensure(sizeof(uint32_t) * n));
  hipLaunchKernelGGL(k_export_status, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->recs.as<SigRec>(), n,
                     c->st_tmp.as<uint8_t>(), c->item_tmp.as<uint32_t>());
  HIPCHK(c, hipMemcpyAsync(st, c->st_tmp.p, n, hipMemcpyDeviceToHost, c->stream));
  if (item) HIPCHK(c, hipMemcpyAsync(item, c->item_tmp.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int bftkv_gpu_last_counters(bftkv_gpu_ctx* c, uint64_t counters[4]) {
  if (!c || !counters) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  uint32_t cnt[4] = {0, 0, 0, 0};
  if (c->hb_last_pieces) {
    for (uint32_t k = 0; k < c->hb_last_pieces; ++k) {
      uint32_t ck[4] = {0, 0, 0, 0};
      if (c->hb_workers[k]->pk_count.p) HIPCHK(c, hipMemcpy(ck, c->hb_workers[k]->pk_count.p, 16, hipMemcpyDeviceToHost));
      for (int j = 0; j < 4; ++j) cnt[j] += ck[j];
    }
  } else
  if (c->pk_count.p) HIPCHK(c, hipMemcpy(cnt, c->pk_count.p, 16, hipMemcpyDeviceToHost));
  counters[0] = c->last_total;
  counters[1] = (uint64_t)cnt[0] + cnt[1] + cnt[2] + cnt[3];
  counters[2] = c->last_items;
  counters[3] = cnt[1];
  return 0;
}

int bftkv_gpu_last_sclk_mhz(bftkv_gpu_ctx* c, float* mhz) {
  if (!c || !mhz) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  uint64_t v[2] = {0, 0};
  if (c->pk_count.p) HIPCHK(c, hipMemcpy(v, (const char*)c->pk_count.p + 64, 16, hipMemcpyDeviceToHost));
  *mhz = v[1] ? (float)((double)v[0] / (double)v[1] * 100.0) : 0.0f;
  return 0;
}

int bftkv_gpu_last_plan_report(bftkv_gpu_ctx* c, uint32_t* out, uint32_t cap, uint32_t* n_out) {
  if (!c || !n_out || (cap && !out)) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  if (!c->have_plan_report) return fail(c, BFTKV_E_STATE, "the last call was not sized by a plan report");
  *n_out = plan_report::N_SLOTS;
  for (uint32_t k = 0; k < cap && k < (uint32_t)plan_report::N_SLOTS; ++k) out[k] = c->last_plan_report[k];
  return 0;
}

int bftkv_gpu_last_timing(bftkv_gpu_ctx* c, float ms[8]) {
  if (!c || !ms) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  if (!c->have_timing) return fail(c, BFTKV_E_STATE, "no timed call yet");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->ev[4]));
  for (int i = 0; i < 8; ++i) ms[i] = 0;
  HIPCHK(c, hipEventElapsedTime(&ms[0], c->ev[0], c->ev[4]));   // whole call
  HIPCHK(c, hipEventElapsedTime(&ms[1], c->ev[0], c->ev[1]));   // walk + scan + parse (incl. the host read of the count)
  HIPCHK(c, hipEventElapsedTime(&ms[2], c->ev[5], c->ev[6]));   // hash stream: midstates + digests (overlaps the modexp)
  HIPCHK(c, hipEventElapsedTime(&ms[3], c->ev[9], c->ev[2]));   // k_rsa_modexp on its own stream (from its turn at the turnstile)
  HIPCHK(c, hipEventElapsedTime(&ms[4], c->ev[3], c->ev[4]));   // tally
  HIPCHK(c, hipEventElapsedTime(&ms[5], c->ev[2], c->ev[8]));   // compare (incl. waiting for the hash stream)
  HIPCHK(c, hipEventElapsedTime(&ms[6], c->ev[8], c->ev[3]));   // k_dsa_mul + k_dsa_modexp (0 without DSA keys)
  return 0;
}

int bftkv_gpu_quorum_tally(bftkv_gpu_ctx* c, int quorum, uint32_t n_lists, const uint64_t* ids, const uint64_t* list_off,
                           uint8_t* verdict_out) {
  if (!c || (n_lists && (!list_off || !verdict_out))) return BFTKV_E_INVALID;
  if (n_lists == 0) return 0;
  ctx_lock lk(c->mu);
  if (c->root) return fail(c, BFTKV_E_STATE, "bftkv_gpu_quorum_tally runs on the root context");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = check_quorum(c, quorum);
  if (rc) return rc;
  QuorumHost& q = c->quorums[quorum];
  if ((rc = check_offsets(c, list_off, n_lists, "list_off not monotone from 0"))) return rc;
  const uint64_t n_ids = list_off[n_lists];
  HIPCHK(c, c->in_ss.ensure(sizeof(uint64_t) * (n_ids + 1)));
  HIPCHK(c, c->in_ss_off.ensure(sizeof(uint64_t) * (n_lists + 1)));
  HIPCHK(c, c->o_verdict.ensure(n_lists));
  if (n_ids) HIPCHK(c, hipMemcpyAsync(c->in_ss.p, ids, sizeof(uint64_t) * n_ids, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->in_ss_off.p, list_off, sizeof(uint64_t) * (n_lists + 1), hipMemcpyHostToDevice, c->stream));
  QuorumDev qd = quorum_dev(c, q);
  const uint64_t* d_ids = q.ids.as<uint64_t>();
  const uint32_t* d_off = (const uint32_t*)(d_ids + q.ids_off[MAX_QC]);
  hipLaunchKernelGGL(k_tally_ids, dim3((n_lists + 3) / 4), dim3(256), 0, c->stream, c->in_ss.as<uint64_t>(),
                     c->in_ss_off.as<uint64_t>(), n_lists, d_ids, d_off, qd, c->o_verdict.as<uint8_t>());
  HIPCHK(c, hipMemcpyAsync(verdict_out, c->o_verdict.p, n_lists, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return 0;
}

int bftkv_gpu_signers(bftkv_gpu_ctx* c, uint32_t n_items, const uint8_t* ss, const uint64_t* ss_off, uint64_t* ids_out,
                      uint64_t* ids_off_out, uint64_t cap) {
  return bftkv_gpu_signers_fenced(c, n_items, ss, ss_off, ids_out, ids_off_out, cap, nullptr);
}

int bftkv_gpu_signers_fenced(bftkv_gpu_ctx* c, uint32_t n_items, const uint8_t* ss, const uint64_t* ss_off, uint64_t* ids_out,
                             uint64_t* ids_off_out, uint64_t cap, uint8_t* fenced_out) {
  // parse-only walk: reuse the parse kernels with no hashing; issuers resolved against PRIMARY
  // key ids only (getCertById, crypto_pgp.go:206-219).
  if (!c || (n_items && (!ss_off || !ids_off_out))) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  HIPCHK(c, hipSetDevice(c->device));
  ids_off_out[0] = 0;
  if (n_items == 0) return 0;
  hipStream_t s = c->stream;
  { int rco = check_offsets(c, ss_off, n_items, "ss_off not monotone from 0"); if (rco) return rco; }
  const uint64_t sl = ss_off[n_items];
  HIPCHK(c, c->in_ss.ensure(sl + 64));
  HIPCHK(c, c->in_ss_off.ensure(sizeof(uint64_t) * (n_items + 1)));
  if (sl) HIPCHK(c, hipMemcpyAsync(c->in_ss.p, ss, sl, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->in_ss_off.p, ss_off, sizeof(uint64_t) * (n_items + 1), hipMemcpyHostToDevice, s));
  HIPCHK(c, c->counts.ensure(sizeof(uint32_t) * (n_items + 1)));
  HIPCHK(c, c->base.ensure(sizeof(uint32_t) * (n_items + 1)));
  HIPCHK(c, c->total.ensure(16));
  const uint32_t nb = (n_items + 63) / 64;
  if (fenced_out) HIPCHK(c, c->o_fenced.ensure(n_items));
  hipLaunchKernelGGL(k_signers<false>, dim3(nb), dim3(64), 0, s, c->in_ss.as<uint8_t>(), c->in_ss_off.as<uint64_t>(), n_items,
                     c->counts.as<uint32_t>(), (const uint32_t*)nullptr, (uint64_t*)nullptr, c->kt, fenced_out ? c->o_fenced.as<uint8_t>() : (uint8_t*)nullptr);
  if (fenced_out) HIPCHK(c, hipMemcpyAsync(fenced_out, c->o_fenced.p, n_items, hipMemcpyDeviceToHost, s));
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, c->counts.as<uint32_t>(), n_items, c->base.as<uint32_t>(),
                     c->total.as<uint32_t>(), (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (uint32_t*)nullptr);
  uint32_t total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, c->total.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (total > cap) return fail(c, BFTKV_E_NOMEM, "ids_out too small");
  HIPCHK(c, c->ids_tmp.ensure(sizeof(uint64_t) * (total + 1)));
  hipLaunchKernelGGL(k_signers<true>, dim3(nb), dim3(64), 0, s, c->in_ss.as<uint8_t>(), c->in_ss_off.as<uint64_t>(), n_items,
                     c->counts.as<uint32_t>(), c->base.as<uint32_t>(), c->ids_tmp.as<uint64_t>(), c->kt, (uint8_t*)nullptr);
  std::vector<uint32_t> hb(n_items);
  HIPCHK(c, hipMemcpyAsync(hb.data(), c->base.p, sizeof(uint32_t) * n_items, hipMemcpyDeviceToHost, s));
  if (total && ids_out) HIPCHK(c, hipMemcpyAsync(ids_out, c->ids_tmp.p, sizeof(uint64_t) * total, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  for (uint32_t i = 0; i < n_items; ++i) ids_off_out[i] = hb[i];
  ids_off_out[n_items] = total;
  return 0;
}

// bftkv_gpu_modexp / bftkv_gpu_modexp_ops: threshold_capi.inc (pooled temporaries, cached Montgomery tables)

}  // extern "C"

#include "../../include/bftkv_host.h"
// Issuer(sig) + VerifyWithCertificate over request certificates (host_capi.inc cert_signature_core; used by the batcher too)
struct CertSigReq { const uint8_t* cert; uint64_t cert_len; const uint8_t* tbs; uint64_t tbs_len; const uint8_t* sig; uint64_t sig_len; };
struct CertSigRes { uint8_t err = BFTKV_ERR_CERTIFICATE_NOT_FOUND; uint64_t issuer_id = 0; uint32_t n_entities = 0; std::vector<uint64_t> certifiers; };
int cert_signature_core(bftkv_gpu_ctx* ctx, const std::vector<CertSigReq>& reqs, std::vector<CertSigRes>* res);
extern "C" int bftkv_host_cert_fingerprint(const uint8_t* cert, uint64_t len, uint8_t out[20]);

#include "rccl_capi.inc"
#include "threshold_capi.inc"
#include "ec_capi.inc"
#include "dsa_verify_capi.inc"
#include "dsa_keyset_capi.inc"
#include "rsa_verify_capi.inc"
#include "tpa_capi.inc"
#include "rsa_psign_capi.inc"
#include "tsig_share_capi.inc"
#include "rsa_sign_capi.inc"
#include "message_capi.inc"
#include "batcher_capi.inc"
#include "host_capi.inc"
