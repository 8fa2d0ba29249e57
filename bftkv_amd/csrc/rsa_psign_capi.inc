// C ABI of threshold RSA signing, the server's side (include/bftkv_gpu.h: bftkv_gpu_rsa_partial_sign; rsa_psign_kernels.hip; the rules:
// docs/parity.md, "Threshold RSA signing (rsaContext.Sign)").
namespace {

constexpr uint32_t PSIGN_MAX_OPS = 1u << 22;          // requests and fragments of a call: fragments * nbytes stays below 2^32 in k_limbs_to_bytes
constexpr uint32_t PSIGN_BATCHER_FRAGS = 4096;        // fragments of ONE batcher request

// The result arrays of a call (host memory).  They fail closed before anything can refuse the call, and again if it fails later.
struct PsignOut {
  uint8_t *out, *st;      // [n_frags][nbytes], [n_frags]
  uint32_t n_frags, nbytes;
  void fail_closed() const {
    if (!n_frags || n_frags > PSIGN_MAX_OPS) return;
    if (st) memset(st, BFTKV_TH_FAILED, n_frags);
    if (out) memset(out, 0, (size_t)n_frags * nbytes);
  }
};

// what refuses a call whatever its numbers: BFTKV_E_INVALID (the batcher refuses its caller by the same rules)
inline bool psign_shape_ok(uint32_t nbytes, uint32_t exp_len, uint32_t t_cap) {
  return nbytes != 0 && nbytes <= PSIGN_MAX_NBYTES && exp_len != 0 && exp_len <= PSIGN_MAX_EXP_LEN && t_cap <= nbytes;
}
// Every row holds its magnitude in its last exp_used[f] bytes (NULL: exp_len) and zeroes ahead of them.  used / negative: per fragment,
// its width and psign_negative of its sign byte and magnitude.
inline bool psign_frags_ok(uint32_t n_frags, const uint8_t* exps, uint32_t exp_len, const uint32_t* exp_used, const uint8_t* sign, uint32_t* used,
                           uint8_t* negative) {
  for (uint32_t f = 0; f < n_frags; ++f) {
    const uint32_t u = exp_used ? exp_used[f] : exp_len;
    if (u > exp_len) return false;
    const uint8_t* row = exps + (size_t)f * exp_len;
    for (uint32_t i = 0; i < exp_len - u; ++i) if (row[i]) return false;
    bool zero = true;
    for (uint32_t i = exp_len - u; i < exp_len && zero; ++i) zero = row[i] == 0;
    used[f] = u;
    negative[f] = bftkv::psign_negative(sign[f], zero) ? 1 : 0;
  }
  return true;
}
inline bool psign_all_zero(const uint8_t* p, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) if (p[i]) return false;
  return true;
}

// Everything between the uploads and the downloads is enqueued on the context's stream: the host waits once, at the end.
int psign_run(bftkv_gpu_ctx* c, const PsignOut& o, uint32_t n_reqs, const uint8_t* t, uint32_t t_cap, const uint32_t* t_len, const uint32_t* mod_idx,
              uint32_t n_mods, const uint8_t* mods, const uint32_t* frag_req, const uint8_t* exps, uint32_t exp_len, const std::vector<uint32_t>& used,
              const std::vector<uint8_t>& negative) {
  const uint32_t n_frags = o.n_frags, nbytes = o.nbytes;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  // N = 0 (a row of zeroes) is no even modulus here: emsaEncode refuses every request under it (emlen 0), which k_psign_em reads off
  // the caller's bytes.  The Montgomery table, which no such chain's answer uses, gets 1 in its place.
  std::vector<uint8_t> tab_mods(mods, mods + (size_t)n_mods * nbytes);
  for (uint32_t m = 0; m < n_mods; ++m) if (psign_all_zero(&tab_mods[(size_t)m * nbytes], nbytes)) tab_mods[(size_t)(m + 1) * nbytes - 1] = 1;
  ModTab mt;
  int rc;
  if ((rc = make_modtab(c, sb, tab_mods.data(), n_mods, nbytes, &mt))) return rc;
  std::vector<uint32_t> rmod(n_reqs, 0u), freq(n_frags, 0u), order(n_frags);
  if (mod_idx) for (uint32_t r = 0; r < n_reqs; ++r) rmod[r] = std::min(mod_idx[r], n_mods - 1u);
  if (frag_req) for (uint32_t f = 0; f < n_frags; ++f) freq[f] = std::min(frag_req[f], n_reqs - 1u);
  // m^-1 once per request that has a negative fragment (k_modinv's gate: bit 2)
  std::vector<uint8_t> gate((size_t)n_reqs + 8, 0);
  bool any_negative = false;
  for (uint32_t f = 0; f < n_frags; ++f) if (negative[f]) { gate[freq[f]] = 2; any_negative = true; }
  // chains longest first, so that the quads of a wave agree on their width (k_psign_pow runs a wave as long as its widest chain);
  // psign_caller_order (BFTKV_PSIGN_ORDER=caller): as submitted -- the answers are the same, the tests hold the kernel to that
  for (uint32_t f = 0; f < n_frags; ++f) order[f] = f;
  if (!c->psign_caller_order) std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return used[a] > used[b]; });
  hipStream_t s = c->stream;
  const uint8_t dummy[16] = {};
  uint8_t *d_t, *d_mods, *d_neg, *d_ex, *d_gate;
  uint32_t *d_tl, *d_rmod, *d_freq, *d_used, *d_order;
  void *d_em, *d_inv, *d_ref, *d_noinv, *d_out, *d_st, *d_tab, *d_bytes;
  if ((rc = to_dev(c, sb, t_cap ? t : dummy, t_cap ? (size_t)n_reqs * t_cap : sizeof(dummy), &d_t)) || (rc = to_dev(c, sb, t_len, (size_t)n_reqs, &d_tl)) ||
      (rc = to_dev(c, sb, rmod.data(), (size_t)n_reqs, &d_rmod)) || (rc = to_dev(c, sb, mods, (size_t)n_mods * nbytes, &d_mods)) ||
      (rc = to_dev(c, sb, freq.data(), (size_t)n_frags, &d_freq)) || (rc = to_dev(c, sb, used.data(), (size_t)n_frags, &d_used)) ||
      (rc = to_dev(c, sb, negative.data(), (size_t)n_frags, &d_neg)) || (rc = to_dev(c, sb, order.data(), (size_t)n_frags, &d_order)) ||
      (rc = to_dev(c, sb, exps, (size_t)n_frags * exp_len, &d_ex)) || (rc = to_dev(c, sb, gate.data(), gate.size(), &d_gate)))
    return rc;
  const uint32_t per_launch = std::min(n_frags, TPA_LAUNCH_CHAINS);
  const size_t tab_quads = (size_t)quad_grid(per_launch).x * QUADS_PER_BLOCK;
  if ((rc = dev_alloc(c, sb, (size_t)n_reqs * MONT_N * 4, &d_em, false)) || (rc = dev_alloc(c, sb, (size_t)n_reqs * MONT_N * 4, &d_inv, true)) ||
      (rc = dev_alloc(c, sb, (size_t)n_reqs + 8, &d_ref, false)) || (rc = dev_alloc(c, sb, (size_t)n_reqs + 8, &d_noinv, true)) ||
      (rc = dev_alloc(c, sb, (size_t)n_frags * MONT_N * 4, &d_out, false)) || (rc = dev_alloc(c, sb, (size_t)n_frags + 8, &d_st, false)) ||
      (rc = dev_alloc(c, sb, tab_quads * CHAIN_ENT * MONT_N * 4, &d_tab, false)) || (rc = dev_alloc(c, sb, (size_t)n_frags * nbytes, &d_bytes, false)))
    return rc;
  hipLaunchKernelGGL(k_psign_em, dim3((uint32_t)(((size_t)n_reqs * MONT_N + 255) / 256)), dim3(256), 0, s, n_reqs, (const uint8_t*)d_t, t_cap, (const uint32_t*)d_tl,
                     (const uint32_t*)d_rmod, (const uint8_t*)d_mods, nbytes, (uint32_t*)d_em, (uint8_t*)d_ref);
  if (any_negative)
    hipLaunchKernelGGL(k_modinv, dim3((n_reqs + 63) / 64), dim3(64), 0, s, n_reqs, (const uint32_t*)d_em, (const uint32_t*)d_rmod, mt, (uint32_t*)d_inv,
                       (uint8_t*)d_noinv, (const uint8_t*)d_gate, (const uint8_t*)d_ref);
  for (uint32_t first = 0; first < n_frags; first += per_launch) {
    const uint32_t n_here = std::min(per_launch, n_frags - first);
    hipLaunchKernelGGL(k_psign_pow, quad_grid(n_here), dim3(RSA_BLOCK), 0, s, n_here, first, (const uint32_t*)d_order, (const uint32_t*)d_freq,
                       (const uint32_t*)d_used, (const uint8_t*)d_neg, (const uint32_t*)d_em, (const uint32_t*)d_inv, (const uint8_t*)d_ref,
                       (const uint8_t*)d_noinv, (const uint8_t*)d_ex, exp_len, (const uint32_t*)d_rmod, mt, (uint32_t*)d_tab, (uint32_t*)d_out, (uint8_t*)d_st);
  }
  hipLaunchKernelGGL(k_limbs_to_bytes, dim3((uint32_t)(((size_t)n_frags * nbytes + 255) / 256)), dim3(256), 0, s, (const uint32_t*)d_out, nbytes, n_frags,
                     (uint8_t*)d_bytes);
  HIPCHK(c, hipMemcpyAsync(o.out, d_bytes, (size_t)n_frags * nbytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(o.st, d_st, (size_t)n_frags, hipMemcpyDeviceToHost, s));
  return finish(c, false);      // (the local vectors were copied from pageable memory: each copy call returned when it was done with them)
}

int psign_impl(bftkv_gpu_ctx* c, uint32_t n_reqs, const uint8_t* t, uint32_t t_cap, const uint32_t* t_len, const uint32_t* mod_idx, uint32_t n_mods,
               const uint8_t* mods, uint32_t nbytes, uint32_t n_frags, const uint32_t* frag_req, const uint8_t* exps, uint32_t exp_len,
               const uint32_t* exp_used, const uint8_t* sign, uint8_t* out, uint8_t* status_out) {
  const PsignOut o{out, status_out, n_frags, nbytes};
  o.fail_closed();
  if (!c || n_reqs == 0 || n_reqs > PSIGN_MAX_OPS || n_frags == 0 || n_frags > PSIGN_MAX_OPS || n_mods == 0 || !psign_shape_ok(nbytes, exp_len, t_cap) ||
      (t_cap && !t) || !t_len || !mods || !exps || !sign || !out || !status_out)
    return BFTKV_E_INVALID;
  for (uint32_t r = 0; r < n_reqs; ++r) if (t_len[r] > t_cap) return BFTKV_E_INVALID;
  std::vector<uint32_t> used(n_frags);
  std::vector<uint8_t> negative(n_frags);
  if (!psign_frags_ok(n_frags, exps, exp_len, exp_used, sign, used.data(), negative.data())) return BFTKV_E_INVALID;
  const int rc = psign_run(c, o, n_reqs, t, t_cap, t_len, mod_idx, n_mods, mods, frag_req, exps, exp_len, used, negative);
  if (rc) o.fail_closed();
  return rc;
}

}  // namespace

extern "C" {

int bftkv_gpu_rsa_partial_sign(bftkv_gpu_ctx* c, uint32_t n_reqs, const uint8_t* t, uint32_t t_cap, const uint32_t* t_len, const uint32_t* mod_idx,
                               uint32_t n_mods, const uint8_t* mods, uint32_t nbytes, uint32_t n_frags, const uint32_t* frag_req, const uint8_t* exps,
                               uint32_t exp_len, const uint32_t* exp_used, const uint8_t* sign, uint8_t* out, uint8_t* status_out) {
  return psign_impl(c, n_reqs, t, t_cap, t_len, mod_idx, n_mods, mods, nbytes, n_frags, frag_req, exps, exp_len, exp_used, sign, out, status_out);
}

}  // extern "C"
