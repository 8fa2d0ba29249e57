// C ABI of raw RSA PKCS#1 v1.5 signing under resident private key sets (include/bftkv_gpu.h: bftkv_gpu_rsa_signer_*,
// bftkv_gpu_rsa_sign_keyset, its _dev form and bftkv_gpu_selftest_rsa_crt; rsa_sign_kernels.hip; the rules: rsa_sign.h, docs/parity.md,
// "RSA signing (rsa.SignPKCS1v15)").  No message of this file names a key's bytes.
namespace {

constexpr uint32_t RSAS_MAX_OPS = 1u << 22, RSA_SIGNER_MAX_KEYS = 1u << 16;
constexpr uint32_t RSAS_LAUNCH_SIGS = BFTKV_RSA_SIGN_LAUNCH;      // signatures of one k_rsas_crt launch: 2 quads each, 2,560 bytes of table per quad

// host memory that held a secret is overwritten before it is given back
inline void rsas_wipe(void* p, size_t bytes) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < bytes; ++i) v[i] = 0;
}
template <typename T>
struct WipedVec : std::vector<T> {
  using std::vector<T>::vector;
  ~WipedVec() { if (!this->empty()) rsas_wipe(this->data(), this->size() * sizeof(T)); }
};

// The rows of one odd prime m >= 3 (big-endian, pbytes) in the 10 x 4 form: m, R^2 mod m and R^3 mod m as 40 limbs, -m^-1 mod 2^28;
// r_words: R mod m on nw words, for qinv R.  Once per key at registration: doubling and double-and-add (host_bignum.h) do.
void rsas_prime_rows(const uint8_t* m_be, uint32_t pbytes, int nw, uint32_t* mod, uint32_t* r2, uint32_t* r3, uint32_t* n0inv, uint32_t* m_words,
                     uint32_t* r_words) {
  WipedVec<uint32_t> a(nw), b(nw);
  hostbn::from_be(m_be, pbytes, m_words, nw);
  std::fill(r_words, r_words + nw, 0u);
  r_words[0] = 1;
  for (int i = 0; i < RSAS_W * RSAS_N; ++i) hostbn::dbl_mod(r_words, m_words, nw);
  hostbn::mul_mod(r_words, r_words, m_words, a.data(), nw);
  hostbn::mul_mod(a.data(), r_words, m_words, b.data(), nw);
  hostbn::to_limbs28(m_words, nw, mod, RSAS_N);
  hostbn::to_limbs28(a.data(), nw, r2, RSAS_N);
  hostbn::to_limbs28(b.data(), nw, r3, RSAS_N);
  uint32_t inv = m_words[0];                       // m0^-1 mod 2^32 by Newton iteration
  for (int i = 0; i < 5; ++i) inv *= 2u - m_words[0] * inv;
  *n0inv = (0u - inv) & MONT_MASK;
}

// every buffer that holds p, q, dp, dq, qinv or a row derived from them is overwritten before it is freed
void RsaSignerSet::release() {
  DevBuf* secret[] = {&mod, &r2, &r3, &n0, &d, &qinv_r};
  bool any = false;
  for (DevBuf* b : secret) if (b->p) { (void)hipMemsetAsync(b->p, 0, b->cap, nullptr); any = true; }
  if (any) (void)hipStreamSynchronize(nullptr);
  for (DevBuf* b : secret) b->release();
  refused.release(); n29.release(); r2_29.release(); meta.release();
}

RsasKeys rsas_view(const RsaSignerSet& ks) {
  return RsasKeys{ks.mod.as<uint32_t>(), ks.r2.as<uint32_t>(), ks.r3.as<uint32_t>(), ks.n0.as<uint32_t>(), ks.d.as<uint8_t>(), ks.qinv_r.as<uint32_t>(),
                  ks.refused.as<uint8_t>(), ks.meta.as<uint4>(), ks.n_keys, ks.pbytes};
}

int rsa_signer_create_impl(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys_n, const uint32_t* keys_e, uint32_t nbytes, const uint8_t* p,
                           const uint8_t* q, const uint8_t* dp, const uint8_t* dq, const uint8_t* qinv, uint32_t pbytes, int* set_out) {
  if (set_out) *set_out = -1;
  if (!c || !keys_n || !keys_e || !p || !q || !dp || !dq || !qinv || !set_out || n_keys == 0 || n_keys > RSA_SIGNER_MAX_KEYS || nbytes == 0 ||
      nbytes > RSAS_MAX_NBYTES || pbytes == 0 || pbytes > RSAS_MAX_PBYTES)
    return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  return KeySets<RsaSignerSet>::create(c, set_out, [&](RsaSignerSet& ks) -> int {
    ks.n_keys = n_keys; ks.nbytes = nbytes; ks.pbytes = pbytes;
    const int nw = (int)pbytes / 4 + 2;                       // words of the host numbers: a word of headroom for the doublings
    const size_t NP = (size_t)n_keys * 2 * RSAS_N;
    WipedVec<uint32_t> mod(NP, 0u), r2(NP, 0u), r3(NP, 0u), n0((size_t)n_keys * 2, 0u), qr((size_t)n_keys * RSAS_N, 0u);
    WipedVec<uint8_t> d((size_t)n_keys * 2 * pbytes, 0);
    std::vector<uint8_t> refused(n_keys, 0);
    WipedVec<uint32_t> mw(nw), rw(nw), qw(nw), tw(nw), pw(nw), prw(nw);
    for (uint32_t k = 0; k < n_keys; ++k) {
      const uint8_t *pk = p + (size_t)k * pbytes, *qk = q + (size_t)k * pbytes;
      if (rsas_key_refused(keys_n + (size_t)k * nbytes, nbytes, pk, qk, pbytes)) { refused[k] = 1; ++ks.n_refused; continue; }
      const size_t row = (size_t)k * 2 * RSAS_N;
      rsas_prime_rows(pk, pbytes, nw, &mod[row], &r2[row], &r3[row], &n0[(size_t)k * 2], pw.data(), prw.data());
      rsas_prime_rows(qk, pbytes, nw, &mod[row + RSAS_N], &r2[row + RSAS_N], &r3[row + RSAS_N], &n0[(size_t)k * 2 + 1], mw.data(), rw.data());
      hostbn::from_be(qinv + (size_t)k * pbytes, pbytes, qw.data(), nw);      // any value of the width: reduced as big.Int.Mod reduces it
      hostbn::reduce(qw.data(), pw.data(), nw);
      hostbn::mul_mod(qw.data(), prw.data(), pw.data(), tw.data(), nw);
      hostbn::to_limbs28(tw.data(), nw, &qr[(size_t)k * RSAS_N], RSAS_N);
      memcpy(&d[(size_t)k * 2 * pbytes], dp + (size_t)k * pbytes, pbytes);
      memcpy(&d[((size_t)k * 2 + 1) * pbytes], dq + (size_t)k * pbytes, pbytes);
    }
    // the verifier's rows of (n, e), by the code that fills an RsaKeySet: the check calls k_rsav_verify<18, 4, 29> as it stands
    RsavRows rows;
    rsav_rows(c, n_keys, keys_n, keys_e, nbytes, false, &rows);
    struct Up { DevBuf* b; const void* src; size_t bytes; };
    const Up ups[] = {{&ks.mod, mod.data(), NP * 4}, {&ks.r2, r2.data(), NP * 4}, {&ks.r3, r3.data(), NP * 4}, {&ks.n0, n0.data(), n0.size() * 4},
                      {&ks.d, d.data(), d.size()}, {&ks.qinv_r, qr.data(), qr.size() * 4}, {&ks.refused, refused.data(), refused.size()},
                      {&ks.n29, rows.n.data(), rows.n.size() * 4}, {&ks.r2_29, rows.r2.data(), rows.r2.size() * 4},
                      {&ks.meta, rows.meta.data(), rows.meta.size() * 4}};
    for (const Up& u : ups) {
      if (u.b->ensure_exact(u.bytes) != hipSuccess) return KeySets<RsaSignerSet>::nomem(c);
      HIPCHK(c, hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (the host vectors die with this call)
    return 0;
  });
}

int rsa_signer_destroy_impl(bftkv_gpu_ctx* c, int set) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  return KeySets<RsaSignerSet>::retire(c, set);
}

int rsa_signer_info_impl(bftkv_gpu_ctx* c, int set, uint32_t* n_keys_out, uint32_t* n_refused_out, uint32_t* nbytes_out, uint32_t* pbytes_out) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const RsaSignerSet* ks = KeySets<RsaSignerSet>::find(c, set);
  if (!ks) return KeySets<RsaSignerSet>::bad_handle(c);
  if (n_keys_out) *n_keys_out = ks->n_keys;
  if (n_refused_out) *n_refused_out = ks->n_refused;
  if (nbytes_out) *nbytes_out = ks->nbytes;
  if (pbytes_out) *pbytes_out = ks->pbytes;
  return 0;
}

// The result arrays of a signing call.  The statuses fail closed before anything can refuse the call; the rows once the set has told
// their width (under a bad handle it is unknown: the rows are left alone), and both again if the call fails later.
struct RsasOut {
  uint8_t *sig, *st;
  uint32_t n_ops;
  bool dev;
  size_t nbytes = 0;
  int fill(bftkv_gpu_ctx* c, uint8_t* p, int v, size_t bytes) const {
    if (!p || !bytes) return 0;
    if (dev) HIPCHK(c, hipMemsetAsync(p, v, bytes, c->stream));
    else memset(p, v, bytes);
    return 0;
  }
  int fail_closed(bftkv_gpu_ctx* c) const {
    if (!n_ops || n_ops > RSAS_MAX_OPS) return 0;
    if (const int rc = fill(c, st, BFTKV_TH_FAILED, n_ops)) return rc;
    return fill(c, sig, 0, n_ops * nbytes);
  }
};

// em (digests != nullptr) or the caller's values (cvals: bftkv_gpu_selftest_rsa_crt, no padding, no check) through the chains, the
// recombination, the check and the statuses.  Everything is enqueued on the context's stream; whatever scratch held a half of a
// signature (m2 and h give q away) or a chain's table is overwritten behind the last kernel.
int rsas_run(bftkv_gpu_ctx* c, const RsaSignerSet& ks, const RsasOut& o, const uint8_t* digests, uint32_t hash_id, uint32_t dlen, const uint8_t* cvals,
             const uint32_t* key_idx) {
  const uint32_t n_ops = o.n_ops, nbytes = ks.nbytes;
  const bool dev = o.dev;
  ScratchBufs sb(c);
  hipStream_t s = c->stream;
  const RsasKeys keys = rsas_view(ks);
  uint32_t* d_ki = nullptr;
  uint8_t* d_in;
  void *d_sig = o.sig, *d_st = o.st, *d_c, *d_rule, *d_tab, *d_m2h, *d_s, *d_fits, *d_valid = nullptr, *d_vst = nullptr, *d_xr = nullptr;
  int rc;
  if (key_idx && (rc = to_dev(c, sb, key_idx, (size_t)n_ops, &d_ki, dev))) return rc;                  // clamped by the kernels
  if ((rc = to_dev(c, sb, digests ? digests : cvals, (size_t)n_ops * (digests ? dlen : nbytes), &d_in, dev))) return rc;
  if (!dev && ((rc = dev_alloc(c, sb, (size_t)n_ops * nbytes, &d_sig, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_st, false)))) return rc;
  const uint32_t per_launch = std::min(n_ops, RSAS_LAUNCH_SIGS);
  const dim3 crt_grid((per_launch + RSAS_SIGS_PER_BLOCK - 1) / RSAS_SIGS_PER_BLOCK);
  const size_t limbs_bytes = (size_t)n_ops * RSAS_VALUE_LIMBS * 4, tab_bytes = (size_t)crt_grid.x * QUADS_PER_BLOCK * CHAIN_ENT * RSAS_N * 4;
  if ((rc = dev_alloc(c, sb, limbs_bytes, &d_c, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_rule, false)) ||
      (rc = dev_alloc(c, sb, tab_bytes, &d_tab, false)) || (rc = dev_alloc(c, sb, limbs_bytes, &d_m2h, true)) ||
      (rc = dev_alloc(c, sb, limbs_bytes, &d_s, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_fits, false)))
    return rc;
  if (digests && ((rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_valid, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_vst, false)) ||
                  (rc = dev_alloc(c, sb, (size_t)n_ops * RSAV_N29 * 4, &d_xr, false))))
    return rc;
  const dim3 limb_grid((uint32_t)(((size_t)n_ops * RSAS_VALUE_LIMBS + 255) / 256)), byte_grid((uint32_t)(((size_t)n_ops * nbytes + 255) / 256));
  if (digests)
    hipLaunchKernelGGL(k_rsas_em, limb_grid, dim3(256), 0, s, n_ops, (const uint8_t*)d_in, dlen, hash_id, (const uint32_t*)d_ki, keys, (uint32_t*)d_c,
                       (uint8_t*)d_rule);
  else
    hipLaunchKernelGGL(k_rsas_value, limb_grid, dim3(256), 0, s, n_ops, (const uint8_t*)d_in, nbytes, (const uint32_t*)d_ki, keys, (uint32_t*)d_c,
                       (uint8_t*)d_rule);
  for (uint32_t first = 0; first < n_ops; first += per_launch) {
    const uint32_t n_here = std::min(per_launch, n_ops - first);
    hipLaunchKernelGGL(k_rsas_crt, dim3((n_here + RSAS_SIGS_PER_BLOCK - 1) / RSAS_SIGS_PER_BLOCK), dim3(RSA_BLOCK), 0, s, n_here, first,
                       (const uint32_t*)d_ki, keys, (const uint32_t*)d_c, (uint32_t*)d_tab, (uint32_t*)d_m2h);
  }
  hipLaunchKernelGGL(k_rsas_recombine, dim3((n_ops + 63) / 64), dim3(64), 0, s, n_ops, (const uint32_t*)d_ki, keys, (const uint32_t*)d_m2h, nbytes,
                     (uint32_t*)d_s, (uint8_t*)d_fits);
  hipLaunchKernelGGL(k_rsas_bytes, byte_grid, dim3(256), 0, s, (const uint32_t*)d_s, nbytes, n_ops, (uint8_t*)d_sig);
  if (digests)
    hipLaunchKernelGGL((k_rsav_verify<RSA29_L, MONT_TPI, RSA29_W>), quad_grid(n_ops), dim3(RSA_BLOCK), 0, s, n_ops, (const uint8_t*)d_sig, nbytes,
                       (const uint8_t*)d_in, dlen, hash_id, (const uint32_t*)d_ki, ks.n_keys,
                       RsavKeys{ks.n29.as<uint32_t>(), ks.r2_29.as<uint32_t>(), ks.meta.as<uint4>()}, (uint32_t*)d_xr, (uint8_t*)d_valid, (uint8_t*)d_vst);
  hipLaunchKernelGGL(k_rsas_finish, byte_grid, dim3(256), 0, s, n_ops, nbytes, (const uint8_t*)d_rule, (const uint8_t*)d_fits, (const uint8_t*)d_valid,
                     (uint8_t*)d_sig, (uint8_t*)d_st);
  HIPCHK(c, hipMemsetAsync(d_tab, 0, tab_bytes, s));
  HIPCHK(c, hipMemsetAsync(d_m2h, 0, limbs_bytes, s));
  HIPCHK(c, hipMemsetAsync(d_c, 0, limbs_bytes, s));
  if (!dev) {
    HIPCHK(c, hipMemcpyAsync(o.sig, d_sig, (size_t)n_ops * nbytes, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(o.st, d_st, (size_t)n_ops, hipMemcpyDeviceToHost, s));
  }
  return finish(c, dev);
}

// The head of both entries, in verify_on_keyset's order: what is refused before the lock leaves the caller's arrays alone but for a host
// caller's statuses; the statuses fail closed; the fork takes its hold on the root's tables; the handle is looked up and tells the
// width, so the rows fail closed; the call's shape is refused; an empty call ends.
int rsa_sign_impl(bftkv_gpu_ctx* c, int set, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen, const uint8_t* cvals,
                  const uint32_t* key_idx, uint8_t* sig_out, uint8_t* status_out, bool dev, bool selftest) {
  RsasOut o{sig_out, status_out, n_ops, dev};
  if (!c) {
    if (!dev) (void)o.fail_closed(nullptr);      // (host arrays: no device call behind it; the rows' width is the set's: unknown)
    return BFTKV_E_INVALID;
  }
  if (n_ops > RSAS_MAX_OPS) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = o.fail_closed(c))) return rc;
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const RsaSignerSet* ks = KeySets<RsaSignerSet>::find(c, set);
  if (!ks) return KeySets<RsaSignerSet>::bad_handle(c);
  o.nbytes = ks->nbytes;
  if ((rc = o.fail_closed(c))) return rc;
  const bool shape_ok = selftest ? (!n_ops || cvals) : (rsav_shape_ok(hash_id, dlen, 1) && (!n_ops || digests));
  if (!shape_ok || (n_ops && (!sig_out || !status_out))) return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  rc = rsas_run(c, *ks, o, selftest ? nullptr : digests, hash_id, dlen, cvals, key_idx);
  if (rc) (void)o.fail_closed(c);
  return rc;
}

}  // namespace

extern "C" {

int bftkv_gpu_rsa_signer_create(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys_n, const uint32_t* keys_e, uint32_t nbytes, const uint8_t* p,
                                const uint8_t* q, const uint8_t* dp, const uint8_t* dq, const uint8_t* qinv, uint32_t pbytes, int* set_out) {
  return rsa_signer_create_impl(c, n_keys, keys_n, keys_e, nbytes, p, q, dp, dq, qinv, pbytes, set_out);
}
int bftkv_gpu_rsa_signer_destroy(bftkv_gpu_ctx* c, int set) { return rsa_signer_destroy_impl(c, set); }
int bftkv_gpu_rsa_signer_info(bftkv_gpu_ctx* c, int set, uint32_t* n_keys_out, uint32_t* n_refused_out, uint32_t* nbytes_out, uint32_t* pbytes_out) {
  return rsa_signer_info_impl(c, set, n_keys_out, n_refused_out, nbytes_out, pbytes_out);
}
int bftkv_gpu_rsa_sign_keyset(bftkv_gpu_ctx* c, int set, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen, const uint32_t* key_idx,
                              uint8_t* sig_out, uint8_t* status_out) {
  return rsa_sign_impl(c, set, n_ops, digests, hash_id, dlen, nullptr, key_idx, sig_out, status_out, false, false);
}
int bftkv_gpu_rsa_sign_keyset_dev(bftkv_gpu_ctx* c, int set, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen,
                                  const uint32_t* key_idx, uint8_t* sig_out, uint8_t* status_out) {
  return rsa_sign_impl(c, set, n_ops, digests, hash_id, dlen, nullptr, key_idx, sig_out, status_out, true, false);
}
int bftkv_gpu_selftest_rsa_crt(bftkv_gpu_ctx* c, int set, uint32_t n_ops, const uint8_t* cvals, const uint32_t* key_idx, uint8_t* out,
                               uint8_t* status_out) {
  return rsa_sign_impl(c, set, n_ops, nullptr, 0, 0, cvals, key_idx, out, status_out, false, true);
}

}  // extern "C"
