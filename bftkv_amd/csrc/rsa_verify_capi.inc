// C ABI of raw RSA PKCS#1 v1.5 verification and of resident RSA key sets (include/bftkv_gpu.h: bftkv_gpu_rsa_verify, its _dev form
// and bftkv_gpu_rsa_keyset_* / bftkv_gpu_rsa_verify_keyset; rsa_verify_kernels.hip; the rules: rsa_verify.h, docs/parity.md).
namespace {

constexpr uint32_t RSAV_MAX_OPS = 1u << 24, RSAV_MAX_KEYS = 1u << 24, RSA_KEYSET_MAX_KEYS = 1u << 20;
constexpr int RSAV_N29 = RSA29_N, RSAV_N80 = MONT_N_WIDE;

// The rows of the call's or the set's keys on the host, in one form (wide: 80 limbs of 28 bits, else 72 of 29): n, R^2 mod n and
// the meta word of every key.  The rows of ONE modulus are remembered by its bytes in a cache of their own beside modrow_cache (the
// forms differ from make_modtab's, whose cache and callers stay as they are), so a recurring key costs no hostbn::mont_setup.
struct RsavRows {
  std::vector<uint32_t> n, r2;
  std::vector<uint32_t> meta;      // uint4 per key
  uint32_t n_refused = 0;
};
// -n^-1 mod 2^29 of an odd n (its low 28 bits are -n^-1 mod 2^28: one word serves both forms)
inline uint32_t rsav_n0inv29(const uint8_t* n_be, uint32_t nbytes) {
  uint32_t n0 = 0;
  for (uint32_t i = 0; i < 4 && i < nbytes; ++i) n0 |= (uint32_t)n_be[nbytes - 1 - i] << (8 * i);
  uint32_t inv = n0;            // n0^-1 mod 2^32 by Newton iteration
  for (int i = 0; i < 5; ++i) inv *= 2u - n0 * inv;
  return (0u - inv) & ((1u << RSA29_W) - 1u);
}
void rsav_rows_one(bftkv_gpu_ctx* c, const uint8_t* n_be, uint32_t nbytes, bool wide, uint32_t* n_out, uint32_t* r2_out) {
  const int NL = wide ? RSAV_N80 : RSAV_N29;
  auto& cache = c->rsav_row_cache[wide ? 1 : 0];
  std::string mk((const char*)n_be, nbytes);
  auto it = cache.find(mk);
  if (it == cache.end()) {
    std::vector<uint32_t> row(2 * (size_t)NL);
    uint32_t n0;
    (void)hostbn::mont_setup(n_be, nbytes, NL, &row[0], &row[NL], &n0, wide ? MONT_W : RSA29_W);
    if (cache.size() >= 4096) cache.clear();
    it = cache.emplace(std::move(mk), std::move(row)).first;
  }
  const std::vector<uint32_t>& row = it->second;
  std::copy(row.begin(), row.begin() + NL, n_out);
  std::copy(row.begin() + NL, row.end(), r2_out);
}
void rsav_rows(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys_n, const uint32_t* keys_e, uint32_t nbytes, bool wide, RsavRows* out) {
  const size_t NL = wide ? RSAV_N80 : RSAV_N29;
  out->n.assign((size_t)n_keys * NL, 0u);
  out->r2.assign((size_t)n_keys * NL, 0u);
  out->meta.assign((size_t)n_keys * 4, 0u);
  out->n_refused = 0;
  for (uint32_t k = 0; k < n_keys; ++k) {
    const uint8_t* nb = keys_n + (size_t)k * nbytes;
    const bool even = !(nb[nbytes - 1] & 1);
    if (even) ++out->n_refused;
    else rsav_rows_one(c, nb, nbytes, wide, &out->n[k * NL], &out->r2[k * NL]);
    uint32_t* m = &out->meta[(size_t)k * 4];
    m[0] = even ? 0u : rsav_n0inv29(nb, nbytes); m[1] = rsav_kbytes(nb, nbytes); m[2] = keys_e[k]; m[3] = even ? 1u : 0u;
  }
}

// what refuses a call whatever its keys: BFTKV_E_INVALID
inline bool rsav_shape_ok(uint32_t hash_id, uint32_t dlen, uint32_t nbytes) {
  return rsav_prefix_len(hash_id) >= 0 && rsav_dlen_ok(hash_id, dlen) && nbytes != 0 && nbytes <= RSAV_MAX_NBYTES;
}

// the per-signature arrays to the device, the scratch, the result arrays and the kernel
int rsav_launch(bftkv_gpu_ctx* c, ScratchBufs& sb, VerdictOut& vo, const uint8_t* digests, uint32_t hash_id, uint32_t dlen, const uint8_t* sigs,
                uint32_t nbytes, const uint32_t* key_idx, uint32_t n_keys, RsavKeys keys, bool wide) {
  const uint32_t n_ops = vo.n_ops;
  const bool dev = vo.dev;
  uint32_t* d_ki = nullptr;
  uint8_t *d_dg, *d_sig;
  void* d_xr;
  int rc;
  if (key_idx && (rc = to_dev(c, sb, key_idx, (size_t)n_ops, &d_ki, dev))) return rc;                  // clamped by the kernel
  if ((rc = to_dev(c, sb, digests, (size_t)n_ops * dlen, &d_dg, dev))) return rc;
  if ((rc = to_dev(c, sb, sigs, (size_t)n_ops * nbytes, &d_sig, dev))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * (wide ? RSAV_N80 : RSAV_N29) * 4, &d_xr, false)) || (rc = vo.device_arrays(c, sb))) return rc;
  if (wide) {
    constexpr uint32_t G = RSA_BLOCK / MULTI_TPI8;
    hipLaunchKernelGGL((k_rsav_verify<MULTI_L8, MULTI_TPI8, MONT_W>), dim3((n_ops + G - 1) / G), dim3(RSA_BLOCK), 0, c->stream, n_ops, (const uint8_t*)d_sig,
                       nbytes, (const uint8_t*)d_dg, dlen, hash_id, (const uint32_t*)d_ki, n_keys, keys, (uint32_t*)d_xr, (uint8_t*)vo.d_valid,
                       (uint8_t*)vo.d_st);
  } else {
    hipLaunchKernelGGL((k_rsav_verify<RSA29_L, MONT_TPI, RSA29_W>), quad_grid(n_ops), dim3(RSA_BLOCK), 0, c->stream, n_ops, (const uint8_t*)d_sig, nbytes,
                       (const uint8_t*)d_dg, dlen, hash_id, (const uint32_t*)d_ki, n_keys, keys, (uint32_t*)d_xr, (uint8_t*)vo.d_valid, (uint8_t*)vo.d_st);
  }
  return vo.finish(c);
}

int rsa_verify_impl(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen, const uint8_t* sigs, uint32_t nbytes,
                    const uint32_t* key_idx, uint32_t n_keys, const uint8_t* keys_n, const uint32_t* keys_e, uint8_t* valid_out, uint8_t* status_out,
                    bool dev) {
  if (!c || n_ops > RSAV_MAX_OPS || (n_ops && (!valid_out || !status_out))) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  VerdictOut vo{valid_out, status_out, n_ops, dev};
  if ((rc = vo.fail_closed(c))) return rc;
  if (!rsav_shape_ok(hash_id, dlen, nbytes) || n_keys == 0 || n_keys > RSAV_MAX_KEYS || !keys_n || !keys_e || (n_ops && (!digests || !sigs)))
    return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ScratchBufs sb(c);
  const bool wide = lanes_wide(c, c->rsav_lanes, n_ops);      // lanes per signature as for k_multiexp (BFTKV_RSAV_LANES overrides)
  RsavRows rows;
  rsav_rows(c, n_keys, keys_n, keys_e, nbytes, wide, &rows);
  uint32_t *d_n, *d_r2, *d_meta;
  if ((rc = to_dev(c, sb, rows.n.data(), rows.n.size(), &d_n)) || (rc = to_dev(c, sb, rows.r2.data(), rows.r2.size(), &d_r2)) ||
      (rc = to_dev(c, sb, rows.meta.data(), rows.meta.size(), &d_meta)))
    return rc;
  // (the host vectors above were copied from pageable memory: each copy call returned when it was done with them)
  return rsav_launch(c, sb, vo, digests, hash_id, dlen, sigs, nbytes, key_idx, n_keys, RsavKeys{d_n, d_r2, (const uint4*)d_meta}, wide);
}

// ---- resident key sets: created and destroyed on the root under KtWrite, read by the forks under KtRead (as DSA key sets are) ----
int rsa_keyset_create_impl(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys_n, const uint32_t* keys_e, uint32_t nbytes, int* keyset_out) {
  if (!c || !keys_n || !keys_e || !keyset_out || n_keys == 0 || n_keys > RSA_KEYSET_MAX_KEYS || nbytes == 0 || nbytes > RSAV_MAX_NBYTES)
    return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  return KeySets<RsaKeySet>::create(c, keyset_out, [&](RsaKeySet& ks) -> int {
    ks.n_keys = n_keys; ks.nbytes = nbytes;
    for (int wide = 0; wide < 2; ++wide) {
      RsavRows rows;
      rsav_rows(c, n_keys, keys_n, keys_e, nbytes, wide != 0, &rows);
      ks.n_refused = rows.n_refused;
      DevBuf& dn = wide ? ks.n80 : ks.n29;
      DevBuf& dr = wide ? ks.r2_80 : ks.r2_29;
      if (dn.ensure_exact(rows.n.size() * 4) != hipSuccess || dr.ensure_exact(rows.r2.size() * 4) != hipSuccess ||
          ks.meta.ensure_exact(rows.meta.size() * 4) != hipSuccess)
        return KeySets<RsaKeySet>::nomem(c);
      HIPCHK(c, hipMemcpyAsync(dn.p, rows.n.data(), rows.n.size() * 4, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(dr.p, rows.r2.data(), rows.r2.size() * 4, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(ks.meta.p, rows.meta.data(), rows.meta.size() * 4, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));          // (the host vectors die with this round)
    }
    return 0;
  });
}

int rsa_keyset_destroy_impl(bftkv_gpu_ctx* c, int keyset) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  return KeySets<RsaKeySet>::retire(c, keyset);
}

int rsa_keyset_info_impl(bftkv_gpu_ctx* c, int keyset, uint32_t* n_keys_out, uint32_t* n_refused_out, uint32_t* nbytes_out) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const RsaKeySet* ks = KeySets<RsaKeySet>::find(c, keyset);
  if (!ks) return KeySets<RsaKeySet>::bad_handle(c);
  if (n_keys_out) *n_keys_out = ks->n_keys;
  if (n_refused_out) *n_refused_out = ks->n_refused;
  if (nbytes_out) *nbytes_out = ks->nbytes;
  return 0;
}

// rsa_verify_impl over a registered set: nothing crosses but digests, signatures and indices, so the device form never waits
int rsa_verify_keyset_impl(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen, const uint8_t* sigs,
                           const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out, bool dev) {
  const bool shape_ok = rsav_shape_ok(hash_id, dlen, 1) && (!n_ops || (digests && sigs));
  return verify_on_keyset<RsaKeySet>(c, keyset, n_ops, RSAV_MAX_OPS, valid_out, status_out, dev, shape_ok, [&](const RsaKeySet& ks, VerdictOut& vo) -> int {
    ScratchBufs sb(c);
    const bool wide = lanes_wide(c, c->rsav_lanes, n_ops);
    const RsavKeys keys{(wide ? ks.n80 : ks.n29).as<uint32_t>(), (wide ? ks.r2_80 : ks.r2_29).as<uint32_t>(), ks.meta.as<uint4>()};
    return rsav_launch(c, sb, vo, digests, hash_id, dlen, sigs, ks.nbytes, key_idx, ks.n_keys, keys, wide);
  });
}

}  // namespace

extern "C" {

int bftkv_gpu_rsa_verify(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen, const uint8_t* sigs, uint32_t nbytes,
                         const uint32_t* key_idx, uint32_t n_keys, const uint8_t* keys_n, const uint32_t* keys_e, uint8_t* valid_out,
                         uint8_t* status_out) {
  return rsa_verify_impl(c, n_ops, digests, hash_id, dlen, sigs, nbytes, key_idx, n_keys, keys_n, keys_e, valid_out, status_out, false);
}
int bftkv_gpu_rsa_verify_dev(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen, const uint8_t* sigs,
                             uint32_t nbytes, const uint32_t* key_idx, uint32_t n_keys, const uint8_t* keys_n, const uint32_t* keys_e,
                             uint8_t* valid_out, uint8_t* status_out) {
  return rsa_verify_impl(c, n_ops, digests, hash_id, dlen, sigs, nbytes, key_idx, n_keys, keys_n, keys_e, valid_out, status_out, true);
}
int bftkv_gpu_rsa_keyset_create(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys_n, const uint32_t* keys_e, uint32_t nbytes, int* keyset_out) {
  return rsa_keyset_create_impl(c, n_keys, keys_n, keys_e, nbytes, keyset_out);
}
int bftkv_gpu_rsa_keyset_destroy(bftkv_gpu_ctx* c, int keyset) { return rsa_keyset_destroy_impl(c, keyset); }
int bftkv_gpu_rsa_keyset_info(bftkv_gpu_ctx* c, int keyset, uint32_t* n_keys_out, uint32_t* n_refused_out, uint32_t* nbytes_out) {
  return rsa_keyset_info_impl(c, keyset, n_keys_out, n_refused_out, nbytes_out);
}
int bftkv_gpu_rsa_verify_keyset(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen,
                                const uint8_t* sigs, const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out) {
  return rsa_verify_keyset_impl(c, keyset, n_ops, digests, hash_id, dlen, sigs, key_idx, valid_out, status_out, false);
}
int bftkv_gpu_rsa_verify_keyset_dev(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t hash_id, uint32_t dlen,
                                    const uint8_t* sigs, const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out) {
  return rsa_verify_keyset_impl(c, keyset, n_ops, digests, hash_id, dlen, sigs, key_idx, valid_out, status_out, true);
}

}  // extern "C"
