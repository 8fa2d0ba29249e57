// C ABI of resident DSA key sets (include/bftkv_gpu.h: bftkv_gpu_dsa_keyset_* and bftkv_gpu_dsa_verify_keyset; dsa_verify_kernels.hip).
// A long-lived key (the distributed CA key of a threshold DSA signature) is registered once: the Montgomery rows of its group and a
// fixed-base window table per distinct base are made at bftkv_gpu_dsa_keyset_create, and every verification after that is
// k_dsav_prep and a chain of table products.  Sets live on the root context like quorums and ECDSA sets: created and destroyed
// there under KtWrite (the forks' calls in flight drain first), read by the forks under KtRead without a copy.
namespace {

constexpr uint32_t DSA_KEYSET_MAX_KEYS = 4096, DSA_KEYSET_MAX_GROUPS = 4096;

// chains of at most 256 entries: one part up to 8-bit windows, 2^(w - 8) beyond (k_dsav_comb_build)
inline uint32_t dsa_keyset_parts(uint32_t w) { return w > 8 ? 1u << (w - 8) : 1u; }

int dsa_keyset_create_impl(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys_y, const uint32_t* key_group, uint32_t pbytes, uint32_t n_groups,
                           const uint8_t* p, const uint8_t* q, const uint8_t* g, uint32_t qbytes, uint32_t window_bits, int* keyset_out) {
  if (!c || !keys_y || !p || !q || !g || !keyset_out || n_keys == 0 || n_keys > DSA_KEYSET_MAX_KEYS || n_groups == 0 || n_groups > DSA_KEYSET_MAX_GROUPS ||
      pbytes == 0 || pbytes > 256 || qbytes == 0 || qbytes > 32 || (window_bits != 0 && (window_bits < DSAV_COMB_WMIN || window_bits > DSAV_COMB_WMAX)))
    return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  return KeySets<DsaKeySet>::create(c, keyset_out, [&](DsaKeySet& ks) -> int {
    ScratchBufs sb(c);
    { int grc = modtab_gc(c); if (grc) return grc; }
    int rc = 0;
    ks.n_keys = n_keys; ks.n_groups = n_groups; ks.pbytes = pbytes; ks.qbytes = qbytes;
    ks.w = window_bits ? window_bits : DSAV_COMB_WDEF;
    const DsaBases hb(n_keys, keys_y, key_group, pbytes, n_groups, q, qbytes, g);
    ks.windows = dsav_comb_windows(hb.max_qbits, ks.w);
    ModTab mp, mq;                                                               // the rows of every p and q
    if ((rc = make_modtab(c, sb, p, n_groups, pbytes, &mp))) return rc;          // (an even p or q: BFTKV_E_UNSUPPORTED, no set)
    if ((rc = make_modtab(c, sb, q, n_groups, qbytes, &mq))) return rc;
    if ((rc = ks.modp.copy_from<DsaKeySet>(c, mp, n_groups, false)) || (rc = ks.modq.copy_from<DsaKeySet>(c, mq, n_groups, false))) return rc;
    if (ks.q_be.ensure_exact((size_t)n_groups * qbytes) != hipSuccess || ks.key_group.ensure_exact((size_t)n_keys * 4) != hipSuccess ||
        ks.tab.ensure_exact(ks.table_bytes()) != hipSuccess)
      return KeySets<DsaKeySet>::nomem(c);
    HIPCHK(c, hipMemcpyAsync(ks.q_be.p, q, (size_t)n_groups * qbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(ks.key_group.p, hb.key_group.data(), (size_t)n_keys * 4, hipMemcpyHostToDevice, c->stream));
    // every q once more in the word form of the share answers (bftkv_gpu_tdsa_share): no verification reads it
    std::vector<TsigMod<8>> qc(n_groups);
    for (uint32_t i = 0; i < n_groups; ++i) tsig_mod_setup<8>(qc[i], q + (size_t)i * qbytes, qbytes);
    if (ks.qc.ensure_exact(qc.size() * sizeof(TsigMod<8>)) != hipSuccess) return KeySets<DsaKeySet>::nomem(c);
    HIPCHK(c, hipMemcpyAsync(ks.qc.p, qc.data(), qc.size() * sizeof(TsigMod<8>), hipMemcpyHostToDevice, c->stream));
    // the bases as one array of limbs (scratch of this call)
    const uint32_t n_bases = n_groups + n_keys;
    uint32_t* d_bases;
    if ((rc = to_dev_limbs(c, sb, hb.bases.data(), n_bases, pbytes, &d_bases))) return rc;
    const uint32_t parts = dsa_keyset_parts(ks.w);
    hipLaunchKernelGGL((k_dsav_comb_build<MONT_L, MONT_TPI>), quad_grid(n_bases * ks.windows * parts), dim3(RSA_BLOCK), 0, c->stream, n_groups, n_keys,
                       (const uint32_t*)d_bases, ks.key_group.as<uint32_t>(), ks.modp.view(), ks.w, ks.windows, parts, ks.tab.as<uint32_t>());
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (the host vectors above die with this call)
    HIPCHK(c, hipGetLastError());
    return 0;
  });
}

int dsa_keyset_destroy_impl(bftkv_gpu_ctx* c, int keyset) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  return KeySets<DsaKeySet>::retire(c, keyset);
}

int dsa_keyset_info_impl(bftkv_gpu_ctx* c, int keyset, uint32_t* n_keys_out, uint32_t* n_groups_out, uint32_t* pbytes_out, uint32_t* qbytes_out,
                         uint32_t* window_bits_out, uint32_t* windows_out, uint64_t* table_bytes_out) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const DsaKeySet* ks = KeySets<DsaKeySet>::find(c, keyset);
  if (!ks) return KeySets<DsaKeySet>::bad_handle(c);
  if (n_keys_out) *n_keys_out = ks->n_keys;
  if (n_groups_out) *n_groups_out = ks->n_groups;
  if (pbytes_out) *pbytes_out = ks->pbytes;
  if (qbytes_out) *qbytes_out = ks->qbytes;
  if (window_bits_out) *window_bits_out = ks->w;
  if (windows_out) *windows_out = ks->windows;
  if (table_bytes_out) *table_bytes_out = ks->table_bytes();
  return 0;
}

// one base's table, as built (test hook); bases count the groups' g first, then the keys' y
int dsa_keyset_table_impl(bftkv_gpu_ctx* c, int keyset, uint32_t base, uint32_t* words_out, uint64_t cap_words) {
  if (!c || !words_out) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const DsaKeySet* ks = KeySets<DsaKeySet>::find(c, keyset);
  if (!ks || base >= ks->n_groups + ks->n_keys) return fail(c, BFTKV_E_INVALID, "bad DSA key set handle or base index");
  const uint64_t words = ks->table_bytes() / 4 / (ks->n_groups + ks->n_keys);
  if (cap_words < words) return fail(c, BFTKV_E_NOMEM, "words_out holds less than one table");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(words_out, ks->tab.as<uint32_t>() + (size_t)base * words, words * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// dsa_verify_impl over a registered set: the same k_dsav_prep, then k_dsav_comb_exp.  Nothing is read from host memory but the host
// form's own arrays (the rows, the orders, the groups and the tables are resident), so the device form never waits.
int dsa_verify_keyset_impl(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs,
                           const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out, bool dev) {
  const bool shape_ok = dlen != 0 && dlen <= 64 && (!n_ops || (digests && sigs));
  return verify_on_keyset<DsaKeySet>(c, keyset, n_ops, DSAV_MAX_OPS, valid_out, status_out, dev, shape_ok, [&](const DsaKeySet& ks, VerdictOut& vo) -> int {
    ScratchBufs sb(c);
    DsavScratch w;
    if (int rc = dsav_prep(c, sb, vo, digests, dlen, sigs, ks.qbytes, key_idx, ks.n_keys, ks.key_group.as<uint32_t>(), ks.q_be.as<uint8_t>(), &w)) return rc;
    hipLaunchKernelGGL((k_dsav_comb_exp<MONT_L, MONT_TPI>), quad_grid(n_ops), dim3(RSA_BLOCK), 0, c->stream, n_ops, (const uint32_t*)w.e, (const uint32_t*)w.ok,
                       (const uint32_t*)w.og, (const uint8_t*)w.flag, ks.n_groups, ks.modp.view(), ks.modq.view(), ks.tab.as<uint32_t>(), ks.w, ks.windows,
                       (uint8_t*)vo.d_valid);
    return vo.finish(c);
  });
}

}  // namespace

extern "C" {

int bftkv_gpu_dsa_keyset_create(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys_y, const uint32_t* key_group, uint32_t pbytes, uint32_t n_groups,
                                const uint8_t* p, const uint8_t* q, const uint8_t* g, uint32_t qbytes, uint32_t window_bits, int* keyset_out) {
  return dsa_keyset_create_impl(c, n_keys, keys_y, key_group, pbytes, n_groups, p, q, g, qbytes, window_bits, keyset_out);
}
int bftkv_gpu_dsa_keyset_destroy(bftkv_gpu_ctx* c, int keyset) { return dsa_keyset_destroy_impl(c, keyset); }
int bftkv_gpu_dsa_keyset_info(bftkv_gpu_ctx* c, int keyset, uint32_t* n_keys_out, uint32_t* n_groups_out, uint32_t* pbytes_out, uint32_t* qbytes_out,
                              uint32_t* window_bits_out, uint32_t* windows_out, uint64_t* table_bytes_out) {
  return dsa_keyset_info_impl(c, keyset, n_keys_out, n_groups_out, pbytes_out, qbytes_out, window_bits_out, windows_out, table_bytes_out);
}
int bftkv_gpu_dsa_verify_keyset(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs,
                                const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out) {
  return dsa_verify_keyset_impl(c, keyset, n_ops, digests, dlen, sigs, key_idx, valid_out, status_out, false);
}
int bftkv_gpu_dsa_verify_keyset_dev(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs,
                                    const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out) {
  return dsa_verify_keyset_impl(c, keyset, n_ops, digests, dlen, sigs, key_idx, valid_out, status_out, true);
}
int bftkv_gpu_selftest_dsa_keyset_table(bftkv_gpu_ctx* c, int keyset, uint32_t base, uint32_t* words_out, uint64_t cap_words) {
  return dsa_keyset_table_impl(c, keyset, base, words_out, cap_words);
}

}  // extern "C"
