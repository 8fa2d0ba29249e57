// C ABI of raw DSA verification (include/bftkv_gpu.h: bftkv_gpu_dsa_verify and its _dev form; dsa_verify_kernels.hip).
namespace {

constexpr uint32_t DSAV_MAX_OPS = 1u << 24, DSAV_MAX_BASES = 1u << 20;

// What a call or a key set makes its tables from: the bases, g of every group and then y of every key, as one array; the keys'
// groups clamped (host pointers); the bit length of the widest order.
struct DsaBases {
  std::vector<uint8_t> bases;
  std::vector<uint32_t> key_group;
  uint32_t max_qbits = 1;
  DsaBases(uint32_t n_keys, const uint8_t* keys_y, const uint32_t* kg, uint32_t pbytes, uint32_t n_groups, const uint8_t* q, uint32_t qbytes,
           const uint8_t* g)
      : bases((size_t)(n_groups + n_keys) * pbytes), key_group(n_keys, 0u) {
    memcpy(bases.data(), g, (size_t)n_groups * pbytes);
    memcpy(bases.data() + (size_t)n_groups * pbytes, keys_y, (size_t)n_keys * pbytes);
    if (kg) for (uint32_t k = 0; k < n_keys; ++k) key_group[k] = std::min(kg[k], n_groups - 1u);
    for (uint32_t i = 0; i < n_groups; ++i) max_qbits = std::max(max_qbits, (uint32_t)hostbn::bit_length(q + (size_t)i * qbytes, qbytes));
  }
};

// The head of a verification, with or without a key set: the per-signature arrays to the device, k_dsav_prep's scratch, the result
// arrays and k_dsav_prep itself.  d_kg, d_q: the keys' groups and the orders, already on the device.
struct DsavScratch { void *e, *ok, *og, *flag; };
int dsav_prep(bftkv_gpu_ctx* c, ScratchBufs& sb, VerdictOut& vo, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs, uint32_t qbytes,
              const uint32_t* key_idx, uint32_t n_keys, const uint32_t* d_kg, const uint8_t* d_q, DsavScratch* w) {
  const uint32_t n_ops = vo.n_ops;
  const bool dev = vo.dev;
  uint32_t* d_ki = nullptr;
  uint8_t *d_dg, *d_sig;
  int rc;
  if (key_idx && (rc = to_dev(c, sb, key_idx, (size_t)n_ops, &d_ki, dev))) return rc;                  // clamped by k_dsav_prep
  if ((rc = to_dev(c, sb, digests, (size_t)n_ops * dlen, &d_dg, dev))) return rc;
  if ((rc = to_dev(c, sb, sigs, (size_t)n_ops * 2 * qbytes, &d_sig, dev))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * DSAV_ROW * 4, &w->e, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * 4, &w->ok, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops * 4, &w->og, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &w->flag, false)) ||
      (rc = vo.device_arrays(c, sb)))
    return rc;
  hipLaunchKernelGGL(k_dsav_prep, dim3((n_ops + 63) / 64), dim3(64), 0, c->stream, n_ops, (const uint8_t*)d_dg, dlen, (const uint8_t*)d_sig, qbytes,
                     (const uint32_t*)d_ki, n_keys, d_kg, d_q, (uint32_t*)w->e, (uint32_t*)w->ok, (uint32_t*)w->og, (uint8_t*)w->flag, (uint8_t*)vo.d_st);
  return 0;
}

int dsa_verify_impl(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs, uint32_t qbytes,
                    const uint32_t* key_idx, uint32_t n_keys, const uint8_t* keys_y, const uint32_t* key_group, uint32_t pbytes, uint32_t n_groups,
                    const uint8_t* p, const uint8_t* q, const uint8_t* g, uint8_t* valid_out, uint8_t* status_out, bool dev) {
  if (!c || n_ops > DSAV_MAX_OPS || (n_ops && (!valid_out || !status_out))) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  VerdictOut vo{valid_out, status_out, n_ops, dev};
  if ((rc = vo.fail_closed(c))) return rc;
  if (dlen == 0 || dlen > 64 || qbytes == 0 || qbytes > 32 || pbytes == 0 || pbytes > 256 || n_keys == 0 || n_keys > DSAV_MAX_BASES || n_groups == 0 ||
      n_groups > DSAV_MAX_BASES || !keys_y || !p || !q || !g || (n_ops && (!digests || !sigs)))
    return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mp, mq;
  if ((rc = make_modtab(c, sb, p, n_groups, pbytes, &mp))) return rc;          // (an even p or q: BFTKV_E_UNSUPPORTED for the call)
  if ((rc = make_modtab(c, sb, q, n_groups, qbytes, &mq))) return rc;
  const DsaBases hb(n_keys, keys_y, key_group, pbytes, n_groups, q, qbytes, g);
  const uint32_t n_bases = n_groups + n_keys;
  const uint32_t exp_windows = (hb.max_qbits + MULTIEXP_WIN - 1) / MULTIEXP_WIN;      // u1, u2 are residues mod q
  uint32_t *d_bases, *d_kg;
  uint8_t* d_q;
  DsavScratch w;
  void* d_tab;
  if ((rc = to_dev_limbs(c, sb, hb.bases.data(), n_bases, pbytes, &d_bases))) return rc;
  if ((rc = to_dev(c, sb, hb.key_group.data(), (size_t)n_keys, &d_kg))) return rc;
  if ((rc = to_dev(c, sb, q, (size_t)n_groups * qbytes, &d_q))) return rc;
  // (by distinct base, not by signature; ahead of dsav_prep: nothing may fail once k_dsav_prep, which writes the caller's status bytes, is queued)
  if ((rc = dev_alloc(c, sb, (size_t)n_bases * MULTIEXP_ENT * MONT_N * 4, &d_tab, false))) return rc;
  if ((rc = dsav_prep(c, sb, vo, digests, dlen, sigs, qbytes, key_idx, n_keys, d_kg, d_q, &w))) return rc;
  hipStream_t s = c->stream;
  // lanes per number as for k_multiexp (BFTKV_MULTIEXP_LANES overrides).  The tables take the form of the exponentiation that reads them.
  if (lanes_wide(c, c->multiexp_lanes, n_ops)) {
    constexpr uint32_t G = RSA_BLOCK / MULTI_TPI8;
    hipLaunchKernelGGL((k_dsav_tables<MULTI_L8, MULTI_TPI8>), dim3((n_bases + G - 1) / G), dim3(RSA_BLOCK), 0, s, n_groups, n_keys, (const uint32_t*)d_bases,
                       (const uint32_t*)d_kg, mp, (uint32_t*)d_tab);
    hipLaunchKernelGGL((k_dsav_exp<MULTI_L8, MULTI_TPI8>), dim3((n_ops + G - 1) / G), dim3(RSA_BLOCK), 0, s, n_ops, (const uint32_t*)w.e, (const uint32_t*)w.ok,
                       (const uint32_t*)w.og, (const uint8_t*)w.flag, n_groups, mp, mq, (const uint32_t*)d_tab, exp_windows, (uint8_t*)vo.d_valid);
  } else {
    hipLaunchKernelGGL((k_dsav_tables<MONT_L, MONT_TPI>), quad_grid(n_bases), dim3(RSA_BLOCK), 0, s, n_groups, n_keys, (const uint32_t*)d_bases,
                       (const uint32_t*)d_kg, mp, (uint32_t*)d_tab);
    hipLaunchKernelGGL((k_dsav_exp<MONT_L, MONT_TPI>), quad_grid(n_ops), dim3(RSA_BLOCK), 0, s, n_ops, (const uint32_t*)w.e, (const uint32_t*)w.ok,
                       (const uint32_t*)w.og, (const uint8_t*)w.flag, n_groups, mp, mq, (const uint32_t*)d_tab, exp_windows, (uint8_t*)vo.d_valid);
  }
  // (the host vectors above were copied from pageable memory: each copy call returned when it was done with them)
  return vo.finish(c);
}

}  // namespace

extern "C" {

int bftkv_gpu_dsa_verify(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs, uint32_t qbytes,
                         const uint32_t* key_idx, uint32_t n_keys, const uint8_t* keys_y, const uint32_t* key_group, uint32_t pbytes,
                         uint32_t n_groups, const uint8_t* p, const uint8_t* q, const uint8_t* g, uint8_t* valid_out, uint8_t* status_out) {
  return dsa_verify_impl(c, n_ops, digests, dlen, sigs, qbytes, key_idx, n_keys, keys_y, key_group, pbytes, n_groups, p, q, g, valid_out, status_out, false);
}
int bftkv_gpu_dsa_verify_dev(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs, uint32_t qbytes,
                             const uint32_t* key_idx, uint32_t n_keys, const uint8_t* keys_y, const uint32_t* key_group, uint32_t pbytes,
                             uint32_t n_groups, const uint8_t* p, const uint8_t* q, const uint8_t* g, uint8_t* valid_out, uint8_t* status_out) {
  return dsa_verify_impl(c, n_ops, digests, dlen, sigs, qbytes, key_idx, n_keys, keys_y, key_group, pbytes, n_groups, p, q, g, valid_out, status_out, true);
}

}  // extern "C"
