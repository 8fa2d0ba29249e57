// C ABI of threshold DSA / ECDSA signing, the server's side (include/bftkv_gpu.h: bftkv_gpu_tdsa_share, bftkv_gpu_tecdsa_share, their
// _dev forms and bftkv_gpu_tsig_partial_s; tsig_share_kernels.hip; the rules: docs/parity.md, "Threshold DSA / ECDSA signing
// (dsaContext.Sign)").
namespace {

// The result arrays of a share call.  They fail closed before anything can refuse the call, and again if it fails later.
struct TsigOut {
  uint8_t *ri, *vi, *ki, *ci, *st;      // [n_reqs][ri_bytes], [n_reqs][qw] three times, [n_reqs]
  uint32_t n_reqs;
  size_t ri_bytes, qw;
  bool dev;
  bool counted() const { return n_reqs != 0 && n_reqs <= TSIG_MAX_ROWS; }
  int fill(bftkv_gpu_ctx* c, uint8_t* p, int v, size_t bytes) const {
    if (!p || !bytes) return 0;
    if (dev) HIPCHK(c, hipMemsetAsync(p, v, bytes, c->stream));
    else memset(p, v, bytes);
    return 0;
  }
  int fail_statuses(bftkv_gpu_ctx* c) const { return counted() ? fill(c, st, BFTKV_TH_FAILED, n_reqs) : 0; }
  int fail_closed(bftkv_gpu_ctx* c) const {
    if (!counted()) return 0;
    int rc;
    if ((rc = fill(c, st, BFTKV_TH_FAILED, n_reqs)) || (rc = fill(c, ri, 0, n_reqs * ri_bytes)) || (rc = fill(c, vi, 0, n_reqs * qw)) ||
        (rc = fill(c, ki, 0, n_reqs * qw)) || (rc = fill(c, ci, 0, n_reqs * qw)))
      return rc;
    return 0;
  }
  bool complete() const { return ri && vi && ki && ci && st; }
};

// what refuses a share call whatever its numbers: BFTKV_E_INVALID (the batcher refuses its caller by the same rule)
inline bool tsig_counts_ok(uint32_t n_reqs, uint32_t m) {
  return n_reqs != 0 && n_reqs <= TSIG_MAX_ROWS && m != 0 && m <= TSIG_MAX_M && (uint64_t)n_reqs * m <= TSIG_MAX_ROWS;
}

// where the kernels write: the caller's device arrays, or scratch that tsig_download copies back
struct TsigDev { uint8_t *ri, *vi, *ki, *ci; };
int tsig_device_arrays(bftkv_gpu_ctx* c, ScratchBufs& sb, const TsigOut& o, TsigDev* d) {
  if (o.dev) { *d = TsigDev{o.ri, o.vi, o.ki, o.ci}; return 0; }
  void *a, *b, *e, *f;
  int rc;
  if ((rc = dev_alloc(c, sb, o.n_reqs * o.ri_bytes, &a, false)) || (rc = dev_alloc(c, sb, o.n_reqs * o.qw, &b, false)) ||
      (rc = dev_alloc(c, sb, o.n_reqs * o.qw, &e, false)) || (rc = dev_alloc(c, sb, o.n_reqs * o.qw, &f, false)))
    return rc;
  *d = TsigDev{(uint8_t*)a, (uint8_t*)b, (uint8_t*)e, (uint8_t*)f};
  return 0;
}
// end of a share call: the statuses are OK behind the kernels (stream order); a host caller's arrays are copied back and waited for
int tsig_finish(bftkv_gpu_ctx* c, const TsigOut& o, const TsigDev& d) {
  if (o.dev) {
    HIPCHK(c, hipMemsetAsync(o.st, BFTKV_TH_OK, o.n_reqs, c->stream));
    return finish(c, true);
  }
  HIPCHK(c, hipMemcpyAsync(o.ri, d.ri, o.n_reqs * o.ri_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(o.vi, d.vi, o.n_reqs * o.qw, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(o.ki, d.ki, o.n_reqs * o.qw, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(o.ci, d.ci, o.n_reqs * o.qw, hipMemcpyDeviceToHost, c->stream));
  if (const int rc = finish(c, false)) return rc;
  memset(o.st, BFTKV_TH_OK, o.n_reqs);
  return 0;
}

// DSA: the widths, the window table of every group's g, the rows of p and the constants of q are the set's.  Nothing is read from host
// memory but the host form's own arrays, so the device form never waits.
int tdsa_share_impl(bftkv_gpu_ctx* c, int keyset, uint32_t n_reqs, const uint32_t* group_idx, uint32_t m, const uint8_t* shares, uint8_t* ri_out,
                    uint8_t* vi_out, uint8_t* ki_out, uint8_t* ci_out, uint8_t* status_out, bool dev) {
  if (!c) {
    if (!dev && status_out && n_reqs && n_reqs <= TSIG_MAX_ROWS) memset(status_out, BFTKV_TH_FAILED, n_reqs);
    return BFTKV_E_INVALID;
  }
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  TsigOut o{ri_out, vi_out, ki_out, ci_out, status_out, n_reqs, 0, 0, dev};
  int rc;
  if ((rc = o.fail_statuses(c))) return rc;      // (the widths of the outputs are the set's: not known yet)
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const DsaKeySet* ks = KeySets<DsaKeySet>::find(c, keyset);
  if (!ks) return KeySets<DsaKeySet>::bad_handle(c);
  o.ri_bytes = ks->pbytes; o.qw = ks->qbytes;
  if ((rc = o.fail_closed(c))) return rc;
  if (!tsig_counts_ok(n_reqs, m) || !shares || !o.complete()) return BFTKV_E_INVALID;
  rc = [&]() -> int {
    ScratchBufs sb(c);
    const uint32_t qb = ks->qbytes;
    uint8_t* d_sh;
    uint32_t* d_gi = nullptr;
    void *d_ai, *d_grp, *d_ones, *d_rl;
    TsigDev d;
    int r;
    if ((r = to_dev(c, sb, shares, (size_t)n_reqs * m * 4 * qb, &d_sh, dev))) return r;
    if (group_idx && (r = to_dev(c, sb, group_idx, (size_t)n_reqs, &d_gi, dev))) return r;
    if ((r = tsig_device_arrays(c, sb, o, &d))) return r;
    if ((r = dev_alloc(c, sb, (size_t)n_reqs * DSAV_EXP_LIMBS * 4, &d_ai, false)) || (r = dev_alloc(c, sb, (size_t)n_reqs * 4, &d_grp, false)) ||
        (r = dev_alloc(c, sb, (size_t)ks->n_groups * MONT_N * 4, &d_ones, false)) || (r = dev_alloc(c, sb, (size_t)n_reqs * MONT_N * 4, &d_rl, false)))
      return r;
    hipStream_t s = c->stream;
    hipLaunchKernelGGL(k_tsig_fold<8>, dim3((n_reqs + EC_BLOCK - 1) / EC_BLOCK), dim3(EC_BLOCK), 0, s, n_reqs, m, (const uint8_t*)d_sh, qb,
                       (const uint32_t*)d_gi, ks->n_groups, ks->qc.as<TsigMod<8>>(), d.vi, d.ki, d.ci, (uint32_t*)d_ai, 1u, (uint32_t*)d_grp);
    hipLaunchKernelGGL(k_tsig_ones, quad_grid(ks->n_groups), dim3(RSA_BLOCK), 0, s, ks->n_groups, ks->modp.view(), (uint32_t*)d_ones);
    hipLaunchKernelGGL(k_tsig_gpow, quad_grid(n_reqs), dim3(RSA_BLOCK), 0, s, n_reqs, (const uint32_t*)d_ai, (const uint32_t*)d_grp, ks->modp.view(),
                       ks->tab.as<uint32_t>(), (const uint32_t*)d_ones, ks->w, ks->windows, (uint32_t*)d_rl);
    hipLaunchKernelGGL(k_limbs_to_bytes, dim3((uint32_t)(((size_t)n_reqs * ks->pbytes + 255) / 256)), dim3(256), 0, s, (const uint32_t*)d_rl, ks->pbytes,
                       n_reqs, d.ri);
    return tsig_finish(c, o, d);
  }();
  if (rc) (void)o.fail_closed(c);
  return rc;
}

// ECDSA: q is the curve's N, the table of G the context's (ec_fb_table).
int tecdsa_share_impl(bftkv_gpu_ctx* c, uint32_t n_reqs, uint32_t m, const uint8_t* shares, const uint8_t* curve, uint32_t bit_size, uint8_t* ri_out,
                      uint8_t* vi_out, uint8_t* ki_out, uint8_t* ci_out, uint8_t* status_out, bool dev) {
  const bool sized = bit_size != 0 && bit_size <= 521;
  const uint32_t f = (bit_size + 7) / 8;
  TsigOut o{ri_out, vi_out, ki_out, ci_out, status_out, n_reqs, sized ? 1 + 2 * (size_t)f : 0, sized ? f : 0, dev};
  if (!c) {
    if (!dev) (void)o.fail_closed(nullptr);      // (host arrays: no device call behind it)
    return BFTKV_E_INVALID;
  }
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = o.fail_closed(c))) return rc;
  if (!sized || !curve || !tsig_counts_ok(n_reqs, m) || !shares || !o.complete()) return BFTKV_E_INVALID;
  const int id = ec_curve_id(curve, bit_size);
  if (id < 0) return BFTKV_E_UNSUPPORTED;
  rc = 0;
  ScratchBufs sb(c);
  ec_dispatch(id, curve, [&](auto C) {
    constexpr int L = decltype(C)::kWords;
    const uint32_t* tab;
    uint32_t w, nwin;
    if ((rc = ec_fb_table<L>(c, id, C, &tab, &w, &nwin))) return;
    TsigMod<L> hm;
    ecf::fe_copy<L>(hm.q, C.n);
    ecf::fe_copy<L>(hm.rr, C.rr_n);
    hm.q0inv = C.n0inv;
    uint8_t* d_sh;
    TsigMod<L>* d_mod;
    void* d_ai;
    TsigDev d;
    if ((rc = to_dev(c, sb, &hm, 1, &d_mod)) || (rc = to_dev(c, sb, shares, (size_t)n_reqs * m * 4 * f, &d_sh, dev)) ||
        (rc = tsig_device_arrays(c, sb, o, &d)) || (rc = dev_alloc(c, sb, (size_t)n_reqs * L * 4, &d_ai, false)))
      return;
    hipStream_t s = c->stream;
    const dim3 grid((n_reqs + EC_BLOCK - 1) / EC_BLOCK), block(EC_BLOCK);
    hipLaunchKernelGGL(k_tsig_fold<L>, grid, block, 0, s, n_reqs, m, (const uint8_t*)d_sh, f, (const uint32_t*)nullptr, 1u, (const TsigMod<L>*)d_mod, d.vi,
                       d.ki, d.ci, (uint32_t*)d_ai, 0u, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_tsig_gmul<L>, grid, block, 0, s, n_reqs, (const uint32_t*)d_ai, C, tab, w, nwin, d.ri);
    rc = tsig_finish(c, o, d);
  });
  if (rc) (void)o.fail_closed(c);
  return rc;
}

// Phase 3 for both schemes (only q differs).  L = 8 words hold a row of up to 32 bytes, 17 words one of up to 66.
template <int L>
int tsig_s_run(bftkv_gpu_ctx* c, uint32_t n_reqs, const uint8_t* m_in, const uint8_t* r, const uint8_t* y, const uint8_t* k, const uint8_t* cc,
               uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* q, uint8_t* si_out) {
  std::vector<TsigMod<L>> hm(n_mods);
  for (uint32_t i = 0; i < n_mods; ++i) tsig_mod_setup<L>(hm[i], q + (size_t)i * nbytes, nbytes);
  std::vector<uint32_t> idx(n_reqs, 0u);
  if (mod_idx) for (uint32_t i = 0; i < n_reqs; ++i) idx[i] = std::min(mod_idx[i], n_mods - 1u);
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  const size_t bytes = (size_t)n_reqs * nbytes;
  TsigMod<L>* d_mod;
  uint32_t* d_idx;
  uint8_t *d_m, *d_r, *d_y, *d_k, *d_c;
  void* d_si;
  int rc;
  if ((rc = to_dev(c, sb, hm.data(), (size_t)n_mods, &d_mod)) || (rc = to_dev(c, sb, idx.data(), (size_t)n_reqs, &d_idx)) ||
      (rc = to_dev(c, sb, m_in, bytes, &d_m)) || (rc = to_dev(c, sb, r, bytes, &d_r)) || (rc = to_dev(c, sb, y, bytes, &d_y)) ||
      (rc = to_dev(c, sb, k, bytes, &d_k)) || (rc = to_dev(c, sb, cc, bytes, &d_c)) || (rc = dev_alloc(c, sb, bytes, &d_si, false)))
    return rc;
  hipLaunchKernelGGL(k_tsig_s<L>, dim3((n_reqs + EC_BLOCK - 1) / EC_BLOCK), dim3(EC_BLOCK), 0, c->stream, n_reqs, (const uint8_t*)d_m, (const uint8_t*)d_r,
                     (const uint8_t*)d_y, (const uint8_t*)d_k, (const uint8_t*)d_c, nbytes, (const uint32_t*)d_idx, (const TsigMod<L>*)d_mod, (uint8_t*)d_si);
  HIPCHK(c, hipMemcpyAsync(si_out, d_si, bytes, hipMemcpyDeviceToHost, c->stream));
  return finish(c, false);      // (the local vectors were copied from pageable memory: each copy call returned when it was done with them)
}

int tsig_partial_s_impl(bftkv_gpu_ctx* c, uint32_t n_reqs, const uint8_t* m_in, const uint8_t* r, const uint8_t* y, const uint8_t* k, const uint8_t* cc,
                        uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* q, uint8_t* si_out, uint8_t* status_out) {
  const bool shaped = n_reqs != 0 && n_reqs <= TSIG_MAX_ROWS && nbytes != 0 && nbytes <= TSIG_MAX_NBYTES;
  auto fail_closed = [&]() {
    if (!shaped) return;
    if (status_out) memset(status_out, BFTKV_TH_FAILED, n_reqs);
    if (si_out) memset(si_out, 0, (size_t)n_reqs * nbytes);
  };
  fail_closed();
  if (!c || !shaped || n_mods == 0 || !m_in || !r || !y || !k || !cc || !q || !si_out || !status_out) return BFTKV_E_INVALID;
  for (uint32_t i = 0; i < n_mods; ++i) if (!(q[(size_t)(i + 1) * nbytes - 1] & 1)) return BFTKV_E_UNSUPPORTED;      // an even q (0 included)
  const int rc = nbytes <= 32 ? tsig_s_run<8>(c, n_reqs, m_in, r, y, k, cc, nbytes, mod_idx, n_mods, q, si_out)
                              : tsig_s_run<17>(c, n_reqs, m_in, r, y, k, cc, nbytes, mod_idx, n_mods, q, si_out);
  if (rc) fail_closed();
  else memset(status_out, BFTKV_TH_OK, n_reqs);
  return rc;
}

}  // namespace

extern "C" {

int bftkv_gpu_tdsa_share(bftkv_gpu_ctx* c, int dsa_keyset, uint32_t n_reqs, const uint32_t* group_idx, uint32_t m, const uint8_t* shares, uint8_t* ri_out,
                         uint8_t* vi_out, uint8_t* ki_out, uint8_t* ci_out, uint8_t* status_out) {
  return tdsa_share_impl(c, dsa_keyset, n_reqs, group_idx, m, shares, ri_out, vi_out, ki_out, ci_out, status_out, false);
}
int bftkv_gpu_tdsa_share_dev(bftkv_gpu_ctx* c, int dsa_keyset, uint32_t n_reqs, const uint32_t* group_idx, uint32_t m, const uint8_t* shares,
                             uint8_t* ri_out, uint8_t* vi_out, uint8_t* ki_out, uint8_t* ci_out, uint8_t* status_out) {
  return tdsa_share_impl(c, dsa_keyset, n_reqs, group_idx, m, shares, ri_out, vi_out, ki_out, ci_out, status_out, true);
}
int bftkv_gpu_tecdsa_share(bftkv_gpu_ctx* c, uint32_t n_reqs, uint32_t m, const uint8_t* shares, const uint8_t* curve, uint32_t bit_size, uint8_t* ri_out,
                           uint8_t* vi_out, uint8_t* ki_out, uint8_t* ci_out, uint8_t* status_out) {
  return tecdsa_share_impl(c, n_reqs, m, shares, curve, bit_size, ri_out, vi_out, ki_out, ci_out, status_out, false);
}
int bftkv_gpu_tecdsa_share_dev(bftkv_gpu_ctx* c, uint32_t n_reqs, uint32_t m, const uint8_t* shares, const uint8_t* curve, uint32_t bit_size,
                               uint8_t* ri_out, uint8_t* vi_out, uint8_t* ki_out, uint8_t* ci_out, uint8_t* status_out) {
  return tecdsa_share_impl(c, n_reqs, m, shares, curve, bit_size, ri_out, vi_out, ki_out, ci_out, status_out, true);
}
int bftkv_gpu_tsig_partial_s(bftkv_gpu_ctx* c, uint32_t n_reqs, const uint8_t* m_in, const uint8_t* r, const uint8_t* y, const uint8_t* k,
                             const uint8_t* cc, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* q, uint8_t* si_out,
                             uint8_t* status_out) {
  return tsig_partial_s_impl(c, n_reqs, m_in, r, y, k, cc, nbytes, mod_idx, n_mods, q, si_out, status_out);
}

}  // extern "C"
