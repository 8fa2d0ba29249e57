// C ABI of the threshold-ECDSA entry points (include/bftkv_gpu.h): CalculateR and CalculatePartialR of
// crypto/threshold/ecdsa/ecdsa.go over crypto/elliptic's four curves, and crypto/ecdsa.Verify on raw signatures, with the key
// in the call or in a resident key set.  Kernels: ec_kernels.hip.
namespace {

// The groups the library recognises, by value: P, N, B, Gx, Gy (big-endian hex) and BitSize of crypto/elliptic's curves.  The
// reference builds its group from the wire (ParseParams, ecdsa.go:105-123) and runs Go's generic a = -3 code on it; any other
// group is refused for the whole call.
struct EcNamedCurve {
  uint32_t bits;
  const char* hex[5];
};
const EcNamedCurve kEcCurves[4] = {
    {224,
     {"ffffffffffffffffffffffffffffffff000000000000000000000001", "ffffffffffffffffffffffffffff16a2e0b8f03e13dd29455c5c2a3d",
      "b4050a850c04b3abf54132565044b0b7d7bfd8ba270b39432355ffb4", "b70e0cbd6bb4bf7f321390b94a03c1d356c21122343280d6115c1d21",
      "bd376388b5f723fb4c22dfe6cd4375a05a07476444d5819985007e34"}},
    {256,
     {"ffffffff00000001000000000000000000000000ffffffffffffffffffffffff", "ffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551",
      "5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b", "6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296",
      "4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5"}},
    {384,
     {"fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffeffffffff0000000000000000ffffffff",
      "ffffffffffffffffffffffffffffffffffffffffffffffffc7634d81f4372ddf581a0db248b0a77aecec196accc52973",
      "b3312fa7e23ee7e4988e056be3f82d19181d9c6efe8141120314088f5013875ac656398d8a2ed19d2a85c8edd3ec2aef",
      "aa87ca22be8b05378eb1c71ef320ad746e1d3b628ba79b9859f741e082542a385502f25dbf55296c3a545e3872760ab7",
      "3617de4a96262c6f5d9e98bf9292dc29f8f41dbd289a147ce9da3113b5f0b8c00a60b1ce1d7e819d7a431d7c90ea0e5f"}},
    {521,
     {"01ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
      "01fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffa51868783bf2f966b7fcc0148f709a5d03bb5c9b8899c47aebb6fb71e91386409",
      "0051953eb9618e1c9a1f929a21a0b68540eea2da725b99b315f3b8b489918ef109e156193951ec7e937b1652c0bd3bb1bf073573df883d2c34f1ef451fd46b503f00",
      "00c6858e06b70404e9cd9e3ecb662395b4429c648139053fb521f828af606b4d3dbaa14b5e77efe75928fe1dc127a2ffa8de3348b3c1856a429bf97e7e31c2e5bd66",
      "011839296a789a3bc0045c8a5fb42c7d1bd998f54449579b446817afbd17273e662c97ee72995ef42640c550b9013fad0761353c7086a272c24088be94769fd16650"}},
};

// curve: P || N || B || Gx || Gy, (bit_size + 7) / 8 bytes each.  Index into kEcCurves, or -1.
int ec_curve_id(const uint8_t* curve, uint32_t bit_size) {
  for (int id = 0; id < 4; ++id) {
    const EcNamedCurve& nc = kEcCurves[id];
    if (nc.bits != bit_size) continue;
    const uint32_t f = (bit_size + 7) / 8;
    bool same = true;
    for (int part = 0; part < 5 && same; ++part)
      for (uint32_t i = 0; i < f && same; ++i) {
        const char* h = nc.hex[part] + 2 * i;
        auto nib = [](char ch) { return (uint32_t)(ch <= '9' ? ch - '0' : ch - 'a' + 10); };
        same = curve[(size_t)part * f + i] == (uint8_t)(nib(h[0]) << 4 | nib(h[1]));
      }
    if (same) return id;
  }
  return -1;
}

// The word count per curve: 7, 8, 12, 17.  f(ecf::Curve<L>) is called with the curve's constants, built on the host.
template <typename F>
void ec_dispatch(int id, const uint8_t* curve, F&& f) {
  const uint32_t fb = (kEcCurves[id].bits + 7) / 8;
  switch (id) {
    case 0: { ecf::Curve<7> C; ecf::curve_setup<7>(C, curve, fb); f(C); break; }
    case 1: { ecf::Curve<8> C; ecf::curve_setup<8>(C, curve, fb); f(C); break; }
    case 2: { ecf::Curve<12> C; ecf::curve_setup<12>(C, curve, fb); f(C); break; }
    default: { ecf::Curve<17> C; ecf::curve_setup<17>(C, curve, fb); f(C); break; }
  }
}

// status bytes start out as BFTKV_TH_FAILED: whatever the call does not reach stays a failure
int ec_status_failed(bftkv_gpu_ctx* c, uint8_t* status_out, uint32_t n_ops, bool dev) {
  if (dev) HIPCHK(c, hipMemsetAsync(status_out, BFTKV_TH_FAILED, n_ops, c->stream));
  else memset(status_out, BFTKV_TH_FAILED, n_ops);
  return 0;
}

// The two result arrays of a verification call (verdict and status byte per signature), shared by the ECDSA and DSA impls.
struct VerdictOut {
  uint8_t *valid_out, *status_out;
  uint32_t n_ops;
  bool dev;
  void *d_valid = nullptr, *d_st = nullptr;      // where the kernels write: the caller's device arrays, or scratch (device_arrays)
  // fail closed: whatever refuses the call afterwards leaves failed statuses and zero verdicts behind
  int fail_closed(bftkv_gpu_ctx* c) {
    if (!n_ops) return 0;
    if (int rc = ec_status_failed(c, status_out, n_ops, dev)) return rc;
    if (dev) HIPCHK(c, hipMemsetAsync(valid_out, 0, n_ops, c->stream));
    else memset(valid_out, 0, n_ops);
    return 0;
  }
  int device_arrays(bftkv_gpu_ctx* c, ScratchBufs& sb) {
    if (dev) { d_valid = valid_out; d_st = status_out; return 0; }
    if (int rc = dev_alloc(c, sb, n_ops, &d_valid, false)) return rc;
    return dev_alloc(c, sb, n_ops, &d_st, false);
  }
  // end of the call: a host caller's arrays are copied back and waited for
  int finish(bftkv_gpu_ctx* c) {
    if (!dev) {
      HIPCHK(c, hipMemcpyAsync(valid_out, d_valid, n_ops, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(status_out, d_st, n_ops, hipMemcpyDeviceToHost, c->stream));
    }
    return ::finish(c, dev);
  }
};

// The head of a verification against a resident key set, for every kind.  In this order: what is refused before the lock leaves the
// caller's arrays alone; the result arrays fail closed; the call's shape (shape_ok, worked out by the caller from its arguments) is
// refused; the fork takes its hold on the root's tables; the handle is looked up; an empty call ends.  body(set, vo) then runs with
// c->mu and KtRead held, which is what KeySets::find asks of whoever uses the set.
template <typename Set, typename Body>
int verify_on_keyset(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, uint32_t max_ops, uint8_t* valid_out, uint8_t* status_out, bool dev, bool shape_ok,
                     Body&& body) {
  if (!c || n_ops > max_ops || (n_ops && (!valid_out || !status_out))) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  VerdictOut vo{valid_out, status_out, n_ops, dev};
  if (const int rc = vo.fail_closed(c)) return rc;
  if (!shape_ok) return BFTKV_E_INVALID;
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const Set* ks = KeySets<Set>::find(c, keyset);
  if (!ks) return KeySets<Set>::bad_handle(c);
  if (n_ops == 0) return 0;
  return body(*ks, vo);
}

int ecdsa_calculate_r_impl(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ri, const uint8_t* vi,
                           const uint8_t* curve, uint32_t bit_size, uint8_t* r_out, uint8_t* status_out, bool dev) {
  if (!c || !curve || bit_size == 0 || bit_size > 521 || k == 0 || k > 1024 || (uint64_t)n_ops * k > (1u << 24) ||
      (n_ops && (!xs || !ri || !vi || !r_out || !status_out)))
    return BFTKV_E_INVALID;
  const int id = ec_curve_id(curve, bit_size);
  if (id < 0) return BFTKV_E_UNSUPPORTED;
  if (n_ops == 0) return 0;
  const uint32_t f = (bit_size + 7) / 8;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ec_status_failed(c, status_out, n_ops, dev))) return rc;
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mq;
  uint32_t *d_vi, *d_gi;
  int32_t* d_xs;
  uint8_t* d_ri;
  void *d_inv, *d_st, *d_lam, *d_v, *d_vinv, *d_r;
  const size_t nk = (size_t)n_ops * k, rw = 1 + 2 * (size_t)f;
  if ((rc = make_modtab(c, sb, curve + f, 1, f, &mq))) return rc;                  // N: the Lagrange coefficients and v live mod N
  if ((rc = idx_to_dev(c, sb, nullptr, n_ops, 1, &d_gi, true))) return rc;           // (one group per call: every index 0)
  if ((rc = to_dev_limbs(c, sb, vi, nk, f, &d_vi, dev))) return rc;
  if ((rc = to_dev(c, sb, xs, nk, &d_xs, dev))) return rc;
  if ((rc = to_dev(c, sb, ri, nk * rw, &d_ri, dev))) return rc;
  if ((rc = dev_alloc(c, sb, nk * MONT_N * 4, &d_inv, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_st, true)) ||
      (rc = dev_alloc(c, sb, nk * MONT_N * 4, &d_lam, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_v, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_vinv, false)))
    return rc;
  if (dev) d_r = r_out;
  else if ((rc = dev_alloc(c, sb, (size_t)n_ops * f, &d_r, false))) return rc;
  hipStream_t s = c->stream;
  // l_j mod N (written out: they become scalars) and v = sum Vi_j l_j mod N, exactly as on the DSA path
  hipLaunchKernelGGL(k_lagrange_inv, dim3((uint32_t)((nk + 63) / 64)), dim3(64), 0, s, n_ops, k, d_xs, d_gi, mq, (uint32_t*)d_inv, (uint8_t*)d_st);
  hipLaunchKernelGGL(k_lagrange_terms, quad_grid(n_ops), dim3(RSA_BLOCK), 0, s, n_ops, k, (uint32_t*)d_inv, d_vi, d_gi, mq, (uint32_t*)d_lam,
                     (uint32_t*)d_v, (const uint8_t*)d_st);
  if (dev ? !lagrange_bound_says_small(c, k) : lagrange_needs_big(xs, n_ops, k))
    if ((rc = lagrange_big_path(c, sb, n_ops, k, d_xs, d_vi, d_gi, mq, (uint32_t*)d_lam, (uint32_t*)d_v, (uint8_t*)d_st, f))) return rc;
  // w = v^-1 mod N (N is up to 521 bits: the general inverse, not the 256-bit one); v = 0 sets status bit 1
  hipLaunchKernelGGL(k_modinv, dim3((n_ops + 63) / 64), dim3(64), 0, s, n_ops, (const uint32_t*)d_v, (const uint32_t*)d_gi, mq, (uint32_t*)d_vinv,
                     (uint8_t*)d_st, (const uint8_t*)nullptr, (const uint8_t*)nullptr);
  // The work split (DESIGN.md section 3): a lane per (operation, term) and an ordered fold per operation.  One lane per operation
  // (BFTKV_EC_SPLIT=2) measured 2.9-4.0x slower at 10,000 operations and 5-13x for a lone call (k = 8 and 22, P-224 to P-384): it
  // leaves k times fewer waves to hide 256-VGPR latencies with.
  const bool per_op = c->ec_split == 2;
  void* d_t = nullptr;
  ec_dispatch(id, curve, [&](auto C) {
    constexpr int L = decltype(C)::kWords;
    if constexpr (L <= 12) {       // (P-521: a term and a running sum in one lane do not fit 256 VGPRs without scratch)
      if (per_op) {
        hipLaunchKernelGGL(k_ec_calc_r_op<L>, dim3((n_ops + EC_BLOCK - 1) / EC_BLOCK), dim3(EC_BLOCK), 0, s, n_ops, k, (const uint8_t*)d_ri,
                           (const uint32_t*)d_lam, (const uint32_t*)d_vinv, C, (uint8_t*)d_st, (uint8_t*)d_r);
        return;
      }
    }
    if ((rc = dev_alloc(c, sb, nk * 3 * L * 4, &d_t, false))) return;
    hipLaunchKernelGGL(k_ec_terms<L>, dim3((uint32_t)((nk + EC_BLOCK - 1) / EC_BLOCK)), dim3(EC_BLOCK), 0, s, n_ops, k, (const uint8_t*)d_ri,
                       (const uint32_t*)d_lam, (const uint32_t*)d_vinv, C, (uint32_t*)d_t, (uint8_t*)d_st);
    hipLaunchKernelGGL(k_ec_fold<L>, dim3((n_ops + EC_BLOCK - 1) / EC_BLOCK), dim3(EC_BLOCK), 0, s, n_ops, k, (const uint32_t*)d_t, C, (uint8_t*)d_st,
                       (uint8_t*)d_r);
  });
  if (rc) return rc;
  if (!dev) HIPCHK(c, hipMemcpyAsync(r_out, d_r, (size_t)n_ops * f, hipMemcpyDeviceToHost, s));
  if ((rc = copy_status(c, status_out, d_st, n_ops, dev))) return rc;
  return finish(c, dev);
}

int ec_scalar_base_mult_impl(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* scalars, uint32_t sbytes, const uint8_t* curve, uint32_t bit_size,
                             uint8_t* out, uint8_t* status_out) {
  if (!c || !curve || bit_size == 0 || bit_size > 521 || n_ops > (1u << 24) || (n_ops && (!scalars || !out || !status_out))) return BFTKV_E_INVALID;
  const int id = ec_curve_id(curve, bit_size);
  if (id < 0) return BFTKV_E_UNSUPPORTED;
  const uint32_t f = (bit_size + 7) / 8;
  if (sbytes == 0 || sbytes > f) return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ec_status_failed(c, status_out, n_ops, false))) return rc;
  ScratchBufs sb(c);
  uint8_t* d_s;
  void *d_out, *d_st;
  const size_t ow = 1 + 2 * (size_t)f;
  if ((rc = to_dev(c, sb, scalars, (size_t)n_ops * sbytes, &d_s))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * ow, &d_out, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_st, false))) return rc;
  hipStream_t s = c->stream;
  ec_dispatch(id, curve, [&](auto C) {
    constexpr int L = decltype(C)::kWords;
    hipLaunchKernelGGL(k_ec_base_mult<L>, dim3((n_ops + EC_BLOCK - 1) / EC_BLOCK), dim3(EC_BLOCK), 0, s, n_ops, (const uint8_t*)d_s, sbytes, C,
                       (uint8_t*)d_out, (uint8_t*)d_st);
  });
  HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)n_ops * ow, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(status_out, d_st, n_ops, hipMemcpyDeviceToHost, s));
  return finish(c, false);
}

// The fixed-base table of G for curve `id` on this context (ec_field.h fb_table_build), built and uploaded at the curve's first
// verification and kept until the context goes.  Window width: 4 bits (BFTKV_EC_WINDOW tries others; DESIGN.md section 4).
template <int L>
int ec_fb_table(bftkv_gpu_ctx* c, int id, const ecf::Curve<L>& C, const uint32_t** tab, uint32_t* w_out, uint32_t* nwin_out) {
  const uint32_t w = c->ec_window >= 2 && c->ec_window <= 8 ? c->ec_window : 4;
  const uint32_t nwin = ecf::fb_windows(C.fbytes, w);
  if (c->ec_fb_w[id] != w) {
    std::vector<uint32_t> host(ecf::fb_table_words<L>(w, nwin));
    ecf::fb_table_build<L>(host.data(), w, nwin, C);
    HIPCHK(c, hipStreamSynchronize(c->stream));            // (a table of another width may still be read)
    int rc;
    if ((rc = upload(c, c->ec_fb_tab[id], host))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));            // the vector dies here
    c->ec_fb_w[id] = w;
  }
  *tab = c->ec_fb_tab[id].as<uint32_t>();
  *w_out = w;
  *nwin_out = nwin;
  return 0;
}

// The chain of an ECDSA verification, with the keys in the call or in a resident set: the per-signature arrays to the device, the
// scratch, the result arrays, then k_ecv_prep, k_modinv (w = s^-1 mod N), k_ecv_base (u1 G from the curve's table `gtab` of width w)
// and the kernel that adds u2 Q and compares.  Only that last one differs: key_kernel(C, grid, block, t) launches it on c->stream
// over the scratch t.  mq: N's rows.
struct EcvScratch { const uint32_t *r, *ki, *u2, *pt; const uint8_t *flag, *ibad; };
template <int L, typename KeyKernel>
int ecv_chain(bftkv_gpu_ctx* c, ScratchBufs& sb, VerdictOut& vo, const ecf::Curve<L>& C, uint32_t bit_size, const uint8_t* digests, uint32_t dlen,
              const uint8_t* sigs, const uint32_t* key_idx, uint32_t n_keys, const ModTab& mq, const uint32_t* gtab, uint32_t w, uint32_t nwin,
              KeyKernel&& key_kernel) {
  const uint32_t n_ops = vo.n_ops, f = (bit_size + 7) / 8;
  const bool dev = vo.dev;
  uint32_t *d_gi, *d_ki = nullptr;
  uint8_t *d_dg, *d_sig;
  void *d_s28, *d_w28, *d_e, *d_r, *d_flag, *d_ibad, *d_pt, *d_u2;
  int rc;
  if ((rc = idx_to_dev(c, sb, nullptr, n_ops, 1, &d_gi, true))) return rc;
  if (key_idx) {                                                                       // clamped on the device, for host callers too
    uint32_t* raw;
    if ((rc = to_dev(c, sb, key_idx, n_ops, &raw, dev)) || (rc = idx_to_dev(c, sb, raw, n_ops, n_keys, &d_ki, true))) return rc;
  }
  if ((rc = to_dev(c, sb, digests, (size_t)n_ops * dlen, &d_dg, dev))) return rc;
  if ((rc = to_dev(c, sb, sigs, (size_t)n_ops * 2 * f, &d_sig, dev))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_s28, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_w28, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_flag, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_ibad, true)))
    return rc;
  if ((rc = vo.device_arrays(c, sb))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * L * 4, &d_e, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * L * 4, &d_u2, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops * L * 4, &d_r, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * 3 * L * 4, &d_pt, false)))
    return rc;
  hipStream_t s = c->stream;
  const dim3 grid((n_ops + EC_BLOCK - 1) / EC_BLOCK), block(EC_BLOCK);
  hipLaunchKernelGGL(k_ecv_prep<L>, grid, block, 0, s, n_ops, (const uint8_t*)d_dg, dlen, bit_size, (const uint8_t*)d_sig, C, (uint32_t*)d_s28,
                     (uint32_t*)d_e, (uint32_t*)d_r, (uint8_t*)d_flag);
  // w = s^-1 mod N: the general inverse (N reaches 521 bits), as in CalculateR
  hipLaunchKernelGGL(k_modinv, dim3((n_ops + 63) / 64), dim3(64), 0, s, n_ops, (const uint32_t*)d_s28, (const uint32_t*)d_gi, mq, (uint32_t*)d_w28,
                     (uint8_t*)d_ibad, (const uint8_t*)nullptr, (const uint8_t*)nullptr);
  hipLaunchKernelGGL(k_ecv_base<L>, grid, block, 0, s, n_ops, (const uint32_t*)d_r, (const uint32_t*)d_e, (const uint32_t*)d_w28,
                     (const uint8_t*)d_flag, C, gtab, w, nwin, (uint32_t*)d_pt, (uint32_t*)d_u2);
  key_kernel(C, grid, block, EcvScratch{(const uint32_t*)d_r, d_ki, (const uint32_t*)d_u2, (const uint32_t*)d_pt, (const uint8_t*)d_flag, (const uint8_t*)d_ibad});
  return vo.finish(c);
}

int ecdsa_verify_impl(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs, const uint32_t* key_idx,
                      uint32_t n_keys, const uint8_t* keys, const uint8_t* curve, uint32_t bit_size, uint8_t* valid_out, uint8_t* status_out, bool dev) {
  if (!c || !curve || !keys || bit_size == 0 || bit_size > 521 || n_keys == 0 || n_keys > (1u << 24) || dlen == 0 || dlen > 66 || n_ops > (1u << 24) ||
      (n_ops && (!digests || !sigs || !valid_out || !status_out)))
    return BFTKV_E_INVALID;
  const int id = ec_curve_id(curve, bit_size);
  if (id < 0) return BFTKV_E_UNSUPPORTED;
  if (n_ops == 0) return 0;
  const uint32_t f = (bit_size + 7) / 8;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  VerdictOut vo{valid_out, status_out, n_ops, dev};
  if ((rc = vo.fail_closed(c))) return rc;
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mq;
  uint8_t* d_keys;
  if ((rc = make_modtab(c, sb, curve + f, 1, f, &mq))) return rc;                      // N, for k_modinv
  if ((rc = to_dev(c, sb, keys, (size_t)n_keys * (1 + 2 * f), &d_keys))) return rc;
  ec_dispatch(id, curve, [&](auto C) {
    constexpr int L = decltype(C)::kWords;
    const uint32_t* tab;
    uint32_t w, nwin;
    if ((rc = ec_fb_table<L>(c, id, C, &tab, &w, &nwin))) return;
    rc = ecv_chain<L>(c, sb, vo, C, bit_size, digests, dlen, sigs, key_idx, n_keys, mq, tab, w, nwin,
                      [&](const ecf::Curve<L>& cv, dim3 grid, dim3 block, const EcvScratch& t) {
                        hipLaunchKernelGGL(k_ecv_key<L>, grid, block, 0, c->stream, vo.n_ops, t.r, (const uint8_t*)d_keys, t.ki, n_keys, t.u2, t.pt, t.flag,
                                           t.ibad, cv, (uint8_t*)vo.d_valid, (uint8_t*)vo.d_st);
                      });
  });
  return rc;
}

// ---- resident key sets ----------------------------------------------------------------------------------------------------
// A long-lived key (the distributed CA key of a threshold signature) is registered once: elliptic.Unmarshal's checks and a
// fixed-base table per key run on the device at bftkv_gpu_ecdsa_keyset_create, and every verification after that takes u2 Q
// from the key's table as it takes u1 G from the curve's.  Sets live on the root context like quorums: created and destroyed
// there under KtWrite (the forks' calls in flight drain first), read by the forks under KtRead without a copy.
constexpr uint32_t EC_KEYSET_MAX_KEYS = 4096;
constexpr size_t EC_KEYSET_TMP_BYTES = (size_t)256 << 20;      // k_ec_keytab_build's temporaries per launch: the keys go in chunks

int ecdsa_keyset_create_impl(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys, const uint8_t* curve, uint32_t bit_size, int* keyset_out) {
  if (!c || !keys || !curve || !keyset_out || bit_size == 0 || bit_size > 521 || n_keys == 0 || n_keys > EC_KEYSET_MAX_KEYS) return BFTKV_E_INVALID;
  const int id = ec_curve_id(curve, bit_size);
  if (id < 0) return BFTKV_E_UNSUPPORTED;
  const uint32_t f = (bit_size + 7) / 8;
  ctx_lock lk(c->mu);
  DevBuf tmp;
  const int created = KeySets<EcKeySet>::create(c, keyset_out, [&](EcKeySet& ks) -> int {
    ScratchBufs sb(c);
    { int grc = modtab_gc(c); if (grc) return grc; }
    int rc = 0;
    ks.curve_id = id; ks.bits = bit_size; ks.n_keys = n_keys;
    ks.curve.assign(curve, curve + 5 * (size_t)f);
    ModTab mq;                                                                     // N's rows, for k_modinv
    if ((rc = make_modtab(c, sb, curve + f, 1, f, &mq)) || (rc = ks.mod.copy_from<EcKeySet>(c, mq, 1, true))) return rc;
    uint8_t* d_keys;
    if ((rc = to_dev(c, sb, keys, (size_t)n_keys * (1 + 2 * f), &d_keys))) return rc;
    ec_dispatch(id, curve, [&](auto C) {
      constexpr int L = decltype(C)::kWords;
      const uint32_t* gtab;
      if ((rc = ec_fb_table<L>(c, id, C, &gtab, &ks.w, &ks.nwin))) return;          // the set keeps the width of the G table for life
      ks.key_words = ecf::fb_table_words<L>(ks.w, ks.nwin);
      const size_t tab_bytes = (size_t)n_keys * ks.key_words * 4, per = ((size_t)1 << ks.w) - 1;
      const size_t key_tmp = (size_t)ks.nwin * per * 2 * L * 4;
      const uint32_t chunk = (uint32_t)std::min<size_t>(n_keys, std::max<size_t>(1, EC_KEYSET_TMP_BYTES / key_tmp));
      if (ks.tab.ensure_exact(tab_bytes) != hipSuccess || ks.refused.ensure(n_keys) != hipSuccess || tmp.ensure_exact(chunk * key_tmp) != hipSuccess) {
        rc = KeySets<EcKeySet>::nomem(c);
        return;
      }
      if (hipMemsetAsync(ks.tab.p, 0, tab_bytes, c->stream) != hipSuccess) { rc = fail(c, BFTKV_E_DEVICE, "hipMemsetAsync"); return; }
      for (uint32_t k0 = 0; k0 < n_keys; k0 += chunk) {
        const uint32_t nk = std::min(chunk, n_keys - k0);
        hipLaunchKernelGGL(k_ec_keytab_build<L>, dim3((nk * ks.nwin + EC_BLOCK - 1) / EC_BLOCK), dim3(EC_BLOCK), 0, c->stream, nk,
                           (const uint8_t*)d_keys + (size_t)k0 * (1 + 2 * f), C, ks.w, ks.nwin, tmp.as<uint32_t>(),
                           ks.tab.as<uint32_t>() + (size_t)k0 * ks.key_words, ks.refused.as<uint8_t>() + k0);
      }
    });
    if (rc) return rc;
    std::vector<uint8_t> refused(n_keys);
    HIPCHK(c, hipMemcpyAsync(refused.data(), ks.refused.p, n_keys, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    for (uint8_t r : refused) ks.n_refused += r != 0;
    return 0;
  });
  tmp.release();          // (k_ec_keytab_build's temporaries: the stream is idle by now, built or not)
  return created;
}

int ecdsa_keyset_destroy_impl(bftkv_gpu_ctx* c, int keyset) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  return KeySets<EcKeySet>::retire(c, keyset);
}

int ecdsa_keyset_info_impl(bftkv_gpu_ctx* c, int keyset, uint32_t* n_keys_out, uint32_t* n_refused_out, uint32_t* window_bits_out,
                           uint64_t* table_bytes_out) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const EcKeySet* ks = KeySets<EcKeySet>::find(c, keyset);
  if (!ks) return KeySets<EcKeySet>::bad_handle(c);
  if (n_keys_out) *n_keys_out = ks->n_keys;
  if (n_refused_out) *n_refused_out = ks->n_refused;
  if (window_bits_out) *window_bits_out = ks->w;
  if (table_bytes_out) *table_bytes_out = (uint64_t)ks->n_keys * ks->key_words * 4;
  return 0;
}

// one key's table, as built (test hook)
int ecdsa_keyset_table_impl(bftkv_gpu_ctx* c, int keyset, uint32_t key, uint32_t* words_out, uint64_t cap_words) {
  if (!c || !words_out) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  const EcKeySet* ks = KeySets<EcKeySet>::find(c, keyset);
  if (!ks || key >= ks->n_keys) return fail(c, BFTKV_E_INVALID, "bad ECDSA key set handle or key index");
  if (cap_words < ks->key_words) return fail(c, BFTKV_E_NOMEM, "words_out holds less than one table");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(words_out, ks->tab.as<uint32_t>() + (size_t)key * ks->key_words, ks->key_words * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ecdsa_verify_impl over a registered set: the same chain, ending in k_ecv_key_tab.  Nothing is read from host memory but the host
// form's own arrays (N's rows and both tables are resident), so the device form never waits.
int ecdsa_verify_keyset_impl(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs,
                             const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out, bool dev) {
  const bool shape_ok = dlen != 0 && dlen <= 66 && (!n_ops || (digests && sigs));
  return verify_on_keyset<EcKeySet>(c, keyset, n_ops, 1u << 24, valid_out, status_out, dev, shape_ok, [&](const EcKeySet& ks, VerdictOut& vo) -> int {
    const bftkv_gpu_ctx* r = c->root ? c->root : c;
    const int id = ks.curve_id;
    // The root's G table is read here without the root's own lock (a fork holds KtRead, not r->mu).  That is safe because the root
    // never rebuilds it: the window width is fixed when the context is made, ec_fb_table fills ec_fb_tab[id] / ec_fb_w[id] once per
    // curve, and the set's creation did that before any fork could name the set.  So the check below cannot fail today; it is
    // there for the day a context may change its width, which would have to take KtWrite.
    if (r->ec_fb_w[id] != ks.w) return fail(c, BFTKV_E_STATE, "the G table of the key set's width is gone");
    const uint32_t* gtab = r->ec_fb_tab[id].as<uint32_t>();
    ScratchBufs sb(c);
    int rc = 0;
    ec_dispatch(id, ks.curve.data(), [&](auto C) {
      constexpr int L = decltype(C)::kWords;
      rc = ecv_chain<L>(c, sb, vo, C, ks.bits, digests, dlen, sigs, key_idx, ks.n_keys, ks.mod.view(), gtab, ks.w, ks.nwin,
                        [&](const ecf::Curve<L>& cv, dim3 grid, dim3 block, const EcvScratch& t) {
                          hipLaunchKernelGGL(k_ecv_key_tab<L>, grid, block, 0, c->stream, vo.n_ops, t.r, ks.tab.as<uint32_t>(), ks.refused.as<uint8_t>(), t.ki,
                                             ks.n_keys, ks.w, ks.nwin, t.u2, t.pt, t.flag, t.ibad, cv, (uint8_t*)vo.d_valid, (uint8_t*)vo.d_st);
                        });
    });
    return rc;
  });
}

}  // namespace

extern "C" {

int bftkv_gpu_ecdsa_calculate_r(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ri, const uint8_t* vi,
                                const uint8_t* curve, uint32_t bit_size, uint8_t* r_out, uint8_t* status_out) {
  return ecdsa_calculate_r_impl(c, n_ops, k, xs, ri, vi, curve, bit_size, r_out, status_out, false);
}
int bftkv_gpu_ecdsa_calculate_r_dev(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ri, const uint8_t* vi,
                                    const uint8_t* curve, uint32_t bit_size, uint8_t* r_out, uint8_t* status_out) {
  return ecdsa_calculate_r_impl(c, n_ops, k, xs, ri, vi, curve, bit_size, r_out, status_out, true);
}
int bftkv_gpu_ec_scalar_base_mult(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* scalars, uint32_t sbytes, const uint8_t* curve,
                                  uint32_t bit_size, uint8_t* out, uint8_t* status_out) {
  return ec_scalar_base_mult_impl(c, n_ops, scalars, sbytes, curve, bit_size, out, status_out);
}

int bftkv_gpu_ecdsa_verify(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs, const uint32_t* key_idx,
                           uint32_t n_keys, const uint8_t* keys, const uint8_t* curve, uint32_t bit_size, uint8_t* valid_out, uint8_t* status_out) {
  return ecdsa_verify_impl(c, n_ops, digests, dlen, sigs, key_idx, n_keys, keys, curve, bit_size, valid_out, status_out, false);
}
int bftkv_gpu_ecdsa_verify_dev(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs, const uint32_t* key_idx,
                               uint32_t n_keys, const uint8_t* keys, const uint8_t* curve, uint32_t bit_size, uint8_t* valid_out, uint8_t* status_out) {
  return ecdsa_verify_impl(c, n_ops, digests, dlen, sigs, key_idx, n_keys, keys, curve, bit_size, valid_out, status_out, true);
}

int bftkv_gpu_ecdsa_keyset_create(bftkv_gpu_ctx* c, uint32_t n_keys, const uint8_t* keys, const uint8_t* curve, uint32_t bit_size, int* keyset_out) {
  return ecdsa_keyset_create_impl(c, n_keys, keys, curve, bit_size, keyset_out);
}
int bftkv_gpu_ecdsa_keyset_destroy(bftkv_gpu_ctx* c, int keyset) { return ecdsa_keyset_destroy_impl(c, keyset); }
int bftkv_gpu_ecdsa_keyset_info(bftkv_gpu_ctx* c, int keyset, uint32_t* n_keys_out, uint32_t* n_refused_out, uint32_t* window_bits_out,
                                uint64_t* table_bytes_out) {
  return ecdsa_keyset_info_impl(c, keyset, n_keys_out, n_refused_out, window_bits_out, table_bytes_out);
}
int bftkv_gpu_ecdsa_verify_keyset(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs,
                                  const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out) {
  return ecdsa_verify_keyset_impl(c, keyset, n_ops, digests, dlen, sigs, key_idx, valid_out, status_out, false);
}
int bftkv_gpu_ecdsa_verify_keyset_dev(bftkv_gpu_ctx* c, int keyset, uint32_t n_ops, const uint8_t* digests, uint32_t dlen, const uint8_t* sigs,
                                      const uint32_t* key_idx, uint8_t* valid_out, uint8_t* status_out) {
  return ecdsa_verify_keyset_impl(c, keyset, n_ops, digests, dlen, sigs, key_idx, valid_out, status_out, true);
}
int bftkv_gpu_selftest_ecdsa_keyset_table(bftkv_gpu_ctx* c, int keyset, uint32_t key, uint32_t* words_out, uint64_t cap_words) {
  return ecdsa_keyset_table_impl(c, keyset, key, words_out, cap_words);
}

}  // extern "C"
