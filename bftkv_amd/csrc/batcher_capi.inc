// Micro-batcher (include/bftkv_gpu.h): aggregates concurrent one-message calls into device batches.
//
// Shape (round 3): no worker thread.  The first caller into an empty batch is its LEADER: it waits for a free LANE (a forked
// verifier context, bftkv_gpu_ctx_fork: own streams and arena over the root's resident key table), closes the batch, runs
// the device call on its own thread and wakes the batch's other callers, who slept on the batch's futex word.  A lone call
// therefore crosses no thread at all, and with L lanes L batches are on the device at once -- the head and tail of one
// call (walk, parse, tally: latency) overlap the others' modular exponentiations.  Callers absorb the whole 64-byte blocks
// of their own payload into a SHA-256 midstate before they queue (host_sha256.h): a payload's hash is one chain, ~0.43 ms on a
// GPU lane whatever the batch size, ~7 us on a host core with the SHA extensions, and the callers hash in parallel.

// grow-only pinned host buffer: batches are assembled straight into page-locked memory, so the copy to the device is one DMA
// transfer instead of the runtime's staged copy out of pageable memory
struct PinnedBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
  bool ensure(size_t n) {
    if (n <= cap) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const size_t want = n + n / 2 + 4096;
    if (hipHostMalloc((void**)&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; }
    cap = want;
    return true;
  }
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
};

void release_small_pin(bftkv_gpu_ctx* c) {
  if (c->small_pin) delete[] (PinnedBuf*)c->small_pin;
  c->small_pin = nullptr;
}

namespace {

// One staged call: everything the device needs sits in ONE pinned buffer and crosses PCIe in one copy.
//   [ midstates n x 8 u32 | prefix n u64 | tail offsets n+1 u64 | signature offsets n+1 u64 | entity indices n u32 |
//     payload tails (< 64 B each) | signature streams ]
struct StagedCall {
  bool collective = true;    // CollectiveSignature.Verify; false: Signature.Verify / VerifyWithCertificate
  int quorum = -1;
  uint32_t n = 0;
  bool has_cert = false;
  size_t off_mid = 0, off_prefix = 0, off_toff = 0, off_soff = 0, off_cert = 0, off_tails = 0, off_ss = 0, bytes = 0;
  uint64_t ss_len = 0;
  void layout(uint32_t n_, uint64_t tails_len, uint64_t ss_len_) {
    n = n_; ss_len = ss_len_;
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    off_mid = 0;
    off_prefix = off_mid + (size_t)n * 32;
    off_toff = off_prefix + (size_t)n * 8;
    off_soff = off_toff + ((size_t)n + 1) * 8;
    off_cert = off_soff + ((size_t)n + 1) * 8;
    off_tails = up8(off_cert + (size_t)n * 4);
    off_ss = up8(off_tails + tails_len);
    bytes = up8(off_ss + ss_len_);
  }
};

// err_out[i]: the call's error byte; flags_out[i]: bit 0 fenced, bit 1 "a signature of this item asks for a hash other than
// SHA-256: submit it again with its payload".
// cert_ref (optional, with cert_key_id): item i names its entity by the certificate GROUP the root's register of valid request
// certificates gave for its bytes (cert_ref[i].first >= 0; .second = the epoch of that answer) instead of by key id -- turned into
// an entity index here, under the fork's hold on the key table (kt_group_ent / kt_cert_epoch change only under KtWrite: no lock);
// unresolved[i] = 1 when the groups have been renumbered since (the caller takes the compound path on the root).
int staged_verify(bftkv_gpu_ctx* c, const StagedCall& L, uint8_t* pin, const uint64_t* cert_key_id, uint8_t* err_out, uint8_t* flags_out,
                  uint64_t* ns_launch = nullptr, uint64_t* ns_spin = nullptr, uint64_t* n_timeouts = nullptr,
                  const std::pair<int, uint64_t>* cert_ref = nullptr, uint8_t* unresolved = nullptr) {
  const auto t_in = std::chrono::steady_clock::now();
  ctx_lock lk(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->h_mail) return fail(c, BFTKV_E_DEVICE, "no mapped mailbox for staged calls");
  const uint32_t n = L.n;
  if (c->out_cap < 2 * (size_t)n + 8) {
    if (c->h_out) { (void)hipHostFree(c->h_out); c->h_out = nullptr; c->d_out = nullptr; c->out_cap = 0; }
    const size_t want = 2 * (size_t)n + 4096;
    HIPCHK(c, hipHostMalloc((void**)&c->h_out, want, hipHostMallocMapped));
    HIPCHK(c, hipHostGetDevicePointer((void**)&c->d_out, c->h_out, 0));
    c->out_cap = want;
  }
  if (L.has_cert) {
    // VerifyWithCertificate: the keyring of item i is the entity whose primary key id is cert_key_id[i]
    uint32_t* ce = (uint32_t*)(pin + L.off_cert);
    bftkv_gpu_ctx* const reg = c->root ? c->root : c;      // (kt_group_ent / kt_cert_epoch: stable under KtRead, see bftkv_gpu_ctx)
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t e = 0xFFFFFFFEu;   // an entity that is not in the table: nothing matches
      if (cert_ref && cert_ref[i].first >= 0) {
        if (cert_ref[i].second == reg->kt_cert_epoch && (size_t)cert_ref[i].first < reg->kt_group_ent.size())
          e = reg->kt_group_ent[(size_t)cert_ref[i].first];
        if (e == 0xFFFFFFFEu && unresolved) unresolved[i] = 1;
      } else {
        for (uint32_t k = 0; k < c->n_entities; ++k) if (c->h_entity_id[k] == cert_key_id[i]) { e = k; break; }
      }
      ce[i] = e;
    }
  }
  HIPCHK(c, c->in_pack.ensure(L.bytes + 64));
  HIPCHK(c, hipMemcpyAsync(c->in_pack.p, pin, L.bytes, hipMemcpyHostToDevice, c->stream));
  const uint8_t* d = c->in_pack.as<uint8_t>();
  const uint32_t* d_mid = (const uint32_t*)(d + L.off_mid);
  const uint64_t* d_prefix = (const uint64_t*)(d + L.off_prefix);
  const uint64_t* d_toff = (const uint64_t*)(d + L.off_toff);
  const uint64_t* d_soff = (const uint64_t*)(d + L.off_soff);
  const uint32_t* d_cert = L.has_cert ? (const uint32_t*)(d + L.off_cert) : nullptr;
  const uint8_t* d_tails = d + L.off_tails;
  const uint8_t* d_ss = d + L.off_ss;
  int rc;
  const uint8_t* res;
  uint32_t from_verdict;
  PipelineCall call;      // tails and midstates instead of payloads, sized up front
  call.n_items = n; call.d_tbs = d_tails; call.d_tbs_off = d_toff; call.d_ss = d_ss; call.d_ss_off = d_soff; call.ss_len = L.ss_len;
  call.d_mid_in = d_mid; call.d_tbs_prefix = d_prefix;
  // Arena and grids for `cap` packet events, no host round trip in mid-pipeline (run_pipeline, staged_cap).  A signature
  // packet of the path's writers is 100 (DSA) to 540 (RSA-4096) bytes; one event per 16 stream bytes leaves room for streams
  // of junk packets, and a call beyond it comes back marked for the ordinary path.
  call.staged_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(4096, L.ss_len / 16 + 64 * (uint64_t)n), 1u << 26);
  // Every packet of every item is verified (no two-phase planning): err and n_verified are the reference's either way, a
  // small call is bound by its chain of launches, not by the 20 % of modexps the planning saves, and it is seven launches
  // shorter.
  if (L.collective) {
    if ((rc = check_quorum(c, L.quorum))) return rc;
    QuorumHost& q = c->quorums[L.quorum];
    if ((rc = build_member(c, q))) return rc;
    const QuorumDev qd = quorum_dev(c, q);
    if ((rc = run_pipeline(c, call))) return rc;
    HIPCHK(c, c->o_nver.ensure(sizeof(uint32_t) * n));
    HIPCHK(c, c->o_verdict.ensure(n));
    hipLaunchKernelGGL(k_tally, dim3((n + 3) / 4), dim3(256), 0, c->stream, c->recs.as<SigRec>(), c->base.as<uint32_t>(), c->counts.as<uint32_t>(), n,
                       c->kt, qd, c->o_verdict.as<uint8_t>(), c->o_nver.as<uint32_t>(), (uint32_t*)nullptr);
    res = c->o_verdict.as<uint8_t>();
    from_verdict = 1;
  } else {
    call.d_cert_ent = d_cert;
    if ((rc = run_pipeline(c, call))) return rc;
    HIPCHK(c, c->o_err.ensure(n));
    hipLaunchKernelGGL(k_sigverify_fold, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->recs.as<SigRec>(), c->base.as<uint32_t>(),
                       c->counts.as<uint32_t>(), c->item_flags.as<uint8_t>(), n, c->o_err.as<uint8_t>());
    res = c->o_err.as<uint8_t>();
    from_verdict = 0;
  }
  if (++c->out_seq == 0) ++c->out_seq;
  const uint32_t seq = c->out_seq;
  hipLaunchKernelGGL(k_finish_staged, dim3(1), dim3(256), 0, c->stream, res, from_verdict, c->item_flags.as<uint8_t>(), c->hash_mask.as<uint32_t>(), n,
                     ITEM_NEEDS_PAYLOAD, c->d_out, c->d_mail + 1, seq, c->total.as<uint32_t>());
  c->have_timing = false;       // (staged calls record no events)
  HIPCHK(c, hipGetLastError());
  // the results arrive in mapped host memory ahead of the sequence number: spin (a call lasts ~0.1 ms), then fall back
  bool got = false;
  const auto t_spin = std::chrono::steady_clock::now();
  if (ns_launch) *ns_launch += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t_spin - t_in).count();
  for (uint32_t it = 0;; ++it) {
    if (__atomic_load_n(&c->h_mail[1], __ATOMIC_ACQUIRE) == seq) { got = true; break; }
    if ((it & 255u) == 255u && std::chrono::steady_clock::now() - t_spin > std::chrono::microseconds(c->staged_spin_us)) break;
    __builtin_ia32_pause();
  }
  if (ns_spin) *ns_spin += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_spin).count();
  if (!got) {
    if (n_timeouts) ++*n_timeouts;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (__atomic_load_n(&c->h_mail[1], __ATOMIC_ACQUIRE) != seq) return fail(c, BFTKV_E_DEVICE, "staged call finished without publishing its results");
  }
  memcpy(err_out, c->h_out, n);
  memcpy(flags_out, c->h_out + n, n);
  uint32_t tot[2];
  memcpy(tot, c->h_out + 2 * (size_t)n, 8);
  if (tot[1]) for (uint32_t i = 0; i < n; ++i) flags_out[i] |= 2;      // more packet events than the staged arena holds: the ordinary path
  if (L.has_cert) {     // an entity the table does not hold: fenced, never a verdict (bftkv_gpu_signature_verify)
    const uint32_t* ce = (const uint32_t*)(pin + L.off_cert);
    for (uint32_t i = 0; i < n; ++i) if (ce[i] == 0xFFFFFFFEu) flags_out[i] |= 1;
  }
  return 0;
}


// One item of a staged group: the caller's buffers and the SHA-256 state after the whole blocks of tbs.
// cert_group / cert_epoch (optional, group >= 0): the entity is the one registered for a request certificate (staged_verify's
// cert_ref) instead of the one cert_key_id names
struct StagedItem {
  const uint8_t* tbs; uint64_t tbs_len; const uint8_t* sig; uint64_t sig_len; uint64_t cert_key_id; const uint32_t* mid;
  int cert_group = -1; uint64_t cert_epoch = 0;
};

// Assembles a group in `pin` and runs it (staged_verify); the items whose signatures ask for a hash other than SHA-256, or a
// whole call with more packet events than the staged arena holds, go through the ordinary entry points with their payloads.
// err / fenced: per item.  device_calls counts what was launched.
int staged_group(bftkv_gpu_ctx* c, PinnedBuf& pin, PinnedBuf& pin_tb, PinnedBuf& pin_sb, bool collective, int quorum, bool has_cert,
                 const std::vector<StagedItem>& g, uint8_t* err, uint8_t* fenced, uint8_t failing, uint64_t* device_calls,
                 uint64_t* ns_assemble = nullptr, uint64_t* ns_device = nullptr, uint64_t* ns_launch = nullptr, uint64_t* ns_spin = nullptr,
                 uint64_t* n_timeouts = nullptr, uint8_t* unresolved = nullptr) {
  auto now_ns = [] { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const uint32_t n = (uint32_t)g.size();
  uint64_t tails = 0, sl = 0;
  for (const StagedItem& r : g) { tails += r.tbs_len & 63; sl += r.sig_len; }
  StagedCall L;
  L.collective = collective; L.quorum = quorum; L.has_cert = has_cert;
  L.layout(n, tails, sl);
  std::vector<uint8_t> flags(n, 0);
  std::vector<uint64_t> certs(n, 0);
  std::vector<std::pair<int, uint64_t>> cert_ref;
  for (const StagedItem& r : g) if (r.cert_group >= 0) { cert_ref.resize(n, {-1, 0}); break; }
  std::vector<uint8_t> unres(cert_ref.empty() ? 0 : n, 0);
  for (uint32_t k = 0; k < n; ++k) { err[k] = failing; fenced[k] = 0; }
  const uint64_t t_a = now_ns();
  if (!pin.ensure(L.bytes + 8)) return BFTKV_E_NOMEM;
  uint8_t* p = pin.p;
  uint64_t* toff = (uint64_t*)(p + L.off_toff);
  uint64_t* soff = (uint64_t*)(p + L.off_soff);
  uint64_t to = 0, so = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const StagedItem& r = g[k];
    memcpy(p + L.off_mid + (size_t)k * 32, r.mid, 32);
    const uint64_t tail = r.tbs_len & 63, pre = r.tbs_len - tail;
    ((uint64_t*)(p + L.off_prefix))[k] = pre;
    toff[k] = to; soff[k] = so;
    if (tail) memcpy(p + L.off_tails + to, r.tbs + pre, tail);
    if (r.sig_len) memcpy(p + L.off_ss + so, r.sig, r.sig_len);
    to += tail; so += r.sig_len;
    certs[k] = r.cert_key_id;
    if (r.cert_group >= 0) cert_ref[k] = {r.cert_group, r.cert_epoch};
  }
  toff[n] = to; soff[n] = so;
  const uint64_t t_d = now_ns();
  if (ns_assemble) *ns_assemble += t_d - t_a;
  int rc = staged_verify(c, L, p, has_cert ? certs.data() : nullptr, err, flags.data(), ns_launch, ns_spin, n_timeouts,
                         cert_ref.empty() ? nullptr : cert_ref.data(), cert_ref.empty() ? nullptr : unres.data());
  if (ns_device) *ns_device += now_ns() - t_d;
  ++*device_calls;
  if (rc) { for (uint32_t k = 0; k < n; ++k) err[k] = failing; return rc; }
  std::vector<uint32_t> again;
  for (uint32_t k = 0; k < n; ++k) {
    if (!cert_ref.empty() && cert_ref[k].first >= 0) {
      // an entity named by its certificate's group: whatever is not a plain verdict (groups renumbered since, a fenced shape -- a DSA
      // certificate key whose table slot was recycled --, another hash, an overflowing call) is left to the compound path
      if (unres[k] || flags[k]) { err[k] = failing; fenced[k] = 0; if (unresolved) unresolved[k] = 1; }
      continue;
    }
    fenced[k] = flags[k] & 1;
    if (flags[k] & 2) again.push_back(k);
  }
  if (again.empty()) return 0;
  // another hash than SHA-256 (or an overflowing call): the device needs the payloads themselves
  std::vector<uint64_t> to2{0}, so2{0}, c2;
  for (uint32_t k : again) { to2.push_back(to2.back() + g[k].tbs_len); so2.push_back(so2.back() + g[k].sig_len); c2.push_back(g[k].cert_key_id); }
  const uint32_t m = (uint32_t)again.size();
  std::vector<uint8_t> e2(m, failing), f2(m, 0);
  int rc2 = 0;
  if (!pin_tb.ensure(to2.back() + 1) || !pin_sb.ensure(so2.back() + 1)) rc2 = BFTKV_E_NOMEM;
  if (!rc2) {
    for (uint32_t j = 0; j < m; ++j) {
      const StagedItem& r = g[again[j]];
      if (r.tbs_len) memcpy(pin_tb.p + to2[j], r.tbs, r.tbs_len);
      if (r.sig_len) memcpy(pin_sb.p + so2[j], r.sig, r.sig_len);
    }
    if (collective)
      rc2 = bftkv_gpu_collective_verify(c, quorum, m, pin_tb.p, to2.data(), pin_sb.p, so2.data(), e2.data(), nullptr, nullptr, f2.data());
    else
      rc2 = bftkv_gpu_signature_verify(c, m, pin_tb.p, to2.data(), pin_sb.p, so2.data(), has_cert ? c2.data() : nullptr, e2.data(), f2.data());
  }
  ++*device_calls;
  for (uint32_t j = 0; j < m; ++j) { err[again[j]] = rc2 ? failing : e2[j]; fenced[again[j]] = rc2 ? 0 : f2[j]; }
  return rc2;
}

}  // namespace

// A batch's callers sleep on ONE futex word of their batch and are woken by one syscall, each returning with the results
// already in its own request: no shared mutex on the way out.  (One condition variable for every caller of the batcher made
// 256 threads wake for every batch, whoever's it was, and queue on the batcher's mutex just to go back to sleep: batches of
// 33 instead of 256 and 2.3 ms median latency at 256 caller threads.)
inline void batch_futex_wait(std::atomic<uint32_t>* w, uint32_t expect) {
  (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), FUTEX_WAIT_PRIVATE, expect, nullptr, nullptr, 0);
}
inline void batch_futex_wake_all(std::atomic<uint32_t>* w) {
  (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}

struct bftkv_gpu_batcher {
  // What a request asks for.  Requests of one batch that agree in (kind, quorum, has_cert, th_shape) share a device call (process).
  enum class Kind {
    Collective, Signature, Message, Cert,                      // CollectiveSignature.Verify, Signature.Verify, a transport message, Issuer + VerifyWithCertificate
    ModmulProduct, LagrangeCombine, DsaCalculateR, Modexp,     // ONE share-combine operation: prod psig mod N, sum l_j y_j mod m, CalculateR, b^x mod n
    EcdsaCalculateR, EcdsaVerify, EcdsaVerifyKeyset, DsaVerify, DsaVerifyKeyset, RsaVerify, RsaVerifyKeyset,
    TpaYi, TpaBi,                                              // ONE password-authentication answer of a server: makeYi, makeBi (crypto/auth)
    RsaPartialSign,                                            // ONE threshold-RSA sign request of a server with all its fragments: rsaContext.Sign
    TdsaShare, TecdsaShare,                                    // ONE threshold DSA / ECDSA sign request of a server with its m shares: dsaContext.Sign, phase 2
    RsaSignKeyset                                              // ONE raw RSA signature under a resident signer set: rsa.SignPKCS1v15
  };
  static bool hashed_by_caller(Kind k) { return k == Kind::Collective || k == Kind::Signature; }      // a SHA-256 midstate of tbs goes to the device, not tbs
  static bool threshold_style(Kind k) { return k >= Kind::ModmulProduct; }      // th_* fields in, a BFTKV_TH_* status byte and th_out out
  static constexpr int NO_QUORUM = -1;       // Req::quorum of the kinds that name neither a quorum nor a key set

  // The fields by kind (f = the curve's field bytes, pb / qb = the bytes of p / q, dlen = the digest's length, curve = P|N|B|Gx|Gy, verdict = one
  // byte, th_out otherwise that many output bytes; in a key-set kind f / qb are the set's; "-": unused):
  //   kind                      quorum  th_k  th_nbytes  th_qbytes  th_xs  th_a            th_b        th_mod  th_mod2        th_g, th_y  ks_key  th_out
  //   Collective                quorum  -     -          -          -      -               -           -       -              -           -       -
  //   Signature, Message, Cert  -       -     -          -          -      -               -           -       -              -           -       -
  //   ModmulProduct             -       k     nbytes     0          -      k factors       -           N       -              -           -       nbytes
  //   LagrangeCombine           -       k     nbytes     0          k x_j  k y_j           -           m       -              -           -       nbytes
  //   DsaCalculateR             -       k     pb         qb         k x_j  k Ri (pb)       k Vi (qb)   p       q              -           -       qb
  //   Modexp                    -       1     nbytes     exp bytes  -      base            exponent    n       -              -           -       nbytes
  //   EcdsaCalculateR           -       k     f          bit size   k x_j  k Ri (1 + 2 f)  k Vi (f)    curve   -              -           -       f
  //   EcdsaVerify               -       dlen  f          bit size   -      digest          r|s (2 f)   curve   key (1 + 2 f)  -           -       verdict
  //   EcdsaVerifyKeyset         set     dlen  -          -          -      digest          r|s (2 f)   -       -              -           key     verdict
  //   DsaVerify                 -       dlen  pb         qb         -      digest          r|s (2 qb)  p       q              g, y (pb)   -       verdict
  //   DsaVerifyKeyset           set     dlen  -          -          -      digest          r|s (2 qb)  -       -              -           key     verdict
  //   RsaVerify                 -       dlen  nbytes     hash id    -      digest          s (nbytes)  n       -              -           e       verdict
  //   RsaVerifyKeyset           set     dlen  -          hash id    -      digest          s (nbytes)  -       -              -           key     verdict
  //   TpaYi                     -       -     nbytes     exp bytes  -      x               y           p       -              -           -       nbytes
  //   TpaBi                     -       salt  nbytes     exp bytes  -      v               b           p       -              Xi, salt    Xi len  nbytes
  //   RsaPartialSign            -       frags nbytes     exp bytes  -      T               magnitudes  N       -              -           T len   frags x nbytes
  //   TdsaShare                 set     m     pb         qb         -      m shares (4 qb) -           -       -              -           group   1 x pb
  //   TecdsaShare               -       m     f          bit size   -      m shares (4 f)  -           curve   -              -           -       1 x (1 + 2 f)
  //   RsaSignKeyset             set     dlen  -          hash id    -      digest          -           -       -              -           key     nbytes of the set
  // (TpaBi: th_k is the salt's length; its keys and MAC, 32 bytes each, go to tpa_keys and tpa_mac.)
  // (RsaPartialSign: th_k is the request's fragment count; ps_used and ps_sign are its widths and sign bytes, ps_status its status bytes.)
  // (TdsaShare, TecdsaShare: th_out is ri; vi, ki and ci go to ts_vi, ts_ki and ts_ci, qb or f bytes each.  TdsaShare's pb and qb are the
  // caller's word for the set's widths: a group whose word the set does not bear out is refused.)
  // An EcdsaCalculateR or EcdsaVerify group shares one recognised curve, which the device call takes by value: its bit size is part of
  // the shape.  A key-set group shares the set: the lane is a fork and passes the handle through.
  struct Req {
    Kind kind;
    int quorum;
    const uint8_t* tbs; uint64_t tbs_len;
    const uint8_t* sig; uint64_t sig_len;
    bool has_cert; uint64_t cert_key_id;
    // Results start out as FAILURES: a caller that looks at the status byte and not at the return code (or a group whose
    // device call failed) must never read "verified".
    uint8_t err = BFTKV_ERR_INVALID_SIGNATURE; int rc = BFTKV_E_STATE;
    uint8_t fenced = 0;
    static uint8_t failing(Kind k) {
      if (threshold_style(k)) return BFTKV_TH_FAILED;
      return k == Kind::Collective ? BFTKV_ERR_INSUFFICIENT_SIGNATURES : k == Kind::Message ? BFTKV_MSG_READ_ERROR : BFTKV_ERR_INVALID_SIGNATURE;
    }
    // requests of one SHAPE (kind, k or dlen, widths) share a device call, whatever their moduli, groups and keys
    static uint64_t shape(Kind k, uint64_t a, uint64_t b = 0, uint64_t c = 0) { return (uint64_t)k | a << 8 | b << 24 | c << 40; }
    // Cert
    const uint8_t* cert = nullptr; uint64_t cert_len = 0, issuer_id = 0;
    // Signature on behalf of bftkv_gpu_batcher_cert_verify: the entity is the one registered for a certificate the root has accepted
    // before (its group and the epoch of that answer); unresolved = 1: no verdict from this route, ask the compound one (Cert)
    int cert_group = -1; uint64_t cert_epoch = 0; uint8_t unresolved = 0;
    // Message results
    uint8_t* plain_out = nullptr; uint64_t plain_cap = 0, plain_len = 0, signer = 0, peer = 0;
    uint8_t* fname_out = nullptr; uint8_t fname_len = 0;
    // hashed_by_caller: SHA-256 state after the whole blocks of tbs, absorbed by the caller's own thread in submit()
    uint32_t mid[8] = {};
    // threshold_style (the table above)
    uint64_t th_shape = 0;
    uint32_t th_k = 0, th_nbytes = 0, th_qbytes = 0;
    const int32_t* th_xs = nullptr;
    const uint8_t *th_a = nullptr, *th_b = nullptr, *th_mod = nullptr, *th_mod2 = nullptr;
    uint8_t* th_out = nullptr;
    uint32_t ks_key = 0;       // the key's index within the set (RsaVerify: the public exponent)
    const uint8_t *th_g = nullptr, *th_y = nullptr;
    uint8_t *tpa_keys = nullptr, *tpa_mac = nullptr;
    const uint32_t* ps_used = nullptr; const uint8_t* ps_sign = nullptr; uint8_t* ps_status = nullptr;
    uint8_t *ts_vi = nullptr, *ts_ki = nullptr, *ts_ci = nullptr;
  };
  struct Batch {
    std::vector<Req*> reqs;
    std::atomic<uint32_t> done{0};     // futex word: 0 while the batch is open, waits for a lane or is being processed
  };
  struct Lane {
    bftkv_gpu_ctx* ctx = nullptr;
    std::atomic<bool> busy{false};
    PinnedBuf pin, pin_tb, pin_sb;     // used by whoever holds the lane
  };
  bftkv_gpu_ctx* ctx = nullptr;        // the root
  uint32_t max_items = 0, max_wait_us = 0;
  // Joining a batch is a critical section of a few dozen nanoseconds (append a pointer, maybe start a batch) that every
  // caller passes, hundreds of them within microseconds of one another when a batch of callers is released.  Under a
  // sleeping mutex that moment became a convoy -- each waiter put to sleep and woken in turn: 14 of the box's 16 usable
  // cores in the kernel at 256 callers.  Under a pure spinlock 256 spinning threads burned the container's CPU quota in
  // milliseconds whenever the holder lost its CPU (20 k calls/s).  So: spin for a few microseconds -- long enough for a
  // burst of joiners to pass one after the other -- then sleep on the lock word (the three-state futex lock of Drepper,
  // "Futexes are tricky").  Nothing blocks while holding it: a leader waits for its lane on the futex word lane_seq,
  // followers on their batch's.
  // ... and the door is SHARDED when many callers are inside: 256 callers released together still queued on one lock word for
  // longer than anyone should spin (sys time 13 of 16 cores, 160 k calls/s where 128 callers made 410 k).  A caller joins the
  // shard its thread hashes to, among as many shards as the number of callers inside calls for (one per ~48, at most
  // DOORS); each shard has its own lock and open batch.  Few callers see one door and batches as large as before.
  struct alignas(64) Door {
    std::atomic<uint32_t> lk{0};       // 0 free, 1 held, 2 held and somebody sleeps
    std::shared_ptr<Batch> open;       // the batch still accepting requests (null: none); under the lock
    void lock() {
      uint32_t c = 0;
      for (int it = 0; it < 256; ++it) {
        c = 0;
        if (lk.load(std::memory_order_relaxed) == 0 && lk.compare_exchange_weak(c, 1, std::memory_order_acquire)) return;
        __builtin_ia32_pause();
      }
      if (c != 2) c = lk.exchange(2, std::memory_order_acquire);
      while (c != 0) {
        (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&lk), FUTEX_WAIT_PRIVATE, 2, nullptr, nullptr, 0);
        c = lk.exchange(2, std::memory_order_acquire);
      }
    }
    void unlock() {
      if (lk.fetch_sub(1, std::memory_order_release) != 1) {
        lk.store(0, std::memory_order_release);
        (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&lk), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
      }
    }
  };
  static constexpr int DOORS = 8;
  Door doors[DOORS];
  Door& my_door() {
    static std::atomic<uint32_t> next_thread{0};
    static thread_local uint32_t me = next_thread.fetch_add(1, std::memory_order_relaxed) * 0x9E3779B1u;
    const int in = inside.load(std::memory_order_relaxed);
    const uint32_t n = (uint32_t)std::min(DOORS, std::max(1, in / 48));
    return doors[(me >> 16) % n];
  }
  std::vector<std::unique_ptr<Lane>> lanes;
  std::atomic<uint32_t> lane_seq{0};   // futex word: bumped whenever a lane is released (or the batcher stops)
  std::atomic<bool> stop{false};
  std::atomic<int> inside{0};          // callers between entry and exit of submit(): destroy() waits for them
  std::atomic<uint64_t> n_calls{0}, n_batches{0}, max_batch{0};
  // where the callers' time goes (bftkv_gpu_batcher_times), nanoseconds summed over callers
  std::atomic<uint64_t> ns_hash{0}, ns_lane_wait{0}, ns_assemble{0}, ns_device{0}, ns_launch{0}, ns_spin{0}, n_spin_timeouts{0}, n_cert_fast{0};
  static uint64_t now_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

  Lane* try_lane() {
    for (auto& l : lanes) {
      bool idle = false;
      if (l->busy.compare_exchange_strong(idle, true, std::memory_order_acquire)) return l.get();
    }
    return nullptr;
  }
  void release_lane(Lane* l) {
    l->busy.store(false, std::memory_order_release);
    lane_seq.fetch_add(1, std::memory_order_release);
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&lane_seq), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
  }

  // Collective, Signature: one staged device call per group, midstates instead of payloads; the (rare) items whose signatures ask for
  // another hash go through the ordinary entry point with their bytes afterwards
  void run_group(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Kind kind = g[0]->kind;
    const uint32_t n = (uint32_t)g.size();
    std::vector<StagedItem> items(n);
    for (uint32_t k = 0; k < n; ++k) {
      items[k] = StagedItem{g[k]->tbs, g[k]->tbs_len, g[k]->sig, g[k]->sig_len, g[k]->cert_key_id, g[k]->mid};
      items[k].cert_group = g[k]->cert_group; items[k].cert_epoch = g[k]->cert_epoch;
    }
    std::vector<uint8_t> err(n), fenced(n), unres(n, 0);
    uint64_t a_ns = 0, d_ns = 0, l_ns = 0, s_ns = 0, n_to = 0;
    const int rc = staged_group(lane.ctx, lane.pin, lane.pin_tb, lane.pin_sb, kind == Kind::Collective, g[0]->quorum, g[0]->has_cert, items, err.data(), fenced.data(),
                                Req::failing(kind), &device_calls, &a_ns, &d_ns, &l_ns, &s_ns, &n_to, unres.data());
    ns_assemble.fetch_add(a_ns, std::memory_order_relaxed); ns_device.fetch_add(d_ns, std::memory_order_relaxed);
    ns_launch.fetch_add(l_ns, std::memory_order_relaxed); ns_spin.fetch_add(s_ns, std::memory_order_relaxed);
    n_spin_timeouts.fetch_add(n_to, std::memory_order_relaxed);
    for (uint32_t k = 0; k < n; ++k) {
      g[k]->rc = rc; g[k]->err = rc ? Req::failing(kind) : err[k]; g[k]->fenced = rc ? 0 : fenced[k];
      g[k]->unresolved = rc ? 1 : unres[k];
    }
  }

  void run_messages(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    std::vector<uint64_t> to{0};
    for (Req* r : g) to.push_back(to.back() + r->tbs_len);
    const size_t n = g.size();
    std::vector<uint8_t> err(n, Req::failing(Kind::Message));
    int rc = 0;
    if (!lane.pin_tb.ensure(to.back() + 1)) rc = BFTKV_E_NOMEM;
    std::vector<uint64_t> signer(n), peer(n), poff(n + 1);
    std::vector<uint8_t> plain(to.back() + 1), fn(n * 256), fl(n);
    if (!rc) {
      for (size_t k = 0; k < n; ++k) if (g[k]->tbs_len) memcpy(lane.pin_tb.p + to[k], g[k]->tbs, g[k]->tbs_len);
      rc = bftkv_gpu_message_verify(lane.ctx, (uint32_t)n, lane.pin_tb.p, to.data(), err.data(), signer.data(), peer.data(), plain.data(), plain.size(),
                                    poff.data(), fn.data(), fl.data());
    }
    ++device_calls;
    for (size_t k = 0; k < n; ++k) {
      Req* r = g[k];
      r->rc = rc;
      if (!rc) {
        r->signer = signer[k]; r->peer = peer[k]; r->plain_len = poff[k + 1] - poff[k]; r->fname_len = fl[k];
        if (r->plain_out && r->plain_len <= r->plain_cap) copy_out(r->plain_out, plain.data() + poff[k], r->plain_len);
        else if (r->plain_out) r->rc = BFTKV_E_NOMEM;
        if (r->fname_out) copy_out(r->fname_out, fn.data() + k * 256, fl[k]);
      }
      r->err = rc ? Req::failing(Kind::Message) : err[k];
    }
  }

  // Cert: certificates are registered on the ROOT context (the key table changes; the lanes' calls in flight drain first),
  // ReadEntity verdicts are remembered by certificate bytes, and the signatures of the group are verified in one device call
  void run_certs(std::vector<Req*>& g, uint64_t& device_calls) {
    std::vector<CertSigReq> reqs;
    for (Req* r : g) reqs.push_back(CertSigReq{r->cert, r->cert_len, r->tbs, r->tbs_len, r->sig, r->sig_len});
    std::vector<CertSigRes> res;
    const int rc = cert_signature_core(ctx, reqs, &res);
    ++device_calls;
    for (size_t k = 0; k < g.size(); ++k) {
      Req* r = g[k];
      r->rc = rc;
      r->err = Req::failing(Kind::Cert); r->fenced = 0;
      if (rc) continue;
      r->issuer_id = res[k].issuer_id;
      if (res[k].err == BFTKV_HOST_ERR_FENCED) r->fenced = 1;     // (the status byte stays a failure)
      else r->err = res[k].err;
    }
  }

  // one field of every request of a group, w bytes each, as one array
  static std::vector<uint8_t> gather(const std::vector<Req*>& g, const uint8_t* Req::*field, size_t w) {
    std::vector<uint8_t> v(g.size() * w);
    if (w) for (size_t i = 0; i < g.size(); ++i) memcpy(&v[i * w], g[i]->*field, w);
    return v;
  }

  // One publish path per result shape.
  // status + verdict byte (the four verify kinds)
  static void publish_verdicts(std::vector<Req*>& g, int rc, const uint8_t* st, const uint8_t* valid) {
    for (size_t i = 0; i < g.size(); ++i) {
      Req* r = g[i];
      r->rc = rc;
      r->err = rc ? Req::failing(r->kind) : st[i];
      *r->th_out = !rc && st[i] == BFTKV_TH_OK ? valid[i] : 0;
    }
  }
  // status + o_w output bytes (the combines and both CalculateR); a failed operation leaves the caller's zeroes
  static void publish_outputs(std::vector<Req*>& g, int rc, const uint8_t* st, const uint8_t* out, size_t o_w) {
    for (size_t i = 0; i < g.size(); ++i) {
      Req* r = g[i];
      r->rc = rc;
      r->err = rc ? Req::failing(r->kind) : st[i];
      if (!rc && st[i] == 0) memcpy(r->th_out, out + i * o_w, o_w);
    }
  }

  // EcdsaCalculateR
  void run_ecdsa(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const uint32_t n = (uint32_t)g.size(), k = r0.th_k, f = r0.th_nbytes;
    const std::vector<uint8_t> ri = gather(g, &Req::th_a, (size_t)k * (1 + 2 * f)), vi = gather(g, &Req::th_b, (size_t)k * f);
    std::vector<uint8_t> out((size_t)n * f), st((size_t)n + 8, BFTKV_TH_FAILED);
    std::vector<int32_t> xs((size_t)n * k);
    for (uint32_t i = 0; i < n; ++i) memcpy(&xs[(size_t)i * k], g[i]->th_xs, (size_t)k * 4);
    const int rc = ecdsa_calculate_r_impl(lane.ctx, n, k, xs.data(), ri.data(), vi.data(), r0.th_mod, r0.th_qbytes, out.data(), st.data(), false);
    ++device_calls;
    publish_outputs(g, rc, st.data(), out.data(), f);
  }

  // EcdsaVerify: the distinct keys of the group make the call's key table, in first-seen order.
  void run_ecdsa_verify(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const uint32_t n = (uint32_t)g.size(), dlen = r0.th_k, f = r0.th_nbytes;
    const size_t kw = 1 + 2 * (size_t)f;
    std::map<std::string, uint32_t> slot;
    const std::vector<uint8_t> dg = gather(g, &Req::th_a, dlen), sg = gather(g, &Req::th_b, 2 * (size_t)f);
    std::vector<uint8_t> keys, valid(n, 0), st((size_t)n + 8, BFTKV_TH_FAILED);
    std::vector<uint32_t> idx(n);
    for (uint32_t i = 0; i < n; ++i) {
      auto ins = slot.emplace(std::string((const char*)g[i]->th_mod2, kw), (uint32_t)slot.size());
      if (ins.second) keys.insert(keys.end(), g[i]->th_mod2, g[i]->th_mod2 + kw);
      idx[i] = ins.first->second;
    }
    const int rc = ecdsa_verify_impl(lane.ctx, n, dg.data(), dlen, sg.data(), idx.data(), (uint32_t)slot.size(), keys.data(), r0.th_mod, r0.th_qbytes,
                                     valid.data(), st.data(), false);
    ++device_calls;
    publish_verdicts(g, rc, st.data(), valid.data());
  }

  // EcdsaVerifyKeyset, DsaVerifyKeyset, RsaVerifyKeyset.  Set: the kind's key set, which tells the bytes of one signature under it;
  // verify: the kind's batched impl.  The lane holds its hold on the root's tables from the look at the set to the end of the device
  // call, so the set cannot be replaced by one of another signature length in between.  The signature bytes of every caller are
  // copied with the length taken from the set found NOW: a caller that retired the set while this request waited, and let a wider set
  // take the handle, has broken the rule in include/bftkv_gpu.h (no destroy while calls naming the set are in flight) and the copy
  // reads past its buffer.
  template <typename Set, typename Verify>
  void run_verify_keyset(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls, Verify verify) {
    const Req& r0 = *g[0];
    const uint32_t n = (uint32_t)g.size(), dlen = r0.th_k;
    std::vector<uint8_t> valid(n, 0), st((size_t)n + 8, BFTKV_TH_FAILED);
    int rc;
    {
      ctx_lock lk(lane.ctx->mu);
      KtRead kr(lane.ctx);
      const Set* ks = kr.rc ? nullptr : KeySets<Set>::find(lane.ctx, r0.quorum);
      const size_t sw = ks ? ks->sig_bytes() : 0;
      if (kr.rc) rc = kr.rc;
      else if (!sw) rc = BFTKV_E_INVALID;
      else {
        const std::vector<uint8_t> dg = gather(g, &Req::th_a, dlen), sg = gather(g, &Req::th_b, sw);
        std::vector<uint32_t> idx(n);
        for (uint32_t i = 0; i < n; ++i) idx[i] = g[i]->ks_key;
        rc = verify(lane.ctx, r0.quorum, n, dg.data(), dlen, sg.data(), idx.data(), valid.data(), st.data(), false);
        ++device_calls;
      }
    }
    publish_verdicts(g, rc, st.data(), valid.data());
  }

  // RsaVerify: a group's callers share (nbytes, hash id, dlen), whatever their keys.  The distinct (n, e) of the group make the call's
  // key table in first-seen order; a recurring modulus finds its rows in the context's cache by value.
  void run_rsa_verify(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const uint32_t n = (uint32_t)g.size(), dlen = r0.th_k, nb = r0.th_nbytes, hash_id = r0.th_qbytes;
    std::map<std::string, uint32_t> slot;
    const std::vector<uint8_t> dg = gather(g, &Req::th_a, dlen), sg = gather(g, &Req::th_b, nb);
    std::vector<uint8_t> keys_n, valid(n, 0), st((size_t)n + 8, BFTKV_TH_FAILED);
    std::vector<uint32_t> idx(n), keys_e;
    for (uint32_t i = 0; i < n; ++i) {
      std::string kk((const char*)g[i]->th_mod, nb);
      kk.append((const char*)&g[i]->ks_key, 4);
      auto ins = slot.emplace(std::move(kk), (uint32_t)slot.size());
      if (ins.second) { keys_n.insert(keys_n.end(), g[i]->th_mod, g[i]->th_mod + nb); keys_e.push_back(g[i]->ks_key); }
      idx[i] = ins.first->second;
    }
    const int rc = rsa_verify_impl(lane.ctx, n, dg.data(), hash_id, dlen, sg.data(), nb, idx.data(), (uint32_t)slot.size(), keys_n.data(), keys_e.data(),
                                   valid.data(), st.data(), false);
    ++device_calls;
    publish_verdicts(g, rc, st.data(), valid.data());
  }

  // DsaVerify: a group's callers share the widths and the digest length, whatever their groups and keys.  The distinct (p, q, g) of
  // the batch make the call's group table in BYTE ORDER (the same groups find their Montgomery rows in the context's cache call after
  // call), the distinct (group, y) its key table in first-seen order.
  void run_dsa_verify(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const uint32_t n = (uint32_t)g.size(), dlen = r0.th_k, pb = r0.th_nbytes, qb = r0.th_qbytes;
    auto group_key = [&](const Req* r) {
      std::string k((const char*)r->th_mod, pb);
      k.append((const char*)r->th_mod2, qb);
      k.append((const char*)r->th_g, pb);
      return k;
    };
    std::map<std::string, uint32_t> gslot, kslot;
    for (Req* r : g) gslot.emplace(group_key(r), 0u);
    uint32_t n_groups = 0;
    std::vector<uint8_t> ps((size_t)gslot.size() * pb), qs((size_t)gslot.size() * qb), gs((size_t)gslot.size() * pb), ys;
    for (auto& kv : gslot) {
      kv.second = n_groups;
      memcpy(&ps[(size_t)n_groups * pb], kv.first.data(), pb);
      memcpy(&qs[(size_t)n_groups * qb], kv.first.data() + pb, qb);
      memcpy(&gs[(size_t)n_groups * pb], kv.first.data() + pb + qb, pb);
      ++n_groups;
    }
    const std::vector<uint8_t> dg = gather(g, &Req::th_a, dlen), sg = gather(g, &Req::th_b, 2 * (size_t)qb);
    std::vector<uint8_t> valid(n, 0), st((size_t)n + 8, BFTKV_TH_FAILED);
    std::vector<uint32_t> idx(n), kgrp;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t gi = gslot[group_key(g[i])];
      std::string kk((const char*)&gi, 4);
      kk.append((const char*)g[i]->th_y, pb);
      auto ins = kslot.emplace(std::move(kk), (uint32_t)kslot.size());
      if (ins.second) { ys.insert(ys.end(), g[i]->th_y, g[i]->th_y + pb); kgrp.push_back(gi); }
      idx[i] = ins.first->second;
    }
    const int rc = dsa_verify_impl(lane.ctx, n, dg.data(), dlen, sg.data(), qb, idx.data(), (uint32_t)kslot.size(), ys.data(), kgrp.data(), pb, n_groups,
                                   ps.data(), qs.data(), gs.data(), valid.data(), st.data(), false);
    ++device_calls;
    publish_verdicts(g, rc, st.data(), valid.data());
  }

  // ModmulProduct, LagrangeCombine, DsaCalculateR, Modexp: the group's operations in ONE call of the batched entry point on the
  // lane's context (threshold_capi.inc).  The distinct moduli of the group go into the call's modulus table in BYTE ORDER, so that the
  // same set of moduli -- a protocol instance combines under the same few CA keys call after call -- finds its Montgomery tables in
  // the context's cache.
  void run_threshold(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const Kind kind = r0.kind;
    const bool calc_r = kind == Kind::DsaCalculateR, modexp = kind == Kind::Modexp;
    const uint32_t n = (uint32_t)g.size(), k = r0.th_k, nb = r0.th_nbytes, qb = r0.th_qbytes;
    auto mod_key = [&](const Req* r) {      // (CalculateR: a group (p, q) is one table row)
      std::string key((const char*)r->th_mod, nb);
      if (calc_r) key.append((const char*)r->th_mod2, qb);
      return key;
    };
    std::map<std::string, uint32_t> slot;
    for (Req* r : g) slot.emplace(mod_key(r), 0u);
    uint32_t n_mods = 0;
    std::vector<uint8_t> mods((size_t)slot.size() * nb), mods2(calc_r ? (size_t)slot.size() * qb : 0);
    for (auto& kv : slot) {
      kv.second = n_mods;
      memcpy(&mods[(size_t)n_mods * nb], kv.first.data(), nb);
      if (calc_r) memcpy(&mods2[(size_t)n_mods * qb], kv.first.data() + nb, qb);
      ++n_mods;
    }
    std::vector<uint32_t> idx(n);
    const size_t a_w = (size_t)(modexp ? 1 : k) * nb;                                  // bytes of th_a per operation
    const size_t b_w = calc_r ? (size_t)k * qb : modexp ? (size_t)qb : 0;              // ... of th_b
    const size_t o_w = calc_r ? qb : nb;
    // (modmul_product_impl and modexp_impl write no status: the bytes start at 0 here, not at BFTKV_TH_FAILED)
    const std::vector<uint8_t> a = gather(g, &Req::th_a, a_w), b = gather(g, &Req::th_b, b_w);
    std::vector<uint8_t> out((size_t)n * o_w), st((size_t)n + 8, 0);
    std::vector<int32_t> xs(kind == Kind::LagrangeCombine || calc_r ? (size_t)n * k : 0);
    for (uint32_t i = 0; i < n; ++i) {
      idx[i] = slot[mod_key(g[i])];
      if (!xs.empty()) memcpy(&xs[(size_t)i * k], g[i]->th_xs, (size_t)k * 4);
    }
    int rc;
    switch (kind) {
      case Kind::ModmulProduct: rc = modmul_product_impl(lane.ctx, n, k, a.data(), nb, idx.data(), n_mods, mods.data(), out.data(), false); break;
      case Kind::LagrangeCombine:
        rc = lagrange_combine_impl(lane.ctx, n, k, xs.data(), a.data(), nb, idx.data(), n_mods, mods.data(), out.data(), st.data(), false); break;
      case Kind::DsaCalculateR:
        rc = dsa_calculate_r_impl(lane.ctx, n, k, xs.data(), a.data(), nb, b.data(), qb, idx.data(), n_mods, mods.data(), mods2.data(), out.data(),
                                  st.data(), false); break;
      default: rc = modexp_impl(lane.ctx, n, a.data(), nb, idx.data(), n_mods, mods.data(), b.data(), qb, true, out.data()); break;
    }
    ++device_calls;
    publish_outputs(g, rc, st.data(), out.data(), o_w);
  }

  // TpaYi, TpaBi: a group's callers share (nbytes, exp_len, salt_len), whatever their moduli, which make the call's table in BYTE ORDER
  // as in run_threshold.  A request's Xi and salt are copied at their own lengths into the rows the batched entry takes.
  void run_tpa(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const bool bi = r0.kind == Kind::TpaBi;
    const uint32_t n = (uint32_t)g.size(), nb = r0.th_nbytes, el = r0.th_qbytes, sl = r0.th_k;
    std::map<std::string, uint32_t> slot;
    for (Req* r : g) slot.emplace(std::string((const char*)r->th_mod, nb), 0u);
    uint32_t n_mods = 0;
    std::vector<uint8_t> mods((size_t)slot.size() * nb);
    for (auto& kv : slot) { kv.second = n_mods; memcpy(&mods[(size_t)n_mods * nb], kv.first.data(), nb); ++n_mods; }
    const std::vector<uint8_t> a = gather(g, &Req::th_a, nb), e = gather(g, &Req::th_b, el);
    std::vector<uint8_t> xi(bi ? (size_t)n * nb : 0, 0), salt(bi ? (size_t)n * sl : 0), out((size_t)n * nb), keys((size_t)n * 32), mac((size_t)n * 32),
        st((size_t)n + 8, BFTKV_TH_FAILED);
    std::vector<uint32_t> idx(n), xl(bi ? n : 0);
    for (uint32_t i = 0; i < n; ++i) {
      idx[i] = slot[std::string((const char*)g[i]->th_mod, nb)];
      if (!bi) continue;
      xl[i] = g[i]->ks_key;
      if (xl[i]) memcpy(&xi[(size_t)i * nb], g[i]->th_g, xl[i]);
      if (sl) memcpy(&salt[(size_t)i * sl], g[i]->th_y, sl);
    }
    const int rc = tpa_impl(lane.ctx, bi ? TpaMode::Bi : TpaMode::Yi, n, a.data(), bi ? xi.data() : nullptr, bi ? xl.data() : nullptr, nb, e.data(), el,
                            sl ? salt.data() : nullptr, sl, idx.data(), n_mods, mods.data(), out.data(), bi ? keys.data() : nullptr,
                            bi ? mac.data() : nullptr, st.data());
    ++device_calls;
    publish_outputs(g, rc, st.data(), out.data(), nb);
    if (bi && !rc)
      for (uint32_t i = 0; i < n; ++i)
        if (st[i] == BFTKV_TH_OK) { memcpy(g[i]->tpa_keys, &keys[(size_t)i * 32], 32); memcpy(g[i]->tpa_mac, &mac[(size_t)i * 32], 32); }
  }

  // RsaPartialSign: a group's callers share (nbytes, exp_len), whatever their moduli (the call's table, in BYTE ORDER as in run_threshold),
  // fragment counts and T lengths: every caller is one request of the call, its fragments rows of the call's fragment arrays.
  void run_psign(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const uint32_t n = (uint32_t)g.size(), nb = r0.th_nbytes, el = r0.th_qbytes;
    std::map<std::string, uint32_t> slot;
    for (Req* r : g) slot.emplace(std::string((const char*)r->th_mod, nb), 0u);
    uint32_t n_mods = 0, t_cap = 0, n_frags = 0;
    std::vector<uint8_t> mods((size_t)slot.size() * nb);
    for (auto& kv : slot) { kv.second = n_mods; memcpy(&mods[(size_t)n_mods * nb], kv.first.data(), nb); ++n_mods; }
    for (Req* r : g) { t_cap = std::max(t_cap, r->ks_key); n_frags += r->th_k; }
    std::vector<uint8_t> t((size_t)n * t_cap + 1, 0), e((size_t)n_frags * el), sg(n_frags), out((size_t)n_frags * nb), st((size_t)n_frags + 8, BFTKV_TH_FAILED);
    std::vector<uint32_t> idx(n), tl(n), fr(n_frags), used(n_frags);
    uint32_t f = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const Req* r = g[i];
      idx[i] = slot[std::string((const char*)r->th_mod, nb)];
      tl[i] = r->ks_key;
      if (tl[i]) memcpy(&t[(size_t)i * t_cap], r->th_a, tl[i]);
      memcpy(&e[(size_t)f * el], r->th_b, (size_t)r->th_k * el);
      memcpy(&sg[f], r->ps_sign, r->th_k);
      for (uint32_t j = 0; j < r->th_k; ++j) { fr[f + j] = i; used[f + j] = r->ps_used ? r->ps_used[j] : el; }
      f += r->th_k;
    }
    const int rc = psign_impl(lane.ctx, n, t.data(), t_cap, tl.data(), idx.data(), n_mods, mods.data(), nb, n_frags, fr.data(), e.data(), el, used.data(),
                              sg.data(), out.data(), st.data());
    ++device_calls;
    f = 0;
    for (Req* r : g) {
      r->rc = rc;
      r->err = rc ? Req::failing(r->kind) : (uint8_t)BFTKV_TH_OK;
      if (!rc) { memcpy(r->th_out, &out[(size_t)f * nb], (size_t)r->th_k * nb); memcpy(r->ps_status, &st[f], r->th_k); }
      f += r->th_k;
    }
  }

  // TdsaShare, TecdsaShare: a group's callers share (set or curve, m) and the widths; every caller is one request of the call.  For a
  // set, the lane holds its hold on the root's tables from the look at the set to the end of the device call (run_verify_keyset).
  void run_tsig_share(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const bool dsa = r0.kind == Kind::TdsaShare;
    const uint32_t n = (uint32_t)g.size(), m = r0.th_k;
    const size_t qw = dsa ? r0.th_qbytes : r0.th_nbytes, rw = dsa ? r0.th_nbytes : 1 + 2 * (size_t)r0.th_nbytes;
    const std::vector<uint8_t> sh = gather(g, &Req::th_a, (size_t)m * 4 * qw);
    std::vector<uint8_t> ri((size_t)n * rw), vi((size_t)n * qw), ki((size_t)n * qw), ci((size_t)n * qw), st((size_t)n + 8, BFTKV_TH_FAILED);
    int rc;
    if (dsa) {
      std::vector<uint32_t> idx(n);
      for (uint32_t i = 0; i < n; ++i) idx[i] = g[i]->ks_key;
      ctx_lock lk(lane.ctx->mu);
      KtRead kr(lane.ctx);
      const DsaKeySet* ks = kr.rc ? nullptr : KeySets<DsaKeySet>::find(lane.ctx, r0.quorum);
      if (kr.rc) rc = kr.rc;
      else if (!ks || ks->pbytes != r0.th_nbytes || ks->qbytes != r0.th_qbytes) rc = BFTKV_E_INVALID;
      else {
        rc = tdsa_share_impl(lane.ctx, r0.quorum, n, idx.data(), m, sh.data(), ri.data(), vi.data(), ki.data(), ci.data(), st.data(), false);
        ++device_calls;
      }
    } else {
      rc = tecdsa_share_impl(lane.ctx, n, m, sh.data(), r0.th_mod, r0.th_qbytes, ri.data(), vi.data(), ki.data(), ci.data(), st.data(), false);
      ++device_calls;
    }
    for (uint32_t i = 0; i < n; ++i) {
      Req* r = g[i];
      r->rc = rc;
      r->err = rc ? Req::failing(r->kind) : st[i];
      if (rc) continue;
      memcpy(r->th_out, &ri[i * rw], rw); memcpy(r->ts_vi, &vi[i * qw], qw); memcpy(r->ts_ki, &ki[i * qw], qw); memcpy(r->ts_ci, &ci[i * qw], qw);
    }
  }

  // RsaSignKeyset: a group's callers share (set, hash id, dlen).  The lane holds its hold on the root's tables from the look at the set,
  // which tells the width of a signature, to the end of the device call (run_verify_keyset).  Whatever fails, a caller whose set was
  // found gets a row of zeroes.
  void run_rsa_sign(Lane& lane, std::vector<Req*>& g, uint64_t& device_calls) {
    const Req& r0 = *g[0];
    const uint32_t n = (uint32_t)g.size(), dlen = r0.th_k, hash_id = r0.th_qbytes;
    std::vector<uint8_t> sig, st((size_t)n + 8, BFTKV_TH_FAILED);
    size_t sw = 0;
    int rc;
    {
      ctx_lock lk(lane.ctx->mu);
      KtRead kr(lane.ctx);
      const RsaSignerSet* ks = kr.rc ? nullptr : KeySets<RsaSignerSet>::find(lane.ctx, r0.quorum);
      sw = ks ? ks->sig_bytes() : 0;
      if (kr.rc) rc = kr.rc;
      else if (!sw) rc = BFTKV_E_INVALID;
      else {
        const std::vector<uint8_t> dg = gather(g, &Req::th_a, dlen);
        std::vector<uint32_t> idx(n);
        for (uint32_t i = 0; i < n; ++i) idx[i] = g[i]->ks_key;
        sig.assign((size_t)n * sw, 0);
        rc = rsa_sign_impl(lane.ctx, r0.quorum, n, dg.data(), hash_id, dlen, nullptr, idx.data(), sig.data(), st.data(), false, false);
        if (rc) std::fill(sig.begin(), sig.end(), 0);
        ++device_calls;
      }
    }
    for (uint32_t i = 0; i < n; ++i) {
      Req* r = g[i];
      r->rc = rc;
      r->err = rc ? Req::failing(r->kind) : st[i];
      if (sw) memcpy(r->th_out, &sig[i * sw], sw);
    }
  }

  // group by (kind, quorum / certificate use, threshold shape): one device call per group
  uint64_t process(Lane& lane, std::vector<Req*>& batch) {
    uint64_t calls = 0;     // device calls made for this batch
    std::vector<bool> taken(batch.size(), false);
    for (size_t i = 0; i < batch.size(); ++i) {
      if (taken[i]) continue;
      std::vector<Req*> g;
      for (size_t j = i; j < batch.size(); ++j)
        if (!taken[j] && batch[j]->kind == batch[i]->kind && batch[j]->quorum == batch[i]->quorum && batch[j]->has_cert == batch[i]->has_cert &&
            batch[j]->th_shape == batch[i]->th_shape) {
          g.push_back(batch[j]); taken[j] = true;
        }
      switch (g[0]->kind) {
        case Kind::Collective: case Kind::Signature: run_group(lane, g, calls); break;
        case Kind::Message: run_messages(lane, g, calls); break;
        case Kind::Cert: run_certs(g, calls); break;
        case Kind::ModmulProduct: case Kind::LagrangeCombine: case Kind::DsaCalculateR: case Kind::Modexp: run_threshold(lane, g, calls); break;
        case Kind::EcdsaCalculateR: run_ecdsa(lane, g, calls); break;
        case Kind::EcdsaVerify: run_ecdsa_verify(lane, g, calls); break;
        case Kind::EcdsaVerifyKeyset:
          run_verify_keyset<EcKeySet>(lane, g, calls, ecdsa_verify_keyset_impl);
          break;
        case Kind::DsaVerify: run_dsa_verify(lane, g, calls); break;
        case Kind::DsaVerifyKeyset:
          run_verify_keyset<DsaKeySet>(lane, g, calls, dsa_verify_keyset_impl);
          break;
        case Kind::RsaVerify: run_rsa_verify(lane, g, calls); break;
        case Kind::RsaVerifyKeyset: {
          const uint32_t hash_id = g[0]->th_qbytes;
          run_verify_keyset<RsaKeySet>(lane, g, calls, [hash_id](bftkv_gpu_ctx* c, int set, uint32_t n, const uint8_t* dg, uint32_t dlen, const uint8_t* sg,
                                                                 const uint32_t* idx, uint8_t* valid, uint8_t* st, bool dev) {
            return rsa_verify_keyset_impl(c, set, n, dg, hash_id, dlen, sg, idx, valid, st, dev);
          });
          break;
        }
        case Kind::TpaYi: case Kind::TpaBi: run_tpa(lane, g, calls); break;
        case Kind::RsaPartialSign: run_psign(lane, g, calls); break;
        case Kind::TdsaShare: case Kind::TecdsaShare: run_tsig_share(lane, g, calls); break;
        case Kind::RsaSignKeyset: run_rsa_sign(lane, g, calls); break;
      }
    }
    return calls;
  }

  int submit(Req& r) {
    r.err = Req::failing(r.kind);
    // entry is announced BEFORE `stop` is looked at (both seq_cst): destroy() sets stop and then waits for inside == 0, so a
    // call that overlaps it either sees stop here and leaves without touching anything else, or is waited for.  (A call that
    // STARTS after destroy() has returned is the caller's bug, as with any destroyed handle.)
    inside.fetch_add(1);
    if (stop.load()) { inside.fetch_sub(1); return BFTKV_E_STATE; }
    // the caller's own thread walks its payload's hash chain (a message's signed bytes are found by the framing)
    if (hashed_by_caller(r.kind)) {
      const uint64_t t_h = now_ns();
      hostsha::midstate(r.tbs, r.tbs_len, r.mid);
      ns_hash.fetch_add(now_ns() - t_h, std::memory_order_relaxed);
    }
    std::shared_ptr<Batch> bt;
    bool leader = false;
    Door& d = my_door();
    d.lock();
    if (!d.open || d.open->reqs.size() >= max_items) { d.open = std::make_shared<Batch>(); leader = true; }   // a full batch is closed to newcomers
    d.open->reqs.push_back(&r);
    bt = d.open;
    d.unlock();
    if (leader) {
      // a lane, or sleep until one is released
      const uint64_t t_w = now_ns();
      Lane* lane = nullptr;
      while (!stop.load(std::memory_order_acquire)) {
        const uint32_t seq = lane_seq.load(std::memory_order_acquire);
        if ((lane = try_lane())) break;
        (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&lane_seq), FUTEX_WAIT_PRIVATE, seq, nullptr, nullptr, 0);
      }
      ns_lane_wait.fetch_add(now_ns() - t_w, std::memory_order_relaxed);
      d.lock();
      if (d.open == bt) d.open.reset();        // taken: later arrivals start the next batch
      d.unlock();
      uint64_t calls = 0;
      if (lane) {                              // (stopped batcher: the requests keep their failing results)
        calls = process(*lane, bt->reqs);
        release_lane(lane);
      }
      const uint64_t n = bt->reqs.size();
      n_calls.fetch_add(n, std::memory_order_relaxed);
      n_batches.fetch_add(calls, std::memory_order_relaxed);
      uint64_t mb = max_batch.load(std::memory_order_relaxed);
      while (n > mb && !max_batch.compare_exchange_weak(mb, n, std::memory_order_relaxed)) {}
      // results are in the callers' requests: publish and wake them (they may return and drop their requests at once)
      bt->done.store(1, std::memory_order_release);
      batch_futex_wake_all(&bt->done);
    } else {
      while (bt->done.load(std::memory_order_acquire) == 0) batch_futex_wait(&bt->done, 0);
    }
    const int rc = r.rc;
    // nothing of the batcher is touched after the decrement: destroy() polls the counter
    inside.fetch_sub(1, std::memory_order_acq_rel);
    return rc;
  }
};

using BatcherKind = bftkv_gpu_batcher::Kind;

extern "C" {

bftkv_gpu_batcher* bftkv_gpu_batcher_create_lanes(bftkv_gpu_ctx* ctx, uint32_t max_items, uint32_t max_wait_us, uint32_t n_lanes) {
  if (!ctx || max_items == 0 || ctx->root) return nullptr;
  if (n_lanes == 0) {
    n_lanes = 3;     // measured (profiles/r03_serving_*): three batches in flight overlap one another's head and tail; more lanes
                     // make more, smaller device calls and each call slower (128 callers: 363 k / 390 k / 304 k calls/s at 2 / 3 / 4)
    if (const char* e = getenv("BFTKV_BATCHER_LANES")) { const int v = atoi(e); if (v > 0) n_lanes = (uint32_t)v; }
  }
  if (n_lanes > 64) n_lanes = 64;
  auto* b = new bftkv_gpu_batcher();
  b->ctx = ctx; b->max_items = max_items; b->max_wait_us = max_wait_us;
  for (uint32_t i = 0; i < n_lanes; ++i) {
    auto l = std::make_unique<bftkv_gpu_batcher::Lane>();
    if (bftkv_gpu_ctx_fork(ctx, &l->ctx) != 0) {
      for (auto& o : b->lanes) bftkv_gpu_destroy(o->ctx);
      delete b;
      return nullptr;
    }
    b->lanes.push_back(std::move(l));
  }
  return b;
}

bftkv_gpu_batcher* bftkv_gpu_batcher_create(bftkv_gpu_ctx* ctx, uint32_t max_items, uint32_t max_wait_us) {
  return bftkv_gpu_batcher_create_lanes(ctx, max_items, max_wait_us, 0);
}

void bftkv_gpu_batcher_destroy(bftkv_gpu_batcher* b) {
  if (!b) return;
  b->stop.store(true);
  while (b->inside.load() != 0) {        // leaders waiting for a lane give up, batches in flight finish
    b->lane_seq.fetch_add(1, std::memory_order_release);
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&b->lane_seq), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
  for (auto& l : b->lanes) bftkv_gpu_destroy(l->ctx);
  delete b;
}

int bftkv_gpu_batcher_collective_verify(bftkv_gpu_batcher* b, int quorum, const uint8_t* tbs, uint64_t tbs_len, const uint8_t* ss,
                                        uint64_t ss_len, uint8_t* err_out, uint8_t* fenced_out) {
  if (err_out) *err_out = BFTKV_ERR_INSUFFICIENT_SIGNATURES;
  if (fenced_out) *fenced_out = 0;
  if (!b || !err_out || (!tbs && tbs_len) || (!ss && ss_len)) return BFTKV_E_INVALID;
  bftkv_gpu_batcher::Req r{BatcherKind::Collective, quorum, tbs, tbs_len, ss, ss_len, false, 0};
  int rc = b->submit(r);
  *err_out = rc ? (uint8_t)BFTKV_ERR_INSUFFICIENT_SIGNATURES : r.err;
  if (fenced_out) *fenced_out = r.fenced;
  return rc;
}

int bftkv_gpu_batcher_signature_verify(bftkv_gpu_batcher* b, const uint8_t* tbs, uint64_t tbs_len, const uint8_t* sig, uint64_t sig_len,
                                       const uint64_t* cert_key_id, uint8_t* err_out, uint8_t* fenced_out) {
  if (err_out) *err_out = BFTKV_ERR_INVALID_SIGNATURE;
  if (fenced_out) *fenced_out = 0;
  if (!b || !err_out || (!tbs && tbs_len) || (!sig && sig_len)) return BFTKV_E_INVALID;
  bftkv_gpu_batcher::Req r{BatcherKind::Signature, bftkv_gpu_batcher::NO_QUORUM, tbs, tbs_len, sig, sig_len, cert_key_id != nullptr, cert_key_id ? *cert_key_id : 0};
  int rc = b->submit(r);
  *err_out = rc ? (uint8_t)BFTKV_ERR_INVALID_SIGNATURE : r.err;
  if (fenced_out) *fenced_out = r.fenced;
  return rc;
}

int bftkv_gpu_batcher_cert_verify(bftkv_gpu_batcher* b, const uint8_t* cert, uint64_t cert_len, const uint8_t* tbs, uint64_t tbs_len,
                                  const uint8_t* sig, uint64_t sig_len, uint8_t* err_out, uint8_t* fenced_out, uint64_t* issuer_id_out,
                                  uint8_t* fingerprint_out) {
  if (err_out) *err_out = BFTKV_ERR_INVALID_SIGNATURE;
  if (fenced_out) *fenced_out = 0;
  if (issuer_id_out) *issuer_id_out = 0;
  if (fingerprint_out) memset(fingerprint_out, 0, 20);
  if (!b || !err_out || (!cert && cert_len) || (!tbs && tbs_len) || (!sig && sig_len)) return BFTKV_E_INVALID;
  static const uint8_t empty = 0;
  // A certificate the root has accepted before (its bytes are in the register of valid request certificates): the request is one
  // signature verification against the entity registered for it -- a staged call on a lane like Signature.Verify's, several in
  // flight, nothing under the root's lock.  Anything but a plain verdict from that route (the register forgot the certificate
  // meanwhile, a fenced shape, an empty signature stream) falls through to the compound call below.
  if (cert_len) {
    bftkv_gpu_ctx::CertFast cf{0, -1, 0};
    bool known = false;
    {
      const std::string key((const char*)cert, cert_len);       // (built outside the lock; lookups share it)
      std::shared_lock<std::shared_mutex> fl(b->ctx->cert_fast_mu);
      auto it = b->ctx->cert_fast.find(key);
      if (it != b->ctx->cert_fast.end()) { cf = it->second; known = true; }
    }
    if (known && !sig) {                       // the issuer alone (Issuer(), server.go:330-331): what the register holds
      b->n_calls.fetch_add(1, std::memory_order_relaxed);
      b->n_cert_fast.fetch_add(1, std::memory_order_relaxed);
      *err_out = BFTKV_ERR_NONE;
      if (issuer_id_out) *issuer_id_out = cf.issuer_id;
      if (fingerprint_out) (void)bftkv_host_cert_fingerprint(cert, cert_len, fingerprint_out);
      return 0;
    }
    if (known && sig_len) {
      bftkv_gpu_batcher::Req f{BatcherKind::Signature, bftkv_gpu_batcher::NO_QUORUM, tbs ? tbs : &empty, tbs_len, sig, sig_len, true, cf.issuer_id};
      f.cert_group = cf.group; f.cert_epoch = cf.epoch;
      const int frc = b->submit(f);
      if (!frc && !f.unresolved && !f.fenced) {
        b->n_cert_fast.fetch_add(1, std::memory_order_relaxed);
        *err_out = f.err;
        if (issuer_id_out) *issuer_id_out = cf.issuer_id;
        if (fingerprint_out) (void)bftkv_host_cert_fingerprint(cert, cert_len, fingerprint_out);
        return 0;
      }
      if (frc == BFTKV_E_STATE) return frc;    // a stopped batcher
      b->n_calls.fetch_sub(1, std::memory_order_relaxed);     // (served once: by the call below)
    }
  }
  bftkv_gpu_batcher::Req r{BatcherKind::Cert, bftkv_gpu_batcher::NO_QUORUM, tbs ? tbs : &empty, tbs_len, sig, sig_len, false, 0};
  r.cert = cert; r.cert_len = cert_len;
  int rc = b->submit(r);
  *err_out = rc ? (uint8_t)BFTKV_ERR_INVALID_SIGNATURE : r.err;
  if (fenced_out) *fenced_out = r.fenced;
  if (issuer_id_out) *issuer_id_out = r.issuer_id;
  if (!rc && fingerprint_out && r.issuer_id) (void)bftkv_host_cert_fingerprint(cert, cert_len, fingerprint_out);
  return rc;
}

int bftkv_gpu_batcher_cert_entity(bftkv_gpu_batcher* b, const uint8_t* cert, uint64_t cert_len, uint8_t* err_out, uint8_t* fenced_out,
                                  uint64_t* issuer_id_out, uint8_t* fingerprint_out, uint64_t* entity_off_out, uint64_t* entity_len_out,
                                  uint32_t* roles_out, uint32_t roles_cap, uint32_t* n_roles_out) {
  if (entity_off_out) *entity_off_out = 0;
  if (entity_len_out) *entity_len_out = 0;
  if (n_roles_out) *n_roles_out = 0;
  if (!n_roles_out || !entity_off_out || !entity_len_out || (roles_cap && !roles_out)) {
    if (err_out) *err_out = BFTKV_ERR_INVALID_SIGNATURE;
    if (fenced_out) *fenced_out = 0;
    return BFTKV_E_INVALID;
  }
  int rc = bftkv_gpu_batcher_cert_verify(b, cert, cert_len, nullptr, 0, nullptr, 0, err_out, fenced_out, issuer_id_out, fingerprint_out);
  if (rc || *err_out != BFTKV_ERR_NONE || (fenced_out && *fenced_out)) return rc;
  // the walk is a function of the bytes alone: parsed again here, on the caller's thread, it is the walk the verdict was given for
  bftkv_certs* cs = bftkv_host_certs_parse(cert, cert_len);
  if (bftkv_host_certs_n_entities(cs) == 0) { bftkv_host_certs_free(cs); *err_out = BFTKV_ERR_CERTIFICATE_NOT_FOUND; return 0; }
  const uint32_t* roles = nullptr;
  uint32_t n = 0;
  uint8_t refused = 0, unknown = 0;
  (void)bftkv_host_certs_structure(cs, 0, &refused, &unknown, nullptr, nullptr);
  (void)bftkv_host_certs_roles(cs, 0, entity_off_out, entity_len_out, &roles, &n);
  if (refused || unknown) { *err_out = BFTKV_ERR_INVALID_SIGNATURE; if (fenced_out) *fenced_out = 1; n = 0; }     // (cannot happen after the verdict above)
  *n_roles_out = n;
  if (n > roles_cap) rc = BFTKV_E_NOMEM;
  else if (n) memcpy(roles_out, roles, (size_t)n * sizeof(uint32_t));
  if (rc) { *err_out = BFTKV_ERR_INVALID_SIGNATURE; }
  bftkv_host_certs_free(cs);
  return rc;
}

int bftkv_gpu_batcher_message_verify(bftkv_gpu_batcher* b, const uint8_t* msg, uint64_t msg_len, uint8_t* status_out, uint64_t* signer_key_id_out,
                                     uint64_t* peer_id_out, uint8_t* plain_out, uint64_t plain_cap, uint64_t* plain_len_out, uint8_t* fname_out,
                                     uint8_t* fname_len_out) {
  if (status_out) *status_out = BFTKV_MSG_READ_ERROR;
  if (!b || !status_out) return BFTKV_E_INVALID;
  bftkv_gpu_batcher::Req r{BatcherKind::Message, bftkv_gpu_batcher::NO_QUORUM, msg, msg_len, nullptr, 0, false, 0};
  r.plain_out = plain_out; r.plain_cap = plain_cap; r.fname_out = fname_out;
  int rc = b->submit(r);
  *status_out = rc ? (uint8_t)BFTKV_MSG_READ_ERROR : r.err;
  if (signer_key_id_out) *signer_key_id_out = r.signer;
  if (peer_id_out) *peer_id_out = r.peer;
  if (plain_len_out) *plain_len_out = r.plain_len;
  if (fname_len_out) *fname_len_out = r.fname_len;
  return rc;
}

// ---- one threshold share-combine operation per call (BASELINE config 5 behind the reference's seam) ----
// a threshold-style request with its shape, about to be filled in by its entry point
static bftkv_gpu_batcher::Req threshold_req(BatcherKind kind, int quorum, uint64_t a, uint64_t b = 0, uint64_t c = 0) {
  bftkv_gpu_batcher::Req r{kind, quorum, nullptr, 0, nullptr, 0, false, 0};
  r.th_shape = bftkv_gpu_batcher::Req::shape(kind, a, b, c);
  return r;
}
// submit, fail closed: the status byte is the request's only when the call succeeded
static int threshold_submit(bftkv_gpu_batcher* b, bftkv_gpu_batcher::Req& r, uint8_t* status_out) {
  const int rc = b->submit(r);
  *status_out = rc ? (uint8_t)BFTKV_TH_FAILED : r.err;
  return rc;
}
// ... and so is the verdict (th_out), for the four verify kinds
static int verdict_submit(bftkv_gpu_batcher* b, bftkv_gpu_batcher::Req& r, uint8_t* status_out) {
  const int rc = threshold_submit(b, r, status_out);
  if (rc) *r.th_out = 0;
  return rc;
}

static int combine_submit(bftkv_gpu_batcher* b, BatcherKind kind, uint32_t k, const int32_t* xs, const uint8_t* a, uint32_t nbytes, const uint8_t* bb,
                          uint32_t qbytes, const uint8_t* mod, const uint8_t* mod2, uint8_t* out, uint32_t out_bytes, uint8_t* status_out) {
  const bool calc_r = kind == BatcherKind::DsaCalculateR;
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (out && out_bytes && out_bytes <= 256) memset(out, 0, out_bytes);
  if (!b || !status_out || !out || !a || !mod || nbytes == 0 || nbytes > 256 || k == 0 || k > 1024) return BFTKV_E_INVALID;
  if ((kind == BatcherKind::LagrangeCombine || calc_r) && !xs) return BFTKV_E_INVALID;
  if (calc_r && (!bb || !mod2 || qbytes == 0 || qbytes > 32)) return BFTKV_E_INVALID;
  if (kind == BatcherKind::Modexp && (!bb || qbytes == 0 || qbytes > 1024)) return BFTKV_E_INVALID;
  // what the batched entry points refuse for the WHOLE call is refused here for this caller alone: an even or over-wide
  // modulus must not fail the strangers it shares a device call with
  if (!(mod[nbytes - 1] & 1) || (calc_r && !(mod2[qbytes - 1] & 1))) return BFTKV_E_UNSUPPORTED;
  if (hostbn::bit_length(mod, nbytes) > 2048 || hostbn::bit_length(mod, nbytes) < 2) return BFTKV_E_UNSUPPORTED;
  if (calc_r && hostbn::bit_length(mod2, qbytes) < 2) return BFTKV_E_UNSUPPORTED;
  bftkv_gpu_batcher::Req r = threshold_req(kind, bftkv_gpu_batcher::NO_QUORUM, k, nbytes, qbytes);
  r.th_k = k; r.th_nbytes = nbytes; r.th_qbytes = qbytes; r.th_xs = xs; r.th_a = a; r.th_b = bb; r.th_mod = mod; r.th_mod2 = mod2; r.th_out = out;
  return threshold_submit(b, r, status_out);
}

int bftkv_gpu_batcher_modmul_product(bftkv_gpu_batcher* b, uint32_t k, const uint8_t* factors, uint32_t nbytes, const uint8_t* mod, uint8_t* out,
                                     uint8_t* status_out) {
  return combine_submit(b, BatcherKind::ModmulProduct, k, nullptr, factors, nbytes, nullptr, 0, mod, nullptr, out, nbytes, status_out);
}
int bftkv_gpu_batcher_lagrange_combine(bftkv_gpu_batcher* b, uint32_t k, const int32_t* xs, const uint8_t* ys, uint32_t nbytes, const uint8_t* mod,
                                       uint8_t* out, uint8_t* status_out) {
  return combine_submit(b, BatcherKind::LagrangeCombine, k, xs, ys, nbytes, nullptr, 0, mod, nullptr, out, nbytes, status_out);
}
int bftkv_gpu_batcher_dsa_calculate_r(bftkv_gpu_batcher* b, uint32_t k, const int32_t* xs, const uint8_t* ri, uint32_t pbytes, const uint8_t* vi,
                                      uint32_t qbytes, const uint8_t* p, const uint8_t* q, uint8_t* r_out, uint8_t* status_out) {
  return combine_submit(b, BatcherKind::DsaCalculateR, k, xs, ri, pbytes, vi, qbytes, p, q, r_out, qbytes, status_out);
}
int bftkv_gpu_batcher_modexp(bftkv_gpu_batcher* b, const uint8_t* base, uint32_t nbytes, const uint8_t* exp, uint32_t exp_len, const uint8_t* mod,
                             uint8_t* out, uint8_t* status_out) {
  return combine_submit(b, BatcherKind::Modexp, 1, nullptr, base, nbytes, exp, exp_len, mod, nullptr, out, nbytes, status_out);
}

int bftkv_gpu_batcher_ecdsa_calculate_r(bftkv_gpu_batcher* b, uint32_t k, const int32_t* xs, const uint8_t* ri, const uint8_t* vi,
                                        const uint8_t* curve, uint32_t bit_size, uint8_t* r_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  const uint32_t f = (bit_size + 7) / 8;
  if (r_out && bit_size && bit_size <= 521) memset(r_out, 0, f);
  if (!b || !status_out || !r_out || !xs || !ri || !vi || !curve || bit_size == 0 || bit_size > 521 || k == 0 || k > 1024) return BFTKV_E_INVALID;
  // refused for this caller alone, as an unsupported modulus is on the other threshold entries
  if (ec_curve_id(curve, bit_size) < 0) return BFTKV_E_UNSUPPORTED;
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::EcdsaCalculateR, bftkv_gpu_batcher::NO_QUORUM, k, bit_size);
  r.th_k = k; r.th_nbytes = f; r.th_qbytes = bit_size; r.th_xs = xs; r.th_a = ri; r.th_b = vi; r.th_mod = curve; r.th_out = r_out;
  return threshold_submit(b, r, status_out);
}

int bftkv_gpu_batcher_ecdsa_verify(bftkv_gpu_batcher* b, const uint8_t* digest, uint32_t dlen, const uint8_t* sig, const uint8_t* key,
                                   const uint8_t* curve, uint32_t bit_size, uint8_t* valid_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (valid_out) *valid_out = 0;
  if (!b || !status_out || !valid_out || !digest || !sig || !key || !curve || bit_size == 0 || bit_size > 521 || dlen == 0 || dlen > 66)
    return BFTKV_E_INVALID;
  if (ec_curve_id(curve, bit_size) < 0) return BFTKV_E_UNSUPPORTED;       // for this caller alone
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::EcdsaVerify, bftkv_gpu_batcher::NO_QUORUM, dlen, bit_size);
  r.th_k = dlen; r.th_nbytes = (bit_size + 7) / 8; r.th_qbytes = bit_size; r.th_a = digest; r.th_b = sig; r.th_mod = curve; r.th_mod2 = key;
  r.th_out = valid_out;
  return verdict_submit(b, r, status_out);
}

// one signature under key `key` of a resident set (an unknown handle fails its own group alone)
static int keyset_submit(bftkv_gpu_batcher* b, BatcherKind kind, uint32_t max_dlen, int keyset, uint32_t key, const uint8_t* digest, uint32_t dlen,
                         const uint8_t* sig, uint8_t* valid_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (valid_out) *valid_out = 0;
  if (!b || !status_out || !valid_out || !digest || !sig || dlen == 0 || dlen > max_dlen) return BFTKV_E_INVALID;
  bftkv_gpu_batcher::Req r = threshold_req(kind, keyset, dlen);
  r.th_k = dlen; r.th_a = digest; r.th_b = sig; r.th_out = valid_out; r.ks_key = key;
  return verdict_submit(b, r, status_out);
}
int bftkv_gpu_batcher_ecdsa_verify_keyset(bftkv_gpu_batcher* b, int keyset, uint32_t key, const uint8_t* digest, uint32_t dlen, const uint8_t* sig,
                                          uint8_t* valid_out, uint8_t* status_out) {
  return keyset_submit(b, BatcherKind::EcdsaVerifyKeyset, 66, keyset, key, digest, dlen, sig, valid_out, status_out);
}
int bftkv_gpu_batcher_dsa_verify_keyset(bftkv_gpu_batcher* b, int keyset, uint32_t key, const uint8_t* digest, uint32_t dlen, const uint8_t* sig,
                                        uint8_t* valid_out, uint8_t* status_out) {
  return keyset_submit(b, BatcherKind::DsaVerifyKeyset, 64, keyset, key, digest, dlen, sig, valid_out, status_out);
}

int bftkv_gpu_batcher_dsa_verify(bftkv_gpu_batcher* b, const uint8_t* digest, uint32_t dlen, const uint8_t* sig, uint32_t qbytes, const uint8_t* y,
                                 uint32_t pbytes, const uint8_t* p, const uint8_t* q, const uint8_t* g, uint8_t* valid_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (valid_out) *valid_out = 0;
  if (!b || !status_out || !valid_out || !digest || !sig || !y || !p || !q || !g || dlen == 0 || dlen > 64 || qbytes == 0 || qbytes > 32 ||
      pbytes == 0 || pbytes > 256)
    return BFTKV_E_INVALID;
  // what the batched entry refuses for the WHOLE call is refused here for this caller alone
  if (!(p[pbytes - 1] & 1) || !(q[qbytes - 1] & 1)) return BFTKV_E_UNSUPPORTED;
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::DsaVerify, bftkv_gpu_batcher::NO_QUORUM, dlen, pbytes, qbytes);
  r.th_k = dlen; r.th_nbytes = pbytes; r.th_qbytes = qbytes; r.th_a = digest; r.th_b = sig; r.th_mod = p; r.th_mod2 = q; r.th_g = g; r.th_y = y;
  r.th_out = valid_out;
  return verdict_submit(b, r, status_out);
}

// A caller whose (hash id, dlen, nbytes) the batched entry would refuse for the WHOLE call is refused here alone, before it joins a batch.
int bftkv_gpu_batcher_rsa_verify(bftkv_gpu_batcher* b, const uint8_t* digest, uint32_t hash_id, uint32_t dlen, const uint8_t* sig, uint32_t nbytes,
                                 const uint8_t* n, uint32_t e, uint8_t* valid_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (valid_out) *valid_out = 0;
  if (!b || !status_out || !valid_out || !digest || !sig || !n || !rsav_shape_ok(hash_id, dlen, nbytes)) return BFTKV_E_INVALID;
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::RsaVerify, bftkv_gpu_batcher::NO_QUORUM, dlen, nbytes, hash_id);
  r.th_k = dlen; r.th_nbytes = nbytes; r.th_qbytes = hash_id; r.th_a = digest; r.th_b = sig; r.th_mod = n; r.ks_key = e; r.th_out = valid_out;
  return verdict_submit(b, r, status_out);
}
int bftkv_gpu_batcher_rsa_verify_keyset(bftkv_gpu_batcher* b, int keyset, uint32_t key, const uint8_t* digest, uint32_t hash_id, uint32_t dlen,
                                        const uint8_t* sig, uint8_t* valid_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (valid_out) *valid_out = 0;
  if (!b || !status_out || !valid_out || !digest || !sig || !rsav_shape_ok(hash_id, dlen, 1)) return BFTKV_E_INVALID;
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::RsaVerifyKeyset, keyset, dlen, hash_id);
  r.th_k = dlen; r.th_qbytes = hash_id; r.th_a = digest; r.th_b = sig; r.th_out = valid_out; r.ks_key = key;
  return verdict_submit(b, r, status_out);
}

// One answer of a server in the password authentication (crypto/auth): makeYi, makeBi.  What bftkv_gpu_tpa_yi / _bi refuse for the WHOLE
// call is refused here for this caller alone, before it joins a batch.
int bftkv_gpu_batcher_tpa_yi(bftkv_gpu_batcher* b, const uint8_t* x, uint32_t nbytes, const uint8_t* y, uint32_t exp_len, const uint8_t* mod,
                             uint8_t* yi_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (yi_out) memset(yi_out, 0, nbytes);
  if (!b || !status_out || !yi_out || !x || !y || !mod || !tpa_shape_ok(TpaMode::Yi, nbytes, exp_len, 0)) return BFTKV_E_INVALID;
  if (!(mod[nbytes - 1] & 1)) return BFTKV_E_UNSUPPORTED;
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::TpaYi, bftkv_gpu_batcher::NO_QUORUM, nbytes, exp_len);
  r.th_nbytes = nbytes; r.th_qbytes = exp_len; r.th_a = x; r.th_b = y; r.th_mod = mod; r.th_out = yi_out;
  return threshold_submit(b, r, status_out);
}
int bftkv_gpu_batcher_tpa_bi(bftkv_gpu_batcher* b, const uint8_t* v, const uint8_t* xi, uint32_t xi_len, uint32_t nbytes, const uint8_t* bexp,
                             uint32_t exp_len, const uint8_t* salt, uint32_t salt_len, const uint8_t* mod, uint8_t* bi_out, uint8_t* keys_out,
                             uint8_t* mac_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (bi_out) memset(bi_out, 0, nbytes);
  if (keys_out) memset(keys_out, 0, 32);
  if (mac_out) memset(mac_out, 0, 32);
  if (!b || !status_out || !bi_out || !keys_out || !mac_out || !v || !bexp || !mod || !tpa_shape_ok(TpaMode::Bi, nbytes, exp_len, salt_len) ||
      xi_len > nbytes || (xi_len && !xi) || (salt_len && !salt))
    return BFTKV_E_INVALID;
  if (!(mod[nbytes - 1] & 1)) return BFTKV_E_UNSUPPORTED;
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::TpaBi, bftkv_gpu_batcher::NO_QUORUM, nbytes, exp_len, salt_len);
  r.th_k = salt_len; r.th_nbytes = nbytes; r.th_qbytes = exp_len; r.th_a = v; r.th_b = bexp; r.th_mod = mod; r.th_g = xi; r.th_y = salt; r.ks_key = xi_len;
  r.th_out = bi_out; r.tpa_keys = keys_out; r.tpa_mac = mac_out;
  const int rc = threshold_submit(b, r, status_out);
  if (rc || *status_out != BFTKV_TH_OK) { memset(bi_out, 0, nbytes); memset(keys_out, 0, 32); memset(mac_out, 0, 32); }
  return rc;
}

// ONE sign request of a threshold-RSA server (rsaContext.Sign) with all its fragments.  What bftkv_gpu_rsa_partial_sign refuses for the
// WHOLE call is refused here for this caller alone, before it joins a batch.
int bftkv_gpu_batcher_rsa_partial_sign(bftkv_gpu_batcher* b, const uint8_t* t, uint32_t t_len, const uint8_t* mod, uint32_t nbytes, uint32_t n_frags,
                                       const uint8_t* exps, uint32_t exp_len, const uint32_t* exp_used, const uint8_t* sign, uint8_t* out,
                                       uint8_t* status_out) {
  const bool counted = n_frags != 0 && n_frags <= PSIGN_BATCHER_FRAGS;
  const PsignOut o{out, status_out, counted ? n_frags : 0u, nbytes};
  o.fail_closed();
  if (!b || !counted || !status_out || !out || !mod || !exps || !sign || !psign_shape_ok(nbytes, exp_len, t_len) || (t_len && !t)) return BFTKV_E_INVALID;
  {
    std::vector<uint32_t> used(n_frags);
    std::vector<uint8_t> negative(n_frags);
    if (!psign_frags_ok(n_frags, exps, exp_len, exp_used, sign, used.data(), negative.data())) return BFTKV_E_INVALID;
  }
  if (!(mod[nbytes - 1] & 1) && !psign_all_zero(mod, nbytes)) return BFTKV_E_UNSUPPORTED;      // (N = 0 is a refused request, not an even modulus)
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::RsaPartialSign, bftkv_gpu_batcher::NO_QUORUM, nbytes, exp_len);
  r.th_k = n_frags; r.th_nbytes = nbytes; r.th_qbytes = exp_len; r.th_a = t; r.ks_key = t_len; r.th_b = exps; r.th_mod = mod; r.th_out = out;
  r.ps_used = exp_used; r.ps_sign = sign; r.ps_status = status_out;
  const int rc = b->submit(r);
  if (rc) o.fail_closed();
  return rc;
}

// ONE sign request of a threshold DSA / ECDSA server (dsaContext.Sign, phase 2) with its m shares.  What the batched entries refuse for
// the WHOLE call is refused here for this caller alone, before it joins a batch.
static int tsig_share_submit(bftkv_gpu_batcher* b, bftkv_gpu_batcher::Req& r, const TsigOut& o) {
  r.th_out = o.ri; r.ts_vi = o.vi; r.ts_ki = o.ki; r.ts_ci = o.ci;
  const int rc = threshold_submit(b, r, o.st);
  if (rc) (void)o.fail_closed(nullptr);
  return rc;
}
int bftkv_gpu_batcher_tdsa_share(bftkv_gpu_batcher* b, int dsa_keyset, uint32_t group_idx, uint32_t m, const uint8_t* shares, uint32_t pbytes,
                                 uint32_t qbytes, uint8_t* ri_out, uint8_t* vi_out, uint8_t* ki_out, uint8_t* ci_out, uint8_t* status_out) {
  const bool sized = pbytes != 0 && pbytes <= 256 && qbytes != 0 && qbytes <= 32;
  const TsigOut o{ri_out, vi_out, ki_out, ci_out, status_out, 1, sized ? pbytes : 0u, sized ? qbytes : 0u, false};
  (void)o.fail_closed(nullptr);
  if (!b || !sized || !tsig_counts_ok(1, m) || !shares || !o.complete()) return BFTKV_E_INVALID;
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::TdsaShare, dsa_keyset, m, pbytes, qbytes);
  r.th_k = m; r.th_nbytes = pbytes; r.th_qbytes = qbytes; r.th_a = shares; r.ks_key = group_idx;
  return tsig_share_submit(b, r, o);
}
int bftkv_gpu_batcher_tecdsa_share(bftkv_gpu_batcher* b, uint32_t m, const uint8_t* shares, const uint8_t* curve, uint32_t bit_size, uint8_t* ri_out,
                                   uint8_t* vi_out, uint8_t* ki_out, uint8_t* ci_out, uint8_t* status_out) {
  const bool sized = bit_size != 0 && bit_size <= 521;
  const uint32_t f = (bit_size + 7) / 8;
  const TsigOut o{ri_out, vi_out, ki_out, ci_out, status_out, 1, sized ? 1 + 2 * (size_t)f : 0, sized ? f : 0u, false};
  (void)o.fail_closed(nullptr);
  if (!b || !sized || !curve || !tsig_counts_ok(1, m) || !shares || !o.complete()) return BFTKV_E_INVALID;
  if (ec_curve_id(curve, bit_size) < 0) return BFTKV_E_UNSUPPORTED;       // for this caller alone
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::TecdsaShare, bftkv_gpu_batcher::NO_QUORUM, m, bit_size);
  r.th_k = m; r.th_nbytes = f; r.th_qbytes = bit_size; r.th_a = shares; r.th_mod = curve;
  return tsig_share_submit(b, r, o);
}

// ONE raw RSA signature under key `key` of a resident signer set.  A caller whose (hash id, dlen) the batched entry would refuse for the
// WHOLE call is refused here alone, before it joins a batch.
int bftkv_gpu_batcher_rsa_sign_keyset(bftkv_gpu_batcher* b, int set, uint32_t key, const uint8_t* digest, uint32_t dlen, uint32_t hash_id,
                                      uint8_t* sig_out, uint8_t* status_out) {
  if (status_out) *status_out = BFTKV_TH_FAILED;
  if (!b || !status_out || !sig_out || !digest || !rsav_shape_ok(hash_id, dlen, 1)) return BFTKV_E_INVALID;
  bftkv_gpu_batcher::Req r = threshold_req(BatcherKind::RsaSignKeyset, set, dlen, hash_id);
  r.th_k = dlen; r.th_qbytes = hash_id; r.th_a = digest; r.th_out = sig_out; r.ks_key = key;
  return threshold_submit(b, r, status_out);
}

int bftkv_gpu_batcher_stats(bftkv_gpu_batcher* b, uint64_t stats[4]) {
  if (!b || !stats) return BFTKV_E_INVALID;
  stats[0] = b->n_calls.load(); stats[1] = b->n_batches.load(); stats[2] = b->max_batch.load(); stats[3] = b->lanes.size();
  return 0;
}

// The staged route for callers that hold a small batch themselves: payload chains hashed on the calling thread, one pinned
// buffer in, results through mapped host memory (what a batcher's leader does for its batch).
static int small_verify(bftkv_gpu_ctx* c, bool collective, int quorum, uint32_t n, const uint8_t* tbs, const uint64_t* tbs_off, const uint8_t* ss,
                        const uint64_t* ss_off, const uint64_t* cert_key_id, uint8_t* err_out, uint8_t* fenced_out) {
  if (!c || (n && (!tbs_off || !ss_off || !err_out))) return BFTKV_E_INVALID;
  if (n == 0) return 0;
  const uint8_t failing = collective ? BFTKV_ERR_INSUFFICIENT_SIGNATURES : BFTKV_ERR_INVALID_SIGNATURE;
  for (uint32_t i = 0; i < n; ++i) { err_out[i] = failing; if (fenced_out) fenced_out[i] = 0; }
  int rco;
  if ((rco = check_offsets(c, tbs_off, n, "tbs_off not monotone from 0")) || (rco = check_offsets(c, ss_off, n, "ss_off not monotone from 0"))) return rco;
  std::vector<uint32_t> mids((size_t)n * 8);
  std::vector<StagedItem> items(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* t = tbs + tbs_off[i];
    const uint64_t tl = tbs_off[i + 1] - tbs_off[i];
    hostsha::midstate(t, tl, &mids[(size_t)i * 8]);
    items[i] = StagedItem{t, tl, ss + ss_off[i], ss_off[i + 1] - ss_off[i], cert_key_id ? cert_key_id[i] : 0, &mids[(size_t)i * 8]};
  }
  std::vector<uint8_t> fenced(n);
  uint64_t calls = 0;
  ctx_lock lk(c->mu);      // the context's staging buffers
  if (!c->small_pin) c->small_pin = new PinnedBuf[3];
  PinnedBuf* pb = (PinnedBuf*)c->small_pin;
  const int rc = staged_group(c, pb[0], pb[1], pb[2], collective, quorum, cert_key_id != nullptr, items, err_out, fenced.data(), failing, &calls);
  if (fenced_out) copy_out(fenced_out, fenced.data(), n);
  return rc;
}

int bftkv_gpu_collective_verify_small(bftkv_gpu_ctx* c, int quorum, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off, const uint8_t* ss,
                                      const uint64_t* ss_off, uint8_t* err_out, uint8_t* fenced_out) {
  return small_verify(c, true, quorum, n_items, tbs, tbs_off, ss, ss_off, nullptr, err_out, fenced_out);
}

int bftkv_gpu_signature_verify_small(bftkv_gpu_ctx* c, uint32_t n_items, const uint8_t* tbs, const uint64_t* tbs_off, const uint8_t* sig,
                                     const uint64_t* sig_off, const uint64_t* cert_key_id, uint8_t* err_out, uint8_t* fenced_out) {
  return small_verify(c, false, -1, n_items, tbs, tbs_off, sig, sig_off, cert_key_id, err_out, fenced_out);
}

int bftkv_gpu_batcher_times(bftkv_gpu_batcher* b, uint64_t ns[8]) {
  if (!b || !ns) return BFTKV_E_INVALID;
  ns[0] = b->ns_hash.load(); ns[1] = b->ns_lane_wait.load(); ns[2] = b->ns_assemble.load(); ns[3] = b->ns_device.load();
  ns[4] = b->ns_launch.load(); ns[5] = b->ns_spin.load(); ns[6] = b->n_spin_timeouts.load(); ns[7] = b->n_cert_fast.load();
  return 0;
}

// SHA-256 of a byte string with the batcher's host-side compression (mode 0: the fastest this CPU offers, 1: the portable
// rounds) -- lets the CPU suite pin both against hashlib.
int bftkv_host_sha256(const uint8_t* data, uint64_t len, int mode, uint8_t out[32]) {
  if ((!data && len) || !out || mode < 0 || mode > 1) return BFTKV_E_INVALID;
  hostsha::digest(data, len, out, mode);
  return hostsha::have_shani() ? 1 : 0;
}

}  // extern "C"
