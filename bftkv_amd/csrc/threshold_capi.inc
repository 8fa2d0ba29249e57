// C ABI of the threshold share-combine entry points (include/bftkv_gpu.h, config 5).
namespace {

// Per-call device temporaries come from a grow-only pool owned by the context (handed out in call order, so a repeated
// call shape re-uses the same allocations: no hipMalloc / hipFree on the steady-state path).
struct ScratchBufs {
  bftkv_gpu_ctx* c;
  size_t next = 0;
  explicit ScratchBufs(bftkv_gpu_ctx* ctx) : c(ctx) {}
  DevBuf* add() {
    if (next == c->scratch_pool.size()) c->scratch_pool.push_back(new DevBuf());
    return c->scratch_pool[next++];
  }
};

// moduli (big-endian, nbytes each) -> device ModTab.  Tables are cached per context by the modulus bytes (a protocol
// instance combines under the same few moduli call after call), so the steady state uploads nothing; a new table is
// uploaded from a local vector and waited for before that vector dies.
// bounded: called once at the start of an entry point (never between the two tables of one call)
int modtab_gc(bftkv_gpu_ctx* c) {
  if (c->modtab_cache.size() < 256) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (auto& kv : c->modtab_cache) for (DevBuf& b : kv.second) b.release();
  c->modtab_cache.clear();
  return 0;
}
int make_modtab(bftkv_gpu_ctx* c, ScratchBufs& sb, const uint8_t* mods, uint32_t n_mods, uint32_t nbytes, ModTab* mt) {
  (void)sb;
  std::string key((const char*)mods, (size_t)n_mods * nbytes);
  key.push_back((char)(nbytes & 0xFF)); key.push_back((char)(nbytes >> 8));
  auto it = c->modtab_cache.find(key);
  if (it == c->modtab_cache.end()) {
    std::vector<uint32_t> nl((size_t)n_mods * MONT_N), r2((size_t)n_mods * MONT_N), n0(n_mods), r2w((size_t)n_mods * MONT_N_WIDE),
        nlw(MONT_N_WIDE);
    // The rows of ONE modulus are remembered on the host by its bytes (ADVICE r05): the micro-batcher hands over whichever moduli
    // its callers of the moment brought, so the SETS differ from call to call while the moduli recur -- a new set then costs its
    // uploads, not two mont_setup per modulus.
    for (uint32_t m = 0; m < n_mods; ++m) {
      const uint8_t* mp = mods + (size_t)m * nbytes;
      std::string mk((const char*)mp, nbytes);
      auto rit = c->modrow_cache.find(mk);
      if (rit == c->modrow_cache.end()) {
        if (hostbn::bit_length(mp, nbytes) > 2048) return fail(c, BFTKV_E_UNSUPPORTED, "modulus wider than 2048 bits");
        std::vector<uint32_t> row(2 * MONT_N + 1 + MONT_N_WIDE);
        if (!hostbn::mont_setup(mp, nbytes, MONT_N, &row[0], &row[MONT_N], &row[2 * MONT_N])) return fail(c, BFTKV_E_UNSUPPORTED, "even modulus");
        uint32_t n0w;                                   // R = 2^2240 for the 8-lane multiplier (same n, same -n^-1 mod 2^28)
        hostbn::mont_setup(mp, nbytes, MONT_N_WIDE, nlw.data(), &row[2 * MONT_N + 1], &n0w);
        if (c->modrow_cache.size() >= 4096) c->modrow_cache.clear();
        rit = c->modrow_cache.emplace(std::move(mk), std::move(row)).first;
      }
      const std::vector<uint32_t>& row = rit->second;
      std::copy(row.begin(), row.begin() + MONT_N, nl.begin() + (size_t)m * MONT_N);
      std::copy(row.begin() + MONT_N, row.begin() + 2 * MONT_N, r2.begin() + (size_t)m * MONT_N);
      n0[m] = row[2 * MONT_N];
      std::copy(row.begin() + 2 * MONT_N + 1, row.end(), r2w.begin() + (size_t)m * MONT_N_WIDE);
    }
    std::array<DevBuf, 4> bufs;
    int rc;
    if ((rc = upload(c, bufs[0], nl)) || (rc = upload(c, bufs[1], r2)) || (rc = upload(c, bufs[2], n0)) || (rc = upload(c, bufs[3], r2w))) {
      for (DevBuf& b : bufs) b.release();
      return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    it = c->modtab_cache.emplace(std::move(key), bufs).first;
  }
  mt->n_limbs = it->second[0].as<uint32_t>(); mt->r2_limbs = it->second[1].as<uint32_t>(); mt->n0inv = it->second[2].as<uint32_t>();
  mt->r2w_limbs = it->second[3].as<uint32_t>();
  return 0;
}

// host big-endian numbers -> device radix-2^28 limbs
// (dev: src already is a device pointer -- the *_dev entry points, inputs resident in HBM)
int to_dev_limbs(bftkv_gpu_ctx* c, ScratchBufs& sb, const uint8_t* src, size_t count, uint32_t nbytes, uint32_t** out, bool dev = false) {
  DevBuf *raw = sb.add(), *lim = sb.add();
  if (!dev) HIPCHK(c, raw->ensure(count * nbytes + 16));
  HIPCHK(c, lim->ensure(count * MONT_N * 4 + 16));
  if (!dev) HIPCHK(c, hipMemcpyAsync(raw->p, src, count * nbytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_bytes_to_limbs, dim3((uint32_t)((count * MONT_N + 255) / 256)), dim3(256), 0, c->stream, dev ? src : raw->as<uint8_t>(), nbytes,
                     (uint32_t)count, lim->as<uint32_t>());
  *out = lim->as<uint32_t>();
  return 0;
}

int from_dev_limbs(bftkv_gpu_ctx* c, ScratchBufs& sb, const uint32_t* limbs, size_t count, uint32_t nbytes, uint8_t* dst, bool dev = false) {
  DevBuf* raw = sb.add();
  if (!dev) HIPCHK(c, raw->ensure(count * nbytes + 16));
  hipLaunchKernelGGL(k_limbs_to_bytes, dim3((uint32_t)((count * nbytes + 255) / 256)), dim3(256), 0, c->stream, limbs, nbytes, (uint32_t)count,
                     dev ? dst : raw->as<uint8_t>());
  if (!dev) HIPCHK(c, hipMemcpyAsync(dst, raw->p, count * nbytes, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

template <typename T>
int to_dev(bftkv_gpu_ctx* c, ScratchBufs& sb, const T* src, size_t count, T** out, bool dev = false) {
  DevBuf* b = sb.add();
  if (dev) { *out = const_cast<T*>(src); return 0; }
  HIPCHK(c, b->ensure(count * sizeof(T) + 16));
  HIPCHK(c, hipMemcpyAsync(b->p, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
  *out = b->as<T>();
  return 0;
}

// modulus / group indices: validated on the host for host callers; device callers get a clamped copy (an index past the
// table would read beyond the ModTab arrays)
__global__ void k_clamp_idx(const uint32_t* __restrict__ in, uint32_t n, uint32_t n_mods, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in ? min(in[i], n_mods - 1u) : 0u;
}
int idx_to_dev(bftkv_gpu_ctx* c, ScratchBufs& sb, const uint32_t* idx, uint32_t n_ops, uint32_t n_mods, uint32_t** out, bool dev) {
  if (!dev) {
    for (uint32_t i = 0; i < n_ops; ++i) if (idx[i] >= n_mods) return fail(c, BFTKV_E_INVALID, "mod_idx out of range");
    return to_dev(c, sb, idx, n_ops, out);
  }
  DevBuf* b = sb.add();
  HIPCHK(c, b->ensure((size_t)n_ops * 4 + 16));
  hipLaunchKernelGGL(k_clamp_idx, dim3((n_ops + 255) / 256), dim3(256), 0, c->stream, idx, n_ops, n_mods, b->as<uint32_t>());
  *out = b->as<uint32_t>();
  return 0;
}
// lanes per number: 8 while that still leaves at most one wave per SIMD (8192 operations on 256 CUs), else 4.  The call is
// as long as its longest-loaded SIMD: an 8-lane wave runs 0.68x the instructions of a 4-lane one (measured: the m-broadcast
// and window shifts do not shrink with the limbs), so 8 lanes win only while no SIMD gets two of them -- 10,000 operations:
// 4 lanes 10.3 ms, 8 lanes 12.8 ms (1250 waves on 1024 SIMDs).  knob: the caller's experiment knob (4 | 8 overrides, 0 = by size).
inline bool lanes_wide(const bftkv_gpu_ctx* c, uint32_t knob, uint64_t n_ops) {
  return knob ? knob == 8 : n_ops * MULTI_TPI8 <= (uint64_t)c->n_cus * 4 * 64;
}
// end of a call: host callers wait for their results; device callers stay asynchronous on the context's stream
int finish(bftkv_gpu_ctx* c, bool dev) {
  if (!dev) HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return 0;
}
// The kernels OR their findings into the byte (1 = an inverse does not exist, 2 = beyond the native bounds): an operation can
// collect both.  Callers see ONE of the documented values (bftkv_gpu.h: BFTKV_TH_OK / _NO_INVERSE / _FENCED), fenced winning --
// "no statement about the reference" must not be read as "the reference would dereference nil" (ADVICE r05).
int copy_status(bftkv_gpu_ctx* c, uint8_t* status_out, const void* d_st, uint32_t n_ops, bool dev) {
  if (!status_out || !n_ops) return 0;
  hipLaunchKernelGGL(k_status_normalise, dim3((n_ops + 255) / 256), dim3(256), 0, c->stream, (uint8_t*)const_cast<void*>(d_st), n_ops);
  HIPCHK(c, hipMemcpyAsync(status_out, d_st, n_ops, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int dev_alloc(bftkv_gpu_ctx* c, ScratchBufs& sb, size_t bytes, void** out, bool zero) {
  DevBuf* b = sb.add();
  HIPCHK(c, b->ensure(bytes + 16));
  if (zero) HIPCHK(c, hipMemsetAsync(b->p, 0, bytes + 16, c->stream));
  *out = b->p;
  return 0;
}

inline dim3 quad_grid(uint32_t n_ops) { return dim3((n_ops + QUADS_PER_BLOCK - 1) / QUADS_PER_BLOCK); }

}  // namespace

// Every entry point exists in two forms sharing one body: host pointers in / out (copy-in, kernels, copy-out, wait), and
// `_dev` with the per-operation arrays already resident in HBM and the results left there, asynchronous on the context's
// stream (moduli -- a few hundred bytes per distinct modulus -- stay host pointers in both forms).
namespace {

// Does any term of any operation leave k_lagrange_inv's exact 31-bit integers (its own rule, restated for host callers)?  Device
// callers cannot be asked: for them the big-integer kernels are always enqueued (their grids return at once for operations that
// are not flagged).
bool lagrange_needs_big(const int32_t* xs, uint32_t n_ops, uint32_t k) {
  for (uint32_t op = 0; op < n_ops; ++op) {
    const int32_t* x = xs + (size_t)op * k;
    for (uint32_t j = 0; j < k; ++j) {
      int64_t a = 1, b = 1;
      for (uint32_t i = 0; i < k; ++i) {
        if (x[i] == x[j]) continue;
        a *= x[i];
        b *= (int64_t)x[i] - x[j];
        if (a >= (1ll << 31) || a <= -(1ll << 31) || b >= (1ll << 31) || b <= -(1ll << 31)) return true;
      }
      if (a < 0) return true;
    }
  }
  return false;
}

// Device-resident callers: the x's cannot be looked at, but the caller may have promised 0 <= x <= bound
// (bftkv_gpu_set_lagrange_x_bound): then |a| <= bound^(k-1) and |b| <= bound^(k-1) -- within k_lagrange_inv's 31 bits or not.
bool lagrange_bound_says_small(const bftkv_gpu_ctx* c, uint32_t k) {
  if (!c->lagrange_x_bound) return false;
  uint64_t v = 1;
  for (uint32_t i = 1; i < k; ++i) { v *= c->lagrange_x_bound; if (v >= (1ull << 31)) return false; }
  return true;
}

// The big-integer side of the Lagrange coefficients (threshold_kernels.hip): redoes the operations k_lagrange_inv flagged and
// overwrites their rows of lambda_out / sum_out and their status byte.  Enqueued BEHIND k_lagrange_terms.
int lagrange_big_path(bftkv_gpu_ctx* c, ScratchBufs& sb, uint32_t n_ops, uint32_t k, const int32_t* d_xs, const uint32_t* d_y, const uint32_t* d_mi,
                      const ModTab& mt, uint32_t* lambda_out, uint32_t* sum_out, uint8_t* d_st, uint32_t mod_bytes) {
  const size_t nk = (size_t)n_ops * k;
  void *d_ab, *d_bb, *d_sg, *d_bst, *d_pre, *d_dp, *d_di, *d_ist;
  int rc;
  if ((rc = dev_alloc(c, sb, nk * MONT_N * 4, &d_ab, false)) || (rc = dev_alloc(c, sb, nk * MONT_N * 4, &d_bb, false)) || (rc = dev_alloc(c, sb, nk + 8, &d_sg, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_bst, true)) || (rc = dev_alloc(c, sb, nk * MONT_N * 4, &d_pre, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_dp, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_di, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_ist, true)))
    return rc;
  hipStream_t s = c->stream;
  hipLaunchKernelGGL(k_lagrange_big, dim3((uint32_t)((nk + 63) / 64)), dim3(64), 0, s, n_ops, k, d_xs, (const uint8_t*)d_st, (uint32_t*)d_ab, (uint32_t*)d_bb,
                     (uint8_t*)d_sg, (uint8_t*)d_bst);
  hipLaunchKernelGGL(k_lagrange_prep, quad_grid(n_ops), dim3(RSA_BLOCK), 0, s, n_ops, k, (uint32_t*)d_bb, (const uint8_t*)d_st, (const uint8_t*)d_bst, d_mi, mt,
                     (uint32_t*)d_pre, (uint32_t*)d_dp);
  // the one inverse per operation: 256-bit arithmetic under an order q (calculateS, CalculateR), the 2176-bit binary GCD otherwise
  if (mod_bytes <= 32)
    hipLaunchKernelGGL(k_u256_inv_modq, dim3((n_ops + 63) / 64), dim3(64), 0, s, n_ops, (const uint32_t*)d_dp, d_mi, mt, (uint32_t*)d_di, (uint8_t*)d_ist,
                       (const uint8_t*)d_st, (const uint8_t*)d_bst);
  else
    hipLaunchKernelGGL(k_modinv, dim3((n_ops + 63) / 64), dim3(64), 0, s, n_ops, (const uint32_t*)d_dp, d_mi, mt, (uint32_t*)d_di, (uint8_t*)d_ist,
                       (const uint8_t*)d_st, (const uint8_t*)d_bst);
  hipLaunchKernelGGL(k_lagrange_finish, quad_grid(n_ops), dim3(RSA_BLOCK), 0, s, n_ops, k, (const uint32_t*)d_ab, (const uint32_t*)d_bb, (const uint8_t*)d_sg,
                     (const uint32_t*)d_pre, (uint32_t*)d_di, (uint32_t*)d_dp /*D is spent: the row of -D^-1 R^2*/, (const uint8_t*)d_ist, (const uint8_t*)d_bst, d_y,
                     d_mi, mt, lambda_out, sum_out, d_st);
  return 0;
}

int modmul_product_impl(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const uint8_t* factors, uint32_t nbytes, const uint32_t* mod_idx,
                        uint32_t n_mods, const uint8_t* mods, uint8_t* out, bool dev) {
  if (!c || nbytes == 0 || nbytes > 256 || k == 0 || n_mods == 0 || (n_ops && (!factors || (!mod_idx && !dev) || !mods || !out))) return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mt;
  int rc;
  uint32_t *d_f, *d_mi;
  void* d_out;
  if ((rc = make_modtab(c, sb, mods, n_mods, nbytes, &mt))) return rc;
  if ((rc = idx_to_dev(c, sb, mod_idx, n_ops, n_mods, &d_mi, dev))) return rc;
  if ((rc = to_dev_limbs(c, sb, factors, (size_t)n_ops * k, nbytes, &d_f, dev))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_out, false))) return rc;
  hipLaunchKernelGGL(k_modmul_product, quad_grid(n_ops), dim3(RSA_BLOCK), 0, c->stream, n_ops, k, d_f, d_mi, mt, (uint32_t*)d_out);
  if ((rc = from_dev_limbs(c, sb, (uint32_t*)d_out, n_ops, nbytes, out, dev))) return rc;
  return finish(c, dev);
}

int lagrange_combine_impl(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ys, uint32_t nbytes,
                          const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods, uint8_t* out, uint8_t* status_out, bool dev) {
  if (!c || nbytes == 0 || nbytes > 256 || k == 0 || n_mods == 0 || (n_ops && (!xs || !ys || (!mod_idx && !dev) || !mods || !out))) return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mt;
  int rc;
  uint32_t *d_y, *d_mi;
  int32_t* d_xs;
  void *d_inv, *d_st, *d_out;
  if ((rc = make_modtab(c, sb, mods, n_mods, nbytes, &mt))) return rc;
  if ((rc = idx_to_dev(c, sb, mod_idx, n_ops, n_mods, &d_mi, dev))) return rc;
  if ((rc = to_dev_limbs(c, sb, ys, (size_t)n_ops * k, nbytes, &d_y, dev))) return rc;
  if ((rc = to_dev(c, sb, xs, (size_t)n_ops * k, &d_xs, dev))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * k * MONT_N * 4, &d_inv, false))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_st, true))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_out, false))) return rc;
  hipLaunchKernelGGL(k_lagrange_inv, dim3((n_ops * k + 63) / 64), dim3(64), 0, c->stream, n_ops, k, d_xs, d_mi, mt, (uint32_t*)d_inv, (uint8_t*)d_st);
  hipLaunchKernelGGL(k_lagrange_terms, quad_grid(n_ops), dim3(RSA_BLOCK), 0, c->stream, n_ops, k, (uint32_t*)d_inv, d_y, d_mi, mt,
                     (uint32_t*)nullptr, (uint32_t*)d_out, (const uint8_t*)d_st);
  uint32_t mod_w = 0;        // the widest modulus of the call, in bytes (the big path inverts under it: 256-bit arithmetic when it fits)
  for (uint32_t m = 0; m < n_mods; ++m) mod_w = std::max(mod_w, ((uint32_t)hostbn::bit_length(mods + (size_t)m * nbytes, nbytes) + 7u) / 8u);
  if (dev ? !lagrange_bound_says_small(c, k) : lagrange_needs_big(xs, n_ops, k))
    if ((rc = lagrange_big_path(c, sb, n_ops, k, d_xs, d_y, d_mi, mt, nullptr, (uint32_t*)d_out, (uint8_t*)d_st, mod_w))) return rc;
  if ((rc = from_dev_limbs(c, sb, (uint32_t*)d_out, n_ops, nbytes, out, dev))) return rc;
  if ((rc = copy_status(c, status_out, d_st, n_ops, dev))) return rc;
  return finish(c, dev);
}

int dsa_calculate_r_impl(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ri, uint32_t pbytes,
                         const uint8_t* vi, uint32_t qbytes, const uint32_t* group_idx, uint32_t n_groups, const uint8_t* p,
                         const uint8_t* q, uint8_t* r_out, uint8_t* status_out, bool dev) {
  if (!c || pbytes == 0 || pbytes > 256 || qbytes == 0 || qbytes > 32 || k == 0 || n_groups == 0 ||
      (n_ops && (!xs || !ri || !vi || (!group_idx && !dev) || !p || !q || !r_out)))
    return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mp, mq;
  int rc;
  uint32_t *d_ri, *d_vi, *d_gi;
  int32_t* d_xs;
  void *d_inv, *d_st, *d_lam, *d_prod, *d_v, *d_vinv, *d_scr, *d_r, *d_rq;
  if ((rc = make_modtab(c, sb, p, n_groups, pbytes, &mp))) return rc;
  if ((rc = make_modtab(c, sb, q, n_groups, qbytes, &mq))) return rc;
  if ((rc = idx_to_dev(c, sb, group_idx, n_ops, n_groups, &d_gi, dev))) return rc;
  if ((rc = to_dev_limbs(c, sb, ri, (size_t)n_ops * k, pbytes, &d_ri, dev))) return rc;
  if ((rc = to_dev_limbs(c, sb, vi, (size_t)n_ops * k, qbytes, &d_vi, dev))) return rc;
  if ((rc = to_dev(c, sb, xs, (size_t)n_ops * k, &d_xs, dev))) return rc;
  const size_t nk = (size_t)n_ops * k;
  if ((rc = dev_alloc(c, sb, nk * MONT_N * 4, &d_inv, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_st, true)) || (rc = dev_alloc(c, sb, nk * MONT_N * 4, &d_lam, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_prod, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_v, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_vinv, false)) || (rc = dev_alloc(c, sb, nk * MULTIEXP_ENT * MONT_N * 4, &d_scr, false)) ||
      (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_r, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_rq, false)))
    return rc;
  hipStream_t s = c->stream;
  // l_j mod q (explicit, they are exponents) and v = sum Vi_j * l_j mod q
  hipLaunchKernelGGL(k_lagrange_inv, dim3((n_ops * k + 63) / 64), dim3(64), 0, s, n_ops, k, d_xs, d_gi, mq, (uint32_t*)d_inv, (uint8_t*)d_st);
  hipLaunchKernelGGL(k_lagrange_terms, quad_grid(n_ops), dim3(RSA_BLOCK), 0, s, n_ops, k, (uint32_t*)d_inv, d_vi, d_gi, mq,
                     (uint32_t*)d_lam, (uint32_t*)d_v, (const uint8_t*)d_st);
  if (dev ? !lagrange_bound_says_small(c, k) : lagrange_needs_big(xs, n_ops, k))
    if ((rc = lagrange_big_path(c, sb, n_ops, k, d_xs, d_vi, d_gi, mq, (uint32_t*)d_lam, (uint32_t*)d_v, (uint8_t*)d_st, qbytes))) return rc;
  // prod Ri_j ^ l_j mod p.  The bases of an operation CAN be split over `parts` quads (partial products multiplied up by
  // k_modmul_product), but measured at k = 8, 10,000 operations: 4 parts 15.1 ms, unsplit 12.9 ms -- every part repeats the 280
  // shared squarings and the kernel's 240 VGPRs allow only two waves per SIMD, so the extra waves queue instead of overlapping.
  // Kept for wide combines (k >= 32), where the squarings are a small share.
  uint32_t parts = c->multiexp_parts ? ((k % c->multiexp_parts == 0) ? c->multiexp_parts : 1u) : ((k >= 32 && k % 4 == 0) ? 4u : 1u);
  if (!c->multiexp_parts) {
    // SMALL calls (a lone DistSign, a micro-batch of a few dozen): the call lasts as long as one wave's chain of dependent products
    // whatever the instruction count, so the bases are spread over as many quad groups as still get a SIMD each -- k = 8 bases on 8
    // groups: 15 + 256 + 64 products per group, 8 to multiply the partial products up, instead of 120 + 256 + 512 in one chain.
    for (uint32_t pp = k; pp > parts; --pp)
      if (k % pp == 0 && lanes_wide(c, 0, (uint64_t)n_ops * pp)) { parts = pp; break; }      // (eight lanes each, one wave per SIMD)
  }
  // exponents are residues mod q: qbytes * 2 four-bit windows
  const uint32_t ew = qbytes * 2;
  auto multiexp = [&](uint32_t ops, uint32_t kb, const uint32_t* bases, const uint32_t* exps, uint32_t* out, uint32_t div) {
    if (lanes_wide(c, c->multiexp_lanes, ops))
      hipLaunchKernelGGL((k_multiexp<MULTI_L8, MULTI_TPI8>), dim3((ops + RSA_BLOCK / MULTI_TPI8 - 1) / (RSA_BLOCK / MULTI_TPI8)), dim3(RSA_BLOCK), 0, s,
                         ops, kb, bases, exps, d_gi, mp, (uint32_t*)d_scr, out, div, ew);
    else if (c->multiexp_block == 64)
      hipLaunchKernelGGL((k_multiexp<MONT_L, MONT_TPI, 64>), dim3((ops + 15) / 16), dim3(64), 0, s, ops, kb, bases, exps, d_gi, mp, (uint32_t*)d_scr, out,
                         div, ew);
    else
      hipLaunchKernelGGL((k_multiexp<MONT_L, MONT_TPI>), quad_grid(ops), dim3(RSA_BLOCK), 0, s, ops, kb, bases, exps, d_gi, mp, (uint32_t*)d_scr, out,
                         div, ew);
  };
  if (parts == 1) {
    multiexp(n_ops, k, d_ri, (uint32_t*)d_lam, (uint32_t*)d_prod, 1u);
  } else {
    void* d_part;
    if ((rc = dev_alloc(c, sb, (size_t)n_ops * parts * MONT_N * 4, &d_part, false))) return rc;
    multiexp(n_ops * parts, k / parts, d_ri, (uint32_t*)d_lam, (uint32_t*)d_part, parts);
    hipLaunchKernelGGL(k_modmul_product, quad_grid(n_ops), dim3(RSA_BLOCK), 0, s, n_ops, parts, (uint32_t*)d_part, d_gi, mp, (uint32_t*)d_prod);
  }
  // v^-1 mod q, then (prod)^(v^-1) mod p, then mod q
  hipLaunchKernelGGL(k_u256_inv_modq, dim3((n_ops + 63) / 64), dim3(64), 0, s, n_ops, (const uint32_t*)d_v, (const uint32_t*)d_gi, mq, (uint32_t*)d_vinv, (uint8_t*)d_st,
                     (const uint8_t*)nullptr, (const uint8_t*)nullptr);
  multiexp(n_ops, 1u, (uint32_t*)d_prod, (uint32_t*)d_vinv, (uint32_t*)d_r, 1u);
  hipLaunchKernelGGL(k_limbs_mod_q, quad_grid(n_ops), dim3(RSA_BLOCK), 0, s, n_ops, (uint32_t*)d_r, d_gi, mq, (uint32_t*)d_rq);
  if ((rc = from_dev_limbs(c, sb, (uint32_t*)d_rq, n_ops, qbytes, r_out, dev))) return rc;
  if ((rc = copy_status(c, status_out, d_st, n_ops, dev))) return rc;
  return finish(c, dev);
}

int sss_distribute_impl(bftkv_gpu_ctx* c, uint32_t n_polys, uint32_t n_shares, uint32_t k, const uint8_t* coeffs, uint32_t nbytes,
                        const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods, uint8_t* shares_out, bool dev) {
  if (!c || nbytes == 0 || nbytes > 256 || k == 0 || n_shares == 0 || n_mods == 0 || (n_polys && (!coeffs || (!mod_idx && !dev) || !mods || !shares_out)))
    return BFTKV_E_INVALID;
  if (n_polys == 0) return 0;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mt;
  int rc;
  uint32_t *d_p, *d_mi;
  void* d_out;
  const uint32_t n_ops = n_polys * n_shares;
  if ((rc = make_modtab(c, sb, mods, n_mods, nbytes, &mt))) return rc;
  if ((rc = idx_to_dev(c, sb, mod_idx, n_polys, n_mods, &d_mi, dev))) return rc;
  if ((rc = to_dev_limbs(c, sb, coeffs, (size_t)n_polys * k, nbytes, &d_p, dev))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_out, false))) return rc;
  hipLaunchKernelGGL(k_sss_distribute, quad_grid(n_ops), dim3(RSA_BLOCK), 0, c->stream, n_ops, n_shares, k, d_p, d_mi, mt, (uint32_t*)d_out);
  if ((rc = from_dev_limbs(c, sb, (uint32_t*)d_out, n_ops, nbytes, shares_out, dev))) return rc;
  return finish(c, dev);
}

int modinv_impl(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* values, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods,
                const uint8_t* mods, uint8_t* out, uint8_t* status_out, bool dev) {
  if (!c || nbytes == 0 || nbytes > 256 || n_mods == 0 || (n_ops && (!values || (!mod_idx && !dev) || !mods || !out))) return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mt;
  int rc;
  uint32_t *d_v, *d_mi;
  void *d_out, *d_st;
  if ((rc = make_modtab(c, sb, mods, n_mods, nbytes, &mt))) return rc;
  if ((rc = idx_to_dev(c, sb, mod_idx, n_ops, n_mods, &d_mi, dev))) return rc;
  if ((rc = to_dev_limbs(c, sb, values, n_ops, nbytes, &d_v, dev))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_out, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops + 8, &d_st, true))) return rc;
  hipLaunchKernelGGL(k_modinv, dim3((n_ops + 63) / 64), dim3(64), 0, c->stream, n_ops, (const uint32_t*)d_v, (const uint32_t*)d_mi, mt, (uint32_t*)d_out, (uint8_t*)d_st,
                     (const uint8_t*)nullptr, (const uint8_t*)nullptr);
  if ((rc = from_dev_limbs(c, sb, (uint32_t*)d_out, n_ops, nbytes, out, dev))) return rc;
  if ((rc = copy_status(c, status_out, d_st, n_ops, dev))) return rc;
  return finish(c, dev);
}

// b^x mod n, one exponent per modulus (threshold-RSA key fragments) or per operation (CalculatePartialR).  Exponents travel as
// little-endian 32-bit words; the chain is 2 products per exponent bit of exp_len, whatever the value.
int modexp_impl(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* base, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods,
                const uint8_t* mods, const uint8_t* exps, uint32_t exp_len, bool exp_per_op, uint8_t* out) {
  if (!c || nbytes == 0 || nbytes > 256 || exp_len == 0 || n_mods == 0 || (n_ops && (!base || !mod_idx || !mods || !exps || !out))) return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mt;
  int rc;
  uint32_t *d_b, *d_mi, *d_ex;
  void* d_out;
  const uint32_t ew = (exp_len + 3) / 4;
  const size_t n_exp = exp_per_op ? n_ops : n_mods;
  std::vector<uint32_t> ex(n_exp * ew, 0);
  for (size_t m = 0; m < n_exp; ++m) hostbn::from_be(exps + m * exp_len, exp_len, &ex[m * ew], (int)ew);
  if ((rc = make_modtab(c, sb, mods, n_mods, nbytes, &mt))) return rc;
  if ((rc = idx_to_dev(c, sb, mod_idx, n_ops, n_mods, &d_mi, false))) return rc;
  if ((rc = to_dev_limbs(c, sb, base, n_ops, nbytes, &d_b))) return rc;
  if ((rc = to_dev(c, sb, ex.data(), ex.size(), &d_ex))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_out, false))) return rc;
  hipLaunchKernelGGL(k_modexp, quad_grid(n_ops), dim3(RSA_BLOCK), 0, c->stream, n_ops, d_b, d_mi, mt.n_limbs, mt.r2_limbs, mt.n0inv, d_ex, ew,
                     exp_per_op ? 1u : 0u, (uint32_t*)d_out);
  if ((rc = from_dev_limbs(c, sb, (uint32_t*)d_out, n_ops, nbytes, out))) return rc;
  return finish(c, false);     // (the exponent words in `ex` were copied from pageable memory: the copy call returned when it was done)
}

int selftest_reduce_impl(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* values, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods,
                         const uint8_t* mods, uint32_t lanes, uint8_t* out) {
  if (!c || nbytes == 0 || nbytes > 256 || n_mods == 0 || (lanes != 4 && lanes != 8) || (n_ops && (!values || !mod_idx || !mods || !out)))
    return BFTKV_E_INVALID;
  if (n_ops == 0) return 0;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mt;
  int rc;
  uint32_t *d_v, *d_mi;
  void* d_out;
  if ((rc = make_modtab(c, sb, mods, n_mods, nbytes, &mt))) return rc;
  if ((rc = idx_to_dev(c, sb, mod_idx, n_ops, n_mods, &d_mi, false))) return rc;
  if ((rc = to_dev_limbs(c, sb, values, n_ops, nbytes, &d_v, false))) return rc;
  if ((rc = dev_alloc(c, sb, (size_t)n_ops * MONT_N * 4, &d_out, false))) return rc;
  if (lanes == 4)
    hipLaunchKernelGGL((k_reduce_once<MONT_L, MONT_TPI>), quad_grid(n_ops), dim3(RSA_BLOCK), 0, c->stream, n_ops, d_v, d_mi, mt, (uint32_t*)d_out);
  else
    hipLaunchKernelGGL((k_reduce_once<MULTI_L8, MULTI_TPI8>), dim3((n_ops + RSA_BLOCK / MULTI_TPI8 - 1) / (RSA_BLOCK / MULTI_TPI8)), dim3(RSA_BLOCK), 0,
                       c->stream, n_ops, d_v, d_mi, mt, (uint32_t*)d_out);
  if ((rc = from_dev_limbs(c, sb, (uint32_t*)d_out, n_ops, nbytes, out, false))) return rc;
  return finish(c, false);
}

}  // namespace

extern "C" {

int bftkv_gpu_set_lagrange_x_bound(bftkv_gpu_ctx* c, uint32_t bound) {
  if (!c) return BFTKV_E_INVALID;
  ctx_lock lk(c->mu);
  c->lagrange_x_bound = bound;
  return 0;
}

int bftkv_gpu_modexp(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* base, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods,
                     const uint8_t* mods, const uint8_t* exps, uint32_t exp_len, uint8_t* out) {
  return modexp_impl(c, n_ops, base, nbytes, mod_idx, n_mods, mods, exps, exp_len, false, out);
}
int bftkv_gpu_modexp_ops(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* base, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods,
                         const uint8_t* mods, const uint8_t* exps, uint32_t exp_len, uint8_t* out) {
  return modexp_impl(c, n_ops, base, nbytes, mod_idx, n_mods, mods, exps, exp_len, true, out);
}
int bftkv_gpu_selftest_reduce(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* values, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods,
                              const uint8_t* mods, uint32_t lanes, uint8_t* out) {
  return selftest_reduce_impl(c, n_ops, values, nbytes, mod_idx, n_mods, mods, lanes, out);
}

int bftkv_gpu_modmul_product(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const uint8_t* factors, uint32_t nbytes, const uint32_t* mod_idx,
                             uint32_t n_mods, const uint8_t* mods, uint8_t* out) {
  return modmul_product_impl(c, n_ops, k, factors, nbytes, mod_idx, n_mods, mods, out, false);
}
int bftkv_gpu_modmul_product_dev(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const uint8_t* factors, uint32_t nbytes, const uint32_t* mod_idx,
                                 uint32_t n_mods, const uint8_t* mods, uint8_t* out) {
  return modmul_product_impl(c, n_ops, k, factors, nbytes, mod_idx, n_mods, mods, out, true);
}
int bftkv_gpu_lagrange_combine(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ys, uint32_t nbytes,
                               const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods, uint8_t* out, uint8_t* status_out) {
  return lagrange_combine_impl(c, n_ops, k, xs, ys, nbytes, mod_idx, n_mods, mods, out, status_out, false);
}
int bftkv_gpu_lagrange_combine_dev(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ys, uint32_t nbytes,
                                   const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods, uint8_t* out, uint8_t* status_out) {
  return lagrange_combine_impl(c, n_ops, k, xs, ys, nbytes, mod_idx, n_mods, mods, out, status_out, true);
}
int bftkv_gpu_dsa_calculate_r(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ri, uint32_t pbytes,
                              const uint8_t* vi, uint32_t qbytes, const uint32_t* group_idx, uint32_t n_groups, const uint8_t* p,
                              const uint8_t* q, uint8_t* r_out, uint8_t* status_out) {
  return dsa_calculate_r_impl(c, n_ops, k, xs, ri, pbytes, vi, qbytes, group_idx, n_groups, p, q, r_out, status_out, false);
}
int bftkv_gpu_dsa_calculate_r_dev(bftkv_gpu_ctx* c, uint32_t n_ops, uint32_t k, const int32_t* xs, const uint8_t* ri, uint32_t pbytes,
                                  const uint8_t* vi, uint32_t qbytes, const uint32_t* group_idx, uint32_t n_groups, const uint8_t* p,
                                  const uint8_t* q, uint8_t* r_out, uint8_t* status_out) {
  return dsa_calculate_r_impl(c, n_ops, k, xs, ri, pbytes, vi, qbytes, group_idx, n_groups, p, q, r_out, status_out, true);
}
int bftkv_gpu_sss_distribute(bftkv_gpu_ctx* c, uint32_t n_polys, uint32_t n_shares, uint32_t k, const uint8_t* coeffs, uint32_t nbytes,
                             const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods, uint8_t* shares_out) {
  return sss_distribute_impl(c, n_polys, n_shares, k, coeffs, nbytes, mod_idx, n_mods, mods, shares_out, false);
}
int bftkv_gpu_sss_distribute_dev(bftkv_gpu_ctx* c, uint32_t n_polys, uint32_t n_shares, uint32_t k, const uint8_t* coeffs, uint32_t nbytes,
                                 const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods, uint8_t* shares_out) {
  return sss_distribute_impl(c, n_polys, n_shares, k, coeffs, nbytes, mod_idx, n_mods, mods, shares_out, true);
}
int bftkv_gpu_modinv(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* values, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods,
                     const uint8_t* mods, uint8_t* out, uint8_t* status_out) {
  return modinv_impl(c, n_ops, values, nbytes, mod_idx, n_mods, mods, out, status_out, false);
}
int bftkv_gpu_modinv_dev(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* values, uint32_t nbytes, const uint32_t* mod_idx, uint32_t n_mods,
                         const uint8_t* mods, uint8_t* out, uint8_t* status_out) {
  return modinv_impl(c, n_ops, values, nbytes, mod_idx, n_mods, mods, out, status_out, true);
}

}  // extern "C"
