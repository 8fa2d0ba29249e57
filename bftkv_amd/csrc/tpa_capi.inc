// C ABI of the threshold password authentication entries (include/bftkv_gpu.h: bftkv_gpu_tpa_yi / _bi / _ni; tpa_kernels.hip; the
// rules: docs/parity.md, "Password authentication (crypto/auth)").
namespace {

enum class TpaMode { Yi, Bi, Ni };
// chains per launch of k_tpa_pow: bounds the window tables (4.75 KB per quad of a launch) at 304 MB, whatever the call's size
constexpr uint32_t TPA_LAUNCH_CHAINS = 1u << 16;
constexpr uint32_t TPA_MAX_OPS = 1u << 22;      // chains * nbytes stays below 2^32 in the conversion kernels

// The result arrays of a call (host memory).  They fail closed before anything can refuse the call, and again if it fails later.
struct TpaOut {
  uint8_t *num, *keys, *mac, *st;      // [n_ops][nbytes] (yi_out / bi_out), [n_ops][32] twice, [n_ops]; NULL: the entry has none such
  uint32_t n_ops, nbytes;
  void fail_closed() const {
    if (!n_ops || n_ops > TPA_MAX_OPS) return;
    if (st) memset(st, BFTKV_TH_FAILED, n_ops);
    if (num) memset(num, 0, (size_t)n_ops * nbytes);
    if (keys) memset(keys, 0, (size_t)n_ops * 32);
    if (mac) memset(mac, 0, (size_t)n_ops * 32);
  }
};

// what refuses a call whatever its numbers: BFTKV_E_INVALID (the batcher refuses its caller by the same rule)
inline bool tpa_shape_ok(TpaMode mode, uint32_t nbytes, uint32_t exp_len, uint32_t salt_len) {
  return nbytes != 0 && nbytes <= 256 && exp_len != 0 && exp_len <= 256 && (mode == TpaMode::Yi || salt_len <= 64);
}

// Yi: base0 = x, one chain.  Bi: base0 = v and xi, two chains that share the exponent; the finish takes Bi from the first and Ki from
// the second.  Ni: base0 = bi, one chain (Ki); the finish takes Bi.Bytes() from the bytes of `bi` as given.
// Everything between the uploads and the downloads is enqueued on the context's stream: the host waits once, at the end.
int tpa_run(bftkv_gpu_ctx* c, TpaMode mode, const TpaOut& o, const uint8_t* base0, const uint8_t* xi, const uint32_t* xi_len, const uint8_t* exps,
            uint32_t exp_len, const uint8_t* salt, uint32_t salt_len, const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods) {
  const uint32_t n_ops = o.n_ops, nbytes = o.nbytes;
  const uint32_t chains = mode == TpaMode::Bi ? 2 * n_ops : n_ops;
  ctx_lock lk(c->mu);
  HIPCHK(c, hipSetDevice(c->device));
  ScratchBufs sb(c);
  { int grc = modtab_gc(c); if (grc) return grc; }
  ModTab mt;
  int rc;
  if ((rc = make_modtab(c, sb, mods, n_mods, nbytes, &mt))) return rc;
  std::vector<uint32_t> idx(n_ops, 0u);
  if (mod_idx) for (uint32_t i = 0; i < n_ops; ++i) idx[i] = std::min(mod_idx[i], n_mods - 1u);
  hipStream_t s = c->stream;
  uint32_t *d_mi, *d_xl = nullptr;
  uint8_t *d_b0, *d_ex, *d_xi = nullptr, *d_salt = nullptr;
  void *d_base, *d_out, *d_tab, *d_bytes, *d_keys = nullptr, *d_mac = nullptr;
  if ((rc = to_dev(c, sb, idx.data(), (size_t)n_ops, &d_mi)) || (rc = to_dev(c, sb, base0, (size_t)n_ops * nbytes, &d_b0)) ||
      (rc = to_dev(c, sb, exps, (size_t)n_ops * exp_len, &d_ex)))
    return rc;
  if (mode != TpaMode::Yi) {
    if ((rc = to_dev(c, sb, xi, (size_t)n_ops * nbytes, &d_xi)) || (rc = to_dev(c, sb, xi_len, (size_t)n_ops, &d_xl))) return rc;
    if (salt_len && (rc = to_dev(c, sb, salt, (size_t)n_ops * salt_len, &d_salt))) return rc;
    if ((rc = dev_alloc(c, sb, (size_t)n_ops * 32, &d_keys, false)) || (rc = dev_alloc(c, sb, (size_t)n_ops * 32, &d_mac, false))) return rc;
  }
  const uint32_t per_launch = std::min(chains, TPA_LAUNCH_CHAINS);
  const size_t tab_quads = (size_t)quad_grid(per_launch).x * QUADS_PER_BLOCK;
  if ((rc = dev_alloc(c, sb, (size_t)chains * MONT_N * 4, &d_base, false)) || (rc = dev_alloc(c, sb, (size_t)chains * MONT_N * 4, &d_out, false)) ||
      (rc = dev_alloc(c, sb, tab_quads * CHAIN_ENT * MONT_N * 4, &d_tab, false)) || (rc = dev_alloc(c, sb, (size_t)chains * nbytes, &d_bytes, false)))
    return rc;
  const dim3 limb_grid((uint32_t)(((size_t)n_ops * MONT_N + 255) / 256));
  hipLaunchKernelGGL(k_tpa_bytes_to_limbs, limb_grid, dim3(256), 0, s, (const uint8_t*)d_b0, nbytes, (const uint32_t*)nullptr, n_ops, (uint32_t*)d_base);
  if (mode == TpaMode::Bi)
    hipLaunchKernelGGL(k_tpa_bytes_to_limbs, limb_grid, dim3(256), 0, s, (const uint8_t*)d_xi, nbytes, (const uint32_t*)d_xl, n_ops,
                       (uint32_t*)d_base + (size_t)n_ops * MONT_N);
  for (uint32_t first = 0; first < chains; first += per_launch) {
    const uint32_t n_here = std::min(per_launch, chains - first);
    hipLaunchKernelGGL(k_tpa_pow, quad_grid(n_here), dim3(RSA_BLOCK), 0, s, n_here, first, n_ops, (const uint32_t*)d_base, (const uint8_t*)d_ex, exp_len,
                       (const uint32_t*)d_mi, mt, (uint32_t*)d_tab, (uint32_t*)d_out);
  }
  hipLaunchKernelGGL(k_limbs_to_bytes, dim3((uint32_t)(((size_t)chains * nbytes + 255) / 256)), dim3(256), 0, s, (const uint32_t*)d_out, nbytes, chains,
                     (uint8_t*)d_bytes);
  if (mode != TpaMode::Ni) HIPCHK(c, hipMemcpyAsync(o.num, d_bytes, (size_t)n_ops * nbytes, hipMemcpyDeviceToHost, s));
  if (mode != TpaMode::Yi) {
    const uint8_t* d_ki = (const uint8_t*)d_bytes + (mode == TpaMode::Bi ? (size_t)n_ops * nbytes : 0);
    const uint8_t* d_bi = mode == TpaMode::Bi ? (const uint8_t*)d_bytes : (const uint8_t*)d_b0;
    hipLaunchKernelGGL(k_tpa_finish, dim3((n_ops + 63) / 64), dim3(64), 0, s, n_ops, d_ki, d_bi, nbytes, (const uint8_t*)d_xi, (const uint32_t*)d_xl,
                       (const uint8_t*)d_salt, salt_len, (uint8_t*)d_keys, (uint8_t*)d_mac);
    HIPCHK(c, hipMemcpyAsync(o.keys, d_keys, (size_t)n_ops * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(o.mac, d_mac, (size_t)n_ops * 32, hipMemcpyDeviceToHost, s));
  }
  return finish(c, false);      // (idx was copied from pageable memory: the copy call returned when it was done with it)
}

int tpa_impl(bftkv_gpu_ctx* c, TpaMode mode, uint32_t n_ops, const uint8_t* base0, const uint8_t* xi, const uint32_t* xi_len, uint32_t nbytes,
             const uint8_t* exps, uint32_t exp_len, const uint8_t* salt, uint32_t salt_len, const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods,
             uint8_t* num_out, uint8_t* keys_out, uint8_t* mac_out, uint8_t* status_out) {
  const TpaOut o{num_out, keys_out, mac_out, status_out, n_ops, nbytes};
  o.fail_closed();
  const bool kdf = mode != TpaMode::Yi;
  if (!c || n_ops == 0 || n_ops > TPA_MAX_OPS || n_mods == 0 || !tpa_shape_ok(mode, nbytes, exp_len, salt_len) || !base0 || !exps || !mods || !status_out ||
      (mode != TpaMode::Ni && !num_out) || (kdf && (!xi || !xi_len || !keys_out || !mac_out || (salt_len && !salt))))
    return BFTKV_E_INVALID;
  if (kdf) for (uint32_t i = 0; i < n_ops; ++i) if (xi_len[i] > nbytes) return BFTKV_E_INVALID;
  const int rc = tpa_run(c, mode, o, base0, xi, xi_len, exps, exp_len, salt, salt_len, mod_idx, n_mods, mods);
  if (rc) o.fail_closed();
  else memset(status_out, BFTKV_TH_OK, n_ops);
  return rc;
}

}  // namespace

extern "C" {

int bftkv_gpu_tpa_yi(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* x, uint32_t nbytes, const uint8_t* y, uint32_t exp_len, const uint32_t* mod_idx,
                     uint32_t n_mods, const uint8_t* mods, uint8_t* yi_out, uint8_t* status_out) {
  return tpa_impl(c, TpaMode::Yi, n_ops, x, nullptr, nullptr, nbytes, y, exp_len, nullptr, 0, mod_idx, n_mods, mods, yi_out, nullptr, nullptr, status_out);
}
int bftkv_gpu_tpa_bi(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* v, const uint8_t* xi, const uint32_t* xi_len, uint32_t nbytes, const uint8_t* b,
                     uint32_t exp_len, const uint8_t* salt, uint32_t salt_len, const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods,
                     uint8_t* bi_out, uint8_t* keys_out, uint8_t* mac_out, uint8_t* status_out) {
  return tpa_impl(c, TpaMode::Bi, n_ops, v, xi, xi_len, nbytes, b, exp_len, salt, salt_len, mod_idx, n_mods, mods, bi_out, keys_out, mac_out, status_out);
}
int bftkv_gpu_tpa_ni(bftkv_gpu_ctx* c, uint32_t n_ops, const uint8_t* bi, const uint8_t* xi, const uint32_t* xi_len, uint32_t nbytes, const uint8_t* e,
                     uint32_t exp_len, const uint8_t* salt, uint32_t salt_len, const uint32_t* mod_idx, uint32_t n_mods, const uint8_t* mods,
                     uint8_t* keys_out, uint8_t* mac_out, uint8_t* status_out) {
  return tpa_impl(c, TpaMode::Ni, n_ops, bi, xi, xi_len, nbytes, e, exp_len, salt, salt_len, mod_idx, n_mods, mods, nullptr, keys_out, mac_out, status_out);
}

}  // extern "C"
