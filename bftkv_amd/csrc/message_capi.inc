// Transport message signatures (SURVEY.md 8(f)-2): the signature half of PGPMessage.Decrypt (crypto_pgp.go:453-471), i.e.
// what openpgp.ReadMessage does after the session key has opened the container -- readSignedMessage and the
// signatureCheckReader at the end of the literal body.  Framing (one-pass signature, literal data with definite or
// partial body lengths, the trailing signature) is walked on the host; the hash over the literal body and the RSA / DSA
// verification of every message in the batch run through the same kernels as detached signatures, with the key and the
// hash algorithm taken from the ONE-PASS packet as Go does.  Included by capi.hip.

namespace {

struct MsgChunk { uint64_t off, len; };
struct MsgPacket { uint32_t tag = 0; std::vector<MsgChunk> chunks; uint64_t start = 0, next = 0; bool partial = false; };
enum MsgRead { MR_OK, MR_EOF, MR_ERROR, MR_UNSUPPORTED };

// packet.Read framing with partialLengthReader; offsets are relative to d
MsgRead msg_read_packet(const uint8_t* d, uint64_t pos, uint64_t len, MsgPacket* out) {
  out->chunks.clear(); out->partial = false; out->start = pos;
  if (pos >= len) return MR_EOF;
  const uint32_t b0 = d[pos];
  if (!(b0 & 0x80)) return MR_ERROR;
  if (!(b0 & 0x40)) {                           // old format
    out->tag = (b0 & 0x3F) >> 2;
    const uint32_t lt = b0 & 3;
    if (lt == 3) return MR_UNSUPPORTED;         // indeterminate length: fenced
    const uint32_t nb = 1u << lt;
    if (pos + 1 + nb > len) return MR_ERROR;
    uint64_t ln = 0;
    for (uint32_t i = 0; i < nb; ++i) ln = (ln << 8) | d[pos + 1 + i];
    if (pos + 1 + nb + ln > len) return MR_ERROR;
    out->chunks.push_back({pos + 1 + nb, ln});
    out->next = pos + 1 + nb + ln;
    return MR_OK;
  }
  out->tag = b0 & 0x3F;
  uint64_t p = pos + 1;
  for (;;) {
    if (p >= len) return MR_ERROR;
    const uint32_t b1 = d[p];
    uint64_t ln;
    bool last = true;
    if (b1 < 192) { ln = b1; p += 1; }
    else if (b1 < 224) { if (p + 1 >= len) return MR_ERROR; ln = ((uint64_t)(b1 - 192) << 8) + d[p + 1] + 192; p += 2; }
    else if (b1 == 255) {
      if (p + 5 > len) return MR_ERROR;
      ln = ((uint64_t)d[p + 1] << 24) | ((uint64_t)d[p + 2] << 16) | ((uint64_t)d[p + 3] << 8) | d[p + 4];
      p += 5;
    } else { ln = 1ull << (b1 & 0x1F); p += 1; last = false; out->partial = true; }
    if (p + ln > len) return MR_ERROR;
    out->chunks.push_back({p, ln});
    p += ln;
    if (last) { out->next = p; return MR_OK; }
  }
}

bool msg_known_tag(uint32_t t) {   // packet types packet.Read constructs; the rest is skipped by Reader.Next
  switch (t) { case 1: case 2: case 3: case 4: case 5: case 6: case 7: case 8: case 9: case 11: case 13: case 14: case 17: case 18: return true; }
  return false;
}

uint64_t msg_body_len(const MsgPacket& p) { uint64_t n = 0; for (auto& c : p.chunks) n += c.len; return n; }
void msg_body_copy(const uint8_t* d, const MsgPacket& p, uint64_t skip, std::string* out) {
  for (auto& c : p.chunks) {
    if (skip >= c.len) { skip -= c.len; continue; }
    out->append((const char*)d + c.off + skip, c.len - skip);
    skip = 0;
  }
}
uint8_t msg_body_byte(const uint8_t* d, const MsgPacket& p, uint64_t i) {
  for (auto& c : p.chunks) { if (i < c.len) return d[c.off + i]; i -= c.len; }
  return 0;
}

}  // namespace

namespace {

// One message: the walk of readSignedMessage + signatureCheckReader up to the point where a key is needed.
struct MsgFrame {
  uint8_t st = BFTKV_MSG_READ_ERROR;   // BFTKV_MSG_* or 0xFF = "trailing signature packet found: verify it"
  bool have_ops = false, have_lit = false;
  uint64_t signer = 0;
  uint8_t ops_hash = 0;
  uint32_t fname_len = 0;
  uint8_t fname[256];
  uint64_t sig_off = 0, sig_len = 0;
};

// plain receives the literal body.  `want_signature` = false skips the search for the trailing signature (the caller
// already knows that no key can verify it: Go does not wrap the body reader then).
void msg_frame(const uint8_t* d, uint64_t len, std::string* plain, MsgFrame* f, bool stop_after_literal) {
  uint64_t pos = 0;
  MsgPacket pk;
  f->st = BFTKV_MSG_READ_ERROR;
  for (;;) {                                                          // FindLiteralData
    const MsgRead r = msg_read_packet(d, pos, len, &pk);
    if (r == MR_UNSUPPORTED) { f->st = BFTKV_MSG_UNSUPPORTED; return; }
    if (r != MR_OK) { f->st = BFTKV_MSG_READ_ERROR; return; }         // io.EOF before the literal included
    pos = pk.next;
    if (pk.tag == 8) { f->st = BFTKV_MSG_UNSUPPORTED; return; }       // compressed data: fenced
    if (pk.tag == 4) {                                                // OnePassSignature.parse
      const uint64_t bl = msg_body_len(pk);
      if (bl < 13 || msg_body_byte(d, pk, 0) != 3) { f->st = BFTKV_MSG_READ_ERROR; return; }
      const uint8_t sig_type = msg_body_byte(d, pk, 1), hid = msg_body_byte(d, pk, 2);
      const bool known = hid == HASH_MD5 || hid == HASH_SHA1 || hid == HASH_RIPEMD160 || hid == HASH_SHA256 || hid == HASH_SHA384 ||
                         hid == HASH_SHA512 || hid == HASH_SHA224;
      if (!known) { f->st = BFTKV_MSG_READ_ERROR; return; }
      if (f->have_ops) { f->st = BFTKV_MSG_UNSUPPORTED; return; }      // several one-pass packets: fenced
      if (msg_body_byte(d, pk, 12) == 0) { f->st = BFTKV_MSG_READ_ERROR; return; }   // nested signatures
      if (hid == HASH_MD5 || hid == HASH_RIPEMD160) { f->st = BFTKV_MSG_UNSUPPORTED; return; }
      if (sig_type == 0x01) { f->st = BFTKV_MSG_UNSUPPORTED; return; }  // canonical text: fenced
      if (sig_type != 0x00) { f->st = BFTKV_MSG_READ_ERROR; return; }
      f->have_ops = true; f->ops_hash = hid;
      f->signer = 0;
      for (int k = 0; k < 8; ++k) f->signer = (f->signer << 8) | msg_body_byte(d, pk, 4 + k);
      continue;
    }
    if (pk.tag == 11) {                                               // LiteralData.parse
      const uint64_t bl = msg_body_len(pk);
      if (bl < 2) { f->st = BFTKV_MSG_READ_ERROR; return; }
      const uint32_t fl = msg_body_byte(d, pk, 1);
      if (bl < 2ull + fl + 4) { f->st = BFTKV_MSG_READ_ERROR; return; }
      f->fname_len = fl;
      for (uint32_t k = 0; k < fl; ++k) f->fname[k] = msg_body_byte(d, pk, 2 + k);
      msg_body_copy(d, pk, 2ull + fl + 4, plain);
      f->have_lit = true;
      break;
    }
    // other known packets fall through Go's type switch; unknown ones are skipped by Reader.Next
  }
  if (!f->have_ops) { f->st = BFTKV_MSG_NOT_SIGNED; return; }
  if (stop_after_literal) { f->st = BFTKV_MSG_UNVERIFIED; return; }
  // signatureCheckReader at the end of the body: the next packet Reader.Next yields must be a signature
  f->st = BFTKV_MSG_SIGNATURE_ERROR;
  for (;;) {
    const MsgRead r = msg_read_packet(d, pos, len, &pk);
    if (r == MR_UNSUPPORTED) { f->st = BFTKV_MSG_UNSUPPORTED; return; }
    if (r != MR_OK) return;                                           // SignatureError = the read error (io.EOF included)
    pos = pk.next;
    if (pk.tag != 2 && !msg_known_tag(pk.tag)) continue;
    if (pk.tag != 2) return;                                          // "LiteralData not followed by signature"
    if (pk.partial) { f->st = BFTKV_MSG_UNSUPPORTED; return; }        // partial-length signature packet: fenced
    f->st = 0xFF;
    f->sig_off = pk.start; f->sig_len = pk.next - pk.start;
    return;
  }
}

}  // namespace

extern "C" int bftkv_host_message_frame(const uint8_t* msg, uint64_t len, uint8_t* framing_out, uint64_t* signer_out, uint8_t* hash_out,
                                        uint8_t* plain_out, uint64_t plain_cap, uint64_t* plain_len_out, uint8_t* fname_out,
                                        uint8_t* fname_len_out, uint64_t* sig_off_out, uint64_t* sig_len_out) {
  if ((!msg && len) || !framing_out) return BFTKV_E_INVALID;
  std::string plain;
  MsgFrame f;
  msg_frame(msg, len, &plain, &f, false);
  *framing_out = f.st;
  if (signer_out) *signer_out = f.have_lit ? f.signer : 0;
  if (hash_out) *hash_out = f.ops_hash;
  if (plain_len_out) *plain_len_out = plain.size();
  if (plain_out) {
    if (plain.size() > plain_cap) return BFTKV_E_NOMEM;
    if (!plain.empty()) memcpy(plain_out, plain.data(), plain.size());
  }
  if (fname_len_out) *fname_len_out = f.have_lit ? (uint8_t)f.fname_len : 0;
  if (fname_out && f.have_lit) memcpy(fname_out, f.fname, f.fname_len);
  if (sig_off_out) *sig_off_out = f.sig_off;
  if (sig_len_out) *sig_len_out = f.sig_len;
  return 0;
}

extern "C" int bftkv_gpu_message_verify(bftkv_gpu_ctx* c, uint32_t n_msgs, const uint8_t* msgs, const uint64_t* msg_off, uint8_t* status_out,
                                        uint64_t* signer_key_id_out, uint64_t* peer_id_out, uint8_t* plain_out, uint64_t plain_cap,
                                        uint64_t* plain_off_out, uint8_t* fname_out, uint8_t* fname_len_out) {
  if (!c || (n_msgs && (!msg_off || !status_out))) return BFTKV_E_INVALID;
  if (n_msgs == 0) { if (plain_off_out) plain_off_out[0] = 0; return 0; }
  if (msg_off[0] != 0) return fail(c, BFTKV_E_INVALID, "msg_off not monotone from 0");
  for (uint32_t i = 0; i < n_msgs; ++i) if (msg_off[i + 1] < msg_off[i]) return fail(c, BFTKV_E_INVALID, "msg_off not monotone from 0");
  // a forked context: its lock and the root's key table are held for the whole call (a root context frames the messages
  // outside its lock, so that callers sharing it overlap their host work)
  std::unique_lock<std::recursive_mutex> fork_lk;
  if (c->root) fork_lk = std::unique_lock<std::recursive_mutex>(c->mu);
  KtRead kr(c);
  if (kr.rc) return kr.rc;
  // key table snapshot: KeysByIdUsage(id, KeyFlagSign)[0] and getCertById(id)
  std::vector<uint64_t> key_id;
  std::vector<uint8_t> key_flags;
  {
    ctx_lock lk(c->mu);
    key_id = c->h_key_id; key_flags = c->h_key_flags;
  }
  std::string plain, sigs;
  std::vector<uint64_t> plain_off(n_msgs + 1, 0), v_tbs_off{0}, v_sig_off{0};
  std::vector<uint32_t> v_slot, v_msg;   // device items: key slot, message index
  std::vector<uint8_t> v_hash;
  std::string tbs;
  for (uint32_t i = 0; i < n_msgs; ++i) {
    const uint8_t* d = msgs + msg_off[i];
    const uint64_t len = msg_off[i + 1] - msg_off[i];
    const size_t plain_start = plain.size();
    MsgFrame f;
    msg_frame(d, len, &plain, &f, false);
    uint64_t peer = 0;
    int32_t slot = -1;
    if (f.have_lit && f.have_ops) {
      // md.SignedBy = KeysByIdUsage(one-pass key id, KeyFlagSign)[0]; peer = getCertById(id) (primary ids only)
      for (size_t k = 0; k < key_id.size(); ++k)
        if (key_id[k] == f.signer && (key_flags[k] & KEYF_USABLE_SIGN) && !(key_flags[k] & KEYF_CERT_ONLY)) { slot = (int32_t)k; break; }
      for (size_t k = 0; k < key_id.size(); ++k)
        if (key_id[k] == f.signer && (key_flags[k] & KEYF_PRIMARY) && !(key_flags[k] & KEYF_CERT_ONLY)) { peer = f.signer; break; }
    }
    uint8_t st = f.st;
    if (f.have_lit && f.have_ops && slot < 0) st = BFTKV_MSG_UNVERIFIED;     // the body reader is not wrapped: no signature check at all
    else if (st == 0xFF) {
      sigs.append((const char*)d + f.sig_off, f.sig_len);
      v_sig_off.push_back(sigs.size());
      tbs.append(plain, plain_start, std::string::npos);
      v_tbs_off.push_back(tbs.size());
      v_slot.push_back((uint32_t)slot); v_hash.push_back(f.ops_hash); v_msg.push_back(i);
    }
    if (fname_len_out) fname_len_out[i] = f.have_lit ? (uint8_t)f.fname_len : 0;
    if (fname_out && f.have_lit) memcpy(fname_out + (size_t)i * 256, f.fname, f.fname_len);
    status_out[i] = st;
    if (signer_key_id_out) signer_key_id_out[i] = f.have_lit ? f.signer : 0;
    if (peer_id_out) peer_id_out[i] = f.have_lit ? peer : 0;
    plain_off[i + 1] = plain.size();
  }
  if (plain_off_out) memcpy(plain_off_out, plain_off.data(), sizeof(uint64_t) * (n_msgs + 1));
  if (plain_out) {
    if (plain.size() > plain_cap) return fail(c, BFTKV_E_NOMEM, "plain_out too small");
    if (!plain.empty()) memcpy(plain_out, plain.data(), plain.size());
  }
  const uint32_t n_items = (uint32_t)v_slot.size();
  if (n_items == 0) return 0;
  std::vector<uint8_t> st(n_items, 0), fz(n_items, 0);
  {
    ctx_lock lk(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->h_key_id != key_id) return fail(c, BFTKV_E_STATE, "keyring changed during bftkv_gpu_message_verify");
    HIPCHK(c, c->in_tbs.ensure(tbs.size() + 64));
    HIPCHK(c, c->in_ss.ensure(sigs.size() + 64));
    HIPCHK(c, c->in_tbs_off.ensure(sizeof(uint64_t) * (n_items + 1)));
    HIPCHK(c, c->in_ss_off.ensure(sizeof(uint64_t) * (n_items + 1)));
    HIPCHK(c, c->cert_ent.ensure(sizeof(uint32_t) * n_items));
    HIPCHK(c, c->sig_class.ensure(n_items + 16));
    hipStream_t s = c->stream;
    if (!tbs.empty()) HIPCHK(c, hipMemcpyAsync(c->in_tbs.p, tbs.data(), tbs.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->in_ss.p, sigs.data(), sigs.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->in_tbs_off.p, v_tbs_off.data(), sizeof(uint64_t) * (n_items + 1), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->in_ss_off.p, v_sig_off.data(), sizeof(uint64_t) * (n_items + 1), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->cert_ent.p, v_slot.data(), sizeof(uint32_t) * n_items, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->sig_class.p, v_hash.data(), n_items, hipMemcpyHostToDevice, s));
    PipelineCall call;
    call.n_items = n_items; call.d_tbs = c->in_tbs.as<uint8_t>(); call.d_tbs_off = c->in_tbs_off.as<uint64_t>();
    call.d_ss = c->in_ss.as<uint8_t>(); call.d_ss_off = c->in_ss_off.as<uint64_t>();
    // (the certificate calls' buffers, reused: a message call has neither an entity nor a signature class per item)
    call.d_msg_slot = c->cert_ent.as<uint32_t>(); call.d_msg_hash = c->sig_class.as<uint8_t>();
    int rc = run_pipeline(c, call);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev[4], s));
    c->have_timing = true;
    // exactly one packet per item: its status is the item's
    const uint32_t n = c->last_total;
    if (n != n_items) return fail(c, BFTKV_E_DEVICE, "message signature walk produced an unexpected packet count");
    HIPCHK(c, c->st_tmp.ensure(n));
    HIPCHK(c, c->item_tmp.ensure(sizeof(uint32_t) * n));
    hipLaunchKernelGGL(k_export_status, dim3((n + 255) / 256), dim3(256), 0, s, c->recs.as<SigRec>(), n, c->st_tmp.as<uint8_t>(),
                       c->item_tmp.as<uint32_t>());
    HIPCHK(c, hipMemcpyAsync(st.data(), c->st_tmp.p, n, hipMemcpyDeviceToHost, s));
    // fenced shapes keep various statuses (a signature value wider than the kernels take: ST_BAD_SIG; embedded signatures nested
    // too deep: ST_PARSE_ERROR; key shapes outside the kernels ...): the item's fence flag decides, not the status
    HIPCHK(c, c->o_fenced.ensure(n_items));
    hipLaunchKernelGGL(k_fenced_out, dim3((n_items + 255) / 256), dim3(256), 0, s, c->item_flags.as<uint8_t>(), c->hash_mask.as<uint32_t>(), n_items,
                       c->o_fenced.as<uint8_t>(), 0u);
    HIPCHK(c, hipMemcpyAsync(fz.data(), c->o_fenced.p, n_items, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
  }
  for (uint32_t k = 0; k < n_items; ++k)
    status_out[v_msg[k]] = (fz[k] || st[k] == ST_UNSUPPORTED) ? BFTKV_MSG_UNSUPPORTED : st[k] == ST_OK ? BFTKV_MSG_OK : BFTKV_MSG_SIGNATURE_ERROR;
  return 0;
}
