"""The characters of the call-order tests (tests/test_state_reference.py asserts what they claim on the CPU,
tests/test_gpu_call_order.py runs them on the device in the orders that could hurt).  Not collected.

A character is a small, seeded, cached input of ONE entry point with its reference answer.  The pipeline characters all verify
under one keyring and one quorum (ring()), so a pair of them needs no keyring_set in between; the others come as good / bad inputs
of one shape per entry at 70 and 141 operations (more than one wave; 70 % 4 = 2 and 141 % 4 = 1, so the last packed status word is
partly dead).  References are the oracle's (oracle/collective.py, oracle/threshold.py) or the restatements the tests of each entry
already use (tests/*_ref.py)."""
from __future__ import annotations

import functools
import hashlib
import struct
from collections import namedtuple

import numpy as np

from corpus import build as cb
from corpus.keys import DRBG, load_keys
from oracle import collective as col
from oracle import openpgp as pgp
from oracle import threshold as T
from oracle import wotqs
from oracle.packet import SignaturePacket
from tests import helpers as H

WALK_CAP_MAX = 320            # kernels.hip: the longest per-item scratch row of the packet walk
RSA29_CAP_BYTES = 261         # kernels.hip: RSA values longer than this under a <= 2048-bit key are SIGF_WIDE_VALUE
N_ITEMS = 24                  # two blocks of the planning kernel (16 items each)
V_IS_QUORUM, V_IS_THRESHOLD, V_IS_SUFFICIENT, V_REJECT = 1, 2, 4, 8
ERR_INVALID, ERR_INSUFFICIENT = 1, 2
SIZES = (70, 141)


# ================================================================================================================================
# the pipeline characters
# ================================================================================================================================
Ring = namedtuple("Ring", "cluster rsa3072 rsa4096 dsa2048 dsa3072 keyring quorum")
Call = namedtuple("Call", "tbs ss")                       # per item: the signed payload and the signature stream
Ref = namedtuple("Ref", "err nver verdict fenced statuses sig_err")
"""Per item of one call: CollectiveSignature.Verify's error byte, len(verified) and the predicate bits of the verified signers at the
exit; the fence flag the construction fixes; the per-packet statuses of everything the reference consumed; Signature.Verify's error
byte.  Where fenced[i] is 1 the reference's columns are what the restatement gives on those bytes and no test compares them."""
Character = namedtuple("Character", "name calls refs")


def _extra_key(kind, idx, name, rng):
    kp = cb.make_keypair(cb.PK_RSA if kind.startswith("rsa") else cb.PK_DSA, load_keys(kind, idx + 1)[idx], name)
    cb.build_entity(kp, [], rng)
    return kp


@functools.lru_cache(maxsize=None)
def ring() -> Ring:
    """RSA-2048 members of a 13-replica clique (f = 4, suff = 9) -- the quorum --, and in the same keyring one RSA-3072 key, one
    RSA-4096 key and DSA keys of both size classes (2048/256 and 3072/256), which sign but are no members."""
    cl = cb.make_cluster(13)
    rng = DRBG("state-ring")
    extra = [_extra_key("rsa3072", 0, "big3072 <k@bftkv.example>", rng), _extra_key("rsa4096", 0, "big4096 <k@bftkv.example>", rng),
             _extra_key("dsa2048", 0, "dsa2048-0 <k@bftkv.example>", rng), _extra_key("dsa2048", 1, "dsa2048-1 <k@bftkv.example>", rng),
             _extra_key("dsa3072", 0, "dsa3072-0 <k@bftkv.example>", rng), _extra_key("dsa3072", 1, "dsa3072-1 <k@bftkv.example>", rng)]
    ents = H.oracle_keyring(cl).keyring + [pgp.read_entities(k.entity)[0] for k in extra]
    return Ring(cl, extra[0], extra[1], extra[2:4], extra[4:6], col.Keyring(keyring=ents), H.clique_quorum(cl))


def sign_v4(kp, payload: bytes, hash_id: int = cb.HASH_SHA256, sig_type: int = 0, srng=None) -> bytes:
    """One v4 signature BODY by an RSA key of any size or a DSA key, over any of the five hashes, binary (0x00) or text mode (0x01)."""
    prefix = cb.sig_prefix(sig_type, kp.algo, cb._hashed_area(kp.key_id), hash_id)
    name = cb.HASH_NAMES[hash_id]
    if sig_type == 1:
        h = pgp.CanonicalTextHash(hashlib.new(name))
        h.update(payload)
        h.raw_update(cb.hash_suffix(prefix))
    else:
        h = hashlib.new(name, payload + cb.hash_suffix(prefix))
    digest = h.digest()
    if kp.algo == cb.PK_RSA:
        k = (kp.n.bit_length() + 7) // 8
        t = pgp.HASH_PREFIXES[name] + digest
        em = int.from_bytes(b"\x00\x01" + b"\xff" * (k - len(t) - 3) + b"\x00" + t, "big")
        mp = cb.go_mpi_bytes(kp.rsa_private(em).to_bytes(k, "big"))
    else:
        r, s = cb._dsa_sign(kp, digest, srng)
        mp = b"".join(cb.go_mpi_bytes(v.to_bytes((v.bit_length() + 7) // 8, "big")) for v in (r, s))
    return prefix + b"\x00\x00" + digest[:2] + mp


def packet(body: bytes) -> bytes:
    return cb._hdr(2, len(body)) + body


def _split(pkt: bytes):
    """(header length, offset of the hash tag) of a definite-length v4 signature packet"""
    hdr = 6 if pkt[1] == 255 else (3 if pkt[1] >= 192 else 2)
    hl = (pkt[hdr + 4] << 8) | pkt[hdr + 5]
    ul = (pkt[hdr + 6 + hl] << 8) | pkt[hdr + 6 + hl + 1]
    return hdr, hdr + 6 + hl + 2 + ul


def packets_of(stream: bytes):
    out, pos = [], 0
    while pos < len(stream):
        p = pgp.packet_read_stream(stream, pos)
        assert p.kind == "sig" and p.pos > pos
        out.append(stream[pos:p.pos])
        pos = p.pos
    return out


def count_events(stream: bytes) -> int:
    """packet.Read calls the reference's reader makes on the stream (the end of the stream not counted)"""
    n, pos = 0, 0
    while True:
        p = pgp.packet_read_stream(stream, pos)
        if p.kind == "eof" or p.pos <= pos:
            return n
        n, pos = n + 1, p.pos


def verdict_bits(q: wotqs.WotQ, nodes) -> int:
    return ((V_IS_QUORUM if q.is_quorum(nodes) else 0) | (V_IS_THRESHOLD if q.is_threshold(nodes) else 0) |
            (V_IS_SUFFICIENT if q.is_sufficient(nodes) else 0) | (V_REJECT if q.reject(nodes) else 0))


def reference(call: Call, kr: col.Keyring, q: wotqs.WotQ, fenced=None) -> Ref:
    n = len(call.tbs)
    err, nver, verdict, sig_err = (np.zeros(n, dtype=t) for t in (np.uint8, np.uint32, np.uint8, np.uint8))
    statuses = []
    for i, (tbs, ss) in enumerate(zip(call.tbs, call.ss)):
        r = col.collective_verify(kr, tbs, SignaturePacket(Type=1, Data=ss or None), q)
        err[i] = 0 if r.err is None else ERR_INSUFFICIENT
        nver[i] = len(r.verified)
        verdict[i] = verdict_bits(q, r.verified)
        statuses.append(list(r.statuses))
        sig_err[i] = 0 if col.signature_verify(kr, tbs, SignaturePacket(1, 0, False, ss or None, None)) is None else ERR_INVALID
    return Ref(err, nver, verdict, np.zeros(n, dtype=np.uint8) if fenced is None else np.array(fenced, dtype=np.uint8), statuses, sig_err)


def _payload(rng, i):
    return cb.serialize_tbs(b"state%04d" % i, rng.bytes(int(rng.integers(1, 160))), 1 + i)


def _members(rng, k):
    return [ring().cluster.replicas[int(j)] for j in rng.permutation(13)[:k]]


@functools.lru_cache(maxsize=None)
def _plain_call() -> Call:
    """binary SHA-256 signatures by 9 .. 13 distinct members: every item sufficient"""
    rng = np.random.default_rng(4801)
    tbs, ss = [], []
    for i in range(N_ITEMS):
        t = _payload(rng, i)
        tbs.append(t)
        ss.append(b"".join(cb.detach_sign(kp, t) for kp in _members(rng, int(rng.integers(9, 14)))))
    return Call(tbs, ss)


def refuse(pkt: bytes, how: int, tbs: bytes) -> bytes:
    """how: 0 a bad value, 1 a wrong hash tag, 2 an unknown issuer (signed afresh by an outsider), 3 a hash id nobody knows"""
    b = bytearray(pkt)
    hdr, tag_at = _split(pkt)
    if how == 0:
        b[-3] ^= 0x10
    elif how == 1:
        b[tag_at] ^= 0x40
    elif how == 2:
        return cb.detach_sign(ring().cluster.outsiders[len(pkt) % 2], tbs)
    else:
        b[hdr + 3] = 99                                     # RFC 4880 9.4 names no such hash
    return bytes(b)


def _all_bad_call() -> Call:
    """the items of `plain`, every packet refused: the four refusals dealt round-robin"""
    p = _plain_call()
    ss, k = [], 0
    for t, s in zip(p.tbs, p.ss):
        out = []
        for pkt in packets_of(s):
            out.append(refuse(pkt, k % 4, t))
            k += 1
        ss.append(b"".join(out))
    return Call(list(p.tbs), ss)


OTHER_HASHES = ((2, 0), (11, 0), (9, 0), (10, 0), (8, 1), (2, 1), (10, 1), (11, 1))      # (hash id, signature type)


def _other_hashes_call() -> Call:
    """Eight valid signatures per item -- SHA-1 / 224 / 384 / 512 in binary mode, SHA-256 / SHA-1 / 512 / 224 in text mode, over
    payloads full of line ends -- and one corrupted one: one short of the quorum, so the error byte is `plain`'s complement while
    every one of the eight must be verified for n_verified to be right."""
    rng = np.random.default_rng(4802)
    alphabet = np.frombuffer(b"\r\n\r\nab \t", dtype=np.uint8)
    tbs, ss = [], []
    for i in range(N_ITEMS):
        t = alphabet[rng.integers(0, len(alphabet), int(rng.integers(1, 200)))].tobytes()
        ms = _members(rng, 9)
        pk = [packet(sign_v4(kp, t, *OTHER_HASHES[(i + j) % 8])) for j, kp in enumerate(ms[:8])]
        pk.insert(int(rng.integers(0, 9)), refuse(packet(sign_v4(ms[8], t, 10, 0)), 0, t))
        tbs.append(t)
        ss.append(b"".join(pk))
    return Call(tbs, ss)


WIDE_LENGTHS = (262, 263, 264, 265, 266)


def widen(pkt: bytes, kp, nbytes: int) -> bytes:
    """the same signature with s + m n in place of s, m such that the value has exactly nbytes bytes (Go <= 1.13 reduces it)"""
    hdr, tag_at = _split(pkt)
    s = int.from_bytes(pkt[tag_at + 4:], "big")
    big = s + kp.n * ((1 << (8 * (nbytes - 1))) // kp.n + 1)
    assert (big.bit_length() + 7) // 8 == nbytes
    body = pkt[hdr:tag_at + 2] + big.bit_length().to_bytes(2, "big") + big.to_bytes(nbytes, "big")
    return packet(body)


def _wide_call() -> Call:
    """eight valid signatures per item whose values are 262 .. 266 bytes long under 2048-bit keys, and a ninth, corrupted wide one"""
    rng = np.random.default_rng(4803)
    tbs, ss = [], []
    for i in range(N_ITEMS):
        t = _payload(rng, i)
        ms = _members(rng, 9)
        pk = [widen(cb.detach_sign(kp, t), kp, WIDE_LENGTHS[(i + j) % 5]) for j, kp in enumerate(ms)]
        j = int(rng.integers(0, 9))
        pk[j] = refuse(pk[j], 0, t)
        tbs.append(t)
        ss.append(b"".join(pk))
    return Call(tbs, ss)


def _all_lists_call() -> Call:
    """DSA of both size classes, RSA-3072 and RSA-4096 ahead of nine members' RSA-2048 signatures, shuffled among them so that the
    early exit still finds the quorum only at the last member: four work lists in every item, every item sufficient"""
    R = ring()
    rng = np.random.default_rng(4804)
    srng = DRBG("state-all-lists")
    tbs, ss = [], []
    for i in range(N_ITEMS):
        t = _payload(rng, i)
        others = [cb.detach_sign(R.dsa2048[i % 2], t, srng), cb.detach_sign(R.dsa3072[i % 2], t, srng), cb.detach_sign(R.rsa3072, t),
                  cb.detach_sign(R.rsa4096, t)]
        mem = [cb.detach_sign(kp, t) for kp in _members(rng, 9)]
        head = others + mem[:8]
        order = rng.permutation(len(head))
        tbs.append(t)
        ss.append(b"".join(head[int(o)] for o in order) + mem[8])
    return Call(tbs, ss)


def _partial_call() -> Call:
    """valid signatures in partial body lengths (chunks of 1 .. 512 bytes, every chunk read whole): the chunk arena; sufficient"""
    rng = np.random.default_rng(4805)
    tbs, ss = [], []
    for i in range(N_ITEMS):
        t = _payload(rng, i)
        pk = []
        for j, kp in enumerate(_members(rng, 10)):
            body = sign_v4(kp, t)
            pk.append(H.partial_frame(2, body, rng, max_pow=int(rng.choice([3, 6, 9]))) if (i + j) % 3 else packet(body))
        tbs.append(t)
        ss.append(b"".join(pk))
    return Call(tbs, ss)


def _long_items_call() -> Call:
    """three items of more than WALK_CAP_MAX packet events each: unknown packet types (skipped) between ten members' signatures"""
    rng = np.random.default_rng(4806)
    tbs, ss = [], []
    for i in range(3):
        t = _payload(rng, i)
        sigs = [cb.detach_sign(kp, t) for kp in _members(rng, 10)]
        parts = [bytes([0xC0 | 60, 1, j & 0xFF]) for j in range(WALK_CAP_MAX + 11 + i)]
        for j, s in enumerate(sigs):
            parts.insert(int(rng.integers(0, len(parts) + 1)) if i else 30 * j, s)
        tbs.append(t)
        ss.append(b"".join(parts))
    return Call(tbs, ss)


def _empty_calls():
    """every signature stream empty (no packet in the whole call), then a call of one item"""
    rng = np.random.default_rng(4807)
    tbs = [_payload(rng, i) for i in range(N_ITEMS)]
    one = _plain_call()
    pk = packets_of(one.ss[0])[:8]                          # seven good signatures and a bad one: insufficient like the empty items
    pk[7] = refuse(pk[7], 0, one.tbs[0])
    return [Call(tbs, [b""] * N_ITEMS), Call(one.tbs[:1], [b"".join(pk)])]


FENCED_NAMES = ("bytes-behind-the-mpis", "partial-length-zero-last-chunk", "partial-length-1100-chunks", "partial-length-17000-byte-body", "md5",
                "value-beyond-R", "nesting-3")


def _fenced_call():
    """the shapes of test_gpu_parity.py::test_fenced_shapes_are_flagged_and_nothing_else_is under this ring: each fenced shape is a
    VALID signature by member 0 followed by eight more members (the item would be sufficient), and between them plain items"""
    R = ring()
    rng = np.random.default_rng(4808)
    kp = R.cluster.replicas[0]
    ct = b"\x05\x02" + struct.pack(">I", cb.CREATION_TIME)
    iss = b"\x09\x10" + struct.pack(">Q", kp.key_id)
    tbs, ss, fenced = [], [], []
    for i in range(21):
        t = _payload(rng, i)

        def v4(hash_id=8, value=None, hashed=None, h=hashlib.sha256):
            hashed_ = (ct + iss) if hashed is None else hashed
            prefix = bytes([4, 0, kp.algo, hash_id]) + struct.pack(">H", len(hashed_)) + hashed_
            digest = h(t + cb.hash_suffix(prefix)).digest()
            sval = kp.rsa_private(cb.emsa(digest, 256)) if value is None else value
            return prefix + b"\x00\x00" + digest[:2] + cb.go_mpi_bytes(sval.to_bytes(max(256, (sval.bit_length() + 7) // 8), "big"))

        def pow2_chunks(b):
            out = bytes([0xC2])
            while b:
                k = len(b).bit_length() - 1
                out += bytes([0xE0 + k]) + b[:1 << k]
                b = b[1 << k:]
            return out
        body = v4()
        rest = b"".join(cb.detach_sign(m, t) for m in R.cluster.replicas[1:9])
        shape = i % 3 == 0 and i // 3
        if i % 3:
            head, f = packet(body), 0
        elif shape == 0:
            head, f = bytes([0xC2, 255]) + (len(body) + 5000).to_bytes(4, "big") + body + bytes(5000), 1
        elif shape == 1:
            head, f = pow2_chunks(body) + b"\x00", 1
        elif shape == 2:
            head, f = bytes([0xC0 | 60]) + b"".join(bytes([0xE0, 7]) for _ in range(1100)) + b"\x00", 1
        elif shape == 3:
            head, f = pow2_chunks(v4(hashed=ct + iss + bytes([255]) + (17000).to_bytes(4, "big") + bytes([100]) + bytes(16999))), 1
        elif shape == 4:
            head, f = packet(v4(hash_id=1, h=hashlib.md5)), 1
        elif shape == 5:
            head, f = packet(v4(value=kp.rsa_private(5) + (1 << 2200))), 1
        else:
            deep = v4()
            for _ in range(3):
                n = len(deep) + 1
                enc = bytes([((n - 192) >> 8) + 192, (n - 192) & 0xFF]) if n >= 192 else bytes([n])
                hashed = ct + iss + enc + bytes([32]) + deep
                deep = bytes([4, 0x19, kp.algo, 8]) + struct.pack(">H", len(hashed)) + hashed + b"\x00\x00\x00\x00" + cb.go_mpi_bytes(b"\x01" * 256)
            head, f = packet(deep), 1
        tbs.append(t)
        ss.append(head + rest)
        fenced.append(f)
    return Call(tbs, ss), fenced


PHASE_MARGIN = 1 + 9 // 64            # capi.hip: margin = 1 + min_suff / 64


def _phase2_call() -> Call:
    """Every packet is a well-formed signature by a member, so the phase-1 window of an item is its first suff + margin = 10 packets.
    Two to four of those are bad (value or hash tag), and nine good ones follow in all: the reference's exit lies behind the window."""
    rng = np.random.default_rng(4809)
    tbs, ss = [], []
    for i in range(N_ITEMS):
        t = _payload(rng, i)
        ms = _members(rng, 13)
        n_bad = 2 + i % 3
        bad_at = set(int(v) for v in rng.permutation(10)[:n_bad])
        pk = []
        for j, kp in enumerate(ms[:n_bad + 9]):
            p = cb.detach_sign(kp, t)
            pk.append(refuse(p, (i + j) % 2, t) if j in bad_at else p)
        tbs.append(t)
        ss.append(b"".join(pk))
    return Call(tbs, ss)


PIPELINE = ("plain", "all_bad", "other_hashes", "wide", "all_lists", "partial", "long_items", "empty", "fenced", "phase2")


@functools.lru_cache(maxsize=None)
def calls_of(name: str):
    if name == "empty":
        return tuple(_empty_calls())
    if name == "fenced":
        return (_fenced_call()[0],)
    return ({"plain": _plain_call, "all_bad": _all_bad_call, "other_hashes": _other_hashes_call, "wide": _wide_call, "all_lists": _all_lists_call,
             "partial": _partial_call, "long_items": _long_items_call, "phase2": _phase2_call}[name](),)


@functools.lru_cache(maxsize=None)
def character(name: str) -> Character:
    R = ring()
    calls = calls_of(name)
    fenced = _fenced_call()[1] if name == "fenced" else None
    return Character(name, calls, tuple(reference(c, R.keyring, R.quorum, fenced) for c in calls))


# successor -> its designated worst predecessors (the issue's table; `fenced` precedes every character)
DESIGNATED = {"plain": ("all_bad", "other_hashes", "wide"), "all_bad": ("plain",), "other_hashes": ("plain",), "wide": ("plain",),
              "empty": ("all_lists",)}
# The pairs the complement condition is asserted on in full.  Behind `fenced` it is asserted on the unfenced items against all_bad,
# other_hashes and wide only (tests/test_state_reference.py): a fenced item's error byte is no statement of the reference, and no
# character can differ in an error byte of two values from `plain` and from `all_bad` at once.
COMPLEMENT_PAIRS = tuple((p, s) for s, ps in DESIGNATED.items() for p in ps)


def designated(name: str):
    return DESIGNATED.get(name, ()) + (("fenced",) if name != "fenced" else ())


def tile(call: Call, times: int) -> Call:
    return Call(list(call.tbs) * times, list(call.ss) * times)


def size(call: Call):
    return len(call.tbs), sum(count_events(s) for s in call.ss), sum(len(s) for s in call.ss), sum(len(t) for t in call.tbs)


def behind(pred: Call, succ) -> Call:
    """The size rule: the predecessor tiled until it has at least as many items, packet events, signature bytes and payload bytes as
    its successor (a call, or a size() tuple: the per-field maximum over several calls), so that nothing stale indexes outside a
    live buffer.  A predecessor without a packet can only match the items and the payload bytes."""
    a, b = size(pred), (size(succ) if isinstance(succ, Call) else tuple(succ))
    return tile(pred, max(1, max(-(-y // x) for x, y in zip(a, b) if x)))


def arrays(call: Call):
    """(tbs_blob, tbs_off, ss_blob, ss_off) as the batched entry points take them"""
    return H.cat(list(call.tbs)) + H.cat(list(call.ss))


# ================================================================================================================================
# the other entry points: good / bad inputs of one shape
# ================================================================================================================================
Entry = namedtuple("Entry", "name family build reference run compared setup")
"""build(kind, n) -> the input (a dict); reference(inp) -> {field: list or array}; run(ctx, inp, handle) -> the same fields from the
device; compared: the fields of the complement condition; setup(ctx, inp) -> handle or None (key sets)."""


def _i2b(v, nbytes):
    return np.frombuffer(b"".join(int(x).to_bytes(nbytes, "big") for x in v), dtype=np.uint8).reshape(len(v), nbytes).copy()


def _b2i(rows):
    return [int.from_bytes(bytes(r), "big") for r in rows]


def _rnd(rng, m):
    return int.from_bytes(rng.bytes((m.bit_length() + 7) // 8 + 8), "big") % m


@functools.lru_cache(maxsize=None)
def _kat():
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "threshold_kat.json")))


@functools.lru_cache(maxsize=None)
def moduli(kind: str):
    """Two odd 2048-bit-class moduli per kind, disjoint between good and bad."""
    k = _kat()
    if kind == "good":
        return (int(k["rsa"]["n"], 16), int(k["sss"]["pb"], 16))
    rs = load_keys("rsa2048", 2)
    return tuple(r["p"] * r["q"] for r in rs)


@functools.lru_cache(maxsize=None)
def composite():
    """3 x a 2041-bit RSA modulus: every Lagrange denominator over seven or more distinct indices shares the factor 3 with it"""
    r = load_keys("rsa2041", 1)[0]
    return 3 * r["p"] * r["q"]


def _seed(name, kind, n):
    return int.from_bytes(hashlib.sha256(repr((name, kind, n)).encode()).digest()[:4], "big")


# ---- modmul_product ----------------------------------------------------------------------------------------------------------
def _modmul_build(kind, n):
    rng = np.random.default_rng(_seed("modmul", kind, n))
    mods = moduli(kind)
    idx = [i % 2 for i in range(n)]
    return {"factors": [[_rnd(rng, mods[i]) or 1 for _ in range(10)] for i in idx], "mods": list(mods), "idx": idx}


def _modmul_ref(inp):
    return {"out": [T.calculate_signature(f, inp["mods"][i]) for f, i in zip(inp["factors"], inp["idx"])]}


def _modmul_run(ctx, inp, handle=None):
    return {"out": ctx.modmul_product(inp["factors"], inp["mods"], inp["idx"])}


# ---- lagrange_combine: the 31-bit path, the big path, and the big path at a width whose products can pass 2128 bits -----------
def _lagrange_build(path):
    k, top = {"small": (7, 10), "big": (22, 64), "huge": (72, 255)}[path]

    def build(kind, n):
        rng = np.random.default_rng(_seed("lagrange-" + path, kind, n))
        if kind == "good":
            mods = list(moduli("good"))
            xs = [[int(v) + 1 for v in rng.permutation(top)[:k]] for _ in range(n)]
        elif path == "huge":
            # 71 factors of 31 bits each: 2201 bits, beyond the 2128 of the exact integers -- fenced
            mods = list(moduli("bad"))
            xs = [[(1 << 31) - 1 - int(v) for v in rng.permutation(4096)[:k]] for _ in range(n)]
        else:
            mods = [composite(), composite() * 5]
            xs = [[int(v) + 1 for v in rng.permutation(top)[:k]] for _ in range(n)]
        idx = [i % 2 for i in range(n)]
        return {"xs": xs, "ys": [[_rnd(rng, mods[i]) for _ in range(k)] for i in idx], "mods": mods, "idx": idx}
    return build


def lagrange_status(xs, m):
    """0; 1 where some denominator has no inverse mod m; 2 where a numerator or denominator passes 2128 bits (76 limbs of 28)"""
    import math
    big, noinv = False, False
    for xj in xs:
        a = b = 1
        for xi in xs:
            if xi == xj:
                continue
            a, b = a * abs(xi), b * abs(xi - xj)
        big |= a.bit_length() > 2128 or b.bit_length() > 2128
        noinv |= math.gcd(b, m) != 1
    return 2 if big else (1 if noinv else 0)


def _needs_big(xs):
    """k_lagrange_inv's rule: some numerator or denominator leaves 31 bits, so the operation is redone on the big path"""
    for xj in xs:
        a = b = 1
        for xi in xs:
            if xi == xj:
                continue
            a, b = a * xi, b * (xi - xj)
            if abs(a) >= 1 << 31 or abs(b) >= 1 << 31:
                return True
    return False


UNCLAIMED = None
"""A result row the header promises nothing about: beside BFTKV_TH_NO_INVERSE the 31-bit Lagrange path leaves the sum of the terms
that do have an inverse, and CalculateR leaves what its chain computed.  No reference speaks for such a row; the call-order tests
still hold it to the baseline, byte for byte.  (The big Lagrange path, bftkv_gpu_modinv and every fenced operation write zeroes.)"""


def _lagrange_ref(inp):
    out, st = [], []
    for xs, ys, i in zip(inp["xs"], inp["ys"], inp["idx"]):
        s = lagrange_status(xs, inp["mods"][i])
        st.append(s)
        out.append(T.calculate_s(list(zip(xs, ys)), inp["mods"][i]) if not s else (UNCLAIMED if s == 1 and not _needs_big(xs) else 0))
    return {"out": out, "status": np.array(st, dtype=np.uint8)}


def _lagrange_run(ctx, inp, handle=None):
    out, st = ctx.lagrange_combine(inp["xs"], inp["ys"], inp["mods"], inp["idx"])
    return {"out": out, "status": st.copy()}


# ---- dsa_calculate_r ---------------------------------------------------------------------------------------------------------
POOL = 12       # where the restatement is slow (2048-bit powers, scalar multiplications) a character cycles through this many distinct
                # operations; 70 and 141 start at different places of the cycle
@functools.lru_cache(maxsize=None)
def dsa_groups(kind):
    ks = load_keys("dsa2048", 4)
    return tuple((k["p"], k["q"], k["g"]) for k in (ks[:2] if kind == "good" else ks[2:4]))


@functools.lru_cache(maxsize=None)
def _calc_r_pool(kind):
    """POOL operations of 2t = 8 partial r's; bad: the last share makes v = sum Vi l_i = 0 mod q, so ModInverse fails"""
    rng = np.random.default_rng(_seed("calc_r", kind, 0))
    groups = dsa_groups(kind)
    k = 8
    ops = []
    for op in range(POOL):
        p, q, g = groups[op % 2]
        x = [int(v) + 1 for v in rng.permutation(10)[:k]]
        r = [pow(g, _rnd(rng, q), p) for _ in range(k)]
        v = [_rnd(rng, q) for _ in range(k)]
        ls = [T.lagrange(xx, x, q) for xx in x]
        if kind == "bad":
            v[-1] = (-sum(a * b for a, b in zip(v[:-1], ls[:-1])) * pow(ls[-1], -1, q)) % q
        if sum(a * b for a, b in zip(v, ls)) % q == 0:
            want = (1, UNCLAIMED)
        else:
            want = (0, T.calculate_r([(xx, rr.to_bytes(256, "big"), vv) for xx, rr, vv in zip(x, r, v)], p, q))
        ops.append((x, r, v, op % 2, want))
    return tuple(ops)


def _calc_r_build(kind, n):
    pool = _calc_r_pool(kind)
    off = 0 if n == SIZES[0] else 5
    ops = [pool[(i + off) % POOL] for i in range(n)]
    return {"xs": [o[0] for o in ops], "ri": [o[1] for o in ops], "vi": [o[2] for o in ops], "groups": [(g[0], g[1]) for g in dsa_groups(kind)],
            "idx": [o[3] for o in ops], "want": [o[4] for o in ops]}


def _calc_r_ref(inp):
    return {"out": [w[1] for w in inp["want"]], "status": np.array([w[0] for w in inp["want"]], dtype=np.uint8)}


def _calc_r_run(ctx, inp, handle=None):
    out, st = ctx.dsa_calculate_r(inp["xs"], inp["ri"], inp["vi"], inp["groups"], inp["idx"])
    return {"out": out, "status": st.copy()}


# ---- sss_distribute ----------------------------------------------------------------------------------------------------------
def _sss_build(kind, n):
    rng = np.random.default_rng(_seed("sss", kind, n))
    mods = moduli(kind)
    idx = [i % 2 for i in range(n)]
    return {"polys": [[_rnd(rng, mods[i]) or 1 for _ in range(7)] for i in idx], "mods": list(mods), "idx": idx}


def _sss_ref(inp):
    return {"shares": [[y for _, y in T.distribute(p[0], 10, 7, inp["mods"][i], p[1:])] for p, i in zip(inp["polys"], inp["idx"])]}


def _sss_run(ctx, inp, handle=None):
    return {"shares": ctx.sss_distribute(inp["polys"], 10, inp["mods"], inp["idx"])}


# ---- modinv ------------------------------------------------------------------------------------------------------------------
def _modinv_build(kind, n):
    import math
    rng = np.random.default_rng(_seed("modinv", kind, n))
    mods = list(moduli("good")) if kind == "good" else [composite(), composite() * 5]
    idx = [i % 2 for i in range(n)]
    vals = []
    for i in idx:
        while True:
            v = _rnd(rng, mods[i]) or 1
            if kind == "bad":
                v = 3 * v % mods[i] or 3
            if (math.gcd(v, mods[i]) == 1) == (kind == "good"):
                break
        vals.append(v)
    return {"values": vals, "mods": mods, "idx": idx}


def _modinv_ref(inp):
    import math
    ok = [math.gcd(v, inp["mods"][i]) == 1 for v, i in zip(inp["values"], inp["idx"])]
    return {"out": [pow(v, -1, inp["mods"][i]) if o else 0 for v, i, o in zip(inp["values"], inp["idx"], ok)],
            "status": np.array([0 if o else 1 for o in ok], dtype=np.uint8)}


def _modinv_run(ctx, inp, handle=None):
    out, st = ctx.modinv(inp["values"], inp["mods"], inp["idx"])
    return {"out": out, "status": st.copy()}


# ---- modexp (one exponent per modulus) and modexp_ops (one per operation) -----------------------------------------------------
def _modexp_build(per_op):
    def build(kind, n):
        rng = np.random.default_rng(_seed("modexp%d" % per_op, kind, n))
        mods = moduli(kind)
        idx = [i % 2 for i in range(n)]
        exps = [int.from_bytes(rng.bytes(32), "big") | 1 for _ in range(n if per_op else 2)]
        return {"base": [_rnd(rng, mods[i]) or 2 for i in idx], "mods": list(mods), "idx": idx, "exps": exps}
    return build


def _modexp_ref(inp):
    per_op = len(inp["exps"]) == len(inp["base"])
    return {"out": [pow(b, inp["exps"][j if per_op else i], inp["mods"][i]) for j, (b, i) in enumerate(zip(inp["base"], inp["idx"]))]}


def _modexp_run(ctx, inp, handle=None):
    per_op = len(inp["exps"]) == len(inp["base"])
    f = ctx.modexp_ops if per_op else ctx.modexp
    return {"out": _b2i(f(_i2b(inp["base"], 256), np.array(inp["idx"], dtype=np.uint32), _i2b(inp["mods"], 256), _i2b(inp["exps"], 32)))}


# ---- threshold ECDSA: CalculateR and CalculatePartialR on P-256 --------------------------------------------------------------
def _curve():
    import ec_ref as E
    return E, E.CURVES["P-256"]


@functools.lru_cache(maxsize=None)
def _ec_pool(kind):
    """POOL operations of k = 4 shares each: random points and shares (good); the same with the second partial R off the curve
    (fenced) or, for every third operation, v = 0 mod N (no inverse)."""
    E, c = _curve()
    rng = np.random.default_rng(_seed("ec_calc_r", kind, 0))
    n, p = c["n"], c["p"]
    ops = []
    for j in range(POOL):
        xs = [int(v) + 1 for v in rng.permutation(10)[:4]]
        ri = [E.calculate_partial_r(c, _rnd(rng, n) or 1) for _ in range(4)]
        vi = [_rnd(rng, n) for _ in range(4)]
        if kind == "bad" and j % 3 == 2:
            ls = [T.lagrange(x, xs, n) for x in xs]
            vi[-1] = (-sum(a * b for a, b in zip(vi[:-1], ls[:-1])) * pow(ls[-1], -1, n)) % n
        elif kind == "bad":
            x0, y0 = int.from_bytes(ri[1][1:33], "big"), int.from_bytes(ri[1][33:], "big")
            ri[1] = E.marshal(c, x0, (y0 + 1) % p)
        ops.append((xs, ri, vi, E.calculate_r(c, xs, ri, vi)))
    return tuple(ops)


def _ec_calc_r_build(kind, n):
    pool = _ec_pool(kind)
    off = 0 if n == SIZES[0] else 5
    return {"ops": [pool[(i + off) % POOL] for i in range(n)]}


def _ec_calc_r_ref(inp):
    return {"out": [o[3][1] for o in inp["ops"]], "status": np.array([o[3][0] for o in inp["ops"]], dtype=np.uint8)}


def _ec_calc_r_run(ctx, inp, handle=None):
    _, c = _curve()
    out, st = ctx.ecdsa_calculate_r([o[0] for o in inp["ops"]], [o[1] for o in inp["ops"]], [o[2] for o in inp["ops"]], c)
    return {"out": out, "status": st.copy()}


@functools.lru_cache(maxsize=None)
def _ec_base_pool(kind):
    E, c = _curve()
    rng = np.random.default_rng(_seed("ec_base", kind, 0))
    n = c["n"]
    if kind == "good":
        ks = [_rnd(rng, n) or 1 for _ in range(POOL)]
        return tuple((k, E.calculate_partial_r(c, k), 0) for k in ks)
    # a scalar of N or more never comes from the reference: fenced, zeroes
    return tuple((n + int(rng.integers(0, 1 << 20)), bytes(65), E.FENCED) for _ in range(POOL))


def _ec_base_build(kind, n):
    pool = _ec_base_pool(kind)
    off = 0 if n == SIZES[0] else 5
    return {"ops": [pool[(i + off) % POOL] for i in range(n)]}


def _ec_base_ref(inp):
    return {"out": [o[1] for o in inp["ops"]], "status": np.array([o[2] for o in inp["ops"]], dtype=np.uint8)}


def _ec_base_run(ctx, inp, handle=None):
    _, c = _curve()
    out, st = ctx.ec_scalar_base_mult([o[0] for o in inp["ops"]], c)
    return {"out": out, "status": st.copy()}


# ---- ecdsa_verify and ecdsa_verify_keyset ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ecv_pool(kind):
    """good: honest signatures under two keys.  bad: fenced, the worst ecdsa_verify reports, both ways -- key 0 is off the curve (the key
    check fences), and under the good key 1 the digest is all zero, honestly signed (e = 0: the per-operation flag of the first kernel
    fences).  For the key set, whose refused key fences as well, the same table serves.  invalid (beyond the issue's two kinds): status 0
    beside validity 0, the answer a stale byte of either neighbour would change."""
    import ecdsa_verify_cases as EC
    import ecdsa_verify_ref as V
    E, c = _curve()
    rng = np.random.default_rng(_seed("ecv", kind, 0))
    ds = [_rnd(rng, c["n"]) or 1 for _ in range(2)]
    qs = [E.scalar_base_mult(c, d) for d in ds]
    keys = [E.marshal(c, *q) for q in qs]
    if kind == "bad":
        keys[0] = E.marshal(c, qs[0][0], (qs[0][1] + 1) % c["p"])
    ops = []
    for j in range(POOL):
        dg = bytes(32) if kind == "bad" and j % 2 else rng.bytes(32)
        r, s = EC.sign(c, ds[j % 2], dg, _rnd(rng, c["n"]) or 1)
        if kind == "invalid":                               # merely invalid: r = 0 (refused before any arithmetic), or another digest
            r, dg = (0, dg) if j % 3 == 0 else (r, bytes([dg[0] ^ 0x80]) + dg[1:])
        sig = EC.sig_bytes(c, r, s)
        ops.append((dg, sig, j % 2, V.verify(c, keys[j % 2], dg, sig)))
    return tuple(keys), tuple(ops)


def _ecv_build(kind, n):
    keys, pool = _ecv_pool(kind)
    off = 0 if n == SIZES[0] else 5
    return {"keys": list(keys), "ops": [pool[(i + off) % POOL] for i in range(n)]}


def _verdict_ref(inp):
    return {"valid": np.array([o[3][0] for o in inp["ops"]], dtype=np.uint8), "status": np.array([o[3][1] for o in inp["ops"]], dtype=np.uint8)}


def _ecv_run(ctx, inp, handle=None):
    _, c = _curve()
    dg, sg, ki = [o[0] for o in inp["ops"]], [o[1] for o in inp["ops"]], [o[2] for o in inp["ops"]]
    v, st = ctx.ecdsa_verify(dg, sg, inp["keys"], c, ki) if handle is None else ctx.ecdsa_verify_keyset(handle, dg, sg, ki)
    return {"valid": v.copy(), "status": st.copy()}


def _ecv_setup(ctx, inp):
    return ctx.ecdsa_keyset_create(inp["keys"], _curve()[1])


# ---- dsa_verify and dsa_verify_keyset ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dsav_pool(kind):
    """good: honest signatures over 32-byte digests under two keys of keys_dsa2048 (the raw entry takes p of at most 2048 bits).  bad:
    the same with 33-byte digests -- one byte more than the order has: fenced, the worst dsa_verify reports under a prime q."""
    import dsa_verify_cases as DC
    import dsa_verify_ref as V
    rng = np.random.default_rng(_seed("dsav", kind, 0))
    ks = load_keys("dsa2048", 6)[4:6]
    if kind == "invalid":
        # merely invalid, 20-byte digests: under a prime q r = q (out of range) or the honest signature of another digest -- validity
        # 0, status 0 --, and under the composite 160-bit q of the verify corpus s = 3, which has no inverse: BFTKV_TH_NO_INVERSE
        G = DC.group("composite_q160")
        ks = [ks[0], {"p": G.p, "q": G.q, "g": G.g, "x": G.x}]
    ys = [pow(k["g"], k["x"], k["p"]) for k in ks]
    ops = []
    for j in range(POOL):
        k = ks[j % 2]
        dg = rng.bytes(20 if kind == "invalid" else 32)
        while True:
            rs = DC.sign(k["p"], k["q"], k["g"], k["x"], dg, DC.rnd(rng, k["q"]) or 1) or (kind == "invalid" and j % 2 and (1 + DC.rnd(rng, k["q"] - 1), 3))
            if rs:
                break
        if kind == "bad":
            dg = dg + b"\x00"
        elif kind == "invalid":
            rs, dg = ((rs[0], 3), dg) if j % 2 else ((k["q"], rs[1]), dg) if j % 4 == 0 else (rs, bytes([dg[0] ^ 0x80]) + dg[1:])
        sig = rs[0].to_bytes(32, "big") + rs[1].to_bytes(32, "big")
        ops.append((dg, sig, j % 2, V.verify(k["p"], k["q"], k["g"], ys[j % 2], dg, *rs)))
    return tuple((k["p"], k["q"], k["g"]) for k in ks), tuple((i, y) for i, y in enumerate(ys)), tuple(ops)


def _dsav_build(kind, n):
    groups, keys, pool = _dsav_pool(kind)
    off = 0 if n == SIZES[0] else 5
    return {"groups": list(groups), "keys": list(keys), "ops": [pool[(i + off) % POOL] for i in range(n)]}


def _dsav_run(ctx, inp, handle=None):
    dg, sg, ki = [o[0] for o in inp["ops"]], [o[1] for o in inp["ops"]], [o[2] for o in inp["ops"]]
    if handle is None:
        v, st = ctx.dsa_verify(dg, sg, inp["keys"], inp["groups"], ki, pbytes=256, qbytes=32)
    else:
        v, st = ctx.dsa_verify_keyset(handle, dg, sg, ki)
    return {"valid": v.copy(), "status": st.copy()}


def _dsav_setup(ctx, inp):
    return ctx.dsa_keyset_create(inp["keys"], inp["groups"], window_bits=4, pbytes=256, qbytes=32)


# ---- rsa_verify and rsa_verify_keyset ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rsav_pool(kind):
    """good: honest SHA-256 signatures under two RSA-2048 keys.  bad: the same signatures under n + 1 (even): fenced."""
    import rsa_verify_ref as V
    rng = np.random.default_rng(_seed("rsav", kind, 0))
    ks = load_keys("rsa2048", 4)[2:4]
    keys = [(k["p"] * k["q"] + (1 if kind == "bad" else 0), k["e"]) for k in ks]
    ops = []
    for j in range(POOL):
        k = ks[j % 2]
        n = k["p"] * k["q"]
        dg = rng.bytes(32)
        s = pow(int.from_bytes(V.em(256, 8, dg), "big"), pow(k["e"], -1, (k["p"] - 1) * (k["q"] - 1)), n)
        if kind == "invalid":                               # the honest signature of another digest: validity 0, status 0
            dg = bytes([dg[0] ^ 1]) + dg[1:]
        ops.append((dg, s.to_bytes(256, "big"), j % 2, V.verify(keys[j % 2][0], keys[j % 2][1], 8, dg, s)))
    return tuple(keys), tuple(ops)


def _rsav_build(kind, n):
    keys, pool = _rsav_pool(kind)
    off = 0 if n == SIZES[0] else 5
    return {"keys": list(keys), "ops": [pool[(i + off) % POOL] for i in range(n)]}


def _rsav_run(ctx, inp, handle=None):
    dg, sg, ki = [o[0] for o in inp["ops"]], [o[1] for o in inp["ops"]], [o[2] for o in inp["ops"]]
    v, st = ctx.rsa_verify(dg, sg, inp["keys"], 8, ki, nbytes=256) if handle is None else ctx.rsa_verify_keyset(handle, dg, sg, 8, ki)
    return {"valid": v.copy(), "status": st.copy()}


def _rsav_setup(ctx, inp):
    return ctx.rsa_keyset_create(inp["keys"], nbytes=256)


# ---- password authentication: makeYi, makeBi, processBi ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tpa_pool(kind):
    import random
    import tpa_ref as R
    rng = random.Random(_seed("tpa", kind, 0))
    mods = moduli(kind)
    ops = []
    for j in range(POOL):
        p = mods[j % 2]
        v, b = rng.randrange(2, p), rng.randrange(1 << 256)
        xi = R.to_bytes(rng.randrange(2, p))
        salt = bytes(rng.getrandbits(8) for _ in range(32))
        vb = R.exp(v, b, p)
        ops.append((j % 2, v, xi, b, salt, vb, (vb,) + R.finish(R.exp(int.from_bytes(xi, "big"), b, p), vb, xi, salt), R.finish(vb, v, xi, salt)))
    return tuple(ops)


def _tpa_build(kind, n):
    pool = _tpa_pool(kind)
    off = 0 if n == SIZES[0] else 5
    return {"mods": list(moduli(kind)), "ops": [pool[(i + off) % POOL] for i in range(n)]}


def _tpa_rows(inp):
    ops = inp["ops"]
    xi = np.zeros((len(ops), 256), dtype=np.uint8)
    for i, o in enumerate(ops):
        xi[i, :len(o[2])] = np.frombuffer(o[2], dtype=np.uint8)
    return (_i2b([o[1] for o in ops], 256), xi, [len(o[2]) for o in ops], _i2b([o[3] for o in ops], 32),
            np.frombuffer(b"".join(o[4] for o in ops), dtype=np.uint8).reshape(len(ops), 32).copy(), _i2b(inp["mods"], 256), [o[0] for o in ops])


def _tpa_ref(which):
    def ref(inp):
        ops, z = inp["ops"], np.zeros(len(inp["ops"]), dtype=np.uint8)
        if which == "yi":
            return {"out": [o[5] for o in ops], "status": z}
        if which == "bi":
            return {"out": [o[6][0] for o in ops], "keys": [o[6][1] for o in ops], "mac": [o[6][2] for o in ops], "status": z}
        return {"keys": [o[7][0] for o in ops], "mac": [o[7][1] for o in ops], "status": z}
    return ref


def _tpa_run(which):
    def run(ctx, inp, handle=None):
        v, xi, xl, b, salt, mods, mi = _tpa_rows(inp)
        if which == "yi":
            out, st = ctx.tpa_yi(v, b, mods, mi)
            return {"out": _b2i(out), "status": st.copy()}
        if which == "bi":
            out, keys, mac, st = ctx.tpa_bi(v, xi, xl, b, salt, mods, mi)
            return {"out": _b2i(out), "keys": [bytes(r) for r in keys], "mac": [bytes(r) for r in mac], "status": st.copy()}
        keys, mac, st = ctx.tpa_ni(v, xi, xl, b, salt, mods, mi)
        return {"keys": [bytes(r) for r in keys], "mac": [bytes(r) for r in mac], "status": st.copy()}
    return run


# ---- rsa_sign_keyset and selftest_rsa_crt: one signer set of 256-byte rows and 128-byte private parts ------------------------
TH_OK, TH_NO_INVERSE, TH_FENCED, TH_INVALID_INPUT, TH_CHECK_FAILED = 0, 1, 2, 3, 4
RSAS_SIGS_PER_BLOCK = 64 // 2         # rsa_sign_kernels.hip: QUADS_PER_BLOCK / 2, two quads of a 256-thread block per signature


@functools.lru_cache(maxsize=None)
def _rsas_keys(kind):
    """good: two honest RSA-2048 keys, none of them a key of _rsav_pool (keys 2 and 3) or of moduli("bad") (keys 0 and 1).  bad: the
    same with qinv + 1: every signature fails the check.  other: two more honest keys (the self-test's `bad`).  refused: key 0 with
    an even p (fenced), and an honest 368-bit key, under which SHA-256 meets the length rule (k = 46 < 51 + 11)."""
    import rsa_sign_cases as SC
    import rsa_sign_ref as R
    ks = [R.key_from_primes(k["p"], k["q"], k["e"]) for k in load_keys("rsa2048", 8)[4:8]]
    if kind == "good":
        return tuple(ks[:2])
    if kind == "bad":
        return tuple(SC._break(k, "qinv+1") for k in ks[:2])
    if kind == "other":
        return tuple(ks[2:4])
    small = load_keys("rsa368", 1)[0]
    return (SC._refuse(ks[0], "even_p"), R.key_from_primes(small["p"], small["q"], small["e"]))


@functools.lru_cache(maxsize=None)
def _rsas_pool(kind):
    """POOL SHA-256 digests, the keys alternating: (digest, key index, status, s).  refused: the even rows are fenced, the odd ones
    refused by the length rule -- neither is the status of `good` (0) or of `bad` (4)."""
    import rsa_sign_ref as R
    rng = np.random.default_rng(_seed("rsas", kind, 0))
    keys = _rsas_keys(kind)
    ops = []
    for j in range(POOL):
        dg = rng.bytes(32)
        ops.append((dg, j % 2) + R.sign(keys[j % 2], 8, dg, 256))
    return keys, tuple(ops)


def _rsas_build(kind, n):
    keys, pool = _rsas_pool(kind)
    off = 0 if n == SIZES[0] else 5
    return {"keys": [k._asdict() for k in keys], "ops": [pool[(i + off) % POOL] for i in range(n)]}


def _rsas_ref(inp):
    return {"sig": [o[3] for o in inp["ops"]], "status": np.array([o[2] for o in inp["ops"]], dtype=np.uint8)}


def _rsas_run(ctx, inp, handle):
    sig, st = ctx.rsa_sign_keyset(handle, [o[0] for o in inp["ops"]], 8, [o[1] for o in inp["ops"]])
    return {"sig": _b2i(sig), "status": st.copy(), "sig_rows": sig}           # (the rows as the wrapper allocated them: section (f))


def _rsas_setup(ctx, inp):
    return ctx.rsa_signer_create(inp["keys"], nbytes=256, pbytes=128)


@functools.lru_cache(maxsize=None)
def _crt_pool(kind):
    """POOL values below n through the chains and the recombination alone (no padding, no check): there is no per-operation
    failure, `bad` is other values under the other two keys."""
    import rsa_sign_ref as R
    rng = np.random.default_rng(_seed("rsa_crt", kind, 0))
    keys = _rsas_keys("good" if kind == "good" else "other")
    ops = []
    for j in range(POOL):
        c = _rnd(rng, keys[j % 2].n) or 2
        ops.append((c, j % 2) + R.selftest(keys[j % 2], c, 256))
    return keys, tuple(ops)


def _crt_build(kind, n):
    keys, pool = _crt_pool(kind)
    off = 0 if n == SIZES[0] else 5
    return {"keys": [k._asdict() for k in keys], "ops": [pool[(i + off) % POOL] for i in range(n)]}


def _crt_ref(inp):
    return {"out": [o[3] for o in inp["ops"]], "status": np.array([o[2] for o in inp["ops"]], dtype=np.uint8)}


def _crt_run(ctx, inp, handle):
    out, st = ctx.selftest_rsa_crt(handle, [o[0] for o in inp["ops"]], [o[1] for o in inp["ops"]])
    return {"out": _b2i(out), "status": st.copy(), "out_rows": out}


# ---- rsa_partial_sign --------------------------------------------------------------------------------------------------------
PSIGN_EXP_LEN = 64
PSIGN_WIDTHS = (64, 33, 17)           # exp_used: three widths, so that the host's longest-first order is a real permutation


def _psign_t(rng, n, bad):
    """T of 51 bytes (the length of a SHA-256 DigestInfo) whose em is a unit mod n, or (bad) a multiple of 3: a counter in its tail"""
    import math
    import rsa_psign_ref as P
    head = rng.bytes(47)
    for ctr in range(1 << 16):
        t = head + ctr.to_bytes(4, "big")
        em = P.emsa_encode(t, n)
        if math.gcd(em, n) == (3 if bad else 1):
            return t
    raise ValueError("no T found")


def _psign_build(kind, n):
    """n fragments over requests of three and two fragments in turn, handed over in a shuffled order (frag_req is no sorted list).
    good: under moduli("good"), every third request without a negative fragment, both signs in each of the others.  bad: every
    fragment negative (three different non-zero sign bytes), under 3 x a 2041-bit modulus and 15 x it, with 3 | em: no inverse.
    positive: `good`'s shape with every sign byte 0 -- the inversion kernel is not launched at all."""
    rng = np.random.default_rng(_seed("psign", kind, n))
    mods = [composite(), composite() * 5] if kind == "bad" else list(moduli("good"))
    ts, frags = [], []
    while len(frags) < n:
        r = len(ts)
        ts.append(_psign_t(rng, mods[r % 2], kind == "bad"))
        for j in range(min(2 + (r + 1) % 2, n - len(frags))):
            used = PSIGN_WIDTHS[(r + j) % 3]
            mag = int.from_bytes(rng.bytes(used), "big") | (1 << (8 * used - 1))
            if kind == "bad":
                sb = (1, 0xFF, 2)[j]
            elif kind == "positive" or r % 3 == 2:
                sb = 0
            else:
                sb = (1, 0xFF, 0)[(r + j) % 3]
            frags.append((r, sb, mag, used))
    frags = [frags[int(i)] for i in rng.permutation(n)]
    return {"t": ts, "mods": mods, "mod_idx": [r % 2 for r in range(len(ts))], "frags": frags}


def _psign_ref(inp):
    import rsa_psign_ref as P
    res = [P.sign(inp["t"][r], inp["mods"][inp["mod_idx"][r]], [(sb, mag)])[0] for r, sb, mag, _ in inp["frags"]]
    return {"out": [v for _, v in res], "status": np.array([s for s, _ in res], dtype=np.uint8)}


def _psign_run(ctx, inp, handle=None):
    ts, fr = inp["t"], inp["frags"]
    t = np.full((len(ts), max(len(b) for b in ts)), 0xEE, dtype=np.uint8)      # what follows T in its row is not zero
    for i, b in enumerate(ts):
        t[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    out, st = ctx.rsa_partial_sign(t, [len(b) for b in ts], _i2b(inp["mods"], 256), _i2b([f[2] for f in fr], PSIGN_EXP_LEN),
                                   np.array([f[1] for f in fr], dtype=np.uint8), inp["mod_idx"], [f[0] for f in fr], [f[3] for f in fr])
    return {"out": _b2i(out), "status": st.copy(), "out_rows": out}


# ---- threshold DSA / ECDSA signing: the share answers and phase 3 --------------------------------------------------------------
TSIG_M = 4                            # shares per request
TSIG_FIELDS = ("ri", "vi", "ki", "ci")


def _tsig_requests(q, seeds, keep):
    """the requests of the classes `keep` admits, those with every share at or above q from row 5 on (where both sizes of a character
    hold them: _tsig_rows)"""
    import tsig_share_cases as K
    cases = [(lb, sh) for s in seeds for lb, sh in K.requests(q, 32, TSIG_M, 4, K.windows_of(q, 4), seed=s) if keep(lb)]
    above, rest = [sh for lb, sh in cases if lb == "s:above_q"], [sh for lb, sh in cases if lb != "s:above_q"]
    return rest[:5] + above + rest[5:]


def _tsig_rows(n):
    off = 0 if n == SIZES[0] else 5
    return [i + off for i in range(n)]


@functools.lru_cache(maxsize=None)
def _tdsa_pool(kind):
    """good: every class of tests/tsig_share_cases.py under group 0 of its two groups (1024 / 160 bits in rows of 256 / 32 bytes), less
    the two whose columns sum to 0 (a result row of a good operation is never zero).  bad: under group 1 (2048 / 256 bits), less the
    classes with an answer that does not depend on the group (ai = 0: ri = 1; all sums 0 or 1; m shares of q - 1 in every column:
    vi = m^2 - m); its `above_q` requests hold shares in [q, 2^256).  No row of one appears in the other
    (tests/test_state_reference.py)."""
    import tsig_share_cases as K
    import tsig_share_ref as R
    gs = [K.dsa_groups()[name] for name in K.DSA_NAMES]
    gi = 0 if kind == "good" else 1
    drop = ("s:sum_0", "s:sum_q") if kind == "good" else ("s:sum_0", "s:sum_q", "s:sum_1", "s:wrap", "a:zero")
    reqs = _tsig_requests(gs[gi].q, (11, 12) if kind == "good" else (13, 14), lambda lb: lb not in drop)[:SIZES[1] + 5]
    G = R.dsa_group(gs[gi].p, gs[gi].q, gs[gi].g, 256, 32)
    ans = [R.phase2(G, sh) for sh in reqs]
    return gs, gi, reqs, [(int.from_bytes(a.ri, "big"), a.vi, a.ki, a.ci) for a in ans]


def _tdsa_build(kind, n):
    gs, gi, reqs, ans = _tdsa_pool(kind)
    rows = _tsig_rows(n)
    return {"groups": [(g.p, g.q, g.g) for g in gs], "keys": [(i, g.y) for i, g in enumerate(gs)], "gi": gi, "reqs": [reqs[i] for i in rows],
            "want": [ans[i] for i in rows]}


def _tsig_ref(inp):
    out = {f: [w[k] for w in inp["want"]] for k, f in enumerate(TSIG_FIELDS)}
    out["status"] = np.zeros(len(inp["want"]), dtype=np.uint8)
    return out


def _tdsa_setup(ctx, inp):
    return ctx.dsa_keyset_create(inp["keys"], inp["groups"], window_bits=4, pbytes=256, qbytes=32)


def _tdsa_run(ctx, inp, handle):
    import tsig_share_cases as K
    ri, vi, ki, ci, st = ctx.tdsa_share(handle, K.shares_array(inp["reqs"], 32), group_idx=[inp["gi"]] * len(inp["reqs"]))
    return {"ri": _b2i(ri), "vi": _b2i(vi), "ki": _b2i(ki), "ci": _b2i(ci), "status": st.copy(), "ri_rows": ri, "vi_rows": vi, "ki_rows": ki, "ci_rows": ci}


@functools.lru_cache(maxsize=None)
def _tecdsa_pool(kind):
    """P-256 (P-521 costs the device 14 ms a call whatever its size, docs/history.md, and the restatement in proportion).  good: every
    class but the two zero sums.  bad: the classes with a random ai alone -- one group serves both kinds, so a fixed scalar (0, 1, 2,
    q - 1, one digit, ...) would put the same ri into both."""
    import tsig_share_ref as R
    E, c = _curve()
    n = c["n"]
    if kind == "good":
        reqs = _tsig_requests(n, (21, 22), lambda lb: lb not in ("s:sum_0", "s:sum_q"))
    else:
        reqs = _tsig_requests(n, (31, 32, 33, 34, 35), lambda lb: lb.startswith("a:random") or lb == "s:above_q")
    reqs = reqs[:SIZES[1] + 5]
    ans = []
    for sh in reqs:
        ki, ai, bi, ci = R.fold(sh, n)
        ans.append((E.calculate_partial_r(c, ai), R.vi_of(n, ki, ai, bi), ki, ci))
    return reqs, ans


def _tecdsa_build(kind, n):
    reqs, ans = _tecdsa_pool(kind)
    rows = _tsig_rows(n)
    return {"reqs": [reqs[i] for i in rows], "want": [ans[i] for i in rows]}


def _tecdsa_run(ctx, inp, handle=None):
    import tsig_share_cases as K
    ri, vi, ki, ci, st = ctx.tecdsa_share(K.shares_array(inp["reqs"], 32), _curve()[1])
    return {"ri": [bytes(r) for r in ri], "vi": _b2i(vi), "ki": _b2i(ki), "ci": _b2i(ci), "status": st.copy(), "ri_rows": ri, "vi_rows": vi, "ki_rows": ki,
            "ci_rows": ci}


@functools.lru_cache(maxsize=None)
def partial_s_orders(kind):
    """Two odd orders in rows of 32 bytes.  good: the 256-bit q of the 2048-bit DSA group and P-256's N.  bad: the 160-bit q of the
    1024-bit group and P-224's N, so that there is room for operands at or above q."""
    import tsig_share_cases as K
    E, c = _curve()
    if kind == "good":
        return (K.dsa_groups()["dsa2048"].q, c["n"])
    return (K.dsa_groups()["dsa1024"].q, E.CURVES["P-224"]["n"])


def _partial_s_build(kind, n):
    """(m, r, y, k, c) per request: below q (good); every operand in [q, 2^256) (bad)"""
    import random
    rng = random.Random(_seed("partial_s", kind, n))
    qs = partial_s_orders(kind)
    idx = [i % 2 for i in range(n)]
    return {"q": list(qs), "idx": idx, "ops": [tuple(rng.randrange(qs[i]) if kind == "good" else rng.randrange(qs[i], 1 << 256) for _ in range(5)) for i in idx]}


def _partial_s_ref(inp):
    import tsig_share_ref as R
    return {"si": [R.phase3(inp["q"][i], r, y, m, k, c) for (m, r, y, k, c), i in zip(inp["ops"], inp["idx"])],
            "status": np.zeros(len(inp["ops"]), dtype=np.uint8)}


def _partial_s_run(ctx, inp, handle=None):
    m, r, y, k, c = (_i2b([o[j] for o in inp["ops"]], 32) for j in range(5))
    si, st = ctx.tsig_partial_s(m, r, y, k, c, _i2b(inp["q"], 32), inp["idx"])
    return {"si": _b2i(si), "status": st.copy(), "si_rows": si}


ENTRIES = (
    Entry("modmul_product", "threshold", _modmul_build, _modmul_ref, _modmul_run, ("out",), None),
    Entry("lagrange_combine_small", "threshold", _lagrange_build("small"), _lagrange_ref, _lagrange_run, ("out", "status"), None),
    Entry("lagrange_combine_big", "threshold", _lagrange_build("big"), _lagrange_ref, _lagrange_run, ("out", "status"), None),
    Entry("lagrange_combine_huge", "threshold", _lagrange_build("huge"), _lagrange_ref, _lagrange_run, ("out", "status"), None),
    Entry("dsa_calculate_r", "threshold", _calc_r_build, _calc_r_ref, _calc_r_run, ("out", "status"), None),
    Entry("sss_distribute", "threshold", _sss_build, _sss_ref, _sss_run, ("shares",), None),
    Entry("modinv", "threshold", _modinv_build, _modinv_ref, _modinv_run, ("out", "status"), None),
    Entry("modexp", "threshold", _modexp_build(False), _modexp_ref, _modexp_run, ("out",), None),
    Entry("modexp_ops", "threshold", _modexp_build(True), _modexp_ref, _modexp_run, ("out",), None),
    Entry("ecdsa_calculate_r", "ec", _ec_calc_r_build, _ec_calc_r_ref, _ec_calc_r_run, ("out", "status"), None),
    Entry("ec_scalar_base_mult", "ec", _ec_base_build, _ec_base_ref, _ec_base_run, ("out", "status"), None),
    Entry("ecdsa_verify", "ec", _ecv_build, _verdict_ref, _ecv_run, ("valid", "status"), None),
    Entry("ecdsa_verify_keyset", "ec", _ecv_build, _verdict_ref, _ecv_run, ("valid", "status"), _ecv_setup),
    Entry("dsa_verify", "raw", _dsav_build, _verdict_ref, _dsav_run, ("valid", "status"), None),
    Entry("dsa_verify_keyset", "raw", _dsav_build, _verdict_ref, _dsav_run, ("valid", "status"), _dsav_setup),
    Entry("rsa_verify", "raw", _rsav_build, _verdict_ref, _rsav_run, ("valid", "status"), None),
    Entry("rsa_verify_keyset", "raw", _rsav_build, _verdict_ref, _rsav_run, ("valid", "status"), _rsav_setup),
    Entry("tpa_yi", "tpa", _tpa_build, _tpa_ref("yi"), _tpa_run("yi"), ("out",), None),
    Entry("tpa_bi", "tpa", _tpa_build, _tpa_ref("bi"), _tpa_run("bi"), ("out", "keys", "mac"), None),
    Entry("tpa_ni", "tpa", _tpa_build, _tpa_ref("ni"), _tpa_run("ni"), ("keys", "mac"), None),
    Entry("rsa_sign_keyset", "sign", _rsas_build, _rsas_ref, _rsas_run, ("sig", "status"), _rsas_setup),
    Entry("rsa_crt_selftest", "sign", _crt_build, _crt_ref, _crt_run, ("out",), _rsas_setup),
    Entry("rsa_partial_sign", "sign", _psign_build, _psign_ref, _psign_run, ("out", "status"), None),
    Entry("tdsa_share", "sign", _tdsa_build, _tsig_ref, _tdsa_run, TSIG_FIELDS, _tdsa_setup),
    Entry("tecdsa_share", "sign", _tecdsa_build, _tsig_ref, _tecdsa_run, TSIG_FIELDS, None),
    Entry("tsig_partial_s", "sign", _partial_s_build, _partial_s_ref, _partial_s_run, ("si",), None),
)
ENTRY = {e.name: e for e in ENTRIES}
VERIFY = tuple(e.name for e in ENTRIES if "valid" in e.compared)      # these also come as kind "invalid"
THIRD_KIND = {"rsa_sign_keyset": "refused", "rsa_partial_sign": "positive"}      # the signing entries' third kinds


@functools.lru_cache(maxsize=None)
def op_input(name: str, kind: str, n: int):
    return ENTRY[name].build(kind, n)


@functools.lru_cache(maxsize=None)
def op_reference(name: str, kind: str, n: int):
    return ENTRY[name].reference(op_input(name, kind, n))
