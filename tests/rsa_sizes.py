"""RSA verification over modulus sizes and hashes: the keys, a signer for any hash (cell_cases) and the case matrix shared by
tests/test_rsa_sizes_reference.py (the two oracles agree on it; it is what it claims to be) and tests/test_gpu_rsa_sizes.py (the
device agrees with the oracle on it).

Every modulus length below is there for a line of the kernels (bftkv_amd/csrc/kernels.hip): with k its byte length and tLen the
length of DigestInfo || digest,
  * k < tLen + 11 is refused before any arithmetic (k_parse_body, rsa.VerifyPKCS1v15);
  * limbs 24 and up of s^e mod n are compared with 00 01 FF .. FF in k_rsa_modexp (em_head_limb: zeros above bit 8(k-2), a
    partial limb there, ones below), the low 84 bytes are rebuilt from the digest in k_rsa_compare (em_word, whose word-straddling
    branches depend on tLen mod 4, k mod 4 and on whether the 00 01 top falls inside the 84 bytes);
  * the size class (<= 2048, <= 3072, <= 4096 bits) picks the mont_mul instantiation and the cap R on a signature VALUE's length
    (266 / 392 / 532 bytes); a modulus shorter than its class leaves the top lanes of n empty.
"""
from __future__ import annotations

import functools
import hashlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

from corpus import build as cb
from corpus.keys import load_keys
from oracle import openpgp as pgp

# (modulus bits, keys of that size)
SIZES: List[Tuple[int, int]] = [
    (256, 1),                                                   # below every tLen + 11
    (360, 1), (368, 1),                                         # SHA-1:   tLen + 11 = 46
    (456, 1), (464, 1),                                         # SHA-224: 58
    (488, 1), (496, 1),                                         # SHA-256: 62
    (616, 1), (624, 1),                                         # SHA-384: 78
    (744, 1), (752, 1),                                         # SHA-512: 94
    (512, 1),                                                   # the whole EM inside the low 84 bytes
    (664, 1), (672, 1), (680, 1), (688, 1), (696, 1),           # the 00 01 top crosses byte 84 / limb 24
    (1016, 1), (1023, 1), (1024, 1), (1025, 1), (1032, 1), (1040, 1),   # k mod 4 = 3, 0, 0, 1, 1, 2; bit lengths off the byte
    (2041, 1), (2047, 1), (2048, 2),                            # top of the first class
    (2049, 1), (2056, 1),                                       # first sizes of the second class
    (3071, 1), (3072, 1), (3073, 1),                            # second class -> third
    (4095, 1), (4096, 1),                                       # top of the third
    (4097, 1), (4104, 1),                                       # above the kernels
]
SMALL_EXPONENT_KEYS = ["rsa%de%d" % (b, e) for b in (1025, 2049, 3073) for e in (3, 17)]
HASHES = [(2, "sha1"), (11, "sha224"), (8, "sha256"), (9, "sha384"), (10, "sha512")]     # RFC 4880 9.4 ids
EM_LOW_BYTES = 84                                               # kernels.hip: the split between k_rsa_compare and k_rsa_modexp
MAX_BITS = 4096

ST_OK, ST_BAD_SIG, ST_UNSUPPORTED = pgp.ST_OK, pgp.ST_BAD_SIG, pgp.ST_UNSUPPORTED


def size_class(bits: int) -> Optional[int]:
    return 0 if bits <= 2048 else 1 if bits <= 3072 else 2 if bits <= MAX_BITS else None


def value_cap(bits: int) -> int:
    """R of the class in bytes: 76, 112 and 152 limbs of 28 bits."""
    return (266, 392, 532)[size_class(bits)]


def t_len(hash_name: str) -> int:
    return len(pgp.HASH_PREFIXES[hash_name]) + hashlib.new(hash_name).digest_size


@dataclass
class Case:
    key: int                   # index into keys()
    bits: int
    hash_id: int
    variant: str
    tbs: bytes
    sig: bytes                 # one signature packet
    fits: bool                 # k >= tLen + 11: an encoding exists
    over_cap: bool = False     # the value is longer than the class's R


@functools.lru_cache(maxsize=None)
def keys() -> List[cb.KeyPair]:
    out = []
    for bits, cnt in SIZES:
        for i, mat in enumerate(load_keys("rsa%d" % bits, cnt)):
            out.append(cb.make_keypair(cb.PK_RSA, mat, "rsa%d-%d <k@bftkv.example>" % (bits, i)))
            assert out[-1].n.bit_length() == bits and out[-1].e == 65537
    for kind in SMALL_EXPONENT_KEYS:
        out.append(cb.make_keypair(cb.PK_RSA, load_keys(kind, 1)[0], "%s <k@bftkv.example>" % kind))
        assert "rsa%de%d" % (out[-1].n.bit_length(), out[-1].e) == kind
    assert len({kp.key_id for kp in out}) == len(out)
    return out


def entity(kp: cb.KeyPair) -> pgp.Entity:
    """The oracle's view of a bare primary key (no self-signature: the short keys cannot make one)."""
    return pgp.Entity(primary=pgp.PublicKey(key_id=kp.key_id, pk_algo=cb.PK_RSA, n=kp.n, e=kp.e), name=kp.name)


def digest_of(kp: cb.KeyPair, tbs: bytes, hash_id: int) -> Tuple[bytes, bytes]:
    """(first bytes of the signature body, digest) of a binary v4 signature by ``kp`` over ``tbs``"""
    prefix = cb.sig_prefix(0x00, cb.PK_RSA, cb._hashed_area(kp.key_id), hash_id)
    return prefix, hashlib.new(dict(HASHES)[hash_id], tbs + cb.hash_suffix(prefix)).digest()


def encode(k: int, hash_name: str, digest: bytes) -> bytes:
    """EMSA-PKCS1-v1_5 in k bytes; where k < tLen + 11 there is none: the low k bytes of the shortest one."""
    t = pgp.HASH_PREFIXES[hash_name] + digest
    return (b"\x00\x01" + b"\xff" * max(0, k - len(t) - 3) + b"\x00" + t)[-k:]


def packet(prefix: bytes, digest: bytes, mpi: bytes) -> bytes:
    body = prefix + b"\x00\x00" + digest[:2] + mpi
    return cb._hdr(2, len(body)) + body


def go_mpi(value: int, nbytes: int) -> bytes:
    return cb.go_mpi_bytes(value.to_bytes(nbytes, "big"))


def tampered_encodings(k: int, hash_name: str, digest: bytes) -> Dict[str, bytes]:
    """Wrong encodings to be signed with the private key, so that s^e mod n itself is the wrong message."""
    prefix = pgp.HASH_PREFIXES[hash_name]
    tl = len(prefix) + len(digest)
    em = encode(k, hash_name, digest)
    out = {}

    def put(name, at_from_low, value):            # byte ``at_from_low`` counted from the least significant one
        b = bytearray(em)
        b[k - 1 - at_from_low] = value
        out[name] = bytes(b)
    put("em 00 02", k - 2, 0x02)
    for name, at in (("em FE above byte 84", EM_LOW_BYTES), ("em FE below byte 84", EM_LOW_BYTES - 1)):
        if tl + 1 <= at <= k - 3:                  # the padding runs from byte tLen + 1 to byte k - 3
            assert em[k - 1 - at] == 0xFF
            put(name, at, 0xFE)
    put("em separator FF", tl, 0xFF)
    same_len = {"sha224": "sha256", "sha256": "sha384", "sha384": "sha512", "sha512": "sha224"}
    other = pgp.HASH_PREFIXES[same_len[hash_name]] if hash_name in same_len else bytes([prefix[0], prefix[1] ^ 1]) + prefix[2:]
    assert len(other) == len(prefix) and other != prefix
    out["em other prefix"] = em[:k - tl] + other + digest
    return out


def cell_cases(ki: int, kp: cb.KeyPair, hash_id: int, tbs: bytes, tamper_pick: Optional[int]) -> List[Case]:
    """All variants of one (key, hash) cell.  ``tamper_pick``: sign only that one of the tampered encodings (the big keys)."""
    bits = kp.n.bit_length()
    k = (bits + 7) // 8
    name = dict(HASHES)[hash_id]
    fits = k >= t_len(name) + 11
    prefix, digest = digest_of(kp, tbs, hash_id)
    n = kp.n
    s = kp.rsa_private(int.from_bytes(encode(k, name, digest), "big") % n)
    out: List[Case] = []

    def add(variant, mpi, **kw):
        out.append(Case(ki, bits, hash_id, variant, tbs, packet(prefix, digest, mpi), fits, **kw))
    add("untouched", go_mpi(s, k))
    add("canonical mpi", cb._mpi(s))
    if s + n < 1 << (8 * k):
        add("s + n", go_mpi(s + n, k))
    else:
        add("s + n, long", go_mpi(s + n, k + 1))
    if bits <= MAX_BITS:
        # s + j n filling the class's R to the last byte, and one byte beyond it (under a modulus too short for the hash only the
        # latter: refused like everything else there, and for that reason not fenced)
        cap = value_cap(bits)
        for variant, nb in (("at the cap", cap), ("over the cap", cap + 1))[0 if fits else 1:]:
            v = s + ((1 << (8 * nb)) - 1 - s) // n * n
            assert v % n == s and v >> (8 * nb - 8) != 0
            add(variant, go_mpi(v, nb), over_cap=nb > cap)
    flip = (7 * bits + 13 * hash_id) % (bits - 1)
    add("bit flipped", go_mpi(s ^ (1 << flip), k))
    if fits and bits <= MAX_BITS:
        tampered = sorted(tampered_encodings(k, name, digest).items())
        if tamper_pick is not None:
            tampered = [tampered[tamper_pick % len(tampered)]]
        for variant, em in tampered:
            v = int.from_bytes(em, "big")
            assert v < n
            add(variant, go_mpi(kp.rsa_private(v), k))
    return out


@functools.lru_cache(maxsize=None)
def cases() -> List[Case]:
    """The matrix: every key x five hashes x the variants.  Keys of 2041 bits and more sign one tampered encoding per cell instead
    of all (Python signing time), a different one from cell to cell."""
    out: List[Case] = []
    cell = 0
    for ki, kp in enumerate(keys()):
        for hash_id, _ in HASHES:
            tbs = b"rsa sizes: key %d, hash %d " % (ki, hash_id) + bytes(range(cell % 61))
            out += cell_cases(ki, kp, hash_id, tbs, cell if kp.n.bit_length() > 2040 else None)
            cell += 1
    return out


def oracle_status(keyring: List[pgp.Entity], c: Case) -> int:
    r = pgp.check_detached_signature(keyring, c.tbs, c.sig, 0)
    assert r.pos == len(c.sig) and r.statuses == [r.status]
    return r.status


def device_expectation(c: Case, oracle_st: int) -> Tuple[int, bool]:
    """(status, fenced) the device must report where the oracle reports ``oracle_st``: the oracle's own, but for the two fences --
    a key above 4096 bits (ST_UNSUPPORTED) and a value longer than R under a modulus long enough for the hash (ST_BAD_SIG); the
    caller takes the reference path for a fenced item."""
    if c.bits > MAX_BITS:
        return ST_UNSUPPORTED, True
    if c.over_cap:
        return ST_BAD_SIG, c.fits            # k < tLen + 11 comes first: the reference refuses whatever the value, no fence needed
    return oracle_st, False
