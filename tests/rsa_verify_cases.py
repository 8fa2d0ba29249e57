"""The seeded corpus of raw RSA PKCS#1 v1.5 verification, shared by tests/test_rsa_verify_reference.py (the restatement against
the oracle and OpenSSL) and the GPU tests (the device against the restatement).  Not collected.

Keys: every tests/golden/keys_rsa*.json of at most 2048 bits (the first key of each), their own e (3, 17, 65537) and, over the same
p and q, further odd exponents coprime to phi (the first that fits from short lists around 7, 65539 and 2^32 - 1, with d from p
and q) and the verify-only exponents 0, 1, 2 and 65536.  Hashes: the seven OpenPGP ids and hash id 0 (no prefix) at dlen 1, 36, 64.

A case is (label, part, n, e, hash_id, digest, s); s is ANY integer below 2^2048 and min_nbytes says how many bytes carry it."""
from __future__ import annotations

import functools
import glob
import json
import os
import re
import zlib
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

import rsa_verify_ref as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_BITS, MAX_NBYTES = 2048, 256
HASH_CELLS: List[Tuple[int, int]] = [(h, V.DLEN[h]) for h in (1, 2, 3, 8, 9, 10, 11)] + [(0, 1), (0, 36), (0, 64)]
ODD_LISTS = [(7, 5, 11, 13), (65539, 65543, 65541, 65537 + 12), (2**32 - 1, 2**32 - 3, 2**32 - 5, 2**32 - 7, 2**32 - 9, 2**32 - 11)]
VERIFY_ONLY = (0, 1, 2, 65536)


@dataclass(frozen=True)
class Key:
    name: str
    p: int
    q: int
    e: int

    @property
    def n(self):
        return self.p * self.q

    @property
    def k(self):
        return (self.n.bit_length() + 7) // 8

    def d(self, e=None):
        return pow(self.e if e is None else e, -1, (self.p - 1) * (self.q - 1))


@dataclass(frozen=True)
class Case:
    label: str
    part: str          # honest | mutation | forgery | small_m | value | wide | exponent | key
    key: str
    n: int
    e: int
    hash_id: int
    digest: bytes
    s: int

    @property
    def min_nbytes(self):
        return max(1, (self.n.bit_length() + 7) // 8, (self.s.bit_length() + 7) // 8)


@functools.lru_cache(maxsize=None)
def keys() -> Tuple[Key, ...]:
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "keys_rsa*.json"))):
        name = os.path.basename(path)[5:-5]
        if int(re.match(r"rsa(\d+)", name).group(1)) > MAX_BITS:
            continue
        k = json.load(open(path))["keys"][0]
        out.append(Key(name, int(k["p"], 16), int(k["q"], 16), int(k["e"], 16)))
    return tuple(sorted(out, key=lambda k: (k.n.bit_length(), k.name)))


def key(name: str) -> Key:
    return next(k for k in keys() if k.name == name)


def extra_exponents(K: Key) -> List[int]:
    """The first exponent of each list that is coprime to phi."""
    import math
    phi = (K.p - 1) * (K.q - 1)
    return [next(e for e in lst if math.gcd(e, phi) == 1) for lst in ODD_LISTS]


def _flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    a = bytearray(b)
    a[byte] ^= 1 << bit
    return bytes(a)


def _rng(*parts) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


@functools.lru_cache(maxsize=None)
def cell(name: str, hash_id: int, dlen: int) -> Tuple[Case, ...]:
    """The cases of one (key, hash) cell."""
    K = key(name)
    n, e, k = K.n, K.e, K.k
    rng = _rng(name, hash_id, dlen)
    dg = rng.bytes(dlen)
    plen = len(V.PREFIX[hash_id])
    out: List[Case] = []

    def add(label, part, s, digest=dg, n_=n, e_=e):
        out.append(Case(label, part, name, n_, e_, hash_id, digest, s))

    fits = k >= plen + dlen + 11
    if fits:
        d = K.d()
        EM = V.em(k, hash_id, dg)
        s0 = pow(int.from_bytes(EM, "big"), d, n)
        add("honest", "honest", s0)
        add("honest, digest bit flipped", "mutation", s0, digest=_flip(dg, int(rng.integers(dlen)), int(rng.integers(8))))
        ff0, ffn = 2, k - plen - dlen - 2            # first and last FF
        regions = [("00 top", 0), ("01", 1), ("first FF", ff0), ("middle FF", (ff0 + ffn) // 2), ("last FF", ffn), ("00 separator", ffn + 1),
                   ("first digest byte", k - dlen), ("last digest byte", k - 1)]
        if plen:
            regions += [("first prefix byte", ffn + 2), ("last prefix byte", ffn + 1 + plen)]
        for lb, pos in regions:
            # (the 00 top: the bit just below n's own top bit, so that the forgery stays below n; none when n's top byte is 01)
            bit = n.bit_length() - 8 * (k - 1) - 2 if pos == 0 else int(rng.integers(8))
            if bit < 0:
                continue
            bad = int.from_bytes(_flip(EM, pos, bit), "big")
            if bad < n:
                add("forged EM: " + lb, "forgery", pow(bad, d, n))
        for lb, m in (("0", 0), ("1", 1), ("2", 2), ("n - 1", n - 1)):
            add("m^d, m = " + lb, "small_m", pow(m, d, n))
        # value shapes: s >= n is reduced
        for lb, s in (("s = 0", 0), ("s = n - 1", n - 1), ("s = n", n), ("s = n + 1", n + 1), ("s = 2^2048 - 1", (1 << 8 * MAX_NBYTES) - 1),
                      ("s = 2^(8k) - 1", (1 << 8 * k) - 1)):
            add(lb, "value", s)
        add("valid s + n", "wide", s0 + n)
        j = int(rng.integers(1, 8 * MAX_NBYTES - n.bit_length() + 1)) if n.bit_length() < 8 * MAX_NBYTES else 0
        if j:
            add("valid s + n 2^%d" % j, "wide", s0 + (n << j))
            add("valid s + n 2^top", "wide", s0 + (n << (8 * MAX_NBYTES - n.bit_length())))
    else:
        add("random s under a short modulus", "mutation", int.from_bytes(rng.bytes(k), "big"))
        add("s = 1 under a short modulus", "value", 1)
    # key shapes (rows 1 and 2 come before any arithmetic)
    s_any = out[0].s
    for lb, nn in (("n - 1 (even)", n - 1), ("n + 1 (even)", n + 1), ("n = 0", 0), ("n = 1", 1)):
        add("key: " + lb, "key", s_any if nn else 5, n_=nn)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exponent_cases(name: str) -> Tuple[Case, ...]:
    """Further exponents over the same p and q, at SHA-256 where the modulus carries it, else without a prefix at one digest byte."""
    K = key(name)
    n, k = K.n, K.k
    hash_id, dlen = (8, 32) if k >= 19 + 32 + 11 else (0, 1)
    rng = _rng(name, "exponents")
    dg = rng.bytes(dlen)
    EM = V.em(k, hash_id, dg)
    m = int.from_bytes(EM, "big")
    out = []
    for e in extra_exponents(K):
        s = pow(m, K.d(e), n)
        out.append(Case("e = %d honest" % e, "exponent", name, n, e, hash_id, dg, s))
        out.append(Case("e = %d honest + n" % e, "exponent", name, n, e, hash_id, dg, s + n))
        out.append(Case("e = %d, digest bit flipped" % e, "exponent", name, n, e, hash_id, _flip(dg, 0), s))
    s0 = pow(m, K.d(), n)
    for e in VERIFY_ONLY:
        out.append(Case("e = %d, the honest signature of e = %d" % (e, K.e), "exponent", name, n, e, hash_id, dg, s0))
        out.append(Case("e = %d, s = EM" % e, "exponent", name, n, e, hash_id, dg, m))          # e = 1: a positive case without a private key
        out.append(Case("e = %d, s = EM + n" % e, "exponent", name, n, e, hash_id, dg, m + n))
        out.append(Case("e = %d, s = 1" % e, "exponent", name, n, e, hash_id, dg, 1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def corpus(hash_id: int, dlen: int) -> Tuple[Case, ...]:
    """Every case of one (hash_id, dlen): what one device call takes."""
    out: List[Case] = []
    for K in keys():
        out += cell(K.name, hash_id, dlen)
        out += [c for c in exponent_cases(K.name) if (c.hash_id, len(c.digest)) == (hash_id, dlen)]
    return tuple(out)


def everything() -> List[Case]:
    return [c for h, dl in HASH_CELLS for c in corpus(h, dl)]


def call_arrays(cases, nbytes: int):
    """(digests, sigs, keys [(n, e)], key_idx) of one call over `cases` at nbytes per signature and modulus."""
    slot, klist, idx = {}, [], []
    for c in cases:
        kk = (c.n, c.e)
        if kk not in slot:
            slot[kk] = len(klist)
            klist.append(kk)
        idx.append(slot[kk])
    return [c.digest for c in cases], [c.s.to_bytes(nbytes, "big") for c in cases], klist, np.array(idx, dtype=np.uint32)


def expected(cases):
    want = [V.verify(c.n, c.e, c.hash_id, c.digest, c.s) for c in cases]
    return np.array([w[0] for w in want], dtype=np.uint8), np.array([w[1] for w in want], dtype=np.uint8)
