"""The corpus of the RSA-signing tests (CPU: tests/test_rsa_sign_reference.py; GPU: tests/test_gpu_rsa_sign.py).  Seeded; not collected.

One signer set of 256-byte moduli and 128-byte private parts holds every key:
  good        corpus.keys.gen_rsa keys of 128, 496, 1024, 2047 and 2048 bits, one unbalanced key (p of 1024 bits, q of 520), the
              known-answer key of tests/golden/threshold_kat.json (p and q recovered from (n, e, d)), and two keys over extremal primes;
  refused     even n, even p, even q, p = 1 -- of the 496-bit and of the 2048-bit key each, so that SHA-384 / SHA-512 under the small
              one meets the length rule first;
  broken      dq + 1, qinv + 1, n + 2, e + 2, p and q (with dp and dq) swapped without a new qinv -- of the 1024-bit and the 2048-bit key.
The extremal primes: tests/golden/extremal_moduli.json holds the all-ones and the 2^k + small form at 2048 bits and above, too wide
for a p or q of a 2048-bit key; the same two forms at 1024 bits are 2^1024 - {105, 179} and 2^1023 + {1155, 1493} (the first two primes
of each form; the CPU suite tests them for primality)."""
import functools
import hashlib
import json
import math
import os
import random

import rsa_sign_ref as R
import rsa_verify_ref as V
from corpus import keys as CK

HERE = os.path.dirname(os.path.abspath(__file__))
NBYTES, PBYTES = 256, 128
SIZES = (128, 496, 1024, 2047, 2048)
FULL_PRIMES = ((1 << 1024) - 105, (1 << 1024) - 179)
SPARSE_PRIMES = ((1 << 1023) + 1155, (1 << 1023) + 1493)
# (hash_id, dlen): all eight hash ids; hash_id 0 at the 128-bit key's last accepted length, the first refused one and the longest
SHAPES = ((0, 5), (0, 6), (0, 64), (1, 16), (2, 20), (3, 20), (8, 32), (9, 48), (10, 64), (11, 28))
REFUSED_KINDS = ("even_n", "even_p", "even_q", "p_one")
BROKEN_KINDS = ("dq+1", "qinv+1", "n+2", "e+2", "swapped")


@functools.lru_cache(maxsize=None)
def kat():
    k = json.load(open(os.path.join(HERE, "golden", "threshold_kat.json")))["rsa"]
    return dict(n=int(k["n"], 16), e=int(k["e"]), d=int(k["d"], 16), tbs=k["tbs"].encode(), sig=int(k["sha256_pkcs1v15_sig"], 16))


def _from_primes(p, q):
    for e in (65537, 17, 3, 5, 257):
        if math.gcd(e, (p - 1) * (q - 1)) == 1:
            return R.key_from_primes(p, q, e)
    raise ValueError("no exponent")


def _gen(bits):
    k = CK.gen_rsa(0, bits=bits) if bits == 128 else CK.load_keys("rsa%d" % bits, 1)[0]
    return R.key_from_primes(k["p"], k["q"], k["e"])


def _refuse(key, kind):
    if kind == "even_n":
        return key._replace(n=key.n - 1)
    if kind == "even_p":
        return key._replace(p=key.p + 1)
    if kind == "even_q":
        return key._replace(q=key.q + 1)
    return key._replace(p=1)


def _break(key, kind):
    if kind == "dq+1":
        return key._replace(dq=key.dq + 1)
    if kind == "qinv+1":
        return key._replace(qinv=key.qinv + 1)
    if kind == "n+2":
        return key._replace(n=key.n + 2)
    if kind == "e+2":
        return key._replace(e=key.e + 2)
    return key._replace(p=key.q, q=key.p, dp=key.dq, dq=key.dp)


@functools.lru_cache(maxsize=None)
def keys():
    """[(tag, Key)] in the set's order"""
    out = [("rsa%d" % b, _gen(b)) for b in SIZES]
    rng = CK.DRBG("rsa-sign-unbalanced", CK.MASTER_SEED, 1024, 520)
    out.append(("unbalanced", _from_primes(CK.gen_prime(1024, rng), CK.gen_prime(520, rng))))
    k = kat()
    p, q = R.recover_primes(k["n"], k["e"], k["d"])
    out.append(("kat", R.Key(k["n"], k["e"], p, q, k["d"] % (p - 1), k["d"] % (q - 1), pow(q, -1, p))))
    out.append(("full", _from_primes(*FULL_PRIMES)))
    out.append(("sparse", _from_primes(*SPARSE_PRIMES)))
    by = dict(out)
    for base in ("rsa496", "rsa2048"):
        out += [("refused:%s:%s" % (kind, base), _refuse(by[base], kind)) for kind in REFUSED_KINDS]
    for base in ("rsa1024", "rsa2048"):
        out += [("broken:%s:%s" % (kind, base), _break(by[base], kind)) for kind in BROKEN_KINDS]
    return out


def good_keys():
    return [(i, t, k) for i, (t, k) in enumerate(keys()) if ":" not in t]


def key_dicts(ks=None):
    """what Context.rsa_signer_create takes"""
    return [k._asdict() for _, k in (keys() if ks is None else ks)]


def digest(hash_id, dlen, tag):
    return hashlib.shake_128(b"rsa-sign %d %d %s" % (hash_id, dlen, tag.encode())).digest(dlen)


@functools.lru_cache(maxsize=None)
def call(hash_id, dlen):
    """(digests, key_idx) of the corpus call of one shape: every key once, the good ones three more times, shuffled"""
    rows = [(i, digest(hash_id, dlen, "%d/0" % i)) for i in range(len(keys()))]
    rows += [(i, digest(hash_id, dlen, "%d/%d" % (i, r))) for i, _, _ in good_keys() for r in (1, 2, 3)]
    random.Random(hash_id * 100 + dlen).shuffle(rows)
    return [d for _, d in rows], [i for i, _ in rows]


@functools.lru_cache(maxsize=None)
def expected(hash_id, dlen):
    """[(status, signature bytes)] of that call"""
    ks = keys()
    return [(st, s.to_bytes(NBYTES, "big")) for st, s in (_sign(i, hash_id, d) for d, i in zip(*call(hash_id, dlen)))]


@functools.lru_cache(maxsize=None)
def _sign(i, hash_id, d):
    return R.sign(keys()[i][1], hash_id, d, NBYTES)


def _crt_of(key, m1, m2):
    """c whose two powers are m1 mod p and m2 mod q, for a consistent key"""
    m = m2 + (m1 - m2) * key.qinv % key.p * key.q
    return pow(m, key.e, key.n)


@functools.lru_cache(maxsize=None)
def selftest_ops():
    """[(key index, class, c)] over the good keys"""
    ops = []
    for i, tag, k in good_keys():
        lo = min(k.p, k.q)
        t = int.from_bytes(hashlib.sha256(tag.encode()).digest(), "big") % (lo - 8) + 4
        ops += [(i, "zero", 0), (i, "one", 1), (i, "p", k.p), (i, "q", k.q), (i, "n-1", k.n - 1), (i, "n", k.n), (i, "all_ones", (1 << (8 * NBYTES)) - 1),
                (i, "m1<m2", _crt_of(k, t, t + 3)), (i, "m1=m2", _crt_of(k, t, t)), (i, "diff+1", _crt_of(k, t + 1, t)), (i, "diff-1", _crt_of(k, t, t + 1)),
                (i, "0 mod p only", 2 * k.p), (i, "0 mod q only", 3 * k.q), (i, "wide", (k.n << 7) + t if k.n.bit_length() <= 8 * NBYTES - 8 else k.n + t)]
    return ops


@functools.lru_cache(maxsize=None)
def selftest_expected():
    return [R.selftest(keys()[i][1], c, NBYTES) for i, _, c in selftest_ops()]


# ---- the small set of the launch-splitting test: the 128-bit key alone, 16-byte rows, 8-byte private parts ---------------------------
def small_key():
    return keys()[0][1]
