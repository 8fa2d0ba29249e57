"""A plain-Python restatement of Go 1.13's rsa.SignPKCS1v15 on raw inputs with the rules of docs/parity.md ("RSA signing
(rsa.SignPKCS1v15)"), for the RSA-signing tests.  Not collected.

    sign(key, hash_id, digest, nbytes) -> (status, s)           s = 0 unless status is OK
    selftest(key, c, nbytes)           -> (status, m2 + h q)    the CRT path alone, on any c

A key is a Key of ints; dp, dq and qinv are taken as given.  The rows, in this order, with k = ceil(bits(n) / 8) and tLen =
len(prefix) + len(digest):
  1. k < tLen + 11 (n = 0 and n = 1 included): INVALID_INPUT (Go: ErrMessageTooLong), whatever the key's state;
  2. the key was refused at registration (n even; p or q even or below 3): FENCED;
  3. s = m2 + h q with m1 = em^dp mod p, m2 = em^dq mod q, h = (m1 - m2) qinv mod p (rsa.decrypt's precomputed branch); s^e mod n != em,
     or s does not fit nbytes: CHECK_FAILED (Go: "rsa: internal error");
  4. otherwise OK."""
import collections
import math

import rsa_verify_ref as V

OK, FENCED, INVALID_INPUT, CHECK_FAILED, FAILED = 0, 2, 3, 4, 0xFF
W, N_LIMBS, VALUE_LIMBS = 28, 40, 80

Key = collections.namedtuple("Key", "n e p q dp dq qinv")


def key_from_primes(p, q, e=65537):
    d = pow(e, -1, math.lcm(p - 1, q - 1))
    return Key(p * q, e, p, q, d % (p - 1), d % (q - 1), pow(q, -1, p))


def recover_primes(n, e, d):
    """p > q of n from (e, d): a square root of 1 other than +-1 splits n."""
    t, s = e * d - 1, 0
    while t % 2 == 0:
        t, s = t // 2, s + 1
    for a in range(2, 200):
        x = pow(a, t, n)
        for _ in range(s):
            y = x * x % n
            if y == 1 and x not in (1, n - 1):
                p = math.gcd(x - 1, n)
                return max(p, n // p), min(p, n // p)
            x = y
    raise ValueError("no split found")


def key_refused(key):
    return key.n % 2 == 0 or any(m % 2 == 0 or m < 3 for m in (key.p, key.q))


def kbytes(n):
    return (n.bit_length() + 7) // 8


def rule(key, hash_id, dlen):
    if kbytes(key.n) < len(V.PREFIX[hash_id]) + dlen + 11:
        return INVALID_INPUT
    return FENCED if key_refused(key) else OK


def crt(key, c):
    m1, m2 = pow(c % key.p, key.dp, key.p), pow(c % key.q, key.dq, key.q)
    return m2 + (m1 - m2) * key.qinv % key.p * key.q


def sign(key, hash_id, digest, nbytes):
    r = rule(key, hash_id, len(digest))
    if r != OK:
        return r, 0
    em = int.from_bytes(V.em(kbytes(key.n), hash_id, digest), "big")
    s = crt(key, em)
    if s >= 1 << (8 * nbytes) or pow(s, key.e, key.n) != em:
        return CHECK_FAILED, 0
    return OK, s


def selftest(key, c, nbytes):
    if key_refused(key):
        return FENCED, 0
    s = crt(key, c)
    return (OK, s) if s < 1 << (8 * nbytes) else (CHECK_FAILED, 0)


# ---- what rsa_sign.h states without a multiplier -------------------------------------------------------------------------------------
def value_limbs(v):
    return [(v >> (W * j)) & ((1 << W) - 1) for j in range(VALUE_LIMBS)]


def em_limbs(n, hash_id, digest):
    """(rule by the length alone, the 80 limbs of em: zero where the length rule refuses)"""
    k = kbytes(n)
    if k < len(V.PREFIX[hash_id]) + len(digest) + 11:
        return INVALID_INPUT, [0] * VALUE_LIMBS
    return OK, value_limbs(int.from_bytes(V.em(k, hash_id, digest), "big"))


def digits(d, pbytes):
    """the chain's windows, most significant first"""
    return [(d >> (4 * w)) & 15 for w in range(2 * pbytes - 1, -1, -1)]


def status(rule_byte, fits, check_ok):
    return rule_byte if rule_byte != OK else (OK if fits and check_ok else CHECK_FAILED)
