"""The seeded corpus of the ECDSA-verification tests (CPU and GPU).  Not collected.

    corpus(name) -> [Case]      Case = (label, group, key, digest, sig, expect)

group is one of "honest", "mutation", "keyflip", "boundary", "constructed", "special_x"; expect is "valid", "invalid", "fenced" where the
construction fixes the answer, else None (the restatement decides).  Every digest length of the corpus is one of DLENS, so a
test can hand the cases of one length to one device call."""
import functools
from collections import namedtuple

import numpy as np

import ec_ref as E
import ecdsa_verify_ref as V

Case = namedtuple("Case", "label group key digest sig expect")
DLENS = (20, 28, 32, 48, 64, 66)


def rnd(rng, c, m=None):
    return int.from_bytes(rng.bytes(E.byte_len(c) + 8), "big") % (m or c["n"])


def sig_bytes(c, r: int, s: int) -> bytes:
    f = E.byte_len(c)
    return r.to_bytes(f, "big") + s.to_bytes(f, "big")


def digest_for(c, e: int) -> bytes:
    """A digest of fbytes bytes whose hashToInt is e (e < 2^bit_size)."""
    f = E.byte_len(c)
    return (e << (8 * f - c["n"].bit_length())).to_bytes(f, "big")


def sign(c, d: int, digest: bytes, k: int):
    """An honest signature: ecdsa_sign_hash_int on the truncated hash integer."""
    return E.ecdsa_sign_hash_int(c, d, V.hash_to_int(c, digest) % c["n"], k)


def sqrt_mod(a: int, p: int):
    """Tonelli-Shanks (P-224's p is 1 mod 4; the other primes are 3 mod 4 and take the first branch).  None: not a square."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, cc, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        b = pow(cc, 1 << (m - i - 1), p)
        m, cc, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


def point_sub(c, a, b):
    nb = E.point_neg(c, b)
    if a == nb:
        return E.affine_from_jacobian(c, *E.double_jacobian(c, *a, 1))
    return E.add(c, *a, *nb)


def flip(b: bytes, bit: int) -> bytes:
    out = bytearray(b)
    out[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def corpus(name: str):
    c = E.CURVES[name]
    n, p, f = c["n"], c["p"], E.byte_len(c)
    rng = np.random.default_rng(20260 + c["bit_size"])
    d1, d2 = rnd(rng, c), rnd(rng, c)
    q1, q2 = E.scalar_base_mult(c, d1), E.scalar_base_mult(c, d2)
    k1, k2 = E.marshal(c, *q1), E.marshal(c, *q2)
    cases = []
    honest = {}
    for dlen in DLENS:
        for j in range(2):
            dg = rng.bytes(dlen)
            r, s = sign(c, d1, dg, rnd(rng, c))
            cases.append(Case(f"honest dlen={dlen} #{j}", "honest", k1, dg, sig_bytes(c, r, s), "valid"))
            honest[dlen] = (dg, r, s)
    # single-bit flips of an honest signature, per digest length 20, 32 and 66
    for dlen in (20, 32, 66):
        dg, r, s = honest[dlen]
        sg = sig_bytes(c, r, s)
        eff = min(dlen, f)       # digest bits that reach e (a flip beyond them changes nothing: still VALID)
        for j in range(3):
            # r or s may leave [1, N) by the flip: the restatement decides
            cases.append(Case(f"flip r dlen={dlen} #{j}", "mutation", k1, dg, flip(sg, int(rng.integers(8 * f))), None))
            cases.append(Case(f"flip s dlen={dlen} #{j}", "mutation", k1, dg, flip(sg, 8 * f + int(rng.integers(8 * f))), None))
            lo = 8 * eff - c["n"].bit_length() if 8 * eff > c["n"].bit_length() else 0
            cases.append(Case(f"flip digest dlen={dlen} #{j}", "mutation", k1, flip(dg, int(rng.integers(8 * eff - lo))), sg, "invalid"))
            cases.append(Case(f"flip key X dlen={dlen} #{j}", "keyflip", flip(k1, 8 + int(rng.integers(8 * f))), dg, sg, None))
        cases.append(Case(f"another key dlen={dlen}", "mutation", k2, dg, sg, "invalid"))
        if dlen > f:
            cases.append(Case(f"flip beyond the order's bytes dlen={dlen}", "honest", k1, flip(dg, 8 * f + 3), sg, "valid"))
    dg, r, s = honest[32]
    ff = (1 << (8 * f)) - 1
    for label, rr, ss in (("r = 0", 0, s), ("s = 0", r, 0), ("r = N", n, s), ("s = N", r, n), ("r = 0xFF..", ff, s), ("s = 0xFF..", r, ff),
                          ("r = s = 0", 0, 0)):
        cases.append(Case(label, "boundary", k1, dg, sig_bytes(c, rr, ss), "invalid"))
    if n + r <= ff:
        cases.append(Case("r = N + valid r", "boundary", k1, dg, sig_bytes(c, n + r, s), "invalid"))
    cases.append(Case("bad key and r = 0", "keyflip", b"\x02" + k1[1:], dg, sig_bytes(c, 0, s), "fenced"))
    for label, kb in (("key prefix 02", b"\x02" + k1[1:]), ("key y + 1", E.marshal(c, q1[0], (q1[1] + 1) % p)), ("key x = P", E.marshal(c, p, q1[1])),
                      ("key (0, 0)", E.marshal(c, 0, 0))):
        cases.append(Case(label, "keyflip", kb, dg, sig_bytes(c, r, s), "fenced"))
    # e above N: the leftmost bytes all ones (P-224 with a 32-byte digest is the issue's example; the same digest on every curve)
    dg = b"\xff" * 16 + rng.bytes(16)
    assert name != "P-224" or V.hash_to_int(c, dg) >= n
    r_, s_ = sign(c, d1, dg, rnd(rng, c))
    cases.append(Case("e from a digest of leading ones", "honest", k1, dg, sig_bytes(c, r_, s_), "valid"))
    # ---- constructed cases (the key is ours to choose: no discrete logarithm needed) -------------------------------
    # x(R) >= N: R = (x, y) with x in [N, p), Q = b^-1 (R - a G), r = x - N, s = r / b, e = a s
    for j in range(2):
        while True:
            x = n + 1 + rnd(rng, c, p - n - 1)
            y = sqrt_mod(x * x * x - 3 * x + c["b"], p)
            if y is not None:
                break
        a, b = rnd(rng, c) or 1, rnd(rng, c) or 1
        rpt = point_sub(c, (x, y), E.scalar_base_mult(c, a))
        q = E.scalar_mult(c, rpt[0], rpt[1], E.int_bytes(pow(b, -1, n)))
        r = x - n
        s = r * pow(b, -1, n) % n
        cases.append(Case(f"x(R) >= N #{j}", "constructed", E.marshal(c, *q), digest_for(c, a * s % n), sig_bytes(c, r, s), "valid"))
        cases.append(Case(f"x(R) >= N, r + 1 #{j}", "constructed", E.marshal(c, *q), digest_for(c, a * s % n), sig_bytes(c, r + 1, s), "invalid"))
    # equal: u1 G = u2 Q  (u1 = k / 2, u2 = k / (2 d))
    k = rnd(rng, c) or 1
    u1, u2 = k * pow(2, -1, n) % n, k * pow(2 * d1, -1, n) % n
    r = E.scalar_base_mult(c, k)[0] % n
    s = r * pow(u2, -1, n) % n
    cases.append(Case("u1 G = u2 Q", "constructed", k1, digest_for(c, u1 * s % n), sig_bytes(c, r, s), "fenced"))
    # opposite: u1 G = -u2 Q
    u2 = rnd(rng, c) or 1
    u1 = -u2 * d1 % n
    r = rnd(rng, c) or 1
    s = r * pow(u2, -1, n) % n
    cases.append(Case("u1 G = -u2 Q", "constructed", k1, digest_for(c, u1 * s % n), sig_bytes(c, r, s), "invalid"))
    # e = 0: an all-zero digest honestly signed
    for dlen in (32, f):
        dg = bytes(dlen)
        r, s = sign(c, d1, dg, rnd(rng, c))
        cases.append(Case(f"e = 0 dlen={dlen}", "constructed", k1, dg, sig_bytes(c, r, s), "fenced"))
    cases.append(Case("e = N", "constructed", k1, digest_for(c, n), sig_bytes(c, *E.ecdsa_sign_hash_int(c, d1, 0, rnd(rng, c))), "fenced"))
    return tuple(cases) + special_x(name)


def special_x(name: str):
    """The group "special_x", behind everything else and from a generator of its own: valid signatures whose R = u1 G + u2 Q is each
    special-x point of tests/ec_form_cases.py (smallest and largest x, Montgomery-form x next to p - 1 and to 2^(32 L - 1)), built as
    the constructed cases above (Q = b^-1 (R - a G), r = x mod N, s = r / b, e = a s), and the same signatures with r + 1.  Where the
    smallest x is 0 (P-256, P-384, P-521) r = 0 and no valid signature exists: the case stands as INVALID, and its r + 1 twin
    (s = 1 / b) is the one that takes x(R) = 0 through the comparison."""
    import ec_form_cases as F           # (it imports this module for sqrt_mod)
    c = E.CURVES[name]
    n = c["n"]
    rng = np.random.default_rng(30260 + c["bit_size"])
    cases = []
    for label, (x, y) in F.special_x_points(name):
        a, b = rnd(rng, c) or 1, rnd(rng, c) or 1
        rpt = point_sub(c, (x, y), E.scalar_base_mult(c, a))
        q = E.scalar_mult(c, rpt[0], rpt[1], E.int_bytes(pow(b, -1, n)))
        r = x % n
        s = (r or 1) * pow(b, -1, n) % n            # (r = 0: with r + 1 = 1 the device still computes that R, and x(R) = 0 is not 1)
        dg = digest_for(c, a * s % n)
        cases.append(Case(f"R of {label}", "special_x", E.marshal(c, *q), dg, sig_bytes(c, r, s), "valid" if r else "invalid"))
        cases.append(Case(f"R of {label}, r + 1", "special_x", E.marshal(c, *q), dg, sig_bytes(c, r + 1, s), "invalid"))
    return tuple(cases)


def by_dlen(cases):
    out = {}
    for i, cs in enumerate(cases):
        out.setdefault(len(cs.digest), []).append(i)
    return out
