"""A plain-Python restatement of Go 1.13's crypto/dsa.Verify with the rules of docs/parity.md ("DSA verification"), for the
DSA-verification tests.  Not collected.

    verify(p, q, g, y, digest, r, s) -> (valid, status)

The rows, in this order:
  1. r = 0, r >= q, s = 0 or s >= q: (0, OK);
  2. bits(q) no multiple of 8: (0, OK) -- Go returns false before it uses w;
  3. len(digest) > bits(q) / 8: (0, FENCED) -- Go takes the whole digest and leaves truncation to its caller; that rests on memory
     of its source, so no answer is claimed;
  4. s has no inverse mod q (a composite q): (0, NO_INVERSE) -- ModInverse returns nil, which Go 1.13.0 dereferences and later
     patch releases answer with false;
  5. w = s^-1 mod q, z = the digest as an integer, u1 = z w mod q, u2 = r w mod q, v = g^u1 y^u2 mod p mod q: (v == r, OK).
g or y >= p are reduced as big.Int.Exp reduces them, x^0 = 1, and p = 1 gives v = 0.  (p = 0, where Go returns false at once, is an
even p: the device refuses the call.)"""
import math

OK, NO_INVERSE, FENCED = 0, 1, 2


def prep(q: int, digest: bytes, r: int, s: int):
    """Rows 1-4 and the exponents: (status, decided, u1, u2); u1 = u2 = 0 where the verdict is decided."""
    if not (0 < r < q and 0 < s < q):
        return OK, 1, 0, 0
    n = q.bit_length()
    if n % 8:
        return OK, 1, 0, 0
    if len(digest) > n // 8:
        return FENCED, 1, 0, 0
    if math.gcd(s, q) != 1:
        return NO_INVERSE, 1, 0, 0
    w = pow(s, -1, q)
    z = int.from_bytes(digest, "big")
    return OK, 0, z * w % q, r * w % q


def verify(p: int, q: int, g: int, y: int, digest: bytes, r: int, s: int):
    status, decided, u1, u2 = prep(q, digest, r, s)
    if decided:
        return 0, status
    v = pow(g, u1, p) * pow(y, u2, p) % p % q
    return int(v == r), OK
