"""A plain-Python restatement of Go 1.13's crypto/ecdsa.Verify on the generic curve path, with the fence rules of
docs/parity.md ("ECDSA verification"), for the ECDSA-verification tests.  Builds on tests/ec_ref.py.  Not collected.

    verify(c, key_bytes, digest, sig) -> (valid, status)

status is ec_ref.OK (valid is Verify's answer) or ec_ref.FENCED (valid 0: the reference decides).  Order of the rules:
  1. a key that elliptic.Unmarshal refuses (prefix, coordinates below P, on the curve): FENCED -- no PublicKey holds such a point,
     so no call of Verify exists whatever r and s are;
  2. r or s outside [1, N): INVALID, decided;
  3. e = hashToInt(digest) = 0 mod N, i.e. u1 = 0: FENCED -- ScalarBaseMult returns the affine (0, 0), which goes into Add;
  4. u1 G = u2 Q: FENCED -- Add's doubling case on the generic path of P-384 and P-521;
  5. u1 G = -u2 Q: the sum is infinity, (0, 0) under either reading: INVALID;
  6. VALID iff x(u1 G + u2 Q) mod N = r."""
import ec_ref as E

OK, FENCED = E.OK, E.FENCED


def hash_to_int(c, digest: bytes) -> int:
    """ecdsa.go's hashToInt (the reference's copy: OS2I, crypto/threshold/ecdsa/ecdsa.go:88-98), not yet reduced mod N."""
    order_bits = c["n"].bit_length()
    order_bytes = (order_bits + 7) // 8
    if len(digest) > order_bytes:
        digest = digest[:order_bytes]
    ret = int.from_bytes(digest, "big")
    excess = len(digest) * 8 - order_bits
    if excess > 0:
        ret >>= excess
    return ret


def split_sig(c, sig: bytes):
    f = E.byte_len(c)
    assert len(sig) == 2 * f
    return int.from_bytes(sig[:f], "big"), int.from_bytes(sig[f:], "big")


def verify(c, key: bytes, digest: bytes, sig: bytes):
    n = c["n"]
    q = E.unmarshal(c, key)
    if q is None:
        return 0, FENCED
    r, s = split_sig(c, sig)
    if not (0 < r < n and 0 < s < n):
        return 0, OK
    e = hash_to_int(c, digest)
    w = pow(s, -1, n)
    u1, u2 = e * w % n, r * w % n
    if u1 == 0:
        return 0, FENCED
    p1 = E.scalar_base_mult(c, u1)
    p2 = E.scalar_mult(c, q[0], q[1], E.int_bytes(u2))
    if p1 == p2:
        return 0, FENCED
    x, y = E.add(c, p1[0], p1[1], p2[0], p2[1])
    if x == 0 and y == 0:
        return 0, OK
    return int(x % n == r), OK


def verify_math(c, key: bytes, digest: bytes, sig: bytes):
    """The mathematical verdict with no fence (what OpenSSL computes), or None for a key that is no point."""
    n = c["n"]
    q = E.unmarshal(c, key)
    if q is None:
        return None
    r, s = split_sig(c, sig)
    if not (0 < r < n and 0 < s < n):
        return 0
    e = hash_to_int(c, digest)
    w = pow(s, -1, n)
    u1, u2 = e * w % n, r * w % n
    p1 = E.scalar_base_mult(c, u1)
    p2 = E.scalar_mult(c, q[0], q[1], E.int_bytes(u2))
    x, y = E.affine_from_jacobian(c, *E.add_jacobian(c, *p1, E.z_for_affine(*p1), *p2, E.z_for_affine(*p2)))
    if x == 0 and y == 0:
        return 0
    return int(x % n == r)
