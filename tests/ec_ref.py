"""A plain-Python restatement of Go 1.13's generic crypto/elliptic CurveParams code and of the reference's
ecdsaGroupOperations (crypto/threshold/ecdsa/ecdsa.go), for the threshold-ECDSA tests.  Not collected (no test_ prefix).

Points are affine (x, y) ints; (0, 0) stands for infinity as in crypto/elliptic.  Two behaviours of Go 1.13 that nobody here
can check (Add of equal points, the affine (0, 0) handed to Add / ScalarMult) are not relied on: `calculate_r` reports them as
fences, the rules of docs/parity.md."""
import json
import os

from oracle.threshold import lagrange

_FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ec_curves.json")))
CURVES = {name: {"p": int(c["p"], 16), "n": int(c["n"], 16), "b": int(c["b"], 16), "gx": int(c["gx"], 16), "gy": int(c["gy"], 16),
                 "bit_size": c["bit_size"]} for name, c in _FIX.items()}
NAMES = ["P-224", "P-256", "P-384", "P-521"]

OK, NO_INVERSE, FENCED = 0, 1, 2


def byte_len(c) -> int:
    return (c["bit_size"] + 7) // 8


def is_on_curve(c, x, y) -> bool:
    p = c["p"]
    return (y * y - (x * x * x - 3 * x + c["b"])) % p == 0


def marshal(c, x, y) -> bytes:
    f = byte_len(c)
    return b"\x04" + x.to_bytes(f, "big") + y.to_bytes(f, "big")


def unmarshal(c, data: bytes):
    """elliptic.Unmarshal: (x, y) or None."""
    f = byte_len(c)
    if len(data) != 1 + 2 * f or data[0] != 4:
        return None
    x, y = int.from_bytes(data[1:1 + f], "big"), int.from_bytes(data[1 + f:], "big")
    if x >= c["p"] or y >= c["p"] or not is_on_curve(c, x, y):
        return None
    return x, y


# ---- Jacobian arithmetic as CurveParams does it (a = -3) ------------------------------------------------------------
def double_jacobian(c, x, y, z):
    p = c["p"]
    delta = z * z % p
    gamma = y * y % p
    alpha = 3 * (x - delta) * (x + delta) % p
    beta = x * gamma % p
    x3 = (alpha * alpha - 8 * beta) % p
    z3 = ((y + z) ** 2 - gamma - delta) % p
    y3 = (alpha * (4 * beta - x3) - 8 * gamma * gamma) % p
    return x3, y3, z3


def add_jacobian(c, x1, y1, z1, x2, y2, z2):
    """add-2007-bl with the infinity and equal-operand cases (the latter as the fenced reading: doubling)."""
    p = c["p"]
    if z1 % p == 0:
        return x2, y2, z2
    if z2 % p == 0:
        return x1, y1, z1
    z1z1, z2z2 = z1 * z1 % p, z2 * z2 % p
    u1, u2 = x1 * z2z2 % p, x2 * z1z1 % p
    h = (u2 - u1) % p
    s1, s2 = y1 * z2 * z2z2 % p, y2 * z1 * z1z1 % p
    r = (s2 - s1) % p
    if h == 0 and r == 0:
        return double_jacobian(c, x1, y1, z1)
    i = (2 * h) ** 2 % p
    j = h * i % p
    r = 2 * r % p
    v = u1 * i % p
    x3 = (r * r - j - 2 * v) % p
    y3 = (r * (v - x3) - 2 * s1 * j) % p
    z3 = ((z1 + z2) ** 2 - z1z1 - z2z2) * h % p
    return x3, y3, z3


def affine_from_jacobian(c, x, y, z):
    p = c["p"]
    if z % p == 0:
        return 0, 0
    zi = pow(z, -1, p)
    return x * zi * zi % p, y * zi * zi * zi % p


def z_for_affine(x, y):
    return 0 if x == 0 and y == 0 else 1


def add(c, x1, y1, x2, y2):
    return affine_from_jacobian(c, *add_jacobian(c, x1, y1, z_for_affine(x1, y1), x2, y2, z_for_affine(x2, y2)))


def scalar_mult(c, bx, by, k: bytes):
    """ScalarMult bit by bit over the scalar's bytes (Bz = 1)."""
    x, y, z = 0, 0, 0
    for byte in k:
        for _ in range(8):
            x, y, z = double_jacobian(c, x, y, z)
            if byte & 0x80:
                x, y, z = add_jacobian(c, bx, by, 1, x, y, z)
            byte = (byte << 1) & 0xFF
    return affine_from_jacobian(c, x, y, z)


def int_bytes(v: int) -> bytes:
    """big.Int.Bytes(): minimal big-endian, empty for 0."""
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def scalar_base_mult(c, k: int):
    return scalar_mult(c, c["gx"], c["gy"], int_bytes(k))


def calculate_partial_r(c, ai: int) -> bytes:
    return marshal(c, *scalar_base_mult(c, ai))


def point_neg(c, pt):
    return pt[0], (-pt[1]) % c["p"]


# ---- ecdsaGroupOperations.CalculateR with the fence rules ----------------------------------------------------------
def calculate_r(c, xs, ri, vi):
    """-> (status, r): the reference's answer where it does not rest on memory, else FENCED."""
    n = c["n"]
    pts, ls = [], []
    for x, r in zip(xs, ri):
        pt = unmarshal(c, r)
        if pt is None:
            return FENCED, 0
        ls.append(lagrange(x, xs, n))
        pts.append(pt)
    if any(l % n == 0 for l in ls):
        return FENCED, 0
    k = len(xs)
    s = None
    for j, (pt, l) in enumerate(zip(pts, ls)):
        t = scalar_mult(c, pt[0], pt[1], int_bytes(l))
        if s is None:
            s = t
            continue
        if s == t:
            return FENCED, 0                       # Add's doubling case
        s = add(c, s[0], s[1], t[0], t[1])
        if s == (0, 0) and j < k - 1:
            return FENCED, 0                       # a prefix sum at infinity goes into the next Add
    v = sum(vv * l for vv, l in zip(vi, ls)) % n
    if v == 0:
        return NO_INVERSE, 0
    w = pow(v, -1, n)
    if s == (0, 0):
        return OK, 0                               # x = 0 under either reading
    q = scalar_mult(c, s[0], s[1], int_bytes(w))
    return OK, q[0] % n


def ecdsa_sign_hash_int(c, d: int, e: int, k: int):
    """Textbook ECDSA (r, s) for a hash integer e and nonce k (no truncation: callers pass e < n)."""
    n = c["n"]
    r = scalar_base_mult(c, k)[0] % n
    s = pow(k, -1, n) * (e + r * d) % n
    return r, s


def ecdsa_verify(c, q, e: int, r: int, s: int) -> bool:
    n = c["n"]
    if not (0 < r < n and 0 < s < n):
        return False
    w = pow(s, -1, n)
    p1 = scalar_base_mult(c, e * w % n)
    p2 = scalar_mult(c, q[0], q[1], int_bytes(r * w % n))
    x, _ = add(c, p1[0], p1[1], p2[0], p2[1])
    return x % n == r
