"""The seeded cases of the EC operation table (tests/c/ec_forms.h) with exact expectations, for the CPU test that runs the table
compiled by g++ (tests/test_ec_forms_reference.py) and the GPU test that runs it on the device (tests/test_gpu_ec_forms.py).  Not
collected.

    cases(name, fam)  -> (Case, ...)     Case = (label, rec, exp, tag): rec is the record's raw little-endian words as bytes
    check(name, fam, case, row) -> []    the names of what differs between a result row (bytes) and the expectation
    order(name, fam), sections(name, fam), pack(name, fam, idx), curve_block(name)      the device program's input file

Everything a record holds is the raw word row that reaches the arithmetic: field elements in Montgomery form (R = 2^(32 L)) exactly
as given, points as X, Y, Z rows.  Expectations are exact Python integers: field results word for word (outputs are fully reduced,
hence unique); a Jacobian result must have every row below p, Z = 0 exactly where the exact answer is infinity, and otherwise be
projectively equal to the exact affine answer (X = x Z^2, Y = y Z^3); case codes as they stand.  The group law here is the textbook
affine one (chord and tangent, None for infinity); the CPU test holds a sample of it to tests/ec_ref.py's Jacobian restatement, so
that this module does not grade itself."""
import functools
import random
import struct
from collections import namedtuple

import ec_ref as E
from ecdsa_verify_cases import sqrt_mod

Case = namedtuple("Case", "label rec exp tag")
WORDS = {"P-224": 7, "P-256": 8, "P-384": 12, "P-521": 17}
(FAM_FE, FAM_INV, FAM_FN, FAM_DBL, FAM_ADD, FAM_ADDA, FAM_MUL, FAM_FB, FAM_AFF, FAM_CHK, FAM_H2I, FAM_XR, FAM_LIMBS) = range(13)
FAM_NAMES = ["fe", "fp_inv", "fn_mul", "pt_dbl", "pt_add", "pt_add_affine", "pt_mul", "fb_mul", "pt_affine", "pt_check", "hash_to_int",
             "x_matches_r", "limbs"]
HOST_FAMS = tuple(range(FAM_LIMBS))            # the host compile has no limb conversions
DG_WORDS, LIMBS = 33, 76
FB_W = (4, 5)                                   # table t of FAM_FB: 4 is the library's width on every curve (ec_capi.inc), 5 the CPU suite's other one
GENERAL, EQUAL, OPPOSITE, INF_OPERAND = 0, 1, 2, 3
CODE_NAMES = ["GENERAL", "EQUAL", "OPPOSITE", "INF_OPERAND"]
CUTS = (1, 63, 64, 65, 129)                     # the wave and block ends (EC_BLOCK = 64)
M32 = 0xFFFFFFFF


def in_words(L, fam):
    return [1 + 2 * L, L, 2 * L, 3 * L, 1 + 6 * L, 1 + 5 * L, 4 * L, 1 + L, 3 * L, 2 * L, 1 + DG_WORDS, 4 * L, L][fam]


def out_words(L, fam):
    return [L, L, L, 3 * L, 3 * L + 1, 3 * L + 1, 3 * L, 3 * L, 2 * L, 1 + 2 * L, L, 1, LIMBS + L][fam]


class Ctx:
    """A curve with its Montgomery radix."""

    def __init__(self, name):
        c = E.CURVES[name]
        self.name, self.c = name, c
        self.p, self.n, self.b, self.g = c["p"], c["n"], c["b"], (c["gx"], c["gy"])
        self.L, self.f, self.bits = WORDS[name], E.byte_len(c), c["bit_size"]
        self.R = 1 << (32 * self.L)
        self.rinv = pow(self.R, -1, self.p)
        self.one = self.R % self.p
        self.seed = 9000 + self.bits

    def to_m(self, v):
        return v * self.R % self.p

    def from_m(self, v):
        return v * self.rinv % self.p

    def w(self, v):
        """L little-endian words"""
        return v.to_bytes(4 * self.L, "little")

    def on_curve(self, x, y):
        return (y * y - (x * x * x - 3 * x + self.b)) % self.p == 0

    def lift(self, x):
        y = sqrt_mod(x * x * x - 3 * x + self.b, self.p)
        return None if y is None else (x, y)


@functools.lru_cache(maxsize=None)
def ctx(name):
    return Ctx(name)


def u32(v):
    return struct.pack("<I", v)


def ints(cx, row, count, off=0):
    return [int.from_bytes(row[4 * (off + i * cx.L):4 * (off + (i + 1) * cx.L)], "little") for i in range(count)]


# ---- the exact group law (affine, None = infinity) ------------------------------------------------------------------------------
def aff_neg(cx, P):
    return None if P is None else (P[0], -P[1] % cx.p)


def aff_add(cx, P, Q):
    if P is None:
        return Q
    if Q is None:
        return P
    p = cx.p
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = (3 * P[0] * P[0] - 3) * pow(2 * P[1], -1, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return x, (lam * (P[0] - x) - P[1]) % p


def aff_mul(cx, P, k):
    """k P for any k >= 0 (not reduced first: the group's order is not assumed), low bit first"""
    acc = None
    while k:
        if k & 1:
            acc = aff_add(cx, acc, P)
        P = aff_add(cx, P, P)
        k >>= 1
    return acc


def add_code(cx, P, Q):
    """the case pt_add must report for exact operands"""
    if P is None or Q is None:
        return INF_OPERAND
    if P == Q:
        return EQUAL
    if P == aff_neg(cx, Q):
        return OPPOSITE
    return GENERAL


def ladder_codes(cx, P, k):
    """The cases the additions of pt_mul's ladder meet, in order (left to right over k's bits, acc starts at infinity)."""
    acc, codes = None, []
    for i in range(k.bit_length() - 1, -1, -1):
        acc = aff_add(cx, acc, acc)
        if (k >> i) & 1:
            codes.append(add_code(cx, acc, P))
            acc = aff_add(cx, acc, P)
    return codes


def walk_codes(cx, w, nwin, k):
    """The cases the mixed additions of fb_mul's walk over G's table meet: [(window, code)], low window first."""
    acc, codes, B = None, [], cx.g
    for i in range(nwin):
        d = (k >> (w * i)) & ((1 << w) - 1)
        if d:
            T = aff_mul(cx, B, d)
            codes.append((i, add_code(cx, acc, T)))
            acc = aff_add(cx, acc, T)
        for _ in range(w):
            B = aff_add(cx, B, B)
    return codes


def jac(cx, P, zraw):
    """The raw rows (X, Y, Z) of the finite point P under the Z whose raw words are zraw"""
    z = cx.from_m(zraw)
    assert P is not None and z
    return cx.to_m(P[0] * z * z), cx.to_m(P[1] * z * z * z), zraw


def jac_differs(cx, J, want):
    """[] or what is wrong with the raw result rows J against the exact affine answer"""
    bad = []
    if any(v >= cx.p for v in J):
        bad.append("row not below p")
    if (J[2] == 0) != (want is None):
        bad.append("infinity")
    elif want is not None:
        z = cx.from_m(J[2])
        if cx.from_m(J[0]) != want[0] * z * z % cx.p:
            bad.append("X")
        if cx.from_m(J[1]) != want[1] * z * z * z % cx.p:
            bad.append("Y")
    return bad


# ---- a 20-line CIOS model: fe_mul's value before the last subtraction, to classify cases only ----------------------------------------
def cios_t(a, b, m, L):
    m0inv = -pow(m, -1, 1 << 32) & M32
    t = 0
    for i in range(L):
        t += a * ((b >> (32 * i)) & M32)
        t = (t + ((t * m0inv) & M32) * m) >> 32
    return t


def cios_class(t, m, L):
    """0: t < m (no subtraction)   1: m <= t < 2^(32 L) (through the compare)   2: t >= 2^(32 L) (through t[L] != 0)"""
    assert t < 2 * m
    return 0 if t < m else 1 if t < 1 << (32 * L) else 2


# ---- field values ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field_values(name, mod):
    """{label: raw value below m} for m = p or n: the extremal words and a dozen random ones"""
    cx = ctx(name)
    m, L = (cx.p, cx.n)[mod], cx.L
    R = cx.R
    cand = [("0", 0), ("1", 1), ("2", 2), ("m-1", m - 1), ("m-2", m - 2), ("(m-1)/2", (m - 1) // 2), ("(m+1)/2", (m + 1) // 2), ("R mod m", R % m),
            ("R mod m - 1", R % m - 1)]
    for i in range(1, L):
        cand += [(f"2^{32 * i}", 1 << (32 * i)), (f"2^{32 * i}-1", (1 << (32 * i)) - 1), (f"m-2^{32 * i}", m - (1 << (32 * i)))]
    cand.append((f"2^{32 * L - 1}", 1 << (32 * L - 1)))
    for phase in (0, 1):
        cand.append((f"alternating from word {phase}", sum(M32 << (32 * i) for i in range(phase, L, 2))))
    for j in range(L):
        for d in (1, -1):
            word = ((m >> (32 * j)) + d) & M32
            cand.append((f"m word {j} {d:+d}", m & ~(M32 << (32 * j)) | word << (32 * j)))
    rng = random.Random(cx.seed + mod)
    cand += [(f"random {i}", rng.randrange(m)) for i in range(12)]
    out, seen = {}, set()
    for label, v in cand:
        if 0 <= v < m and v not in seen:
            seen.add(v)
            out[label] = v
    return out


def _fe_rec(cx, op, mod, a, b):
    return u32(op | mod << 4) + cx.w(a) + cx.w(b)


def _fe_cases(name):
    cx = ctx(name)
    L, R = cx.L, cx.R
    out = []
    for mod, mname in ((0, "p"), (1, "n")):
        m = (cx.p, cx.n)[mod]
        rinv = pow(R, -1, m)
        vals = list(field_values(name, mod).items())
        for i, (la, a) in enumerate(vals):
            for j, (lb, b) in enumerate(vals):
                prod = cx.w(a * b * rinv % m)
                tag = ("mul", mod, cios_class(cios_t(a, b, m, L), m, L))
                out.append(Case(f"fe_mul {mname}: {la} * {lb}", _fe_rec(cx, 2, mod, a, b), prod, tag))
                alias = 3 + (i + j) % 2
                out.append(Case(f"fe_mul {mname}, r is {'ab'[alias - 3]}: {la} * {lb}", _fe_rec(cx, alias, mod, a, b), prod, tag))
                out.append(Case(f"fe_add {mname}: {la} + {lb}", _fe_rec(cx, 0, mod, a, b), cx.w((a + b) % m), ("add", mod, a + b >= R)))
                out.append(Case(f"fe_sub {mname}: {la} - {lb}", _fe_rec(cx, 1, mod, a, b), cx.w((a - b) % m), ("sub", mod, a < b)))
        rng = random.Random(cx.seed + 10 + mod)
        firsts = [2, (m + 1) // 2, m - 1, rng.randrange(2, m - 1), rng.randrange(2, m - 1)]
        for s, ls in ((m - 1, "m-1"), (m, "m"), (m + 1, "m+1")):
            for a in firsts:
                out.append(Case(f"fe_add {mname}: a + b = {ls}, a = {a:#x}", _fe_rec(cx, 0, mod, a, s - a), cx.w(s % m), ("add", mod, False)))
        if 2 * (m - 1) >= R:                        # a carry out of the top word: the full-width moduli
            pairs = [(m - 1, m - 1), (m - 1, R - (m - 1)), (m - 1, R + 1 - (m - 1)), (m - 2, m - 1)]
            pairs += [(a, rng.randrange(R - a, m)) for a in (rng.randrange(R - m + 1, m) for _ in range(4))]
            if 1 << (32 * L - 1) < m:
                pairs.append((1 << (32 * L - 1), 1 << (32 * L - 1)))
            for a, b in pairs:
                assert a < m and b < m and a + b >= R
                out.append(Case(f"fe_add {mname}: carry out of the top word, {a:#x} + {b:#x}", _fe_rec(cx, 0, mod, a, b), cx.w((a + b) % m),
                                ("add", mod, True)))
        for a in (0, 1, m - 2, rng.randrange(m - 1), rng.randrange(m - 1)):
            out.append(Case(f"fe_sub {mname}: a - b = 0, a = {a:#x}", _fe_rec(cx, 1, mod, a, a), cx.w(0), ("sub", mod, False)))
            out.append(Case(f"fe_sub {mname}: a - b = -1, a = {a:#x}", _fe_rec(cx, 1, mod, a, a + 1), cx.w(m - 1), ("sub", mod, True)))
        for i in range(1, L):
            if 1 << (32 * i) < m:
                a = 1 << (32 * i)
                out.append(Case(f"fe_sub {mname}: 2^{32 * i} - 1, a borrow through {i} words", _fe_rec(cx, 1, mod, a, 1), cx.w(a - 1), ("sub", mod, False)))
        out.append(Case(f"fe_sub {mname}: 0 - (m-1), a borrow through every word", _fe_rec(cx, 1, mod, 0, m - 1), cx.w(1), ("sub", mod, True)))
    return out


def _inv_cases(name):
    cx = ctx(name)
    return [Case(f"fp_inv: {la}", cx.w(a), cx.w(pow(a, -1, cx.p) * cx.R * cx.R % cx.p if a else 0), a)
            for la, a in field_values(name, 0).items()]


def _fn_cases(name):
    cx = ctx(name)
    vals = list(field_values(name, 1).items())
    vals = vals[:9] + vals[9::2]
    return [Case(f"fn_mul: {la} * {lb}", cx.w(a) + cx.w(b), cx.w(a * b % cx.n), None) for la, a in vals for lb, b in vals]


# ---- points ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def special_x_points(name):
    """((label, (x, y)), ...): the points of smallest and largest x, and the first ones whose Montgomery-form x, stepped down from
    p - 1 and up from 2^(32 L - 1) (where that is below p), is on the curve"""
    cx = ctx(name)
    p = cx.p
    out = []
    x = 0
    while cx.lift(x) is None:
        x += 1
    out.append((f"smallest x = {x}", cx.lift(x)))
    x = p - 1
    while cx.lift(x) is None:
        x -= 1
    out.append((f"largest x = p-{p - x}", cx.lift(x)))
    xm = p - 1
    while cx.lift(cx.from_m(xm)) is None:
        xm -= 1
    out.append((f"Montgomery x = p-{p - xm}", cx.lift(cx.from_m(xm))))
    if 1 << (32 * cx.L - 1) < p:
        xm = 1 << (32 * cx.L - 1)
        while cx.lift(cx.from_m(xm)) is None:
            xm += 1
        out.append((f"Montgomery x = 2^{32 * cx.L - 1}+{xm - (1 << (32 * cx.L - 1))}", cx.lift(cx.from_m(xm))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def points(name):
    cx = ctx(name)
    rng = random.Random(cx.seed + 20)
    out = [("G", cx.g)] + [(f"random multiple {i}", aff_mul(cx, cx.g, rng.randrange(1, cx.n))) for i in range(3)]
    out += list(special_x_points(name))
    assert all(cx.on_curve(*pt) for _, pt in out)
    return tuple(out)


def _extremal_z(cx):
    fv = field_values(cx.name, 0)
    keys = ["1", "2", "alternating from word 0", "alternating from word 1", f"2^{32 * (cx.L - 1)}", "R mod m - 1", "m-2", f"2^{32 * cx.L - 1}",
            f"2^{32 * (cx.L - 1)}-1", "(m+1)/2"]
    return [(k, fv[k]) for k in keys if k in fv and fv[k]]


@functools.lru_cache(maxsize=None)
def jac_forms(name):
    """((label, point index, affine, (X, Y, Z)), ...): every point at Z = 1, Z = p - 1, a random Z and an extremal Z; then infinity
    (point index None) as all-zero words and as Z = 0 under the X, Y of G and of a random point"""
    cx = ctx(name)
    rng = random.Random(cx.seed + 30)
    ext = _extremal_z(cx)
    out = []
    for i, (lp, P) in enumerate(points(name)):
        le, ze = ext[i % len(ext)]
        for lz, z in (("Z = 1", cx.one), ("Z = p-1", cx.p - 1), ("random Z", rng.randrange(1, cx.p)), (f"Z raw {le}", ze)):
            out.append((f"{lp} at {lz}", i, P, jac(cx, P, z)))
    out.append(("infinity, all words zero", None, None, (0, 0, 0)))
    out.append(("infinity, Z = 0 under G's X, Y", None, None, (cx.to_m(cx.g[0]), cx.to_m(cx.g[1]), 0)))
    out.append(("infinity, Z = 0 under random X, Y", None, None, (rng.randrange(1, cx.p), rng.randrange(1, cx.p), 0)))
    return tuple(out)


def _jw(cx, J):
    return cx.w(J[0]) + cx.w(J[1]) + cx.w(J[2])


def _neg_jac(cx, J):
    return J[0], -J[1] % cx.p, J[2]


def _dbl_cases(name):
    cx = ctx(name)
    return [Case(f"pt_dbl: {lab}", _jw(cx, J), aff_add(cx, P, P), None) for lab, _, P, J in jac_forms(name)]


def _add_pairs(name):
    """[(label, P form, Q form)] over jac_forms: general pairs, equal and opposite points under equal and different Z, infinity"""
    cx = ctx(name)
    forms = jac_forms(name)
    fin = [f for f in forms if f[1] is not None]
    inf = [f for f in forms if f[1] is None]
    out = []
    for i, a in enumerate(fin):
        b = fin[(7 * i + 5) % len(fin)]
        if b[1] == a[1]:
            b = fin[(7 * i + 9) % len(fin)]
        assert b[1] != a[1]
        out.append((f"{a[0]} + {b[0]}", a, b))
    for k in range(0, len(fin), 4):
        z1, zm, zr, ze = fin[k:k + 4]
        for a, b, how in ((z1, z1, "equal Z"), (zr, zr, "equal Z"), (z1, zr, "different Z"), (zm, ze, "different Z"), (ze, z1, "different Z")):
            out.append((f"P + P, {how}: {a[0]} + {b[0]}", a, b))
            nb = (f"-({b[0]})", b[1], aff_neg(cx, b[2]), _neg_jac(cx, b[3]))
            out.append((f"P + (-P), {how}: {a[0]} + {nb[0]}", a, nb))
    for z in inf:
        for a in (fin[0], fin[6], fin[-1]):
            out.append((f"{z[0]} + {a[0]}", z, a))
            out.append((f"{a[0]} + {z[0]}", a, z))
        for z2 in inf:
            out.append((f"{z[0]} + {z2[0]}", z, z2))
    return out


def _add_cases(name):
    cx = ctx(name)
    out = []
    for lab, a, b in _add_pairs(name):
        want, code = aff_add(cx, a[2], b[2]), add_code(cx, a[2], b[2])
        for form, lf in enumerate(("R distinct", "R is P", "R is Q")):
            out.append(Case(f"pt_add, {lf}: {lab}", u32(form) + _jw(cx, a[3]) + _jw(cx, b[3]), (want, code), code))
    return out


def _adda_cases(name):
    cx = ctx(name)
    out = []
    for lab, a, b in _add_pairs(name):
        if b[2] is None:
            continue                              # the affine operand is finite
        Q = b[2]
        want, code = aff_add(cx, a[2], Q), add_code(cx, a[2], Q)
        for form, lf in enumerate(("R distinct", "R is P")):
            out.append(Case(f"pt_add_affine, {lf}: {lab}", u32(form) + _jw(cx, a[3]) + cx.w(cx.to_m(Q[0])) + cx.w(cx.to_m(Q[1])), (want, code), code))
    return out


def mul_scalars(name):
    """[(label, k, the case the ladder's last addition must meet or None)]"""
    cx = ctx(name)
    n, R = cx.n, cx.R
    rng = random.Random(cx.seed + 40)
    ks = [("k = 0", 0, None), ("k = 1", 1, None), ("k = 2", 2, None), ("k = 3", 3, None), ("k = n-2", n - 2, None), ("k = n-1", n - 1, None),
          ("k = n: ends on OPPOSITE", n, OPPOSITE), ("k = n+1", n + 1, None), ("k = n+2: ends on EQUAL", n + 2, EQUAL),
          (f"k = 2^{32 * cx.L}-1", R - 1, None)]
    if 2 * n + 2 < R:
        ks += [("k = 2n", 2 * n, None), ("k = 2n+1: ends on INF_OPERAND", 2 * n + 1, INF_OPERAND), ("k = 2n+2", 2 * n + 2, None)]
    ks += [(f"k = 2^{i}", 1 << i, None) for i in (31, 32, 33, 32 * (cx.L - 1), 32 * cx.L - 1)]
    ks += [(f"k random {i}", rng.randrange(R if i & 1 else n), None) for i in range(4)]
    return ks


def _mul_cases(name):
    cx = ctx(name)
    forms = jac_forms(name)
    fin = [f for f in forms if f[1] is not None]
    by = {f[0]: f for f in forms}
    pts = points(name)
    bases = [by["G at Z = 1"], by[f"{pts[1][0]} at random Z"], by[f"{pts[5][0]} at Z = p-1"], fin[4 * 6 + 3]]
    out = []
    for base in bases:
        chain = [base[2]]                         # 2^i P
        for _ in range(32 * cx.L):
            chain.append(aff_add(cx, chain[-1], chain[-1]))
        for lk, k, last in mul_scalars(name):
            want = None
            for i in range(k.bit_length()):
                if (k >> i) & 1:
                    want = aff_add(cx, want, chain[i])
            out.append(Case(f"pt_mul: {lk}, P = {base[0]}", _jw(cx, base[3]) + cx.w(k), want, (last, base[2], k)))
    for z in forms[-2:]:
        for lk, k, _ in mul_scalars(name)[3:7]:
            out.append(Case(f"pt_mul: {lk}, P = {z[0]}", _jw(cx, z[3]) + cx.w(k), None, (None, None, k)))
    return out


def fb_windows(cx, w):
    return (8 * cx.f + w - 1) // w


def _fb_cases(name):
    cx = ctx(name)
    n = cx.n
    chain = [cx.g]
    for _ in range(32 * cx.L + 8):
        chain.append(aff_add(cx, chain[-1], chain[-1]))
    out = []
    for t, w in enumerate(FB_W):
        nwin = fb_windows(cx, w)
        span = min(w * nwin, 32 * cx.L)          # k < 2^(w nwin), in L words
        rng = random.Random(cx.seed + 50 + t)
        ks = []
        for i in range(nwin):
            d = ((1, (1 << w) - 1, rng.randrange(1, 1 << w))[i % 3] << (w * i)) & ((1 << span) - 1)
            if d:
                ks.append((f"one digit, window {i}", d, None))
        ks += [("all digits at their maximum", (1 << span) - 1, None), ("all digits zero", 0, None), ("k = n-1", n - 1, None), ("k = n", n, None)]
        ks += [(f"k random {i}", rng.randrange(n), None) for i in range(4)]
        top = w * (nwin - 1)
        if 1 << top > n:                          # P-521: the windows cover more than the order's bits
            ks.append((f"k = 2^{top} + (2^{top} mod n) >= n: EQUAL in the top window", (1 << top) | (1 << top) % n, (nwin - 1, EQUAL)))
        for lk, k, meet in ks:
            assert k < 1 << span
            want = None
            for i in range(k.bit_length()):
                if (k >> i) & 1:
                    want = aff_add(cx, want, chain[i])
            out.append(Case(f"fb_mul w = {w}: {lk}", u32(t) + cx.w(k), want, (meet, w, nwin, k)))
    return out


def _aff_cases(name):
    cx = ctx(name)
    return [Case(f"pt_affine: {lab}", _jw(cx, J), cx.w(P[0]) + cx.w(P[1]) if P else cx.w(0) + cx.w(0), None) for lab, _, P, J in jac_forms(name)]


def _chk_cases(name):
    cx = ctx(name)
    p, R = cx.p, cx.R
    out = []
    pts = [points(name)[0], points(name)[1]] + list(special_x_points(name))
    for lp, (x, y) in pts:
        pairs = [("the point", x, y), ("p - y", x, p - y), ("y + 1", x, (y + 1) % p), ("x + 1", (x + 1) % p, y)]
        for lv, v in (("p", p), ("p+1", p + 1), (f"2^{32 * cx.L}-1", R - 1)):
            pairs += [(f"x = {lv}", v, y), (f"y = {lv}", x, v), (f"x = y = {lv}", v, v)]
        for lab, a, b in pairs:
            ok = a < p and b < p
            exp = u32(int(ok and cx.on_curve(a, b))) + (cx.w(cx.to_m(a)) + cx.w(cx.to_m(b)) if ok else cx.w(0) + cx.w(0))
            out.append(Case(f"pt_check: {lp}, {lab}", cx.w(a) + cx.w(b), exp, None))
    out.append(Case("pt_check: (0, 0)", cx.w(0) + cx.w(0), u32(0) + cx.w(0) + cx.w(0), None))
    return out


def hash_to_int(cx, dg):
    take = dg[:cx.f]
    e = int.from_bytes(take, "big")
    if 8 * len(take) > cx.bits:
        e >>= 8 * len(take) - cx.bits
    assert e < 2 * cx.n
    return e - cx.n if e >= cx.n else e


def _h2i_cases(name):
    cx = ctx(name)
    f, n = cx.f, cx.n
    rng = random.Random(cx.seed + 60)
    dgs = []
    lens = sorted({1, f - 1, f, f + 1, 2 * f} | ({65, 66} if name == "P-521" else set()))
    for dlen in lens:
        dgs += [(f"random, dlen {dlen} #{j}", rng.randbytes(dlen)) for j in range(2)]
        dgs.append((f"all ones, dlen {dlen}", b"\xff" * dlen))
    for lv, v in (("n-1", n - 1), ("n", n), ("n+1", n + 1), ("2^bits-1", (1 << cx.bits) - 1), ("0", 0)):
        d = (v << (8 * f - cx.bits)).to_bytes(f, "big")
        dgs.append((f"truncated value {lv}, dlen {f}", d))
        dgs.append((f"truncated value {lv}, dlen {2 * f}", d + rng.randbytes(f)))
    if 8 * f > cx.bits:                           # P-521: the bits shifted out are set as well
        d = ((n << (8 * f - cx.bits)) | ((1 << (8 * f - cx.bits)) - 1)).to_bytes(f, "big")
        dgs.append((f"truncated value n with the shifted-out bits set, dlen {f}", d))
    return [Case(f"hash_to_int: {lab}", u32(len(d)) + d.ljust(4 * DG_WORDS, b"\0"), cx.w(hash_to_int(cx, d)), len(d)) for lab, d in dgs]


def _xr_cases(name):
    cx = ctx(name)
    p, n, R = cx.p, cx.n, cx.R
    rng = random.Random(cx.seed + 70)
    out = []

    def put(lab, P, r, tag=None):
        assert 0 < r < n
        want = P[0] == r or P[0] == r + n
        for lz, z in (("Z = 1", cx.one), ("random Z", rng.randrange(1, p))):
            out.append(Case(f"x_matches_r: {lab}, {lz}", _jw(cx, jac(cx, P, z)) + cx.w(r), u32(int(want)), tag))

    low = [pt for _, pt in points(name) if 1 < pt[0] < n - 1][:3]
    for i, P in enumerate(low):
        put(f"x(R) = r #{i}", P, P[0], "x = r")
        put(f"x(R) = r + 1 #{i}", P, P[0] - 1)
        put(f"x(R) = r - 1 #{i}", P, P[0] + 1)
    x = n + 2
    for i in range(2):                            # x(R) = r + n < p
        while cx.lift(x) is None:
            x += 1
        P = cx.lift(x)
        put(f"x(R) = r + n < p #{i}", P, x - n, "x = r + n")
        put(f"x(R) = r + n + 1 #{i}", P, x - n - 1)
        put(f"x(R) = r + n - 1 #{i}", P, x - n + 1)
        x += 1
    lx, hi = points(name)[5]                      # the point of largest x: r + n at and around p
    assert hi[0] >= n
    put(f"x(R) = r + n, {lx}", hi, hi[0] - n, "x = r + n")
    for r, lr in ((p - n, "r + n = p"), (p - n + 1, "r + n = p+1"), (p - n - 1, "r + n = p-1")):
        for P in (hi, low[0]):
            if 0 < r < n:
                put(f"{lr}, x(R) = {'r + n - ' + str(r + n - P[0]) if P is hi else 'another'}", P, r, "r + n >= p" if r + n >= p else None)
    r = p - n + 2
    while cx.lift(r) is None:
        r += 1
    put("x(R) = r, r + n >= p", cx.lift(r), r, "r + n >= p")
    if 2 * n - 1 >= R:                            # r + n >= 2^(32 L): the carry-out exit, the full-width curves
        put("r = n-1: r + n carries out of the top word", low[0], n - 1, "carry")
        r = R - n
        while cx.lift(r + n - R) is None:
            r += 1
        put("r + n carries out of the top word, x(R) = r + n - 2^(32 L)", cx.lift(r + n - R), r, "carry")
        r = rng.randrange(R - n, n)
        put("random r, r + n carries out of the top word", low[1], r, "carry")
    return out


def _limb_cases(name):
    cx = ctx(name)
    L = cx.L
    vals = {}
    for mod in (0, 1):
        for lab, v in field_values(name, mod).items():
            if not lab.startswith("random"):
                vals.setdefault(v, f"{'pn'[mod]}-set {lab}")
    vals.setdefault((1 << (32 * L)) - 1, "all ones")
    for b in sorted({28 * k for k in range((32 * L + 27) // 28)} | {32 * k for k in range(L)}):
        vals.setdefault(1 << b, f"bit {b}")
        vals.setdefault((1 << (32 * L)) - 1 - (1 << b), f"all ones but bit {b}")
    rng = random.Random(cx.seed + 80)
    for i in range(4):
        vals.setdefault(rng.randrange(1 << (32 * L)), f"random {i}")
    return [Case(f"limbs: {lab}", cx.w(v), b"".join(u32((v >> (28 * k)) & 0x0FFFFFFF) for k in range(LIMBS)) + cx.w(v), None) for v, lab in vals.items()]


_BUILD = [_fe_cases, _inv_cases, _fn_cases, _dbl_cases, _add_cases, _adda_cases, _mul_cases, _fb_cases, _aff_cases, _chk_cases, _h2i_cases, _xr_cases,
          _limb_cases]


@functools.lru_cache(maxsize=None)
def cases(name, fam):
    out = tuple(_BUILD[fam](name))
    L = WORDS[name]
    assert all(len(cs.rec) == 4 * in_words(L, fam) for cs in out) and len({cs.label for cs in out}) == len(out)
    return out


def check(name, fam, case, row):
    """[] or the names of what differs between a result row (out_words(L, fam) words as bytes) and the case's expectation"""
    cx = ctx(name)
    L = cx.L
    assert len(row) == 4 * out_words(L, fam)
    if fam in (FAM_DBL, FAM_MUL, FAM_FB):
        return jac_differs(cx, ints(cx, row, 3), case.exp)
    if fam in (FAM_ADD, FAM_ADDA):
        want, code = case.exp
        got = struct.unpack_from("<I", row, 12 * L)[0]
        return jac_differs(cx, ints(cx, row, 3), want) + ([f"code {got} for {CODE_NAMES[code]}"] if got != code else [])
    if row == case.exp:
        return []
    if fam == FAM_INV:
        return ["r"] + (["r a != 1"] if case.tag and ints(cx, row, 1)[0] * case.tag * cx.rinv % cx.p != cx.one else [])
    if fam == FAM_AFF:
        return [nm for nm, g, e in zip("xy", ints(cx, row, 2), ints(cx, case.exp, 2)) if g != e]
    if fam == FAM_CHK:
        return [nm for nm, lo, hi in (("verdict", 0, 4), ("xm", 4, 4 + 4 * L), ("ym", 4 + 4 * L, 4 + 8 * L)) if row[lo:hi] != case.exp[lo:hi]]
    if fam == FAM_LIMBS:
        return [nm for nm, lo, hi in (("limbs", 0, 4 * LIMBS), ("words", 4 * LIMBS, 4 * (LIMBS + L))) if row[lo:hi] != case.exp[lo:hi]]
    return ["r" if fam in (FAM_FE, FAM_FN) else "e" if fam == FAM_H2I else "verdict"]


# ---- the device program's input file ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def order(name, fam):
    """the whole set, shuffled: neighbouring lanes hold different cases"""
    idx = list(range(len(cases(name, fam))))
    random.Random(ctx(name).seed + 100 + fam).shuffle(idx)
    return tuple(idx)


def sections(name, fam):
    """[indices into cases(name, fam)]: the shuffled whole, then its head cut at the wave and block ends (a list shorter than a cut
    goes round again)"""
    o = order(name, fam)
    return [list(o)] + [[o[i % len(o)] for i in range(g)] for g in CUTS]


def curve_block(name):
    cx = ctx(name)
    be = b"".join(cx.c[k].to_bytes(cx.f, "big") for k in ("p", "n", "b", "gx", "gy"))
    return struct.pack("<III", cx.L, cx.f, cx.bits) + be.ljust((len(be) + 3) // 4 * 4, b"\0")


def pack(name, fam, idx):
    cs = cases(name, fam)
    return struct.pack("<III", WORDS[name], fam, len(idx)) + b"".join(cs[i].rec for i in idx)


def rows(name, fam, count, buf, off):
    """-> ([row bytes], the offset behind them)"""
    step = 4 * out_words(WORDS[name], fam)
    assert off + count * step <= len(buf)
    return [buf[off + i * step:off + (i + 1) * step] for i in range(count)], off + count * step
