"""The operand set of the 18 x 4 form at radix 2^29 (csrc/mont28.h with W = 29: k_rsa_modexp<18,4,29>), built the way
tests/mont_cases.py builds the sets of the 28-bit forms, for tests/test_mont29_model.py (CPU) and tests/test_gpu_mont29.py
(device, through tests/c/mont_form29.hip).

The model (tests/mont_model.py) keeps its limb width in the module globals W and MASK; `width29` sets them to 29 bits through
pytest's MonkeyPatch for the length of a `with` block and puts 28 back, so every other test still sees 28.  Everything here
that touches the model runs inside such a block.

Moduli: the full and the sparse 2048-bit prime of tests/golden/extremal_moduli.json, a seeded random odd 2047-bit and
1025-bit number, and one of 64 bits, far too short for the class (its upper three lanes are zero).
Rows under a modulus n: 0, 1, n - 1, n, 2n - 1, the longest run of limbs equal to 2^29 that stays below 2n, 0 and 2^29
alternating, a seeded random value below 2n.  Every ordered pair goes through MUL, every row through SQR; then x = R - 1
times R^2, the carry pairs whose product comes out at exactly n + 2^(29 m) - 1, a chain of 64 lazy squarings, and e = 65537
as k_rsa_modexp schedules it, with the x-shortcut (16 squarings, times plain x) and without (times xR, then times 1)."""
import contextlib
import functools
import random
import struct

import pytest

from tests import mont_cases as K28
from tests import mont_model as M

W = 29
L, TPI = 18, 4
FORM = (L, TPI)
N = L * TPI
MASK = (1 << W) - 1
LIMB = 1 << W
R = 1 << (W * N)


@contextlib.contextmanager
def width29():
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(M, "W", W)
        mp.setattr(M, "MASK", MASK)
        yield


def to_limbs(x):
    assert 0 <= x < R
    return [(x >> (W * i)) & MASK for i in range(N)]


def from_limbs(row):
    return sum(int(v) << (W * i) for i, v in enumerate(row))


def n0inv_of(n):
    return (-pow(n, -1, LIMB)) & MASK


@functools.lru_cache(maxsize=None)
def moduli():
    rng = random.Random(2929)
    odd = lambda bits: rng.getrandbits(bits - 1) | (1 << (bits - 1)) | 1          # noqa: E731
    return [("full2048", K28.rsa_modulus("full2048")), ("sparse2048", K28.rsa_modulus("sparse2048")), ("random2047", odd(2047)),
            ("random1025", odd(1025)), ("random64", odd(64))]


def _run_of(n, step):
    row = [0] * N
    for i in range(0, N, step):
        row[i] = LIMB
        if from_limbs(row) >= 2 * n:
            row[i] = 0
            break
    return row


def rows(n, label):
    rng = random.Random(label)
    out = [("0", to_limbs(0)), ("1", to_limbs(1)), ("n-1", to_limbs(n - 1)), ("n", to_limbs(n)), ("2n-1", to_limbs(2 * n - 1)),
           ("all2^29", _run_of(n, 1)), ("alt2^29", _run_of(n, 2)), ("random", to_limbs(rng.randrange(2 * n)))]
    for _, r in out:
        assert from_limbs(r) < 2 * n and max(r) <= LIMB
    return out


def carry_pairs(n):
    """[(name, a, b)] with a b = t n + d R, d = 2^(29 m) - 1: mont_mul's output is n + d exactly, so reduce_once's borrow
    runs from limb 0 up to limb m.  m: the largest that keeps b below 2n, and one that ends in the third lane."""
    a = 2 * n - 1
    m_max = ((a * n) // R).bit_length() // W
    while m_max > 0 and (1 << (W * m_max)) - 1 >= (a * n) // R:
        m_max -= 1
    if m_max == 0:
        return []
    out = []
    for m in sorted({m_max, min(m_max, 2 * L + 1)}):
        d = (1 << (W * m)) - 1
        t = (-d * R * pow(n, -1, a)) % a
        b, rem = divmod(t * n + d * R, a)
        assert rem == 0 and 0 < t and b < 2 * n
        assert (a * b + ((-a * b * pow(n, -1, R)) % R) * n) // R == n + d
        out.append(("n+2^(29*%d)-1" % m, to_limbs(a), to_limbs(b)))
    return out


class Case:
    __slots__ = ("label", "op", "k", "a", "b", "n", "n0inv", "nval", "residue")

    def __init__(self, label, op, k, a, b, n_row, nval, residue):
        self.label, self.op, self.k, self.a, self.b, self.n, self.nval = label, op, k, a, b, n_row, nval
        self.n0inv = n0inv_of(nval)
        self.residue = residue


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    with width29():
        for mlabel, n in moduli():
            nrow = to_limbs(n)
            Ri = pow(R, -1, n)
            rs = rows(n, "18x4w29" + mlabel)
            val = {name: from_limbs(r) for name, r in rs}
            mk = lambda label, op, k, a, b, res: out.append(Case("%s %s" % (mlabel, label), op, k, a, b, nrow, n, res % n))   # noqa: E731
            for an, a in rs:
                for bn, b in rs:
                    mk("MUL %s * %s" % (an, bn), M.MUL, 0, a, b, val[an] * val[bn] * Ri)
                mk("SQR %s" % an, M.SQR, 0, a, a, val[an] ** 2 * Ri)
            r2 = to_limbs(R * R % n)
            mk("MUL R-1 * R^2", M.MUL, 0, [MASK] * N, r2, (R - 1) * R)
            for name, a, b in carry_pairs(n):
                mk("MUL " + name, M.MUL, 0, a, b, from_limbs(a) * from_limbs(b) * Ri)
            mk("CHAIN64 2n-1", M.CHAIN, 64, dict(rs)["2n-1"], dict(rs)["random"], pow(val["2n-1"], 1 << 64, n) * val["random"] * pow(Ri, 1 << 64, n))
            # e = 65537 as k_rsa_modexp runs it: x R (the lazy output of the to-Montgomery product), 16 squarings, then
            # times plain x (the x-shortcut), or times x R and then times 1
            for xn, x in (("random", val["random"] % n), ("n-1", n - 1)):
                xr = M.mont_mul(to_limbs(x), r2, nrow, n0inv_of(n), L, TPI)
                mk("CHAIN16 shortcut x=%s" % xn, M.CHAIN, 16, xr, to_limbs(x), pow(x, 65537, n))
                mk("CHAIN16 times xR x=%s" % xn, M.CHAIN, 16, xr, xr, pow(x, 65537, n) * R)
                y = M.run_op(M.CHAIN, 16, xr, xr, nrow, n0inv_of(n), L, TPI)[0]
                mk("MUL 1 * (x^65537 R) x=%s" % xn, M.MUL, 0, to_limbs(1), y, pow(x, 65537, n))
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """The model's (lazy, canonical, reduced) rows of every case, in order, and the Stats over the whole set."""
    st = M.Stats()
    with width29():
        return [M.run_op(c.op, c.k, c.a, c.b, c.n, c.n0inv, L, TPI, st) for c in cases()], st


def all_maximum(bound):
    """Every limb of a and b at 2^29, every limb of n at 2^29 - 1 and (bound) every row's Montgomery factor at 2^29 - 1:
    the largest column of the general and of the squaring form."""
    tops = []
    with width29():
        for sqr in (False, True):
            st = M.Stats()
            M.mont_mul([LIMB] * N, [LIMB] * N, [MASK] * N, 1, L, TPI, sqr, st, (M.BOUND_M,) if bound else ())
            tops.append(st.max_col)
    return tops


# ---- the driver's byte layout (tests/c/mont_form29.hip): that of tests/c/mont_forms.hip

def pack(case_list):
    parts = [struct.pack("<3I", L, TPI, len(case_list))]
    for c in case_list:
        parts.append(struct.pack("<%dI" % (3 + 3 * N), c.op, c.k, c.n0inv, *c.a, *c.b, *c.n))
    return b"".join(parts)


def unpack(count, buf, off):
    out = []
    for _ in range(count):
        v = struct.unpack_from("<%dI" % (3 * N), buf, off)
        off += 12 * N
        out.append((list(v[:N]), list(v[N:2 * N]), list(v[2 * N:])))
    return out, off


def cut_sizes():
    """Group counts that put the last working group at, and just past, the end of a DPP row, a wave and a block."""
    return [1, 16 // TPI, 16 // TPI + 1, 64 // TPI, 64 // TPI + 1, 256 // TPI, 256 // TPI + 1]


def shuffled():
    idx = list(range(len(cases())))
    random.Random("18x4w29").shuffle(idx)
    return idx
