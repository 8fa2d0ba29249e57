"""The operand set of the Montgomery-form tests (tests/test_mont_model.py on the CPU, tests/test_gpu_mont_forms.py on the
device): per form of csrc/mont28.h the moduli, the limb rows, the operations on them, what the model (tests/mont_model.py)
says each gives, the exact residue it must equal, and the byte layout tests/c/mont_forms.hip reads and writes.

Moduli per form, B the largest size the form is used for: the full and the sparse prime of tests/golden/extremal_moduli.json,
one seeded random odd B-bit number, and one far shorter than the class, whose top lanes are zero.

Rows under a modulus n: 0, 1, n - 1, n, 2n - 1; the longest run of limbs equal to 2^28 whose value stays below 2n; 0 and
2^28 alternating, as far as stays below 2n; a seeded random value below 2n.  Every ordered pair goes through MUL (the two
operands of mont_mul play different parts: one is broadcast from LDS, one sits in registers), every row through SQR.

Constructed pairs (`carry_pairs`): a product a b = t n + d R (0 < t, d small) leaves mont_mul's output at exactly n + d, so
for d = 2^(28 m) - 1 the subtraction of reduce_once carries a borrow from limb 0 up to limb m: across every lane for the
largest m that keeps b below 2n.  a = n gives the output n itself, which under the sparse modulus is the number whose middle
lanes are zero: each of them holds 2^(28 L) minus the carry of the lane below before the cross-lane hop, so the hop's ripple
reaches the third limb and canonicalize has to carry through whole lanes of full limbs.  `travel` measures all three with the
model's Stats; tests/test_mont_model.py asserts the distances."""
import functools
import json
import os
import random
import struct

from tests import mont_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FORMS = list(M.FORMS)
SHORT = {(19, 4): 1025, (10, 8): 1025, (14, 8): 2049, (19, 8): 3073}
LIMB = 1 << M.W


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(GOLDEN, "extremal_moduli.json")) as f:
        return json.load(f)


def rsa_modulus(name):
    return next(int(e["n"], 16) for e in fixture()["rsa"] if e["name"] == name)


def form_id(form):
    return "%dx%d" % form


@functools.lru_cache(maxsize=None)
def moduli(form):
    """[(label, n)]"""
    B = M.FORMS[form]
    rng = random.Random(1000 * form[0] + form[1])
    odd = lambda bits: rng.getrandbits(bits - 1) | (1 << (bits - 1)) | 1          # noqa: E731
    short = ("full%d" % SHORT[form], rsa_modulus("full%d" % SHORT[form])) if SHORT[form] > 2048 else ("random%d" % SHORT[form], odd(SHORT[form]))
    return [("full%d" % B, rsa_modulus("full%d" % B)), ("sparse%d" % B, rsa_modulus("sparse%d" % B)), ("random%d" % B, odd(B)), short]


def _run_of(n, N, step):
    """Limbs equal to 2^28 at positions 0, step, 2 step, ...: as many as keep the value below 2n."""
    row = [0] * N
    for i in range(0, N, step):
        row[i] = LIMB
        if M.from_limbs(row) >= 2 * n:
            row[i] = 0
            break
    return row


def rows(form, n, label):
    """[(name, limb row)]: every value below 2n, every limb at most 2^28."""
    N = form[0] * form[1]
    rng = random.Random(label)
    out = [("0", M.to_limbs(0, N)), ("1", M.to_limbs(1, N)), ("n-1", M.to_limbs(n - 1, N)), ("n", M.to_limbs(n, N)), ("2n-1", M.to_limbs(2 * n - 1, N)),
           ("all2^28", _run_of(n, N, 1)), ("alt2^28", _run_of(n, N, 2)), ("random", M.to_limbs(rng.randrange(2 * n), N))]
    for _, r in out:
        assert M.from_limbs(r) < 2 * n and max(r) <= LIMB
    return out


def carry_pairs(form, n):
    """[(name, a, b)] with a b = t n + d R, d = 2^(28 m) - 1: mont_mul's output is n + d exactly.  m: the largest that keeps b
    below 2n, and one that ends in the third lane."""
    L, TPI = form
    N = L * TPI
    R = 1 << (M.W * N)
    a = 2 * n - 1                                                   # coprime to n
    m_max = ((a * n) // R).bit_length() // M.W
    while m_max > 0 and (1 << (M.W * m_max)) - 1 >= (a * n) // R:
        m_max -= 1
    if m_max == 0:
        return []                                                   # a modulus this far below R: the output never reaches n + 1
    out = []
    for m in sorted({m_max, min(m_max, 2 * L + 1)}):
        d = (1 << (M.W * m)) - 1
        t = (-d * R * pow(n, -1, a)) % a
        b, rem = divmod(t * n + d * R, a)
        assert rem == 0 and 0 < t and b < 2 * n
        assert (a * b + ((-a * b * pow(n, -1, R)) % R) * n) // R == n + d
        out.append(("n+2^(28*%d)-1" % m, M.to_limbs(a, N), M.to_limbs(b, N)))
    return out


class Case:
    __slots__ = ("label", "op", "k", "a", "b", "n", "n0inv", "nval", "residue", "random_only")

    def __init__(self, label, op, k, a, b, n_row, nval, residue, random_only=False):
        self.label, self.op, self.k, self.a, self.b, self.n, self.nval = label, op, k, a, b, n_row, nval
        self.n0inv = M.n0inv_of(nval)
        self.residue = residue                                      # the exact integer every output row must reduce to
        self.random_only = random_only                              # a random row under a random modulus: what the suite had


@functools.lru_cache(maxsize=None)
def cases(form):
    L, TPI = form
    N = L * TPI
    R = 1 << (M.W * N)
    out = []
    for mlabel, n in moduli(form):
        nrow = M.to_limbs(n, N)
        Ri = pow(R, -1, n)
        rs = rows(form, n, form_id(form) + mlabel)
        val = {name: M.from_limbs(r) for name, r in rs}
        rnd = mlabel.startswith("random")
        mk = lambda label, op, k, a, b, res, ro=False: out.append(Case("%s %s" % (mlabel, label), op, k, a, b, nrow, n, res % n, ro))   # noqa: E731
        for an, a in rs:
            for bn, b in rs:
                mk("MUL %s * %s" % (an, bn), M.MUL, 0, a, b, val[an] * val[bn] * Ri, rnd and an == bn == "random")
            mk("SQR %s" % an, M.SQR, 0, a, a, val[an] ** 2 * Ri, rnd and an == "random")
        # the to-Montgomery product at its largest x: every one of the N limbs full
        mk("MUL R-1 * R^2", M.MUL, 0, [M.MASK] * N, M.to_limbs(R * R % n, N), (R - 1) * R)
        for name, a, b in carry_pairs(form, n):
            mk("MUL " + name, M.MUL, 0, a, b, M.from_limbs(a) * M.from_limbs(b) * Ri)
        b = dict(rs)["random"]
        for an in ("n-1", "2n-1", "random"):
            mk("CHAIN64 %s" % an, M.CHAIN, 64, dict(rs)[an], b, pow(val[an], 1 << 64, n) * val["random"] * pow(Ri, 1 << 64, n), rnd and an == "random")
        # e = 65537 as k_rsa_modexp runs it: x R (the lazy output of the to-Montgomery product), 16 squarings, times plain x
        for xn, x in (("random", val["random"] % n), ("n-1", n - 1)):
            xr = M.mont_mul(M.to_limbs(x, N), M.to_limbs(R * R % n, N), nrow, M.n0inv_of(n), L, TPI)
            mk("CHAIN16 x=%s" % xn, M.CHAIN, 16, xr, M.to_limbs(x, N), pow(x, 65537, n), rnd and xn == "random")
    return out


@functools.lru_cache(maxsize=None)
def expected(form):
    """The model's (lazy, canonical, reduced) rows of every case, in order, and the Stats over the whole set."""
    st = M.Stats()
    L, TPI = form
    return [M.run_op(c.op, c.k, c.a, c.b, c.n, c.n0inv, L, TPI, st) for c in cases(form)], st


def travel(form, case, mut=()):
    st = M.Stats()
    M.run_op(case.op, case.k, case.a, case.b, case.n, case.n0inv, form[0], form[1], st, mut)
    return st


def all_maximum(form, bound=False):
    """Every limb of a and b at 2^28 and every limb of n at 2^28 - 1, the largest values mont_mul admits: the largest
    column value over the general and the squaring form.  The Montgomery factor m of a row is what these inputs make it; with
    `bound` every row's m is taken as 2^28 - 1 as well, which no input can exceed in any term: an upper bound for all inputs
    (the result is then no Montgomery product, only the columns' sizes mean something)."""
    L, TPI = form
    N = L * TPI
    top = 0
    for sqr in (False, True):
        st = M.Stats()
        M.mont_mul([LIMB] * N, [LIMB] * N, [M.MASK] * N, 1, L, TPI, sqr, st, (M.BOUND_M,) if bound else ())
        top = max(top, st.max_col)
    return top


# ---- the driver's byte layout (tests/c/mont_forms.hip)

def pack(form, case_list):
    L, TPI = form
    parts = [struct.pack("<3I", L, TPI, len(case_list))]
    for c in case_list:
        parts.append(struct.pack("<%dI" % (3 + 3 * L * TPI), c.op, c.k, c.n0inv, *c.a, *c.b, *c.n))
    return b"".join(parts)


def unpack(form, count, buf, off):
    """-> ([(lazy, canonical, reduced)], offset past the section)"""
    N = form[0] * form[1]
    out = []
    for _ in range(count):
        v = struct.unpack_from("<%dI" % (3 * N), buf, off)
        off += 12 * N
        out.append((list(v[:N]), list(v[N:2 * N]), list(v[2 * N:])))
    return out, off


def cut_sizes(form):
    """Group counts that put the last working group at, and just past, the end of a DPP row, a wave and a block."""
    t = form[1]
    return [1, 16 // t, 16 // t + 1, 64 // t, 64 // t + 1, 256 // t, 256 // t + 1]


def shuffled(form):
    """The indices of cases(form) in the order the device gets them: neighbours hold different moduli and operations."""
    idx = list(range(len(cases(form))))
    random.Random(form_id(form)).shuffle(idx)
    return idx


def mutation_table(muts=(M.MUT_NO_MASK, M.MUT_ROW_END, M.MUT_CANON_HOP, M.MUT_CANON_2HOPS)):
    """{(mutation, form): labels of the cases whose rows differ from the unmutated model's}.  The row-end defect needs a
    neighbour to read, so every case runs as the last group of a DPP row with the next case of the list behind it."""
    out = {}
    for form in FORMS:
        L, TPI = form
        cs, (exp, _) = cases(form), expected(form)
        for mut in muts:
            bad = []
            for i, c in enumerate(cs):
                if mut == M.MUT_ROW_END:
                    if c.op != M.MUL:
                        continue
                    nb = cs[(i + 1) % len(cs)]
                    pad = [(c.a, c.b, c.n, c.n0inv)] * (M.ROW // TPI) + [(nb.a, nb.b if nb.b else nb.a, nb.n, nb.n0inv)]
                    got = M.mont_mul_lanes(pad, L, TPI, False, None, (mut,))[M.ROW // TPI - 1]
                    if got != exp[i][0]:
                        bad.append(c.label)
                elif M.run_op(c.op, c.k, c.a, c.b, c.n, c.n0inv, L, TPI, None, (mut,)) != exp[i]:
                    bad.append(c.label + (" [random operands, random modulus]" if c.random_only else ""))
            out[(mut, form)] = bad
    return out


if __name__ == "__main__":
    for (mut, form), bad in mutation_table().items():
        print("%-26s %-5s %3d of %d fail: %s" % (mut, form_id(form), len(bad), len(cases(form)), "; ".join(bad)))
