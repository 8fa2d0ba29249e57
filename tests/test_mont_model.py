"""The lane-by-lane model of csrc/mont28.h (tests/mont_model.py) against exact integer arithmetic on the operand set of
tests/mont_cases.py, the figures the header's overflow argument rests on, and the cross-compile of the driver that runs the
same set on the device (tests/c/mont_forms.hip; tests/test_gpu_mont_forms.py runs it).  No tolerance anywhere: every
comparison is integer equality.

Measured here (model, unbounded integers), per form L x TPI; DESIGN.md section 3.1 carries the table:

                                              19x4        10x8        14x8        19x8
  largest column, operand set      / 2^64     0.14844     0.07812     0.10937     0.14844
  largest column, all-maximum      / 2^64     0.07422     0.03906     0.05469     0.07422
  largest column, m forced to max  / 2^64     0.14844     0.07813     0.10938     0.14844    (2L products of 2^56: the bound)
  largest output limb                         2^28        2^28        2^28        2^28

All-maximum is every limb of a and b at 2^28 and every limb of n at 2^28 - 1; the Montgomery factors these inputs produce are
small, which is why the operand set (full modulus, operands 2n - 1) gets higher: it comes within 10^-8 of the bound."""
import os
import subprocess

import pytest

from tests import mont_cases as K
from tests import mont_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_IDS = [K.form_id(f) for f in K.FORMS]


@pytest.mark.parametrize("form", K.FORMS, ids=FORM_IDS)
def test_model_is_exact_on_the_operand_set(form):
    """The lazy output is congruent to the exact residue, below 2n, with every limb <= 2^28; canonicalize leaves the same
    integer with every limb < 2^28; reduce_once leaves the residue itself.  For CHAIN cases the residue is pow()'s."""
    cs, (exp, _) = K.cases(form), K.expected(form)
    assert 300 <= len(cs) <= 400
    bad = []
    for c, (lazy, canon, red) in zip(cs, exp):
        y = M.from_limbs(lazy)
        ok = (y % c.nval == c.residue and y < 2 * c.nval and max(lazy) <= 1 << M.W
              and M.from_limbs(canon) == y and max(canon) < 1 << M.W
              and M.from_limbs(red) == c.residue and max(red) < 1 << M.W)
        if not ok:
            bad.append(c.label)
    assert not bad, bad[:10]


@pytest.mark.parametrize("form", K.FORMS, ids=FORM_IDS)
def test_chains_equal_pow(form):
    """The residues the CHAIN cases are held to, restated with nothing but pow(): 2^k-th power of a, times b, with the factor
    R^-(2^k) the Montgomery products leave; and x^65537 for the e = 65537 schedule."""
    L, TPI = form
    R = 1 << (M.W * L * TPI)
    cs, (exp, _) = K.cases(form), K.expected(form)
    seen = 0
    for c, (_, _, red) in zip(cs, exp):
        if c.op != M.CHAIN:
            continue
        seen += 1
        a, b, n = M.from_limbs(c.a), M.from_limbs(c.b), c.nval
        assert M.from_limbs(red) == pow(a, 1 << c.k, n) * b * pow(R, -(1 << c.k), n) % n, c.label
        if c.k == 16:
            assert M.from_limbs(red) == pow(b, 65537, n), c.label
    assert seen == 4 * 5


@pytest.mark.parametrize("form", K.FORMS, ids=FORM_IDS)
def test_columns_fit_64_bits(form):
    """The largest value any column accumulator holds: over the operand set, over the all-maximum inputs, and with every
    row's Montgomery factor forced to 2^28 - 1 on top of them -- which bounds every input.  A column receives one a b and one
    m n product from each of the L rows it is in the window for, 2L products of less than 2^56 (2^57 halved in count for
    the doubled terms of a squaring), plus carries: NOT 2 TPI L products, as mont28.h used to say."""
    L, TPI = form
    _, st = K.expected(form)
    amax, bound = K.all_maximum(form), K.all_maximum(form, bound=True)
    print("%s: largest column over the operand set %d (%.4f x 2^64), all-maximum %d (%.4f), m forced %d (%.4f); largest output limb %#x"
          % (K.form_id(form), st.max_col, st.max_col / 2**64, amax, amax / 2**64, bound, bound / 2**64, st.max_limb))
    assert st.max_col < 1 << 64 and amax < 1 << 64 and bound < 1 << 64
    assert st.max_col <= bound and amax <= bound
    assert bound < (2 * L + 1) << 56                                  # 2L products and less than one more in carries
    assert st.max_limb == 1 << M.W                                    # the lazy form's 2^28 limb does occur in the set


@pytest.mark.parametrize("form", K.FORMS, ids=FORM_IDS)
def test_operand_set_drives_carries_across_lanes(form):
    """What the search put into the set: the cross-lane hop's ripple reaches the third limb; canonicalize's carry starts in
    lane 1 (lane 0 takes no carry in, so it stays canonical) and travels to the top lane, TPI - 2 hops, the longest there is;
    reduce_once's borrow crosses every lane.  (Under a 2048-bit modulus the 80-limb form's R is so far above n that the
    constructed outputs n + 2^(28 m) - 1 stop at m = 66, in lane 6; there the full modulus' own carry chain does the rest.)"""
    L, TPI = form
    cs, (_, st) = K.cases(form), K.expected(form)
    assert st.hop_third > 0 and st.canon_hops == TPI - 2 and st.borrow_hops == TPI - 1
    by = {c.label: c for c in cs}
    B = M.FORMS[form]
    assert K.travel(form, by["sparse%d MUL n * random" % B]).canon_hops == TPI - 2
    top = [c for c in cs if " MUL n+2^(28*" in c.label]                # the constructed outputs n + 2^(28 m) - 1
    assert len(top) >= 4 and max(K.travel(form, c).borrow_hops for c in top) >= TPI - 2


@pytest.mark.parametrize("form", K.FORMS, ids=FORM_IDS)
def test_neighbouring_groups_do_not_meet(form):
    """Two DPP rows and a bit of groups holding different numbers under different moduli, side by side as a wave holds them:
    each gives what it gives alone.  (The last lane of a group reads the next group's lane 0, whose retired columns are zero
    by construction; the last lane of a row reads 0.)"""
    L, TPI = form
    cs = [K.cases(form)[i] for i in K.shuffled(form) if K.cases(form)[i].op == M.MUL][:2 * M.ROW // TPI + 1]
    assert len({c.nval for c in cs}) > 2
    for sqr in (False, True):
        rows = M.mont_mul_lanes([(c.a, c.b, c.n, c.n0inv) for c in cs], L, TPI, sqr)
        assert rows == [M.mont_mul(c.a, c.b, c.n, c.n0inv, L, TPI, sqr) for c in cs]


def test_the_set_notices_defects():
    """That the comparison bites (the whole table is in docs/history.md; `python -m tests.mont_cases` prints it).  Without the
    28-bit mask on the limb taken from the next lane, and with two carry steps fewer in canonicalize, named cases of the set
    come out wrong while the random row under the random modulus does not.  One step fewer in canonicalize, and a row's last
    lane reading its neighbour, change nothing: mont_mul's lane 0 never carries out and its retired columns are zero."""
    form = (14, 8)
    L, TPI = form
    cs, (exp, _) = K.cases(form), K.expected(form)
    by = {c.label: i for i, c in enumerate(cs)}
    run = lambda i, mut: M.run_op(cs[i].op, cs[i].k, cs[i].a, cs[i].b, cs[i].n, cs[i].n0inv, L, TPI, None, (mut,))     # noqa: E731
    rnd = by["random3072 MUL random * random"]
    assert cs[rnd].random_only
    i = by["sparse3072 MUL n * random"]
    assert run(i, M.MUT_CANON_2HOPS) != exp[i] and run(i, M.MUT_CANON_HOP) == exp[i]
    assert run(rnd, M.MUT_CANON_2HOPS) == exp[rnd]
    i = by["full3072 MUL 2n-1 * 2n-1"]
    assert run(i, M.MUT_NO_MASK) != exp[i]


def test_driver_cross_compiles(tmp_path):
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "c", "mont_forms.hip"),
                        "-o", str(tmp_path / "mont_forms")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
