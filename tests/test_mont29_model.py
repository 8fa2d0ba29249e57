"""CPU: the 18 x 4 form at radix 2^29 (k_rsa_modexp<18,4,29>, csrc/mont28.h with W = 29) on the lane-by-lane model
(tests/mont_model.py, its limb width set to 29 bits through MonkeyPatch: tests/mont29_cases.py) -- exact residues on the
operand set, the size of the 64-bit column accumulators, the size of the output limbs, and a defect the set must notice.

Recorded: with every limb of a at 2^29, every limb of n and every row's Montgomery factor at 2^29 - 1 the largest column is
exactly 0.5625 * 2^64 = 36 * 2^58, general and squaring form alike (0.28125 * 2^64 with the factors those operands really
give); over the operand set 0.5625 * 2^64 to four places (rows of 2^29 limbs under the sparse modulus, whose limbs are all
ones) and no output limb above 2^29; without the limb mask 120 of 152 single products differ."""

from tests import mont29_cases as K
from tests import mont_model as M


def test_model_is_back_at_28_bits_outside_the_block():
    with K.width29():
        assert (M.W, M.MASK) == (29, (1 << 29) - 1)
    assert (M.W, M.MASK) == (28, (1 << 28) - 1)
    assert not M.is_norm(K.L, K.TPI)                    # the ring window, no block-boundary normalisation


def test_exact_residues_on_the_whole_set():
    cs, (exp, st) = K.cases(), K.expected()
    assert len(cs) > 400
    bad = []
    for c, (lazy, canon, red) in zip(cs, exp):
        v = K.from_limbs(lazy)
        ok = v < 2 * c.nval or c.nval < 1 << 64         # value < 2n (the 64-bit modulus: R / n is huge, outputs stay below n + 1)
        if not (ok and v % c.nval == c.residue and K.from_limbs(canon) == v and max(canon) <= K.MASK
                and K.from_limbs(red) == c.residue and max(red) <= K.MASK):
            bad.append(c.label)
    assert not bad, bad[:10]
    print("largest column over the set: %.4f * 2^64; largest output limb 2^29 + %d" % (st.max_col / 2.0 ** 64, st.max_limb - K.LIMB))
    assert st.max_col < 1 << 64
    assert st.max_limb <= K.LIMB


def test_column_bound_with_every_factor_at_its_maximum():
    """36 products of at most 2^29 * 2^29 (a squaring's doubled ones 2^30 * 2^29, and half as many) plus the carry of the
    column before: expected 0.5625 * 2^64 = 36 * 2^58."""
    free = K.all_maximum(bound=False)
    bound = K.all_maximum(bound=True)
    print("largest column, all-maximum operands: %s; with every m at 2^29 - 1: %s (in units of 2^64)"
          % (["%.6f" % (v / 2.0 ** 64) for v in free], ["%.6f" % (v / 2.0 ** 64) for v in bound]))
    for v in free + bound:
        assert v < 1 << 64
    assert max(bound) >= max(free)
    assert [round(v / 2.0 ** 64, 4) for v in bound] == [0.5625, 0.5625]


def test_e65537_schedule_random_moduli():
    """to-Montgomery, 16 lazy squarings, last product by plain x (shortcut) or by xR and then by 1, under random moduli of
    512, 1025, 2047 and 2048 bits and moduli 2^2048 - j 2^29 - 1: equal to pow(x, 65537, n), columns below 2^64, limbs at most 2^29."""
    import random
    rng = random.Random(65537)
    mods = [rng.getrandbits(b - 1) | (1 << (b - 1)) | 1 for b in (512, 1025, 2047, 2048)] + [(1 << 2048) - j * (1 << 29) - 1 for j in (1, 3)]
    st = M.Stats()
    with K.width29():
        for n in mods:
            nrow, n0 = K.to_limbs(n), K.n0inv_of(n)
            x = rng.randrange(n)
            xr = M.mont_mul(K.to_limbs(x), K.to_limbs(K.R * K.R % n), nrow, n0, K.L, K.TPI, False, st)
            y = M.run_op(M.CHAIN, 16, xr, K.to_limbs(x), nrow, n0, K.L, K.TPI, st)
            # the x-shortcut's claim: the last product leaves y < n (1 + 2^-39), so y itself is the residue or the residue + n
            assert K.from_limbs(y[0]) < n + (n >> 39) + 1
            assert K.from_limbs(y[2]) == pow(x, 65537, n)
            z = M.run_op(M.CHAIN, 16, xr, xr, nrow, n0, K.L, K.TPI, st)[0]
            one = M.run_op(M.MUL, 0, K.to_limbs(1), z, nrow, n0, K.L, K.TPI, st)
            assert K.from_limbs(one[0]) <= n and K.from_limbs(one[2]) == pow(x, 65537, n)
    assert st.max_col < 1 << 64 and st.max_limb <= K.LIMB


def test_the_set_bites_without_the_limb_mask():
    """MUT_NO_MASK (the limb read from the next lane keeps all its 32 bits): most single products of the set come out wrong."""
    cs, (exp, _) = K.cases(), K.expected()
    single = [(c, e) for c, e in zip(cs, exp) if c.op != M.CHAIN and c.label.split()[0] in ("full2048", "random1025")]
    with K.width29():
        bad = sum(M.run_op(c.op, c.k, c.a, c.b, c.n, c.n0inv, K.L, K.TPI, None, (M.MUT_NO_MASK,)) != e for c, e in single)
    print("MUT_NO_MASK: %d of %d cases differ" % (bad, len(single)))
    assert bad > len(single) // 2
