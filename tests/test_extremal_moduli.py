"""CPU: tests/golden/extremal_moduli.json holds what tests/golden/make_extremal_moduli.py says it does -- the form, the
primality and the limb pattern of every modulus, the exponents its signer needs, and DSA groups that are groups."""
import random

import pytest

from tests import extremal_keys as X
from tests import mont_model as M

MASK = (1 << 28) - 1
SMALL = [3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]


def _probably_prime(n, rounds=6):
    if any(n % p == 0 for p in SMALL):
        return n in SMALL
    rng = random.Random(n & 0xFFFFFFFF)
    d, k = n - 1, 0
    while d % 2 == 0:
        d, k = d // 2, k + 1
    for i in range(rounds):
        x = pow(2 if i == 0 else rng.randrange(3, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(k - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_the_fixture_lists_every_modulus_and_group():
    fx = X.fixture()
    assert sorted(e["name"] for e in fx["rsa"]) == sorted(["full%d" % b for b in (2048, 2049, 3072, 3073, 4096)] + ["sparse%d" % b for b in (2048, 3072, 4096)])
    assert sorted(g["name"] for g in fx["dsa"]) == ["dsa2048_high", "dsa2048_low", "dsa3072_high", "dsa3072_low"]


@pytest.mark.parametrize("entry", X.fixture()["rsa"], ids=lambda e: e["name"])
def test_rsa_modulus(entry):
    n, B, j = int(entry["n"], 16), entry["bits"], entry["j"]
    assert n.bit_length() == B and 0 < j < 1 << 28
    limbs = M.to_limbs(n, (B + 27) // 28)
    if entry["form"] == "full":
        assert n == (1 << B) - (j << 28) - 1
        top = (1 << (B - 28 * (len(limbs) - 1))) - 1                      # the top limb is as full as the bit length lets it be
        assert [i for i, v in enumerate(limbs) if v != (top if i == len(limbs) - 1 else MASK)] == [1] and limbs[1] == MASK - j
        assert M.n0inv_of(n) == 1
    else:
        assert n == (1 << (B - 1)) + (j << 28) + 1
        assert [i for i, v in enumerate(limbs) if v] == [0, 1, len(limbs) - 1] and limbs[:2] == [1, j]
        assert M.n0inv_of(n) == MASK
    assert all((n - 1) % e for e in (3, 17, 65537))
    assert _probably_prime(n)
    # the closest candidate of the same form on the extremal side is no such prime: j is the first that is
    if j > 1:
        nb = n + (1 << 28) if entry["form"] == "full" else n - (1 << 28)
        assert not (all((nb - 1) % e for e in (3, 17, 65537)) and _probably_prime(nb, 2))


@pytest.mark.parametrize("grp", X.fixture()["dsa"], ids=lambda g: g["name"])
def test_dsa_group(grp):
    p, q, g, x = (int(grp[f], 16) for f in ("p", "q", "g", "x"))
    B = grp["bits"]
    assert p.bit_length() == B and q.bit_length() == 256 and (p - 1) % q == 0 and 0 < x < q
    assert _probably_prime(q) and _probably_prime(p)
    assert 1 < g < p and pow(g, q, p) == 1
    limbs = M.to_limbs(p, (B + 27) // 28)
    if grp["name"].endswith("high"):
        assert (1 << B) - p < q << 16                                      # within 2^16 candidates q m + 1 of 2^B ...
        assert all(v == MASK for v in limbs[10:-1])                        # ... so every limb above q's nine and a bit is full
    else:
        assert p - (1 << (B - 1)) < q << 16
        assert not any(limbs[10:-1]) and limbs[-1] == 1 << ((B - 1) % 28)


def test_signers_exist():
    for kp in X.rsa_keys():
        m = 0x1234567 << 900
        assert pow(kp.rsa_private(m), kp.e, kp.n) == m
    assert len(X.rsa_keys()) == 8 + 6 and len(X.dsa_keys()) == 4
