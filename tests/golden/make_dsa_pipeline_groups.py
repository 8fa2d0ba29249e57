"""Writes tests/golden/dsa_pipeline_groups.json: the DSA groups and non-groups that tests/dsa_pipeline_cases.py adds to those of
dsa_verify_groups.json and extremal_moduli.json -- orders at and beyond both ends of what the OpenPGP pipeline's key table admits
(32 .. 256 bits, odd), a composite 256-bit order, a 256-bit order just above 2^255, p = 3, an even q and an even p.
Pure Python, seeded, Miller-Rabin; a few seconds.  Run from the repository root: python tests/golden/make_dsa_pipeline_groups.py"""
import json
import os
import random

SMALL = [p for p in range(3, 4000, 2) if all(p % d for d in range(3, int(p ** 0.5) + 1, 2))]
SEED = 0xD5A0917E


def is_prime(n: int, rng, rounds: int = 24) -> bool:
    if n < 2:
        return False
    if n % 2 == 0:
        return n == 2
    for sp in SMALL:
        if n % sp == 0:
            return n == sp
    d, k = n - 1, 0
    while d % 2 == 0:
        d, k = d // 2, k + 1
    for i in range(rounds):
        x = pow(2 if i == 0 else rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(k - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_of(rng, bits: int, lo_frac: int = 0) -> int:
    """A prime of exactly `bits` bits; with lo_frac, within 2^(bits - 1 - lo_frac) of the lower end of that range."""
    while True:
        c = (1 << (bits - 1)) | rng.randrange(1 << (bits - 1 - lo_frac)) | 1
        if is_prime(c, rng):
            return c


def modulus_for(rng, order: int, pbits: int) -> int:
    """A prime p = k * order + 1 of exactly pbits bits."""
    while True:
        p = (1 << (pbits - 1)) | rng.randrange(1 << (pbits - 2))
        p -= (p - 1) % (2 * order)
        if p.bit_length() == pbits and is_prime(p, rng):
            return p


def element_of_order(rng, p: int, order: int, factors) -> int:
    """g of exactly that order mod p (factors: the prime factors of the order)."""
    while True:
        g = pow(rng.randrange(2, p - 1), (p - 1) // order, p)
        if g != 1 and all(pow(g, order // f, p) != 1 for f in factors):
            return g


def build():
    rng = random.Random(SEED)
    out = []

    def add(name, kind, p, q, g):
        out.append({"name": name, "kind": kind, "p": p, "q": q, "g": g, "x": rng.randrange(2, max(q, 4) - 1)})

    # true groups: the narrowest order the key table admits, one byte more, and the widest below the 256-bit class
    for qbits, pbits in ((32, 1024), (40, 1024), (248, 1024)):
        q = prime_of(rng, qbits)
        p = modulus_for(rng, q, pbits)
        add("p%d_q%d" % (pbits, qbits), "group", p, q, element_of_order(rng, p, q, (q,)))
    # a 256-bit prime order within 2^-40 of 2^255: the digest, cut to 256 bits, is not below q every other time
    q = prime_of(rng, 256, lo_frac=40)
    p = modulus_for(rng, q, 2048)
    add("p2048_q256_low", "group", p, q, element_of_order(rng, p, q, (q,)))
    # orders beyond both ends (true groups all the same)
    for qbits, pbits in ((24, 512), (264, 1024)):
        q = prime_of(rng, qbits)
        p = modulus_for(rng, q, pbits)
        add("p%d_q%d" % (pbits, qbits), "group", p, q, element_of_order(rng, p, q, (q,)))
    # a composite 256-bit order 3 * 5 * q' under a 2048-bit prime, g of exactly that order
    while True:
        q1 = prime_of(rng, 253)
        if (15 * q1).bit_length() == 256:
            break
    p = modulus_for(rng, 15 * q1, 2048)
    add("composite_q256", "composite", p, 15 * q1, element_of_order(rng, p, 15 * q1, (3, 5, q1)))
    # no groups at all
    add("p_is_3", "no_group", 3, prime_of(rng, 160), 2)
    p = modulus_for(rng, prime_of(rng, 160), 1024)
    add("even_q", "no_group", p, 2 * prime_of(rng, 159), rng.randrange(2, p - 1))
    add("even_p", "no_group", 2 * prime_of(rng, 1023), prime_of(rng, 160), rng.randrange(2, 1 << 1000))
    doc = {"generator": "tests/golden/make_dsa_pipeline_groups.py",
           "groups": [{k: (format(v, "x") if isinstance(v, int) else v) for k, v in g.items()} for g in out]}
    return json.dumps(doc, indent=1) + "\n"


def main():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "dsa_pipeline_groups.json"), "w") as f:
        f.write(build())


if __name__ == "__main__":
    main()
