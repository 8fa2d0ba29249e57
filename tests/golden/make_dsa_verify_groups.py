"""Writes tests/golden/dsa_verify_groups.json: the small DSA groups (and three non-groups) of the DSA-verification tests, whose
moduli straddle a limb, a byte and the row ends of both lane forms.  Pure Python, seeded; a group takes a second or three, which
is why the result is a fixture.  Run from the repository root: python tests/golden/make_dsa_verify_groups.py"""
import json
import os
import random

SMALL = [p for p in range(3, 2000, 2) if all(p % d for d in range(3, int(p ** 0.5) + 1, 2))]


def is_prime(n: int, rng, rounds: int = 24) -> bool:
    if n < 2:
        return False
    if n in (2, 3):
        return True
    if n % 2 == 0:
        return False
    for sp in SMALL:
        if n % sp == 0:
            return n == sp
    d, k = n - 1, 0
    while d % 2 == 0:
        d, k = d // 2, k + 1
    for i in range(rounds):
        a = 2 if i == 0 else rng.randrange(2, n - 1)
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(k - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def low_half(rng, bits: int) -> int:
    """An odd number of exactly `bits` bits in the lowest quarter of that range, so that r + q and g + p still fit the bytes."""
    if bits <= 8:
        return rng.randrange(1 << (bits - 1), 1 << bits) | 1
    return (1 << (bits - 1)) | rng.randrange(1 << (bits - 3)) | 1


def prime_of(rng, bits: int) -> int:
    while True:
        c = low_half(rng, bits)
        if is_prime(c, rng):
            return c


def modulus_for(rng, q: int, pbits: int) -> int:
    """A prime p = k q + 1 of exactly pbits bits."""
    while True:
        p = low_half(rng, pbits)
        p -= (p - 1) % (2 * q)
        if p.bit_length() == pbits and is_prime(p, rng):
            return p


def generator(rng, p: int, q: int) -> int:
    while True:
        g = pow(rng.randrange(2, p - 1), (p - 1) // q, p)
        if g != 1:
            return g


def main():
    rng = random.Random(0xD5A7E51F)
    out = []
    for pbits, qbits in ((512, 160), (1016, 160), (1023, 224), (1025, 256), (2041, 160), (2047, 224), (2048, 256), (768, 64), (512, 8)):
        q = prime_of(rng, qbits)
        p = modulus_for(rng, q, pbits)
        out.append({"name": "p%d_q%d" % (pbits, qbits), "kind": "group", "p": p, "q": q, "g": generator(rng, p, q), "x": rng.randrange(1, q)})
        print(out[-1]["name"], flush=True)
    # non-groups: a composite odd order 3 q' of 160 bits under a prime p (g still has that order), a 161-bit order, and p = 1
    while True:
        q = 3 * prime_of(rng, 159)
        if q.bit_length() == 160:
            break
    p = modulus_for(rng, q, 1024)
    while True:
        g = pow(rng.randrange(2, p - 1), (p - 1) // q, p)
        if pow(g, q // 3, p) != 1 and pow(g, 3, p) != 1:
            break
    out.append({"name": "composite_q160", "kind": "composite", "p": p, "q": q, "g": g, "x": rng.randrange(1, q)})
    q = prime_of(rng, 161)
    p = modulus_for(rng, q, 1024)
    out.append({"name": "q161", "kind": "odd_width", "p": p, "q": q, "g": generator(rng, p, q), "x": rng.randrange(1, q)})
    out.append({"name": "p_is_1", "kind": "p_one", "p": 1, "q": prime_of(rng, 160), "g": 2, "x": rng.randrange(1, 1 << 159)})
    doc = {"generator": "tests/golden/make_dsa_verify_groups.py", "groups": [{k: (format(v, "x") if isinstance(v, int) else v) for k, v in g.items()} for g in out]}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "dsa_verify_groups.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
