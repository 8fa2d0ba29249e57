"""Writes tests/golden/extremal_moduli.json: prime moduli whose radix-2^28 limbs are as full or as empty as a modulus can
have them, and DSA groups at the two ends of their size class.

  full    the largest prime 2^B - j 2^28 - 1: every limb but one is 0x0FFFFFFF, -n^-1 mod 2^28 = 1
  sparse  the smallest prime 2^(B-1) + j 2^28 + 1: all limbs but three are zero, -n^-1 mod 2^28 = 2^28 - 1
for B = 2048, 3072, 4096, and the full form at 2049 and 3073 bits (the shortest moduli of the 112- and 152-limb forms).  Every
prime p has p - 1 coprime to 3, 17 and 65537, so that d = e^-1 mod (p - 1) exists for the public exponents the suite uses: a
prime modulus gives a signer without factoring, and neither the library nor the reference asks for two primes.

DSA groups for p of 2048 and 3072 bits under a 256-bit prime q (the largest below 2^256): `high` is the largest prime
q m + 1 below 2^B (its top limbs all full), `low` the smallest above 2^(B-1); g = h^((p-1)/q) for the smallest h that gives
g != 1, x seeded.

Pure Python; the 4096-bit search takes about a minute, the rest seconds.  Run from the repository root:
python tests/golden/make_extremal_moduli.py"""
import json
import os
import random

SMALL = [p for p in range(3, 20000, 2) if all(p % d for d in range(3, int(p ** 0.5) + 1, 2))]
EXPONENTS = (3, 17, 65537)


def is_prime(n, rng, rounds=16):
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


def rsa_prime(rng, form):
    j = 1
    while True:
        p = form(j)
        if all((p - 1) % e for e in EXPONENTS) and is_prime(p, rng):
            return j, p
        j += 1


def dsa_group(rng, q, bits, high):
    m = ((1 << bits) - 2) // q if high else -(-(1 << (bits - 1)) // q)
    m -= m % 2
    if not high and q * m + 1 < 1 << (bits - 1):
        m += 2
    while True:
        p = q * m + 1
        assert p.bit_length() == bits
        if is_prime(p, rng):
            break
        m += -2 if high else 2
    h = 2
    while pow(h, (p - 1) // q, p) == 1:
        h += 1
    return p, pow(h, (p - 1) // q, p)


def main():
    rng = random.Random(0xE7E3A1)
    rsa = []
    for name, bits, form in [("full%d" % B, B, (lambda j, B=B: (1 << B) - (j << 28) - 1)) for B in (2048, 3072, 2049, 3073, 4096)] + \
                            [("sparse%d" % B, B, (lambda j, B=B: (1 << (B - 1)) + (j << 28) + 1)) for B in (2048, 3072, 4096)]:
        j, p = rsa_prime(rng, form)
        assert p.bit_length() == bits
        rsa.append({"name": name, "bits": bits, "form": name.rstrip("0123456789"), "j": j, "n": format(p, "x")})
        print(name, j, flush=True)
    q = (1 << 256) - 1
    while not is_prime(q, rng, 32):
        q -= 2
    dsa = []
    for bits in (2048, 3072):
        for high in (True, False):
            p, g = dsa_group(rng, q, bits, high)
            dsa.append({"name": "dsa%d_%s" % (bits, "high" if high else "low"), "bits": bits, "p": format(p, "x"), "q": format(q, "x"),
                        "g": format(g, "x"), "x": format(rng.randrange(1, q), "x")})
            print(dsa[-1]["name"], flush=True)
    doc = {"generator": "tests/golden/make_extremal_moduli.py", "rsa": rsa, "dsa": dsa}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "extremal_moduli.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
