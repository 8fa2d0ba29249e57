"""A plain-Python restatement of threshold DSA / ECDSA signing (crypto/threshold/dsa/dsa_core.go, dsa.go, ecdsa.go; crypto/sss/sss.go)
on Python integers, for the share-answer tests (CPU and GPU).  Builds on tests/ec_ref.py.  Not collected.

    distribute(rng, secret, n, t, q)     sss.Distribute: a degree t - 1 polynomial at x = 1 .. n           -> [(x, y)]
    joint_random / joint_zero            generateJointRandom / generateJointZero (dsa_core.go:165-175)
    fold(shares, q)                      decrypt's fold of (k, a, b, c) shares (:235-238)                   -> (ki, ai, bi, ci)
    phase2(G, shares)                    Sign's second phase (:126-141)                                     -> Answer(ki, ai, bi, ci, ri, vi)
    phase3(q, r, y, m, k, c)             Sign's last phase (:150-155)                                       -> si
    calculate_r(G, partials)             CalculateR (dsa.go:33-53; ecdsa.go:36-59 through ec_ref)           -> r
    calculate_s(coords, q), format_dsa   calculateS, formatDSA (:338-366)
    sign(G, n, t, responders, x, digest, rng)   the whole protocol among `responders` servers              -> Run

A group G is dsa_group(p, q, g) or ec_group(curve): .q, .partial_r(ai) -> bytes as sent (fixed width here: .Bytes() left-padded /
Marshal), .os2i(digest), .calculate_r(partials) with partials [(x, ri bytes, vi)].

Two rules rest on memory of Go, not on the reference's text (docs/parity.md): big.Int.Mod of a non-negative value by a positive
modulus is the mathematical residue (Python's %), and ScalarBaseMult of an empty slice (ai = 0, whose .Bytes() is empty) returns the
affine (0, 0), which Marshal writes as 04 || 0 .. 0."""
from collections import namedtuple

import ec_ref as E
import ecdsa_verify_ref as EV

OK, FAILED = 0, 0xFF
Answer = namedtuple("Answer", "ki ai bi ci ri vi")
Run = namedtuple("Run", "r s sig k_total answers si")
Group = namedtuple("Group", "kind q pbytes qbytes partial_r os2i calculate_r params")


def lagrange(x, xs, q):
    a, b = 1, 1
    for o in xs:
        if o == x:
            continue
        a *= o
        b *= o - x
    return a * pow(b % q, -1, q) % q


def distribute(rng, secret, n, t, q):
    poly = [secret] + [rng.randrange(q) for _ in range(t - 1)]
    out = []
    for i in range(n):
        x0, x, f = i + 1, i + 1, poly[0]
        for j in range(1, t):
            f = (f + poly[j] * x) % q
            x *= x0
        out.append((i + 1, f))
    return out


def joint_random(rng, t, n, q):
    return distribute(rng, rng.randrange(q), n, t, q)


def joint_zero(rng, t, n, q):
    return distribute(rng, 0, n, t, q)


def fold(shares, q):
    """shares: [(k, a, b, c)] non-negative integers (ReadBigInt is SetBytes), one Mod per addition as decrypt has it"""
    acc = [0, 0, 0, 0]
    for sh in shares:
        for i in range(4):
            acc[i] = (acc[i] + sh[i]) % q
    return tuple(acc)


def vi_of(q, ki, ai, bi):
    return ((ki * ai % q) + bi) % q


def phase2(G, shares):
    ki, ai, bi, ci = fold(shares, G.q)
    return Answer(ki, ai, bi, ci, G.partial_r(ai), vi_of(G.q, ki, ai, bi))


def phase3(q, r, y, m, k, c):
    si = r * y % q
    si = (si + m) % q
    si = si * k % q
    return (si + c) % q


def calculate_s(coords, q):
    xs = [x for x, _ in coords]
    s = 0
    for x, y in coords:
        s = (s + y * lagrange(x, xs, q) % q) % q
    return s


def format_dsa(r, s, q):
    n = (q.bit_length() + 7) // 8
    return r.to_bytes(n, "big") + s.to_bytes(n, "big")


def dsa_group(p, q, g, pbytes=None, qbytes=None):
    pb = pbytes or max(1, (p.bit_length() + 7) // 8)
    qb = qbytes or max(1, (q.bit_length() + 7) // 8)

    def calc_r(partials):
        xs = [x for x, _, _ in partials]
        r, v = 1, 0
        for x, ri, vi in partials:
            lam = lagrange(x, xs, q)
            r = r * pow(int.from_bytes(ri, "big"), lam, p) % p
            v = (v + vi * lam % q) % q
        return pow(r, pow(v, -1, q), p) % q
    return Group("dsa", q, pb, qb, lambda ai: (pow(g, ai, p) if p > 1 else 0).to_bytes(pb, "big"),
                 lambda dg: int.from_bytes(dg[:(q.bit_length() + 7) // 8], "big"), calc_r, (p, q, g))


def ec_group(c):
    f = E.byte_len(c)

    def calc_r(partials):
        st, r = E.calculate_r(c, [x for x, _, _ in partials], [ri for _, ri, _ in partials], [vi for _, _, vi in partials])
        assert st == E.OK
        return r
    return Group("ec", c["n"], 1 + 2 * f, f, lambda ai: E.calculate_partial_r(c, ai), lambda dg: EV.hash_to_int(c, dg), calc_r, c)


def sign(G, n, t, responders, x, digest, rng):
    """The protocol among the servers `responders` (0-based indices into the n nodes), however many they are: phase 1 at every
    responder, the client's kmap, phase 2 and 3 at every responder, CalculateR, calculateS, formatDSA.  The reference waits for 2t."""
    q = G.q
    key = distribute(rng, x, n, t, q)                                    # Distribute: share i belongs to node i
    joint = {}                                                           # phase 1 at responder j: coordinates for every node
    for j in responders:
        joint[j] = (joint_random(rng, t, n, q), joint_random(rng, t, n, q), joint_zero(rng, 2 * t, n, q), joint_zero(rng, 2 * t, n, q))
    answers = {}
    for i in responders:                                                 # phase 2 at node i: one share from every responder
        shares = [tuple(joint[j][col][i][1] for col in range(4)) for j in responders]
        assert all(joint[j][col][i][0] == i + 1 for j in responders for col in range(4))
        answers[i] = phase2(G, shares)
    r = G.calculate_r([(i + 1, answers[i].ri, answers[i].vi) for i in responders])
    m = G.os2i(digest)
    si = {i: phase3(q, r, key[i][1], m, answers[i].ki, answers[i].ci) for i in responders}
    s = calculate_s([(i + 1, si[i]) for i in responders], q)
    k_total = sum(_secret(joint[j][0], t, q) for j in responders) % q      # the k the shares add up to
    return Run(r, s, format_dsa(r, s, q), k_total, answers, si)


def _secret(coords, t, q):
    """f(0) of a degree t - 1 polynomial from its first t coordinates"""
    pts = coords[:t]
    xs = [x for x, _ in pts]
    return sum(y * lagrange(x, xs, q) for x, y in pts) % q
