"""The seeded corpus of the DSA-verification tests (CPU and GPU).  Not collected.

    groups() -> [Group]          the groups of tests/golden/dsa_verify_groups.json, then the first key of keys_dsa{1024,1536,2048,3072}
    corpus(name) -> (Case, ...)  Case = (label, part, p, q, g, y, digest, r, s)

Group = (name, kind, p, q, g, x, y, pbytes, qbytes): kind is "group" for a true group (prime q of whole bytes, g of order q), else
"composite", "odd_width" or "p_one"; pbytes / qbytes are the widths a call uses for it (qbytes alternates between the order's own
bytes and 32, as formatDSA's output and a wider caller would have it).  part is "honest", "mutation" (random single-bit flips of
an honest signature) or "constructed"; every Case carries its own g and y, since some cases replace them."""
import functools
import json
import math
import os
import zlib
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Group = namedtuple("Group", "name kind p q g x y pbytes qbytes")
Case = namedtuple("Case", "label part p q g y digest r s")
STANDARD = ("dsa1024", "dsa1536", "dsa2048", "dsa3072")


def nbytes(v: int) -> int:
    return (v.bit_length() + 7) // 8


@functools.lru_cache(maxsize=None)
def groups():
    out = []
    raw = [(g["name"], g["kind"], g) for g in json.load(open(os.path.join(GOLDEN, "dsa_verify_groups.json")))["groups"]]
    raw += [(name, "group", json.load(open(os.path.join(GOLDEN, "keys_%s.json" % name)))["keys"][0]) for name in STANDARD]
    for i, (name, kind, g) in enumerate(raw):
        p, q, gg, x = (int(g[k], 16) for k in ("p", "q", "g", "x"))
        out.append(Group(name, kind, p, q, gg, x, pow(gg, x, p), max(4, nbytes(p)), nbytes(q) if i % 2 == 0 else 32))
    return tuple(out)


def group(name: str) -> Group:
    return next(g for g in groups() if g.name == name)


def rnd(rng, m: int) -> int:
    return int.from_bytes(rng.bytes(nbytes(m) + 8), "big") % m


def sign(p, q, g, x, digest: bytes, k: int):
    """(r, s) of an honest signature over the whole digest, or None where k, r or s will not do."""
    if math.gcd(k, q) != 1:
        return None
    r = pow(g, k, p) % q
    s = pow(k, -1, q) * (int.from_bytes(digest, "big") + x * r) % q
    return (r, s) if r and s and math.gcd(s, q) == 1 else None


def sign_try(rng, G: Group, digest: bytes, g=None, want=lambda r, s: True, tries=60):
    """An honest signature (retrying k), or None."""
    for _ in range(tries):
        rs = sign(G.p, G.q, g or G.g, G.x, digest, rnd(rng, G.q) or 1)
        if rs and want(*rs):
            return rs
    return None


def sign_some(rng, G: Group, digest: bytes, g=None, want=lambda r, s: True):
    """An honest signature, or random r, s in [1, q) where the group allows none for this digest (p = 1: r would be 0; a
    composite q whose factor divides x and the digest: no s is invertible)."""
    return sign_try(rng, G, digest, g, want) or (1 + rnd(rng, G.q - 1), 1 + rnd(rng, G.q - 1))


def honest_pair(rng, G: Group, dlen: int):
    """A random digest of dlen bytes with an honest signature; under p = 1 there is none and r, s are random."""
    for _ in range(40):
        dg = rng.bytes(dlen)
        rs = sign_try(rng, G, dg, tries=8)
        if rs:
            return dg, rs
    return dg, sign_some(rng, G, dg)


def flip_int(v: int, bit: int) -> int:
    return v ^ (1 << bit)


def sig_bytes(G: Group, r: int, s: int) -> bytes:
    return r.to_bytes(G.qbytes, "big") + s.to_bytes(G.qbytes, "big")


@functools.lru_cache(maxsize=None)
def corpus(name: str):
    G = group(name)
    p, q, g, x, y = G.p, G.q, G.g, G.x, G.y
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    qb = q.bit_length() // 8
    rmax, pmax = 1 << (8 * G.qbytes), 1 << (8 * G.pbytes)
    cases = []
    add = lambda label, part, dg, r, s, gg=g, yy=y: cases.append(Case(label, part, p, q, gg, yy, dg, r, s))    # noqa: E731
    honest = {}
    for dlen in sorted({d for d in (1, qb - 1, qb) if d >= 1}):
        for j in range(3):
            dg, (r, s) = honest_pair(rng, G, dlen)
            add(f"honest dlen={dlen} #{j}", "honest", dg, r, s)
            honest[dlen] = (dg, r, s)
        dg, r, s = honest[dlen]
        for j in range(2):
            add(f"flip r dlen={dlen} #{j}", "mutation", dg, flip_int(r, int(rng.integers(8 * G.qbytes))), s)
            while True:       # (under a composite q a flipped s may lose its inverse: those are constructed below, not drawn)
                s2 = flip_int(s, int(rng.integers(8 * G.qbytes)))
                if not 0 < s2 < q or math.gcd(s2, q) == 1:
                    break
            add(f"flip s dlen={dlen} #{j}", "mutation", dg, r, s2)
            add(f"flip digest dlen={dlen} #{j}", "mutation", bytes(flip_int(int.from_bytes(dg, "big"), int(rng.integers(8 * dlen))).to_bytes(dlen, "big")), r, s)
            add(f"flip y dlen={dlen} #{j}", "mutation", dg, r, s, yy=flip_int(y, int(rng.integers(8 * G.pbytes))))
    dlen = max(honest)
    dg, r, s = honest[dlen]
    for label, rr, ss in (("r = 0", 0, s), ("r = q", q, s), ("r = q - 1", q - 1, s), ("s = 0", r, 0), ("s = q", r, q), ("s = q - 1", r, q - 1)):
        if max(rr, ss) < rmax:
            add(label, "constructed", dg, rr, ss)
    r2, s2 = sign_some(rng, G, dg, want=lambda r_, s_: r_ + q < rmax)
    if r2 + q < rmax:
        add("r + q", "constructed", dg, r2 + q, s2)
    # u1 = 0: an all-zero digest, honestly signed
    zero = bytes(dlen)
    add("digest = 0", "constructed", zero, *sign_some(rng, G, zero))
    # u2 small (its top windows are zero): s = r / t, and the digest that makes the signature honest
    for t in (1, 5):
        for _ in range(200):
            k = rnd(rng, q) or 1
            r3 = pow(g, k, p) % q
            if r3 and math.gcd(r3, q) == 1 and math.gcd(t, q) == 1:
                break
        if r3 and math.gcd(r3, q) == 1 and math.gcd(t, q) == 1:
            s3 = r3 * pow(t, -1, q) % q
            z3 = (k - x * t) * s3 % q            # u1 = z / s = k - x t, so that u1 + x u2 = k
            if qb >= 1 and z3 < (1 << (8 * qb)):
                add(f"u2 = {t}", "constructed", z3.to_bytes(max(qb, 1), "big"), r3, s3)
    # public values at and around the ends of [0, p)
    for label, yy in (("y = 0", 0), ("y = 1", 1), ("y = p", p), ("y = p + 1", p + 1)):
        if yy < pmax:
            add(label, "constructed", dg, r, s, yy=yy)
    # generators at and beyond p: 0, p (both 0 mod p), and g' + p for a generator g' of the same subgroup, honestly signed
    add("g = 0", "constructed", dg, r, s, gg=0)
    if p < pmax:
        add("g = p", "constructed", dg, r, s, gg=p)
    g2 = g
    for _ in range(2000):
        if g2 + p < pmax and g2 > 1:
            break
        g2 = g2 * g % p
    if g2 + p < pmax:
        r4, s4 = sign_some(rng, G, dg, g=g2)
        add("g >= p", "constructed", dg, r4, s4, gg=g2 + p, yy=pow(g2, x, p))
    # one byte more than the order has: fenced
    if qb + 1 <= 64:
        add("dlen = bytes(q) + 1", "constructed", dg + b"\x00" if len(dg) == qb else rng.bytes(qb + 1), r, s)
        add("dlen = bytes(q) + 1, r = 0", "constructed", rng.bytes(qb + 1), 0, s)
    if G.kind == "composite":
        for m in (1, 2, 5):
            add(f"s = {3 * m}", "constructed", dg, r, 3 * m)
        add("s = q / 3", "constructed", dg, r, q // 3)
        for j in range(3):
            dg5, rs5 = honest_pair(rng, G, dlen)
            add(f"s coprime to q #{j}", "constructed", dg5, *rs5)
        add("s = 3 and one byte more", "constructed", rng.bytes(qb + 1), r, 3)          # FENCED wins over NO_INVERSE
    return tuple(cases)


def by_dlen(cases):
    out = {}
    for i, cs in enumerate(cases):
        out.setdefault(len(cs.digest), []).append(i)
    return out


def tables(cases):
    """The group and key tables of one call over `cases`: ([(p, q, g)], [(group, y)], key_idx)."""
    gs, ks, idx = [], [], []
    for cs in cases:
        grp = (cs.p, cs.q, cs.g)
        if grp not in gs:
            gs.append(grp)
        key = (gs.index(grp), cs.y)
        if key not in ks:
            ks.append(key)
        idx.append(ks.index(key))
    return gs, ks, idx
