"""One seeded corpus for the password-authentication entries (tests/test_tpa_reference.py asserts its coverage, tests/test_gpu_tpa.py
runs it on the device).  An Op is generic: the same (modulus, base v, raw Xi, exponent b, salt) is one makeYi (x = v, y = b), one
makeBi (v, Xi, b, salt) and one processBi (Bi = v as given, Xi, e = b, salt).  `tags` names the classes an Op stands for."""
import functools
import json
import os
import random
from collections import namedtuple

import tpa_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
Op = namedtuple("Op", "p nbytes v xi b exp_len salt tags")

SHAPES = [(256, 256, 32), (256, 32, 16), (256, 1, 0), (128, 255, 64), (128, 256, 16), (255, 32, 32), (128, 1, 64), (255, 255, 0)]      # (nbytes, exp_len, salt_len)
XI_LENS = [0, 1, 55, 56, 63, 64, 119, 120, 255, 256]
BASE_CLASSES = ["0", "1", "2", "p-1", "p", "p+1", "max", "random"]


def _golden(name):
    return json.load(open(os.path.join(HERE, "golden", name)))


@functools.lru_cache(maxsize=None)
def moduli():
    """name -> odd modulus: the reference's p, extremal 2048-bit forms, and RSA moduli off the byte and off the limb."""
    m = {"auth_p": R.P}
    for r in _golden("extremal_moduli.json")["rsa"]:
        if r["bits"] == 2048:
            m[r["name"]] = int(r["n"], 16)
    for bits in (1023, 1024, 1025, 2041, 2047):
        k = _golden("keys_rsa%d.json" % bits)["keys"][0]
        m["rsa%d" % bits] = int(k["p"], 16) * int(k["q"], 16)
    assert all(v & 1 for v in m.values())
    return m


def moduli_for(nbytes):
    return [(k, v) for k, v in moduli().items() if (v.bit_length() + 7) // 8 <= nbytes]


def exponent_classes(exp_len, every_edge):
    """(tag, exponent) for every class that fits exp_len bytes.  every_edge: 2^k and 2^k - 1 at EVERY limb edge k = 28 j (the shape
    128/256/16 carries them: the restatement's pow is four times cheaper under a 1024-bit modulus); the other shapes take the edges at
    the ends and in the middle."""
    bits = 8 * exp_len
    out = [(str(v), v) for v in (0, 1, 2, 15, 16) if v < 1 << bits]
    ks = set()
    if every_edge:
        ks.update(28 * j for j in range(1, bits // 28 + 1))
    for j in (1, 36, 73) + ((2, 37, 72) if every_edge else ()):      # limb edges of the radix-2^28 form and their neighbours
        ks.update((28 * j - 1, 28 * j, 28 * j + 1))
    for i in (1, 255, 511) + ((2, 8, 256, 510) if every_edge else ()):      # window edges (4 i) and their neighbours
        ks.update((4 * i - 1, 4 * i, 4 * i + 1))
    for k in sorted(ks):
        if k < bits:
            out.append(("2^%d" % k, 1 << k))
        if k <= bits:
            out.append(("2^%d-1" % k, (1 << k) - 1))
    out.append(("ones", (1 << bits) - 1))
    out.append(("0f", int.from_bytes(b"\x0f" * exp_len, "big")))
    out.append(("f0", int.from_bytes(b"\xf0" * exp_len, "big")))
    if exp_len == 256:
        out += [("q", R.Q), ("p-1", R.P - 1)]
    return out


def _base(rng, cls, p, nbytes):
    top = (1 << (8 * nbytes)) - 1
    v = {"0": 0, "1": 1, "2": 2, "p-1": p - 1, "p": p, "p+1": p + 1, "max": top}.get(cls)
    return min(v, top) if v is not None else rng.randrange(top + 1)


def _full_width_power(rng, p, nbytes, exp_len):
    """(v, b) with v^b mod p of exactly nbytes bytes"""
    while True:
        v, b = rng.randrange(p), rng.randrange(1 << (8 * exp_len))
        if len(R.to_bytes(R.exp(v, b, p))) == nbytes:
            return v, b


@functools.lru_cache(maxsize=None)
def honest_runs():
    rng = random.Random(0x7A5)
    return [R.honest_run(rng, b"correct horse", 5, 3), R.honest_run(rng, b"battery staple", 10, 7)]


@functools.lru_cache(maxsize=None)
def corpus():
    rng = random.Random(0xA07)
    ops = []

    def add(p, nbytes, v, xi, b, exp_len, salt_len, *tags):
        assert len(xi) <= nbytes and v < 1 << (8 * nbytes) and b < 1 << (8 * exp_len)
        ops.append(Op(p, nbytes, v, bytes(xi), b, exp_len, bytes(rng.getrandbits(8) for _ in range(salt_len)), frozenset(tags)))

    def rnd_xi(nbytes):
        return bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, nbytes + 1)))

    # every shape: bases and exponent classes over the moduli that fit it
    for nbytes, exp_len, salt_len in SHAPES:
        mods = moduli_for(nbytes)
        shape = "shape:%d/%d/%d" % (nbytes, exp_len, salt_len)
        i = 0
        for cls in BASE_CLASSES:
            for which in ("v", "xi"):
                name, p = mods[i % len(mods)]
                i += 1
                val = _base(rng, cls, p, nbytes)
                v = val if which == "v" else rng.randrange(p)
                xi = R.to_bytes(val) if which == "xi" else rnd_xi(nbytes)
                add(p, nbytes, v, xi, rng.randrange(1 << (8 * exp_len)), exp_len, salt_len, shape, "mod:" + name, "base:%s:%s" % (which, cls), "exp:random")
        for tag, e in exponent_classes(exp_len, (nbytes, exp_len, salt_len) == (128, 256, 16)):
            name, p = mods[i % len(mods)]
            i += 1
            add(p, nbytes, rng.randrange(2, p), R.to_bytes(rng.randrange(2, p)), e, exp_len, salt_len, shape, "mod:" + name, "exp:" + tag)

    # honest protocol runs under the reference's p: the server's and the client's operations of every answering server
    for run in honest_runs():
        who = "honest:%d/%d" % (run["n"], run["k"])
        for s in run["servers"]:
            ops.append(Op(R.P, 256, int.from_bytes(run["X"], "big"), run["X"], s["y"], 256, s["salt"], frozenset((who, "honest:yi"))))
            ops.append(Op(R.P, 256, s["v"], s["xi"], s["b"], 256, s["salt"], frozenset((who, "honest:bi"))))
            ops.append(Op(R.P, 256, s["bi"], s["xi"], s["e"], 256, s["salt"], frozenset((who, "honest:ni"))))

    # HKDF's secret Ki = Xi^b mod p at its length classes (shape 256/256/32)
    for tag, xi, b in (("0", b"", 3), ("0z", b"\0\0\0", 1), ("1", b"\x01", 12345), ("55", b"\x02", 439), ("56", b"\x02", 447),
                       ("255", R.to_bytes(0x1234567), 255)):
        add(R.P, 256, rng.randrange(R.P), xi, b, 256, 32, "ki:" + tag)
    v, b = _full_width_power(rng, R.P, 256, 256)
    add(R.P, 256, rng.randrange(R.P), R.to_bytes(v), b, 256, 32, "ki:256")

    # the MAC's input Xi | Bi.Bytes(): every xi_len against a 256-byte Bi, then the short Bi
    for xl in XI_LENS:
        v, b = _full_width_power(rng, R.P, 256, 2)            # (a short exponent in a 256-byte row: the restatement's pow is cheap)
        add(R.P, 256, v, bytes(rng.getrandbits(8) for _ in range(xl)), b, 256, 32, "mac:xi%d+bi256" % xl)
    bi255 = rng.randrange(1 << 2032, 1 << 2040)
    for tag, v, xls in (("bi255", bi255, (1, 56, 57)), ("bi0", 0, (0, 55, 64)), ("bi1", 1, (0, 55, 62, 63))):
        for xl in xls:
            add(R.P, 256, v, bytes(rng.getrandbits(8) | 1 for _ in range(xl)), 1, 256, 32, "mac:%s" % tag, "mac:xi%d+%s" % (xl, tag))

    # raw Xi: the same number with and without leading zero bytes (same powers, another MAC), and a number of p or more
    x = rng.randrange(1 << 1000, 1 << 2000)
    b = rng.randrange(R.P)
    v = rng.randrange(R.P)
    ops.append(Op(R.P, 256, v, R.to_bytes(x), b, 256, b"s" * 32, frozenset(("rawxi:plain",))))
    ops.append(Op(R.P, 256, v, b"\0\0" + R.to_bytes(x), b, 256, b"s" * 32, frozenset(("rawxi:zeros",))))
    add(R.P, 256, v, (R.P + 5).to_bytes(256, "big"), b, 256, 32, "rawxi:ge_p")
    # Bi of p or more as the client parses it: the power reduces it, the MAC takes its bytes as given
    add(R.P, 256, R.P + 7, rnd_xi(256), rng.randrange(R.Q), 256, 32, "ni:bi_ge_p")
    return tuple(ops)


def by_shape():
    """(nbytes, exp_len, salt_len) -> [index into corpus()]"""
    out = {}
    for i, op in enumerate(corpus()):
        out.setdefault((op.nbytes, op.exp_len, len(op.salt)), []).append(i)
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """Per op of corpus(): (yi, (Bi, keys, mac), (keys, Ni)) by the restatement, computed once."""
    out = []
    for op in corpus():
        vb = R.exp(op.v, op.b, op.p)            # makeYi's power, makeBi's Bi and processBi's Ki are the same number: raise it once
        ki = R.exp(int.from_bytes(op.xi, "big"), op.b, op.p)
        out.append((vb, (vb,) + R.finish(ki, vb, op.xi, op.salt), R.finish(vb, op.v, op.xi, op.salt)))
    return tuple(out)
