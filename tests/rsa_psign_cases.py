"""The cases of threshold RSA signing (rsaContext.Sign): seeded, not collected.  calls() is the corpus -- every Call is ONE device call
of one (nbytes, exp_len) -- and tree() the n = 4, k = 2 key tree over the known-answer key of tests/golden/threshold_kat.json.
The expected answers come from tests/rsa_psign_ref.py, computed once."""
import collections
import functools
import hashlib
import json
import math
import os
import random

import rsa_psign_ref as R
import rsa_verify_ref as V

HERE = os.path.dirname(os.path.abspath(__file__))

Frag = collections.namedtuple("Frag", "sign mag used cls")       # the stored sign byte, the magnitude, exp_used, the magnitude's class
Req = collections.namedtuple("Req", "n t frags tags")            # modulus, T as received, [Frag], what the request is there for
Call = collections.namedtuple("Call", "name nbytes exp_len reqs")

SIGN_BYTES = (0, 1, 2, 0xFF)
MAG_CLASSES = ("zero", "one", "all15", "low_digit", "top_digit", "zero_run", "random", "random_short")
EXP_LENS = (1, 2, 3, 5, 512, 513)
BIG_EXP_LEN = 4097


@functools.lru_cache(maxsize=None)
def kat():
    k = json.load(open(os.path.join(HERE, "golden", "threshold_kat.json")))["rsa"]
    return dict(n=int(k["n"], 16), e=int(k["e"]), d=int(k["d"], 16), tbs=k["tbs"].encode(), sig=int(k["sha256_pkcs1v15_sig"], 16))


def digest_infos():
    """the seven DigestInfo shapes: hash id -> prefix | digest of the fixture's tbs (any bytes of the hash's length would do)"""
    tbs = kat()["tbs"]
    dg = {1: hashlib.md5(tbs).digest(), 2: hashlib.sha1(tbs).digest(), 3: hashlib.sha1(b"r" + tbs).digest(), 8: hashlib.sha256(tbs).digest(),
          9: hashlib.sha384(tbs).digest(), 10: hashlib.sha512(tbs).digest(), 11: hashlib.sha224(tbs).digest()}
    return {h: V.PREFIX[h] + dg[h] for h in sorted(dg)}


def t_classes(nbytes):
    """(tag, T) of every class a request's T comes in, for rows of nbytes"""
    rng = random.Random(0x7C00 + nbytes)
    out = [("t:empty", b""), ("t:one", b"\x5a"), ("t:leading_zeroes", b"\0\0\0" + bytes(rng.getrandbits(8) for _ in range(29))), ("t:all_ff", b"\xff" * 40)]
    out += [("t:digestinfo:%d" % h, t) for h, t in digest_infos().items()]
    out.append(("t:nbytes", bytes(rng.getrandbits(8) for _ in range(nbytes))))
    return out


def _odd(rng, bits):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def _modulus(rng, bits, ts):
    """an odd modulus of `bits` bits under which every T of ts that is not refused encodes to a unit: the no-inverse row is a class of
    its own (no_inverse_moduli), not an accident of the draw"""
    while True:
        n = _odd(rng, bits)
        if all(m is None or math.gcd(m, n) == 1 for m in (R.emsa_encode(t, n) for t in ts)):
            return n


@functools.lru_cache(maxsize=None)
def moduli():
    """name -> (modulus, bits).  Tiny moduli sit at emlen 3, 53, 54, 55: one byte either side of the SHA-256 DigestInfo's 51 + 3."""
    rng = random.Random(0x9516)
    ts = [t for _, t in t_classes(256)] + [t for _, t in t_classes(128)]
    m = {"kat2048": kat()["n"]}
    for bits in (2041, 2040, 1024, 1023, 520):
        m["odd%d" % bits] = _modulus(rng, bits, ts)
    for el in (3, 53, 54, 55):
        m["tiny_emlen%d" % el] = _modulus(rng, 8 * el - 3, ts)
    m["one"], m["three"] = 1, 3
    assert all(math.gcd(x, m["kat2048"]) == 1 for x in (R.emsa_encode(t, m["kat2048"]) for t in ts) if x is not None)
    return m


@functools.lru_cache(maxsize=None)
def no_inverse_case():
    """(N = 3 P, T with 3 | em, T with gcd(em, N) = 1): the two T differ in their last byte alone"""
    rng = random.Random(0x3333)
    while True:
        n = 3 * _odd(rng, 2040)
        head = bytes(rng.getrandbits(8) for _ in range(50))
        bad = [head + bytes([b]) for b in range(256) if R.emsa_encode(head + bytes([b]), n) % 3 == 0]
        good = [head + bytes([b]) for b in range(256) if math.gcd(R.emsa_encode(head + bytes([b]), n), n) == 1]
        if bad and good and n.bit_length() <= 2048:
            return n, bad[0], good[0]


def magnitude(rng, cls, used):
    """a magnitude of class cls that fits `used` bytes (used >= 1)"""
    digits = 2 * used
    if cls == "zero":
        return 0
    if cls == "one":
        return 1
    if cls == "all15":
        return (1 << (8 * used)) - 1
    if cls == "low_digit":
        return rng.randrange(1, 16)
    if cls == "top_digit":
        return rng.randrange(1, 16) << (4 * (digits - 1))
    if cls == "zero_run":                               # random, with the middle third of its digits zero
        lo, hi = digits // 3, max(digits // 3 + 1, 2 * digits // 3)
        v = rng.getrandbits(8 * used) | (1 << (8 * used - 1)) | 1
        return v & ~(((1 << (4 * (hi - lo))) - 1) << (4 * lo))
    if cls == "random_short":                           # shorter than the row it travels in: leading zero digits inside exp_used
        return rng.getrandbits(max(1, 8 * used - 12)) | 1
    return rng.getrandbits(8 * used) | (1 << (8 * used - 1))


def _true_len(mag):
    return (mag.bit_length() + 7) // 8


def _frags(rng, exp_len, count, start=0):
    """`count` fragments that walk MAG_CLASSES x SIGN_BYTES from `start`; exp_used: the row's width, the magnitude's own length (0 for
    a zero), or something between"""
    out = []
    for j in range(start, start + count):
        cls, sb = MAG_CLASSES[j % len(MAG_CLASSES)], SIGN_BYTES[(j // len(MAG_CLASSES) + j) % len(SIGN_BYTES)]
        width = (exp_len, max(1, exp_len - 1), max(1, exp_len // 2))[j % 3]
        mag = magnitude(rng, cls, width)
        used = (exp_len, _true_len(mag), width)[(j // 3) % 3]
        out.append(Frag(sb, mag, max(used, _true_len(mag)), cls))
    return out


def _all_frags(rng, exp_len):
    """every magnitude class under every sign byte"""
    out = []
    for i, cls in enumerate(MAG_CLASSES):
        for j, sb in enumerate(SIGN_BYTES):
            mag = magnitude(rng, cls, exp_len)
            out.append(Frag(sb, mag, (exp_len, _true_len(mag))[(i + j) % 2], cls))
    return out


@functools.lru_cache(maxsize=None)
def calls():
    rng = random.Random(0x51C4)
    m = moduli()
    out = []
    for exp_len in EXP_LENS:
        for nbytes in (256, 128):
            reqs = []
            names = [k for k, v in m.items() if R.emlen(v) <= nbytes]
            ts = t_classes(nbytes)
            step = 0
            for name in names:
                # the long exponents cost the restatement 10 ms a fragment under a 2048-bit modulus: every T under the fixture's key and
                # under the tiny moduli, where a byte of T decides the row; four T elsewhere
                every_t = name == "kat2048" or name.startswith("tiny") or exp_len <= 5 or name in ("one", "three")
                for i, (tag, t) in enumerate(ts):
                    if not every_t and (i + step) % 3:
                        continue
                    nf = 1 + (step % 3) if exp_len > 5 and m[name].bit_length() > 600 else 2 + step % 4
                    reqs.append(Req(m[name], t, tuple(_frags(rng, exp_len, nf, start=5 * step)), frozenset({"mod:" + name, tag})))
                    step += 1
            # every magnitude class under every sign byte: the fixture's key (256-byte rows) or the 1023-bit modulus (128)
            full_n = m["kat2048"] if nbytes == 256 else m["odd1023"]
            reqs.append(Req(full_n, digest_infos()[8], tuple(_all_frags(rng, exp_len)), frozenset({"frags:all", "t:digestinfo:8"})))
            if nbytes == 256:
                n3, t_bad, t_good = no_inverse_case()
                fr = (Frag(1, magnitude(rng, "random", exp_len), exp_len, "random"), Frag(0, magnitude(rng, "random", exp_len), exp_len, "random"),
                      Frag(0xFF, 0, exp_len, "zero"), Frag(2, 1, exp_len, "one"), Frag(0, 1, 1, "one"))
                reqs.append(Req(n3, t_bad, fr, frozenset({"noinv:bad"})))
                reqs.append(Req(n3, t_good, fr, frozenset({"noinv:good"})))
            out.append(Call("e%d_n%d" % (exp_len, nbytes), nbytes, exp_len, tuple(reqs)))
    big = tuple(Frag(SIGN_BYTES[j % 4], magnitude(rng, cls, BIG_EXP_LEN - (j % 3)), BIG_EXP_LEN - (j % 3), cls)
                for j, cls in enumerate(("random", "all15", "top_digit", "zero_run", "random", "low_digit", "random_short", "random")))
    out.append(Call("e4097_n256", 256, BIG_EXP_LEN, (Req(m["kat2048"], digest_infos()[8], big, frozenset({"frags:big"})),)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(call_index):
    """[(status, ci)] per fragment of calls()[call_index], request after request"""
    out = []
    for r in calls()[call_index].reqs:
        out += R.sign(r.t, r.n, [(f.sign, f.mag) for f in r.frags])
    return tuple(out)


def call_arrays(call, order=None):
    """The arrays of bftkv_gpu_rsa_partial_sign for a Call (numpy): requests in the call's order, fragments in `order` (default: request
    after request).  What follows T in its row is NOT zero, and every request names its modulus by index into the sorted table."""
    import numpy as np
    mods = sorted({r.n for r in call.reqs})
    t_cap = max(len(r.t) for r in call.reqs)
    t = np.full((len(call.reqs), max(t_cap, 1)), 0xEE, dtype=np.uint8)
    for i, r in enumerate(call.reqs):
        t[i, :len(r.t)] = np.frombuffer(r.t, dtype=np.uint8)
    flat = [(i, f) for i, r in enumerate(call.reqs) for f in r.frags]
    order = list(range(len(flat))) if order is None else list(order)
    be = lambda v, w: np.frombuffer(int(v).to_bytes(w, "big"), dtype=np.uint8)      # noqa: E731
    return dict(t=t[:, :t_cap] if t_cap else t[:, :0], t_len=np.array([len(r.t) for r in call.reqs], dtype=np.uint32),
                mods=np.stack([be(n, call.nbytes) for n in mods]), mod_idx=np.array([mods.index(r.n) for r in call.reqs], dtype=np.uint32),
                frag_req=np.array([flat[j][0] for j in order], dtype=np.uint32), exps=np.stack([be(flat[j][1].mag, call.exp_len) for j in order]),
                exp_used=np.array([flat[j][1].used for j in order], dtype=np.uint32), sign=np.array([flat[j][1].sign for j in order], dtype=np.uint8))


# ---- the n = 4, k = 2 tree over the known-answer key -------------------------------------------------------------------------------------
TREE_N, TREE_K = 4, 2
LIVE_SETS = ((0, 1), (2, 3), (0, 1, 2, 3))


@functools.lru_cache(maxsize=None)
def tree():
    """[{kid: di}] per server"""
    return tuple(R.distribute(kat()["d"], TREE_N, TREE_K, random.Random(0x7EE)))


def tree_t():
    """T of the fixture's signature: the SHA-256 DigestInfo of its tbs"""
    return V.PREFIX[8] + hashlib.sha256(kat()["tbs"]).digest()


def tree_fragments():
    """[(server, kid, sign byte, magnitude bytes)]: every fragment every server holds, as serializePartialParam stores it"""
    return [(srv, kid) + R.stored(di) for srv, keys in enumerate(tree()) for kid, di in sorted(keys.items())]
