"""The seeded corpus of the OpenPGP DSA pipeline tests (k_dsa_inv, k_dsa_inv_batched, k_dsa_mul, k_dsa_build_comb, k_dsa_split,
k_dsa_modexp in csrc/kernels.hip), CPU and GPU.  Not collected.

Family A, chosen window digits.  A valid OpenPGP DSA signature whose u2 = r / s, or whose u1 = z / s, is a number we pick exists
under a key made for it: take the group, the payload and the signature prefix, hence z; pick k, r = (g^k mod p) mod q; for the
target t set w = t / r (u2 = t) or w = t / z (u1 = t), s = 1 / w, u1 = z w, u2 = r w; x = (k - u1) / u2 and y = g^x.  Then
g^u1 y^u2 = g^k.  z must not depend on the key, so the issuer subpacket (a hash of y) sits in the unhashed area and the hashed
area holds the creation time alone; the oracle and the device take the issuer from either area (docs/parity.md).

    digits(wbits, q)     the targets of one table width, as (label, value)
    ring(wbits, mixed)   Ring(keys, cases): one keyring and its cases -- every target as u2 and as u1, each under a key of its own,
                         each valid, each with a twin (the same r and s over the payload plus one byte, the two hash-tag bytes
                         re-written for that payload so that the twin is refused by the arithmetic and not by the tag)
    sparse_wave()        Ring for width 13: 16 signatures whose u2 has one and the same single non-zero window, and one u2 = q - 1

Widths 4 and 8 .. 18.  19 and 20 bits stay out: their tables take 4.5 and 8.3 GB per key.  The tables of a ring stay under
RING_CAP bytes by construction (targets are taken in the order listed until the next pair of keys would cross it).

Family B, keys an attacker would choose: hostile_ring().  Every case carries rule "oracle" (the device answers what the oracle
answers) or "unsupported" (the key is one the key table turns away, unsupported_key(): status ST_UNSUPPORTED, fenced, refused).

Family C, runs for the batched inversion: inversion_runs().  Composite orders, one signature in eight under them with an s in
(0, q) that has no inverse, so that most 16-entry runs of k_dsa_inv_batched multiply up a product without an inverse."""
import functools
import hashlib
import json
import math
import os
import struct
from collections import namedtuple

from corpus import build as cb
from corpus.keys import DRBG
from oracle import openpgp as pgp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTHS = (4, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18)
HASHES = (2, 8, 10)                      # SHA-1, SHA-256, SHA-512: z shorter than a 256-bit q, as wide, cut to it
RING_CAP = 16 * 10 ** 9                  # bytes of table a ring may need
SMALL_2048 = ("dsa2048", "dsa2048_low", "p2048_q256_low")     # the 2048-bit groups of family A

Group = namedtuple("Group", "name p q g x")
# kind: "valid" | "twin" for family A; "honest" | "twin" | "ends" for B; "honest" | "flipped" | "no inverse" | "range" for C.
# key: index into the ring's keys.  which, target: family A's exponent ("u1" | "u2") and its value.  rule: "oracle" | "unsupported".
Case = namedtuple("Case", "label kind key payload sig hash_id which target rule", defaults=(None, None, "oracle"))
Ring = namedtuple("Ring", "keys cases")


class Key:
    """A DSA public key as the corpus key pairs carry it, with y and g free (y = 0, g >= p ...): p, q, g, y, key_id, pub_body, name."""
    algo = cb.PK_DSA

    def __init__(self, p, q, g, y, name, x=None):
        self.p, self.q, self.g, self.y, self.x, self.name = p, q, g, y, x, name
        self.pub_body = bytes([4]) + struct.pack(">I", cb.CREATION_TIME) + bytes([cb.PK_DSA]) + cb._mpi(p) + cb._mpi(q) + cb._mpi(g) + cb._mpi(y)
        fp = hashlib.sha1(b"\x99" + struct.pack(">H", len(self.pub_body)) + self.pub_body).digest()
        self.key_id = int.from_bytes(fp[12:], "big")


def entity(kp):
    return pgp.Entity(primary=pgp.PublicKey(key_id=kp.key_id, pk_algo=cb.PK_DSA, p=kp.p, q=kp.q, g=kp.g, y=kp.y), name=kp.name)


@functools.lru_cache(maxsize=None)
def groups():
    """{name: Group}: the first key's group of keys_dsa{1024,2048,3072}.json, the groups of extremal_moduli.json, of
    dsa_verify_groups.json and of dsa_pipeline_groups.json."""
    def load(name):
        with open(os.path.join(GOLDEN, name)) as f:
            return json.load(f)
    raw = [(n, load("keys_%s.json" % n)["keys"][0]) for n in ("dsa1024", "dsa2048", "dsa3072")]
    raw += [(g["name"], g) for g in load("extremal_moduli.json")["dsa"]]
    raw += [(g["name"], g) for g in load("dsa_verify_groups.json")["groups"]]
    raw += [(g["name"], g) for g in load("dsa_pipeline_groups.json")["groups"]]
    out = {}
    for name, g in raw:
        assert name not in out
        out[name] = Group(name, *(int(g[f], 16) for f in ("p", "q", "g", "x")))
    return out


# ---- packets

def prefix_of(hash_id):
    """A v4 binary-document DSA signature's hashed part: the creation time and nothing that names the key."""
    return cb.sig_prefix(0x00, cb.PK_DSA, b"\x05\x02" + struct.pack(">I", cb.CREATION_TIME), hash_id)


def digest_of(payload, hash_id):
    return hashlib.new(cb.HASH_NAMES[hash_id], payload + cb.hash_suffix(prefix_of(hash_id))).digest()


def z_of(digest, q):
    """The digest as dsa.Verify reads it: its leftmost bytes(q) bytes."""
    return int.from_bytes(digest[:(q.bit_length() + 7) // 8], "big")


def packet(key_id, payload, hash_id, r, s):
    """The signature packet: hashed area as prefix_of, the issuer in the unhashed area, the hash tag of `payload`."""
    unhashed = b"\x09\x10" + struct.pack(">Q", key_id)
    enc = b"".join(cb.go_mpi_bytes(v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")) for v in (r, s))
    body = prefix_of(hash_id) + struct.pack(">H", len(unhashed)) + unhashed + digest_of(payload, hash_id)[:2] + enc
    return cb._hdr(2, len(body)) + body


def read_packet(sig):
    """(hash_id, r, s) of a packet made by packet()."""
    g = pgp.packet_read_stream(sig, 0).sig
    return g.hash_id, int.from_bytes(g.mpis[0][1], "big"), int.from_bytes(g.mpis[1][1], "big")


def exponents(kp, payload, sig):
    """(u1, u2, z) as dsa.Verify computes them for this packet under this key (s invertible)."""
    hash_id, r, s = read_packet(sig)
    z = z_of(digest_of(payload, hash_id), kp.q)
    w = pow(s, -1, kp.q)
    return z * w % kp.q, r * w % kp.q, z


# ---- family A

def digit(u, w, j):
    return (u >> (w * j)) & ((1 << w) - 1)


def straddling_window(w):
    """The lowest window whose bits lie in two 32-bit words; 1 where no window does (4, 8 and 16 bits)."""
    return next((j for j in range(256 // w) if (w * j) % 32 + w > 32), 1)


def digits(wbits, q):
    w, full = wbits, (1 << wbits) - 1
    top = 1 << (w * ((q.bit_length() - 1) // w))
    while top >= q:
        top >>= 1
    nwin = (q.bit_length() + w - 1) // w
    comb = sum(full << (w * j) for j in range(0, nwin, 2))
    j = nwin
    while comb >= q:
        j -= 1
        comb &= (1 << (w * j)) - 1
    out = [("1", 1), ("window 0 full", full), ("straddling window full", full << (w * straddling_window(w))), ("top window alone", top),
           ("even windows full", comb), ("q - 1", q - 1)]
    assert all(0 < t < q for _, t in out)
    return out


def craft(G, target, which, payload, hash_id, rng, name):
    """(Key, r, s): a key and a signature of `payload` under it whose u2 (which == "u2") or u1 is `target`."""
    p, q, g = G.p, G.q, G.g
    z = z_of(digest_of(payload, hash_id), q)
    assert 0 < target < q
    while True:
        k = 1 + rng.below(q - 1)
        r = pow(g, k, p) % q
        den = r if which == "u2" else z % q
        if r == 0 or math.gcd(den, q) != 1:
            assert which == "u2" or den, "z = 0 mod q: another payload"
            continue
        w = target * pow(den, -1, q) % q
        if w == 0 or math.gcd(w, q) != 1:
            continue
        s, u1, u2 = pow(w, -1, q), z * w % q, r * w % q
        if u2 == 0 or math.gcd(u2, q) != 1:
            continue
        x = (k - u1) * pow(u2, -1, q) % q
        if x < 2:
            continue
        return Key(p, q, g, pow(g, x, p), name, x=x), r, s


def twin_of(kp, payload, hash_id, r, s):
    return payload + b"\x00", packet(kp.key_id, payload + b"\x00", hash_id, r, s)


@functools.lru_cache(maxsize=None)
def chosen(wbits, gname):
    """((Key, valid Case, twin Case), ...) of one width under one group, targets in the order of digits(), u2 before u1.  The
    cases' key index is their position here."""
    G = groups()[gname]
    rng = DRBG("dsa pipeline chosen digits", wbits, gname)
    out = []
    for ti, (label, t) in enumerate(digits(wbits, G.q)):
        for which in ("u2", "u1"):
            i = len(out)
            hash_id = HASHES[(i + wbits) % 3]
            payload = b"chosen digits: %d bits, %s, %s = %s " % (wbits, gname.encode(), which.encode(), label.encode()) + rng.bytes(i % 7)
            if gname == "p2048_q256_low" and hash_id != 2:
                # q just above 2^255: a digest of 256 bits or more lies on either side of it.  The side is chosen, not met
                above = (ti + wbits + (hash_id == 8)) % 2 == 0
                while (z_of(digest_of(payload, hash_id), G.q) >= G.q) != above:
                    payload += rng.bytes(1)
            kp, r, s = craft(G, t, which, payload, hash_id, rng, "%s w%d %s=%s <k@bftkv.example>" % (gname, wbits, which, label))
            tag = "%s %s = %s" % (gname, which, label)
            tp, ts = twin_of(kp, payload, hash_id, r, s)
            out.append((kp, Case(tag, "valid", i, payload, packet(kp.key_id, payload, hash_id, r, s), hash_id, which, t),
                        Case(tag + " (twin)", "twin", i, tp, ts, hash_id, which, t)))
    return tuple(out)


def slot_bytes(wbits, entry_limbs):
    """dsa_slot_stride(wbits, E) * 4 of csrc/device_types.h: the table bytes of one key."""
    nwin = (256 + wbits - 1) // wbits
    return (2 * nwin * ((1 << wbits) - 1) * entry_limbs + entry_limbs * 10 + 12) * 4


def ring_bytes(keys, wbits):
    E = 112 if any(kp.p.bit_length() > 2048 for kp in keys) else 76
    return len(keys) * slot_bytes(wbits, E)


def _assemble(triples):
    keys, cases = [], []
    for kp, valid, twin in triples:
        cases += [valid._replace(key=len(keys)), twin._replace(key=len(keys))]
        keys.append(kp)
    assert len({kp.key_id for kp in keys}) == len(keys)
    return Ring(tuple(keys), tuple(cases))


@functools.lru_cache(maxsize=None)
def ring(wbits, mixed=False):
    """The twelve (target, exponent) pairs of a width under 2048-bit keys, the three 2048-bit groups taking turns; `mixed` adds
    the pairs under the 1024/160 and the 3072/256 group (widths up to 13), or is four 2048-bit and two 3072-bit keys (above 13)."""
    n_t = len(digits(wbits, groups()["dsa2048"].q))
    small = [chosen(wbits, SMALL_2048[(ti + wbits) % 3])[2 * ti + k] for ti in range(n_t) for k in (0, 1)]
    if mixed and wbits > 13:
        pick = small[:4] + list(chosen(wbits, "dsa3072")[2:4])       # 1 and a full window 0, as u2 and as u1; 3072 bits: window 0
    elif mixed:
        pick = small + list(chosen(wbits, "dsa1024")) + list(chosen(wbits, "dsa3072"))
    else:
        pick = small
    E = 112 if mixed else 76
    n = len(pick)
    if not mixed:
        while n > 2 and n * slot_bytes(wbits, E) >= RING_CAP:       # targets in the order listed, a pair of keys each
            n -= 2
    out = _assemble(pick[:n])
    assert ring_bytes(out.keys, wbits) < RING_CAP
    return out


@functools.lru_cache(maxsize=None)
def sparse_wave():
    """Width 13, the gpg-shaped 2048-bit group: keys 0 .. 15 with u2 = d << (13 * 7) for sixteen digits d (window 7 straddles
    bits 91 .. 103, two words), key 16 with u2 = q - 1.  Cases: a valid one and a twin per key."""
    G = groups()["dsa2048"]
    rng = DRBG("dsa pipeline sparse wave")
    ds = [1, 2, 8191, 4096, 4095, 0x1555, 0x0AAA, 31] + [1 + rng.below(8191) for _ in range(8)]
    triples = []
    for i, t in enumerate([d << (13 * 7) for d in ds] + [G.q - 1]):
        hash_id = HASHES[i % 3]
        payload = b"sparse wave %d" % i
        kp, r, s = craft(G, t, "u2", payload, hash_id, rng, "sparse %d <k@bftkv.example>" % i)
        tp, ts = twin_of(kp, payload, hash_id, r, s)
        triples.append((kp, Case("sparse %d" % i, "valid", i, payload, packet(kp.key_id, payload, hash_id, r, s), hash_id, "u2", t),
                        Case("sparse %d (twin)" % i, "twin", i, tp, ts, hash_id, "u2", t)))
    return _assemble(triples)


# ---- family B

VERIFY_GROUPS = ("p512_q160", "p1016_q160", "p1023_q224", "p1025_q256", "p2041_q160", "p2047_q224", "p768_q64", "composite_q160", "q161",
                 "p512_q8", "p_is_1")
PIPELINE_GROUPS = ("p1024_q32", "p1024_q40", "p1024_q248", "p512_q24", "p1024_q264", "composite_q256", "p_is_3", "even_q", "even_p",
                   "p2048_q256_low")
VARIANT_GROUPS = ("p1016_q160", "p2048_q256_low")
# groups under which an honest signature exists and verifies: a g of order q, q of whole bytes within what the key table admits
HONEST_GROUPS = ("p512_q160", "p1016_q160", "p1023_q224", "p1025_q256", "p2041_q160", "p2047_q224", "p768_q64", "composite_q160",
                 "p1024_q32", "p1024_q40", "p1024_q248", "composite_q256", "p2048_q256_low")


def unsupported_key(kp):
    """The keys the pipeline's key table turns away (make_key_entry in csrc/capi.hip)."""
    pb, qb = kp.p.bit_length(), kp.q.bit_length()
    cap = 2048 if pb <= 2048 else 3072
    return (pb < 2 or pb > 3072 or qb < 32 or qb > 256 or kp.q % 2 == 0 or kp.p % 2 == 0 or
            kp.g.bit_length() > cap or kp.y.bit_length() > cap)


def sign(p, q, g, x, z, rng, want=lambda r, s: True, tries=32):
    """An honest (r, s) over z, or None where the numbers allow none that `want` takes."""
    if any(q % f == 0 and x % f == 0 and z % f == 0 for f in (3, 5)):
        return None                    # s = (z + x r) / k is a multiple of that factor of q whatever k is
    for _ in range(tries):
        k = 1 + rng.below(q - 1)
        if math.gcd(k, q) != 1:
            continue
        r = pow(g, k, p) % q
        s = pow(k, -1, q) * (z + x * r) % q
        if r and s and math.gcd(s, q) == 1 and want(r, s):
            return r, s
    return None


def _refused_with_its_ends(kp, z, r, s):
    """Under p = 3 there is no group of order q, and v = r still happens every other time, by parity.  The cases under that key
    are the draws that dsa.Verify refuses, together with their twin and their r and s moved to 1 and q - 1.  z: (its own, the twin's)."""
    dg, dg_twin = (v.to_bytes((kp.q.bit_length() + 7) // 8, "big") for v in z)
    return not (pgp.dsa_verify(kp.p, kp.q, kp.g, kp.y, dg_twin, r, s) or
                any(pgp.dsa_verify(kp.p, kp.q, kp.g, kp.y, dg, rr, ss) for rr, ss in ((r, s), (1, s), (kp.q - 1, s), (r, 1), (r, kp.q - 1))))


def _hostile_cases(ki, kp, G, g_sign, rng, tag, n_honest=3):
    """Honest signatures by (G.x, g_sign) presented under key kp, a tampered twin each, and r and s at 1 and q - 1."""
    out = []
    rule = "unsupported" if unsupported_key(kp) else "oracle"
    last = None
    for j in range(n_honest):
        hash_id = HASHES[(ki + j) % 3]
        for attempt in range(8):       # (a composite q whose factor divides x and z leaves no invertible s: another payload)
            payload = b"hostile keys: %s #%d.%d " % (tag.encode(), j, attempt) + rng.bytes((ki + j) % 5)
            z = z_of(digest_of(payload, hash_id), G.q)
            if G.name == "p_is_3":
                z_twin = z_of(digest_of(payload + b"\x00", hash_id), G.q)
                rs = sign(G.p, G.q, g_sign, G.x, z, rng, want=lambda r, s: _refused_with_its_ends(kp, (z, z_twin), r, s), tries=4000)
            else:
                rs = sign(G.p, G.q, g_sign, G.x, z, rng)
            if rs:
                break
        rs = rs or (1 + rng.below(G.q - 1), 1 + rng.below(G.q - 1))
        last = (payload, hash_id) + rs
        out.append(Case("%s honest #%d" % (tag, j), "honest", ki, payload, packet(kp.key_id, payload, hash_id, *rs), hash_id, rule=rule))
        tp, ts = twin_of(kp, payload, hash_id, *rs)
        out.append(Case("%s twin #%d" % (tag, j), "twin", ki, tp, ts, hash_id, rule=rule))
    payload, hash_id, r, s = last
    for label, rr, ss in (("r = 1", 1, s), ("r = q - 1", G.q - 1, s), ("s = 1", r, 1), ("s = q - 1", r, G.q - 1)):
        out.append(Case("%s %s" % (tag, label), "ends", ki, payload, packet(kp.key_id, payload, hash_id, rr, ss), hash_id, rule=rule))
    return out


@functools.lru_cache(maxsize=None)
def hostile_ring():
    rng = DRBG("dsa pipeline hostile keys")
    gs = groups()
    keys, cases = [], []

    def add(kp, G, g_sign, tag, n_honest=3):
        cases.extend(_hostile_cases(len(keys), kp, G, g_sign, rng, tag, n_honest))
        keys.append(kp)
    for name in VERIFY_GROUPS + PIPELINE_GROUPS:
        G = gs[name]
        add(Key(G.p, G.q, G.g, pow(G.g, G.x, G.p), "%s <k@bftkv.example>" % name), G, G.g, name)
    for name in VARIANT_GROUPS:
        G = gs[name]
        p, y1 = G.p, pow(G.g, G.x, G.p)
        cap = 2048 if p.bit_length() <= 2048 else 3072
        m = -((y1 - (1 << cap)) // p)                 # the least multiple of p that lifts y to cap + 1 bits
        assert (y1 + p * m).bit_length() == cap + 1 and (y1 + p * (m - 1)).bit_length() <= cap
        for label, g, y in (("y = 0", G.g, 0), ("y = 1", G.g, 1), ("y = p - 1", G.g, p - 1), ("y + p", G.g, y1 + p), ("g = 0", 0, y1),
                            ("g = 1", 1, y1), ("g + p", G.g + p, y1), ("y over the cap", G.g, y1 + p * m)):
            add(Key(p, G.q, g, y, "%s, %s <k@bftkv.example>" % (name, label)), G, G.g, "%s, %s" % (name, label), n_honest=2)
    assert len({kp.key_id for kp in keys}) == len(keys)
    return Ring(tuple(keys), tuple(cases))


# ---- family C

INVERSION_KEYS = ("composite_q160", "composite_q256", "p1016_q160", "p2048_q256_low")
N_RUN_ITEMS = 16 * 38 + 1


def small_factor(name):
    return 3 if name == "composite_q160" else 15


@functools.lru_cache(maxsize=None)
def inversion_runs():
    """Ring over INVERSION_KEYS with N_RUN_ITEMS one-packet cases; kind is "honest", "flipped" (prime keys: a bit of s), "no inverse"
    (composite keys: s = 3 m, q / 3 or 15 m, in range) or "range" (r = 0, s = 0, r >= q, s >= q)."""
    rng = DRBG("dsa pipeline inversion runs")
    gs = [groups()[n] for n in INVERSION_KEYS]
    keys = [Key(G.p, G.q, G.g, pow(G.g, G.x, G.p), "%s <k@bftkv.example>" % G.name, x=G.x) for G in gs]
    cases = []
    for i in range(N_RUN_ITEMS):
        ki = (0, 1, 0, 1, 2, 1, 0, 3)[i % 8] if i % 5 else rng.below(4)      # three quarters under the composite keys
        G, kp = gs[ki], keys[ki]
        hash_id = HASHES[i % 3]
        rs, attempt = None, 0
        while rs is None:              # (a composite q whose factor divides x and z leaves no invertible s: another payload)
            payload = b"inversion runs %d.%d " % (i, attempt) + rng.bytes(i % 9)
            z = z_of(digest_of(payload, hash_id), G.q)
            rs, attempt = sign(G.p, G.q, G.g, G.x, z, rng), attempt + 1
        r, s = rs
        kind, m = "honest", rng.below(40)
        if m < 4:
            kind = "range"
            r, s = ((0, s), (r, 0), (G.q + rng.below(1 << 20), s), (r, G.q + 5))[m]
        elif ki < 2 and m < 9:
            kind = "no inverse"
            f = small_factor(G.name)
            s = (3 * (1 + rng.below(G.q // 3 - 1)), G.q // 3, f * (1 + rng.below(G.q // f - 1)), 3, 15 if f == 15 else 9)[m - 4]
            assert 0 < s < G.q and math.gcd(s, G.q) != 1
        elif ki >= 2 and m < 9:
            kind = "flipped"
            s ^= 1 << rng.below(G.q.bit_length() - 1)
        cases.append(Case("run item %d, %s, %s" % (i, G.name, kind), kind, ki, payload, packet(kp.key_id, payload, hash_id, r, s), hash_id))
    return Ring(tuple(keys), tuple(cases))


# ---- the oracle's answer

def oracle_statuses(rg):
    """The status pgp.check_detached_signature gives every case of a ring (one packet each: exactly one status)."""
    ents = [entity(kp) for kp in rg.keys]
    out = []
    for c in rg.cases:
        r = pgp.check_detached_signature(ents, c.payload, c.sig, 0)
        assert r.pos == len(c.sig) and r.statuses == [r.status], c.label
        out.append(r.status)
    return out


def expectation(case, status):
    """(status, fenced, accepted) the device owes a case whose oracle status is `status`."""
    if case.rule == "unsupported":
        return pgp.ST_UNSUPPORTED, True, False
    return status, False, status == pgp.ST_OK
