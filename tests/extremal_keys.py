"""RSA keys over the prime moduli of tests/golden/extremal_moduli.json (every radix-2^28 limb full, or almost every limb zero)
and DSA keys over its groups, shaped for tests/rsa_sizes.py (`cell_cases`, `entity`) and the corpus signer.

A prime modulus has a signer without factoring: d = e^-1 mod (n - 1).  Valid signatures therefore exist under these moduli,
and a verdict of "valid" can only come from an exact s^e mod n.  Neither the library nor the reference tests a modulus for being
a product of two primes.  corpus.build.KeyPair.rsa_private assumes two primes, so the RSA keys here are objects of their own."""
import functools
import hashlib
import json
import os
import struct

from corpus import build as cb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# every modulus under 65537, and the two small exponents in each size class at one end or the other
SMALL_EXPONENTS = [("full2048", 3), ("sparse2048", 17), ("sparse3072", 3), ("full3072", 17), ("full4096", 3), ("sparse4096", 17)]


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(GOLDEN, "extremal_moduli.json")) as f:
        return json.load(f)


class PrimeModulusKey:
    """What RS.cell_cases and RS.entity read of a key pair: n, e, key_id, pub_body, name, rsa_private."""
    algo = cb.PK_RSA

    def __init__(self, n, e, name):
        self.n, self.e, self.name = n, e, name
        self.d = pow(e, -1, n - 1)
        self.pub_body = bytes([4]) + struct.pack(">I", cb.CREATION_TIME) + bytes([cb.PK_RSA]) + cb._mpi(n) + cb._mpi(e)
        fp = hashlib.sha1(b"\x99" + struct.pack(">H", len(self.pub_body)) + self.pub_body).digest()
        self.key_id = int.from_bytes(fp[12:], "big")

    def rsa_private(self, m):
        return pow(m, self.d, self.n)


@functools.lru_cache(maxsize=None)
def rsa_keys():
    mods = {e["name"]: int(e["n"], 16) for e in fixture()["rsa"]}
    out = [PrimeModulusKey(n, 65537, "%s <k@bftkv.example>" % name) for name, n in mods.items()]
    out += [PrimeModulusKey(mods[name], e, "%se%d <k@bftkv.example>" % (name, e)) for name, e in SMALL_EXPONENTS]
    assert len({kp.key_id for kp in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def dsa_keys():
    """{name: corpus KeyPair} over the extremal groups."""
    return {g["name"]: cb.make_keypair(cb.PK_DSA, {f: int(g[f], 16) for f in ("p", "q", "g", "x")}, "%s <k@bftkv.example>" % g["name"])
            for g in fixture()["dsa"]}


@functools.lru_cache(maxsize=None)
def rsa_cases():
    """Every extremal key under the five hashes, each cell in the value shapes of RS.cell_cases (one tampered encoding per cell,
    a different one from cell to cell)."""
    from tests import rsa_sizes as RS
    out = []
    for ki, kp in enumerate(rsa_keys()):
        for hi, (hash_id, _) in enumerate(RS.HASHES):
            cell = ki * len(RS.HASHES) + hi
            out += RS.cell_cases(ki, kp, hash_id, b"extremal keys: key %d, hash %d " % (ki, hash_id) + bytes(range(cell % 61)), cell)
    return out
