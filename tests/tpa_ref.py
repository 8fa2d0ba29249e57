"""The threshold password authentication of crypto/auth/auth.go restated on Python integers, hashlib and hmac: what the device
entries (bftkv_gpu_tpa_yi / _bi / _ni) are compared with, byte for byte.  crypto/rand is replaced by a seeded random.Random.

Three rules rest on memory, their sources not being at hand: Go's big.Int.Exp returns 1 for an exponent <= 0; x/crypto's
hkdf.New(hash, secret, salt, nil) expands with an empty info; two 16-byte reads from that reader come out of the same T(1)."""
import functools
import hashlib
import hmac
import json
import os

from oracle import threshold as th

HERE = os.path.dirname(os.path.abspath(__file__))
P = int(json.load(open(os.path.join(HERE, "golden", "threshold_kat.json")))["sss"]["pb"], 16)      # auth.go:81-112
Q = (P - 1) // 2


def to_bytes(v: int) -> bytes:
    """big.Int.Bytes(): minimal big-endian, empty for 0."""
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def sha256(*args: bytes) -> bytes:                                  # auth.go:407-413
    h = hashlib.sha256()
    for a in args:
        h.update(a)
    return h.digest()


def PI(password: bytes) -> int:                                     # auth.go:401-405
    t = int.from_bytes(sha256(password), "big")
    return t * t % Q


@functools.lru_cache(maxsize=None)
def exp(base: int, e: int, m: int) -> int:
    """big.Int.Exp(base, e, m) for e >= 0 and m > 0: the base is reduced, an exponent of 0 gives 1 (0 under m = 1).  (Remembered: the
    corpus asks for the powers of its honest runs again, and a 2048-bit pow takes tens of milliseconds.)"""
    return pow(base, e, m)


def hmac_sha256(key: bytes, msg: bytes) -> bytes:
    return hmac.new(key, msg, hashlib.sha256).digest()


def hkdf32(secret: bytes, salt: bytes) -> bytes:
    """The first 32 bytes of HKDF-SHA256(secret, salt, info = nil), written out: PRK = HMAC(salt, secret), T1 = HMAC(PRK, 0x01).
    (An absent salt is hashLen zero bytes, which HMAC pads to the same key block as the empty one.)"""
    return hmac_sha256(hmac_sha256(salt, secret), b"\x01")


def key_sched(ki: bytes, salt: bytes):                              # auth.go:182-194 -> (km, ke)
    t = hkdf32(ki, salt)
    return t[:16], t[16:]


def make_yi(x: bytes, y: int, p: int = P) -> int:                   # auth.go:196-200
    return exp(int.from_bytes(x, "big"), y, p)


def finish(ki: int, bi: int, xi: bytes, salt: bytes):
    """What both sides do with their Ki: keySched(Ki.Bytes(), salt), then calculateMac(km, Xi, Bi.Bytes()) -> (km | ke, mac)."""
    km, ke = key_sched(to_bytes(ki), salt)
    return km + ke, hmac_sha256(km, xi + to_bytes(bi))


def make_bi(v: int, xi: bytes, b: int, salt: bytes, p: int = P):    # auth.go:202-223 -> (Bi, km | ke, mac)
    bi = exp(v, b, p)
    return (bi,) + finish(exp(int.from_bytes(xi, "big"), b, p), bi, xi, salt)


def process_bi(bi: int, xi: bytes, e: int, salt: bytes, p: int = P):    # auth.go:331-347 -> (km | ke, Ni); bi as parsed, not reduced
    return finish(exp(bi, e, p), bi, xi, salt)


def generate_params(rng, cred: bytes, n: int, k: int):
    """GeneratePartialAuthenticationParams (auth.go:117-154) -> (S, [{x, y, v, salt}])."""
    s = rng.randrange(Q)
    coords = th.distribute(s, n, k, Q, [rng.randrange(Q) for _ in range(k - 1)])
    pi = PI(cred)
    salt = bytes(rng.getrandbits(8) for _ in range(16))
    params = []
    for i, (x, y) in enumerate(coords):
        sl = sha256(salt, bytes([i]))
        si = int.from_bytes(sha256(cred, sl), "big") * s % Q
        params.append({"x": x, "y": y, "v": exp(pi, si, P), "salt": sl})
    return s, params


def process_yi(cred: bytes, answers, a2s):
    """processYi once k answers [(x, Yi, salt)] are in (auth.go:304-329, calculateSharedSecret :386-399) -> (gs, [Xi bytes])."""
    xs = [x for x, _, _ in answers]
    gs = 1
    for x, yi, _ in answers:
        gs = gs * exp(yi, th.lagrange(x, xs, Q), P) % P
    xis = []
    for (_, _, salt), a2 in zip(answers, a2s):
        si = int.from_bytes(sha256(cred, salt), "big")
        xis.append(to_bytes(exp(gs, a2 * si % Q, P)))
    return gs, xis


def honest_run(rng, cred: bytes, n: int, k: int):
    """The whole protocol up to the MACs with the first k servers answering.  Returns what each side computed, server by server."""
    s, params = generate_params(rng, cred, n, k)
    a = rng.randrange(Q)
    big_x = to_bytes(exp(PI(cred), a, P))                           # generateX, auth.go:294-302
    servers = params[:k]
    answers = [(sp["x"], make_yi(big_x, sp["y"]), sp["salt"]) for sp in servers]
    a2s = [rng.randrange(Q) for _ in servers]
    gs, xis = process_yi(cred, answers, a2s)
    out = []
    for sp, (_, yi, _), a2, xi in zip(servers, answers, a2s, xis):
        b = rng.randrange(P)
        bi, skeys, mac = make_bi(sp["v"], xi, b, sp["salt"])
        e = a * a2 % Q
        ckeys, ni = process_bi(bi, xi, e, sp["salt"])
        out.append({"x": sp["x"], "y": sp["y"], "v": sp["v"], "salt": sp["salt"], "yi": yi, "xi": xi, "b": b, "bi": bi, "e": e,
                    "server_keys": skeys, "mac": mac, "client_keys": ckeys, "ni": ni})
    return {"cred": cred, "n": n, "k": k, "S": s, "a": a, "X": big_x, "gs": gs, "servers": out}
