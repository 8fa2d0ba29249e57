"""Threshold RSA signing (crypto/threshold/rsa/rsa.go) restated on Python integers: emsaEncode (:356-378), Sign (:140-178), splitKey
(:98-117), makeKeyTree / collectKeys (:75-127), and the client's missingKeys / registerPartialSignature / calculateSignature
(:264-338).  Not collected: the tests import it.  Randomness comes from the caller's random.Random, so a tree is a function of its seed."""
import math

OK, NO_INVERSE, INVALID_INPUT, FAILED = 0, 1, 3, 0xFF
W, LIMBS = 28, 76


# ---- emsaEncode and Sign ----------------------------------------------------------------------------------------------------------------
def emlen(n: int) -> int:
    return (n.bit_length() + 7) // 8


def emsa_encode(t: bytes, n: int):
    """em as an integer, or None where the reference returns crypto.ErrInvalidInput (padlen < 3)."""
    padlen = emlen(n) - len(t)
    if padlen < 3:
        return None
    em = bytearray(emlen(n))
    i = 0
    em[i] = 0x00
    i += 1
    em[i] = 0x01
    i += 1
    while i < padlen - 1:
        em[i] = 0xFF
        i += 1
    em[i] = 0x00
    i += 1
    em[i:] = t
    assert len(em) == emlen(n)
    return int.from_bytes(em, "big")


def em_limbs(t: bytes, n: int):
    """([76 limbs of 28 bits], refusal byte) as k_psign_em writes them: zero limbs for a refused request."""
    m = emsa_encode(t, n)
    if m is None:
        return [0] * LIMBS, INVALID_INPUT
    return [(m >> (W * j)) & ((1 << W) - 1) for j in range(LIMBS)], OK


def fragment(sign_byte: int, magnitude: int) -> int:
    """parsePartialParam (:457-469): the stored byte and chunk -> di"""
    return -magnitude if sign_byte != 0 else magnitude


def sign(t: bytes, n: int, frags):
    """Sign's loop over frags = [(sign byte, magnitude)] -> [(status, ci)]; a refused request refuses every fragment."""
    m = emsa_encode(t, n)
    if m is None:
        return [(INVALID_INPUT, 0)] * len(frags)
    out = []
    for sb, mag in frags:
        di = fragment(sb, mag)
        if di < 0:
            ci = pow(m, -di, n)
            if math.gcd(ci, n) != 1:                  # ModInverse returns nil and leaves ci alone: no statement, take the reference path
                out.append((NO_INVERSE, 0))
                continue
            ci = pow(ci, -1, n)
        else:
            ci = pow(m, di, n)
        out.append((OK, ci))
    return out


# ---- Distribute: the key tree -----------------------------------------------------------------------------------------------------------
def depth(idx: int, n: int) -> int:
    d = 0
    while idx != 0:
        idx = (idx - 1) // n
        d += 1
    return d


def in_path(i: int, path: int, n: int) -> bool:
    while path != 0:
        if i == (path - 1) % n:
            return True
        path = (path - 1) // n
    return False


def split_key(d: int, n: int, rng):
    mx = 1 << (abs(d).bit_length() * 2)
    di, total = [], 0
    for _ in range(n - 1):
        x = rng.randrange(mx)
        neg = x & 1
        x >>= 1
        if neg:
            x = -x
        di.append(x)
        total += x
    di.append(d - total)
    return di


class ParamTree:
    def __init__(self, idx, di, children):
        self.idx, self.di, self.children = idx, di, children


def make_key_tree(key: int, idx: int, n: int, k: int, rng) -> ParamTree:
    d = depth(idx, n)
    if d > n - k:
        return ParamTree(idx, key, None)
    di = split_key(key, n - d, rng)
    tr = ParamTree(idx, key, {})
    j = 0
    for i in range(n):
        if not in_path(i, idx, n):
            tr.children[i] = make_key_tree(di[j], idx * n + i + 1, n, k, rng)
            j += 1
    return tr


def collect_keys(tr: ParamTree, i: int, keys: dict):
    for j, c in (tr.children or {}).items():
        if j == i:
            keys[tr.idx] = c.di
        else:
            collect_keys(c, i, keys)


def distribute(d: int, n: int, k: int, rng):
    """-> [keys of server i: {kid: di}]"""
    kt = make_key_tree(d, 0, n, k, rng)
    shares = []
    for i in range(n):
        keys = {}
        collect_keys(kt, i, keys)
        shares.append(keys)
    return shares


def stored(di: int):
    """serializePartialParam (:419-430): (sign byte, k.Bytes())"""
    mag = abs(di)
    return (1 if di < 0 else 0), mag.to_bytes((mag.bit_length() + 7) // 8, "big")


# ---- the client -------------------------------------------------------------------------------------------------------------------------
class SigTree:
    def __init__(self, idx, psig, completed):
        self.idx, self.psig, self.completed, self.children = idx, psig, completed, None


def missing_keys(st, keys, n, k):
    if st is None or st.completed:
        return keys
    if not st.children:
        keys.append(st.idx)
    else:
        if depth(st.idx, n) >= n - k:
            return keys
        for i in range(n):
            if in_path(i, st.idx, n):
                continue
            c = st.children.get(i)
            if c is None:
                keys.append(st.idx * n + i + 1)
            elif not c.completed:
                keys = missing_keys(c, keys, n, k)
    return keys


def register_partial_signature(st, idx, psig, d, n):
    me = idx
    for _ in range(d - 1):
        me = (me - 1) // n
    i = (me - 1) % n
    if st.children is None:
        st.children = {}
    c = st.children.get(i)
    if c is None:
        c = SigTree(me, psig, True) if d <= 1 else SigTree(me, None, False)
        st.children[i] = c
    if d > 1:
        register_partial_signature(c, idx, psig, d - 1, n)
    if len(st.children) >= n - depth(st.idx, n):
        st.completed = all(ch.completed for ch in st.children.values())


def collect_signature(st, factors):
    """calculateSignature's walk: the partial signatures it multiplies, in its order"""
    if not st.completed:
        return
    if st.psig is not None:
        factors.append(st.psig)
        return
    for c in st.children.values():
        collect_signature(c, factors)


def client_factors(n: int, k: int, live, answer):
    """DistSign's rounds against the servers in `live`: MakeRequest (missingKeys) -> every live server's Sign -> ProcessResponse, until the
    tree is complete or a round asks what the last one asked.  answer(server, kid) -> ci, or None where the server holds no such key.
    -> the factors of calculateSignature, or None when no signature comes out."""
    tree = SigTree(0, None, False)
    last = None
    while not tree.completed:
        keys = missing_keys(tree, [], n, k)
        if not keys or keys == last:
            return None
        last = keys
        for srv in sorted(live):
            for kid in keys:
                ci = answer(srv, kid)
                if ci is not None:
                    idx = kid * n + srv + 1
                    register_partial_signature(tree, idx, ci, depth(idx, n), n)
    factors = []
    collect_signature(tree, factors)
    return factors


def fold(factors, n: int) -> int:
    s = 1
    for f in factors:
        s = s * f % n
    return s
