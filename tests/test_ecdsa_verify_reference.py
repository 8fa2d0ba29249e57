"""CPU: the groundwork of ECDSA verification.  The Python restatement of crypto/ecdsa.Verify with its fence rules
(tests/ecdsa_verify_ref.py) against OpenSSL's ECDSA_do_verify over the seeded corpus (tests/ecdsa_verify_cases.py), the fence
rate of that corpus, the new pieces of bftkv_amd/csrc/ec_field.h compiled for the host against the restatement, and the new
C-ABI names."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ec_ref as E
import ecdsa_verify_cases as K
import ecdsa_verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIDS = {"P-224": 713, "P-256": 415, "P-384": 715, "P-521": 716}
NEW_NAMES = ["bftkv_gpu_ecdsa_verify", "bftkv_gpu_ecdsa_verify_dev", "bftkv_gpu_batcher_ecdsa_verify"]


@pytest.fixture(scope="module")
def ossl():
    try:
        lib = C.CDLL("libcrypto.so.3")
    except OSError:
        pytest.skip("libcrypto.so.3 not loadable")
    vp = C.c_void_p
    for name, res, args in [("EC_KEY_new_by_curve_name", vp, [C.c_int]), ("EC_KEY_set_public_key_affine_coordinates", C.c_int, [vp, vp, vp]),
                            ("EC_KEY_free", None, [vp]), ("BN_bin2bn", vp, [C.c_char_p, C.c_int, vp]), ("ECDSA_SIG_new", vp, []),
                            ("ECDSA_SIG_set0", C.c_int, [vp, vp, vp]), ("ECDSA_SIG_free", None, [vp]),
                            ("ECDSA_do_verify", C.c_int, [C.c_char_p, C.c_int, vp, vp]), ("ERR_clear_error", None, [])]:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def openssl_verify(lib, name, key: bytes, digest: bytes, sig: bytes):
    """ECDSA_do_verify's verdict (True / False), or None where OpenSSL takes no such key."""
    c = E.CURVES[name]
    f = E.byte_len(c)
    bn = lambda b: lib.BN_bin2bn(b, len(b), None)   # noqa: E731
    k = lib.EC_KEY_new_by_curve_name(NIDS[name])
    try:
        if key[0] != 4 or lib.EC_KEY_set_public_key_affine_coordinates(k, bn(key[1:1 + f]), bn(key[1 + f:])) != 1:
            return None
        s = lib.ECDSA_SIG_new()
        assert lib.ECDSA_SIG_set0(s, bn(sig[:f]), bn(sig[f:])) == 1
        ok = lib.ECDSA_do_verify(digest, len(digest), s, k) == 1
        lib.ECDSA_SIG_free(s)
        return ok
    finally:
        lib.EC_KEY_free(k)
        lib.ERR_clear_error()


def _special_points(name):
    import ec_form_cases as F
    return F.special_x_points(name)


@pytest.mark.parametrize("name", E.NAMES)
def test_restatement_against_openssl_over_the_corpus(ossl, name):
    c = E.CURVES[name]
    cases = K.corpus(name)
    assert {len(cs.digest) for cs in cases} <= set(K.DLENS)
    recorded = []
    for cs in cases:
        valid, st = V.verify(c, cs.key, cs.digest, cs.sig)
        got = "fenced" if st == V.FENCED else ("valid" if valid else "invalid")
        assert cs.expect in (None, got), (name, cs.label, got)
        o = openssl_verify(ossl, name, cs.key, cs.digest, cs.sig)
        if st == V.FENCED:
            # OpenSSL's mathematical verdict is recorded, not compared; it is the restatement's unfenced reading all the same
            recorded.append((cs.label, o))
            m = V.verify_math(c, cs.key, cs.digest, cs.sig)
            assert (o is None and m is None) or o == bool(m), (name, cs.label)
        else:
            assert o is not None and o == bool(valid), (name, cs.label, o, valid)
    print(name, "fenced cases, OpenSSL's verdict:", recorded)
    labels = {cs.label for cs in cases}
    assert {"x(R) >= N #0", "u1 G = u2 Q", "u1 G = -u2 Q", "e = 0 dlen=32", "r = N", "s = 0xFF.."} <= labels
    assert dict(recorded)["u1 G = u2 Q"] is True          # the doubling case is a valid signature mathematically
    # the group "special_x": R at the smallest and largest x and at the Montgomery-form x next to p - 1 and 2^(32 L - 1), each with r + 1
    special = [cs for cs in cases if cs.group == "special_x"]
    assert special == list(cases[-len(special):]) and len(special) == (6 if name == "P-521" else 8)
    assert [cs.expect for cs in special[1::2]] == ["invalid"] * (len(special) // 2)
    assert [cs.expect for cs in special[0::2]] == (["valid"] if name == "P-224" else ["invalid"]) + ["valid"] * (len(special) // 2 - 1)
    for cs in special:
        u1, u2 = V.hash_to_int(c, cs.digest), V.split_sig(c, cs.sig)[0]
        w = pow(V.split_sig(c, cs.sig)[1], -1, c["n"])
        q = E.unmarshal(c, cs.key)
        rpt = E.add(c, *E.scalar_base_mult(c, u1 * w % c["n"]), *E.scalar_mult(c, q[0], q[1], E.int_bytes(u2 * w % c["n"])))
        # R = u1 G + u2 Q is the special point; with r + 1 it is another, but for x = 0 (r = 0 is refused, s = 1 / b, so r + 1 = 1 gives that R)
        if u2 and ("r + 1" not in cs.label or cs.label.startswith("R of smallest x = 0")):
            assert rpt in [pt for _, pt in _special_points(name)], (name, cs.label)


@pytest.mark.parametrize("name", E.NAMES)
def test_fence_rate(name):
    """A fence cannot hide a wrong answer: outside the listed constructions and the keys that are no points, nothing is fenced."""
    c = E.CURVES[name]
    allowed = {"u1 G = u2 Q", "e = N"}
    for cs in K.corpus(name):
        st = V.verify(c, cs.key, cs.digest, cs.sig)[1]
        if cs.group in ("honest", "mutation", "boundary"):
            assert st == V.OK, (name, cs.label)
        elif cs.group == "keyflip":
            assert (st == V.FENCED) == (E.unmarshal(c, cs.key) is None), (name, cs.label)
        else:
            assert (st == V.FENCED) == (cs.label in allowed or cs.label.startswith("e = 0")), (name, cs.label)


def test_hash_to_int_rules():
    c = E.CURVES["P-521"]
    d = bytes(range(1, 67))
    assert V.hash_to_int(c, d) == int.from_bytes(d, "big") >> 7
    assert V.hash_to_int(c, d + b"\x55") == int.from_bytes(d, "big") >> 7          # longer: the leftmost 66 bytes
    assert V.hash_to_int(c, d[:65]) == int.from_bytes(d[:65], "big")              # shorter: whole, no shift
    c = E.CURVES["P-224"]
    assert V.hash_to_int(c, b"\xff" * 32) == (1 << 224) - 1 > c["n"]


# ---- the host-compiled pieces of ec_field.h ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def evh(tmp_path_factory):
    so = tmp_path_factory.mktemp("ecv_host") / "ecdsa_verify_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "c", "ecdsa_verify_host.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.evh_op.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p]
    lib.evh_op.restype = C.c_int
    return lib


class _Host:
    def __init__(self, lib, c):
        self.lib, self.c, self.f = lib, c, E.byte_len(c)
        self.cb = b"".join(c[k].to_bytes(self.f, "big") for k in ("p", "n", "b", "gx", "gy"))

    def raw(self, code, arg, data: bytes, out_len):
        buf = C.create_string_buffer(out_len)
        assert self.lib.evh_op(self.cb, self.f, self.c["bit_size"], code, arg, data, len(data), buf) == 0
        return buf.raw

    def op(self, code, arg, *nums, out_len=None):
        return self.raw(code, arg, b"".join(v.to_bytes(self.f, "big") for v in nums), out_len or 2 * self.f + 1)

    def pt(self, code, arg, *nums):
        r = self.op(code, arg, *nums)
        return int.from_bytes(r[:self.f], "big"), int.from_bytes(r[self.f:2 * self.f], "big"), r[2 * self.f]


@pytest.mark.parametrize("name", E.NAMES)
def test_host_compiled_mixed_addition(evh, name):
    c = E.CURVES[name]
    p = c["p"]
    h = _Host(evh, c)
    rng = np.random.default_rng(21)
    pts = [E.scalar_base_mult(c, K.rnd(rng, c)) for _ in range(4)] + [(c["gx"], c["gy"])]
    for a, b in zip(pts, pts[1:]):
        for z in (1, 2, p - 1, K.rnd(rng, c, p) or 1):
            assert h.pt(0, 0, *a, z, *b) == (*E.add(c, *a, *b), 0), (name, z)
    a = pts[0]
    z = K.rnd(rng, c, p) or 1
    assert h.pt(0, 0, *a, z, *a) == (*E.scalar_mult(c, a[0], a[1], b"\x02"), 1)          # equal: doubling
    assert h.pt(0, 0, *a, z, *E.point_neg(c, a)) == (0, 0, 2)                            # opposite: infinity
    assert h.pt(0, 0, 0, 0, 0, *a) == (*a, 3)                                            # the Jacobian operand at infinity


@pytest.mark.parametrize("name", E.NAMES)
def test_host_compiled_fixed_base_table(evh, name):
    c = E.CURVES[name]
    n, f = c["n"], E.byte_len(c)
    h = _Host(evh, c)
    rng = np.random.default_rng(22)
    for w in (4, 5):
        nwin = (8 * f + w - 1) // w
        # entries: j 2^(w i) G, the corners and a seeded sample
        picks = [(0, 1), (0, (1 << w) - 1), (nwin - 1, 1), (nwin - 1, (1 << w) - 1)]
        picks += [(int(rng.integers(nwin)), int(rng.integers(1, 1 << w))) for _ in range(4)]
        for i, j in picks:
            k = (j << (w * i)) % n
            assert h.pt(2, w | i << 8 | j << 20)[:2] == E.scalar_base_mult(c, k), (name, w, i, j)
        # lookups
        for k in [1, 2, 15, 16, (1 << w) - 1, 1 << w, n - 1, n - 2, (1 << (c["bit_size"] - 1))] + [K.rnd(rng, c) for _ in range(6)]:
            assert h.pt(1, w, k % n)[:2] == E.scalar_base_mult(c, k % n), (name, w, k)
        assert h.pt(1, w, 0)[:2] == (0, 0)


@pytest.mark.parametrize("name", E.NAMES)
def test_host_compiled_hash_to_int(evh, name):
    c = E.CURVES[name]
    f = E.byte_len(c)
    h = _Host(evh, c)
    rng = np.random.default_rng(23)
    digests = [rng.bytes(dlen) for dlen in (1, 19, 20, 27, 28, 29, 32, 47, 48, 49, 64, 65, 66) for _ in range(3)]
    digests += [b"\xff" * dlen for dlen in (28, 32, 48, 66)] + [bytes(32), (c["n"] << (8 * f - c["n"].bit_length())).to_bytes(f, "big")]
    for d in digests:
        assert int.from_bytes(h.raw(3, 0, d, f), "big") == V.hash_to_int(c, d) % c["n"], (name, d.hex())


@pytest.mark.parametrize("name", E.NAMES)
def test_host_compiled_x_comparison(evh, name):
    c = E.CURVES[name]
    p, n = c["p"], c["n"]
    h = _Host(evh, c)
    rng = np.random.default_rng(24)
    pts = [E.scalar_base_mult(c, K.rnd(rng, c)) for _ in range(4)]
    # points with x in [N, p): the second branch, r + N = x; and with x below p - N, where r + N < p is tried and must not match
    for lo, span in ((n + 1, p - n - 1), (1, p - n - 1)):
        want = len(pts) + 3
        while len(pts) < want:
            x = lo + K.rnd(rng, c, span)
            y = K.sqrt_mod(x * x * x - 3 * x + c["b"], p)
            if y is not None:
                pts.append((x, y))
    assert sum(x >= n for x, _ in pts) == 3 and sum(x < p - n for x, _ in pts) == 3
    for x, y in pts:
        assert E.is_on_curve(c, x, y)
        for z in (1, K.rnd(rng, c, p) or 1):
            r = x % n
            assert h.op(4, 0, x, y, z, r, out_len=1)[0] == 1, (name, x >= n)
            for bad in (r ^ 1, (r + 1) % n or 1, (x + 1) % n or 1, n - 1 if r != n - 1 else 1):
                if bad != r and 0 < bad < n:
                    assert h.op(4, 0, x, y, z, bad, out_len=1)[0] == 0, (name, bad)


@pytest.mark.parametrize("name", E.NAMES)
def test_host_compiled_pieces_in_the_kernels_order_over_the_corpus(evh, name):
    """The header pieces strung together as k_ecv_prep / k_ecv_base / k_ecv_key string them, on every case of the corpus."""
    c = E.CURVES[name]
    n, f = c["n"], E.byte_len(c)
    h = _Host(evh, c)
    for cs in K.corpus(name):
        _, s = V.split_sig(c, cs.sig)
        w = pow(s, -1, n) if 0 < s < n else 1
        got = h.raw(5, 4, cs.key + cs.sig + w.to_bytes(f, "big") + cs.digest, 2)
        assert (got[0], got[1]) == V.verify(c, cs.key, cs.digest, cs.sig), (name, cs.label)


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_verify_names_declared_and_exported():
    import __graft_entry__ as ge
    from bftkv_amd import _native
    hdr = open(os.path.join(ROOT, "include", "bftkv_gpu.h")).read()
    declared = set(re.findall(r"\b(bftkv_gpu_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW_NAMES:
        assert name in declared and name in _native.EXPORTS, name
    ge.build()
    lib = _native.load_library()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
