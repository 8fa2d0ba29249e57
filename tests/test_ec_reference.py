"""CPU: the threshold-ECDSA groundwork.  The curve fixture against OpenSSL's named groups, the Python restatement of Go's
generic curve code (tests/ec_ref.py) against OpenSSL's EC_POINT arithmetic, the reference's own TestMul identity, the
host-compiled field and point code of bftkv_amd/csrc/ec_field.h against the restatement, and the new C-ABI names."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ec_ref as E
from oracle.threshold import lagrange

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIDS = {"P-224": 713, "P-256": 415, "P-384": 715, "P-521": 716}
NEW_NAMES = ["bftkv_gpu_ecdsa_calculate_r", "bftkv_gpu_ecdsa_calculate_r_dev", "bftkv_gpu_batcher_ecdsa_calculate_r",
             "bftkv_gpu_ec_scalar_base_mult"]


# ---- OpenSSL through ctypes (skipped where libcrypto.so.3 does not load) ---------------------------------------------
@pytest.fixture(scope="module")
def ossl():
    try:
        lib = C.CDLL("libcrypto.so.3")
    except OSError:
        pytest.skip("libcrypto.so.3 not loadable")
    vp = C.c_void_p
    for name, res, args in [("EC_GROUP_new_by_curve_name", vp, [C.c_int]), ("EC_GROUP_get_curve", C.c_int, [vp] * 5),
                            ("EC_GROUP_get0_generator", vp, [vp]), ("EC_GROUP_get0_order", vp, [vp]),
                            ("EC_POINT_new", vp, [vp]), ("EC_POINT_free", None, [vp]),
                            ("EC_POINT_get_affine_coordinates", C.c_int, [vp] * 5), ("EC_POINT_set_affine_coordinates", C.c_int, [vp] * 5),
                            ("EC_POINT_mul", C.c_int, [vp] * 6), ("EC_POINT_add", C.c_int, [vp] * 5), ("EC_POINT_is_at_infinity", C.c_int, [vp, vp]),
                            ("EC_GROUP_free", None, [vp]), ("BN_new", vp, []), ("BN_free", None, [vp]), ("BN_bin2bn", vp, [C.c_char_p, C.c_int, vp]),
                            ("BN_bn2binpad", C.c_int, [vp, C.c_char_p, C.c_int]), ("BN_num_bits", C.c_int, [vp])]:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def _bn(lib, v: int):
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return lib.BN_bin2bn(b, len(b), None)


def _int(lib, bn) -> int:
    n = (lib.BN_num_bits(bn) + 7) // 8
    buf = C.create_string_buffer(max(n, 1))
    lib.BN_bn2binpad(bn, buf, max(n, 1))
    return int.from_bytes(buf.raw, "big")


class _Ossl:
    def __init__(self, lib, name):
        self.lib, self.g = lib, lib.EC_GROUP_new_by_curve_name(NIDS[name])

    def point(self, xy):
        pt = self.lib.EC_POINT_new(self.g)
        if xy != (0, 0):
            bx, by = _bn(self.lib, xy[0]), _bn(self.lib, xy[1])
            assert self.lib.EC_POINT_set_affine_coordinates(self.g, pt, bx, by, None) == 1
        return pt

    def xy(self, pt):
        if self.lib.EC_POINT_is_at_infinity(self.g, pt):
            return (0, 0)
        bx, by = self.lib.BN_new(), self.lib.BN_new()
        assert self.lib.EC_POINT_get_affine_coordinates(self.g, pt, bx, by, None) == 1
        return _int(self.lib, bx), _int(self.lib, by)

    def mul(self, xy, k):
        r = self.lib.EC_POINT_new(self.g)
        assert self.lib.EC_POINT_mul(self.g, r, None, self.point(xy), _bn(self.lib, k), None) == 1
        return self.xy(r)

    def add(self, a, b):
        r = self.lib.EC_POINT_new(self.g)
        assert self.lib.EC_POINT_add(self.g, r, self.point(a), self.point(b), None) == 1
        return self.xy(r)


@pytest.mark.parametrize("name", E.NAMES)
def test_fixture_is_openssls_named_group(ossl, name):
    g = ossl.EC_GROUP_new_by_curve_name(NIDS[name])
    bp, ba, bb = ossl.BN_new(), ossl.BN_new(), ossl.BN_new()
    assert ossl.EC_GROUP_get_curve(g, bp, ba, bb, None) == 1
    gx, gy = ossl.BN_new(), ossl.BN_new()
    assert ossl.EC_POINT_get_affine_coordinates(g, ossl.EC_GROUP_get0_generator(g), gx, gy, None) == 1
    c = E.CURVES[name]
    assert (_int(ossl, bp), _int(ossl, ba), _int(ossl, bb)) == (c["p"], c["p"] - 3, c["b"])
    assert (_int(ossl, gx), _int(ossl, gy), _int(ossl, ossl.EC_GROUP_get0_order(g))) == (c["gx"], c["gy"], c["n"])
    assert c["p"].bit_length() == c["bit_size"]


@pytest.mark.parametrize("name", E.NAMES)
def test_restatement_against_openssl(ossl, name):
    c, o = E.CURVES[name], _Ossl(ossl, name)
    n = c["n"]
    rng = np.random.default_rng(11)
    g = (c["gx"], c["gy"])
    rnd = lambda: int.from_bytes(rng.bytes(E.byte_len(c) + 8), "big") % n   # noqa: E731
    pts = [E.scalar_base_mult(c, rnd()) for _ in range(3)] + [g]
    for pt in pts:
        assert E.is_on_curve(c, *pt)
        for k in (0, 1, 2, n - 1, n, rnd(), rnd()):
            assert E.scalar_mult(c, pt[0], pt[1], E.int_bytes(k)) == o.mul(pt, k), (name, k)
    for a, b in zip(pts, pts[1:]):
        assert E.add(c, *a, *b) == o.add(a, b)
    a = pts[0]
    assert E.add(c, *a, *E.point_neg(c, a)) == (0, 0) == o.add(a, E.point_neg(c, a))
    # P + P: the doubling reading the fences stay away from, against OpenSSL's doubling
    assert E.affine_from_jacobian(c, *E.add_jacobian(c, *a, 1, *a, 1)) == o.add(a, a) == E.scalar_mult(c, a[0], a[1], b"\x02")
    assert E.unmarshal(c, E.marshal(c, *a)) == a
    assert E.unmarshal(c, b"\x02" + E.marshal(c, *a)[1:]) is None
    assert E.unmarshal(c, E.marshal(c, 0, 0)) is None


@pytest.mark.parametrize("name", E.NAMES)
def test_reference_testmul_identity(name):
    """ecdsa_test.go's TestMul: shares f(x_i) of a polynomial with f(0) = f0, R_i = f(x_i) G, V_i = f(x_i): S = f0 G, v = f0,
    CalculateR = Gx mod N."""
    c = E.CURVES[name]
    n = c["n"]
    rng = np.random.default_rng(3)
    coef = [int.from_bytes(rng.bytes(E.byte_len(c) + 8), "big") % n for _ in range(4)]
    xs = [1, 2, 3, 4, 5, 6, 7, 8]
    fx = [sum(a * x ** i for i, a in enumerate(coef)) % n for x in xs]
    assert sum(lagrange(x, xs, n) * f for x, f in zip(xs, fx)) % n == coef[0]
    ri = [E.calculate_partial_r(c, f) for f in fx]
    assert E.calculate_r(c, xs, ri, fx) == (E.OK, c["gx"] % n)


# ---- the host-compiled ec_field.h -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ech(tmp_path_factory):
    so = tmp_path_factory.mktemp("ec_host") / "ec_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "c", "ec_host.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.ech_op.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.c_char_p]
    lib.ech_op.restype = C.c_int
    return lib


class _Host:
    def __init__(self, lib, c):
        self.lib, self.c, self.f = lib, c, E.byte_len(c)
        self.cb = b"".join(c[k].to_bytes(self.f, "big") for k in ("p", "n", "b", "gx", "gy"))

    def op(self, code, *nums, out_len=None):
        f = self.f
        buf = C.create_string_buffer(out_len or 2 * f + 1)
        assert self.lib.ech_op(self.cb, f, code, b"".join(v.to_bytes(f, "big") for v in nums), buf) == 0
        return buf.raw

    def num(self, code, *nums):
        return int.from_bytes(self.op(code, *nums)[:self.f], "big")

    def pt(self, code, *nums):
        r = self.op(code, *nums)
        return int.from_bytes(r[:self.f], "big"), int.from_bytes(r[self.f:2 * self.f], "big"), r[2 * self.f]


@pytest.mark.parametrize("name", E.NAMES)
def test_host_compiled_field_and_points(ech, name):
    c = E.CURVES[name]
    p, n = c["p"], c["n"]
    h = _Host(ech, c)
    rng = np.random.default_rng(7)
    rnd = lambda m: int.from_bytes(rng.bytes(h.f + 8), "big") % m   # noqa: E731
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, 1 << (c["bit_size"] - 1)] + [rnd(p) for _ in range(12)]
    for a in vals:
        b = rnd(p)
        assert h.num(0, a, b) == a * b % p
        assert h.num(1, a) == a * a % p
        assert h.num(2, a) == (pow(a, -1, p) if a else 0)
    for a in [0, 1, n - 1, rnd(n), rnd(n)]:
        b = rnd(n)
        assert h.num(3, a, b) == a * b % n
    g = (c["gx"], c["gy"])
    pts = [g] + [E.scalar_base_mult(c, rnd(n)) for _ in range(3)]
    for a, b in zip(pts, pts[1:]):
        assert h.pt(4, *a, *b) == (*E.add(c, *a, *b), 0)
        assert h.pt(5, *a)[:2] == E.scalar_mult(c, a[0], a[1], b"\x02")
    a = pts[1]
    assert h.pt(4, *a, *a) == (*E.scalar_mult(c, a[0], a[1], b"\x02"), 1)          # equal operands: doubling
    assert h.pt(4, *a, *E.point_neg(c, a)) == (0, 0, 2)                            # opposite: infinity
    assert h.pt(4, 0, 0, *a) == (*a, 3) and h.pt(4, *a, 0, 0) == (*a, 3)           # an operand at infinity
    assert h.pt(5, 0, 0)[:2] == (0, 0)
    for k in [0, 1, 2, n - 1, n, rnd(n)]:
        assert h.pt(6, *a, k)[:2] == E.scalar_mult(c, a[0], a[1], E.int_bytes(k)), k
    assert h.op(7, *a, out_len=1)[0] == 1
    assert h.op(7, a[0], (a[1] + 1) % p, out_len=1)[0] == 0
    assert h.op(7, 0, 0, out_len=1)[0] == 0
    assert h.op(7, p, a[1], out_len=1)[0] == 0


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_new_names_declared_and_exported():
    import __graft_entry__ as ge
    from bftkv_amd import _native
    hdr = open(os.path.join(ROOT, "include", "bftkv_gpu.h")).read()
    declared = set(re.findall(r"\b(bftkv_gpu_[a-z_0-9]+)\s*\(", hdr))
    ge.build()
    lib = _native.load_library()
    for name in NEW_NAMES:
        assert name in declared and name in _native.EXPORTS, name
        assert hasattr(lib, name), name
