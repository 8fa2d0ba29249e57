"""Writes tests/golden/ec_curves.json: the domain parameters of crypto/elliptic's four curves (P-224, P-256, P-384, P-521),
read from OpenSSL's named groups (secp224r1, prime256v1, secp384r1, secp521r1) through libcrypto.so.3.

    python tests/golden/make_ec_curves.py
"""
import ctypes as C
import json
import os

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ec_curves.json")
NAMES = [("P-224", 713, 224), ("P-256", 415, 256), ("P-384", 715, 384), ("P-521", 716, 521)]   # NIDs of OpenSSL's obj_mac.h


def load_crypto():
    lib = C.CDLL("libcrypto.so.3")
    vp = C.c_void_p
    lib.EC_GROUP_new_by_curve_name.restype = vp
    lib.EC_GROUP_new_by_curve_name.argtypes = [C.c_int]
    lib.EC_GROUP_get_curve.argtypes = [vp, vp, vp, vp, vp]
    lib.EC_GROUP_get0_generator.restype = vp
    lib.EC_GROUP_get0_generator.argtypes = [vp]
    lib.EC_GROUP_get0_order.restype = vp
    lib.EC_GROUP_get0_order.argtypes = [vp]
    lib.EC_POINT_get_affine_coordinates.argtypes = [vp, vp, vp, vp, vp]
    lib.EC_GROUP_free.argtypes = [vp]
    lib.BN_new.restype = vp
    lib.BN_free.argtypes = [vp]
    lib.BN_bn2hex.restype = C.c_void_p
    lib.BN_bn2hex.argtypes = [vp]
    lib.CRYPTO_free.argtypes = [vp, C.c_char_p, C.c_int]
    return lib


def bn_int(lib, bn) -> int:
    p = lib.BN_bn2hex(bn)
    s = C.cast(p, C.c_char_p).value.decode()
    lib.CRYPTO_free(p, b"", 0)
    return int(s, 16)


def read_curves(lib):
    out = {}
    for name, nid, bits in NAMES:
        g = lib.EC_GROUP_new_by_curve_name(nid)
        bp, ba, bb, gx, gy = (lib.BN_new() for _ in range(5))
        assert lib.EC_GROUP_get_curve(g, bp, ba, bb, None) == 1
        assert lib.EC_POINT_get_affine_coordinates(g, lib.EC_GROUP_get0_generator(g), gx, gy, None) == 1
        p, a, b = bn_int(lib, bp), bn_int(lib, ba), bn_int(lib, bb)
        assert a == p - 3
        out[name] = {"bit_size": bits, "p": hex(p), "n": hex(bn_int(lib, lib.EC_GROUP_get0_order(g))), "b": hex(b),
                     "gx": hex(bn_int(lib, gx)), "gy": hex(bn_int(lib, gy))}
        for x in (bp, ba, bb, gx, gy):
            lib.BN_free(x)
        lib.EC_GROUP_free(g)
    return out


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(read_curves(load_crypto()), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)
