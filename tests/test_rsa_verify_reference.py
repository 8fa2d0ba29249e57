"""CPU: the groundwork of raw RSA PKCS#1 v1.5 verification.  The Python restatement of rsa.VerifyPKCS1v15 with its rules
(tests/rsa_verify_ref.py) against the oracle's rsa_verify_pkcs1v15 and OpenSSL over the seeded corpus (tests/rsa_verify_cases.py),
the conditions that corpus has to meet, the reference's known answer, the rules and the EM builder of k_rsav_verify
(bftkv_amd/csrc/rsa_verify.h) compiled for the host against the restatement, and the new C-ABI names.

OpenSSL: RSA_verify for six hashes.  Its RIPEMD-160 DigestInfo carries the TeleTrusT identifier where Go's (and so the reference's,
crypto/threshold/rsa/rsa.go:353) carries ISO/IEC 10118-3's, so for hash id 3 the comparison runs through RSA_public_decrypt with
PKCS#1 type-1 padding -- OpenSSL's arithmetic and padding check -- and the recovered T is compared with Go's prefix || digest.  The
set of cases left out of the OpenSSL comparison stays exactly {s >= n} | {even or trivial n} | {hash id 0}."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rsa_verify_cases as K
import rsa_verify_ref as V
from oracle import openpgp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["bftkv_gpu_rsa_verify", "bftkv_gpu_rsa_verify_dev", "bftkv_gpu_rsa_keyset_create", "bftkv_gpu_rsa_keyset_destroy",
             "bftkv_gpu_rsa_keyset_info", "bftkv_gpu_rsa_verify_keyset", "bftkv_gpu_rsa_verify_keyset_dev", "bftkv_gpu_batcher_rsa_verify",
             "bftkv_gpu_batcher_rsa_verify_keyset"]
HASH_NAME = {1: "md5", 2: "sha1", 3: "ripemd160", 8: "sha256", 9: "sha384", 10: "sha512", 11: "sha224"}
CELL_IDS = ["hash%d_dlen%d" % c for c in K.HASH_CELLS]


def _verdict(c):
    return V.verify(c.n, c.e, c.hash_id, c.digest, c.s)


def test_key_files_are_what_the_issue_names():
    ks = K.keys()
    assert len(ks) == 28 and ks[0].n.bit_length() == 256 and ks[-1].n.bit_length() == 2048
    assert {k.e for k in ks} == {3, 17, 65537}
    bits = {k.n.bit_length() for k in ks}
    # the k = tLen + 10 / tLen + 11 pair of every hash size class
    assert {360, 368, 456, 464, 488, 496, 616, 624, 744, 752} <= bits
    for k in ks:
        es = K.extra_exponents(k)
        assert len(es) == 3 and all(e % 2 == 1 and (e * k.d(e)) % ((k.p - 1) * (k.q - 1)) == 1 for e in es), k.name
    assert V.PREFIX[3] == openpgp.HASH_PREFIXES["ripemd160"] and all(V.PREFIX[h] == openpgp.HASH_PREFIXES[nm] for h, nm in HASH_NAME.items())


@pytest.mark.parametrize("cellid", K.HASH_CELLS, ids=CELL_IDS)
def test_restatement_against_the_oracle_over_the_corpus(cellid):
    hash_id, dlen = cellid
    cases = K.corpus(hash_id, dlen)
    labels = {}
    for c in cases:
        valid, st = _verdict(c)
        labels.setdefault(c.key, {})[c.label] = (valid, st)
        if hash_id and c.n > 1 and c.n % 2 == 1:         # (the oracle has no row 2, and pow() refuses n = 0)
            assert openpgp.rsa_verify_pkcs1v15(c.n, c.e, HASH_NAME[hash_id], c.digest, c.s.to_bytes(c.min_nbytes, "big")) == bool(valid), (c.key, c.label)
            assert st == V.OK
        if c.s >= c.n > 1:
            assert (valid, st) == V.verify(c.n, c.e, c.hash_id, c.digest, c.s % c.n), (c.key, c.label)      # s >= n answers as s mod n does
        if c.part in ("honest", "mutation", "forgery", "small_m"):
            assert st == V.OK, (c.key, c.label)          # nothing honest or bit-mutated is fenced
        if c.part in ("mutation", "forgery", "small_m"):
            assert valid == 0, (c.key, c.label)
        if c.part in ("honest", "wide"):
            assert (valid, st) == (1, V.OK), (c.key, c.label)
    tlen = len(V.PREFIX[hash_id]) + dlen
    for k in K.keys():
        lb = labels[k.name]
        if k.k >= tlen + 11:
            assert lb["honest"] == (1, V.OK) and lb["valid s + n"] == (1, V.OK) and lb["s = n + 1"] == (0, V.OK)
            assert lb["key: n - 1 (even)"] == (0, V.FENCED) and lb["key: n + 1 (even)"] == (0, V.FENCED)
            top = int(k.n.bit_length() % 8 != 1)             # a modulus whose top byte is 01 leaves no room for a forged 00 top
            assert sum(1 for x in lb if x.startswith("forged EM")) >= (9 if hash_id else 7) + top, k.name
        else:
            assert not any(v for v, _ in lb.values()) and lb["key: n - 1 (even)"] == (0, V.OK), k.name       # row 1 comes first
        assert lb["key: n = 0"] == (0, V.OK) and lb["key: n = 1"] == (0, V.OK)
    fit = [k.k for k in K.keys() if k.k >= tlen + 11]
    assert min(fit) == tlen + 11 or hash_id in (0, 1, 3), (hash_id, min(fit), tlen)      # the boundary pair exists for the five sizes the key files name


def test_exponent_classes_of_the_corpus():
    seen = set()
    for k in K.keys():
        for c in K.exponent_cases(k.name):
            valid, st = _verdict(c)
            assert st == V.OK
            seen.add(c.e)
            if c.label.endswith("honest") or c.label.endswith("honest + n") or c.label in ("e = 1, s = EM", "e = 1, s = EM + n"):
                assert valid == 1, (k.name, c.label)
            else:
                assert valid == 0, (k.name, c.label)
    assert {0, 1, 2, 65536} <= seen and any(e > 2**31 for e in seen) and any(2 < e < 16 for e in seen) and any(65537 < e < 70000 for e in seen)


def test_rsa1024_value_shapes_and_single_bit_forgeries():
    k = K.key("rsa1024")
    n, d = k.n, k.d()
    dg = hashlib.sha256(b"rsa1024").digest()
    EM = V.em(k.k, 8, dg)
    s = pow(int.from_bytes(EM, "big"), d, n)
    assert V.verify(n, k.e, 8, dg, s) == (1, V.OK) and V.verify(n, k.e, 8, dg, s + n) == (1, V.OK)
    assert V.verify(n, k.e, 8, dg, s + (n << 1000)) == (1, V.OK)
    for i in range(128):                                  # one bit in every byte of EM
        bad = bytearray(EM)
        bad[i] ^= 1 << (i % 8)
        m = int.from_bytes(bad, "big")
        if m < n:
            assert V.verify(n, k.e, 8, dg, pow(m, d, n)) == (0, V.OK), i
    for m in (0, 1, 2, n - 1):
        assert V.verify(n, k.e, 8, dg, pow(m, d, n)) == (0, V.OK)


def test_known_answer_of_the_reference():
    kat = json.load(open(os.path.join(K.GOLDEN, "threshold_kat.json")))["rsa"]
    n, e, sig = int(kat["n"], 16), int(kat["e"]), int(kat["sha256_pkcs1v15_sig"], 16)
    dg = hashlib.sha256(kat["tbs"].encode()).digest()
    assert V.verify(n, e, 8, dg, sig) == (1, V.OK)
    assert V.verify(n, e, 8, dg, sig ^ 1) == (0, V.OK) and V.verify(n, e, 8, bytes([dg[0] ^ 1]) + dg[1:], sig) == (0, V.OK)


# ---- OpenSSL ----------------------------------------------------------------------------------------------------------
NID = {1: 4, 2: 64, 8: 672, 9: 673, 10: 674, 11: 675}
RSA_PKCS1_PADDING = 1


@pytest.fixture(scope="module")
def ossl():
    try:
        lib = C.CDLL("libcrypto.so.3")
    except OSError:
        pytest.skip("libcrypto.so.3 not loadable")
    vp = C.c_void_p
    for name, res, args in [("RSA_new", vp, []), ("RSA_free", None, [vp]), ("RSA_set0_key", C.c_int, [vp, vp, vp, vp]),
                            ("BN_bin2bn", vp, [C.c_char_p, C.c_int, vp]), ("ERR_clear_error", None, []),
                            ("RSA_verify", C.c_int, [C.c_int, C.c_char_p, C.c_uint, C.c_char_p, C.c_uint, vp]),
                            ("RSA_public_decrypt", C.c_int, [C.c_int, C.c_char_p, C.c_char_p, vp, C.c_int])]:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def openssl_verify(lib, c):
    def bn(v):
        b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
        return lib.BN_bin2bn(b, len(b), None)
    k = (c.n.bit_length() + 7) // 8
    sig = c.s.to_bytes(k, "big")
    r = lib.RSA_new()
    try:
        assert lib.RSA_set0_key(r, bn(c.n), bn(c.e), None) == 1
        if c.hash_id in NID:
            return int(lib.RSA_verify(NID[c.hash_id], c.digest, len(c.digest), sig, k, r) == 1)
        out = C.create_string_buffer(k)
        got = lib.RSA_public_decrypt(k, sig, out, r, RSA_PKCS1_PADDING)
        return int(got > 0 and out.raw[:got] == V.PREFIX[c.hash_id] + c.digest)
    finally:
        lib.RSA_free(r)
        lib.ERR_clear_error()


def test_restatement_against_openssl(ossl):
    cases = K.everything()
    left_out = {i for i, c in enumerate(cases) if c.s >= c.n} | {i for i, c in enumerate(cases) if c.n % 2 == 0 or c.n <= 1} | \
               {i for i, c in enumerate(cases) if c.hash_id == 0}
    compared = [i for i, c in enumerate(cases) if c.s < c.n and c.n % 2 == 1 and c.hash_id != 0]
    assert set(range(len(cases))) - set(compared) == left_out            # computed from the inputs, never from answers
    n_valid = 0
    for i in compared:
        c = cases[i]
        valid, st = _verdict(c)
        assert st == V.OK
        assert openssl_verify(ossl, c) == valid, (c.key, c.hash_id, c.label, valid)
        n_valid += valid
    assert len(compared) > 2000 and n_valid > 150


# ---- the host-compiled rules and EM builder of k_rsav_verify -----------------------------------------------------------------
@pytest.fixture(scope="module")
def rvh(tmp_path_factory):
    so = tmp_path_factory.mktemp("rsav_host") / "rsa_verify_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "c", "rsa_verify_host.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.rvh_em_limbs.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_void_p]
    lib.rvh_rule.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.rvh_shape.argtypes = [C.c_uint32, C.c_uint32]
    return lib


@pytest.mark.parametrize("cellid", K.HASH_CELLS, ids=CELL_IDS)
def test_host_compiled_em_limbs(rvh, cellid):
    """em_limb at W = 28 and 29 is the restatement's EM, limb for limb: every k from tLen + 11 to 256, every limb of 72, 76 and 80."""
    hash_id, dlen = cellid
    dg = np.random.default_rng(hash_id * 100 + dlen).bytes(dlen)
    tlen = len(V.PREFIX[hash_id]) + dlen
    out = np.zeros(80, dtype=np.uint32)
    for k in range(tlen + 11, 257):
        em = int.from_bytes(V.em(k, hash_id, dg), "big")
        for W in (28, 29):
            want = [(em >> (W * j)) & ((1 << W) - 1) for j in range(80)]
            for nl in (72, 76, 80):
                out[:] = 0xFFFFFFFF
                assert rvh.rvh_em_limbs(W, nl, k, hash_id, dg, dlen, out.ctypes.data) == 0
                assert out[:nl].tolist() == want[:nl], (k, W, nl)
    assert rvh.rvh_em_limbs(28, 76, tlen + 10, hash_id, dg, dlen, out.ctypes.data) == -1


def test_host_compiled_rules_on_every_key_shape(rvh):
    out = np.zeros(3, dtype=np.uint32)
    seen = set()
    for hash_id, dlen in K.HASH_CELLS:
        ns = set()
        for k in K.keys():
            ns |= {k.n, k.n - 1, k.n + 1}
        for n in sorted(ns | {0, 1, 2, 3, (1 << 2048) - 1, 1 << 2047}):
            for nbytes in sorted({max(1, (n.bit_length() + 7) // 8), 256}):
                assert rvh.rvh_rule(n.to_bytes(nbytes, "big"), nbytes, hash_id, dlen, out.ctypes.data) == 0
                r = V.rule(n, hash_id, dlen)
                assert out.tolist() == [r, V.FENCED if r == 2 else V.OK, (n.bit_length() + 7) // 8], (n.bit_length(), hash_id, dlen)
                seen.add(r)
    assert seen == {0, 1, 2}
    for hash_id in range(0, 16):
        for dlen in range(0, 70):
            want = (hash_id == 0 and 1 <= dlen <= 64) or V.DLEN.get(hash_id) == dlen
            assert rvh.rvh_shape(hash_id, dlen) == int(want), (hash_id, dlen)


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
