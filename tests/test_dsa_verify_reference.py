"""CPU: the groundwork of raw DSA verification.  The Python restatement of crypto/dsa.Verify with its rules
(tests/dsa_verify_ref.py) against the oracle's dsa_verify and OpenSSL's DSA_do_verify over the seeded corpus
(tests/dsa_verify_cases.py), the conditions that corpus has to meet, the per-signature logic of k_dsav_prep
(bftkv_amd/csrc/dsa_verify.h) compiled for the host against the restatement, and the new C-ABI names."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dsa_verify_cases as K
import dsa_verify_ref as V
from oracle import openpgp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["bftkv_gpu_dsa_verify", "bftkv_gpu_dsa_verify_dev", "bftkv_gpu_batcher_dsa_verify"]
NAMES = [g.name for g in K.groups()]


def _verdict(cs):
    return V.verify(cs.p, cs.q, cs.g, cs.y, cs.digest, cs.r, cs.s)


def test_fixture_groups_are_what_the_issue_names():
    gs = {g.name: g for g in K.groups()}
    assert sorted(g.p.bit_length() for g in gs.values() if g.kind == "group" and g.name not in K.STANDARD) == [512, 512, 768, 1016, 1023, 1025, 2041, 2047, 2048]
    assert {g.q.bit_length() for g in gs.values() if g.kind == "group"} == {8, 64, 160, 224, 256}
    for g in gs.values():
        if g.kind == "group":
            assert (g.p - 1) % g.q == 0 and pow(g.g, g.q, g.p) == 1 and g.g != 1 and g.q.bit_length() % 8 == 0, g.name
    c, o, one = gs["composite_q160"], gs["q161"], gs["p_is_1"]
    assert c.q % 3 == 0 and c.q.bit_length() == 160 and c.q % 2 == 1 and c.p % 2 == 1 and pow(c.g, c.q, c.p) == 1 and pow(c.g, c.q // 3, c.p) != 1
    assert o.q.bit_length() == 161 and one.p == 1
    assert [gs[n].q.bit_length() for n in K.STANDARD] == [160, 224, 256, 256]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_oracle_over_the_corpus(name):
    G = K.group(name)
    cases = K.corpus(name)
    seen = set()
    for cs in cases:
        valid, st = _verdict(cs)
        seen.add((valid, st))
        if st == V.OK:
            assert openpgp.dsa_verify(cs.p, cs.q, cs.g, cs.y, cs.digest, cs.r, cs.s) == bool(valid), (name, cs.label)
        else:
            assert valid == 0
        if cs.part in ("honest", "mutation"):
            assert st == V.OK, (name, cs.label)           # nothing drawn at random is fenced or without an inverse
        if cs.part == "honest" and G.kind in ("group", "composite"):
            assert valid == 1, (name, cs.label)
    labels = {cs.label: _verdict(cs) for cs in cases}
    assert labels["dlen = bytes(q) + 1"] == ((0, V.FENCED) if G.kind != "odd_width" else (0, V.OK))
    assert labels["dlen = bytes(q) + 1, r = 0"] == (0, V.OK)           # the range rule comes first
    for lb in ("r = 0", "r = q", "s = 0", "s = q"):
        assert labels[lb] == (0, V.OK), (name, lb)
    if G.kind == "group":
        assert sum(v == (1, V.OK) for v in labels.values()) >= 6, name
        assert labels["digest = 0"] == (1, V.OK) and labels["u2 = 1"] == (1, V.OK) and labels["u2 = 5"] == (1, V.OK)
        assert labels.get("g >= p", (1, V.OK)) == (1, V.OK) and labels["y = 0"] == (0, V.OK)
        if "r + q" in labels:
            assert labels["r + q"] == (0, V.OK)
    if G.kind == "composite":
        for lb in ("s = 3", "s = 6", "s = 15", "s = q / 3"):
            assert labels[lb] == (0, V.NO_INVERSE), lb
        assert labels["s = 3 and one byte more"] == (0, V.FENCED)
        assert all(labels[f"s coprime to q #{j}"] == (1, V.OK) for j in range(3))
        assert seen == {(1, V.OK), (0, V.OK), (0, V.FENCED), (0, V.NO_INVERSE)}
    if G.kind in ("odd_width", "p_one"):
        assert not any(v for v, _ in labels.values()), name


def test_corpus_reaches_the_named_shapes():
    have = set()
    for name in NAMES:
        have |= {cs.label for cs in K.corpus(name)}
    assert {"r + q", "g >= p", "g = p", "y = p", "y = p + 1", "u2 = 1", "digest = 0"} <= have
    # g >= p with a valid signature exists under a modulus that fills its bytes, and under one that does not
    assert any(cs.label == "g >= p" for cs in K.corpus("p2048_q256")) and any(cs.label == "g >= p" for cs in K.corpus("p2047_q224"))


def test_two_hundred_honest_signatures_from_the_key_files():
    rng = np.random.default_rng(200)
    n = 0
    for name in K.STANDARD:
        keys = json.load(open(os.path.join(K.GOLDEN, "keys_%s.json" % name)))["keys"]
        for i in range(50):
            k = keys[i % len(keys)]
            p, q, g, x = (int(k[f], 16) for f in ("p", "q", "g", "x"))
            y = pow(g, x, p)
            dg = rng.bytes(q.bit_length() // 8)
            rs = None
            while rs is None:
                rs = K.sign(p, q, g, x, dg, K.rnd(rng, q) or 1)
            assert V.verify(p, q, g, y, dg, *rs) == (1, V.OK), (name, i)
            assert openpgp.dsa_verify(p, q, g, y, dg, *rs) is True, (name, i)
            n += 1
    assert n == 200


# ---- OpenSSL ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ossl():
    try:
        lib = C.CDLL("libcrypto.so.3")
    except OSError:
        pytest.skip("libcrypto.so.3 not loadable")
    vp = C.c_void_p
    for name, res, args in [("DSA_new", vp, []), ("DSA_free", None, [vp]), ("DSA_set0_pqg", C.c_int, [vp, vp, vp, vp]),
                            ("DSA_set0_key", C.c_int, [vp, vp, vp]), ("BN_bin2bn", vp, [C.c_char_p, C.c_int, vp]), ("DSA_SIG_new", vp, []),
                            ("DSA_SIG_set0", C.c_int, [vp, vp, vp]), ("DSA_SIG_free", None, [vp]),
                            ("DSA_do_verify", C.c_int, [C.c_char_p, C.c_int, vp, vp]), ("ERR_clear_error", None, [])]:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def openssl_verify(lib, cs):
    """DSA_do_verify's answer: 1, 0, or -1 (an error)."""
    def bn(v):
        b = v.to_bytes(max(1, K.nbytes(v)), "big")
        return lib.BN_bin2bn(b, len(b), None)
    d = lib.DSA_new()
    try:
        assert lib.DSA_set0_pqg(d, bn(cs.p), bn(cs.q), bn(cs.g)) == 1 and lib.DSA_set0_key(d, bn(cs.y), None) == 1
        s = lib.DSA_SIG_new()
        assert lib.DSA_SIG_set0(s, bn(cs.r), bn(cs.s)) == 1
        ok = lib.DSA_do_verify(cs.digest, len(cs.digest), s, d)
        lib.DSA_SIG_free(s)
        return ok
    finally:
        lib.DSA_free(d)
        lib.ERR_clear_error()


@pytest.mark.parametrize("name", K.STANDARD)
def test_restatement_against_openssl_under_the_standard_groups(ossl, name):
    n = 0
    for cs in K.corpus(name):
        valid, st = _verdict(cs)
        if st != V.OK:
            continue
        assert openssl_verify(ossl, cs) == valid, (name, cs.label, valid)
        n += 1
    assert n >= 40


# ---- the host-compiled rules of k_dsav_prep ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dvh(tmp_path_factory):
    so = tmp_path_factory.mktemp("dsav_host") / "dsa_verify_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "c", "dsa_verify_host.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.dvh_prep.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p]
    lib.dvh_prep.restype = C.c_int
    return lib


def _limbs(v):
    return [(v >> (28 * j)) & 0xFFFFFFF for j in range(10)]


@pytest.mark.parametrize("name", NAMES)
def test_host_compiled_prep_over_the_corpus(dvh, name):
    G = K.group(name)
    for cs in K.corpus(name):
        out = C.create_string_buffer(66 + 120)
        assert dvh.dvh_prep(K.sig_bytes(G, cs.r, cs.s), G.qbytes, cs.q.to_bytes(G.qbytes, "big"), cs.digest, len(cs.digest), out) == 0
        raw = out.raw
        got = (raw[0], raw[1], int.from_bytes(raw[2:34], "big"), int.from_bytes(raw[34:66], "big"))
        want = V.prep(cs.q, cs.digest, cs.r, cs.s)
        assert got == want, (name, cs.label, got, want)
        words = list(np.frombuffer(raw[66:], dtype="<u4"))
        assert words == _limbs(want[2]) + _limbs(want[3]) + _limbs(cs.r), (name, cs.label)


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
