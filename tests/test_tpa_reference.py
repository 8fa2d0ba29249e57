"""CPU: the restatement of crypto/auth (tests/tpa_ref.py) closes the protocol's loop and agrees with OpenSSL; the corpus
(tests/tpa_cases.py) holds every class it promises; the library exports the password-authentication entries, and each direct entry
refuses a NULL context before it needs a device, failing closed."""
import concurrent.futures
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import tpa_cases as K
import tpa_ref as R
from bftkv_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bftkv_gpu_tpa_yi", "bftkv_gpu_tpa_bi", "bftkv_gpu_tpa_ni", "bftkv_gpu_batcher_tpa_yi", "bftkv_gpu_batcher_tpa_bi"]
E_INVALID, FAILED = -1, 0xFF


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", K.honest_runs(), ids=lambda r: "n%d_k%d" % (r["n"], r["k"]))
def test_round_trip(run):
    assert len(run["servers"]) == run["k"]
    for s in run["servers"]:
        assert s["mac"] == s["ni"], s["x"]                           # makeZi's compare would pass
        assert s["server_keys"] == s["client_keys"], s["x"]          # km and ke: the client can open Zi
        assert s["server_keys"][16:] == s["client_keys"][16:]
    assert run["gs"] == pow(R.PI(run["cred"]), run["a"] * run["S"] % R.Q, R.P)
    assert len({s["mac"] for s in run["servers"]}) == run["k"]


def test_p_is_a_safe_prime_of_2048_bits():
    assert R.P.bit_length() == 2048 and R.P % 2 == 1 and R.Q * 2 + 1 == R.P
    for a in (2, 3, 5, 7):                                           # Fermat witnesses: a fixture that was cut short would not pass
        assert pow(a, R.P - 1, R.P) == 1 and pow(a, R.Q - 1, R.Q) == 1


def _openssl(args, stdin=b""):
    r = subprocess.run(["openssl"] + args, input=stdin, capture_output=True, timeout=60)
    assert r.returncode == 0, (args[:4], r.stderr[-300:])
    return r.stdout


def _secrets_and_keys():
    """Every (Ki.Bytes(), salt) that the corpus feeds to HKDF and every (km, Xi | Bi.Bytes()) it feeds to the MAC, on both sides."""
    hk, mac = set(), set()
    for op, (vb, _, _) in zip(K.corpus(), K.expected()):
        ki_server = R.exp(int.from_bytes(op.xi, "big"), op.b, op.p)
        for ki, bi in ((ki_server, vb), (vb, op.v)):
            hk.add((R.to_bytes(ki), op.salt))
            mac.add((R.key_sched(R.to_bytes(ki), op.salt)[0], op.xi + R.to_bytes(bi)))
    return sorted(hk), sorted(mac)


def test_hkdf_and_hmac_against_openssl():
    if shutil.which("openssl") is None or b"HKDF" not in subprocess.run(["openssl", "list", "-kdf-algorithms"], capture_output=True).stdout:
        pytest.skip("no openssl with the kdf command on the path")
    hk, mac = _secrets_and_keys()
    hk = [(s, salt) for s, salt in hk if s]
    assert len(hk) > 500 and len(mac) > 500 and {len(s) for s, _ in hk} >= {1, 55, 56, 255, 256}

    def kdf(item):
        secret, salt = item
        args = ["kdf", "-keylen", "32", "-kdfopt", "digest:SHA2-256", "-kdfopt", "hexkey:" + secret.hex()]
        if salt:
            args += ["-kdfopt", "hexsalt:" + salt.hex()]
        return _openssl(args + ["-binary", "HKDF"]) == R.hkdf32(secret, salt)

    def hm(item):
        key, msg = item
        return _openssl(["dgst", "-sha256", "-mac", "hmac", "-macopt", "hexkey:" + key.hex(), "-binary"], msg) == R.hmac_sha256(key, msg)

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        assert all(ex.map(kdf, hk))
        assert all(ex.map(hm, mac))


# ---- the corpus: every class it promises, class by class ------------------------------------------------------------------------------
def _tags():
    return set().union(*(op.tags for op in K.corpus()))


def test_corpus_size_and_shapes():
    ops = K.corpus()
    assert 300 <= len(ops) <= 700
    shapes = set(K.by_shape())
    assert shapes == set(K.SHAPES)
    assert {s[0] for s in shapes} == {128, 255, 256} and {s[1] for s in shapes} == {1, 32, 255, 256} and {s[2] for s in shapes} == {0, 16, 32, 64}
    for op in ops:
        assert op.p & 1 and op.p.bit_length() <= 8 * op.nbytes and len(op.xi) <= op.nbytes and len(op.salt) <= 64


def test_corpus_moduli():
    m = K.moduli()
    assert m["auth_p"] == R.P
    bits = sorted(v.bit_length() for v in m.values())
    assert bits[0] == 1023 and bits[-1] == 2048
    assert any(b % 8 for b in bits) and any(b % 28 for b in bits) and {1023, 1025, 2041, 2047} <= set(bits)
    assert len(m) >= 6 and {"mod:" + k for k in m} <= _tags()


def test_corpus_bases():
    tags = _tags()
    for which in ("v", "xi"):
        for cls in K.BASE_CLASSES:
            assert "base:%s:%s" % (which, cls) in tags
    top = {(op.nbytes, op.v) for op in K.corpus() if "base:v:max" in op.tags}
    assert all(v == (1 << (8 * nb)) - 1 for nb, v in top) and {nb for nb, _ in top} == {128, 255, 256}
    assert any(op.v == op.p for op in K.corpus()) and any(op.v == op.p + 1 for op in K.corpus()) and any(op.v == op.p - 1 for op in K.corpus())
    assert any(int.from_bytes(op.xi, "big") == op.p for op in K.corpus()) and any(op.xi == b"" for op in K.corpus())


def test_corpus_exponents():
    by_len = {}
    for op in K.corpus():
        by_len.setdefault(op.exp_len, set()).add(op.b)
    assert set(by_len) == {1, 32, 255, 256}
    for el, es in by_len.items():
        bits = 8 * el
        assert {0, 1, 2, 15, 16, (1 << bits) - 1, int.from_bytes(b"\x0f" * el, "big"), int.from_bytes(b"\xf0" * el, "big")} <= es, el
    full = by_len[256]
    assert {R.Q, R.P - 1} <= full
    for j in range(1, 74):                                           # every limb edge of the radix-2^28 form
        assert {1 << (28 * j), (1 << (28 * j)) - 1} <= full, j
    for k in (27, 28, 29, 1007, 1008, 1009, 2043, 2044, 2045, 3, 4, 5, 1019, 1020, 1021):      # limb and window edges, with neighbours
        assert {1 << k, (1 << k) - 1} <= full, k
    for el in (32, 255):
        assert {1 << 28, (1 << 28) - 1, 1 << 4, (1 << 4) - 1, 1 << 27, 1 << 29} <= by_len[el]


def test_corpus_honest_runs():
    tags = _tags()
    assert {"honest:5/3", "honest:10/7", "honest:yi", "honest:bi", "honest:ni"} <= tags
    n = {w: sum(1 for op in K.corpus() if w in op.tags) for w in ("honest:5/3", "honest:10/7")}
    assert n == {"honest:5/3": 9, "honest:10/7": 21}
    exp = dict(zip(K.corpus(), K.expected()))
    for run in K.honest_runs():
        for s in run["servers"]:
            bi_op = next(op for op in K.corpus() if "honest:bi" in op.tags and op.v == s["v"] and op.b == s["b"])
            ni_op = next(op for op in K.corpus() if "honest:ni" in op.tags and op.v == s["bi"] and op.b == s["e"])
            assert exp[bi_op][1] == (s["bi"], s["server_keys"], s["mac"]) and exp[ni_op][2] == (s["client_keys"], s["ni"])
            assert exp[bi_op][1][1:] == exp[ni_op][2]


def test_corpus_hkdf_secret_lengths():
    want = {"ki:0": 0, "ki:0z": 0, "ki:1": 1, "ki:55": 55, "ki:56": 56, "ki:255": 255, "ki:256": 256}
    for tag, n in want.items():
        ops = [op for op in K.corpus() if tag in op.tags]
        assert ops, tag
        for op in ops:
            assert op.p == R.P and len(R.to_bytes(R.exp(int.from_bytes(op.xi, "big"), op.b, op.p))) == n, tag
    one = next(op for op in K.corpus() if "ki:1" in op.tags)
    assert R.exp(int.from_bytes(one.xi, "big"), one.b, one.p) == 1


def test_corpus_mac_inputs():
    exp = dict(zip(K.corpus(), K.expected()))
    seen = {}
    for op in K.corpus():
        if any(t.startswith("mac:") for t in op.tags):
            seen.setdefault(len(R.to_bytes(exp[op][0])), set()).add(len(op.xi))
    assert seen[256] >= set(K.XI_LENS) == {0, 1, 55, 56, 63, 64, 119, 120, 255, 256}
    assert {255, 0, 1} <= set(seen)                                  # a Bi with a leading zero byte, Bi = 0 and Bi = 1
    residues = {(xl + bl) % 64 for bl, xls in seen.items() if bl != 256 for xl in xls}
    assert {0, 55, 56, 63} <= residues and {0, 55, 56, 63} <= {xl % 64 for xl in seen[256]}


def test_corpus_raw_xi():
    exp = dict(zip(K.corpus(), K.expected()))
    plain = next(op for op in K.corpus() if "rawxi:plain" in op.tags)
    zeros = next(op for op in K.corpus() if "rawxi:zeros" in op.tags)
    assert zeros.xi == b"\0\0" + plain.xi and plain._replace(xi=b"", tags=None) == zeros._replace(xi=b"", tags=None)
    assert exp[plain][1][:2] == exp[zeros][1][:2] and exp[plain][1][2] != exp[zeros][1][2]      # same Bi and keys, another MAC
    ge_p = next(op for op in K.corpus() if "rawxi:ge_p" in op.tags)
    assert int.from_bytes(ge_p.xi, "big") >= ge_p.p
    big = next(op for op in K.corpus() if "ni:bi_ge_p" in op.tags)
    assert big.v >= big.p and exp[big][2] != R.process_bi(big.v % big.p, big.xi, big.b, big.salt, big.p)      # (the MAC sees the bytes as given)


# ---- the library ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _native.load_library()


def test_entries_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "bftkv_gpu.h")).read()
    declared = set(re.findall(r"\b(bftkv_gpu_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _native.EXPORTS and hasattr(lib, name), name
    from bftkv_amd import Batcher, Context
    assert all(hasattr(Context, n) for n in ("tpa_yi", "tpa_bi", "tpa_ni")) and all(hasattr(Batcher, n) for n in ("tpa_yi", "tpa_bi"))


@pytest.mark.parametrize("entry", ["yi", "bi", "ni"])
def test_null_context_is_refused_and_fails_closed(lib, entry):
    """No device is needed: the refusal comes before anything touches one.  The arrays go in dirty and come back failed and zero."""
    n, nb, el, sl = 3, 256, 32, 16
    a = lambda *shape: np.full(shape, 0xA5, dtype=np.uint8)      # noqa: E731
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))         # noqa: E731
    base, xi, e, salt, mods = a(n, nb), a(n, nb), a(n, el), a(n, sl), np.frombuffer(R.P.to_bytes(nb, "big"), dtype=np.uint8).copy()
    xl = np.full(n, 7, dtype=np.uint32)
    num, keys, mac, st = a(n, nb), a(n, 32), a(n, 32), np.zeros(n, dtype=np.uint8)
    if entry == "yi":
        rc = lib.bftkv_gpu_tpa_yi(None, n, p(base), nb, p(e), el, None, 1, p(mods), p(num), p(st))
        outs = [num]
    elif entry == "bi":
        rc = lib.bftkv_gpu_tpa_bi(None, n, p(base), p(xi), xl.ctypes.data, nb, p(e), el, p(salt), sl, None, 1, p(mods), p(num), p(keys), p(mac), p(st))
        outs = [num, keys, mac]
    else:
        rc = lib.bftkv_gpu_tpa_ni(None, n, p(base), p(xi), xl.ctypes.data, nb, p(e), el, p(salt), sl, None, 1, p(mods), p(keys), p(mac), p(st))
        outs = [keys, mac]
    assert rc == E_INVALID
    assert (st == FAILED).all() and all(not o.any() for o in outs)
