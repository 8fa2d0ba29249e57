"""CPU: the restatement of RSA signing (tests/rsa_sign_ref.py) agrees with plain exponentiation, the known-answer signature and the
verifier's restatement; the corpus (tests/rsa_sign_cases.py) holds every class it promises; the model of mont_mul carries the 10 x 4
form at the operands the kernel produces; the rules of bftkv_amd/csrc/rsa_sign.h compiled for the host agree with the restatement; and
the library exports the entries, which refuse a NULL context before they need a device, failing closed."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import mont_model as M
import rsa_sign_cases as K
import rsa_sign_ref as R
import rsa_verify_ref as V
from bftkv_amd import _native
from corpus import keys as CK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bftkv_gpu_rsa_signer_create", "bftkv_gpu_rsa_signer_destroy", "bftkv_gpu_rsa_signer_info", "bftkv_gpu_rsa_sign_keyset",
         "bftkv_gpu_rsa_sign_keyset_dev", "bftkv_gpu_selftest_rsa_crt", "bftkv_gpu_batcher_rsa_sign_keyset"]
E_INVALID = -1


def _flat():
    """(tag, key, hash_id, digest, (status, signature bytes)) of every signature of the corpus"""
    ks = K.keys()
    for h, dl in K.SHAPES:
        for d, i, exp in zip(*K.call(h, dl), K.expected(h, dl)):
            yield ks[i][0], ks[i][1], h, d, exp


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_consistent_keys_sign_as_the_plain_exponentiation_does():
    seen = 0
    for tag, k, h, d, (st, sig) in _flat():
        if ":" in tag or st != R.OK:
            continue
        em = int.from_bytes(V.em(R.kbytes(k.n), h, d), "big")
        dd = pow(k.e, -1, (k.p - 1) * (k.q - 1))
        assert int.from_bytes(sig, "big") == pow(em, dd, k.n), (tag, h)
        seen += 1
    assert seen > 200


def test_the_known_answer_signature():
    k = K.kat()
    key = dict(K.keys())["kat"]
    assert key.p * key.q == k["n"] and key.p > key.q > 1
    assert R.sign(key, 8, hashlib.sha256(k["tbs"]).digest(), 256) == (R.OK, k["sig"])


def test_the_verifier_accepts_every_signature_and_no_flipped_one():
    rng = random.Random(11)
    seen = 0
    for tag, k, h, d, (st, sig) in _flat():
        if st != R.OK:
            assert not any(sig)
            continue
        s = int.from_bytes(sig, "big")
        assert V.verify(k.n, k.e, h, d, s) == (1, V.OK), (tag, h)
        assert V.verify(k.n, k.e, h, d, s ^ 1 << rng.randrange(k.n.bit_length() - 1))[0] == 0, (tag, h)
        seen += 1
    assert seen > 200


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------
def test_corpus_keys():
    ks = dict(K.keys())
    assert [ks["rsa%d" % b].n.bit_length() for b in K.SIZES] == list(K.SIZES) == [128, 496, 1024, 2047, 2048]
    u = ks["unbalanced"]
    assert (u.p.bit_length(), u.q.bit_length()) == (1024, 520)
    rng = CK.DRBG("primality")
    for p in K.FULL_PRIMES + K.SPARSE_PRIMES:
        assert CK.is_probable_prime(p, rng)
    assert all(M.to_limbs(p, 40)[1:36] == [M.MASK] * 35 for p in K.FULL_PRIMES) and all(sum(1 for v in M.to_limbs(p, 40) if v) == 2 for p in K.SPARSE_PRIMES)
    assert (ks["full"].p, ks["full"].q) == K.FULL_PRIMES and (ks["sparse"].p, ks["sparse"].q) == K.SPARSE_PRIMES
    for tag, k in K.keys():
        assert k.n < 1 << (8 * K.NBYTES) and all(v < 1 << (8 * K.PBYTES) for v in (k.p, k.q, k.dp, k.dq, k.qinv)), tag
        if ":" not in tag:
            assert k.p * k.q == k.n and k.qinv * k.q % k.p == 1 and not R.key_refused(k), tag
    for kind in K.REFUSED_KINDS:
        got = [k for t, k in K.keys() if t.startswith("refused:%s:" % kind)]
        assert len(got) >= 2 and all(R.key_refused(k) for k in got), kind
    assert any(k.n % 2 == 0 for t, k in K.keys()) and any(k.p % 2 == 0 for t, k in K.keys()) and any(k.q % 2 == 0 for t, k in K.keys())
    assert any(k.p == 1 for t, k in K.keys())
    for kind in K.BROKEN_KINDS:
        got = [k for t, k in K.keys() if t.startswith("broken:%s:" % kind)]
        assert len(got) >= 2 and not any(R.key_refused(k) for k in got), kind


def test_corpus_holds_every_class():
    assert {h for h, _ in K.SHAPES} == {0, 1, 2, 3, 8, 9, 10, 11}
    cells = {}
    for tag, k, h, d, (st, sig) in _flat():
        cells.setdefault((tag, h, len(d)), set()).add(st)
        assert (st == R.OK) == any(sig)
    # the length rule: 496 bits under SHA-384 / SHA-512, 128 bits under everything but hash_id 0 with dlen <= 5
    assert cells[("rsa496", 9, 48)] == cells[("rsa496", 10, 64)] == {R.INVALID_INPUT} and cells[("rsa496", 8, 32)] == {R.OK}
    for h, dl in K.SHAPES:
        assert cells[("rsa128", h, dl)] == ({R.OK} if (h, dl) == (0, 5) else {R.INVALID_INPUT}), (h, dl)
        for tag in ("rsa1024", "rsa2047", "rsa2048", "unbalanced", "kat", "full", "sparse"):
            assert cells[(tag, h, dl)] == {R.OK}, (tag, h)
        # every broken key fails the check and nothing else
        for tag, _ in K.keys():
            if tag.startswith("broken:"):
                assert cells[(tag, h, dl)] == {R.CHECK_FAILED}, (tag, h)
            if tag.startswith("refused:") and tag.endswith("rsa2048"):
                assert cells[(tag, h, dl)] == {R.FENCED}, (tag, h)
    # each refused kind is hit once by a signature the length rule also catches: the length rule wins
    for kind in K.REFUSED_KINDS:
        tag = "refused:%s:rsa496" % kind
        assert cells[(tag, 10, 64)] == {R.INVALID_INPUT} and cells[(tag, 8, 32)] == {R.FENCED}, kind


def test_corpus_selftest_operands():
    ops, exp = K.selftest_ops(), K.selftest_expected()
    ks = K.keys()
    classes = {}
    for (i, cls, c), (st, s) in zip(ops, exp):
        k = ks[i][1]
        assert st == R.OK and 0 <= c < 1 << (8 * K.NBYTES) and s < k.n
        m1, m2 = pow(c % k.p, k.dp, k.p), pow(c % k.q, k.dq, k.q)
        assert s % k.p == m1 and s % k.q == m2 and s == pow(c, pow(k.e, -1, (k.p - 1) * (k.q - 1)), k.n)
        classes.setdefault(ks[i][0], {})[cls] = (c, m1, m2)
    for tag, by in classes.items():
        k = dict(ks)[tag]
        assert {"zero", "one", "p", "q", "n-1", "n", "all_ones", "m1<m2", "m1=m2", "diff+1", "diff-1", "0 mod p only", "0 mod q only", "wide"} == set(by), tag
        assert by["m1<m2"][1] < by["m1<m2"][2] and by["m1=m2"][1] == by["m1=m2"][2] > 1
        assert (by["diff+1"][1] - by["diff+1"][2]) % k.p == 1 and (by["diff-1"][1] - by["diff-1"][2]) % k.p == k.p - 1
        assert by["0 mod p only"][1] == 0 != by["0 mod p only"][2] and by["0 mod q only"][2] == 0 != by["0 mod q only"][1]
        assert by["p"][0] == k.p and by["q"][0] == k.q and by["all_ones"][0] == (1 << 2048) - 1 and by["wide"][0] > k.n
    assert set(classes) == {t for _, t, _ in K.good_keys()} and {"full", "sparse", "unbalanced"} <= set(classes)


# ---- the model of mont_mul on the 10 x 4 form ---------------------------------------------------------------------------------------------
def _primes():
    return sorted({m for _, _, k in K.good_keys() for m in (k.p, k.q)})


@pytest.mark.parametrize("mut", [(), (M.BOUND_M,)], ids=["plain", "factor_at_maximum"])
def test_model_carries_the_ten_by_four_form(mut):
    """The operands k_rsas_crt produces: the base below 4m into the first squaring and as the broadcast operand of the table's
    products, everything else below 2m; the base's two products take any 1120-bit half against R^2 and R^3 mod m.  Results must be
    right (with the factor forced to its maximum the rows are no Montgomery reduction: only the columns are looked at) and no column
    reaches 2^64 -- a condition, not a tolerance."""
    L, TPI, N = 10, 4, 40
    Rr = 1 << (28 * N)
    st = M.Stats()
    rng = random.Random(40)
    for m in _primes():
        n0 = M.n0inv_of(m)
        nl = M.to_limbs(m, N)
        pairs = [(4 * m - 1, 4 * m - 1, True), (2 * m - 1, 2 * m - 1, True), (4 * m - 1, 2 * m - 1, False), (2 * m - 1, 2 * m - 1, False),
                 (Rr - 1, m - 1, False), (Rr - 1, Rr * Rr % m, False), ((1 << 928) - 1, Rr * Rr * Rr % m, False), (1, 2 * m - 1, False), (0, 0, True)]
        pairs += [(x, x, True) for x in (rng.randrange(2 * m) for _ in range(3))] + [(rng.randrange(4 * m), rng.randrange(2 * m), False) for _ in range(3)]
        for a, b, sqr in pairs:
            out = M.mont_mul(M.to_limbs(a, N), M.to_limbs(b, N), nl, n0, L, TPI, sqr, st, mut)
            if not mut:
                v = M.from_limbs(out)
                assert v % m == a * b * pow(Rr, -1, m) % m and v < 2 * m and max(out) <= 1 << 28, (m.bit_length(), a.bit_length(), sqr)
    assert 0 < st.max_col < 1 << 64
    if not mut:
        assert st.max_col < 1 << 62       # 20 products of at most 2^57 and a carry


# ---- rsa_sign.h on the host ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rsas_host") / "rsa_sign_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "c", "rsa_sign_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-300:], r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in ln.split()] for ln in out]
    return run


def test_the_header_gives_the_restatements_rule_and_em(host):
    rows = [(k, h, d) for _, k, h, d, _ in _flat()]
    got = host(["E %d %s %d %s %d" % (K.NBYTES, k.n.to_bytes(K.NBYTES, "big").hex(), h, d.hex(), R.key_refused(k)) for k, h, d in rows])
    for (k, h, d), g in zip(rows, got):
        by_len, limbs = R.em_limbs(k.n, h, d)
        assert g[0] == R.rule(k, h, len(d)) and g[1:] == limbs and (by_len == R.OK or g[0] == R.INVALID_INPUT), (k.n.bit_length(), h)
    # rows of exactly k bytes, and n = 0 and n = 1
    for n, nb in ((K.keys()[1][1].n, 62), (0, 1), (1, 1), (0, 256), (1, 256)):
        g = host(["E %d %s 0 %s 0" % (nb, n.to_bytes(nb, "big").hex(), "0102")])[0]
        assert g[0] == (R.OK if n > 1 else R.INVALID_INPUT) and g[1:] == R.em_limbs(n, 0, b"\1\2")[1]


def test_the_header_gives_the_restatements_values_digits_refusals_and_statuses(host):
    rng = random.Random(3)
    vals = [(c, K.NBYTES) for _, _, c in K.selftest_ops()] + [(rng.getrandbits(8 * nb), nb) for nb in (1, 2, 3, 4, 5, 16, 139, 140, 141, 255, 256) for _ in range(4)]
    for (v, nb), g in zip(vals, host(["V %d %s" % (nb, v.to_bytes(nb, "big").hex()) for v, nb in vals])):
        assert g == R.value_limbs(v), nb
    exps = [(d, K.PBYTES) for _, k in K.keys() for d in (k.dp, k.dq)] + [(rng.getrandbits(8 * pb), pb) for pb in (1, 2, 8, 65, 128)] + [(0, 1), (0xF0, 1), (0x0F, 1)]
    for (d, pb), g in zip(exps, host(["D %d %s" % (pb, d.to_bytes(pb, "big").hex()) for d, pb in exps])):
        assert g == R.digits(d, pb) and len(g) == 2 * pb
    ks = [k for _, k in K.keys()] + [R.Key(15, 3, p, q, 1, 1, 1) for p in (0, 1, 2, 3, 5) for q in (0, 1, 2, 3, 5)]
    hexrow = lambda v, w: v.to_bytes(w, "big").hex()                 # noqa: E731
    got = host(["R %d %s %d %s %s" % (K.NBYTES, hexrow(k.n, K.NBYTES), K.PBYTES, hexrow(k.p, K.PBYTES), hexrow(k.q, K.PBYTES)) for k in ks])
    assert [g[0] for g in got] == [int(R.key_refused(k)) for k in ks] and {g[0] for g in got} == {0, 1}
    got1 = host(["R 1 0f 1 %02x %02x" % (k.p, k.q) for k in ks[-25:]])
    assert [g[0] for g in got1] == [int(R.key_refused(k)) for k in ks[-25:]]
    combos = [(r, f, c) for r in (R.OK, R.FENCED, R.INVALID_INPUT) for f in (0, 1) for c in (0, 1)]
    assert [g[0] for g in host(["S %d %d %d" % x for x in combos])] == [R.status(*x) for x in combos]


# ---- the library --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _native.load_library()


def test_entries_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "bftkv_gpu.h")).read()
    declared = set(re.findall(r"\b(bftkv_gpu_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _native.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define\s+BFTKV_TH_CHECK_FAILED\s+4\b", hdr) and re.search(r"#define\s+BFTKV_RSA_SIGN_LAUNCH\s+16384u\b", hdr)
    from bftkv_amd import Batcher, Context
    for m in ("rsa_signer_create", "rsa_signer_destroy", "rsa_signer_info", "rsa_sign_keyset", "selftest_rsa_crt"):
        assert hasattr(Context, m), m
    assert hasattr(Batcher, "rsa_sign_keyset")


def test_null_context_and_null_batcher_are_refused_and_fail_closed(lib):
    """No device is needed: the refusal comes before anything touches one.  The statuses go in dirty and come back failed; a row's
    width is the set's, which nobody can ask without a context, so the rows are left alone -- and the handle comes back as -1."""
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))             # noqa: E731
    n = 3
    dg, ki = np.full((n, 32), 0x11, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    for entry in ("sign", "selftest"):
        out, st = np.full((n, 256), 0xA5, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        if entry == "sign":
            rc = lib.bftkv_gpu_rsa_sign_keyset(None, 0, n, p(dg), 8, 32, ki.ctypes.data, p(out), p(st))
        else:
            rc = lib.bftkv_gpu_selftest_rsa_crt(None, 0, n, p(out), ki.ctypes.data, p(out), p(st))
        assert rc == E_INVALID and (st == R.FAILED).all() and (out == 0xA5).all(), entry
    # the device form touches nothing: its arrays are not the host's to write
    assert lib.bftkv_gpu_rsa_sign_keyset_dev(None, 0, n, None, 8, 32, None, None, None) == E_INVALID
    st1, sig = np.zeros(1, dtype=np.uint8), np.full(256, 0xA5, dtype=np.uint8)
    assert lib.bftkv_gpu_batcher_rsa_sign_keyset(None, 0, 0, p(dg), 32, 8, p(sig), p(st1)) == E_INVALID and st1[0] == R.FAILED
    row = np.full((1, 128), 3, dtype=np.uint8)
    nn, e, h = np.full((1, 256), 0xFF, dtype=np.uint8), np.array([65537], dtype=np.uint32), C.c_int(7)
    assert lib.bftkv_gpu_rsa_signer_create(None, 1, p(nn), e.ctypes.data, 256, p(row), p(row), p(row), p(row), p(row), 128, C.byref(h)) == E_INVALID
    assert h.value == -1
    v = C.c_uint32(9)
    assert lib.bftkv_gpu_rsa_signer_info(None, 0, C.byref(v), None, None, None) == E_INVALID and v.value == 9
    assert lib.bftkv_gpu_rsa_signer_destroy(None, 0) == E_INVALID
