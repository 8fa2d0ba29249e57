"""CPU: the restatement of threshold RSA signing (tests/rsa_psign_ref.py) closes the loop over the known-answer key, the rules of
bftkv_amd/csrc/rsa_psign.h compiled for the host agree with it, the corpus (tests/rsa_psign_cases.py) holds every class it promises,
and the library exports the entries, which refuse a NULL context before they need a device, failing closed."""
import ctypes as C
import functools
import hashlib
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import rsa_psign_cases as K
import rsa_psign_ref as R
import rsa_verify_ref as V
from bftkv_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bftkv_gpu_rsa_partial_sign", "bftkv_gpu_batcher_rsa_partial_sign"]
E_INVALID = -1


# ---- the restatement over the known-answer key --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _answer(srv, kid):
    di = K.tree()[srv].get(kid)
    if di is None:
        return None
    sb, mag = R.stored(di)
    st, ci = R.sign(K.tree_t(), K.kat()["n"], [(sb, int.from_bytes(mag, "big"))])[0]
    assert st == R.OK
    return ci


def test_the_tree_is_the_one_the_issue_describes():
    """n = 4, k = 2: every server holds ten fragments, of 512, 1023/1024 and 2045-2047 bytes, about half of them negative"""
    fr = K.tree_fragments()
    assert len(fr) == 40 and [sum(1 for f in fr if f[0] == s) for s in range(4)] == [10] * 4
    assert {len(f[3]) for f in fr} <= {512, 1023, 1024, 2045, 2046, 2047} and {512, 1024, 2047} <= {len(f[3]) for f in fr}
    assert 10 <= sum(f[2] for f in fr) <= 30 and {f[2] for f in fr} == {0, 1}
    for srv in range(4):                                             # depths 1, 2, 3: one, three and six fragments
        assert sorted(R.depth(kid * 4 + srv + 1, 4) for kid in K.tree()[srv]) == [1] + [2] * 3 + [3] * 6


@pytest.mark.parametrize("live", K.LIVE_SETS, ids=str)
def test_live_sets_give_the_fixture_signature(live):
    k = K.kat()
    factors = R.client_factors(K.TREE_N, K.TREE_K, live, _answer)
    assert factors is not None and R.fold(factors, k["n"]) == k["sig"]
    assert len(factors) == (4 if len(live) == 4 else 10)
    digest = hashlib.sha256(k["tbs"]).digest()
    assert V.verify(k["n"], k["e"], 8, digest, R.fold(factors, k["n"])) == (1, V.OK)      # rsa_verify_ref accepts what the restatement signs
    assert V.verify(k["n"], k["e"], 8, digest, R.fold(factors[:-1], k["n"]))[0] == 0


def test_one_server_of_four_gives_no_signature():
    assert R.client_factors(K.TREE_N, K.TREE_K, (1,), _answer) is None


def test_em_is_below_the_modulus_and_the_base_may_be_inverted_instead_of_the_power():
    rng = random.Random(5)
    for bits in (17, 24, 25, 520, 1023, 1024, 2041, 2048):
        for _ in range(20):
            n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
            t = bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, max(1, R.emlen(n) - 2))))
            m = R.emsa_encode(t, n)
            assert m is not None and m < n
            mag = rng.getrandbits(40) | 1
            if math.gcd(m, n) == 1:
                assert pow(pow(m, -1, n), mag, n) == pow(pow(m, mag, n), -1, n)
            else:
                assert math.gcd(pow(m, mag, n), n) != 1


# ---- rsa_psign.h on the host ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("psign_host") / "rsa_psign_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "c", "rsa_psign_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-300:], r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in ln.split()] for ln in out]
    return run


def _grid():
    """(modulus, row width, T): emlen 1, 2, 3, 53-56, 255, 256 against T of 0, 1, 35, 51, 83 and nbytes bytes, and every emlen - len(T)
    from 0 to 5; N = 0 and N = 1; rows of exactly emlen bytes and of 256"""
    rng = random.Random(0xE3)
    cases = [(0, 1, b""), (0, 256, b"\1\2\3"), (1, 1, b""), (1, 256, b"")]
    for el in (1, 2, 3, 53, 54, 55, 56, 255, 256):
        for top_bits in (1, 5, 8):
            n = rng.getrandbits(8 * el) >> (8 - top_bits) | 1 << (8 * (el - 1) + top_bits - 1) | 1
            assert R.emlen(n) == el
            lens = {0, 1, 35, 51, 83} | {el - d for d in range(6) if el - d >= 0}
            for nbytes in {el, 256}:
                for tl in sorted(lens | {nbytes}):
                    if tl <= nbytes:
                        for fill in (None, 0x00, 0xFF):
                            t = bytes(rng.getrandbits(8) for _ in range(tl)) if fill is None else bytes([fill]) * tl
                            cases.append((n, nbytes, t))
    return cases


def test_the_header_gives_the_restatements_em_and_refusal(host):
    cases = _grid()
    got = host(["E %d %s %s" % (nb, n.to_bytes(nb, "big").hex(), t.hex() or "-") for n, nb, t in cases])
    deltas = set()
    for (n, nb, t), g in zip(cases, got):
        limbs, refusal = R.em_limbs(t, n)
        assert g[0] == R.emlen(n) and g[1] == refusal and g[2:] == limbs, (n.bit_length(), nb, len(t))
        deltas.add((R.emlen(n) - len(t), refusal))
    assert {(d, R.INVALID_INPUT if d < 3 else R.OK) for d in range(6)} <= deltas and len(cases) > 600
    assert any(refusal == R.OK and R.emlen(n) - len(t) == 3 and R.emlen(n) == 256 for (n, _, t), (_, refusal, *_) in zip(cases, got))


def test_the_header_gives_the_restatements_sign_and_status(host):
    rows = [(sb, z, ref, ni) for sb in (0, 1, 2, 0x80, 0xFF) for z in (0, 1) for ref in (0, 1) for ni in (0, 1)]
    got = host(["S %d %d %d %d" % r for r in rows])
    for (sb, z, ref, ni), (neg, st) in zip(rows, got):
        assert neg == (1 if R.fragment(sb, 0 if z else 7) < 0 else 0), (sb, z)
        assert st == (R.INVALID_INPUT if ref else R.NO_INVERSE if neg and ni else R.OK), (sb, z, ref, ni)


# ---- the corpus: every row of the table and every boundary, nothing skipped ------------------------------------------------------------------
def _flat():
    """(call, request, fragment, (status, ci)) of every fragment of the corpus"""
    for ci, call in enumerate(K.calls()):
        exp = iter(K.expected(ci))
        for r in call.reqs:
            for f in r.frags:
                yield call, r, f, next(exp)
        assert next(exp, None) is None


def test_corpus_shapes_and_moduli():
    calls = K.calls()
    assert {(c.nbytes, c.exp_len) for c in calls} == {(nb, el) for nb in (256, 128) for el in K.EXP_LENS} | {(256, K.BIG_EXP_LEN)}
    big = [c for c in calls if c.exp_len == K.BIG_EXP_LEN]
    assert len(big) == 1 and sum(len(r.frags) for r in big[0].reqs) == 8
    m = K.moduli()
    assert m["kat2048"] == K.kat()["n"] and m["one"] == 1 and m["three"] == 3
    assert {v.bit_length() for v in m.values()} >= {2048, 2041, 2040, 1024, 1023, 520} and {R.emlen(v) for v in m.values()} >= {3, 53, 54, 55, 255, 256}
    for c in calls:
        assert all(f.mag < 1 << (8 * f.used) and f.used <= c.exp_len for r in c.reqs for f in r.frags), c.name
        if c.exp_len == K.BIG_EXP_LEN:
            continue
        tags = set().union(*(r.tags for r in c.reqs))
        assert {"mod:" + k for k, v in m.items() if R.emlen(v) <= c.nbytes} <= tags, c.name
        assert {t for t, _ in K.t_classes(c.nbytes)} <= tags and len({t for t, _ in K.t_classes(c.nbytes)}) == 12, c.name
        assert any(len(r.t) == c.nbytes for r in c.reqs) and any(r.t == b"" for r in c.reqs)
        assert all(r.n & 1 and R.emlen(r.n) <= c.nbytes and len(r.t) <= c.nbytes and r.frags for r in c.reqs)
    assert {"mod:kat2048", "mod:odd2041", "mod:odd2040"} <= set().union(*(r.tags for r in calls[0].reqs))


def test_corpus_holds_every_row_of_the_table():
    rows = {}
    for call, r, f, (st, ci) in _flat():
        neg = f.sign != 0 and f.mag != 0
        row = "refused" if st == R.INVALID_INPUT else "no_inverse" if st == R.NO_INVERSE else "inverse" if neg else "zero_under_sign" if f.sign and not f.mag else "power"
        rows.setdefault(call.name, set()).add(row)
        m = R.emsa_encode(r.t, r.n)
        if row == "refused":
            assert m is None and ci == 0
        elif row == "no_inverse":
            assert math.gcd(m, r.n) != 1 and ci == 0 and "noinv:bad" in r.tags
        elif row == "inverse":
            assert 0 < ci < r.n and (f.used > 5 or ci * pow(m, f.mag, r.n) % r.n == 1)      # (the long powers were raised once, by expected())
        elif row == "zero_under_sign":
            assert ci == 1
        else:
            assert 0 < ci < r.n and (f.used > 5 or ci == pow(m, f.mag, r.n))
    for c in K.calls():
        want = {"refused", "inverse", "zero_under_sign", "power"} | ({"no_inverse"} if c.nbytes == 256 else set())
        assert rows[c.name] == (want if c.exp_len != K.BIG_EXP_LEN else {"inverse", "power"}), c.name


def test_corpus_padding_boundaries():
    """emlen - len(T) of 2, 3 and 4 under the tiny moduli (refused, no FF at all, one FF) and 255 bytes of em in a 256-byte row"""
    for c in K.calls():
        if c.exp_len == K.BIG_EXP_LEN:
            continue
        pad = {R.emlen(r.n) - len(r.t) for r in c.reqs if any(t.startswith("mod:tiny") for t in r.tags)}
        assert {2, 3, 4} <= pad and {0, -1} & pad or min(pad) < 0, c.name
        em3 = [r for r in c.reqs if R.emlen(r.n) - len(r.t) == 3]
        assert em3 and all(R.emsa_encode(r.t, r.n) >> (8 * len(r.t)) == 1 << 8 for r in em3)      # 00 01 00 | T
        if c.nbytes == 256:
            assert any(R.emlen(r.n) == 255 and R.emsa_encode(r.t, r.n) is not None for r in c.reqs)
        assert any(r.n == 1 for r in c.reqs) and any(r.n == 3 for r in c.reqs)
        assert all(R.emsa_encode(r.t, r.n) is None for r in c.reqs if r.n in (1, 3))


def test_corpus_sign_bytes_and_magnitudes():
    for c in K.calls():
        if c.exp_len == K.BIG_EXP_LEN:
            continue
        frags = [f for r in c.reqs for f in r.frags]
        assert {(f.cls, f.sign) for f in frags} >= {(cls, sb) for cls in K.MAG_CLASSES for sb in K.SIGN_BYTES}, c.name
        live = [f for r in c.reqs if R.emsa_encode(r.t, r.n) is not None for f in r.frags]
        assert {(f.cls, f.sign != 0) for f in live} >= {(cls, s) for cls in K.MAG_CLASSES for s in (False, True)}, c.name
        digits = lambda f: [(f.mag >> (4 * i)) & 15 for i in range(2 * f.used)]      # noqa: E731
        assert any(f.cls == "all15" and set(digits(f)) == {15} for f in frags)
        assert any(f.cls == "low_digit" and f.mag < 16 for f in frags) and any(f.cls == "top_digit" and sum(1 for d in digits(f) if d) == 1 for f in frags)
        if c.exp_len >= 3:
            assert any(f.cls == "zero_run" and digits(f)[len(digits(f)) // 3:2 * len(digits(f)) // 3] == [0] * (2 * len(digits(f)) // 3 - len(digits(f)) // 3)
                       and digits(f)[0] and digits(f)[-1] for f in frags), c.name
        used = {("zero" if f.used == 0 else "row" if f.used == c.exp_len else "short") for f in frags}
        assert used == ({"zero", "row", "short"} if c.exp_len > 1 else {"zero", "row"}), c.name
        assert any(f.used > (f.mag.bit_length() + 7) // 8 for f in frags) and any(f.used == (f.mag.bit_length() + 7) // 8 for f in frags if f.mag)


def test_corpus_no_inverse_case():
    n3, t_bad, t_good = K.no_inverse_case()
    assert n3 % 3 == 0 and n3 & 1 and t_bad[:-1] == t_good[:-1] and R.emsa_encode(t_bad, n3) % 3 == 0 and math.gcd(R.emsa_encode(t_good, n3), n3) == 1
    seen = 0
    for ci, c in enumerate(K.calls()):
        if c.nbytes != 256 or c.exp_len == K.BIG_EXP_LEN:
            continue
        exp, at = K.expected(ci), 0
        for r in c.reqs:
            st = [s for s, _ in exp[at:at + len(r.frags)]]
            at += len(r.frags)
            if "noinv:bad" in r.tags:
                assert st == [R.NO_INVERSE if f.sign and f.mag else R.OK for f in r.frags] and R.NO_INVERSE in st and R.OK in st
                seen += 1
            elif "noinv:good" in r.tags:
                assert st == [R.OK] * len(r.frags) and any(f.sign and f.mag for f in r.frags)
                seen += 1
    assert seen == 2 * len(K.EXP_LENS)


def test_call_arrays_are_what_the_entry_takes():
    c = K.calls()[0]
    a = K.call_arrays(c)
    n_frags = sum(len(r.frags) for r in c.reqs)
    assert a["exps"].shape == (n_frags, c.exp_len) and a["mods"].shape[1] == c.nbytes and len(a["t_len"]) == len(c.reqs) == len(a["mod_idx"])
    assert a["t"].shape == (len(c.reqs), c.nbytes) and (a["t"][0, int(a["t_len"][0]):] == 0xEE).all()
    for j in range(n_frags):                                          # zeroes ahead of the last exp_used bytes
        assert not a["exps"][j, :c.exp_len - int(a["exp_used"][j])].any()


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _native.load_library()


def test_entries_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "bftkv_gpu.h")).read()
    declared = set(re.findall(r"\b(bftkv_gpu_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _native.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define\s+BFTKV_TH_INVALID_INPUT\s+3\b", hdr)
    from bftkv_amd import Batcher, Context
    assert hasattr(Context, "rsa_partial_sign") and hasattr(Batcher, "rsa_partial_sign")


def test_null_context_and_null_batcher_are_refused_and_fail_closed(lib):
    """No device is needed: the refusal comes before anything touches one.  The arrays go in dirty and come back failed and zero."""
    n_frags, nb, el = 3, 256, 8
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))             # noqa: E731
    t, tl = np.full((1, 51), 0x11, dtype=np.uint8), np.array([51], dtype=np.uint32)
    mods = np.frombuffer(K.kat()["n"].to_bytes(nb, "big"), dtype=np.uint8).copy()
    exps, sign = np.full((n_frags, el), 0x33, dtype=np.uint8), np.array([0, 1, 2], dtype=np.uint8)
    for batcher in (False, True):
        out, st = np.full((n_frags, nb), 0xA5, dtype=np.uint8), np.zeros(n_frags, dtype=np.uint8)
        if batcher:
            rc = lib.bftkv_gpu_batcher_rsa_partial_sign(None, p(t), 51, p(mods), nb, n_frags, p(exps), el, None, p(sign), p(out), p(st))
        else:
            rc = lib.bftkv_gpu_rsa_partial_sign(None, 1, p(t), 51, tl.ctypes.data, None, 1, p(mods), nb, n_frags, None, p(exps), el, None, p(sign), p(out), p(st))
        assert rc == E_INVALID and (st == R.FAILED).all() and not out.any(), batcher
