"""CPU: the restatement of threshold DSA / ECDSA signing (tests/tsig_share_ref.py) closes the loop -- what the servers' share answers
add up to verifies under the DSA and ECDSA verification restatements -- the rules of bftkv_amd/csrc/tsig_share.h and the fixed-schedule
walk fb_mul_fixed of ec_field.h compiled for the host agree with it, and the library exports the entries, which refuse a NULL context
before they need a device, failing closed."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import dsa_verify_ref as DV
import ec_ref as E
import ecdsa_verify_ref as EV
import tsig_share_cases as K
import tsig_share_ref as R
from bftkv_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bftkv_gpu_tdsa_share", "bftkv_gpu_tdsa_share_dev", "bftkv_gpu_tecdsa_share", "bftkv_gpu_tecdsa_share_dev", "bftkv_gpu_tsig_partial_s",
         "bftkv_gpu_batcher_tdsa_share", "bftkv_gpu_batcher_tecdsa_share"]
E_INVALID = -1
CONFIGS = [(4, 2, 4), (7, 3, 6)]      # (n, t, responders): everyone of four; exactly 2t of seven


def _groups():
    out = [(name, R.dsa_group(g.p, g.q, g.g), g) for name, g in K.dsa_groups().items()]
    return out + [(name, R.ec_group(c), c) for name, c in K.curves().items()]


def _verifies(name, G, raw, x, digest, sig):
    if G.kind == "dsa":
        qb = len(sig) // 2
        r, s = int.from_bytes(sig[:qb], "big"), int.from_bytes(sig[qb:], "big")
        return DV.verify(raw.p, raw.q, raw.g, pow(raw.g, x, raw.p), digest, r, s) == (1, DV.OK)
    key = E.marshal(raw, *E.scalar_base_mult(raw, x))
    f = E.byte_len(raw)
    r, s = int.from_bytes(sig[:len(sig) // 2], "big"), int.from_bytes(sig[len(sig) // 2:], "big")
    return EV.verify(raw, key, digest, r.to_bytes(f, "big") + s.to_bytes(f, "big")) == (1, EV.OK)


# ---- the loop closes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,m", CONFIGS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(K.DSA_NAMES) + E.NAMES)
def test_the_share_answers_add_up_to_a_signature_that_verifies(name, n, t, m):
    gname, G, raw = next(g for g in _groups() if g[0] == name)
    rng = random.Random("%s/%d/%d" % (name, n, t))
    q = G.q
    x = rng.randrange(1, q)
    digest = bytes(rng.getrandbits(8) for _ in range((q.bit_length()) // 8))      # whole bytes, at most the order's length
    responders = sorted(rng.sample(range(n), m))
    assert m == 2 * t
    run = R.sign(G, n, t, responders, x, digest, rng)
    assert run.r and run.s and _verifies(name, G, raw, x, digest, run.sig)
    # r is the r of the nonce k^-1, for the k the shares add up to
    kinv = pow(run.k_total, -1, q)
    if G.kind == "dsa":
        assert run.r == pow(raw.g, kinv, raw.p) % q
    else:
        assert run.r == E.scalar_base_mult(raw, kinv)[0] % q
    assert run.s == run.k_total * (G.os2i(digest) + x * run.r) % q
    # one responder short: the zero polynomials of degree 2t - 1 do not cancel, and nothing verifies
    short = R.sign(G, n, t, responders[:-1], x, digest, random.Random("short/" + name))
    assert not _verifies(name, G, raw, x, digest, short.sig)


def test_fold_is_one_mod_per_addition_and_wraps():
    q = K.dsa_groups()["dsa1024"].q
    for m in (1, 2, 4, 7):
        assert R.fold([(q - 1,) * 4] * m, q) == ((m * (q - 1)) % q,) * 4 == ((q - m) % q,) * 4
    assert R.fold([(q, q + 1, 2 * q, 0)], q) == (0, 1, 0, 0)
    assert R.phase3(q, q - 1, q - 1, q - 1, q - 1, q - 1) == ((((q - 1) ** 2 % q + q - 1) % q) * (q - 1) + q - 1) % q


# ---- tsig_share.h and fb_mul_fixed on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tsig_host") / "tsig_share_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "tsig_share_host.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-300:], r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return [ln.split() for ln in out]
    return run


def _moduli():
    """(L, width, q): the DSA orders in their own and in 32-byte rows, the curves' N, and tiny ones"""
    out = []
    for g in K.dsa_groups().values():
        out += [(8, DK_nbytes(g.q), g.q), (8, 32, g.q)]
    out += [({28: 7, 32: 8, 48: 12, 66: 17}[E.byte_len(c)], E.byte_len(c), c["n"]) for c in K.curves().values()]
    return out + [(8, 1, 1), (8, 1, 3), (8, 4, 0xFFFFFFFB), (17, 66, 3), (7, 28, (1 << 224) - 63)]


def DK_nbytes(v):
    return max(1, (v.bit_length() + 7) // 8)


def test_the_header_gives_the_restatements_fold_and_vi(host):
    lines, want, labels = [], [], set()
    for L, width, q in _moduli():
        for m in (1, 2, 4, 7):
            w = 8 if q.bit_length() > 8 else 4
            for label, sh in K.requests(q, width, m, w, K.windows_of(q, w), seed=m):
                if q <= 3 and not label.startswith("s:"):
                    continue
                hexes = "".join(v.to_bytes(width, "big").hex() for tup in sh for v in tup)
                lines.append("F %d %d %d %s %s" % (L, width, m, q.to_bytes(width, "big").hex(), hexes))
                ki, ai, bi, ci = R.fold(sh, q)
                want.append([v.to_bytes(width, "big").hex() for v in (ki, ai, ci, R.vi_of(q, ki, ai, bi))])
                labels.add(label.split("@")[0])
    got = host(lines)
    bad = [(ln[:60], g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:3]
    assert {"s:" + c for c in K.SUM_CLASSES} <= labels and {"a:zero", "a:q_minus_1", "a:all_max", "a:top_only", "a:digit"} <= labels and len(lines) > 1500


def test_the_header_gives_the_restatements_si(host):
    lines, want = [], []
    mods = [(8, 20, K.dsa_groups()["dsa1024"].q), (8, 28, K.curves()["P-224"]["n"]), (8, 32, K.dsa_groups()["dsa2048"].q), (8, 32, K.curves()["P-256"]["n"]),
            (17, 48, K.curves()["P-384"]["n"]), (17, 66, K.curves()["P-521"]["n"]), (8, 1, 3), (8, 2, 0xFFF1)]
    for L, nb, q in mods:
        for label, m, r, y, k, c in K.s_cases(q, nb):
            lines.append("S %d %d %s" % (L, nb, " ".join(v.to_bytes(nb, "big").hex() for v in (q, m, r, y, k, c))))
            want.append(R.phase3(q, r, y, m, k, c).to_bytes(nb, "big").hex())
            if label == "inner_on_q":
                assert r * y % q + m == q or q == 1
            if label == "outer_on_q":
                assert (r * y % q + m) % q * k % q + c == q or q == 1
    got = host(lines)
    assert [g[0] for g in got] == want and len(lines) > 300


@pytest.mark.parametrize("name", E.NAMES)
def test_fb_mul_fixed_is_pt_mul(host, name):
    c = K.curves()[name]
    f, n = E.byte_len(c), c["n"]
    L = {28: 7, 32: 8, 48: 12, 66: 17}[f]
    nwin = (8 * f + 3) // 4
    sc = [(lb, v) for lb, v in K.scalars(n, 4, nwin, 4 * L)]
    assert {"zero", "one", "two", "fifteen", "sixteen", "q_minus_1", "all_max", "top_only"} <= {lb for lb, _ in sc}
    assert sum(lb.startswith("digit@") for lb, _ in sc) >= (n.bit_length() - 1) // 4 and sum(lb.startswith("random") for lb, _ in sc) == 32
    assert dict(sc)["all_max"] == (1 << (4 * nwin)) - 1 >= n                              # every digit 15, over every window of the table
    curve_hex = "".join(int(c[k]).to_bytes(f, "big").hex() for k in ("p", "n", "b", "gx", "gy"))
    got = host(["C %d %s" % (f, curve_hex)] + ["E " + v.to_bytes(4 * L, "big").hex() for _, v in sc])
    assert got[0] == ["ok"]
    for (lb, v), g in zip(sc, got[1:]):
        assert g[0] == "1", (name, lb)
        if lb in ("zero", "one", "two", "q_minus_1", "top_only", "random0", "random1"):      # ... and it is the restatement's point
            x, y = E.scalar_base_mult(c, v % n)
            assert (int(g[1], 16), int(g[2], 16)) == (x, y), (name, lb)
    assert got[1][1:] == ["00" * f, "00" * f]


@pytest.mark.parametrize("w", [4, 5, 8, 13])
@pytest.mark.parametrize("gname", K.DSA_NAMES)
def test_the_fixed_walk_over_a_pow_built_table_is_pow(host, gname, w):
    """The model of k_tsig_gpow: start at 1, one product per window of the set with the row the header names -- the entry of the
    window's digit, or 1 for the one row -- whatever the exponent.  The table is built by pow()."""
    g = K.dsa_groups()[gname]
    windows = K.windows_of(g.q, w)
    nent = (1 << w) - 1
    sc = K.scalars(g.q, w, windows, 32)
    got = host(["G %d %d %s" % (w, windows, (v % g.q).to_bytes(32, "big").hex()) for _, v in sc])
    for (lb, v), rows in zip(sc, got):
        assert len(rows) == windows                                                     # the schedule: a function of the set's window count alone
        acc, ones = 1, 0
        for i, e in enumerate(int(r) for r in rows):
            if e < 0:
                ones += 1
                continue
            assert e // nent == i and 1 <= e % nent + 1 <= nent
            acc = acc * pow(g.g, (e % nent + 1) << (w * i), g.p) % g.p
        assert acc == pow(g.g, v % g.q, g.p), (gname, w, lb)
        if lb == "zero":
            assert ones == windows
    assert any(lb == "q_minus_1" for lb, _ in sc)


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
    from bftkv_amd import Batcher, Context
    assert all(hasattr(Context, n) for n in ("tdsa_share", "tecdsa_share", "tsig_partial_s")) and all(hasattr(Batcher, n) for n in ("tdsa_share", "tecdsa_share"))


def test_null_context_and_null_batcher_are_refused_and_fail_closed(lib):
    """No device is needed: the refusal comes before anything touches one.  The arrays go in dirty and come back failed and zero."""
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))             # noqa: E731
    c = K.curves()["P-256"]
    f, n, m = 32, 3, 2
    cb = np.frombuffer(b"".join(int(c[k]).to_bytes(f, "big") for k in ("p", "n", "b", "gx", "gy")), dtype=np.uint8).copy()
    sh = np.full((n, m, 4, f), 0x11, dtype=np.uint8)
    dirty = lambda *shape: np.full(shape, 0xA5, dtype=np.uint8)      # noqa: E731
    ri, vi, ki, ci, st = dirty(n, 1 + 2 * f), dirty(n, f), dirty(n, f), dirty(n, f), np.zeros(n, dtype=np.uint8)
    assert lib.bftkv_gpu_tecdsa_share(None, n, m, p(sh), p(cb), 256, p(ri), p(vi), p(ki), p(ci), p(st)) == E_INVALID
    assert (st == R.FAILED).all() and not any(a.any() for a in (ri, vi, ki, ci))
    ri, vi, ki, ci, st = dirty(1 + 2 * f), dirty(f), dirty(f), dirty(f), np.zeros(1, dtype=np.uint8)
    assert lib.bftkv_gpu_batcher_tecdsa_share(None, m, p(sh), p(cb), 256, p(ri), p(vi), p(ki), p(ci), p(st)) == E_INVALID
    assert st[0] == R.FAILED and not any(a.any() for a in (ri, vi, ki, ci))
    ri, vi, ki, ci, st = dirty(256), dirty(f), dirty(f), dirty(f), np.zeros(1, dtype=np.uint8)
    assert lib.bftkv_gpu_batcher_tdsa_share(None, 0, 0, m, p(sh), 256, f, p(ri), p(vi), p(ki), p(ci), p(st)) == E_INVALID
    assert st[0] == R.FAILED and not any(a.any() for a in (ri, vi, ki, ci))
    st = np.zeros(n, dtype=np.uint8)
    assert lib.bftkv_gpu_tdsa_share(None, 0, n, None, m, p(sh), p(dirty(n, 256)), p(vi), p(ki), p(ci), p(st)) == E_INVALID and (st == R.FAILED).all()
    a = [dirty(n, f) for _ in range(5)]
    q = np.frombuffer(int(c["n"]).to_bytes(f, "big"), dtype=np.uint8).copy()
    si, st = dirty(n, f), np.zeros(n, dtype=np.uint8)
    assert lib.bftkv_gpu_tsig_partial_s(None, n, *[p(x) for x in a], f, None, 1, p(q), p(si), p(st)) == E_INVALID
    assert (st == R.FAILED).all() and not si.any()
