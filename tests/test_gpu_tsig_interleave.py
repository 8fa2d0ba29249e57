"""-m gpu: the share answers of threshold DSA / ECDSA signing read the tables that verification reads -- a DSA key set's window table
of g, the context's table of G -- and write neither.  Share calls interleaved with dsa_verify_keyset and ecdsa_verify calls on the same
set and curve: every call gives its stand-alone answer, and the set's tables are word for word what they were."""
import numpy as np
import pytest

import dsa_verify_cases as DK
import dsa_verify_ref as DV
import ec_ref as E
import ecdsa_verify_ref as EV
import tsig_share_cases as K
from test_gpu_tsig_share import _check, _dsa_want, _ec_want

pytestmark = pytest.mark.gpu


def _dsa_sigs(g, rng, n):
    """honest signatures over 32-byte digests (20 for a 160-bit q), every third with one bit of s flipped"""
    dlen = g.q.bit_length() // 8
    out = []
    while len(out) < n:
        dg = rng.bytes(dlen)
        rs = DK.sign_try(rng, g, dg)
        if rs:
            r, s = rs
            out.append((dg, r, s ^ 2 if len(out) % 3 == 2 else s))
    return out


def test_dsa_share_calls_between_keyset_verifications(gpu_ctx):
    gs = [K.dsa_groups()[n] for n in K.DSA_NAMES]
    g = gs[1]
    ks = gpu_ctx.dsa_keyset_create([(0, g.y)], [(g.p, g.q, g.g)], window_bits=4)
    try:
        before = [gpu_ctx.selftest_dsa_keyset_table(ks, b).copy() for b in (0, 1)]
        rng = np.random.default_rng(77)
        sigs = _dsa_sigs(g, rng, 24)
        dgs = [dg for dg, _, _ in sigs]
        sgs = [r.to_bytes(32, "big") + s.to_bytes(32, "big") for _, r, s in sigs]
        want_v = [DV.verify(g.p, g.q, g.g, g.y, dg, r, s) for dg, r, s in sigs]
        assert {v for v, _ in want_v} == {0, 1}
        cases = K.requests(g.q, 32, 2, 4, 64, seed=5)[:40]
        labels, reqs = [lb for lb, _ in cases], [sh for _, sh in cases]
        sh, want_s = K.shares_array(reqs, 32), _dsa_want(g, 256, 32, reqs)
        for _ in range(3):
            valid, st = gpu_ctx.dsa_verify_keyset(ks, dgs, sgs)
            assert [(int(v), int(s)) for v, s in zip(valid, st)] == want_v
            _check(gpu_ctx.tdsa_share(ks, sh), want_s, labels, "between verifications")
        valid, st = gpu_ctx.dsa_verify_keyset(ks, dgs, sgs)
        assert [(int(v), int(s)) for v, s in zip(valid, st)] == want_v
        after = [gpu_ctx.selftest_dsa_keyset_table(ks, b) for b in (0, 1)]
        assert all((a == b).all() for a, b in zip(before, after))
    finally:
        gpu_ctx.dsa_keyset_destroy(ks)


@pytest.mark.parametrize("name", ["P-256", "P-521"])
def test_ecdsa_share_calls_between_verifications(gpu_ctx, name):
    c = E.CURVES[name]
    f, n = E.byte_len(c), c["n"]
    rng = np.random.default_rng(78)
    d = int.from_bytes(rng.bytes(f), "big") % (n - 1) + 1
    key = E.marshal(c, *E.scalar_base_mult(c, d))
    dgs, sgs = [], []
    for i in range(8):
        dg = rng.bytes(f if name == "P-256" else 64)
        r, s = E.ecdsa_sign_hash_int(c, d, EV.hash_to_int(c, dg) % n, int.from_bytes(rng.bytes(f), "big") % (n - 1) + 1)
        if i % 3 == 2:
            s ^= 4
        dgs.append(dg)
        sgs.append(r.to_bytes(f, "big") + s.to_bytes(f, "big"))
    want_v = [EV.verify(c, key, dg, sg) for dg, sg in zip(dgs, sgs)]
    assert {v for v, _ in want_v} == {0, 1}
    cases = K.requests(n, f, 2, 4, (8 * f + 3) // 4, seed=2)[:12]          # (the scalars of test_gpu_tsig_share: their points are remembered)
    labels, reqs = [lb for lb, _ in cases], [sh for _, sh in cases]
    sh, want_s = K.shares_array(reqs, f), _ec_want(name, reqs)
    ks = gpu_ctx.ecdsa_keyset_create([key], c)
    try:
        before = gpu_ctx.selftest_ecdsa_keyset_table(ks, 0).copy()
        for _ in range(2):
            _check(gpu_ctx.tecdsa_share(sh, c), want_s, labels, "before a verification")
            valid, st = gpu_ctx.ecdsa_verify(dgs, sgs, [key], c)
            assert [(int(v), int(s)) for v, s in zip(valid, st)] == want_v
            valid, st = gpu_ctx.ecdsa_verify_keyset(ks, dgs, sgs)
            assert [(int(v), int(s)) for v, s in zip(valid, st)] == want_v
        _check(gpu_ctx.tecdsa_share(sh, c), want_s, labels, "after the verifications")
        assert (gpu_ctx.selftest_ecdsa_keyset_table(ks, 0) == before).all()
    finally:
        gpu_ctx.ecdsa_keyset_destroy(ks)
