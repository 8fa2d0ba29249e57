"""-m gpu: the OpenPGP pipeline's DSA kernels (k_dsa_inv, k_dsa_inv_batched, k_dsa_mul, k_dsa_build_comb, k_dsa_split, k_dsa_modexp)
on the cases of tests/dsa_pipeline_cases.py, through the C ABI: signatures whose window digits are chosen, at every table width
that can be set up to 18 bits; keys whoever presents a certificate might choose; runs of signatures whose product of s has no
inverse.  Status, fence and verdict of every item against the oracle (or the `unsupported` rule), exactly, every case in the call.
tests/test_dsa_pipeline_reference.py holds the cases to what they claim to be."""
import functools
import os

import numpy as np
import pytest

from oracle import collective as col
from oracle import openpgp as pgp
from oracle import wotqs as W
from oracle.packet import SignaturePacket
from tests import dsa_pipeline_cases as P
from tests import helpers as H

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _want(which, *args):
    """(Ring, [(status, fenced, accepted)]) of P.ring(*args), P.sparse_wave(), P.hostile_ring() or P.inversion_runs(): computed once."""
    rg = getattr(P, which)(*args)
    return rg, [P.expectation(c, s) for c, s in zip(rg.cases, P.oracle_statuses(rg))]


def _keyring(rg):
    return col.Keyring(keyring=[P.entity(kp) for kp in rg.keys])


def _verify(ctx, rg, want, idx):
    """One signature_verify call over the cases idx, in that order: everything equal to `want`.  Returns err."""
    tb, to = H.cat([rg.cases[i].payload for i in idx])
    sb, so = H.cat([rg.cases[i].sig for i in idx])
    assert ctx.check_small                                         # the same call again on the small-call route, and both agree
    err = ctx.signature_verify(tb, to, sb, so)
    fenced = ctx.last_fenced.copy()
    st, st_item = ctx.last_statuses()
    assert list(st_item) == list(range(len(idx)))                  # one packet per item
    bad = [(rg.cases[i].label, (int(st[pos]), bool(fenced[pos]), bool(err[pos] == 0)), want[i])
           for pos, i in enumerate(idx) if (int(st[pos]), bool(fenced[pos]), bool(err[pos] == 0)) != want[i]]
    assert not bad, (len(bad), bad[:24])
    return err


def _own_context():
    import torch  # noqa: F401  (its HIP runtime first, as the gpu_ctx fixture does)
    from bftkv_amd import Context
    ctx = Context(0)
    ctx.check_small = True
    return ctx


def _at_width(gpu_ctx, wbits, body):
    """body(ctx) with the tables pinned at wbits.  16 bits and more: a context of its own, closed at the end (gigabytes of tables)."""
    ctx = gpu_ctx if wbits < 16 else _own_context()
    ctx.set_dsa_window_bits(wbits)
    try:
        body(ctx)
    finally:
        ctx.set_dsa_window_bits(0)
        if ctx is not gpu_ctx:
            ctx.close()


@pytest.mark.parametrize("wbits", P.WIDTHS)
def test_chosen_digits_at_every_width(gpu_ctx, wbits):
    """u2, then u1, at 1, a full window 0, a full window across a 32-bit word boundary, the top window of q alone, every other
    window full, and q - 1, each under its own 2048-bit key, with a refused twin each: one shuffled call."""
    rg, want = _want("ring", wbits, False)

    def body(ctx):
        ctx.keyring_set(H.abi_keys(_keyring(rg)))
        assert ctx.dsa_window_bits() == wbits and ctx.dsa_table_bytes()[1] == 76
        idx = [int(i) for i in np.random.default_rng(wbits).permutation(len(rg.cases))]
        err = _verify(ctx, rg, want, idx)
        assert int((err == 0).sum()) == len(rg.keys) == len(rg.cases) // 2
    _at_width(gpu_ctx, wbits, body)


@pytest.mark.parametrize("wbits", (8, 13, 16))
def test_chosen_digits_with_both_size_classes(gpu_ctx, wbits):
    """The same under 1024-, 2048- and 3072-bit keys in one ring (2048 and 3072 at 16 bits): entries of 112 limbs, k_dsa_split, both
    instantiations of k_dsa_modexp in one call; then as one-packet items of collective_verify, every packet verified."""
    rg, want = _want("ring", wbits, True)
    kr = _keyring(rg)
    ids = [kp.key_id for kp in rg.keys]
    q = W.WotQ([W.QC(ids, 0, 1, 1, 1)])                            # one verified signer suffices

    def body(ctx):
        ctx.keyring_set(H.abi_keys(kr))
        assert ctx.dsa_window_bits() == wbits and ctx.dsa_table_bytes()[1] == 112
        idx = [int(i) for i in np.random.default_rng(100 + wbits).permutation(len(rg.cases))]
        err = _verify(ctx, rg, want, idx)
        assert int((err == 0).sum()) == len(rg.keys)
        qh = ctx.quorum_create([(0, 1, 1, 1, ids)])
        ctx.set_early_exit(False)
        try:
            tb, to = H.cat([rg.cases[i].payload for i in idx])
            sb, so = H.cat([rg.cases[i].sig for i in idx])
            cerr, nver, _ = ctx.collective_verify(qh, tb, to, sb, so)
            st, st_item = ctx.last_statuses()
            assert list(st_item) == list(range(len(idx))) and not ctx.last_fenced.any()
            for pos, i in enumerate(idx):
                c = rg.cases[i]
                r = col.collective_verify(kr, c.payload, SignaturePacket(1, 0, False, c.sig, None), q)
                assert r.statuses == [want[i][0]]
                assert (int(st[pos]), cerr[pos] == 0, int(nver[pos])) == (r.statuses[0], r.err is None, len(r.verified)), c.label
        finally:
            ctx.set_early_exit(True)
            ctx.quorum_destroy(qh)
    _at_width(gpu_ctx, wbits, body)


def test_wave_of_sparse_exponents(gpu_ctx):
    """Sixteen signatures in a row -- the groups of one block -- whose u2 all have the same single non-zero 13-bit window (7, which
    lies in two words): the wave skips every other step of that base.  Then fifteen of them around one u2 = q - 1: no step is
    skipped and the sparse lanes ride along with zero digits.  Then the sixteen twins."""
    rg, want = _want("sparse_wave")

    def body(ctx):
        ctx.keyring_set(H.abi_keys(_keyring(rg)))
        assert ctx.dsa_window_bits() == 13
        sparse, twins, dense = list(range(0, 32, 2)), list(range(1, 32, 2)), 32
        assert (_verify(ctx, rg, want, sparse) == 0).all()
        err = _verify(ctx, rg, want, sparse[:7] + [dense] + sparse[8:])
        assert (err == 0).all()
        err = _verify(ctx, rg, want, sparse[:3] + twins[3:7] + [dense] + twins[8:12] + sparse[12:])
        assert int((err == 0).sum()) == 8
        assert (_verify(ctx, rg, want, twins) != 0).all()
    _at_width(gpu_ctx, 13, body)


@pytest.mark.parametrize("wbits", (8, 13))
def test_keys_an_attacker_would_choose(gpu_ctx, wbits):
    """Orders of 32 to 256 bits, off the byte, composite; p of 512 to 2048 bits off the limb and the byte, and p = 3; y and g at 0,
    1, p - 1 and beyond p; and the keys the key table turns away (p = 1, even p or q, q under 32 or over 256 bits, y over the cap),
    uploaded with the others: those are fenced with ST_UNSUPPORTED, everything else is the oracle's answer and not fenced."""
    rg, want = _want("hostile_ring")

    def body(ctx):
        ctx.keyring_set(H.abi_keys(_keyring(rg)))
        assert ctx.dsa_window_bits() == wbits and ctx.dsa_table_bytes()[1] == 76
        idx = [int(i) for i in np.random.default_rng(wbits).permutation(len(rg.cases))]
        err = _verify(ctx, rg, want, idx)
        accepted = {rg.keys[rg.cases[i].key].name.split(" <")[0] for pos, i in enumerate(idx) if err[pos] == 0}
        assert set(P.HONEST_GROUPS) <= accepted, set(P.HONEST_GROUPS) - accepted
        assert sum(c.rule == "unsupported" for c in rg.cases) >= 60 and not any(f for (_, f, _), c in zip(want, rg.cases) if c.rule == "oracle")
    _at_width(gpu_ctx, wbits, body)


def test_runs_whose_product_has_no_inverse():
    """k_dsa_inv_batched's fallback: under a composite q, one s in eight shares a factor with q, so most 16-entry runs multiply up a
    product without an inverse and every member goes through the per-signature routine -- the honest ones must still verify.
    BFTKV_DSA_INV=single against =batched: the same four result arrays, and every item the oracle's."""
    import torch  # noqa: F401
    from bftkv_amd import Context
    rg, want = _want("inversion_runs")
    kr = _keyring(rg)
    ids = [kp.key_id for kp in rg.keys]
    tb, to = H.cat([c.payload for c in rg.cases])
    sb, so = H.cat([c.sig for c in rg.cases])
    got = {}
    for mode in ("single", "batched"):
        os.environ["BFTKV_DSA_INV"] = mode
        try:
            ctx = Context(0)
        finally:
            del os.environ["BFTKV_DSA_INV"]
        try:
            ctx.set_early_exit(False)
            ctx.keyring_set(H.abi_keys(kr))
            qh = ctx.quorum_create([(0, 1, 1, 1, ids)])
            err, nver, _ = ctx.collective_verify(qh, tb, to, sb, so)
            st, st_item = ctx.last_statuses()
            assert not ctx.last_fenced.any()
            got[mode] = (err.copy(), nver.copy(), st.copy(), st_item.copy())
        finally:
            ctx.close()
    for a, b in zip(got["single"], got["batched"]):
        assert a.shape == b.shape and (a == b).all()
    for mode in ("single", "batched"):
        err, nver, st, st_item = got[mode]
        assert list(st_item) == list(range(len(rg.cases)))
        bad = [(c.label, (int(st[i]), bool(err[i] == 0), int(nver[i])), want[i]) for i, c in enumerate(rg.cases)
               if (int(st[i]), bool(err[i] == 0), int(nver[i])) != (want[i][0], want[i][2], int(want[i][2]))]
        assert not bad, (mode, len(bad), bad[:24])
        honest = [i for i, c in enumerate(rg.cases) if c.key < 2 and c.kind == "honest"]
        assert len(honest) > 250 and all(st[i] == pgp.ST_OK and err[i] == 0 for i in honest)
