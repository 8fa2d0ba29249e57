"""-m gpu: RSA verification over modulus sizes, hashes, public exponents and value shapes (tests/rsa_sizes.py) against the Python
oracle, exactly: verdict, per-packet status and fence of every signature.  tests/test_rsa_sizes_reference.py holds the matrix to
what it claims to be."""
import numpy as np
import pytest

from oracle import collective as col
from oracle import openpgp as pgp
from oracle import wotqs as W
from oracle.packet import SignaturePacket
from tests import helpers as H
from tests import rsa_sizes as RS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matrix():
    keys, cases = RS.keys(), RS.cases()
    ring = [RS.entity(kp) for kp in keys]
    want = [RS.device_expectation(c, RS.oracle_status(ring, c)) for c in cases]
    return keys, cases, col.Keyring(keyring=ring), want


@pytest.mark.parametrize("order", ["shuffled", "by-key"])
def test_every_size_hash_and_value_shape_in_one_call(gpu_ctx, matrix, order):
    """All keys of the table as one keyring, every case as one item of ONE signature_verify call (the fixture's check_small also
    sends it through the <10,8> small-call route, which must agree).  Shuffled, a wave of k_rsa_modexp mixes modulus lengths,
    hashes, exponents and shortcut classes; sorted by key, its waves are uniform."""
    keys, cases, kr, want = matrix
    gpu_ctx.keyring_set(H.abi_keys(kr))
    idx = np.random.default_rng(20240).permutation(len(cases)) if order == "shuffled" else np.arange(len(cases))
    tb, to = H.cat([cases[i].tbs for i in idx])
    sb, so = H.cat([cases[i].sig for i in idx])
    assert gpu_ctx.check_small and len(cases) <= 4096
    err = gpu_ctx.signature_verify(tb, to, sb, so)
    fenced = gpu_ctx.last_fenced.copy()
    st, st_item = gpu_ctx.last_statuses()
    assert list(st_item) == list(range(len(cases)))           # one packet per item
    bad = []
    for pos, i in enumerate(idx):
        c, (w_st, w_fenced) = cases[i], want[i]
        got = (int(st[pos]), bool(fenced[pos]), err[pos] == 0)
        if got != (w_st, w_fenced, w_st == pgp.ST_OK):
            bad.append((c.bits, keys[c.key].e, c.hash_id, c.variant, got, (w_st, w_fenced)))
    assert not bad, (len(bad), bad[:40])
    assert (err == 0).sum() > 500 and fenced.sum() == sum(f for _, f in want) > 150


def test_collective_verify_over_short_and_odd_moduli(gpu_ctx, matrix):
    """A quorum of one key per size class and the 512-, 688- and 1025-bit keys: every item carries one packet of each under
    rotating hashes (SHA-384 and SHA-512 do not fit the 512-bit key, SHA-512 not the 688-bit one) and value shapes; statuses,
    n_verified and err follow the oracle with the early exit on and off."""
    keys, cases, _, _ = matrix
    by_bits = {}
    for kp in keys:
        if kp.e == 65537:
            by_bits.setdefault(kp.n.bit_length(), kp)
    signers = [by_bits[b] for b in (2048, 3072, 4096, 512, 688, 1025)]
    kr = col.Keyring(keyring=[RS.entity(kp) for kp in signers])
    gpu_ctx.keyring_set(H.abi_keys(kr))
    q = W.WotQ([W.new_qc([kp.key_id for kp in signers], len(signers), W.AUTH, 0)])
    qh = gpu_ctx.quorum_create(H.abi_qcs(q))
    rng = np.random.default_rng(35)
    tbs_l, ss_l = [], []
    for i in range(24):
        tbs = rng.bytes(int(rng.integers(0, 200)))
        parts = []
        for j, kp in enumerate(signers):
            cell = RS.cell_cases(j, kp, RS.HASHES[(i + 2 * j) % 5][0], tbs, i + j)
            pick = ("untouched", "s + n", "at the cap", "bit flipped", "canonical mpi", "untouched", "em")[(i + j) % 7]
            parts.append(next((c.sig for c in cell if c.variant.startswith(pick)), cell[0].sig))
        tbs_l.append(tbs + b"x" if i % 6 == 5 else tbs)               # every sixth: other bytes than were signed
        ss_l.append(b"".join(parts[int(o)] for o in rng.permutation(len(parts))))
    tb, to = H.cat(tbs_l)
    sb, so = H.cat(ss_l)
    try:
        seen, seen_st = set(), set()
        for early in (True, False):
            gpu_ctx.set_early_exit(early)
            err, nver, _ = gpu_ctx.collective_verify(qh, tb, to, sb, so)
            st, st_item = gpu_ctx.last_statuses()
            assert not gpu_ctx.last_fenced.any()
            for i in range(24):
                r = col.collective_verify(kr, tbs_l[i], SignaturePacket(1, 0, False, ss_l[i], None), q)
                got = list(st[st_item == i])
                assert got[:len(r.statuses)] == r.statuses, (early, i, got, r.statuses)
                assert (err[i] == 0) == (r.err is None) and nver[i] == len(r.verified), (early, i)
                seen.add(r.err is None)
                if not early:                                             # every packet on its own, the ones behind the exit too
                    each, pos = [], 0
                    while pos < len(ss_l[i]):
                        step = pgp.check_detached_signature(kr.get_keyring(), tbs_l[i], ss_l[i], pos)
                        each += step.statuses
                        pos = step.pos
                    assert got == each and len(got) == len(signers), (i, got, each)
                    seen_st.update(got)
        assert seen == {True, False} and {pgp.ST_OK, pgp.ST_BAD_SIG, pgp.ST_HASH_TAG} <= seen_st
    finally:
        gpu_ctx.set_early_exit(True)
        gpu_ctx.quorum_destroy(qh)
