"""-m gpu: RSA keys over prime moduli with every radix-2^28 limb full or almost every limb zero, and DSA groups at the two ends
of their size class (tests/extremal_keys.py, tests/golden/extremal_moduli.json), through the C ABI.  Verdict, status and fence of
every signature against the oracle, exactly.  A public key is chosen by whoever presents a certificate: these are the moduli an
attacker would pick to make column sums, carries and borrows in csrc/mont28.h as large or as long as they get.
tests/test_rsa_sizes_reference.py holds the RSA cases to what they claim to be; tests/test_gpu_mont_forms.py runs the same moduli
through the multiplier alone."""
import numpy as np
import pytest

from corpus import build as cb
from corpus.keys import DRBG
from oracle import collective as col
from oracle import openpgp as pgp
from tests import extremal_keys as X
from tests import helpers as H
from tests import rsa_sizes as RS

import dsa_verify_cases as K
import dsa_verify_ref as V
from test_gpu_dsa_verify import lane_ctx  # noqa: F401  (a context per lane form of the raw DSA entry)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matrix():
    keys, cases = X.rsa_keys(), X.rsa_cases()
    ring = [RS.entity(kp) for kp in keys]
    want = [RS.device_expectation(c, RS.oracle_status(ring, c)) for c in cases]
    return keys, cases, col.Keyring(keyring=ring), want


def _verify(gpu_ctx, cases, want, idx, keys):
    tb, to = H.cat([cases[i].tbs for i in idx])
    sb, so = H.cat([cases[i].sig for i in idx])
    err = gpu_ctx.signature_verify(tb, to, sb, so)
    fenced = gpu_ctx.last_fenced.copy()
    st, st_item = gpu_ctx.last_statuses()
    assert list(st_item) == list(range(len(idx)))             # one packet per item
    bad = []
    for pos, i in enumerate(idx):
        c, (w_st, w_fenced) = cases[i], want[i]
        got = (int(st[pos]), bool(fenced[pos]), err[pos] == 0)
        if got != (w_st, w_fenced, w_st == pgp.ST_OK):
            bad.append((keys[c.key].name, c.hash_id, c.variant, got, (w_st, w_fenced)))
    assert not bad, (len(bad), bad[:40])
    return err, fenced


@pytest.mark.parametrize("order", ["shuffled", "by-key"])
def test_every_extremal_key_hash_and_value_shape_in_one_call(gpu_ctx, matrix, order):
    """14 keys x 5 hashes x 7 value shapes as ONE signature_verify call: k_rsa_modexp<19,4>, <14,8> and <19,8>, and through the
    fixture's check_small the whole call again on the small-call route, where the keys of up to 2048 bits run <10,8>."""
    keys, cases, kr, want = matrix
    gpu_ctx.keyring_set(H.abi_keys(kr))
    idx = np.random.default_rng(2128).permutation(len(cases)) if order == "shuffled" else np.arange(len(cases))
    assert gpu_ctx.check_small and len(cases) == 14 * 5 * 7
    err, fenced = _verify(gpu_ctx, cases, want, idx, keys)
    ok = {(cases[i].key, cases[i].hash_id) for pos, i in enumerate(idx) if err[pos] == 0}
    assert ok == {(ki, h) for ki in range(len(keys)) for h, _ in RS.HASHES}          # a valid case in every (key, hash) cell
    assert fenced.sum() == sum(f for _, f in want) == 14 * 5                         # the over-the-cap value of every cell
    assert (err == 0).sum() == 14 * 5 * 4                                            # untouched, canonical, s + n, at the cap


@pytest.fixture(scope="module")
def class_pools(matrix):
    """Per 8-lane size class (1: <= 3072 bits, 2: <= 4096) the extremal keys' cases and the SHA-256 cell of the suite's ordinary
    key of that size, nothing over the cap; and the keyring that holds them all."""
    keys, cases, _, _ = matrix
    ordinary = [next(kp for kp in RS.keys() if kp.n.bit_length() == bits and kp.e == 65537) for bits in (3072, 4096)]
    ring = [RS.entity(kp) for kp in list(keys) + ordinary]
    pools = {}
    for cls, kp in zip((1, 2), ordinary):
        ext = [(keys[c.key].name, c) for c in cases if RS.size_class(c.bits) == cls and not c.over_cap]
        cell = RS.cell_cases(-1, kp, 8, b"an ordinary key beside the extremal ones, class %d" % cls, cls)
        pools[cls] = ext, [(kp.name, c) for c in cell if not c.over_cap]
    return ring, pools


@pytest.mark.parametrize("n_sigs", [7, 8, 9, 31, 32, 33])
def test_eight_lane_group_boundaries(gpu_ctx, class_pools, n_sigs):
    """n signatures of the 3072-bit class and n of the 4096-bit class in one call: k_rsa_modexp<14,8> and <19,8> get n groups
    each, the last of them just before / at / just past the end of a wave (8 groups) and of a block (32).  Two in three are under
    extremal keys, the rest under an ordinary key of the class, valid and invalid values mixed, in random order."""
    ring, pools = class_pools
    rng = np.random.default_rng(n_sigs)
    sel = []
    for cls in (1, 2):
        ext, ordinary = pools[cls]
        n_ord = n_sigs // 3
        sel += [ext[int(j)] for j in rng.permutation(len(ext))[:n_sigs - n_ord]] + [ordinary[j % len(ordinary)] for j in range(n_ord)]
    sel = [sel[int(j)] for j in rng.permutation(len(sel))]
    assert [sum(RS.size_class(c.bits) == cls for _, c in sel) for cls in (1, 2)] == [n_sigs, n_sigs]
    want = [RS.oracle_status(ring, c) for _, c in sel]
    gpu_ctx.keyring_set(H.abi_keys(col.Keyring(keyring=ring)))
    tb, to = H.cat([c.tbs for _, c in sel])
    sb, so = H.cat([c.sig for _, c in sel])
    err = gpu_ctx.signature_verify(tb, to, sb, so)
    st, st_item = gpu_ctx.last_statuses()
    assert list(st_item) == list(range(len(sel))) and not gpu_ctx.last_fenced.any()
    got = [(int(s), e == 0) for s, e in zip(st, err)]
    exp = [(w, w == pgp.ST_OK) for w in want]
    assert got == exp, [(name, c.variant, g, e) for (name, c), g, e in zip(sel, got, exp) if g != e]
    assert 0 < sum(ok for _, ok in exp) < len(exp)


# ---- DSA

def _dsa_entity(kp):
    return pgp.Entity(primary=pgp.PublicKey(key_id=kp.key_id, pk_algo=cb.PK_DSA, p=kp.p, q=kp.q, g=kp.g, y=kp.y), name=kp.name)


def test_openpgp_dsa_signatures_under_extremal_groups(gpu_ctx):
    """Valid and tampered OpenPGP DSA signatures (the corpus signer) under the four groups: k_dsa_build_comb and k_dsa_modexp in
    <19,4> (2048-bit p) and <14,8> (3072-bit p); status and verdict are the oracle's, whose arithmetic is dsa_verify."""
    kps = list(X.dsa_keys().values())
    ring = [_dsa_entity(kp) for kp in kps]
    gpu_ctx.keyring_set(H.abi_keys(col.Keyring(keyring=ring)))
    srng = DRBG("extremal dsa groups")
    rng = np.random.default_rng(3072)
    tbs_l, sig_l = [], []
    for i in range(48):
        kp = kps[i % 4]
        tbs = b"extremal dsa %d " % i + rng.bytes(int(rng.integers(0, 120)))
        sig = cb.detach_sign(kp, tbs, srng, hash_id=(8, 9, 10)[(i // 4) % 3])
        if i % 3 == 1:
            sig = sig[:-1] + bytes([sig[-1] ^ 1])              # the lowest bit of s
        if i % 8 == 6:
            tbs += b"x"                                        # other bytes than were signed
        tbs_l.append(tbs); sig_l.append(sig)
    want = []
    for tbs, sig in zip(tbs_l, sig_l):
        r = pgp.check_detached_signature(ring, tbs, sig, 0)
        assert r.pos == len(sig) and r.statuses == [r.status]
        want.append(r.status)
    assert [w == pgp.ST_OK for w in want] == [i % 3 != 1 and i % 8 != 6 for i in range(48)]
    tb, to = H.cat(tbs_l)
    sb, so = H.cat(sig_l)
    err = gpu_ctx.signature_verify(tb, to, sb, so)
    st, st_item = gpu_ctx.last_statuses()
    assert list(st_item) == list(range(48)) and not gpu_ctx.last_fenced.any()
    assert [int(s) for s in st] == want and [e == 0 for e in err] == [w == pgp.ST_OK for w in want]
    for j in range(4):                                         # valid and refused under every group
        assert {w == pgp.ST_OK for w in want[j::4]} == {True, False}


def test_raw_dsa_under_extremal_2048_bit_groups_in_both_lane_forms(lane_ctx):   # noqa: F811
    """r || s through bftkv_gpu_dsa_verify under the two 2048-bit groups in one call, with 4 and with 8 lanes per number:
    honest signatures, a flipped bit in r, in s and in the digest, r and s at q - 1."""
    rng = np.random.default_rng(256)
    grp = [X.dsa_keys()[n] for n in ("dsa2048_high", "dsa2048_low")]
    gs, ks = [(kp.p, kp.q, kp.g) for kp in grp], [(i, kp.y) for i, kp in enumerate(grp)]
    digests, sigs, idx, want = [], [], [], []
    for j in range(36):
        gi = j % 2
        kp = grp[gi]
        dg = rng.bytes(32)
        rs = None
        while rs is None:
            rs = K.sign(kp.p, kp.q, kp.g, kp.x, dg, K.rnd(rng, kp.q) or 1)
        r, s = rs
        how = (j // 2) % 6
        if how == 1:
            r ^= 1 << int(rng.integers(255))
        elif how == 2:
            s ^= 1 << int(rng.integers(255))
        elif how == 3:
            dg = bytes([dg[0] ^ 0x80]) + dg[1:]
        elif how == 4:
            r, s = kp.q - 1, kp.q - 1
        digests.append(dg); sigs.append(r.to_bytes(32, "big") + s.to_bytes(32, "big")); idx.append(gi)
        want.append(V.verify(kp.p, kp.q, kp.g, kp.y, dg, r, s))
        assert bool(want[-1][0]) == pgp.dsa_verify(kp.p, kp.q, kp.g, kp.y, dg, r, s) and want[-1][1] == V.OK
    valid, st = lane_ctx.dsa_verify(digests, sigs, ks, gs, key_idx=idx, pbytes=256, qbytes=32)
    assert [(int(v), int(s)) for v, s in zip(valid, st)] == want
    assert sum(v for v, _ in want) == 12 and all(v == 0 for (v, _), j in zip(want, range(36)) if (j // 2) % 6 in (1, 2, 3, 4))
