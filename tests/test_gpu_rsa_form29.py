"""-m gpu: RSA verification through the C ABI on the 4-lane route of big calls -- k_rsa_modexp<18,4,29>, and behind it the
19 x 4 form of 28 bits for the values too long for 72 limbs of 29 bits -- against the Python oracle, exactly: verdict,
per-packet status and fence of every signature.

Keys: the suite's first 2048-bit key and the full 2048-bit prime modulus of tests/golden/extremal_moduli.json under 65537,
that modulus under e = 3 and the sparse one under e = 17, the 1025-bit key under 65537, 3 and 17.  Hashes: SHA-256, SHA-512.
Values per (key, hash): s, its canonical MPI, s behind three zero bytes, s + j n of exactly 257, 261 (the last length 72
limbs hold), 262 and 266 bytes (the 28-bit form's share) and 267 (beyond R of the class: fenced, as ever), s with a bit
flipped, and a wrong encoding signed with the private key.  One call holds them all, shuffled, so that a wave mixes 261- and
262-byte values, exponents and shortcut classes; then its head cut to 63, 64 and 65 signatures (the end of a block of 64)."""
import numpy as np
import pytest

from oracle import collective as col
from oracle import openpgp as pgp
from tests import extremal_keys as X
from tests import helpers as H
from tests import rsa_sizes as RS

pytestmark = pytest.mark.gpu

LENGTHS = [257, 261, 262, 266, 267]
HASH_IDS = [8, 10]


def _keys():
    mods = {e["name"]: int(e["n"], 16) for e in X.fixture()["rsa"]}
    by = {}
    for kp in RS.keys():
        by.setdefault((kp.n.bit_length(), kp.e), kp)
    return [by[(2048, 65537)], X.PrimeModulusKey(mods["full2048"], 65537, "full2048 <k@bftkv.example>"),
            X.PrimeModulusKey(mods["full2048"], 3, "full2048e3 <k@bftkv.example>"), X.PrimeModulusKey(mods["sparse2048"], 17, "sparse2048e17 <k@bftkv.example>"),
            by[(1025, 65537)], by[(1025, 3)], by[(1025, 17)]]


def _cell(ki, kp, hash_id, tbs):
    bits = kp.n.bit_length()
    k = (bits + 7) // 8
    name = dict(RS.HASHES)[hash_id]
    prefix, digest = RS.digest_of(kp, tbs, hash_id)
    n = kp.n
    em = RS.encode(k, name, digest)
    s = kp.rsa_private(int.from_bytes(em, "big") % n)
    out = []

    def add(variant, mpi, over_cap=False):
        out.append(RS.Case(ki, bits, hash_id, variant, tbs, RS.packet(prefix, digest, mpi), True, over_cap))
    add("s", RS.go_mpi(s, k))
    add("canonical mpi", RS.cb._mpi(s))
    add("s behind zero bytes", RS.go_mpi(s, k + 3))
    for nb in LENGTHS:
        v = s + ((1 << (8 * nb)) - 1 - s) // n * n
        assert v % n == s and v >> (8 * nb - 8) != 0 and v < 1 << (8 * nb)
        add("s + jn, %d bytes" % nb, RS.go_mpi(v, nb), over_cap=nb > RS.value_cap(bits))
    add("bit flipped", RS.go_mpi(s ^ (1 << ((7 * bits + 13 * hash_id + ki) % (bits - 1))), k))
    name_t, em_t = sorted(RS.tampered_encodings(k, name, digest).items())[(ki + hash_id) % 4]
    add(name_t, RS.go_mpi(kp.rsa_private(int.from_bytes(em_t, "big")), k))
    return out


@pytest.fixture(scope="module")
def matrix():
    keys = _keys()
    assert len({kp.key_id for kp in keys}) == len(keys)
    cases = []
    for ki, kp in enumerate(keys):
        for h in HASH_IDS:
            cases += _cell(ki, kp, h, b"rsa form 29: key %d, hash %d " % (ki, h) + bytes(range(3 * ki + h)))
    ring = [RS.entity(kp) for kp in keys]
    want = [RS.device_expectation(c, RS.oracle_status(ring, c)) for c in cases]
    return keys, cases, col.Keyring(keyring=ring), want


def _verify(gpu_ctx, matrix, idx):
    keys, cases, kr, want = matrix
    gpu_ctx.keyring_set(H.abi_keys(kr))
    tb, to = H.cat([cases[i].tbs for i in idx])
    sb, so = H.cat([cases[i].sig for i in idx])
    err = gpu_ctx.signature_verify(tb, to, sb, so)              # the 4-lane route (and, check_small, the <10,8> route again)
    fenced = gpu_ctx.last_fenced.copy()
    st, st_item = gpu_ctx.last_statuses()
    assert list(st_item) == list(range(len(idx)))
    bad = []
    for pos, i in enumerate(idx):
        c, (w_st, w_fenced) = cases[i], want[i]
        got = (int(st[pos]), bool(fenced[pos]), err[pos] == 0)
        if got != (w_st, w_fenced, w_st == pgp.ST_OK):
            bad.append((pos, keys[c.key].name, c.hash_id, c.variant, got, (w_st, w_fenced)))
    assert not bad, (len(bad), bad[:40])
    return err, fenced


def test_every_key_exponent_and_value_length_in_one_call(gpu_ctx, matrix):
    keys, cases, _, want = matrix
    assert len(cases) == 7 * 2 * 10 == 140
    idx = np.random.default_rng(2088).permutation(len(cases))
    # a wave of the modexp holds 16 signatures: 261- and 262-byte values meet inside one
    wide = [("262" in cases[i].variant or "266" in cases[i].variant) for i in idx]
    narrow = ["261" in cases[i].variant for i in idx]
    assert any(any(wide[j:j + 16]) and any(narrow[j:j + 16]) for j in range(0, len(idx), 16))
    err, fenced = _verify(gpu_ctx, matrix, idx)
    assert (err == 0).sum() == 7 * 2 * 7                        # s, canonical, zero bytes, 257, 261, 262, 266
    assert fenced.sum() == sum(f for _, f in want) == 7 * 2     # the 267-byte value of every cell
    for pos, i in enumerate(idx):
        if "bit flipped" in cases[i].variant or cases[i].variant.startswith("em "):
            assert err[pos] != 0 and not fenced[pos]


@pytest.mark.parametrize("n_sigs", [63, 64, 65])
def test_cut_at_the_end_of_a_block(gpu_ctx, matrix, n_sigs):
    idx = np.random.default_rng(2088).permutation(len(matrix[1]))[:n_sigs]
    _verify(gpu_ctx, matrix, idx)
