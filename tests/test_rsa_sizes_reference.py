"""CPU: the RSA modulus-size x hash matrix of tests/rsa_sizes.py is what tests/test_gpu_rsa_sizes.py takes it for, and the two
oracles -- Python integers (oracle/openpgp.py) and OpenSSL bignums (oracle/c/oracle.c) -- give every case the same status."""
import json
import os
from collections import Counter

from corpus.keys import gen_rsa
from oracle import collective as col
from oracle.cbind import COracle
from tests import rsa_sizes as RS

N_KEYS = 42
N_CASES = 1643          # pinned: the GPU test cannot pass by having lost its cases


def test_gen_rsa_draws_for_even_sizes_are_unchanged():
    """Odd bit lengths give p the larger half; an even length draws what it always drew, so every cached key is still the
    generator's output."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "keys_rsa2048.json")) as f:
        first = json.load(f)["keys"][0]
    assert {name: "%x" % v for name, v in gen_rsa(0, 2048).items()} == first
    for bits in (255, 256, 257, 333):
        k = gen_rsa(0, bits)
        assert (k["p"] * k["q"]).bit_length() == bits and k["p"].bit_length() == bits - bits // 2 and k["q"].bit_length() == bits // 2
    k = gen_rsa(0, 257, e=3)
    assert k["e"] == 3 and ((k["p"] - 1) * (k["q"] - 1)) % 3 != 0


def test_matrix_is_what_it_claims_and_the_oracles_agree():
    keys, cases = RS.keys(), RS.cases()
    assert len(keys) == N_KEYS and len(cases) == N_CASES
    ring = [RS.entity(kp) for kp in keys]
    co = COracle()
    co.set_keyring(col.Keyring(keyring=ring))
    status = []
    for c in cases:
        st = RS.oracle_status(ring, c)
        tr, nv, err = co.trace_item(c.tbs, c.sig)
        assert tr == [st] and nv == (1 if st == RS.ST_OK else 0), (c.bits, c.hash_id, c.variant, st, tr)
        assert st in (RS.ST_OK, RS.ST_BAD_SIG)
        status.append(st)

    # every cell: five hashes under every key; the boundary k = tLen + 11 lies where the table says
    cells = Counter((c.key, c.hash_id) for c in cases)
    assert len(cells) == N_KEYS * len(RS.HASHES)
    for c in cases:
        k = (c.bits + 7) // 8
        assert c.fits == (k >= RS.t_len(dict(RS.HASHES)[c.hash_id]) + 11)
    boundary = {"sha1": (360, 368), "sha224": (456, 464), "sha256": (488, 496), "sha384": (616, 624), "sha512": (744, 752)}
    for hash_id, name in RS.HASHES:
        below, at = boundary[name]
        assert {c.fits for c in cases if c.bits == below and c.hash_id == hash_id} == {False}
        assert {c.fits for c in cases if c.bits == at and c.hash_id == hash_id} == {True}
    assert not any(c.fits for c in cases if c.bits == 256)

    # the untouched signature is accepted wherever an encoding exists; without one everything is refused
    for c, st in zip(cases, status):
        if c.variant == "untouched" and c.fits:
            assert st == RS.ST_OK, (c.bits, c.hash_id)
        if not c.fits:
            assert st == RS.ST_BAD_SIG, (c.bits, c.hash_id, c.variant)
    assert sum(1 for c in cases if c.variant == "untouched") == len(cells)

    # Every variant, overall and in each size class: accepted at least once where it can be accepted at all (a value congruent to
    # the signature: the reference reduces it, over the cap too), refused at least once where it can be refused (a wrong value
    # anywhere; a congruent one only under a modulus too short for the hash, and those are all below 2048 bits).
    congruent = ["untouched", "canonical mpi", "s + n", "s + n, long", "at the cap", "over the cap"]
    wrong = ["bit flipped", "em 00 02", "em FE above byte 84", "em FE below byte 84", "em separator FF", "em other prefix"]
    assert {c.variant for c in cases} == set(congruent + wrong)
    tally = Counter((RS.size_class(c.bits), c.variant, st) for c, st in zip(cases, status))
    for cls in (0, 1, 2):
        for v in congruent:
            assert tally[(cls, v, RS.ST_OK)] > 0, (cls, v)
            assert tally[(cls, v, RS.ST_BAD_SIG)] == 0 or cls == 0, (cls, v)
        for v in wrong:
            assert tally[(cls, v, RS.ST_BAD_SIG)] > 0 and tally[(cls, v, RS.ST_OK)] == 0, (cls, v)
    for v in ("untouched", "canonical mpi", "s + n", "s + n, long", "bit flipped"):
        assert tally[(0, v, RS.ST_BAD_SIG)] > 0, v                      # under a modulus too short for the hash
        assert tally[(None, v, RS.ST_OK)] + tally[(None, v, RS.ST_BAD_SIG)] > 0, v     # under a key above 4096 bits
    # e = 3 and e = 17 verify in every class
    for kp_i, kp in enumerate(keys):
        if kp.e != 65537:
            assert any(c.key == kp_i and st == RS.ST_OK and c.variant == "at the cap" for c, st in zip(cases, status)), kp.name
    assert sorted((kp.e, RS.size_class(kp.n.bit_length())) for kp in keys if kp.e != 65537) == [(3, 0), (3, 1), (3, 2), (17, 0), (17, 1), (17, 2)]
    # what the device is expected to fence: every case under the two keys above 4096 bits, every over-the-cap value
    fenced = [RS.device_expectation(c, st)[1] for c, st in zip(cases, status)]
    # (an over-the-cap value under a modulus too short for the hash is refused by the reference like any other: no fence)
    assert sum(fenced) == sum(1 for c in cases if c.bits > RS.MAX_BITS) + sum(1 for c in cases if c.over_cap and c.fits)
    assert all(st == (RS.ST_OK if c.fits else RS.ST_BAD_SIG) for c, st in zip(cases, status) if c.over_cap)
    assert sum(1 for c in cases if c.over_cap and not c.fits) >= 20


def test_oracles_agree_under_extremal_prime_moduli():
    """The keys of tests/extremal_keys.py (prime moduli with every limb full / almost every limb zero, e = 65537, 3 and 17) in
    the value shapes of cell_cases: Python integers and OpenSSL bignums give every case the same status, the untouched signature
    is accepted in every (key, hash) cell and every wrong value refused.  If the C oracle refuses a prime modulus the assertion
    on its trace says so."""
    from tests import extremal_keys as X
    keys, cases = X.rsa_keys(), X.rsa_cases()
    assert len(keys) == 14 and all(RS.size_class(kp.n.bit_length()) is not None for kp in keys)
    ring = [RS.entity(kp) for kp in keys]
    co = COracle()
    co.set_keyring(col.Keyring(keyring=ring))
    tally = Counter()
    for c in cases:
        st = RS.oracle_status(ring, c)
        tr, nv, err = co.trace_item(c.tbs, c.sig)
        assert tr == [st] and nv == (1 if st == RS.ST_OK else 0), "the C oracle differs: %r" % ((c.bits, keys[c.key].name, c.hash_id, c.variant, st, tr),)
        assert c.fits
        tally[(c.key, c.hash_id, c.variant, st)] += 1
    congruent = ["untouched", "canonical mpi", "at the cap", "over the cap"]
    for ki in range(len(keys)):
        for hash_id, _ in RS.HASHES:
            for v in congruent:
                assert tally[(ki, hash_id, v, RS.ST_OK)] == 1, (keys[ki].name, hash_id, v)
            assert tally[(ki, hash_id, "s + n", RS.ST_OK)] + tally[(ki, hash_id, "s + n, long", RS.ST_OK)] == 1
            assert tally[(ki, hash_id, "bit flipped", RS.ST_BAD_SIG)] == 1
            assert sum(n for (k, h, v, st), n in tally.items() if (k, h) == (ki, hash_id) and v.startswith("em ") and st == RS.ST_BAD_SIG) == 1
    assert sum(tally.values()) == len(cases) == 14 * 5 * 7
