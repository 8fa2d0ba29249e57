"""Holds the cases of tests/dsa_pipeline_cases.py to what they claim to be, on the CPU: the chosen-digit signatures verify under the
oracle and carry the exponent they were made for, the digit vectors are the ones the kernels' branches need, the hostile keys'
rules follow from their numbers, and the inversion runs hold what poisons a batched product.  tests/test_gpu_dsa_pipeline.py runs
the same cases on the device."""
import functools
import json
import math
import os

import pytest

from oracle import openpgp as pgp
from tests import dsa_pipeline_cases as P


@functools.lru_cache(maxsize=None)
def _statuses(wbits, mixed):
    return P.oracle_statuses(P.ring(wbits, mixed))


RINGS = [(w, False) for w in P.WIDTHS] + [(w, True) for w in (8, 13, 16)]


@pytest.mark.parametrize("wbits,mixed", RINGS)
def test_chosen_digit_cases_verify_and_carry_their_exponent(wbits, mixed):
    rg = P.ring(wbits, mixed)
    st = _statuses(wbits, mixed)
    assert len(rg.cases) == 2 * len(rg.keys) and len({kp.key_id for kp in rg.keys}) == len(rg.keys)
    assert P.ring_bytes(rg.keys, wbits) < P.RING_CAP == 16 * 10 ** 9
    for c, s in zip(rg.cases, st):
        kp = rg.keys[c.key]
        assert s == (pgp.ST_OK if c.kind == "valid" else pgp.ST_BAD_SIG), (c.label, s)
        if c.kind == "valid":
            u1, u2, _ = P.exponents(kp, c.payload, c.sig)
            assert (u2 if c.which == "u2" else u1) == c.target, c.label
            assert pow(kp.g, kp.x, kp.p) == kp.y and 0 < c.target < kp.q
    assert sorted({c.hash_id for c in rg.cases}) == [2, 8, 10]
    assert {c.which for c in rg.cases} == {"u1", "u2"}


def test_ring_sizes():
    """Twelve keys up to 17 bits, six at 18; a mixed ring holds both size classes, all three up to 13 bits."""
    for w in P.WIDTHS:
        assert len(P.ring(w).keys) == (6 if w == 18 else 12), w
        assert all(kp.p.bit_length() == 2048 for kp in P.ring(w).keys)
        assert len(P.ring(w).keys) == 12 or (len(P.ring(w).keys) + 2) * P.slot_bytes(w, 76) >= P.RING_CAP     # cut by the cap alone
        assert {c.label.split(" ")[0] for c in P.ring(w).cases} >= set(P.SMALL_2048[:2 if w == 18 else 3])
    for w in (8, 13):
        assert sorted(kp.p.bit_length() for kp in P.ring(w, True).keys) == [1024] * 12 + [2048] * 12 + [3072] * 12
    assert sorted(kp.p.bit_length() for kp in P.ring(16, True).keys) == [2048] * 4 + [3072] * 2
    assert P.slot_bytes(18, 76) == (2 * 15 * 262143 * 76 + 772) * 4 and P.slot_bytes(16, 112) == (2 * 16 * 65535 * 112 + 1132) * 4


@pytest.mark.parametrize("wbits", P.WIDTHS)
@pytest.mark.parametrize("gname", ("dsa2048", "dsa1024"))
def test_digit_vectors_are_as_described(wbits, gname):
    w, q = wbits, P.groups()[gname].q
    nwin = (256 + w - 1) // w                       # the windows the device walks, whatever the order's width
    vec = {label: [P.digit(t, w, j) for j in range(nwin)] for label, t in P.digits(w, q)}
    full = (1 << w) - 1
    nz = lambda v: [j for j, d in enumerate(v) if d]          # noqa: E731
    assert nz(vec["1"]) == [0] and vec["1"][0] == 1
    assert nz(vec["window 0 full"]) == [0] and vec["window 0 full"][0] == full
    j = nz(vec["straddling window full"])
    assert len(j) == 1 and vec["straddling window full"][j[0]] == full and j[0] >= 1
    crosses = [k for k in range(nwin) if (w * k) % 32 + w > 32 and w * k + w <= 256]
    assert (w in (4, 8, 16)) == (not crosses)
    if crosses:
        assert j[0] == crosses[0] and (w * j[0]) // 32 != (w * j[0] + w - 1) // 32        # its bits lie in two words
    else:
        assert j[0] == 1
    top = nz(vec["top window alone"])
    assert len(top) == 1 and top[0] == (q.bit_length() - 1) // w          # the first non-zero digit comes as late as it can
    assert all(vec[label][k] == 0 for label in ("1", "window 0 full", "straddling window full") for k in range(top[0], nwin))   # empty top windows
    ev = vec["even windows full"]
    assert all(d == 0 for d in ev[1::2]) and all(d in (0, full) for d in ev[0::2]) and sum(d == full for d in ev) >= top[0] // 2
    assert 4 * sum(P.digit(q - 1, w, k) != 0 for k in range(nwin)) >= 3 * (top[0] + 1) and P.digit(q - 1, w, top[0])   # q - 1: a dense vector, top window at work
    if q.bit_length() == 160:
        assert all(v[k] == 0 for v in vec.values() for k in range((160 + w - 1) // w, nwin))


def test_digests_fall_on_both_sides_of_an_order_just_above_2_255():
    """k_dsa_mul subtracts q from z when the digest, cut to 256 bits, is not below q.  The order of p2048_q256_low lies within
    2^215 of 2^255 (dsa2048_low of extremal_moduli.json has q = 2^256 - 189: under it z >= q does not happen)."""
    q = P.groups()["p2048_q256_low"].q
    assert 0 < q - (1 << 255) < 1 << 215 and (1 << 256) - P.groups()["dsa2048_low"].q == 189
    zs = []
    for w in P.WIDTHS:
        rg = P.ring(w)
        for c in rg.cases:
            if c.kind == "valid" and c.label.startswith("p2048_q256_low "):
                zs.append(P.exponents(rg.keys[c.key], c.payload, c.sig)[2])
    above = sum(z >= q for z in zs)
    assert len(zs) >= 40 and 4 * above >= len(zs) and 4 * (len(zs) - above) >= len(zs), (len(zs), above)


def test_sparse_wave():
    rg = P.sparse_wave()
    st = P.oracle_statuses(rg)
    assert [s for s in st] == [pgp.ST_OK, pgp.ST_BAD_SIG] * 17 and len(rg.keys) == 17
    for c in rg.cases[:32:2]:
        u2 = P.exponents(rg.keys[c.key], c.payload, c.sig)[1]
        assert [j for j in range(20) if P.digit(u2, 13, j)] == [7] and u2 == c.target
    assert len({P.digit(c.target, 13, 7) for c in rg.cases[:32]}) == 16
    assert P.exponents(rg.keys[16], rg.cases[32].payload, rg.cases[32].sig)[1] == rg.keys[16].q - 1
    assert P.ring_bytes(rg.keys, 13) < P.RING_CAP


# ---- family B

@functools.lru_cache(maxsize=None)
def _hostile():
    rg = P.hostile_ring()
    return rg, P.oracle_statuses(rg)


def test_rule_follows_from_the_keys_numbers():
    rg, _ = _hostile()
    turned_away = set()
    for c in rg.cases:
        kp = rg.keys[c.key]
        pb, qb = kp.p.bit_length(), kp.q.bit_length()
        cap = 2048 if pb <= 2048 else 3072
        unsupported = pb < 2 or pb > 3072 or qb < 32 or qb > 256 or kp.q % 2 == 0 or kp.p % 2 == 0 or kp.g.bit_length() > cap or kp.y.bit_length() > cap
        assert c.rule == ("unsupported" if unsupported else "oracle"), c.label
        if unsupported:
            turned_away.add(kp.name.split(" <")[0])
    assert turned_away == {"p512_q8", "p_is_1", "p512_q24", "p1024_q264", "even_q", "even_p", "p1016_q160, y over the cap",
                           "p2048_q256_low, y over the cap"}
    names = [kp.name.split(" <")[0] for kp in rg.keys]
    assert set(P.VERIFY_GROUPS + P.PIPELINE_GROUPS) <= set(names) and len(names) == len(P.VERIFY_GROUPS + P.PIPELINE_GROUPS) + 16
    gs = P.groups()
    assert [gs[n].q.bit_length() for n in ("p1024_q32", "p1024_q40", "p1024_q248", "p512_q24", "p1024_q264", "composite_q256")] == [32, 40, 248, 24, 264, 256]
    assert gs["composite_q256"].q % 15 == 0 and gs["composite_q256"].p.bit_length() == 2048 and gs["p_is_3"].p == 3 and gs["p_is_3"].q % 2 == 1
    assert gs["even_q"].q % 2 == 0 and gs["even_p"].p % 2 == 0
    g = gs["composite_q256"]
    assert pow(g.g, g.q, g.p) == 1 and all(pow(g.g, g.q // f, g.p) != 1 for f in (3, 5, g.q // 15))


def test_every_group_that_can_sign_has_an_accepted_case():
    rg, st = _hostile()
    ok = {rg.keys[c.key].name.split(" <")[0] for c, s in zip(rg.cases, st) if s == pgp.ST_OK and c.rule == "oracle"}
    assert set(P.HONEST_GROUPS) <= ok, set(P.HONEST_GROUPS) - ok
    assert {"p1024_q32", "p1024_q40", "p768_q64", "p1024_q248", "composite_q160", "composite_q256"} <= ok
    assert {"%s, %s" % (g, v) for g in P.VARIANT_GROUPS for v in ("y + p", "g + p")} <= ok           # reduced mod p, then verified
    assert not ok & {"q161", "p_is_3"}
    for c, s in zip(rg.cases, st):
        name = rg.keys[c.key].name.split(" <")[0]
        if c.kind == "twin" or name in ("q161", "p_is_3") or name.split(", ")[-1] in ("y = 0", "y = 1", "y = p - 1", "g = 0", "g = 1"):
            assert s != pgp.ST_OK, c.label
        if c.kind == "honest" and c.rule == "oracle" and name in P.HONEST_GROUPS:
            assert s == pgp.ST_OK, c.label
        assert s in (pgp.ST_OK, pgp.ST_BAD_SIG), (c.label, s)          # every case reaches the arithmetic


# ---- family C

def test_inversion_runs_hold_what_poisons_a_product():
    rg = P.inversion_runs()
    st = P.oracle_statuses(rg)
    assert len(rg.cases) == P.N_RUN_ITEMS and P.N_RUN_ITEMS % 16 == 1 and 550 <= P.N_RUN_ITEMS <= 650
    for ki, name in enumerate(P.INVERSION_KEYS):
        kp = rg.keys[ki]
        mine = [(c, s) for c, s in zip(rg.cases, st) if c.key == ki]
        classes = {"valid": 0, "no inverse": 0, "range": 0, "other": 0}
        product = 1
        for c, s in mine:
            _, r, s_ = P.read_packet(c.sig)
            in_range = 0 < r < kp.q and 0 < s_ < kp.q
            if in_range:
                product = product * s_ % kp.q
            cls = "range" if not in_range else "no inverse" if math.gcd(s_, kp.q) != 1 else "valid" if s == pgp.ST_OK else "other"
            classes[cls] += 1
            assert (cls == "valid") == (s == pgp.ST_OK) and (cls == c.kind or (cls, c.kind) in (("valid", "honest"), ("other", "flipped"))), (c.label, cls)
        if name.startswith("composite"):
            assert classes["valid"] > 100 and classes["range"] > 5 and classes["other"] == 0, classes
            assert 6 * classes["no inverse"] < len(mine) < 11 * classes["no inverse"], classes                # one in eight
            assert math.gcd(product, kp.q) != 1 and kp.q % 3 == 0
        else:
            assert classes["valid"] > 20 and classes["no inverse"] == 0 and classes["other"] > 0, classes
    assert sum(c.key < 2 for c in rg.cases) > 400


def test_the_generator_reproduces_the_groups():
    import runpy
    build = runpy.run_path(os.path.join(P.GOLDEN, "make_dsa_pipeline_groups.py"))["build"]
    with open(os.path.join(P.GOLDEN, "dsa_pipeline_groups.json")) as f:
        committed = f.read()
    assert build() == committed
    assert [g["name"] for g in json.loads(committed)["groups"]] == ["p1024_q32", "p1024_q40", "p1024_q248", "p2048_q256_low", "p512_q24", "p1024_q264",
                                                                    "composite_q256", "p_is_3", "even_q", "even_p"]
