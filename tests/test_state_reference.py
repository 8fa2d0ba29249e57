"""What the characters of tests/state_cases.py claim, asserted on the CPU: the property each pipeline character stands for, the
good / bad outcome of every operation of the other entries, and the COMPLEMENT CONDITION -- for every designated pair of the
call-order tests the reference answers of predecessor and successor differ in every compared field of every item (operation) they
share by index, so that a stale read can never coincide with the right answer.  That is a condition on the characters, asserted
at 100 %: a weak pair fails here instead of passing silently on the device."""
import math

import numpy as np
import pytest

from oracle import openpgp as pgp
import state_cases as S


def _sigs(stream):
    """the signature packets the reference's reader parses out of a stream"""
    out, pos = [], 0
    while True:
        p = pgp.packet_read_stream(stream, pos)
        if p.kind == "eof" or p.pos <= pos:
            return out
        if p.kind == "sig":
            out.append(p.sig)
        pos = p.pos


def _one(name):
    ch = S.character(name)
    assert len(ch.calls) == 1
    return ch.calls[0], ch.refs[0]


def test_the_ring_holds_what_the_characters_need():
    R = S.ring()
    assert len(R.cluster.replicas) == 13 and all(k.algo == S.cb.PK_RSA and k.n.bit_length() == 2048 for k in R.cluster.replicas)
    assert R.cluster.suff == 9 and R.quorum.qcs[0].suff == 9 and len(R.quorum.qcs) == 1
    assert R.rsa3072.n.bit_length() == 3072 and R.rsa4096.n.bit_length() == 4096
    assert [(k.p.bit_length(), k.q.bit_length()) for k in R.dsa2048 + R.dsa3072] == [(2048, 256)] * 2 + [(3072, 256)] * 2
    assert len(R.keyring.keyring) == 19 and len({e.id for e in R.keyring.keyring}) == 19
    members = set(R.quorum.qcs[0].nodes)
    assert members == {k.key_id for k in R.cluster.replicas}


@pytest.mark.parametrize("name", S.PIPELINE)
def test_sizes_stay_small(name):
    for call in S.character(name).calls:
        items, events, ss_bytes, _ = S.size(call)
        assert items <= S.N_ITEMS and events <= 1500 and ss_bytes < 400000


def test_plain_is_sufficient_everywhere():
    call, ref = _one("plain")
    assert len(call.tbs) == S.N_ITEMS and not ref.err.any() and (ref.nver == 9).all() and (ref.verdict & S.V_IS_SUFFICIENT).all()
    assert all(set(st) == {pgp.ST_OK} for st in ref.statuses) and not ref.sig_err.any()
    for s in call.ss:
        assert {(g.hash_id, g.sig_type, g.pk_algo) for g in _sigs(s)} == {(8, 0, 1)}


def test_all_bad_holds_no_ok_status_and_every_refusal():
    call, ref = _one("all_bad")
    plain = _one("plain")[0]
    assert call.tbs == plain.tbs and [S.count_events(s) for s in call.ss] == [S.count_events(s) for s in plain.ss]
    seen = set()
    for st, s in zip(ref.statuses, call.ss):
        assert pgp.ST_OK not in st and len(st) == S.count_events(s)          # never sufficient: the reference reads every packet
        seen.update(st)
    assert {pgp.ST_BAD_SIG, pgp.ST_HASH_TAG, pgp.ST_UNKNOWN_ISSUER} <= seen and len(seen) >= 4, seen
    assert (ref.err == S.ERR_INSUFFICIENT).all() and not ref.nver.any() and not (ref.verdict & S.V_IS_SUFFICIENT).any()
    assert (ref.sig_err == S.ERR_INVALID).all()


def test_other_hashes_names_each_hash_in_both_modes():
    call, ref = _one("other_hashes")
    seen = set()
    for s in call.ss:
        seen.update((g.hash_id, g.sig_type) for g in _sigs(s))
    assert seen >= set(S.OTHER_HASHES) and {h for h, _ in seen} >= {2, 8, 9, 10, 11}
    assert (ref.nver == 8).all() and (ref.err == S.ERR_INSUFFICIENT).all()
    assert all(sorted(st) == [pgp.ST_OK] * 8 + [pgp.ST_BAD_SIG] for st in ref.statuses)
    assert any(b"\r" in t or b"\n" in t for t in call.tbs)


def test_wide_holds_a_value_of_each_length():
    call, ref = _one("wide")
    lengths = set()
    assert all(g.pk_algo == 1 for s in call.ss for g in _sigs(s))
    for s in call.ss:
        for pkt in S.packets_of(s):
            _, tag_at = S._split(pkt)
            nb = (int.from_bytes(pkt[tag_at + 2:tag_at + 4], "big") + 7) // 8
            assert nb == len(pkt) - tag_at - 4 and pkt[tag_at + 4] != 0
            lengths.add(nb)
    assert lengths == set(S.WIDE_LENGTHS) and min(lengths) > S.RSA29_CAP_BYTES and max(lengths) * 8 <= 2128
    assert (ref.nver == 8).all() and (ref.err == S.ERR_INSUFFICIENT).all()
    assert all(sorted(st) == [pgp.ST_OK] * 8 + [pgp.ST_BAD_SIG] for st in ref.statuses)


def test_all_lists_fills_four_work_lists_in_every_item():
    R = S.ring()
    call, ref = _one("all_lists")
    bits = {k.key_id: (k.algo, (k.n or k.p).bit_length()) for k in list(R.cluster.replicas) + [R.rsa3072, R.rsa4096] + list(R.dsa2048) + list(R.dsa3072)}
    both = set()
    for s, st in zip(call.ss, ref.statuses):
        kinds = [bits[g.issuer] for g in _sigs(s)]
        assert set(kinds) >= {(1, 2048), (1, 3072), (1, 4096)} and {k for k in kinds if k[0] == 17} and len(kinds) == 13
        both.update(k for k in kinds if k[0] == 17)
        assert st == [pgp.ST_OK] * 13                                       # the quorum is found at the last packet only
    assert both == {(17, 2048), (17, 3072)}
    assert not ref.err.any() and (ref.nver == 13).all() and (ref.verdict & S.V_IS_SUFFICIENT).all()


def test_partial_uses_partial_body_lengths_and_nothing_fenced():
    call, ref = _one("partial")
    n_partial = 0
    for s in call.ss:
        assert pgp.fence_reason(s) is None
        pos = 0
        while pos < len(s):
            n_partial += s[pos] == 0xC2 and 224 <= s[pos + 1] < 255
            pos = pgp.packet_read_stream(s, pos).pos
    assert n_partial > 4 * S.N_ITEMS
    assert not ref.err.any() and (ref.nver == 9).all() and all(set(st) == {pgp.ST_OK} for st in ref.statuses)


def test_long_items_exceed_the_walk_row():
    call, ref = _one("long_items")
    assert len(call.ss) == 3 and all(S.count_events(s) > S.WALK_CAP_MAX for s in call.ss)
    assert all(pgp.fence_reason(s) is None for s in call.ss)
    assert not ref.err.any() and (ref.nver == 9).all()


def test_empty_has_no_packet_at_all_and_a_one_item_call():
    ch = S.character("empty")
    assert len(ch.calls) == 2
    assert len(ch.calls[0].tbs) == S.N_ITEMS and not any(ch.calls[0].ss)
    assert (ch.refs[0].err == S.ERR_INSUFFICIENT).all() and not ch.refs[0].nver.any() and all(st == [] for st in ch.refs[0].statuses)
    assert len(ch.calls[1].tbs) == 1 and ch.refs[1].err[0] == S.ERR_INSUFFICIENT and ch.refs[1].nver[0] == 7


def test_fenced_shapes_and_their_plain_neighbours():
    call, ref = _one("fenced")
    assert int(ref.fenced.sum()) == len(S.FENCED_NAMES) == 7
    for i, s in enumerate(call.ss):
        why = pgp.fence_reason(s)
        if not ref.fenced[i]:
            assert why is None and ref.err[i] == 0 and ref.nver[i] == 9
        elif i // 3 < 4:
            assert why in ("unread", "bounds"), (i, why)                    # the structural fences; MD5, value >= R and nesting are semantic
        else:
            assert why is None


def test_phase2_exits_behind_the_phase_1_window():
    call, ref = _one("phase2")
    members = {k.key_id for k in S.ring().cluster.replicas}
    window = 9 + S.PHASE_MARGIN
    assert S.PHASE_MARGIN == 1 + 9 // 64 == 1
    for s, st in zip(call.ss, ref.statuses):
        sigs = _sigs(s)
        assert len(sigs) == S.count_events(s) and all(g.issuer in members for g in sigs)      # every packet counts towards the window
        assert set(st) <= {pgp.ST_OK, pgp.ST_HASH_TAG, pgp.ST_BAD_SIG}
        assert st.count(pgp.ST_OK) == 9 and st[-1] == pgp.ST_OK and len(st) > window
        assert st[:window].count(pgp.ST_OK) < 9
    assert not ref.err.any() and (ref.nver == 9).all()


def test_complement_condition_of_the_pipeline_pairs():
    assert set(S.COMPLEMENT_PAIRS) == {("all_bad", "plain"), ("other_hashes", "plain"), ("wide", "plain"), ("plain", "all_bad"), ("plain", "other_hashes"),
                                       ("plain", "wide"), ("all_lists", "empty")}
    for pred, succ in S.COMPLEMENT_PAIRS:
        p = S.character(pred)
        for sref in S.character(succ).refs:
            for pref in p.refs:
                n = min(len(pref.err), len(sref.err))
                assert n and (pref.err[:n] != sref.err[:n]).all(), (pred, succ)
                assert (pref.verdict[:n] != sref.verdict[:n]).all(), (pred, succ)
                assert (pref.sig_err[:n] != sref.sig_err[:n]).all(), (pred, succ)
    # behind `fenced` the condition can hold only where the reference speaks and only against the insufficient characters: its plain
    # neighbours (two of every three items) differ from all_bad, other_hashes and wide in every compared byte
    f = S.character("fenced").refs[0]
    for succ in ("all_bad", "other_hashes", "wide"):
        sref = S.character(succ).refs[0]
        n = min(len(f.err), len(sref.err))
        ok = f.fenced[:n] == 0
        assert ok.sum() == 14
        for a, b in ((f.err, sref.err), (f.verdict, sref.verdict), (f.sig_err, sref.sig_err)):
            assert (a[:n][ok] != b[:n][ok]).all(), ("fenced", succ)


# ---- the other entry points ------------------------------------------------------------------------------------------------
WORST = {"lagrange_combine_small": 1, "lagrange_combine_big": 1, "lagrange_combine_huge": 2, "dsa_calculate_r": 1, "modinv": 1, "ec_scalar_base_mult": 2,
         "ecdsa_verify": 2, "ecdsa_verify_keyset": 2, "dsa_verify": 2, "dsa_verify_keyset": 2, "rsa_verify": 2, "rsa_verify_keyset": 2,
         "rsa_sign_keyset": 4, "rsa_partial_sign": 1}
"""The status every operation of `bad` ends with: 1 = no inverse (a composite modulus; v = 0 mod q; a negative fragment of a request
whose em shares the factor 3 with its modulus), 2 = fenced (integers beyond 2128 bits, a scalar of N or more, a key off the curve,
a digest longer than the order, an even modulus), 4 = the check failed (a signature under a key whose qinv is off by one: s^e != em,
and no byte of s leaves the device).  ecdsa_calculate_r mixes both (a partial R off the curve; v = 0 mod N).  The entries that are
not listed have no per-operation failure."""
NAMES = [e.name for e in S.ENTRIES]


def _zero(v):
    return not any(v) if isinstance(v, (bytes, bytearray, list, tuple, np.ndarray)) else v == 0


@pytest.mark.parametrize("name", NAMES)
def test_good_succeeds_and_bad_ends_the_worst_way(name):
    e = S.ENTRY[name]
    for n in S.SIZES:
        good, bad = S.op_reference(name, "good", n), S.op_reference(name, "bad", n)
        assert all(len(v) == n for v in good.values()) and all(len(v) == n for v in bad.values())
        if "status" in good:
            assert not np.asarray(good["status"]).any()
        if "valid" in good:
            assert (good["valid"] == 1).all() and not bad["valid"].any()
        if name in WORST:
            assert (bad["status"] == WORST[name]).all(), name
        elif name == "ecdsa_calculate_r":
            assert set(bad["status"].tolist()) == {1, 2}
        else:
            assert "status" not in bad or not np.asarray(bad["status"]).any()
        if name in WORST or name == "ecdsa_calculate_r":                      # zeroes beside a status that is not 0
            for f in ("out", "sig"):
                if f in bad:
                    assert all(_zero(v) for v in bad[f] if v is not S.UNCLAIMED), name
                    assert (name in ("lagrange_combine_small", "dsa_calculate_r")) == any(v is S.UNCLAIMED for v in bad[f]), name
        for f in e.compared:
            if f not in ("status", "valid"):
                assert not any(_zero(v) for v in good[f]), (name, f)


@pytest.mark.parametrize("name", NAMES)
def test_complement_condition_of_the_same_entry_pairs(name):
    """bad(141) -> good(70) and good(141) -> bad(70): every compared field differs at every shared operation"""
    e = S.ENTRY[name]
    for pk, sk in (("bad", "good"), ("good", "bad")):
        pred, succ = S.op_reference(name, pk, S.SIZES[1]), S.op_reference(name, sk, S.SIZES[0])
        for f in e.compared:
            for i in range(S.SIZES[0]):
                a, b = pred[f][i], succ[f][i]
                if a is S.UNCLAIMED or b is S.UNCLAIMED:
                    assert "status" in e.compared          # no reference row: the status byte carries the pair
                    continue
                assert not np.array_equal(a, b), (name, f, i)
    if not ({"status", "valid"} & set(e.compared)):
        # no per-operation failure: `bad` is `good` under other moduli and operands; no result row of one appears in the other
        for f in e.compared:
            rows = lambda r: {repr(v) for v in r[f]}                                   # noqa: E731
            assert not (rows(S.op_reference(name, "good", 141)) & rows(S.op_reference(name, "bad", 141))), (name, f)


@pytest.mark.parametrize("name", S.VERIFY)
def test_invalid_is_status_0_beside_validity_0_and_no_inverse_under_a_composite_q(name):
    """The third kind of the verify entries: every operation invalid, status 0 (dsa_verify: status 1 under the composite q, every second
    operation).  Against `good` the validity byte differs at every shared operation, against `bad` the status byte."""
    for n in S.SIZES:
        inv = S.op_reference(name, "invalid", n)
        assert len(inv["valid"]) == n and not inv["valid"].any()
        if name.startswith("dsa"):
            assert set(inv["status"].tolist()) == {0, 1} and abs(int((inv["status"] == 1).sum()) - n // 2) <= 1
        else:
            assert not inv["status"].any()
    for a, b in (("invalid", "good"), ("good", "invalid"), ("invalid", "bad"), ("bad", "invalid")):
        pred, succ = S.op_reference(name, a, 141), S.op_reference(name, b, 70)
        f = "valid" if "good" in (a, b) else "status"
        assert (pred[f][:70] != succ[f]).all(), (name, a, b)


def test_refused_signatures_are_fenced_and_invalid_input_in_turn():
    """The third kind of rsa_sign_keyset: under an even-p key BFTKV_TH_FENCED (2), under a 368-bit key the length rule's
    BFTKV_TH_INVALID_INPUT (3), alternating, zeroes beside both.  Against `good` (0) and against `bad` (4) the status byte differs
    at every shared operation, and so does the row against `good`."""
    assert S.THIRD_KIND["rsa_sign_keyset"] == "refused"
    keys = S._rsas_keys("refused")
    assert keys[0].p % 2 == 0 and keys[0].n % 2 == 1 and keys[1].n.bit_length() <= 408 and (keys[1].n.bit_length() + 7) // 8 < 51 + 11
    assert keys[1].n == keys[1].p * keys[1].q and keys[1].p % 2 == 1 and keys[1].q % 2 == 1           # refused by the length alone
    for n in S.SIZES:
        r = S.op_reference("rsa_sign_keyset", "refused", n)
        assert len(r["status"]) == n and set(r["status"].tolist()) == {S.TH_FENCED, S.TH_INVALID_INPUT}
        assert (r["status"][0::2] == r["status"][0]).all() and (r["status"][1::2] == r["status"][1]).all() and r["status"][0] != r["status"][1]
        assert not any(r["sig"])
    for a, b in (("refused", "good"), ("good", "refused"), ("refused", "bad"), ("bad", "refused")):
        pred, succ = S.op_reference("rsa_sign_keyset", a, 141), S.op_reference("rsa_sign_keyset", b, 70)
        assert (pred["status"][:70] != succ["status"]).all(), (a, b)
        if "good" in (a, b):
            assert all(x != y for x, y in zip(pred["sig"][:70], succ["sig"])), (a, b)


def test_positive_fragments_need_no_inverse():
    """The third kind of rsa_partial_sign: no negative fragment in the whole call, status 0, no row zero.  Against `bad` status
    and row differ at every shared fragment, against `good` the row."""
    assert S.THIRD_KIND["rsa_partial_sign"] == "positive"
    for n in S.SIZES:
        i, r = S.op_input("rsa_partial_sign", "positive", n), S.op_reference("rsa_partial_sign", "positive", n)
        assert len(i["frags"]) == n and not any(sb for _, sb, _, _ in i["frags"])
        assert not r["status"].any() and all(r["out"])
    for a, b in (("positive", "good"), ("good", "positive"), ("positive", "bad"), ("bad", "positive")):
        pred, succ = S.op_reference("rsa_partial_sign", a, 141), S.op_reference("rsa_partial_sign", b, 70)
        assert all(x != y for x, y in zip(pred["out"][:70], succ["out"])), (a, b)
        if "bad" in (a, b):
            assert (pred["status"][:70] != succ["status"]).all(), (a, b)


def test_the_partial_sign_calls_have_the_shape_the_host_sort_needs():
    """Two or three fragments per request, handed over out of request order; exp_used over three widths, every magnitude exactly as
    wide as it says; good: both signs, and at least a quarter of the requests without a negative fragment; bad: every fragment negative
    and non-zero under a modulus of at most 2048 bits that 3 divides."""
    for kind in ("good", "bad", "positive"):
        for n in S.SIZES + (1,):
            i = S.op_input("rsa_partial_sign", kind, n)
            per = {}
            for r, sb, mag, used in i["frags"]:
                per.setdefault(r, []).append(sb)
                assert used in S.PSIGN_WIDTHS and (mag.bit_length() + 7) // 8 == used and mag > 0
            assert sorted(per) == list(range(len(i["t"]))) and all(len(t) == 51 for t in i["t"])
            if n == 1:
                assert kind == "positive" or i["frags"][0][1] != 0                      # the one-fragment call takes the inversion
                continue
            assert set(len(per[r]) for r in sorted(per)[:-1]) == {2, 3} and len(per) < n
            assert [f[0] for f in i["frags"]] != sorted(f[0] for f in i["frags"])
            assert {f[3] for f in i["frags"]} == set(S.PSIGN_WIDTHS)
            assert [f[3] for f in i["frags"]] != sorted((f[3] for f in i["frags"]), reverse=True)      # the longest-first order moves rows
            if kind == "good":
                assert {bool(sb) for v in per.values() for sb in v} == {False, True}
                assert 4 * sum(not any(v) for v in per.values()) >= len(per)
            elif kind == "bad":
                assert all(sb for v in per.values() for sb in v) and all(m % 3 == 0 and m % 2 == 1 and m.bit_length() <= 2048 for m in i["mods"])


def test_the_share_requests_of_the_two_kinds():
    """tdsa_share: good under group 0, bad under group 1, with share columns at or above q in `bad`; tecdsa_share: two disjoint
    request pools on one curve; tsig_partial_s: two odd orders per kind, the operands of `bad` at or above q."""
    for n in S.SIZES:
        g, b = S.op_input("tdsa_share", "good", n), S.op_input("tdsa_share", "bad", n)
        assert (g["gi"], b["gi"]) == (0, 1) and g["groups"] == b["groups"] and len(g["groups"]) == 2
        assert all(len(sh) == S.TSIG_M for sh in g["reqs"] + b["reqs"])
        q1 = b["groups"][1][1]
        assert any(all(v >= q1 for tup in sh for v in tup) for sh in b["reqs"])
        g, b = S.op_input("tecdsa_share", "good", n), S.op_input("tecdsa_share", "bad", n)
        assert not {repr(sh) for sh in g["reqs"]} & {repr(sh) for sh in b["reqs"]}
        g, b = S.op_input("tsig_partial_s", "good", n), S.op_input("tsig_partial_s", "bad", n)
        assert not set(g["q"]) & set(b["q"]) and all(q % 2 == 1 and q.bit_length() <= 256 for q in g["q"] + b["q"]) and len(set(g["q"] + b["q"])) == 4
        assert all(v < g["q"][i] for o, i in zip(g["ops"], g["idx"]) for v in o)
        assert all(b["q"][i] <= v < 1 << 256 for o, i in zip(b["ops"], b["idx"]) for v in o)
    assert S.partial_s_orders("good")[0].bit_length() == 256 and S.partial_s_orders("good")[1] == S._curve()[1]["n"]


def test_no_signature_of_the_signing_entry_is_a_signature_of_the_verify_pool():
    """rsa_sign_keyset behind rsa_verify (and the reverse) reuses 256-byte rows: the two entries share no key, so no signature row"""
    vkeys, vops = S._rsav_pool("good")
    assert not {k.n for kind in ("good", "bad", "other", "refused") for k in S._rsas_keys(kind)} & ({n for n, _ in vkeys} | set(S.moduli("bad")))
    theirs = {int.from_bytes(sg, "big") for _, sg, _, _ in vops}
    assert not set(S.op_reference("rsa_sign_keyset", "good", 141)["sig"]) & theirs and len(theirs) == S.POOL


def test_independent_restatements_of_the_good_answers():
    """The references come from the oracle / restatement modules the tests of each entry use; here the cheap ones are checked once more
    from their defining property."""
    r = S.op_reference("modinv", "good", 70)
    i = S.op_input("modinv", "good", 70)
    assert all(v * o % i["mods"][k] == 1 for v, o, k in zip(i["values"], r["out"], i["idx"]))
    i, r = S.op_input("sss_distribute", "good", 70), S.op_reference("sss_distribute", "good", 70)
    for poly, k, sh in zip(i["polys"], i["idx"], r["shares"]):
        m = i["mods"][k]
        pick = [(x + 1, sh[x]) for x in (0, 2, 3, 5, 6, 8, 9)]
        assert S.T.calculate_secret(pick, m) == poly[0]
    i = S.op_input("rsa_verify", "good", 70)
    import rsa_verify_ref as V
    for dg, sg, k, want in i["ops"][:12]:
        n, e = i["keys"][k]
        assert want == (1, 0) and pow(int.from_bytes(sg, "big"), e, n).to_bytes(256, "big") == V.em(256, 8, dg)
    i = S.op_input("lagrange_combine_small", "bad", 70)
    assert all(any(math.gcd(math.prod(x - xj for x in xs if x != xj), i["mods"][k]) != 1 for xj in xs) for xs, k in zip(i["xs"], i["idx"]))
    i = S.op_input("lagrange_combine_huge", "bad", 70)
    assert all(math.prod(xs[1:]).bit_length() > 2128 for xs in i["xs"])
    i = S.op_input("lagrange_combine_big", "good", 70)
    assert all(math.prod(xs[1:]) >= 1 << 31 for xs in i["xs"])                         # the big path, not the 31-bit one
    i = S.op_input("lagrange_combine_small", "good", 141)
    assert all(abs(math.prod(x for x in xs if x != xj)) < 1 << 31 and abs(math.prod(x - xj for x in xs if x != xj)) < 1 << 31 for xs in i["xs"] for xj in xs)
    # the signing entries: a good signature verifies; a partial signature is em^mag or its inverse; no bad request's em is a unit
    i, r = S.op_input("rsa_sign_keyset", "good", 70), S.op_reference("rsa_sign_keyset", "good", 70)
    for (dg, k, st, _), sig in list(zip(i["ops"], r["sig"]))[:12]:
        key = i["keys"][k]
        assert st == 0 and pow(sig, key["e"], key["n"]).to_bytes(256, "big") == V.em(256, 8, dg)
    i, r = S.op_input("rsa_crt_selftest", "good", 70), S.op_reference("rsa_crt_selftest", "good", 70)
    for (c, k, st, _), out in list(zip(i["ops"], r["out"]))[:12]:
        key = i["keys"][k]
        d = pow(key["e"], -1, (key["p"] - 1) * (key["q"] - 1))
        assert st == 0 and c < key["n"] and out == pow(c, d, key["n"])               # an honest key: the CRT value is c^d mod n
    import rsa_psign_ref as P
    i, r = S.op_input("rsa_partial_sign", "good", 70), S.op_reference("rsa_partial_sign", "good", 70)
    seen = set()
    for (req, sb, mag, _), out in zip(i["frags"], r["out"]):
        N = i["mods"][i["mod_idx"][req]]
        em = P.emsa_encode(i["t"][req], N)
        assert out * pow(em, mag, N) % N == 1 if sb else out == pow(em, mag, N)
        seen.add(bool(sb))
    assert seen == {False, True}
    i = S.op_input("rsa_partial_sign", "bad", 70)
    assert all(math.gcd(P.emsa_encode(t, i["mods"][k]), i["mods"][k]) == 3 for t, k in zip(i["t"], i["mod_idx"]))
    i, r = S.op_input("tsig_partial_s", "bad", 70), S.op_reference("tsig_partial_s", "bad", 70)
    assert all(si == ((r_ * y + m) * k + c) % i["q"][j] for (m, r_, y, k, c), j, si in zip(i["ops"], i["idx"], r["si"]))
    i, r = S.op_input("tdsa_share", "bad", 70), S.op_reference("tdsa_share", "bad", 70)
    p, q, g = i["groups"][1]
    for sh, ri, vi, ki, ci in list(zip(i["reqs"], r["ri"], r["vi"], r["ki"], r["ci"]))[:12]:
        k, a, b, c = (sum(col) % q for col in zip(*sh))
        assert (ri, vi, ki, ci) == (pow(g, a, p), (k * a + b) % q, k, c)
