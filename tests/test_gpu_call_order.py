"""-m gpu: no call's answer depends on the calls made before it.

Every per-call temporary of the library is a grow-only buffer that is reused without being cleared, the scratch pool hands the
same allocations out in other roles from one entry point to the next, status bytes are OR-ed into packed words, and the pipeline
steers its own later kernels through device words.  Fresh memory reads as zero, so a missing clear passes every test that is the
first to touch its buffers.  Here each character of tests/state_cases.py runs BEHIND the predecessor that would hurt it most, on a
context of its own (not the session's, which carries the suite's history), and every assertion has two halves:

  * the answer equals the reference (tests/test_state_reference.py asserts the references and that predecessor and successor differ
    in every compared byte, so a stale read cannot coincide with the right answer);
  * the answer is byte-identical to the BASELINE: the same call as the first call on a fresh context.

A predecessor is tiled until it has at least as many items, packet events and bytes (operations) as its successor, so whatever is
stale still lies inside a live allocation and a bug shows as a wrong byte."""
import contextlib

import numpy as np
import pytest

import state_cases as S
from tests import helpers as H

pytestmark = pytest.mark.gpu


# ---- contexts ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def fresh(kr=None, keyring=True):
    """A context of its own under the characters' ring (DSA tables of 8-bit windows: megabytes, not gigabytes)."""
    import torch  # noqa: F401  (its HIP runtime first: tests/conftest.py)
    from bftkv_amd import Context
    ctx = Context(0)
    try:
        ctx.set_dsa_window_bits(8)
        qh = None
        if keyring:
            R = S.ring()
            ctx.keyring_set(H.abi_keys(kr or R.keyring))
            qh = ctx.quorum_create(H.abi_qcs(R.quorum))
        yield ctx, qh
    finally:
        ctx.close()


# ---- one pipeline call and its checks -------------------------------------------------------------------------------------------
def _per_item(st, st_item, n):
    out = [[] for _ in range(n)]
    for s, i in zip(st.tolist(), st_item.tolist()):
        out[i].append(s)
    return out


def observe(ctx, qh, call, route="collective"):
    tb, to, sb, so = S.arrays(call)
    n = len(call.tbs)
    if route == "collective":
        err, nver, verdict = ctx.collective_verify(qh, tb, to, sb, so)
        a = {"err": err.copy(), "nver": nver.copy(), "verdict": verdict.copy(), "fenced": ctx.last_fenced.copy()}
    elif route == "signature":
        a = {"err": ctx.signature_verify(tb, to, sb, so).copy(), "fenced": ctx.last_fenced.copy()}
    elif route == "collective_small":
        err, fenced = ctx.collective_verify_small(qh, tb, to, sb, so)
        return {"err": err.copy(), "fenced": fenced.copy()}
    elif route == "signature_small":
        err, fenced = ctx.signature_verify_small(tb, to, sb, so)
        return {"err": err.copy(), "fenced": fenced.copy()}
    elif route == "segments":
        # payload i = prefix i || segment i: the last seven bytes of every second payload come as a shared segment
        cut = [min(7, len(t)) if i % 2 else 0 for i, t in enumerate(call.tbs)]
        pb, po = H.cat([t[:len(t) - c] for t, c in zip(call.tbs, cut)])
        segs = [t[len(t) - c:] for t, c in zip(call.tbs, cut) if c]
        shb, sho = H.cat(segs or [b"x"])
        seg, k = [], 0
        for c in cut:
            seg.append(k if c else 0xFFFFFFFF)
            k += 1 if c else 0
        err, nver, verdict = ctx.collective_verify_segments(qh, pb, po, shb, sho, np.array(seg, dtype=np.uint32), sb, so)
        a = {"err": err.copy(), "nver": nver.copy(), "verdict": verdict.copy(), "fenced": ctx.last_fenced.copy()}
    else:
        raise ValueError(route)
    st, st_item = ctx.last_statuses()
    a["statuses"] = _per_item(st, st_item, n)
    return a


def check(ans, ref, base, what, early=True, sig=False):
    """Both halves for one call.  The reference decides the items that are not fenced (with the early exit off the verdict bits
    cover every signer, not those up to the exit: only the baseline speaks for them); the baseline decides every byte."""
    assert np.array_equal(ans["fenced"], ref.fenced), (what, "fenced", ans["fenced"].tolist())
    ok = ref.fenced == 0
    want_err = ref.sig_err if sig else ref.err
    assert np.array_equal(ans["err"][ok], want_err[ok]), (what, "err", ans["err"].tolist(), want_err.tolist())
    if "nver" in ans:
        assert np.array_equal(ans["nver"][ok], ref.nver[ok]), (what, "n_verified", ans["nver"].tolist(), ref.nver.tolist())
        if early:
            assert np.array_equal(ans["verdict"][ok], ref.verdict[ok]), (what, "verdict", ans["verdict"].tolist(), ref.verdict.tolist())
    if "statuses" in ans and not sig:
        for i in np.nonzero(ok)[0]:
            assert ans["statuses"][i][:len(ref.statuses[i])] == ref.statuses[i], (what, "statuses of item", int(i), ans["statuses"][i], ref.statuses[i])
    for k in ("err", "nver", "verdict", "fenced"):
        if k in ans:
            assert np.array_equal(ans[k], base[k]), (what, k, "differs from the first call on a fresh context", ans[k].tolist(), base[k].tolist())
    if "statuses" in ans:
        for i in range(len(ref.err)):
            upto = len(ref.statuses[i]) if (ok[i] and early and not sig) else None      # every packet is verified: every status counts
            assert ans["statuses"][i][:upto] == base["statuses"][i][:upto], (what, "statuses of item", i, "differ from the baseline")


_BASE = {}


def baseline(name, route="collective", early=True):
    """the character's answers as the first calls on a fresh context (each call of a character on a context of its own)"""
    key = (name, route, early)
    if key not in _BASE:
        out = []
        for call in S.character(name).calls:
            with fresh() as (ctx, qh):
                ctx.set_early_exit(early)
                out.append(observe(ctx, qh, call, route))
        _BASE[key] = out
    return _BASE[key]


def run_pred(ctx, qh, pred, succ, route="collective"):
    want = tuple(max(v) for v in zip(*(S.size(c) for c in S.character(succ).calls)))      # per field, over all of the successor's calls
    for call in S.character(pred).calls:
        observe(ctx, qh, S.behind(call, want), route)


def run_succ(ctx, qh, succ, what, route="collective", early=True):
    ch = S.character(succ)
    for k, (call, ref) in enumerate(zip(ch.calls, ch.refs)):
        check(observe(ctx, qh, call, route), ref, baseline(succ, route, early)[k], what + (succ, k), early, route.startswith("signature"))


# ---- (a) every ordered pair of pipeline characters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("succ", S.PIPELINE)
def test_every_character_behind_every_character(succ):
    for pred in S.PIPELINE:
        with fresh() as (ctx, qh):
            run_pred(ctx, qh, pred, succ)
            run_succ(ctx, qh, succ, (pred, "->"))


def test_baselines_equal_the_references():
    for name in S.PIPELINE:
        ch = S.character(name)
        for route, early in (("collective", True), ("collective", False), ("signature", True)):
            for k, ref in enumerate(ch.refs):
                b = baseline(name, route, early)[k]
                check(b, ref, b, (name, route, early, k), early, route == "signature")


@pytest.mark.parametrize("succ", S.PIPELINE)
def test_designated_pairs_with_every_packet_verified_and_through_signature_verify(succ):
    for pred in S.designated(succ):
        with fresh() as (ctx, qh):
            ctx.set_early_exit(False)
            run_pred(ctx, qh, pred, succ)
            run_succ(ctx, qh, succ, (pred, "-> every packet"), early=False)
        with fresh() as (ctx, qh):
            run_pred(ctx, qh, pred, succ, "signature")
            run_succ(ctx, qh, succ, (pred, "-> signature_verify"), "signature")
        with fresh() as (ctx, qh):                                   # and across the two entry points, which share every buffer
            run_pred(ctx, qh, pred, succ, "collective")
            run_succ(ctx, qh, succ, (pred, "collective -> signature_verify"), "signature")


# ---- (b) routes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("succ", S.PIPELINE)
def test_small_call_route_and_resident_route_behind_each_other(succ):
    for pred in S.designated(succ):
        for small, resident in (("collective_small", "collective"), ("signature_small", "signature")):
            with fresh() as (ctx, qh):                               # the small call behind a resident call
                run_pred(ctx, qh, pred, succ, resident)
                run_succ(ctx, qh, succ, (pred, resident, "->", small), small)
            with fresh() as (ctx, qh):                               # a resident call behind a small call
                run_pred(ctx, qh, pred, succ, small)
                run_succ(ctx, qh, succ, (pred, small, "->", resident), resident)
            with fresh() as (ctx, qh):                               # small behind small
                run_pred(ctx, qh, pred, succ, small)
                run_succ(ctx, qh, succ, (pred, small, "->", small), small)


def _overflowing_call():
    """three items of `plain` behind 5000 empty packets of an unknown type each: more packet events than a staged call's arena holds
    (max(4096, bytes / 16 + 64 items)), so the call turns itself into an empty one and is run again through the ordinary entry"""
    p = S.character("plain").calls[0]
    return S.Call(p.tbs[:3], [b"\xd4\x00" * 5000 + s for s in p.ss[:3]])


@pytest.mark.parametrize("succ", S.PIPELINE)
def test_small_call_that_fits_behind_a_staged_call_that_overflowed(succ):
    over = _overflowing_call()
    n_ev = sum(S.count_events(s) for s in over.ss)
    assert n_ev > max(4096, sum(len(s) for s in over.ss) // 16 + 64 * 3)
    want = S.character("plain").refs[0].err[:3]
    for small in ("collective_small", "signature_small"):
        with fresh() as (ctx, qh):
            a = observe(ctx, qh, over, small)
            assert np.array_equal(a["err"], want) and not a["fenced"].any(), (small, a)
            run_succ(ctx, qh, succ, ("overflowed ->", small), small)


@pytest.mark.parametrize("succ", S.PIPELINE)
def test_segmented_calls_and_the_host_pipeline_in_pieces(succ):
    for pred in S.designated(succ):
        with fresh() as (ctx, qh):
            ctx.set_host_pipeline(1)
            run_pred(ctx, qh, pred, succ, "segments")
            run_succ(ctx, qh, succ, (pred, "segments ->"), "segments")
        for pieces, copy in ((3, "ring"), (2, "direct")):
            with fresh() as (ctx, qh):
                ctx.set_host_pipeline(pieces, copy)
                run_pred(ctx, qh, pred, succ)
                run_succ(ctx, qh, succ, (pred, "%d pieces" % pieces, copy, "->"))
                run_pred(ctx, qh, pred, succ, "segments")
                run_succ(ctx, qh, succ, (pred, "%d pieces" % pieces, copy, "segments ->"), "segments")


def _through_lane(b, qh, call):
    """every item of the call through the batcher from eight threads at once, so that the lane's batches hold several items:
    [(rc, err, fenced) of collective_verify, the same of signature_verify] per item"""
    import threading
    n = len(call.tbs)
    out = [None] * n

    def worker(k):
        for i in range(k, n, 8):
            out[i] = (b.collective_verify(qh, call.tbs[i], call.ss[i], raw=True), b.signature_verify(call.tbs[i], call.ss[i], raw=True))
    ths = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert all(o is not None for o in out)
    return out


def test_one_batcher_lane_serves_other_hashes_then_plain():
    """One lane, midstates from the callers: the items of `other_hashes` come back for resubmission with their payloads (the lane runs
    them again through the ordinary entry), then the same lane serves `plain`, `all_bad`, ...  Both halves: every byte is the
    reference's where the reference speaks, and equals what a fresh lane on a fresh context answers to the same character."""
    from bftkv_amd import Batcher
    order = ("other_hashes", "plain", "all_bad", "wide", "plain", "fenced", "plain", "all_lists", "all_bad")
    base = {}
    for name in set(order):
        with fresh() as (ctx, qh):
            b = Batcher(ctx, max_items=8, n_lanes=1)
            try:
                base[name] = _through_lane(b, qh, S.character(name).calls[0])
            finally:
                b.close()
    with fresh() as (ctx, qh):
        b = Batcher(ctx, max_items=8, n_lanes=1)
        try:
            for name in order:
                ch = S.character(name)
                ref = ch.refs[0]
                got = _through_lane(b, qh, ch.calls[0])
                for i, ((rc, err, fenced), (rc2, err2, fenced2)) in enumerate(got):
                    assert rc == 0 and fenced == ref.fenced[i] and (fenced or err == ref.err[i]), (name, i, rc, err, fenced)
                    assert rc2 == 0 and fenced2 == ref.fenced[i] and (fenced2 or err2 == ref.sig_err[i]), (name, "signature", i, rc2, err2, fenced2)
                assert got == base[name], (name, "differs from a fresh lane")
            assert b.stats()["max_batch"] > 1                 # the lane did run batches of several items
        finally:
            b.close()


# ---- (c) grow, then shrink -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.PIPELINE)
def test_tiled_then_single_then_tiled(name):
    """8 x, once, 8 x again: a reallocation in between, and the tail of the tiled call is stale while the single call runs"""
    ch = S.character(name)
    with fresh() as (ctx, qh):
        for k, (call, ref) in enumerate(zip(ch.calls, ch.refs)):
            base = baseline(name)[k]
            n = len(call.tbs)
            tiled = S.tile(call, 8)
            first = observe(ctx, qh, tiled)
            check(observe(ctx, qh, call), ref, base, (name, k, "single behind 8 x"))
            again = observe(ctx, qh, tiled)
            for t in range(8):
                for a in (first, again):
                    part = {f: (v[t * n:(t + 1) * n]) for f, v in a.items()}
                    check(part, ref, base, (name, k, "tile", t))


# ---- (d) keyring transitions -------------------------------------------------------------------------------------------------------------
def _rings():
    import copy
    R = S.ring()
    base = list(R.keyring.keyring)
    r1 = base[:13]
    twin = copy.deepcopy(base[1])
    twin.primary = copy.deepcopy(base[1].primary)
    twin.primary.key_id = base[0].primary.key_id                  # another member's key under member 0's id, behind the genuine key
    return {"R1": S.col.Keyring(keyring=r1), "R2": S.col.Keyring(keyring=base + [twin]), "R3": S.col.Keyring(keyring=r1[:5] + r1[6:])}


@pytest.fixture(scope="module")
def ring_refs():
    """reference and baseline of plain / all_bad / all_lists under each of the three rings"""
    rings = _rings()
    out = {}
    for rn, kr in rings.items():
        for name in ("plain", "all_bad", "all_lists"):
            call = S.character(name).calls[0]
            ref = S.reference(call, kr, S.ring().quorum)
            with fresh(kr) as (ctx, qh):
                out[rn, name] = (ref, observe(ctx, qh, call))
    return rings, out


@pytest.mark.parametrize("forked", (False, True), ids=("root", "fork"))
def test_keyring_transitions(ring_refs, forked):
    """R1 (RSA-2048 only) -> R2 (the full ring and two keys under one id) -> R1 -> R3 (R1 less one member) -> R1: every result is the
    reference's under the ring in force -- DSA keys, the 3072 / 4096-bit classes, the ambiguous id and the DSA table slots do not
    survive the ring that brought them."""
    rings, refs = ring_refs
    assert (refs["R1", "all_lists"][0].nver == 9).all() and (refs["R2", "all_lists"][0].nver == 13).all()      # R1 knows the 13 members only
    assert (refs["R3", "plain"][0].err != 0).any() and (refs["R3", "plain"][0].err == 0).any()
    with fresh(rings["R1"]) as (root, qh):
        ctx = root.fork() if forked else root
        try:
            for step, rn in enumerate(("R1", "R2", "R1", "R3", "R1")):
                if step:
                    root.quorum_destroy(qh)
                    root.keyring_set(H.abi_keys(rings[rn]))
                    qh = root.quorum_create(H.abi_qcs(S.ring().quorum))
                for name in ("plain", "all_bad", "all_lists", "plain"):
                    ref, base = refs[rn, name]
                    check(observe(ctx, qh, S.character(name).calls[0]), ref, base, (step, rn, name, "fork" if forked else "root"))
        finally:
            if forked:
                ctx.close()


# ---- (e) the other entry points ------------------------------------------------------------------------------------------------------------
NAMES = [e.name for e in S.ENTRIES]
_OP_BASE = {}


def run_op(ctx, name, kind, n, handles):
    e = S.ENTRY[name]
    inp = S.op_input(name, kind, n)
    h = None
    if e.setup:
        key = (name, kind)
        if key not in handles:
            handles[key] = e.setup(ctx, inp)         # the creation builds its tables through the pool: a predecessor call of its own
        h = handles[key]
    return e.run(ctx, inp, h)


def op_baseline(name, kind, n):
    if (name, kind, n) not in _OP_BASE:
        with fresh(keyring=False) as (ctx, _):
            _OP_BASE[name, kind, n] = run_op(ctx, name, kind, n, {})
    return _OP_BASE[name, kind, n]


def check_op(got, name, kind, n, what):
    want, base = S.op_reference(name, kind, n), op_baseline(name, kind, n)
    for f in want:
        claimed = [i for i, w in enumerate(want[f]) if w is not S.UNCLAIMED]
        assert [got[f][i] for i in claimed] == [want[f][i] for i in claimed], (what, name, kind, n, f, "differs from the reference")
        assert np.array_equal(np.asarray(got[f], dtype=object), np.asarray(base[f], dtype=object)), (what, name, kind, n, f, "differs from the baseline")


@pytest.mark.parametrize("name", NAMES)
def test_same_entry_bad_then_good_and_good_then_bad(name):
    check_op(op_baseline(name, "good", 70), name, "good", 70, "first call")
    check_op(op_baseline(name, "bad", 70), name, "bad", 70, "first call")
    for pk, sk in (("bad", "good"), ("good", "bad")):
        with fresh(keyring=False) as (ctx, _):
            hs = {}
            check_op(run_op(ctx, name, pk, 141, hs), name, pk, 141, "first call")
            check_op(run_op(ctx, name, sk, 70, hs), name, sk, 70, (pk, 141, "->"))
            check_op(run_op(ctx, name, pk, 141, hs), name, pk, 141, (sk, 70, "->"))


@pytest.mark.parametrize("name", S.VERIFY)
def test_merely_invalid_operations_between_good_and_bad(name):
    """The verify entries' third kind -- validity 0 beside status 0, and BFTKV_TH_NO_INVERSE from dsa_verify under a composite q --
    behind good(141) (a stale validity byte would read 1) and behind bad(141) (a stale status byte would read fenced), and the
    reverse: good(70) and bad(70) behind invalid(141)."""
    check_op(op_baseline(name, "invalid", 70), name, "invalid", 70, "first call")
    for pk, sk in (("good", "invalid"), ("bad", "invalid"), ("invalid", "good"), ("invalid", "bad")):
        with fresh(keyring=False) as (ctx, _):
            hs = {}
            check_op(run_op(ctx, name, pk, 141, hs), name, pk, 141, "first call")
            check_op(run_op(ctx, name, sk, 70, hs), name, sk, 70, (pk, 141, "->"))
            check_op(run_op(ctx, name, pk, 141, hs), name, pk, 141, (sk, 70, "->"))


@pytest.mark.parametrize("name", sorted(S.THIRD_KIND))
def test_refused_signatures_and_positive_fragments_between_good_and_bad(name):
    """The signing entries' third kinds.  rsa_sign_keyset `refused` -- fenced under an even-p key, refused by the length rule under a
    368-bit one, in turn: behind good(141) a stale check byte would let a row out, behind bad(141) a stale rule byte would read 0.
    rsa_partial_sign `positive` -- no negative fragment, so the inversion kernel is not launched: behind bad(141) its inverse rows and
    no-inverse bytes are the predecessor's but for their clear.  And the reverse: good(70) and bad(70) behind the third kind's 141."""
    third = S.THIRD_KIND[name]
    check_op(op_baseline(name, third, 70), name, third, 70, "first call")
    for pk, sk in (("good", third), ("bad", third), (third, "good"), (third, "bad")):
        with fresh(keyring=False) as (ctx, _):
            hs = {}
            check_op(run_op(ctx, name, pk, 141, hs), name, pk, 141, "first call")
            check_op(run_op(ctx, name, sk, 70, hs), name, sk, 70, (pk, 141, "->"))
            check_op(run_op(ctx, name, pk, 141, hs), name, pk, 141, (sk, 70, "->"))


@pytest.mark.parametrize("name,n", [("rsa_sign_keyset", 1), ("rsa_sign_keyset", S.RSAS_SIGS_PER_BLOCK + 1), ("rsa_partial_sign", 1)])
def test_padding_pairs_of_the_last_block_leave_nothing(name, n):
    """One signature (31 padding pairs re-run it), one more than a block holds (the second block: one signature, 31 padding pairs), one
    fragment (63 padding quads): first on a fresh context (the baseline), then behind bad(141), whose scratch is as wide and whose
    every row ended the other way.  Both halves: the n answers are the reference's and the baseline's; nothing of a padding pair's run
    shows in them."""
    assert S.RSAS_SIGS_PER_BLOCK == 32
    check_op(op_baseline(name, "good", n), name, "good", n, "first call")
    with fresh(keyring=False) as (ctx, _):
        hs = {}
        check_op(run_op(ctx, name, "bad", 141, hs), name, "bad", 141, "first call")
        check_op(run_op(ctx, name, "good", n, hs), name, "good", n, ("bad", 141, "->"))
        check_op(run_op(ctx, name, "bad", 141, hs), name, "bad", 141, ("good", n, "->"))
        check_op(run_op(ctx, name, "good", n, hs), name, "good", n, ("bad", 141, "-> again"))


@pytest.mark.parametrize("name", ("rsa_sign_keyset", "tdsa_share"))
def test_a_fork_reads_the_roots_sets_from_a_scratch_pool_of_its_own(name):
    """good(70) on a fork behind bad(141) on the root (the fork's pool is fresh, the set's resident rows are the root's) and behind
    bad(141) on the fork itself (its own pool, used), and the root's good(70) behind the fork's calls"""
    with fresh(keyring=False) as (root, _):
        hs = {}
        for kind in ("bad", "good"):
            run_op(root, name, kind, 70, hs)                 # the sets are created on the root: a fork may not
        hs_used = dict(hs)
        check_op(run_op(root, name, "bad", 141, hs), name, "bad", 141, "root")
        fork = root.fork()
        try:
            check_op(run_op(fork, name, "good", 70, hs), name, "good", 70, ("root bad 141 ->", "fork"))
            check_op(run_op(fork, name, "bad", 141, hs), name, "bad", 141, "fork")
            check_op(run_op(fork, name, "good", 70, hs), name, "good", 70, ("fork bad 141 ->", "fork"))
            check_op(run_op(root, name, "good", 70, hs), name, "good", 70, ("fork good 70 ->", "root"))
        finally:
            fork.close()
        assert hs == hs_used                                 # no set was created behind the root's back


@pytest.mark.parametrize("name", NAMES)
def test_behind_the_141_operation_call_of_every_other_entry(name):
    """good(70) and bad(70) directly behind the 141-operation call of every OTHER entry, good and bad alternating: the pool hands
    the predecessor's allocations out again in other roles (limb rows as status bytes and the reverse)."""
    with fresh(keyring=False) as (ctx, _):
        hs = {}
        for k, pred in enumerate(n for n in NAMES if n != name):
            kinds = ("good", "bad") if k % 2 == 0 else ("bad", "good")
            for pk, sk in (kinds, kinds[::-1]):
                run_op(ctx, pred, pk, 141, hs)
                check_op(run_op(ctx, name, sk, 70, hs), name, sk, 70, (pred, pk, 141, "->"))


def test_across_families():
    """every entry's good(70) behind the tiled `all_lists` pipeline call, and `plain` behind the big Lagrange path's bad(141)"""
    big = S.tile(S.character("all_lists").calls[0], 8)
    with fresh() as (ctx, qh):
        hs = {}
        for name in NAMES:
            observe(ctx, qh, big)
            check_op(run_op(ctx, name, "good", 70, hs), name, "good", 70, ("all_lists x 8 ->",))
        for pred in ("lagrange_combine_big", "lagrange_combine_huge", "tpa_bi", "ecdsa_verify"):
            run_op(ctx, pred, "bad", 141, hs)
            for succ in ("plain", "all_bad", "all_lists"):
                run_succ(ctx, qh, succ, (pred, "bad 141 ->"))
                run_op(ctx, pred, "bad", 141, hs)


# ---- (f) output coverage: every byte the header promises is written ------------------------------------------------------------------------
class _A5:
    """numpy as bftkv_amd._native sees it, with zeros() and zeros_like() filled with 0xA5: every array those wrappers allocate that way
    is an output of the C call that follows, so a byte the library does not write reads back as 0xA5.  `made` keeps what was handed
    out, so that a test can see that the outputs of a call did come from here (a wrapper that allocated them another way would turn
    the pattern into nothing) and that the bytes behind n_ops were left alone."""

    def __init__(self):
        self.made = []

    def __getattr__(self, k):
        return getattr(np, k)

    def zeros(self, shape, dtype=float):
        self.made.append(np.full(shape, 0xA5A5A5A5A5A5A5A5 & ((1 << (8 * np.dtype(dtype).itemsize)) - 1), dtype=dtype))
        return self.made[-1]

    def zeros_like(self, a):
        self.made.append(np.full_like(a, 0xA5))
        return self.made[-1]


@pytest.fixture
def a5(monkeypatch):
    import bftkv_amd._native as N
    shim = _A5()
    monkeypatch.setattr(N, "np", shim)
    assert N.np.zeros(3, dtype=np.uint8).tolist() == [0xA5] * 3
    return shim


def _outputs_came_patterned(shim, got, n, what):
    """Every array of the answer is (a view or a copy of) one the shim handed out for this call, and the status / validity arrays of
    n + 8 bytes still read 0xA5 behind n."""
    made, shim.made = shim.made, []
    assert made, (what, "no output array was allocated through the patched numpy")
    for f, v in got.items():
        if isinstance(v, np.ndarray):
            assert any(m.dtype == v.dtype and m.shape[0] >= len(v) and np.array_equal(m[:len(v)], v) for m in made), (what, f, "not an array this call was given")
    for m in made:
        if m.ndim == 1 and m.dtype == np.uint8 and len(m) == n + 8:
            assert (m[n:] == 0xA5).all(), (what, "bytes behind n_ops were written")


def test_host_forms_write_every_output_byte(a5):
    """the caller's arrays start as 0xA5: results and status of every operation are written, refused and fenced ones included (zeroes
    beside a status that is not 0: tests/test_state_reference.py asserts that of the references)"""
    with fresh() as (ctx, qh):
        hs = {}
        for name in NAMES:
            for kind in ("bad", "good", "bad"):
                if S.ENTRY[name].setup and (name, kind) not in hs:
                    run_op(ctx, name, kind, 70, hs)          # (the set's creation and its info calls, before the counted call)
                a5.made = []
                got = run_op(ctx, name, kind, 70, hs)
                _outputs_came_patterned(a5, got, 70, (name, kind))
                check_op(got, name, kind, 70, ("0xA5",))
        for name in S.PIPELINE:
            for route in ("collective", "signature", "collective_small", "signature_small"):
                a5.made = []
                run_succ(ctx, qh, name, ("0xA5", route), route)
                assert a5.made, (name, route)


def test_device_forms_write_every_output_byte():
    """the _dev forms with the caller's device arrays filled with 0xA5: n_ops results and status bytes are written, nothing behind them"""
    import ctypes as C
    import torch
    import tsig_share_cases as K
    from bftkv_amd._native import _curve_bytes, _ints_to_be, _ptr
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    a5 = lambda *shape: torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda:0")      # noqa: E731
    toi = lambda t: [int.from_bytes(bytes(r), "big") for r in t.cpu().numpy()]      # noqa: E731
    flat = lambda rows: [v for r in rows for v in r]      # noqa: E731
    P = lambda t: t.data_ptr()      # noqa: E731
    n = 70
    with fresh(keyring=False) as (ctx, _):
        lib, h = ctx.lib, ctx.h
        sets = {}
        for kind in ("good", "bad", "good", "bad"):
            # RSA combine
            i = S.op_input("modmul_product", kind, n)
            o, f, mi = a5(n + 1, 256), up(_ints_to_be(flat(i["factors"]), 256)), up(np.array(i["idx"], dtype=np.int32))
            ctx._check(lib.bftkv_gpu_modmul_product_dev(h, n, 10, P(f), 256, P(mi), 2, _ptr(_ints_to_be(i["mods"], 256)), P(o)), "modmul_product_dev")
            ctx.sync()
            assert toi(o[:n]) == S.op_reference("modmul_product", kind, n)["out"] and (o[n:] == 0xA5).all(), kind
            # Lagrange: the 31-bit path, the big path, and integers beyond 2128 bits
            for name, k in (("lagrange_combine_small", 7), ("lagrange_combine_big", 22), ("lagrange_combine_huge", 72)):
                i, want = S.op_input(name, kind, n), S.op_reference(name, kind, n)
                o, st = a5(n + 1, 256), a5(n + 8)
                x, y, mi = up(np.array(i["xs"], dtype=np.int32)), up(_ints_to_be(flat(i["ys"]), 256)), up(np.array(i["idx"], dtype=np.int32))
                ctx._check(lib.bftkv_gpu_lagrange_combine_dev(h, n, k, P(x), P(y), 256, P(mi), 2, _ptr(_ints_to_be(i["mods"], 256)), P(o), P(st)), name)
                ctx.sync()
                assert st.cpu().numpy()[:n].tolist() == want["status"].tolist() and (st[n:] == 0xA5).all(), (name, kind)
                assert [v for v, w in zip(toi(o[:n]), want["out"]) if w is not S.UNCLAIMED] == [w for w in want["out"] if w is not S.UNCLAIMED], (name, kind)
                assert (o[n:] == 0xA5).all() and not (o[:n] == 0xA5).all(dim=1).any(), (name, kind)
            # CalculateR
            i, want = S.op_input("dsa_calculate_r", kind, n), S.op_reference("dsa_calculate_r", kind, n)
            o, st = a5(n + 1, 32), a5(n + 8)
            x, ri, vi = up(np.array(i["xs"], dtype=np.int32)), up(_ints_to_be(flat(i["ri"]), 256)), up(_ints_to_be(flat(i["vi"]), 32))
            gi = up(np.array(i["idx"], dtype=np.int32))
            pb, qb = _ints_to_be([g[0] for g in i["groups"]], 256), _ints_to_be([g[1] for g in i["groups"]], 32)
            ctx._check(lib.bftkv_gpu_dsa_calculate_r_dev(h, n, 8, P(x), P(ri), 256, P(vi), 32, P(gi), 2, _ptr(pb), _ptr(qb), P(o), P(st)), "dsa_calculate_r_dev")
            ctx.sync()
            assert st.cpu().numpy()[:n].tolist() == want["status"].tolist() and (st[n:] == 0xA5).all(), kind
            assert [v for v, w in zip(toi(o[:n]), want["out"]) if w is not S.UNCLAIMED] == [w for w in want["out"] if w is not S.UNCLAIMED], kind
            assert (o[n:] == 0xA5).all() and not (o[:n] == 0xA5).all(dim=1).any(), kind
            # the raw verify entries
            def verdicts(name, call):
                i, want = S.op_input(name, kind, n), S.op_reference(name, kind, n)
                dg, sg = up(np.frombuffer(b"".join(o_[0] for o_ in i["ops"]), dtype=np.uint8).copy()), up(np.frombuffer(b"".join(o_[1] for o_ in i["ops"]), dtype=np.uint8).copy())
                ki = up(np.array([o_[2] for o_ in i["ops"]], dtype=np.int32))
                valid, st = a5(n + 8), a5(n + 8)
                ctx._check(call(i, P(dg), len(i["ops"][0][0]), P(sg), P(ki), P(valid), P(st)), name + "_dev")
                ctx.sync()
                assert valid.cpu().numpy()[:n].tolist() == want["valid"].tolist() and st.cpu().numpy()[:n].tolist() == want["status"].tolist(), (name, kind)
                assert (valid[n:] == 0xA5).all() and (st[n:] == 0xA5).all(), (name, kind)
            cb_, bits, fb = _curve_bytes(S._curve()[1])
            keep = []                                   # the host tables of a call, alive until it has returned

            def vp(a):
                keep.append(np.ascontiguousarray(a))
                return keep[-1].ctypes.data_as(C.c_void_p)
            verdicts("ecdsa_verify", lambda i, dg, dl, sg, ki, v, st: lib.bftkv_gpu_ecdsa_verify_dev(
                h, n, dg, dl, sg, ki, len(i["keys"]), vp(np.frombuffer(b"".join(i["keys"]), dtype=np.uint8).copy()), vp(cb_), bits, v, st))
            verdicts("rsa_verify", lambda i, dg, dl, sg, ki, v, st: lib.bftkv_gpu_rsa_verify_dev(
                h, n, dg, 8, dl, sg, 256, ki, len(i["keys"]), vp(_ints_to_be([k[0] for k in i["keys"]], 256)),
                vp(np.array([k[1] for k in i["keys"]], dtype=np.uint32)), v, st))
            verdicts("dsa_verify", lambda i, dg, dl, sg, ki, v, st: lib.bftkv_gpu_dsa_verify_dev(
                h, n, dg, dl, sg, 32, ki, len(i["keys"]), vp(_ints_to_be([k[1] for k in i["keys"]], 256)), vp(np.array([k[0] for k in i["keys"]], dtype=np.uint32)),
                256, len(i["groups"]), vp(_ints_to_be([g[0] for g in i["groups"]], 256)), vp(_ints_to_be([g[1] for g in i["groups"]], 32)),
                vp(_ints_to_be([g[2] for g in i["groups"]], 256)), v, st))
            # ... and under resident key sets: the sets are created on this context (their tables come through the scratch pool),
            # one per kind and entry, and stay until the context closes
            for name, call in (("ecdsa_verify_keyset", lambda ks, dg, dl, sg, ki, v, st: lib.bftkv_gpu_ecdsa_verify_keyset_dev(h, ks, n, dg, dl, sg, ki, v, st)),
                               ("dsa_verify_keyset", lambda ks, dg, dl, sg, ki, v, st: lib.bftkv_gpu_dsa_verify_keyset_dev(h, ks, n, dg, dl, sg, ki, v, st)),
                               ("rsa_verify_keyset", lambda ks, dg, dl, sg, ki, v, st: lib.bftkv_gpu_rsa_verify_keyset_dev(h, ks, n, dg, 8, dl, sg, ki, v, st))):
                if (name, kind) not in sets:
                    sets[name, kind] = S.ENTRY[name].setup(ctx, S.op_input(name, kind, n))
                verdicts(name, lambda i, dg, dl, sg, ki, v, st, call=call, ks=sets[name, kind]: call(ks, dg, dl, sg, ki, v, st))
            # the signing entries: RSA under a resident signer set, the share answers under a resident DSA key set and on P-256
            for name in ("rsa_sign_keyset", "tdsa_share"):
                if (name, kind) not in sets:
                    sets[name, kind] = S.ENTRY[name].setup(ctx, S.op_input(name, kind, n))
            i, want = S.op_input("rsa_sign_keyset", kind, n), S.op_reference("rsa_sign_keyset", kind, n)
            dg = up(np.frombuffer(b"".join(o_[0] for o_ in i["ops"]), dtype=np.uint8).copy())
            ki = up(np.array([o_[1] for o_ in i["ops"]], dtype=np.int32))
            sig, st = a5(n + 1, 256), a5(n + 8)
            ctx._check(lib.bftkv_gpu_rsa_sign_keyset_dev(h, sets["rsa_sign_keyset", kind], n, P(dg), 8, 32, P(ki), P(sig), P(st)), "rsa_sign_keyset_dev")
            ctx.sync()
            assert st.cpu().numpy()[:n].tolist() == want["status"].tolist() and (st[n:] == 0xA5).all(), kind
            assert toi(sig[:n]) == want["sig"] and (sig[n:] == 0xA5).all(), kind
            for name, rw in (("tdsa_share", 256), ("tecdsa_share", 65)):
                i, want = S.op_input(name, kind, n), S.op_reference(name, kind, n)
                sh = up(K.shares_array(i["reqs"], 32).reshape(-1))
                ri, vi, ki, ci, st = a5(n + 1, rw), a5(n + 1, 32), a5(n + 1, 32), a5(n + 1, 32), a5(n + 8)
                if name == "tdsa_share":
                    gi = up(np.full(n, i["gi"], dtype=np.int32))
                    rc = lib.bftkv_gpu_tdsa_share_dev(h, sets[name, kind], n, P(gi), S.TSIG_M, P(sh), P(ri), P(vi), P(ki), P(ci), P(st))
                else:
                    rc = lib.bftkv_gpu_tecdsa_share_dev(h, n, S.TSIG_M, P(sh), vp(cb_), bits, P(ri), P(vi), P(ki), P(ci), P(st))
                ctx._check(rc, name + "_dev")
                ctx.sync()
                assert not st[:n].any() and (st[n:] == 0xA5).all(), (name, kind)
                assert (toi(ri[:n]) if rw == 256 else [bytes(r) for r in ri[:n].cpu().numpy()]) == want["ri"] and (ri[n:] == 0xA5).all(), (name, kind)
                for f, t in (("vi", vi), ("ki", ki), ("ci", ci)):
                    assert toi(t[:n]) == want[f] and (t[n:] == 0xA5).all(), (name, kind, f)
