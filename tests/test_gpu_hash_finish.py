"""-m gpu: the hash finish (kernels.hip digest_body / tail_byte behind k_sha256_mid, k_hash_mid_other, k_hash_mid_text, and
host_sha256.h for the staged calls) at every padding boundary of all seven hashes -- the case set of tests/hash_finish_cases.py
against the Python oracle, exactly: verdict, per-packet status and fence of every signature.  Every signature is by a 1024-bit RSA
key, so all of the digest lies in the bytes k_rsa_compare rebuilds from it: a positive verifies only if the device's digest is
exact.  tests/test_hash_finish_reference.py holds the set to what it claims to cover."""
import pytest

from oracle import openpgp as pgp
from tests import helpers as H
from tests import hash_finish_cases as HF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected():
    """(cases, keyring, per case (accepted, statuses)) -- computed once, shared, never changed."""
    cs, kr = HF.cases(), HF.keyring()
    with HF.weak_hashes_available():
        want = tuple(HF.oracle_verdict(kr, c) for c in cs)
    assert sum(ok for ok, _ in want) > 2000 and sum(not ok for ok, _ in want) > 250
    return cs, kr, want


@pytest.fixture
def weak_hashes(gpu_ctx):
    """MD5 and RIPEMD-160 declared available on both sides; the default (unknown: fenced) afterwards."""
    saved = dict(pgp.HASH_POLICY)
    try:
        gpu_ctx.set_hash_policy(1, 1)
        gpu_ctx.set_hash_policy(3, 1)
        pgp.HASH_POLICY.update(md5=True, ripemd160=True)
        yield
    finally:
        pgp.HASH_POLICY.update(saved)
        gpu_ctx.set_hash_policy(1, 0)
        gpu_ctx.set_hash_policy(3, 0)


def _one_call(gpu_ctx, expected, order):
    """The cases in ``order`` (and layout()'s fillers) as ONE signature_verify call; the fixture's check_small also sends it through
    the staged small-call route -- host midstates, tbs_prefix -- which must agree.  Returns err by case index."""
    cs, kr, want = expected
    gpu_ctx.keyring_set(H.abi_keys(kr))
    lay = HF.layout(order)
    tb, to = H.cat(lay.tbs)
    sb, so = H.cat(lay.sig)
    assert gpu_ctx.check_small and len(lay.tbs) <= 4096
    err = gpu_ctx.signature_verify(tb, to, sb, so)
    fenced = gpu_ctx.last_fenced.copy()
    st, st_item = gpu_ctx.last_statuses()
    got_st = [[] for _ in lay.tbs]
    for s, it in zip(st.tolist(), st_item.tolist()):
        got_st[it].append(s)
    bad, out = [], {}
    for pos, ci in enumerate(lay.case):
        got = (err[pos] == 0, got_st[pos], bool(fenced[pos]))
        if ci is None:                                    # a filler: no signature stream, hence invalid; nothing to report
            if got != (False, [], False):
                bad.append(("filler", pos, got))
            continue
        ok, tr = want[ci]
        out[ci] = int(err[pos])
        if got != (ok, tr, False):
            bad.append((cs[ci].group,) + cs[ci].label + ("start %% 4 = %d" % (lay.start[pos] % 4), "got", got, "want", (ok, tr)))
    assert not bad, (len(bad), bad[:40])
    assert not fenced.any() and set(err.tolist()) <= {0, 1}
    return out


def test_every_boundary_of_every_hash_in_one_shuffled_call(gpu_ctx, expected, weak_hashes):
    """Shuffled, a wave of the digest kernels mixes hashes, versions, text and binary, one finish block and a thousand."""
    cs = expected[0]
    out = _one_call(gpu_ctx, expected, HF.shuffled_order())
    assert len(out) == len(cs)


def test_grouped_by_hash_and_a_call_of_sha256_binary_only(gpu_ctx, expected, weak_hashes):
    """Sorted by hash, k_digest_other's grid-stride loop sees long runs of one kind; a call that holds nothing but binary SHA-256
    signatures leaves the any_other gate shut (k_digest_other has nothing to do), the call after it opens it again."""
    cs = expected[0]
    only256 = HF.sha256_binary_order()
    assert 150 < len(only256) < len(cs) // 4
    a = _one_call(gpu_ctx, expected, only256)
    b = _one_call(gpu_ctx, expected, HF.by_hash_order())
    assert len(b) == len(cs) and all(b[i] == a[i] for i in only256)


def test_batcher_one_call_per_case(gpu_ctx, expected):
    """The staged single-item path (host-side SHA-256 midstate, tbs_prefix, the single-item arena): the SHA-256 v4-binary cases of
    groups A-C and their twins one Batcher call each, and a handful of text-mode and SHA-512 cases, which the staged call cannot
    finish from a SHA-256 midstate (the payload is run again).  Each answer is the batched one, which is the oracle's."""
    from bftkv_amd import Batcher
    cs, kr, want = expected
    picks = [i for i, c in enumerate(cs) if c.hash_id == 8 and c.kind == "v4" and c.group in "ABC"]
    extra = [i for i, c in enumerate(cs) if (c.kind == "text" and c.hash_id in (8, 10) and c.detail != "mixed") or (c.hash_id == 10 and c.group == "C")]
    picks += extra[::5]
    assert len(picks) > 200 and sum(1 for i in picks if cs[i].twin_of is not None) > 15
    assert {cs[i].kind for i in picks} == {"v4", "text"} and {cs[i].hash_id for i in picks} == {8, 10}
    assert max(cs[i].unit for i in picks if cs[i].hash_id == 8) == max(HF.UNITS)
    batched = _one_call(gpu_ctx, expected, picks)
    b = Batcher(gpu_ctx, max_items=8, n_lanes=1)
    try:
        bad = []
        for i in picks:
            rc, err, fenced = b.signature_verify(cs[i].tbs, cs[i].sig, raw=True)
            if (rc, err, fenced) != (0, batched[i], 0) or (err == 0) != want[i][0]:
                bad.append((cs[i].group,) + cs[i].label + ((rc, err, fenced), batched[i]))
        assert not bad, (len(bad), bad[:40])
    finally:
        b.close()
