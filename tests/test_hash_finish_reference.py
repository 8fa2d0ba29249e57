"""CPU: the hash-finish case set of tests/hash_finish_cases.py is what tests/test_gpu_hash_finish.py takes it for -- every
positive verifies and every twin is refused under the Python oracle, the C restatement (oracle/c/oracle.c, OpenSSL's hashes) gives
every case the same statuses, and every residue, block count, load alignment and payload shape the module's docstring names is
there.  The coverage is computed from the recorded (hash, kind, n, unit, rem) and from the item lists the GPU test submits: an
edit that drops a boundary fails here."""
from collections import Counter

import pytest

from oracle import openpgp as pgp
from oracle.cbind import COracle
from tests import hash_finish_cases as HF

N_POSITIVE = 2027       # pinned: the GPU test cannot pass by having lost its cases
N_TWINS = 254


@pytest.fixture(scope="module")
def verdicts():
    cs, kr = HF.cases(), HF.keyring()
    with HF.weak_hashes_available():
        return cs, [HF.oracle_verdict(kr, c) for c in cs]


def test_positives_verify_twins_do_not_and_the_oracles_agree(verdicts):
    cs, want = verdicts
    assert sum(1 for c in cs if c.twin_of is None) == N_POSITIVE and sum(1 for c in cs if c.twin_of is not None) == N_TWINS
    co = COracle()
    co.set_keyring(HF.keyring())
    co.set_weak_hashes(True, True)
    try:
        for c, (ok, tr) in zip(cs, want):
            assert ok == (c.twin_of is None) and len(tr) == 1, (c.label, tr)
            ctr, nv, _ = co.trace_item(c.tbs, c.sig)
            assert ctr == tr and nv == (1 if ok else 0), "the C oracle differs: %r" % ((c.label, tr, ctr),)
            assert pgp.fence_reason(c.sig) is None, c.label           # nothing here is a shape the device fences by design
    finally:
        co.set_weak_hashes(False, False)
    # a flipped payload bit fails at the hash tag (a BAD_SIG would be the 2^-16 accident of a matching tag: none in this set)
    assert Counter(tr[0] for c, (_, tr) in zip(cs, want) if c.twin_of is not None) == {pgp.ST_HASH_TAG: N_TWINS}
    # under the default policy (availability unknown) the oracle refuses MD5 and RIPEMD-160: the policy is what admits them
    weak = next(c for c in cs if c.hash_id == 1)
    assert HF.oracle_verdict(HF.keyring(), weak) == (False, [pgp.ST_HASH_UNSUPPORTED])


def test_every_targeted_residue_block_count_and_alignment_is_present():
    cs = HF.cases()
    pos = [c for c in cs if c.twin_of is None]
    for c in cs:                                                   # the records are true
        B = HF.block(c.hash_id)
        assert c.n == HF.stream_len(c.kind, c.tbs) and c.rem == c.n % B + c.unit, c.label
        assert c.unit == (5 if c.kind == "v3" else 12 + int.from_bytes(_body(c.sig)[4:6], "big")), c.label
        assert _body(c.sig)[0] == (3 if c.kind == "v3" else 4) and (c.kind != "text" or _body(c.sig)[1] == 1), c.label
    assert {c.hash_id for c in pos} == set(HF.NAMES) and len(HF.HASHES) == 7
    for hash_id, name in HF.HASHES:
        B, L = HF.block(hash_id), HF.len_field(hash_id)
        assert (B, L) == ((128, 16) if name in ("sha384", "sha512") else (64, 8))
        edge = HF.boundary_residues(hash_id)
        assert edge == [B - L - 2, B - L - 1, B - L, B - L + 1, B - 1, 0, 1]
        mine = [c for c in pos if c.hash_id == hash_id]
        sel = lambda g, **kw: [c for c in mine if c.group == g and all(getattr(c, a) == v for a, v in kw.items())]   # noqa: E731

        # A: every residue behind exactly one whole block, under the plain hashed area
        a = sel("A")
        assert {c.rem % B for c in a} == set(range(B)) and len(a) == B, name
        assert all(c.kind == "v4" and c.unit == HF.PLAIN_UNIT == 28 and B <= c.n < 2 * B for c in a), name
        assert {HF.finish_blocks(hash_id, c.rem) for c in a} == {1, 2}, name

        # B: 0 .. 5 whole blocks, each with no tail, one byte and B - 1 bytes
        b = sel("B")
        assert {(c.n // B, c.n % B) for c in b} == {(k, d) for k in range(6) for d in (0, 1, B - 1)}, name
        assert all(c.k == c.n // B and c.kind == "v4" for c in b), name

        # C: under every unit every boundary residue, over a tail shorter than a block
        for unit in HF.UNITS:
            cu = sel("C", unit=unit)
            assert {c.rem % B for c in cu} == set(edge) and len(cu) == len(edge), (name, unit)
            assert all(c.kind == "v4" and c.n < 2 * B for c in cu), (name, unit)
        assert {c.n // B for c in sel("C")} == {0, 1}, name
        # second and third finish block: the length field just fits / just does not, one block up
        rems = {c.rem for c in sel("C")}
        assert {2 * B - L - 1, 2 * B - L} <= rems and ({119, 120} if B == 64 else {239, 240}) <= rems, name
        assert {1, 2, 3} <= {HF.finish_blocks(hash_id, c.rem) for c in sel("C")}, name
        top = max(c.rem for c in sel("C"))
        assert top >= 12 + 65535 and HF.finish_blocks(hash_id, top) > 65535 // B, name

        # D: v3, no trailer
        d = sel("D")
        assert all(c.kind == "v3" and c.unit == 5 and c.n >= B for c in d), name
        assert {c.rem % B for c in d} == (set(range(B)) if name in ("sha256", "sha512") else set(edge)), name

        # E: text mode, n the canonical length
        e = sel("E")
        assert all(c.kind == "text" and c.unit == HF.PLAIN_UNIT and c.n >= B for c in e), name
        for shape in HF.TEXT_SHAPES:
            assert {c.rem % B for c in e if c.detail == shape} == set(edge), (name, shape)
        mixed = [c for c in e if c.detail == "mixed"]
        assert {c.rem % B for c in mixed} == (set(range(B)) if name in ("sha256", "sha512") else set()), name
        for c in e:
            canon = HF.canonical(c.tbs)
            grown = len(canon) - len(c.tbs)
            if c.detail == "lf":                # bare LFs only: every one expands
                assert b"\r" not in c.tbs and grown == c.tbs.count(b"\n") > 0, c.label
            elif c.detail == "crlf":            # nothing expands; the lone CR at the end passes
                assert canon == c.tbs and c.tbs.endswith(b"\r") and not c.tbs.endswith(b"\n\r") and c.tbs.count(b"\r\n") > 0, c.label
            elif c.detail in ("edge", "edge+1"):    # the inserted CR ends a block (or starts the next), its LF follows
                at = B - 1 + (c.detail == "edge+1")
                assert c.tbs[at] == 0x0A and b"\r" not in c.tbs and canon[at:at + 2] == b"\r\n" and grown == 1, c.label
            else:                               # bare LFs, CRLFs, a CR in front of another byte, CR CR LF
                assert c.detail == "mixed" and grown > 0 and all(t in c.tbs for t in (b"\r\n", b"b\n", b"e\rf", b"\r\r\n")), c.label

    # the three short unit sets: all four word alignments of the marker and the trailer
    for units in HF.UNIT_SETS[:3]:
        assert {u % 4 for u in units} == {0, 1, 2, 3}, units
    assert HF.UNIT_SETS[3] == (312,) and HF.UNIT_SETS[4] == (12 + 65535,)
    big = next(c for c in pos if c.unit == 312)
    assert 192 <= _body(big.sig)[6 + 6] < 255            # behind the creation time: a subpacket with a two-octet length

    # F: every eighth case has a twin, over the same signature; the four places take turns
    twins = [c for c in cs if c.twin_of is not None]
    assert len(twins) == (N_POSITIVE + HF.TWIN_EVERY - 1) // HF.TWIN_EVERY
    for t in twins:
        p = cs[t.twin_of]
        diff = [i for i, (x, y) in enumerate(zip(p.tbs, t.tbs)) if x != y]
        assert p.twin_of is None and t.sig == p.sig and len(t.tbs) == len(p.tbs) and len(diff) == 1, t.label
        B, ln = HF.block(t.hash_id), len(p.tbs)
        assert diff[0] == {"first byte": 0, "last byte of the last whole block": ln // B * B - 1, "first byte of the tail": ln // B * B,
                           "last byte": ln - 1}[t.flipped], t.label
    assert min(Counter(t.flipped for t in twins).values()) >= N_TWINS // 8
    assert {(t.hash_id, t.kind) for t in twins} >= {(h, "v4") for h in HF.NAMES} | {(8, "v3"), (10, "v3"), (8, "text"), (10, "text")}


def _body(sig: bytes) -> bytes:
    return sig[6:] if sig[1] == 255 else sig[3:] if sig[1] >= 192 else sig[2:]


@pytest.mark.parametrize("order", ["shuffled", "by-hash", "sha256-binary"])
def test_item_lists_hold_every_loader_block_count_and_start_offset(order):
    """layout(): in each order the GPU test submits, every case once; for each of the four block loaders every k = 1 .. 5 at every
    payload start offset mod 4; fillers are 1-3 bytes with no signature stream; the last payload of the blob is misaligned and made
    of whole blocks only."""
    cs = HF.cases()
    idx = {"shuffled": HF.shuffled_order, "by-hash": HF.by_hash_order, "sha256-binary": HF.sha256_binary_order}[order]()
    lay = HF.layout(idx)
    assert sorted(i for i in lay.case if i is not None) == sorted(idx) and len(set(idx)) == len(idx)
    assert len(idx) == (len(cs) if order != "sha256-binary" else sum(1 for c in cs if c.hash_id == 8 and c.kind == "v4"))
    assert len(lay.tbs) <= 4096                                   # the small-call cross-check of the fixture takes the call too
    pos = 0
    seen = set()
    for tbs, sig, ci, start in zip(lay.tbs, lay.sig, lay.case, lay.start):
        assert start == pos
        pos += len(tbs)
        if ci is None:
            assert 1 <= len(tbs) <= 3 and sig == b""
            continue
        c = cs[ci]
        assert tbs == c.tbs and sig == c.sig
        if c.want_off is not None:
            assert start % 4 == c.want_off, c.label
        if c.group == "B" and c.twin_of is None and c.k:
            seen.add((c.hash_id, c.k, start % 4))
    loaders = HF.LOADERS if order != "sha256-binary" else (8,)
    assert set(HF.LOADERS) == {8, 2, 1, 10}
    assert seen >= {(h, k, off) for h in loaders for k in range(1, 6) for off in range(4)}
    last = cs[lay.case[-1]]
    B = HF.block(last.hash_id)
    assert last.last and lay.start[-1] % 4 != 0 and last.n % B == 0 and last.n >= B and last.hash_id in loaders
    if order == "by-hash":                                        # long runs of one hash
        runs = [cs[i].hash_id for i in lay.case if i is not None and not cs[i].last]
        assert sum(1 for x, y in zip(runs, runs[1:]) if x != y) == len(HF.HASHES) - 1
