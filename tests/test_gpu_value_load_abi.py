"""-m gpu: the signature value's loader (csrc/value_load.h) through the C ABI, at every start alignment of the signature blob.

Two batches against the Python oracle.  A clique of ten replicas signs 30 writes with the corpus' mutations (300 packets, valid
and invalid).  Seven keys -- a 2047-bit key, the full 2048-bit prime modulus and the 1025-bit key under 65537, that modulus under 3, the 1025-bit keys
under 3 and 17, the sparse prime modulus under 17 -- sign 15 further writes, each packet carrying another shape of the value: s, its
canonical MPI, s behind three zero bytes, s + j n of exactly 257 ... 261 bytes (the lengths 72 limbs of 29 bits hold) and 262 ... 266
(the share of the 28-bit pass behind it), s with a bit flipped, and a wrong encoding signed with the private key.

The resident route (bftkv_gpu_collective_verify_dev: k_rsa_modexp<18,4,29> and the pass for long values) reads the signature blob
at byte offsets 0, 1, 2 and 3 of a larger device tensor filled with A5: error, exit count, fence and per-packet status of every
item must be the oracle's at every offset.  The small-call route (k_rsa_modexp<10,8>) takes host buffers and lays the streams out
itself, one behind the other; it is given the items in four rotations, so that every stream starts at another byte, and the seven
keys' packets as one-packet calls of bftkv_gpu_signature_verify_small too, where the error IS the packet's verdict (the staged
route keeps no per-packet statuses)."""
import numpy as np
import pytest

from corpus import build as cb
from oracle import collective as col
from oracle import openpgp as pgp
from oracle import wotqs
from oracle.packet import SignaturePacket
from tests import extremal_keys as X
from tests import helpers as H
from tests import rsa_sizes as RS

pytestmark = pytest.mark.gpu

LENGTHS = list(range(257, 267))
HASH_ID = 8               # SHA-256: the small-call route hands every other hash on to the ordinary entry point
GUARD = 0xA5


def _special_keys(taken):
    """Seven keys whose ids are not among ``taken`` (the clique draws on the same stored key material)."""
    mods = {e["name"]: int(e["n"], 16) for e in X.fixture()["rsa"]}
    by = {}
    for kp in RS.keys():
        if kp.key_id not in taken:
            by.setdefault((kp.n.bit_length(), kp.e), kp)
    return [by[(2047, 65537)], X.PrimeModulusKey(mods["full2048"], 65537, "full2048 <k@bftkv.example>"),
            X.PrimeModulusKey(mods["full2048"], 3, "full2048e3 <k@bftkv.example>"), X.PrimeModulusKey(mods["sparse2048"], 17, "sparse2048e17 <k@bftkv.example>"),
            by[(1025, 65537)], by[(1025, 3)], by[(1025, 17)]]


def _variants(ki, kp, tbs):
    """[(name, packet)] of key ``kp`` over ``tbs``, the shapes of the module's docstring in a fixed order."""
    bits = kp.n.bit_length()
    k = (bits + 7) // 8
    name = dict(RS.HASHES)[HASH_ID]
    prefix, digest = RS.digest_of(kp, tbs, HASH_ID)
    n = kp.n
    s = kp.rsa_private(int.from_bytes(RS.encode(k, name, digest), "big") % n)
    out = [("s", RS.go_mpi(s, k)), ("canonical mpi", cb._mpi(s)), ("s behind zero bytes", RS.go_mpi(s, k + 3))]
    for nb in LENGTHS:
        v = s + ((1 << (8 * nb)) - 1 - s) // n * n
        assert v % n == s and v >> (8 * nb - 8) != 0 and v < 1 << (8 * nb) and nb <= RS.value_cap(bits)
        out.append(("s + jn, %d bytes" % nb, RS.go_mpi(v, nb)))
    out.append(("bit flipped", RS.go_mpi(s ^ (1 << ((7 * bits + 13 * HASH_ID + ki) % (bits - 1))), k)))
    name_t, em_t = sorted(RS.tampered_encodings(k, name, digest).items())[ki % 4]
    out.append((name_t, RS.go_mpi(kp.rsa_private(int.from_bytes(em_t, "big")), k)))
    return [(v, RS.packet(prefix, digest, mpi)) for v, mpi in out]


class Batch:
    """Items (tbs, [pieces of the stream]) under one quorum, with what the oracle says of each: error, exit count, per-packet statuses."""

    def __init__(self, kr, q, items):
        self.q, self.items = q, items
        self.tb, self.to = H.cat([t for t, _ in items])
        self.sb, self.so = H.cat([b"".join(ps) for _, ps in items])
        self.want = []
        for t, ps in items:
            r = col.collective_verify(kr, t, SignaturePacket(Type=1, Data=b"".join(ps) or None), q)
            each = [st for p in ps for st in pgp.check_detached_signature(kr.get_keyring(), t, p, 0).statuses]
            assert each[:len(r.statuses)] == r.statuses
            self.want.append((r.err is None, len(r.verified), each))


@pytest.fixture(scope="module")
def world():
    cl = cb.make_cluster(10)
    rates = {cb.MUT_BAD_MPI: 0.1, cb.MUT_UNKNOWN_ISSUER: 0.1, cb.MUT_DUP_SIGNER: 0.1, cb.MUT_ONE_SHORT: 0.15, cb.MUT_BAD_TAG: 0.1}
    c = cb.make_write_corpus(cl, 30, mutation_rates=rates)
    keys = _special_keys({r.key_id for r in cl.replicas})
    ring = H.oracle_keyring(cl).get_keyring() + [RS.entity(kp) for kp in keys]
    kr = col.Keyring(keyring=ring)
    assert len({e.id for e in ring}) == len(ring)
    # the clique's writes, cut where a call of the reference's verifier ends (a packet of an unknown issuer is skipped inside the
    # call that reads the packet behind it: such a piece holds two packets and has two statuses)
    clique_items = []
    for i in range(c.n_items):
        data, ps, pos = c.ss_data(i), [], 0
        while pos < len(data):
            r = pgp.check_detached_signature(ring, c.tbss(i), data[pos:], 0)
            assert r.pos > 0
            ps.append(data[pos:pos + r.pos])
            pos += r.pos
        clique_items.append((c.tbss(i), ps))
    clique = Batch(kr, H.clique_quorum(cl), clique_items)
    # the seven keys: write j carries shape (j + key) mod 15 of every key
    nv = 3 + len(LENGTHS) + 2
    special_items = []
    for j in range(nv):
        tbs = b"value load: write %d " % j + bytes(range(7 * j))
        per_key = [_variants(ki, kp, tbs) for ki, kp in enumerate(keys)]
        assert all(len(v) == nv for v in per_key)
        special_items.append((tbs, [per_key[ki][(j + ki) % nv][1] for ki in range(len(keys))]))
    ids = [kp.key_id for kp in keys]
    qc = wotqs.new_qc(ids, len(ids), wotqs.AUTH, 0)
    special = Batch(kr, wotqs.WotQ([qc]), special_items)
    return kr, clique, special


@pytest.fixture(scope="module")
def device(gpu_ctx, world):
    """The keyring and both quorums on the device; every packet of every item is examined, so that each has a status."""
    kr, clique, special = world
    gpu_ctx.keyring_set(H.abi_keys(kr))
    qhs = [gpu_ctx.quorum_create(H.abi_qcs(b.q)) for b in (clique, special)]
    gpu_ctx.set_early_exit(False)
    yield dict(zip(("clique", "special"), qhs))
    gpu_ctx.set_early_exit(True)
    for qh in qhs:
        gpu_ctx.quorum_destroy(qh)


def test_the_batches_hold_what_they_should(world):
    _, clique, special = world
    n_packets = sum(len(ps) for _, ps in clique.items)
    assert 200 <= n_packets <= 400
    ok = [w for w in clique.want if w[0]]
    assert 0 < len(ok) < len(clique.want)                                                      # valid and invalid writes
    assert {pgp.ST_OK, pgp.ST_BAD_SIG} <= {st for _, _, each in clique.want for st in each}
    assert sum(len(ps) for _, ps in special.items) == 7 * 15
    good = sum(st == pgp.ST_OK for _, _, each in special.want for st in each)
    assert good == 7 * 13                                                                      # all but the flipped bit and the wrong encoding


def _resident(gpu_ctx, qh, batch, offset):
    import torch
    dev = torch.device("cuda", 0)
    n = len(batch.items)
    ss_len = int(batch.so[-1])
    d_ss = torch.full((ss_len + 64,), GUARD, dtype=torch.uint8, device=dev)
    d_ss[offset:offset + ss_len] = torch.from_numpy(batch.sb[:ss_len].copy()).to(dev)
    d_tb = torch.from_numpy(np.ascontiguousarray(batch.tb)).to(dev)
    d_to = torch.from_numpy(batch.to.astype(np.int64)).to(dev)
    d_so = torch.from_numpy(batch.so.astype(np.int64)).to(dev)
    err = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    nver = torch.full((n,), -1, dtype=torch.int32, device=dev)
    verdict = torch.zeros(n, dtype=torch.uint8, device=dev)
    fenced = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert d_ss.data_ptr() % 4 == 0
    gpu_ctx.collective_verify_dev(qh, n, d_tb.data_ptr(), d_to.data_ptr(), d_ss.data_ptr() + offset, d_so.data_ptr(), ss_len,
                                  err.data_ptr(), nver.data_ptr(), verdict.data_ptr(), fenced.data_ptr())
    gpu_ctx.sync()
    st, st_item = gpu_ctx.last_statuses()
    return err.cpu().numpy(), nver.cpu().numpy(), fenced.cpu().numpy(), st, st_item


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("which", ["clique", "special"])
def test_resident_route_at_every_blob_alignment(gpu_ctx, world, device, which, offset):
    batch = world[1] if which == "clique" else world[2]
    err, nver, fenced, st, st_item = _resident(gpu_ctx, device[which], batch, offset)
    bad = []
    for i, (ok, n_ok, each) in enumerate(batch.want):
        got = (err[i] == 0, int(nver[i]), int(fenced[i]), [int(x) for x in st[st_item == i]])
        if got != (ok, n_ok, 0, each):
            bad.append((i, got, (ok, n_ok, 0, each)))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
@pytest.mark.parametrize("which", ["clique", "special"])
def test_small_call_route_with_the_streams_at_every_alignment(gpu_ctx, world, device, which, rotation):
    batch = world[1] if which == "clique" else world[2]
    order = list(range(rotation, len(batch.items))) + list(range(rotation))
    tb, to = H.cat([batch.items[i][0] for i in order])
    sb, so = H.cat([b"".join(batch.items[i][1]) for i in order])
    assert {int(o) % 4 for o in so[:-1]} == {0, 1, 2, 3}           # the route packs the streams back to back: every residue occurs
    err, fenced = gpu_ctx.collective_verify_small(device[which], tb, to, sb, so)
    want = [batch.want[i][0] for i in order]
    assert [e == 0 for e in err] == want and not fenced.any()


def test_small_call_route_packet_by_packet(gpu_ctx, world, device):
    """The seven keys' 105 packets as 105 items of one packet: the item's error is the packet's verdict."""
    _, _, special = world
    flat = [(t, p, st) for (t, ps), (_, _, each) in zip(special.items, special.want) for p, st in zip(ps, each)]
    tb, to = H.cat([t for t, _, _ in flat])
    sb, so = H.cat([p for _, p, _ in flat])
    assert {int(o) % 4 for o in so[:-1]} == {0, 1, 2, 3}
    err, fenced = gpu_ctx.signature_verify_small(tb, to, sb, so)
    assert [e == 0 for e in err] == [st == pgp.ST_OK for _, _, st in flat] and not fenced.any()
