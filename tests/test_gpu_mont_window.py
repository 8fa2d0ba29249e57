"""-m gpu: exact residues through the 4-lane Montgomery multiplier's ring window (csrc/mont28.h).

In every row of a block a lane reads, through DPP row_shl:1, the column the NEXT lane retired one row earlier; the last lane
of a group reads the next group's lane 0 (zero by construction) and the last lane of a DPP row reads 0.  The cases put groups
at the end of a DPP row of 16 lanes (4 groups), of a wave (16) and of a block (64), beside groups that hold other numbers
and other moduli and beside idle padding groups, and compare every residue with Python's pow().  `k_modexp` runs both the
squaring and the general form of mont_mul<19,4>."""
import numpy as np
import pytest

from corpus import build as cb
from tests import helpers as H

pytestmark = pytest.mark.gpu

NBYTES = 256
EXPONENTS = [1, 2, 3, 65537, 2**32 - 1]
OP_COUNTS = [1, 4, 5, 15, 16, 17, 64, 65]


def _moduli():
    rng = np.random.default_rng(2128)
    rnd = lambda nbits: int.from_bytes(rng.bytes((nbits + 7) // 8), "big") % (1 << (nbits - 1)) | (1 << (nbits - 1)) | 1
    return [2**2048 - 159,      # every limb full
            2**2047 + 1,        # sparse: two non-zero limbs
            rnd(1024), rnd(1025), rnd(2048)]


def _bases(n, rng):
    # a 256-byte operand fills 73 limbs and 4 bits of the 74th: 2^2048 - 1 is "all limbs 0x0FFFFFFF" as far as it can be given
    return [0, 1, n - 1, n - 2, 2**2047, 2**2048 - 1, int.from_bytes(rng.bytes(NBYTES), "big")]


def _be(vals, nbytes):
    return np.frombuffer(b"".join(int(v).to_bytes(nbytes, "big") for v in vals), dtype=np.uint8).reshape(len(vals), nbytes).copy()


@pytest.fixture(scope="module")
def cross():
    """Every (modulus, exponent, base) once, shuffled so that a wave mixes moduli: ops, the table of (modulus, exponent) rows
    `Context.modexp` takes (one exponent per row), and pow() of each op."""
    rng = np.random.default_rng(19)
    rows = [(n, e) for n in _moduli() for e in EXPONENTS]
    ops = [(ri, b) for ri, (n, _) in enumerate(rows) for b in _bases(n, rng)]
    ops = [ops[i] for i in rng.permutation(len(ops))]
    want = [pow(b, rows[ri][1], rows[ri][0]) for ri, b in ops]
    return rows, ops, want


def _run(gpu_ctx, rows, ops, per_op=False):
    base = _be([b for _, b in ops], NBYTES)
    if per_op:       # modexp_ops: one exponent per operation, the moduli alone in the table
        mods = sorted({n for n, _ in rows})
        idx = np.array([mods.index(rows[ri][0]) for ri, _ in ops], dtype=np.uint32)
        out = gpu_ctx.modexp_ops(base, idx, _be(mods, NBYTES), _be([rows[ri][1] for ri, _ in ops], 4))
    else:
        idx = np.array([ri for ri, _ in ops], dtype=np.uint32)
        out = gpu_ctx.modexp(base, idx, _be([n for n, _ in rows], NBYTES), _be([e for _, e in rows], 4))
    return [int.from_bytes(o.tobytes(), "big") for o in out]


def _assert_equal(got, want, rows, ops):
    bad = [(i, ops[i][0]) for i in range(len(ops)) if got[i] != want[i]]
    assert not bad, "op (index, table row) with a wrong residue: %s; rows are (modulus bits, exponent) %s" % (
        bad[:8], [(rows[r][0].bit_length(), rows[r][1]) for _, r in bad[:8]])


def test_every_modulus_exponent_and_base_in_one_call(gpu_ctx, cross):
    rows, ops, want = cross
    assert len(ops) == 5 * 5 * 7 and len({rows[ri][0] for ri, _ in ops[:16]}) > 1     # 175 groups = 3 blocks; moduli mixed in wave 0
    _assert_equal(_run(gpu_ctx, rows, ops), want, rows, ops)


@pytest.mark.parametrize("n_ops", OP_COUNTS)
def test_last_group_at_row_wave_and_block_ends(gpu_ctx, cross, n_ops):
    """The last working group sits just before / at / just past the end of a DPP row, a wave and a block; what follows it is
    padding.  Two windows of the shuffled cross per count, so the groups beside the boundary hold different numbers."""
    rows, ops, want = cross
    for start in (0, 71):
        sel = slice(start, start + n_ops)
        _assert_equal(_run(gpu_ctx, rows, ops[sel]), want[sel], rows, ops[sel])


def test_one_exponent_per_operation(gpu_ctx, cross):
    rows, ops, want = cross
    _assert_equal(_run(gpu_ctx, rows, ops[:65], per_op=True), want[:65], rows, ops[:65])


def test_signature_verify_batched_and_small_call_routes(gpu_ctx):
    """One call of 60 packets: `k_rsa_modexp<19,4>`, and -- the suite's context repeats every call of this size through the
    small-call route and compares -- `k_rsa_modexp<10,8>`.  Verdicts against the oracle."""
    from oracle import collective as col
    from oracle.packet import SignaturePacket
    assert gpu_ctx.check_small
    cl = cb.make_cluster(4)
    kr = H.oracle_keyring(cl)
    gpu_ctx.keyring_set(H.abi_keys(kr))
    rng = np.random.default_rng(5)
    tbs_l, sig_l = [], []
    for i in range(60):
        tbs = cb.serialize_tbs(b"key%04d" % i, rng.bytes(int(rng.integers(0, 200))), i)
        sig = cb.detach_sign(cl.replicas[i % 4], tbs)
        if i % 7 == 3:
            sig = sig[:-1] + bytes([sig[-1] ^ 1])      # the value's lowest bit
        if i % 11 == 5:
            tbs += b"x"                                # signed bytes differ
        tbs_l.append(tbs); sig_l.append(sig)

    def cat(parts):
        off = np.zeros(len(parts) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), off
    tb, to = cat(tbs_l)
    sb, so = cat(sig_l)
    err = gpu_ctx.signature_verify(tb, to, sb, so)
    want = [col.signature_verify(kr, t, SignaturePacket(1, 0, False, s, None)) is None for t, s in zip(tbs_l, sig_l)]
    assert [e == 0 for e in err] == want
    assert 40 <= sum(want) < 60
