"""-m gpu: ONE micro-batcher serving every threshold-style request kind at once.  The batcher's leader splits a batch into groups by
(kind, quorum or key set, shape) and makes one device call per group; each kind's own test drives it with callers of that kind alone,
so nothing else puts several kinds into one batch.  Expected values are what the direct batched entry of the same kind returned for
the same cases, called once (once per digest length for the DSA kinds) before the batcher exists."""
import contextlib
import threading

import numpy as np
import pytest

import dsa_verify_cases as DK
import ec_ref as E
import ecdsa_verify_cases as EK

pytestmark = pytest.mark.gpu
E_INVALID = -1
OK, NO_INVERSE, FENCED, FAILED = 0, 1, 2, 0xFF
NB, QB, K3 = 64, 20, 3                      # the combines: 512-bit moduli, a 160-bit order, k = 3
CALLERS, CALLS = 2, 10                      # caller threads per kind, calls per thread


def _be(vals, nbytes):
    return np.frombuffer(b"".join(int(v).to_bytes(nbytes, "big") for v in vals), dtype=np.uint8).reshape(len(vals), nbytes).copy()


def _by_label(cases, labels):
    return [next(cs for cs in cases if cs.label == lb) for lb in labels]


def _kinds(ctx, stack):
    """name -> (cases, want, call): want[i] = (0, status, verdict or value) from the direct entry, call(batcher, case) the same
    operation as one micro-batched call.  The two key sets are destroyed when `stack` unwinds."""
    rng = np.random.default_rng(4512)
    big = lambda nb: int.from_bytes(rng.bytes(nb), "big")                    # noqa: E731
    m_a, m_b = (big(NB) | (1 << 511) | 1 for _ in range(2))
    m_3 = 3 * (big(NB - 1) | 1)                                              # shares the factor 3 with the denominator 1 - 4
    G = DK.group("dsa1024")
    assert G.q.bit_length() == 8 * QB
    c = E.CURVES["P-256"]
    out = {}

    def add(name, cases, values, st, call, statuses):
        # (an operation whose status is not OK: the batched entry leaves what its kernels wrote, the one-operation entry the caller's
        # zeroes -- include/bftkv_gpu.h, and test_gpu_threshold.py pins it: 0 is what the batcher must give)
        want = [(0, int(s), int(v) if s == OK else 0) for v, s in zip(values, st)]
        assert len(cases) == CALLS and {w[1] for w in want} == statuses, (name, want)
        out[name] = (cases, want, call)

    # -- the four combines
    mods = [m_a, m_b]
    cs = [([big(NB) for _ in range(K3)], i % 2) for i in range(CALLS)]
    add("modmul_product", cs, ctx.modmul_product([f for f, _ in cs], mods, [i for _, i in cs], nbytes=NB), [OK] * CALLS,
        lambda b, a: b.modmul_product(a[0], mods[a[1]], nbytes=NB), {OK})
    mods_l = [m_a, m_b, m_3]
    cs = [(([1, 2, 3], [2, 3, 4], [1, 3, 5])[i % 3], [big(NB) % mods_l[i % 2] for _ in range(K3)], i % 2) for i in range(CALLS - 1)]
    cs.append(([1, 4, 6], [big(NB) % m_3 for _ in range(K3)], 2))
    vals, st = ctx.lagrange_combine([x for x, _, _ in cs], [y for _, y, _ in cs], mods_l, [i for _, _, i in cs], nbytes=NB)
    add("lagrange_combine", cs, vals, st, lambda b, a: b.lagrange_combine(a[0], a[1], mods_l[a[2]], nbytes=NB), {OK, NO_INVERSE})
    cs = [([1, 2, 3], [big(NB) % m_a for _ in range(K3)], [0] * K3 if i == 4 else [big(QB) % G.q for _ in range(K3)]) for i in range(CALLS)]
    vals, st = ctx.dsa_calculate_r([x for x, _, _ in cs], [r for _, r, _ in cs], [v for _, _, v in cs], [(m_a, G.q)], [0] * CALLS, pbytes=NB, qbytes=QB)
    add("dsa_calculate_r", cs, vals, st, lambda b, a: b.dsa_calculate_r(a[0], a[1], a[2], m_a, G.q, pbytes=NB, qbytes=QB), {OK, NO_INVERSE})
    cs = [(big(NB) % mods[i % 2], big(QB), i % 2) for i in range(CALLS)]
    res = ctx.modexp_ops(_be([a[0] for a in cs], NB), [a[2] for a in cs], _be(mods, NB), _be([a[1] for a in cs], QB))
    add("modexp", cs, [int.from_bytes(row.tobytes(), "big") for row in res], [OK] * CALLS,
        lambda b, a: b.modexp(a[0], a[1], mods[a[2]], nbytes=NB, exp_len=QB), {OK})

    # -- ECDSA on P-256: CalculateR (one caller's R_i with a prefix Unmarshal refuses: fenced), verification with the key in the call and
    # under a resident set (honest, mutated, out of range, refused keys)
    pts = [E.calculate_partial_r(c, EK.rnd(rng, c) or 1) for _ in range(4)]
    cs = [([1, 2, 3], [pts[(i + j) % 4] for j in range(K3)], [EK.rnd(rng, c) for _ in range(K3)]) for i in range(CALLS)]
    cs[7] = (cs[7][0], [cs[7][1][0], b"\x02" + cs[7][1][1][1:], cs[7][1][2]], cs[7][2])
    vals, st = ctx.ecdsa_calculate_r([x for x, _, _ in cs], [r for _, r, _ in cs], [v for _, _, v in cs], c)
    add("ecdsa_calculate_r", cs, vals, st, lambda b, a: b.ecdsa_calculate_r(a[0], a[1], a[2], c), {OK, FENCED})
    ecs = _by_label(EK.corpus("P-256"), ["honest dlen=32 #0", "honest dlen=32 #1", "flip r dlen=32 #0", "flip s dlen=32 #0", "flip digest dlen=32 #0",
                                         "flip key X dlen=32 #0", "another key dlen=32", "r = 0", "key prefix 02", "key (0, 0)"])
    assert {len(x.digest) for x in ecs} == {32}
    keys = sorted({x.key for x in ecs})
    kidx = [keys.index(x.key) for x in ecs]
    valid, st = ctx.ecdsa_verify([x.digest for x in ecs], [x.sig for x in ecs], keys, c, key_idx=kidx)
    assert {int(v) for v in valid} == {0, 1}
    add("ecdsa_verify", ecs, valid, st, lambda b, x: b.ecdsa_verify(x.digest, x.sig, x.key, c), {OK, FENCED})
    eset = ctx.ecdsa_keyset_create(keys, c)
    stack.callback(ctx.ecdsa_keyset_destroy, eset)
    valid, st = ctx.ecdsa_verify_keyset(eset, [x.digest for x in ecs], [x.sig for x in ecs], key_idx=kidx)
    assert {int(v) for v in valid} == {0, 1}
    add("ecdsa_verify_keyset", list(zip(kidx, ecs)), valid, st, lambda b, a: b.ecdsa_verify_keyset(eset, a[0], a[1].digest, a[1].sig), {OK, FENCED})

    # -- DSA in the 1024-bit group, two keys (y and y with one bit flipped), two digest lengths (one byte more than the order: fenced)
    dcs = _by_label(DK.corpus("dsa1024"), ["honest dlen=20 #0", "honest dlen=20 #1", "honest dlen=20 #2", "flip r dlen=20 #0", "flip s dlen=20 #0",
                                           "flip digest dlen=20 #0", "flip y dlen=20 #0", "r = 0", "dlen = bytes(q) + 1", "dlen = bytes(q) + 1, r = 0"])
    gs, ks, didx = DK.tables(dcs)
    assert len(gs) == 1 and len(ks) == 2
    sig = lambda x: DK.sig_bytes(G, x.r, x.s)                                # noqa: E731
    dset = ctx.dsa_keyset_create(ks, gs, window_bits=4, pbytes=G.pbytes, qbytes=G.qbytes)
    stack.callback(ctx.dsa_keyset_destroy, dset)
    raw, resident = [None] * CALLS, [None] * CALLS
    for dlen in (QB, QB + 1):
        rows = [i for i, x in enumerate(dcs) if len(x.digest) == dlen]
        args = ([dcs[i].digest for i in rows], [sig(dcs[i]) for i in rows])
        for res, (valid, st) in ((raw, ctx.dsa_verify(*args, ks, gs, key_idx=[didx[i] for i in rows], pbytes=G.pbytes, qbytes=G.qbytes)),
                                 (resident, ctx.dsa_verify_keyset(dset, *args, key_idx=[didx[i] for i in rows]))):
            for i, v, s in zip(rows, valid, st):
                res[i] = (v, s)
    assert None not in raw + resident and {int(v) for v, _ in raw} == {0, 1} and {int(v) for v, _ in resident} == {0, 1}
    add("dsa_verify", dcs, [v for v, _ in raw], [s for _, s in raw],
        lambda b, x: b.dsa_verify(x.digest, sig(x), (x.p, x.q, x.g), x.y, pbytes=G.pbytes), {OK, FENCED})
    add("dsa_verify_keyset", list(zip(didx, dcs)), [v for v, _ in resident], [s for _, s in resident],
        lambda b, a: b.dsa_verify_keyset(dset, a[0], a[1].digest, sig(a[1])), {OK, FENCED})
    return out


def test_every_threshold_kind_in_one_batcher(gpu_ctx):
    """Two caller threads per kind, nine kinds, all released together onto one lane: batches hold several kinds (and, for the DSA
    kinds, two shapes of one kind) and every caller still gets exactly what the direct entry gave for its case: return code, status
    and, where the status is OK, the verdict or the output bytes; zeroes where it is not.

    After close() the wrapper holds no handle, so one more call of each kind is refused with BFTKV_E_INVALID, failed status and zero
    result.  (BFTKV_E_STATE is what a call gets that overlaps the destruction; a call that starts after it uses a freed handle, which
    include/bftkv_gpu.h forbids and no test may do.)"""
    from bftkv_amd import Batcher
    with contextlib.ExitStack() as stack:       # (unwinds in reverse: the batcher and its lanes go before the sets they read)
        kinds = _kinds(gpu_ctx, stack)
        assert len(kinds) == 9
        b = Batcher(gpu_ctx, max_items=64, n_lanes=1)
        stack.callback(b.close)
        got = {(name, t): [None] * CALLS for name in kinds for t in range(CALLERS)}
        gate = threading.Barrier(len(got))

        def run(name, t):
            cases, _, call = kinds[name]
            gate.wait()
            for i in range(CALLS):
                j = (i + 5 * t) % CALLS                                      # (the two callers of a kind are at different cases)
                got[(name, t)][j] = call(b, cases[j])

        th = [threading.Thread(target=run, args=key) for key in got]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        stats = b.stats()
        b.close()
        print("batcher:", stats)
        for (name, t), row in got.items():
            for j, (g, w) in enumerate(zip(row, kinds[name][1])):
                assert g == w, (name, t, j, w, g)
        assert stats["calls"] == len(got) * CALLS and stats["max_batch"] >= 2, stats
        for name, (cases, _, call) in kinds.items():
            assert call(b, cases[0]) == (E_INVALID, FAILED, 0), name
