"""-m gpu: ONE micro-batcher serving every threshold-style request kind at once.  The batcher's leader splits a batch into groups by
(kind, quorum or key set, shape) and makes one device call per group; each kind's own test drives it with callers of that kind alone,
so nothing else puts several kinds into one batch.  Expected values are what the direct batched entry of the same kind returned for
the same cases, called once (once per digest length for the DSA kinds) before the batcher exists."""
import contextlib
import math
import threading

import numpy as np
import pytest

import dsa_verify_cases as DK
import ec_ref as E
import ecdsa_verify_cases as EK
import rsa_psign_ref as PR
import rsa_sign_ref as SR
import rsa_verify_ref as RV
from corpus import keys as CK

pytestmark = pytest.mark.gpu
E_INVALID = -1
OK, NO_INVERSE, FENCED, INVALID_INPUT, CHECK_FAILED, FAILED = 0, 1, 2, 3, 4, 0xFF
NB, QB, K3 = 64, 20, 3                      # the combines: 512-bit moduli, a 160-bit order, k = 3
CALLERS, CALLS = 2, 10                      # caller threads per kind, calls per thread


def _be(vals, nbytes):
    return np.frombuffer(b"".join(int(v).to_bytes(nbytes, "big") for v in vals), dtype=np.uint8).reshape(len(vals), nbytes).copy()


def _by_label(cases, labels):
    return [next(cs for cs in cases if cs.label == lb) for lb in labels]


def _kinds(ctx, stack):
    """name -> (cases, want, call, refused): want[i] = (0, status, verdict or value(s)) from the direct entry, call(batcher, case) the
    same operation as one micro-batched call, refused what that call returns once the batcher is gone.  The key sets are destroyed
    when `stack` unwinds."""
    rng = np.random.default_rng(4512)
    big = lambda nb: int.from_bytes(rng.bytes(nb), "big")                    # noqa: E731
    m_a, m_b = (big(NB) | (1 << 511) | 1 for _ in range(2))
    m_3 = 3 * (big(NB - 1) | 1)                                              # shares the factor 3 with the denominator 1 - 4
    G = DK.group("dsa1024")
    assert G.q.bit_length() == 8 * QB
    c = E.CURVES["P-256"]
    out = {}

    def blank(v):
        return tuple(blank(x) for x in v) if isinstance(v, tuple) else bytes(len(v)) if isinstance(v, bytes) else 0

    def add(name, cases, values, st, call, statuses, refused=None):
        # (an operation whose status is not OK: the batched entry leaves what its kernels wrote, the one-operation entry the caller's
        # zeroes -- include/bftkv_gpu.h, and test_gpu_threshold.py pins it: 0 is what the batcher must give)
        # values[i]: an integer, the bytes of a row, or a tuple of rows for a kind with several outputs (they follow the status one by
        # one); st[i]: a status, or a tuple of them for a request with a status per fragment, whose values are a tuple as long
        norm = lambda v: v if isinstance(v, (bytes, tuple)) else int(v)      # noqa: E731
        want = []
        for v, s in zip(values, st):
            if isinstance(s, tuple):
                want.append((0, s, tuple(norm(x) if y == OK else blank(norm(x)) for x, y in zip(v, s))))
            else:
                v = norm(v) if s == OK else blank(norm(v))
                want.append((0, int(s)) + (v if isinstance(v, tuple) else (v,)))
        seen = {y for w in want for y in (w[1] if isinstance(w[1], tuple) else (w[1],))}
        assert len(cases) == CALLS and seen == statuses, (name, want)
        if refused is None:                          # what a call gets once the batcher is gone: failed statuses beside zeroes
            w = want[0]
            refused = (E_INVALID, (FAILED,) * len(w[1]) if isinstance(w[1], tuple) else FAILED) + tuple(blank(x) for x in w[2:])
        out[name] = (cases, want, call, refused)

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

    # -- RSA PKCS#1 v1.5 under two 512-bit keys: verification with the key in the call and under a resident set (case 3 is the honest
    # signature of another digest: invalid; case 6 under n + 1, even: fenced), signing under a resident signer set whose third key has
    # qinv + 1 (cases 2 and 7: the check fails, no byte of s comes back)
    rk = [SR.key_from_primes(k["p"], k["q"], k["e"]) for k in (CK.load_keys("rsa512", 1)[0], CK.gen_rsa(1, bits=512))]
    assert all(k.n.bit_length() == 512 for k in rk) and rk[0].n != rk[1].n
    vkeys = [(rk[0].n, rk[0].e), (rk[1].n, rk[1].e), (rk[0].n + 1, rk[0].e)]
    dgs = [rng.bytes(32) for _ in range(CALLS)]
    vki = [2 if i == 6 else i % 2 for i in range(CALLS)]
    sgs = [SR.crt(rk[k % 2], int.from_bytes(RV.em(NB, 8, d), "big")).to_bytes(NB, "big") for d, k in zip(dgs, vki)]
    dgs[3] = bytes([dgs[3][0] ^ 1]) + dgs[3][1:]
    valid, st = ctx.rsa_verify(dgs, sgs, vkeys, 8, key_idx=vki, nbytes=NB)
    assert [int(v) for v in valid] == [0 if i in (3, 6) else 1 for i in range(CALLS)]
    add("rsa_verify", list(zip(dgs, sgs, vki)), valid, st, lambda b, a: b.rsa_verify(a[0], a[1], vkeys[a[2]][0], vkeys[a[2]][1], 8), {OK, FENCED})
    vset = ctx.rsa_keyset_create(vkeys, nbytes=NB)
    stack.callback(ctx.rsa_keyset_destroy, vset)
    valid, st = ctx.rsa_verify_keyset(vset, dgs, sgs, 8, key_idx=vki)
    assert [int(v) for v in valid] == [0 if i in (3, 6) else 1 for i in range(CALLS)]
    add("rsa_verify_keyset", list(zip(dgs, sgs, vki)), valid, st, lambda b, a: b.rsa_verify_keyset(vset, a[2], a[0], a[1], 8), {OK, FENCED})
    sset = ctx.rsa_signer_create([k._asdict() for k in rk + [rk[1]._replace(qinv=rk[1].qinv + 1)]], nbytes=NB, pbytes=NB // 2)
    stack.callback(ctx.rsa_signer_destroy, sset)
    ski = [2 if i in (2, 7) else i % 2 for i in range(CALLS)]
    sig_rows, st = ctx.rsa_sign_keyset(sset, dgs, 8, key_idx=ski)
    assert all(pow(int.from_bytes(r.tobytes(), "big"), rk[k].e, rk[k].n).to_bytes(NB, "big") == RV.em(NB, 8, d) for r, k, d in zip(sig_rows, ski, dgs) if k < 2)
    # (under a batcher that is gone nobody knows the set's row width: the header leaves the row alone, here the wrapper's 0xAA)
    add("rsa_sign_keyset", list(zip(ski, dgs)), [r.tobytes() for r in sig_rows], st, lambda b, a: b.rsa_sign_keyset(sset, a[0], a[1], 8), {OK, CHECK_FAILED},
        refused=(E_INVALID, FAILED, b"\xaa" * NB))

    # -- password authentication: makeYi and makeBi, 64-byte values, 16-byte exponents and salts, xi as received (1 .. 64 bytes)
    EL = 16
    modb = [int(m).to_bytes(NB, "big") for m in mods]
    cs = [(int(big(NB) % mods[i % 2]).to_bytes(NB, "big"), rng.bytes(EL), i % 2) for i in range(CALLS)]
    yi, st = ctx.tpa_yi(_be([int.from_bytes(a[0], "big") for a in cs], NB), np.frombuffer(b"".join(a[1] for a in cs), dtype=np.uint8).reshape(CALLS, EL),
                        _be(mods, NB), [a[2] for a in cs])
    add("tpa_yi", cs, [r.tobytes() for r in yi], st, lambda b, a: b.tpa_yi(a[0], a[1], modb[a[2]]), {OK})
    cs = [(int(big(NB) % mods[i % 2]).to_bytes(NB, "big"), rng.bytes(1 + (13 * i) % NB), rng.bytes(EL), rng.bytes(EL), i % 2) for i in range(CALLS)]
    xi = np.zeros((CALLS, NB), dtype=np.uint8)
    for i, a in enumerate(cs):
        xi[i, :len(a[1])] = np.frombuffer(a[1], dtype=np.uint8)
    rows = lambda j, w: np.frombuffer(b"".join(a[j] for a in cs), dtype=np.uint8).reshape(CALLS, w).copy()      # noqa: E731
    bi, keys_, mac, st = ctx.tpa_bi(rows(0, NB), xi, [len(a[1]) for a in cs], rows(2, EL), rows(3, EL), _be(mods, NB), [a[4] for a in cs])
    add("tpa_bi", cs, [(x.tobytes(), y.tobytes(), z.tobytes()) for x, y, z in zip(bi, keys_, mac)], st,
        lambda b, a: b.tpa_bi(a[0], a[1], a[2], a[3], modb[a[4]]), {OK})

    # -- threshold RSA signing: three fragments per request.  Request 4's T leaves no room for the padding (emlen - len(T) < 3: every
    # fragment INVALID_INPUT); request 8 is under m_3 with 3 | em and its second fragment is negative: NO_INVERSE for that one alone
    def t_under(m, want3):
        while True:
            t = rng.bytes(20)
            if (PR.emsa_encode(t, m) % 3 == 0) if want3 else math.gcd(PR.emsa_encode(t, m), m) == 1:
                return t
    cs = []
    for i in range(CALLS):
        m = 2 if i == 8 else i % 2
        t = rng.bytes(NB - 2) if i == 4 else t_under(mods_l[m], i == 8)
        signs = (0, 1, 0) if i == 8 else ((0, 1, 0xFF), (1, 0, 0), (0, 0, 0))[i % 3]
        cs.append((t, m, tuple(rng.bytes(EL) for _ in range(3)), signs))
    tt = np.full((CALLS, NB - 2), 0xEE, dtype=np.uint8)
    for i, a in enumerate(cs):
        tt[i, :len(a[0])] = np.frombuffer(a[0], dtype=np.uint8)
    po, pst = ctx.rsa_partial_sign(tt, [len(a[0]) for a in cs], _be(mods_l, NB), np.frombuffer(b"".join(e for a in cs for e in a[2]), dtype=np.uint8).reshape(3 * CALLS, EL),
                                   np.array([s_ for a in cs for s_ in a[3]], dtype=np.uint8), [a[1] for a in cs], [i for i in range(CALLS) for _ in range(3)])
    assert [int(s_) for s_ in pst[12:15]] == [INVALID_INPUT] * 3 and [int(s_) for s_ in pst[24:27]] == [OK, NO_INVERSE, OK]
    modb_l = [int(m).to_bytes(NB, "big") for m in mods_l]

    def psign(b, a):
        rc, st_, o_ = b.rsa_partial_sign(a[0], modb_l[a[1]], np.frombuffer(b"".join(a[2]), dtype=np.uint8).reshape(3, EL), np.array(a[3], dtype=np.uint8))
        return rc, tuple(int(s_) for s_ in st_), tuple(int.from_bytes(r.tobytes(), "big") for r in o_)
    add("rsa_partial_sign", cs, [tuple(int.from_bytes(r.tobytes(), "big") for r in po[3 * i:3 * i + 3]) for i in range(CALLS)],
        [tuple(int(s_) for s_ in pst[3 * i:3 * i + 3]) for i in range(CALLS)], psign, {OK, NO_INVERSE, INVALID_INPUT})

    # -- threshold DSA / ECDSA signing, the share answers: two shares per request, under the 1024-bit group's resident set and on P-256
    cs = [np.stack([np.stack([_be([EK.rnd(rng, c) % G.q], QB)[0] for _ in range(4)]) for _ in range(2)]) for _ in range(CALLS)]
    ri, vi, ki, ci, st = ctx.tdsa_share(dset, np.stack(cs))
    quad = lambda *a: [tuple(x.tobytes() for x in r) for r in zip(*a)]      # noqa: E731
    add("tdsa_share", cs, quad(ri, vi, ki, ci), st, lambda b, a: b.tdsa_share(dset, 0, a), {OK})
    cs = [np.stack([np.stack([_be([EK.rnd(rng, c)], 32)[0] for _ in range(4)]) for _ in range(2)]) for _ in range(CALLS)]
    ri, vi, ki, ci, st = ctx.tecdsa_share(np.stack(cs), c)
    add("tecdsa_share", cs, quad(ri, vi, ki, ci), st, lambda b, a: b.tecdsa_share(a, c), {OK})
    return out


def test_every_threshold_kind_in_one_batcher(gpu_ctx):
    """Two caller threads per kind, seventeen kinds, all 34 released together onto one lane: batches hold several kinds (and, for the
    DSA kinds, two shapes of one kind) and every caller still gets exactly what the direct entry gave for its case: return code, status
    (one per fragment for RsaPartialSign) and, where a status is OK, the verdict or the output bytes (three rows for TpaBi, four for
    the share kinds); zeroes where it is not.

    After close() the wrapper holds no handle, so one more call of each kind is refused with BFTKV_E_INVALID, failed status and zero
    result (RsaSignKeyset: the row as the caller handed it in, since only the set could tell its width).  (BFTKV_E_STATE is what a call gets that overlaps the destruction; a call that starts after it uses a freed handle, which
    include/bftkv_gpu.h forbids and no test may do.)"""
    from bftkv_amd import Batcher
    with contextlib.ExitStack() as stack:       # (unwinds in reverse: the batcher and its lanes go before the sets they read)
        kinds = _kinds(gpu_ctx, stack)
        assert len(kinds) == 17
        b = Batcher(gpu_ctx, max_items=64, n_lanes=1)
        stack.callback(b.close)
        got = {(name, t): [None] * CALLS for name in kinds for t in range(CALLERS)}
        gate = threading.Barrier(len(got))

        def run(name, t):
            cases, _, call, _ = kinds[name]
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
        for name, (cases, _, call, refused) in kinds.items():
            assert call(b, cases[0]) == refused, name
