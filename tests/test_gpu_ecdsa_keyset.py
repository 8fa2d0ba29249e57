"""-m gpu: resident ECDSA key sets.  Keys registered once (Unmarshal's checks and a table per key on the device), then
verification with both multiples table-driven: byte for byte (valid, status) against the restatement with its fence rules
(tests/ecdsa_verify_ref.py) and against the raw entry bftkv_gpu_ecdsa_verify, and the device-built tables word for word against
the host's fb_table_build (tests/c/ecdsa_keyset_host.cpp).  Shapes are the smallest at which the kernels can still go wrong."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import ec_ref as E
import ecdsa_keyset_host as KH
import ecdsa_verify_cases as K
import ecdsa_verify_ref as V
from test_gpu_ecdsa_verify import _signed_batch

pytestmark = pytest.mark.gpu
E_INVALID, E_NOMEM, E_UNSUPPORTED, E_STATE = -1, -3, -4, -5
FAILED = 0xFF


@functools.lru_cache(maxsize=None)
def _corpus_want(name):
    c = E.CURVES[name]
    return tuple(V.verify(c, cs.key, cs.digest, cs.sig) for cs in K.corpus(name))


@pytest.fixture(scope="module")
def ekh(tmp_path_factory):
    return KH.build(tmp_path_factory.mktemp("eks_host"))


def _pairs(valid, st):
    return [(int(v), int(s)) for v, s in zip(valid, st)]


@pytest.mark.parametrize("name", E.NAMES)
def test_corpus(gpu_ctx, name):
    c = E.CURVES[name]
    cases, want = K.corpus(name), _corpus_want(name)
    keys = sorted({cs.key for cs in cases})          # the refused ones among them: prefix 02, (0, 0), y + 1, x = P, the flipped X
    refused = [E.unmarshal(c, k) is None for k in keys]
    ks = gpu_ctx.ecdsa_keyset_create(keys, c)
    try:
        info = gpu_ctx.ecdsa_keyset_info(ks)
        print(name, info)
        w = info["window_bits"]
        assert info == {"n_keys": len(keys), "n_refused": sum(refused), "window_bits": w, "table_bytes": len(keys) * KH.table_words(c, w) * 4}
        assert sum(refused) >= 5 and not all(refused)
        got, raw = [None] * len(cases), [None] * len(cases)
        for dlen, idx in K.by_dlen(cases).items():      # one call per digest length
            dg, sg, ki = [cases[i].digest for i in idx], [cases[i].sig for i in idx], [keys.index(cases[i].key) for i in idx]
            for out, (valid, st) in ((got, gpu_ctx.ecdsa_verify_keyset(ks, dg, sg, key_idx=ki)), (raw, gpu_ctx.ecdsa_verify(dg, sg, keys, c, key_idx=ki))):
                for j, i in enumerate(idx):
                    out[i] = (int(valid[j]), int(st[j]))
        for cs, wt, g, r in zip(cases, want, got, raw):
            print(name, cs.label, "want", wt, "key set", g, "raw entry", r)
        bad = [(cs.label, wt, g, r) for cs, wt, g, r in zip(cases, want, got, raw) if not wt == g == r]
        assert not bad, (name, bad)
        assert sum(wt == (1, V.OK) for wt in want) >= 14 and sum(wt[1] == V.FENCED for wt in want) >= 8
        assert sum(cs.group == "special_x" and wt == (1, V.OK) for cs, wt in zip(cases, want)) >= 2     # R at the special x
        assert sum(cs.group == "special_x" and wt == (0, V.OK) for cs, wt in zip(cases, want)) >= 3     # ... and with r + 1
    finally:
        gpu_ctx.ecdsa_keyset_destroy(ks)


@pytest.mark.parametrize("name", E.NAMES)
def test_table_identity(gpu_ctx, ekh, name):
    """The device build against the host's fb_table_build, word for word; a refused key in mid-set has an all-zero table."""
    c = E.CURVES[name]
    f = E.byte_len(c)
    h = KH.Host(ekh, c)
    rng = np.random.default_rng(50 + c["bit_size"])
    q0, q2 = (E.scalar_base_mult(c, K.rnd(rng, c) or 1) for _ in range(2))
    keys = [E.marshal(c, *q0), E.marshal(c, q0[0], (q0[1] + 1) % c["p"]), E.marshal(c, *q2)]
    ks = gpu_ctx.ecdsa_keyset_create(keys, c)
    try:
        info = gpu_ctx.ecdsa_keyset_info(ks)
        w = info["window_bits"]
        assert (info["n_keys"], info["n_refused"]) == (3, 1)
        for i, q in ((0, q0), (2, q2)):
            dev, host = gpu_ctx.selftest_ecdsa_keyset_table(ks, i), h.table(w, q)
            assert dev.shape == host.shape and (dev == host).all(), (name, i, np.flatnonzero(dev != host)[:8])
            assert h.entry(dev, w, 0, 1) == q
        assert not gpu_ctx.selftest_ecdsa_keyset_table(ks, 1).any()
        words = np.zeros(8, dtype=np.uint32)
        assert gpu_ctx.lib.bftkv_gpu_selftest_ecdsa_keyset_table(gpu_ctx.h, ks, 0, words.ctypes.data, 8) == E_NOMEM
        assert gpu_ctx.lib.bftkv_gpu_selftest_ecdsa_keyset_table(gpu_ctx.h, ks, 3, words.ctypes.data, 8) == E_INVALID
        assert f and not words.any()
    finally:
        gpu_ctx.ecdsa_keyset_destroy(ks)


@pytest.mark.parametrize("n_keys", [1, 2, 65])
@pytest.mark.parametrize("name", E.NAMES)
def test_wave_and_block_edges(gpu_ctx, name, n_keys):
    """200 signatures: three full waves and a tail of 8 lanes; the build lanes of 2 and 65 keys straddle keys inside a wave (56
    windows per key on P-224, 132 on P-521)."""
    c = E.CURVES[name]
    rng = np.random.default_rng(61 * c["bit_size"] + n_keys)
    dlen = {"P-224": 28, "P-256": 32, "P-384": 48, "P-521": 64}[name]
    digests, sigs, keys, key_idx, expect = _signed_batch(gpu_ctx, c, rng, 200, n_keys, dlen)
    ks = gpu_ctx.ecdsa_keyset_create(keys, c)
    try:
        assert gpu_ctx.ecdsa_keyset_info(ks)["n_refused"] == 0
        valid, st = gpu_ctx.ecdsa_verify_keyset(ks, digests, sigs, key_idx=None if n_keys == 1 else key_idx)
    finally:
        gpu_ctx.ecdsa_keyset_destroy(ks)
    assert not st.any(), (name, np.flatnonzero(st)[:8])
    assert (valid == expect).all(), (name, np.flatnonzero(valid != expect)[:8])
    assert expect.sum() == 200 - len(range(3, 200, 7))
    for i in [int(v) for v in rng.choice(200, 12, replace=False)] + [3, 10, 17, 199]:
        assert (int(valid[i]), int(st[i])) == V.verify(c, keys[key_idx[i] if n_keys > 1 else 0], digests[i], sigs[i]), (name, i)


@pytest.mark.parametrize("name", E.NAMES)
def test_chosen_digits(gpu_ctx, name):
    """Signatures with a prescribed u2 (the scalar the key's table is walked with): R = u1 G + u2 Q, r = x(R) mod N, s = r / u2,
    e = u1 s.  All VALID; with r + 1 INVALID."""
    c = E.CURVES[name]
    n = c["n"]
    rng = np.random.default_rng(70 + c["bit_size"])
    d = K.rnd(rng, c) or 1
    key = E.marshal(c, *E.scalar_base_mult(c, d))
    ks = gpu_ctx.ecdsa_keyset_create([key], c)
    try:
        w = gpu_ctx.ecdsa_keyset_info(ks)["window_bits"]
        digests, sigs, expect = [], [], []
        for u2 in KH.chosen_scalars(c, w, rng):
            while True:
                u1 = K.rnd(rng, c) or 1
                t = (u1 + u2 * d) % n
                r = E.scalar_base_mult(c, t)[0] % n if t else 0
                if r and r + 1 < n and u1 != u2 * d % n:
                    break
            s = r * pow(u2, -1, n) % n
            for rr, ok in ((r, 1), (r + 1, 0)):
                digests.append(K.digest_for(c, u1 * s % n))
                sigs.append(K.sig_bytes(c, rr, s))
                expect.append(ok)
        valid, st = gpu_ctx.ecdsa_verify_keyset(ks, digests, sigs)
    finally:
        gpu_ctx.ecdsa_keyset_destroy(ks)
    assert not st.any(), (name, np.flatnonzero(st)[:8])
    assert (valid == np.array(expect, dtype=np.uint8)).all(), (name, np.flatnonzero(valid != np.array(expect, dtype=np.uint8))[:8])
    for i in range(12):
        assert (int(valid[i]), int(st[i])) == V.verify(c, key, digests[i], sigs[i]) == (expect[i], V.OK), (name, i)


def test_key_index_is_clamped(gpu_ctx):
    c = E.CURVES["P-256"]
    rng = np.random.default_rng(5)
    digests, sigs, keys, key_idx, expect = _signed_batch(gpu_ctx, c, rng, 6, 2, 32)
    want = [V.verify(c, keys[min(i, 1)], digests[j], sigs[j]) for j, i in enumerate([0, 1, 2, 7, 0xFFFFFFFF, 1])]
    ks = gpu_ctx.ecdsa_keyset_create(keys, c)
    try:
        assert _pairs(*gpu_ctx.ecdsa_verify_keyset(ks, digests, sigs, key_idx=[0, 1, 2, 7, 0xFFFFFFFF, 1])) == want
        assert {w for w in want} == {(1, V.OK), (0, V.OK)}
    finally:
        gpu_ctx.ecdsa_keyset_destroy(ks)


@pytest.mark.parametrize("name", E.NAMES)
def test_device_form_against_host_form(gpu_ctx, name):
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.h
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    c = E.CURVES[name]
    f = E.byte_len(c)
    cases = [cs for cs in K.corpus(name) if len(cs.digest) == f]
    keys = sorted({cs.key for cs in cases})
    idx = [keys.index(cs.key) for cs in cases]
    n_ops = len(cases)
    ks = gpu_ctx.ecdsa_keyset_create(keys, c)
    try:
        valid, st = gpu_ctx.ecdsa_verify_keyset(ks, [cs.digest for cs in cases], [cs.sig for cs in cases], key_idx=idx)
        assert _pairs(valid, st) == [V.verify(c, cs.key, cs.digest, cs.sig) for cs in cases]
        assert st.any() and valid.any()
        d_dg = up(np.frombuffer(b"".join(cs.digest for cs in cases), dtype=np.uint8).copy())
        d_sg = up(np.frombuffer(b"".join(cs.sig for cs in cases), dtype=np.uint8).copy())
        d_ki = up(np.array(idx, dtype=np.uint32).view(np.int32))
        d_valid = torch.full((n_ops + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n_ops + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
        gpu_ctx._check(lib.bftkv_gpu_ecdsa_verify_keyset_dev(h, ks, n_ops, d_dg.data_ptr(), f, d_sg.data_ptr(), d_ki.data_ptr(), d_valid.data_ptr(),
                                                             d_st.data_ptr()), "ecdsa_verify_keyset_dev")
        gpu_ctx.sync()
        assert (d_valid.cpu().numpy()[:n_ops] == valid).all() and (d_st.cpu().numpy()[:n_ops] == st).all(), name
        assert (d_valid.cpu().numpy()[n_ops:] == 0x55).all() and (d_st.cpu().numpy()[n_ops:] == 0x55).all()      # nothing past n_ops
    finally:
        gpu_ctx.ecdsa_keyset_destroy(ks)


def _two_sets(gpu_ctx):
    """A P-256 and a P-384 set over the keys of their corpora, and jobs (set, key index, curve, case) over both."""
    sets, jobs = {}, []
    for name in ("P-256", "P-384"):
        c = E.CURVES[name]
        cases = [cs for cs in K.corpus(name) if len(cs.digest) in (32, 66)]        # two digest lengths, mutations and fences among them
        keys = sorted({cs.key for cs in cases})
        sets[name] = gpu_ctx.ecdsa_keyset_create(keys, c)
        jobs += [(sets[name], keys.index(cs.key), c, cs) for cs in cases]
    return sets, jobs


def test_two_sets_alive_at_once(gpu_ctx):
    sets, jobs = _two_sets(gpu_ctx)
    a, b = sets["P-256"], sets["P-384"]
    assert a != b

    def answers(ks):
        mine = [(k, c, cs) for s, k, c, cs in jobs if s == ks and len(cs.digest) == 32]
        got = gpu_ctx.ecdsa_verify_keyset(ks, [cs.digest for _, _, cs in mine], [cs.sig for _, _, cs in mine], key_idx=[k for k, _, _ in mine])
        return _pairs(*got), [V.verify(c, cs.key, cs.digest, cs.sig) for _, c, cs in mine]

    try:
        for ks in (a, b):
            got, want = answers(ks)
            assert got == want and (1, V.OK) in want
        gpu_ctx.ecdsa_keyset_destroy(a)
        got, want = answers(b)                      # the other still answers
        assert got == want
        # the destroyed handle: BFTKV_E_INVALID, statuses 0xFF, verdicts 0
        buf = np.zeros(4096, dtype=np.uint8)
        P = lambda x: x.ctypes.data_as(C.c_void_p)        # noqa: E731
        valid, st = np.full(8, 0xAA, dtype=np.uint8), np.full(8, 0xAA, dtype=np.uint8)
        assert gpu_ctx.lib.bftkv_gpu_ecdsa_verify_keyset(gpu_ctx.h, a, 4, P(buf), 32, P(buf), None, P(valid), P(st)) == E_INVALID
        assert (st[:4] == FAILED).all() and (valid[:4] == 0).all() and (st[4:] == 0xAA).all() and (valid[4:] == 0xAA).all()
        assert gpu_ctx.lib.bftkv_gpu_ecdsa_keyset_destroy(gpu_ctx.h, a) == E_INVALID
        assert gpu_ctx.lib.bftkv_gpu_ecdsa_keyset_info(gpu_ctx.h, a, None, None, None, None) == E_INVALID
        # a new set takes the free handle and answers for its own curve
        c = E.CURVES["P-224"]
        cs = K.corpus("P-224")[0]
        a2 = gpu_ctx.ecdsa_keyset_create([cs.key], c)
        assert a2 == a
        assert _pairs(*gpu_ctx.ecdsa_verify_keyset(a2, [cs.digest], [cs.sig])) == [(1, V.OK)]
        gpu_ctx.ecdsa_keyset_destroy(a2)
    finally:
        gpu_ctx.ecdsa_keyset_destroy(b)


def test_batcher(gpu_ctx):
    """3 threads, 40 calls each, over two sets and two digest lengths, mutated and fenced cases among them.  The lanes are forks: they
    read the root's sets.  Callers of one group share device calls."""
    from bftkv_amd import Batcher
    sets, jobs = _two_sets(gpu_ctx)
    try:
        # call i of every thread is of one (set, digest length) group: what arrives while the lane is busy can share a call
        groups = {}
        for j in jobs:
            groups.setdefault((j[0], len(j[3].digest)), []).append(j)
        order = sorted(groups)
        assert len(order) == 4
        plan = [[groups[order[(i // 5) % 4]][(3 * i + t) % len(groups[order[(i // 5) % 4]])] for i in range(40)] for t in range(3)]
        want = [[V.verify(c, cs.key, cs.digest, cs.sig) for _, _, c, cs in row] for row in plan]
        assert {w for row in want for w in row} == {(1, V.OK), (0, V.OK), (0, V.FENCED)}
        b = Batcher(gpu_ctx, max_items=64, n_lanes=1)
        got = [[None] * 40 for _ in range(3)]

        def run(t):
            for i, (ks, key, _, cs) in enumerate(plan[t]):
                got[t][i] = b.ecdsa_verify_keyset(ks, key, cs.digest, cs.sig)

        th = [threading.Thread(target=run, args=(t,)) for t in range(3)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        stats = b.stats()
        # errors of one caller alone: an unknown handle, an empty digest
        P = lambda x: x.ctypes.data_as(C.c_void_p)        # noqa: E731
        buf, v1, s1 = np.zeros(256, dtype=np.uint8), np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        assert gpu_ctx.lib.bftkv_gpu_batcher_ecdsa_verify_keyset(b.h, 999, 0, P(buf), 32, P(buf), P(v1), P(s1)) == E_INVALID
        assert (int(v1[0]), int(s1[0])) == (0, FAILED)
        v1[0], s1[0] = 0xAA, 0
        assert gpu_ctx.lib.bftkv_gpu_batcher_ecdsa_verify_keyset(b.h, sets["P-256"], 0, P(buf), 0, P(buf), P(v1), P(s1)) == E_INVALID
        assert (int(v1[0]), int(s1[0])) == (0, FAILED)
        v1[0], s1[0] = 0xAA, 0
        assert gpu_ctx.lib.bftkv_gpu_batcher_ecdsa_verify_keyset(None, sets["P-256"], 0, P(buf), 32, P(buf), P(v1), P(s1)) == E_INVALID
        assert (int(v1[0]), int(s1[0])) == (0, FAILED)
        b.close()
        for t in range(3):
            for i in range(40):
                assert got[t][i] == (0, want[t][i][1], want[t][i][0]), (t, i, plan[t][i][3].label, want[t][i], got[t][i])
        print("batcher:", stats)
        assert stats["calls"] == 120 and stats["batches"] < 120, stats
    finally:
        for ks in sets.values():
            gpu_ctx.ecdsa_keyset_destroy(ks)


def test_errors(gpu_ctx):
    from bftkv_amd._native import NativeError, _curve_bytes
    c = E.CURVES["P-256"]
    cs = K.corpus("P-256")[0]
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cb, bits, f = _curve_bytes(c)
    other = dict(c, b=c["b"] ^ 1)
    cb2, bits2, _ = _curve_bytes(other)
    P = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    key = np.frombuffer(cs.key, dtype=np.uint8).copy()
    many = np.zeros(4097 * (1 + 2 * f), dtype=np.uint8)
    out = C.c_int(-7)
    create = lambda *a: lib.bftkv_gpu_ecdsa_keyset_create(*a)     # noqa: E731
    assert create(h, 0, P(key), P(cb), bits, C.byref(out)) == E_INVALID
    assert create(h, 4097, P(many), P(cb), bits, C.byref(out)) == E_INVALID
    assert create(h, 1, None, P(cb), bits, C.byref(out)) == E_INVALID
    assert create(h, 1, P(key), None, bits, C.byref(out)) == E_INVALID
    assert create(h, 1, P(key), P(cb), bits, None) == E_INVALID
    assert create(None, 1, P(key), P(cb), bits, C.byref(out)) == E_INVALID
    assert create(h, 1, P(key), P(cb2), bits2, C.byref(out)) == E_UNSUPPORTED        # a group that is not one of the four
    assert create(h, 1, P(key), P(cb), 255, C.byref(out)) == E_UNSUPPORTED
    assert out.value == -7
    with pytest.raises(NativeError, match=r"\(-4\)"):
        gpu_ctx.ecdsa_keyset_create([cs.key], other)
    ks = gpu_ctx.ecdsa_keyset_create([cs.key], c)
    fork = gpu_ctx.fork()
    try:
        # key sets are made and unmade on the root; the fork reads them
        assert create(fork.h, 1, P(key), P(cb), bits, C.byref(out)) == E_STATE
        assert lib.bftkv_gpu_ecdsa_keyset_destroy(fork.h, ks) == E_STATE
        assert fork.ecdsa_keyset_info(ks) == gpu_ctx.ecdsa_keyset_info(ks)
        assert _pairs(*fork.ecdsa_verify_keyset(ks, [cs.digest], [cs.sig])) == [(1, V.OK)]
        dg, sg = np.frombuffer(cs.digest, dtype=np.uint8).copy(), np.frombuffer(cs.sig, dtype=np.uint8).copy()
        valid, st = np.full(8, 0xAA, dtype=np.uint8), np.full(8, 0xAA, dtype=np.uint8)
        call = lambda *a: lib.bftkv_gpu_ecdsa_verify_keyset(*a)     # noqa: E731
        for bad_dlen in (0, 67):
            valid[:], st[:] = 0xAA, 0xAA
            assert call(h, ks, 1, P(dg), bad_dlen, P(sg), None, P(valid), P(st)) == E_INVALID
            assert (int(valid[0]), int(st[0])) == (0, FAILED) and (valid[1:] == 0xAA).all() and (st[1:] == 0xAA).all()      # fail closed
        assert call(None, ks, 1, P(dg), 32, P(sg), None, P(valid), P(st)) == E_INVALID
        assert call(h, ks, 1, None, 32, P(sg), None, P(valid), P(st)) == E_INVALID
        assert call(h, ks, 1, P(dg), 32, None, None, P(valid), P(st)) == E_INVALID
        assert call(h, ks, 1, P(dg), 32, P(sg), None, None, P(st)) == E_INVALID
        assert call(h, ks, 1, P(dg), 32, P(sg), None, P(valid), None) == E_INVALID
        assert call(h, -1, 1, P(dg), 32, P(sg), None, P(valid), P(st)) == E_INVALID
        assert call(h, ks + 100, 1, P(dg), 32, P(sg), None, P(valid), P(st)) == E_INVALID
        assert (int(valid[0]), int(st[0])) == (0, FAILED)
        assert call(h, ks, 0, None, 32, None, None, None, None) == 0                 # n_ops = 0
        assert call(h, ks, 1, P(dg), len(cs.digest), P(sg), None, P(valid), P(st)) == 0
        assert (int(valid[0]), int(st[0])) == (1, V.OK)
    finally:
        fork.close()
        gpu_ctx.ecdsa_keyset_destroy(ks)
