"""-m gpu: resident DSA key sets.  Groups and keys registered once (Montgomery rows and a fixed-base window table per g and y on the
device), then verification as a chain of table products: byte for byte (valid, status) against the restatement with its rules
(tests/dsa_verify_ref.py) and against the raw entry bftkv_gpu_dsa_verify, and the device-built tables limb for limb against tables
built by pow() (tests/dsa_keyset_host.py).  Shapes are the smallest at which the kernels can still go wrong."""
import ctypes as C
import contextlib
import functools
import json
import os
import threading

import numpy as np
import pytest

import dsa_keyset_host as KH
import dsa_verify_cases as K
import dsa_verify_ref as V
from test_gpu_dsa_verify import GPU_NAMES

pytestmark = pytest.mark.gpu
E_INVALID, E_NOMEM, E_UNSUPPORTED, E_STATE = -1, -3, -4, -5
FAILED = 0xFF
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731


def _pairs(valid, st):
    return [(int(v), int(s)) for v, s in zip(valid, st)]


@contextlib.contextmanager
def _keyset(ctx, keys, groups, **kw):
    ks = ctx.dsa_keyset_create(keys, groups, **kw)
    try:
        yield ks
    finally:
        ctx.dsa_keyset_destroy(ks)


def _standard(name, i=0):
    k = json.load(open(os.path.join(K.GOLDEN, "keys_%s.json" % name)))["keys"][i]
    p, q, g, x = (int(k[f], 16) for f in ("p", "q", "g", "x"))
    return p, q, g, x, pow(g, x, p)


def _sign(rng, p, q, g, x, dg):
    rs = None
    while rs is None:
        rs = K.sign(p, q, g, x, dg, K.rnd(rng, q) or 1)
    return rs


def _sig(r, s, qbytes):
    return r.to_bytes(qbytes, "big") + s.to_bytes(qbytes, "big")


@functools.lru_cache(maxsize=None)
def _corpus_want(name):
    return tuple(V.verify(cs.p, cs.q, cs.g, cs.y, cs.digest, cs.r, cs.s) for cs in K.corpus(name))


@pytest.mark.parametrize("w", [4, 5, 8])
@pytest.mark.parametrize("name", GPU_NAMES)
def test_corpus(gpu_ctx, name, w):
    """Every case under its own (mutated) g and y: about a dozen distinct bases per group.  One call per digest length; the key set,
    the raw entry and the restatement agree on every case."""
    G = K.group(name)
    cases, want = K.corpus(name), _corpus_want(name)
    gs, ks, idx = K.tables(cases)
    with _keyset(gpu_ctx, ks, gs, window_bits=w, pbytes=G.pbytes, qbytes=G.qbytes) as h:
        info = gpu_ctx.dsa_keyset_info(h)
        print(name, info)
        windows = -(-max(q.bit_length() for _, q, _ in gs) // w)
        assert info == {"n_keys": len(ks), "n_groups": len(gs), "pbytes": G.pbytes, "qbytes": G.qbytes, "window_bits": w, "windows": windows,
                        "table_bytes": (len(gs) + len(ks)) * windows * ((1 << w) - 1) * 304}
        got, raw = [None] * len(cases), [None] * len(cases)
        for dlen, ids in K.by_dlen(cases).items():
            dg, sg, ki = [cases[i].digest for i in ids], [K.sig_bytes(G, cases[i].r, cases[i].s) for i in ids], [idx[i] for i in ids]
            for out, (valid, st) in ((got, gpu_ctx.dsa_verify_keyset(h, dg, sg, key_idx=ki)),
                                     (raw, gpu_ctx.dsa_verify(dg, sg, ks, gs, key_idx=ki, pbytes=G.pbytes, qbytes=G.qbytes))):
                for j, i in enumerate(ids):
                    out[i] = (int(valid[j]), int(st[j]))
    for cs, wt, g, r in zip(cases, want, got, raw):
        print(name, w, cs.label, "want", wt, "key set", g, "raw entry", r)
    bad = [(cs.label, wt, g, r) for cs, wt, g, r in zip(cases, want, got, raw) if not wt == g == r]
    assert not bad, (name, w, bad)


@pytest.mark.parametrize("w", [4, 6])
@pytest.mark.parametrize("name", ["dsa1024", "dsa2048"])
def test_table_identity(gpu_ctx, name, w):
    """The device's words against the pow() table, limb for limb: g, y, and y + p where it fits the width (the same table as y's: an
    entry is fully reduced, so a table is a function of b mod p, p and w)."""
    p, q, g, x, y = _standard(name)
    bases = [g, y] + ([y + p] if (y + p).bit_length() <= 2048 else [])
    if name == "dsa1024":
        assert len(bases) == 3
    keys = [(0, b) for b in bases[1:]]
    with _keyset(gpu_ctx, keys, [(p, q, g)], window_bits=w, pbytes=256, qbytes=K.nbytes(q)) as h:
        info = gpu_ctx.dsa_keyset_info(h)
        windows = info["windows"]
        assert windows == -(-q.bit_length() // w)
        rinv = pow(KH.R, -1, p)
        for i, b in enumerate(bases):
            dev, host = gpu_ctx.selftest_dsa_keyset_table(h, i), KH.table_words(b, p, w, windows)
            assert dev.shape == host.shape and (dev == host).all(), (name, w, i, np.argwhere(dev != host)[:4])
            assert KH.decode(dev[0, 0]) == b * KH.R % p and KH.decode(dev[0, 0]) * rinv % p == b % p       # (window 0, d = 1) is b R mod p
        words = np.zeros(8, dtype=np.uint32)
        assert gpu_ctx.lib.bftkv_gpu_selftest_dsa_keyset_table(gpu_ctx.h, h, 0, words.ctypes.data, 8) == E_NOMEM
        full = windows * ((1 << w) - 1) * 76
        big = np.zeros(full, dtype=np.uint32)
        assert gpu_ctx.lib.bftkv_gpu_selftest_dsa_keyset_table(gpu_ctx.h, h, 0, big.ctypes.data, full - 1) == E_NOMEM
        assert gpu_ctx.lib.bftkv_gpu_selftest_dsa_keyset_table(gpu_ctx.h, h, len(bases), big.ctypes.data, full) == E_INVALID
        assert not words.any() and not big.any()


def _prescribed(q, w, rng):
    """(u1, u2) pairs at which a table walk can go wrong.  None stands for a random exponent."""
    bits = q.bit_length()
    top = (bits - 1) // w
    assert bits - w * top < w or bits % w == 0    # the top window is narrower than w where w does not divide the order's length
    ones = min((1 << (w * (top + 1))) - 1, q - 1)
    lone = [1, 3 << (w * (top // 2)), 1 << (w * top)]       # a lone digit in the lowest, a middle and the top window, all below q
    assert all(0 < e < q for e in lone)
    pairs = [(e, None) for e in lone] + [(None, e) for e in lone]
    pairs += [(ones, ones), (ones, None), (None, ones), (0, None), (None, 1), (0, 1), (1, 1)]
    return [(rng_or(u1, q, rng), rng_or(u2, q, rng) or 1) for u1, u2 in pairs]


def rng_or(v, q, rng):
    return K.rnd(rng, q) if v is None else v


@pytest.mark.parametrize("w", [5, 8])
@pytest.mark.parametrize("name", ["dsa1024", "dsa1536", "dsa2048"])
def test_chosen_digits(gpu_ctx, name, w):
    """Signatures with prescribed (u1, u2): k = u1 + x u2, r = g^k mod p mod q, s = r / u2, z = u1 s mod q.  All VALID; with r + 1
    all INVALID."""
    p, q, g, x, y = _standard(name)
    qb = K.nbytes(q)
    rng = np.random.default_rng(90 + w + q.bit_length())
    digests, sigs, expect, labels = [], [], [], []
    for u1, u2 in _prescribed(q, w, rng):
        r = pow(g, (u1 + x * u2) % q, p) % q
        assert r and r + 1 < q
        s = r * pow(u2, -1, q) % q
        z = u1 * s % q
        assert V.prep(q, z.to_bytes(qb, "big"), r, s) == (V.OK, 0, u1, u2)
        for rr, ok in ((r, 1), (r + 1, 0)):
            digests.append(z.to_bytes(qb, "big")); sigs.append(_sig(rr, s, qb)); expect.append(ok); labels.append((hex(u1), hex(u2), ok))
    assert bytes(qb) in digests                   # u1 = 0 through an all-zero digest
    with _keyset(gpu_ctx, [(0, y)], [(p, q, g)], window_bits=w) as h:
        valid, st = gpu_ctx.dsa_verify_keyset(h, digests, sigs)
    want = [V.verify(p, q, g, y, dg, int.from_bytes(sg[:qb], "big"), int.from_bytes(sg[qb:], "big")) for dg, sg in zip(digests, sigs)]
    assert want == [(e, V.OK) for e in expect]
    bad = [(lb, g_) for lb, g_, wt in zip(labels, _pairs(valid, st), want) if g_ != wt]
    assert not bad, (name, w, bad)


def test_twelve_bit_windows(gpu_ctx):
    """w = 12: 16 parts per window in the build, 22 windows of 4,095 entries (27 MB per base).  Honest signatures only."""
    p, q, g, x, y = _standard("dsa2048", 1)
    rng = np.random.default_rng(12)
    digests = [rng.bytes(32) for _ in range(20)]
    sigs = [_sig(*_sign(rng, p, q, g, x, dg), 32) for dg in digests]
    with _keyset(gpu_ctx, [(0, y)], [(p, q, g)], window_bits=12) as h:
        info = gpu_ctx.dsa_keyset_info(h)
        assert (info["windows"], info["table_bytes"]) == (22, 2 * 22 * 4095 * 304)
        valid, st = gpu_ctx.dsa_verify_keyset(h, digests, sigs)
    assert _pairs(valid, st) == [(1, V.OK)] * 20


@functools.lru_cache(maxsize=None)
def _volume(n_keys):
    """200 honest signatures under n_keys keys of keys_dsa2048.json, every 7th one forged."""
    rng = np.random.default_rng(700 + n_keys)
    grp = [_standard("dsa2048", i) for i in range(n_keys)]
    gs = []
    for p, q, g, _, _ in grp:
        if (p, q, g) not in gs:
            gs.append((p, q, g))
    ks = [(gs.index((p, q, g)), y) for p, q, g, _, y in grp]
    digests, sigs, idx, expect = [], [], [], []
    for i in range(200):
        ki = int(rng.integers(n_keys))
        p, q, g, x, _ = grp[ki]
        dg = rng.bytes(32)
        r, s = _sign(rng, p, q, g, x, dg)
        ok = 1
        if i % 7 == 3:
            ok = 0
            which = (i // 7) % 3
            if which == 0:
                r ^= 1 << int(rng.integers(255))
            elif which == 1:
                s ^= 1 << int(rng.integers(255))
            else:
                dg = bytes(K.flip_int(int.from_bytes(dg, "big"), int(rng.integers(256))).to_bytes(32, "big"))
        digests.append(dg); sigs.append(_sig(r, s, 32)); idx.append(ki); expect.append(ok)
    return grp, gs, ks, digests, sigs, idx, expect


@pytest.mark.parametrize("n_keys", [1, 2, 65])
def test_wave_and_block_edges(gpu_ctx, n_keys):
    """16 lane groups make a wave and 64 a block: one under, exactly, one over, a lone signature, and three blocks with a tail.  The
    build's lane groups (32 windows per base at w = 8) straddle bases inside a wave."""
    grp, gs, ks, digests, sigs, idx, expect = _volume(n_keys)
    rng = np.random.default_rng(n_keys)
    with _keyset(gpu_ctx, ks, gs, pbytes=256, qbytes=32) as h:
        assert gpu_ctx.dsa_keyset_info(h)["window_bits"] == 8
        for n_ops in (1, 15, 16, 17, 63, 64, 65, 200):
            lo = 0 if n_ops == 200 else 3          # (the shorter ones start at a forged signature)
            sl = slice(lo, lo + n_ops)
            valid, st = gpu_ctx.dsa_verify_keyset(h, digests[sl], sigs[sl], key_idx=None if n_keys == 1 else idx[sl])
            assert not st.any(), (n_ops, np.flatnonzero(st)[:8])
            assert [int(v) for v in valid] == expect[sl], (n_ops, n_keys)
            for j in sorted({0, n_ops - 1} | {int(v) for v in rng.choice(n_ops, min(n_ops, 4), replace=False)}):
                i = lo + j
                p, q, g, _, y = grp[idx[i]]
                assert (int(valid[j]), int(st[j])) == V.verify(p, q, g, y, digests[i], int.from_bytes(sigs[i][:32], "big"), int.from_bytes(sigs[i][32:], "big"))
    assert sum(expect) == 200 - len(range(3, 200, 7))


def test_mixed_groups_in_one_set(gpu_ctx):
    """1024/160, 1536/224 and 2048/256 in one set with qbytes = 32: the window count follows the widest order and the shorter orders
    verify with all-zero top windows.  At dlen = 32 the signatures under the shorter orders are fenced."""
    rng = np.random.default_rng(41)
    grp = [_standard(n) for n in ("dsa1024", "dsa1536", "dsa2048")]
    gs, ks = [(p, q, g) for p, q, g, _, _ in grp], [(i, t[4]) for i, t in enumerate(grp)]
    with _keyset(gpu_ctx, ks, gs, pbytes=256, qbytes=32) as h:
        assert gpu_ctx.dsa_keyset_info(h)["windows"] == 32
        for dlen in (20, 32):
            digests, sigs, idx, want = [], [], [], []
            for j in range(18):
                gi = j % 3
                p, q, g, x, y = grp[gi]
                dg = rng.bytes(dlen)
                r, s = _sign(rng, p, q, g, x, dg if dlen <= q.bit_length() // 8 else dg[:q.bit_length() // 8])
                if j % 6 >= 3:
                    s ^= 1
                digests.append(dg); sigs.append(_sig(r, s, 32)); idx.append(gi)
                want.append(V.verify(p, q, g, y, dg, r, s))
            got = _pairs(*gpu_ctx.dsa_verify_keyset(h, digests, sigs, key_idx=idx))
            raw = _pairs(*gpu_ctx.dsa_verify(digests, sigs, ks, gs, key_idx=idx, pbytes=256, qbytes=32))
            assert got == want == raw, dlen
            if dlen == 20:
                assert [v for v, _ in got] == [1, 1, 1, 0, 0, 0] * 3
            else:
                assert [s for _, s in got] == [V.FENCED, V.FENCED, V.OK] * 6


def _two_key_batch(rng, n=6):
    grp = [_standard("dsa2048", i) for i in range(2)]
    gs = []
    for p, q, g, _, _ in grp:
        if (p, q, g) not in gs:
            gs.append((p, q, g))
    ks = [(gs.index((p, q, g)), y) for p, q, g, _, y in grp]
    digests = [rng.bytes(32) for _ in range(n)]
    signer = [j % 2 for j in range(n)]
    sigs = [_sig(*_sign(rng, *grp[k][:4], dg), 32) for dg, k in zip(digests, signer)]
    return grp, gs, ks, digests, sigs


def test_key_index_is_clamped(gpu_ctx):
    grp, gs, ks, digests, sigs = _two_key_batch(np.random.default_rng(5))
    key_idx = [0, 1, 2, 7, 0xFFFFFFFF, 1]
    want = []
    for dg, sg, ki in zip(digests, sigs, key_idx):
        p, q, g, _, y = grp[min(ki, 1)]
        want.append(V.verify(p, q, g, y, dg, int.from_bytes(sg[:32], "big"), int.from_bytes(sg[32:], "big")))
    assert {w for w in want} == {(1, V.OK), (0, V.OK)}
    with _keyset(gpu_ctx, ks, gs, window_bits=4) as h:
        assert _pairs(*gpu_ctx.dsa_verify_keyset(h, digests, sigs, key_idx=key_idx)) == want
        # NULL key_idx: key 0 for all
        assert [int(v) for v in gpu_ctx.dsa_verify_keyset(h, digests, sigs)[0]] == [1, 0, 1, 0, 1, 0]


def test_device_form_against_host_form(gpu_ctx):
    import torch
    lib, ch = gpu_ctx.lib, gpu_ctx.h
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")    # noqa: E731
    for name in ("composite_q160", "p2048_q256"):
        G = K.group(name)
        dlen = max(K.by_dlen(K.corpus(name)))                                # (the fenced ones: one byte more than the order)
        pool = [cs for cs in K.corpus(name) if len(cs.digest) == G.q.bit_length() // 8]
        for cases in ([cs for cs in K.corpus(name) if len(cs.digest) == dlen], [pool[i % len(pool)] for i in range(70)]):
            gs, ks, idx = K.tables(cases)
            n = len(cases)
            want = [V.verify(cs.p, cs.q, cs.g, cs.y, cs.digest, cs.r, cs.s) for cs in cases]
            with _keyset(gpu_ctx, ks, gs, window_bits=5, pbytes=G.pbytes, qbytes=G.qbytes) as h:
                dg = np.frombuffer(b"".join(cs.digest for cs in cases), dtype=np.uint8).copy()
                sg = np.frombuffer(b"".join(K.sig_bytes(G, cs.r, cs.s) for cs in cases), dtype=np.uint8).copy()
                ki = np.array(idx, dtype=np.uint32)
                valid, st = np.full(n + 8, 0x55, dtype=np.uint8), np.full(n + 8, 0x55, dtype=np.uint8)
                gpu_ctx._check(lib.bftkv_gpu_dsa_verify_keyset(ch, h, n, P(dg), len(cases[0].digest), P(sg), P(ki), P(valid), P(st)), "dsa_verify_keyset")
                assert _pairs(valid[:n], st[:n]) == want
                assert (valid[n:] == 0x55).all() and (st[n:] == 0x55).all()                            # nothing past n_ops
                d_dg, d_sg, d_ki = up(dg), up(sg), up(ki.view(np.int32))
                d_valid = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
                d_st = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
                gpu_ctx._check(lib.bftkv_gpu_dsa_verify_keyset_dev(ch, h, n, d_dg.data_ptr(), len(cases[0].digest), d_sg.data_ptr(), d_ki.data_ptr(),
                                                                   d_valid.data_ptr(), d_st.data_ptr()), "dsa_verify_keyset_dev")
                gpu_ctx.sync()
                assert (d_valid.cpu().numpy()[:n] == valid[:n]).all() and (d_st.cpu().numpy()[:n] == st[:n]).all(), name
                assert (d_valid.cpu().numpy()[n:] == 0x55).all() and (d_st.cpu().numpy()[n:] == 0x55).all()


def _two_sets(gpu_ctx):
    """A set over the composite 160-bit group's corpus and one over dsa2048's, and jobs (set, key index, group, case) over both, each
    of two digest lengths (the order's bytes and one more: the fenced ones)."""
    sets, jobs = {}, []
    for name in ("composite_q160", "dsa2048"):
        G = K.group(name)
        qb = G.q.bit_length() // 8
        cases = [cs for cs in K.corpus(name) if len(cs.digest) in (qb, qb + 1)]
        gs, ks, idx = K.tables(cases)
        sets[name] = gpu_ctx.dsa_keyset_create(ks, gs, window_bits=4, pbytes=G.pbytes, qbytes=G.qbytes)
        jobs += [(sets[name], ki, G, cs) for ki, cs in zip(idx, cases)]
    return sets, jobs


def _verdict(cs):
    return V.verify(cs.p, cs.q, cs.g, cs.y, cs.digest, cs.r, cs.s)


def test_two_sets_alive_at_once(gpu_ctx):
    sets, jobs = _two_sets(gpu_ctx)
    a, b = sets["composite_q160"], sets["dsa2048"]
    assert a != b

    def answers(ks):
        mine = [(k, G, cs) for s, k, G, cs in jobs if s == ks and len(cs.digest) == G.q.bit_length() // 8]
        got = gpu_ctx.dsa_verify_keyset(ks, [cs.digest for _, _, cs in mine], [K.sig_bytes(G, cs.r, cs.s) for _, G, cs in mine], key_idx=[k for k, _, _ in mine])
        return _pairs(*got), [_verdict(cs) for _, _, cs in mine]

    try:
        for ks in (a, b):
            got, want = answers(ks)
            assert got == want and (1, V.OK) in want
        gpu_ctx.dsa_keyset_destroy(a)
        got, want = answers(b)                      # the other still answers
        assert got == want
        # the destroyed handle: BFTKV_E_INVALID, statuses 0xFF, verdicts 0
        buf = np.zeros(4096, dtype=np.uint8)
        valid, st = np.full(8, 0xAA, dtype=np.uint8), np.full(8, 0xAA, dtype=np.uint8)
        assert gpu_ctx.lib.bftkv_gpu_dsa_verify_keyset(gpu_ctx.h, a, 4, P(buf), 20, P(buf), None, P(valid), P(st)) == E_INVALID
        assert (st[:4] == FAILED).all() and (valid[:4] == 0).all() and (st[4:] == 0xAA).all() and (valid[4:] == 0xAA).all()
        assert gpu_ctx.lib.bftkv_gpu_dsa_keyset_destroy(gpu_ctx.h, a) == E_INVALID
        assert gpu_ctx.lib.bftkv_gpu_dsa_keyset_info(gpu_ctx.h, a, None, None, None, None, None, None, None) == E_INVALID
        # a new set takes the free handle and answers for its own group
        p, q, g, x, y = _standard("dsa1536")
        rng = np.random.default_rng(3)
        dg = rng.bytes(28)
        a2 = gpu_ctx.dsa_keyset_create([(0, y)], [(p, q, g)], window_bits=4)
        assert a2 == a
        assert _pairs(*gpu_ctx.dsa_verify_keyset(a2, [dg], [_sig(*_sign(rng, p, q, g, x, dg), 28)])) == [(1, V.OK)]
        gpu_ctx.dsa_keyset_destroy(a2)
    finally:
        gpu_ctx.dsa_keyset_destroy(b)


def test_batcher(gpu_ctx):
    """3 threads, 40 calls each, over two sets and two digest lengths, mutated and fenced cases among them.  The lanes are forks: they
    read the root's sets.  Callers of one group share device calls."""
    from bftkv_amd import Batcher
    sets, jobs = _two_sets(gpu_ctx)
    try:
        groups = {}
        for j in jobs:
            groups.setdefault((j[0], len(j[3].digest)), []).append(j)
        order = sorted(groups)
        assert len(order) == 4
        plan = [[groups[order[(i // 5) % 4]][(3 * i + t) % len(groups[order[(i // 5) % 4]])] for i in range(40)] for t in range(3)]
        want = [[_verdict(cs) for _, _, _, cs in row] for row in plan]
        assert {w for row in want for w in row} >= {(1, V.OK), (0, V.OK), (0, V.FENCED)}
        b = Batcher(gpu_ctx, max_items=64, n_lanes=1)
        got = [[None] * 40 for _ in range(3)]

        def run(t):
            for i, (ks, key, G, cs) in enumerate(plan[t]):
                got[t][i] = b.dsa_verify_keyset(ks, key, cs.digest, K.sig_bytes(G, cs.r, cs.s))

        th = [threading.Thread(target=run, args=(t,)) for t in range(3)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        stats = b.stats()
        # errors of one caller alone: an unknown handle, an empty digest, no batcher
        buf, v1, s1 = np.zeros(256, dtype=np.uint8), np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        call = gpu_ctx.lib.bftkv_gpu_batcher_dsa_verify_keyset
        assert call(b.h, 999, 0, P(buf), 20, P(buf), P(v1), P(s1)) == E_INVALID
        assert (int(v1[0]), int(s1[0])) == (0, FAILED)
        v1[0], s1[0] = 0xAA, 0
        assert call(b.h, sets["dsa2048"], 0, P(buf), 0, P(buf), P(v1), P(s1)) == E_INVALID
        assert (int(v1[0]), int(s1[0])) == (0, FAILED)
        v1[0], s1[0] = 0xAA, 0
        assert call(None, sets["dsa2048"], 0, P(buf), 32, P(buf), P(v1), P(s1)) == E_INVALID
        assert (int(v1[0]), int(s1[0])) == (0, FAILED)
        # and a good call after them
        _, key, G, cs = next(j for j in jobs if j[0] == sets["dsa2048"] and _verdict(j[3]) == (1, V.OK))
        assert b.dsa_verify_keyset(sets["dsa2048"], key, cs.digest, K.sig_bytes(G, cs.r, cs.s)) == (0, V.OK, 1)
        b.close()
        for t in range(3):
            for i in range(40):
                assert got[t][i] == (0, want[t][i][1], want[t][i][0]), (t, i, plan[t][i][3].label, want[t][i], got[t][i])
        print("batcher:", stats)
        assert stats["calls"] == 120 and stats["batches"] < 120, stats
    finally:
        for ks in sets.values():
            gpu_ctx.dsa_keyset_destroy(ks)


def test_errors(gpu_ctx):
    from bftkv_amd._native import NativeError, _ints_to_be
    lib, h = gpu_ctx.lib, gpu_ctx.h
    p, q, g, x, y = _standard("dsa1024")
    rng = np.random.default_rng(77)
    dgb = rng.bytes(20)
    sgb = _sig(*_sign(rng, p, q, g, x, dgb), 20)
    pb, qb = 128, 20
    a = dict(p=_ints_to_be([p], pb), q=_ints_to_be([q], qb), g=_ints_to_be([g], pb), y=_ints_to_be([y], pb), kg=np.zeros(1, dtype=np.uint32))
    out = C.c_int(-7)

    def create(ctx=h, n_keys=1, y=a["y"], kg=a["kg"], pbytes=pb, n_groups=1, p=a["p"], q=a["q"], g=a["g"], qbytes=qb, w=4, res=C.byref(out)):
        return lib.bftkv_gpu_dsa_keyset_create(ctx, n_keys, P(y), P(kg), pbytes, n_groups, P(p), P(q), P(g), qbytes, w, res)

    even_p, even_q = a["p"].copy(), a["q"].copy()
    even_p[0, -1] &= 0xFE
    even_q[0, -1] &= 0xFE
    wide = np.zeros((1, 257), dtype=np.uint8)
    wide[0, -1] = 1
    refused = [(dict(ctx=None), E_INVALID), (dict(y=None), E_INVALID), (dict(p=None), E_INVALID), (dict(q=None), E_INVALID), (dict(g=None), E_INVALID),
               (dict(res=None), E_INVALID), (dict(n_keys=0), E_INVALID), (dict(n_keys=4097), E_INVALID), (dict(n_groups=0), E_INVALID),
               (dict(n_groups=4097), E_INVALID), (dict(w=3), E_INVALID), (dict(w=17), E_INVALID), (dict(pbytes=257, p=wide, g=wide, y=wide), E_INVALID),
               (dict(pbytes=0), E_INVALID), (dict(qbytes=33), E_INVALID), (dict(qbytes=0), E_INVALID), (dict(p=even_p), E_UNSUPPORTED),
               (dict(q=even_q), E_UNSUPPORTED)]
    for kw, code in refused:
        assert create(**kw) == code, (list(kw), code)
        assert out.value == -7, list(kw)                               # *keyset_out untouched
    with pytest.raises(NativeError, match=r"\(-4\)"):
        gpu_ctx.dsa_keyset_create([(0, y)], [(p - 1, q, g)])
    assert create(kg=None) == 0                                        # NULL key_group: group 0
    gpu_ctx.dsa_keyset_destroy(out.value)
    out.value = -7
    ks = gpu_ctx.dsa_keyset_create([(0, y)], [(p, q, g)], window_bits=4)
    fork = gpu_ctx.fork()
    try:
        # key sets are made and unmade on the root; the fork reads them
        assert create(ctx=fork.h) == E_STATE and out.value == -7
        assert lib.bftkv_gpu_dsa_keyset_destroy(fork.h, ks) == E_STATE
        assert fork.dsa_keyset_info(ks) == gpu_ctx.dsa_keyset_info(ks)
        assert gpu_ctx.dsa_keyset_info(ks) == {"n_keys": 1, "n_groups": 1, "pbytes": 128, "qbytes": 20, "window_bits": 4, "windows": 40,
                                               "table_bytes": 2 * 40 * 15 * 304}
        assert _pairs(*fork.dsa_verify_keyset(ks, [dgb], [sgb])) == [(1, V.OK)]
        dg, sg = np.frombuffer(dgb, dtype=np.uint8).copy(), np.frombuffer(sgb, dtype=np.uint8).copy()
        valid, st = np.full(8, 0xAA, dtype=np.uint8), np.full(8, 0xAA, dtype=np.uint8)
        call = lib.bftkv_gpu_dsa_verify_keyset
        for bad_dlen in (0, 65):
            valid[:], st[:] = 0xAA, 0xAA
            assert call(h, ks, 1, P(dg), bad_dlen, P(sg), None, P(valid), P(st)) == E_INVALID
            assert (int(valid[0]), int(st[0])) == (0, FAILED) and (valid[1:] == 0xAA).all() and (st[1:] == 0xAA).all()      # fail closed
        assert call(None, ks, 1, P(dg), 20, P(sg), None, P(valid), P(st)) == E_INVALID
        assert call(h, ks, 1, None, 20, P(sg), None, P(valid), P(st)) == E_INVALID
        assert call(h, ks, 1, P(dg), 20, None, None, P(valid), P(st)) == E_INVALID
        assert call(h, ks, 1, P(dg), 20, P(sg), None, None, P(st)) == E_INVALID
        assert call(h, ks, 1, P(dg), 20, P(sg), None, P(valid), None) == E_INVALID
        valid[:], st[:] = 0xAA, 0xAA
        assert call(h, -1, 1, P(dg), 20, P(sg), None, P(valid), P(st)) == E_INVALID
        assert call(h, ks + 100, 1, P(dg), 20, P(sg), None, P(valid), P(st)) == E_INVALID
        assert (int(valid[0]), int(st[0])) == (0, FAILED)
        assert call(h, ks, 0, None, 20, None, None, None, None) == 0                 # n_ops = 0
        assert call(h, ks, 1, P(dg), 20, P(sg), None, P(valid), P(st)) == 0
        assert (int(valid[0]), int(st[0])) == (1, V.OK)
        assert lib.bftkv_gpu_dsa_keyset_info(h, ks, None, None, None, None, None, None, None) == 0       # any output may be NULL
        assert lib.bftkv_gpu_dsa_keyset_info(None, ks, None, None, None, None, None, None, None) == E_INVALID
        assert lib.bftkv_gpu_dsa_keyset_destroy(None, ks) == E_INVALID
        # more operations than a call takes (2^24): refused before anything is read or written
        valid[:], st[:] = 0xAA, 0xAA
        assert call(h, ks, (1 << 24) + 1, P(dg), 20, P(sg), None, P(valid), P(st)) == E_INVALID
        assert (valid == 0xAA).all() and (st == 0xAA).all()
        # the test hook: a NULL context, NULL words
        words = np.zeros(2 * 40 * 15 * 76, dtype=np.uint32)
        table = lib.bftkv_gpu_selftest_dsa_keyset_table
        assert table(None, ks, 0, words.ctypes.data, len(words)) == E_INVALID
        assert table(h, ks, 0, None, len(words)) == E_INVALID
        assert table(h, ks, 0, words.ctypes.data, len(words)) == 0 and words.any()
        # the batcher entry: every NULL argument fails that caller, closed
        from bftkv_amd import Batcher
        b = Batcher(gpu_ctx, max_items=8, n_lanes=1)
        try:
            v1, s1 = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
            bcall = lib.bftkv_gpu_batcher_dsa_verify_keyset
            for a_dg, a_sg, a_v, a_s in ((None, sg, v1, s1), (dg, None, v1, s1), (dg, sg, None, s1), (dg, sg, v1, None)):
                v1[0], s1[0] = 0xAA, 0
                assert bcall(b.h, ks, 0, P(a_dg), 20, P(a_sg), P(a_v), P(a_s)) == E_INVALID
                assert (a_v is None or int(v1[0]) == 0) and (a_s is None or int(s1[0]) == FAILED)
            assert bcall(b.h, ks, 0, P(dg), 65, P(sg), P(v1), P(s1)) == E_INVALID and (int(v1[0]), int(s1[0])) == (0, FAILED)
            assert bcall(b.h, ks, 0, P(dg), 20, P(sg), P(v1), P(s1)) == 0 and (int(v1[0]), int(s1[0])) == (1, V.OK)
        finally:
            b.close()
    finally:
        fork.close()
        gpu_ctx.dsa_keyset_destroy(ks)
